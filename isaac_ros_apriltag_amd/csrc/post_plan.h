// post_plan.h -- the stages behind k_reconcile: what the setters set (PostMode), which of it a captured graph holds (post_graph_key)
// and what one submission launches there, with which grids, on which records, into which pinned blocks (plan_post).  detector.hip
// executes the plan, and finish_once walks the same plan's block list for the stamps.  Plain C++ without HIP, so that
// tests/test_post_plan_cpu.py compiles it on the host.  (The functions are static: the library exports no symbol from here.)
#pragma once
#include <stdint.h>

#include "../../include/apriltag_amd.h"   // AMDAT_MAX_BUNDLES

// What the six setters set.  The undistortion models and the device-resident layouts, iteration count and sigma^2 stay with the handle.
struct PostMode {
  uint32_t nbundles = 0;          // amdAprilTagsSetBundles: planar bundles, 0: off
  uint32_t nrigid = 0;            // amdAprilTagsSetBundlesEx: rigid bundles, 0: off (one kind is on at a time)
  uint32_t pose_iterations = 0;   // amdAprilTagsSetPoseRefinement, 0: off
  double cov_sigma = 0.0;         // amdAprilTagsSetPoseCovariance: corner sigma in pixels, 0: off
  uint32_t nundist = 0;           // amdAprilTagsSetCornerUndistortion: camera models, 0: off
  uint32_t nrig = 0;              // amdAprilTagsSetRig: rig cameras, 0: off (the stage runs where the rigid kind is on)
};

enum PostSetting { POST_SET_PLANAR, POST_SET_RIGID, POST_SET_REFINE, POST_SET_COV, POST_SET_UNDISTORT, POST_SET_RIG };

// The mode after a setter's request (a count, or the sigma).  Turning one bundle kind on turns the other off; turning it off leaves
// the other alone.
static inline PostMode post_apply(PostMode m, PostSetting what, double value) {
  const uint32_t count = (uint32_t)value;
  switch (what) {
    case POST_SET_PLANAR: m.nbundles = count; if (count) m.nrigid = 0; break;
    case POST_SET_RIGID: m.nrigid = count; if (count) m.nbundles = 0; break;
    case POST_SET_REFINE: m.pose_iterations = count; break;
    case POST_SET_COV: m.cov_sigma = value; break;
    case POST_SET_UNDISTORT: m.nundist = count; break;
    case POST_SET_RIG: m.nrig = count; break;
  }
  return m;
}

// What a captured graph holds of the mode: each stage on or off.  Counts, layouts, the iteration number, sigma and the models live
// in device memory or travel through the descriptors, so a setter retires the graphs if and only if this key changes -- the
// covariance bit included where neither pose launch runs.
enum : uint32_t { POST_UNDISTORT = 1u, POST_PLANAR = 2u, POST_RIGID = 4u, POST_REFINE = 8u, POST_COV = 16u, POST_RIG = 32u };
static inline uint32_t post_graph_key(const PostMode& m) {
  return (m.nundist ? POST_UNDISTORT : 0u) | (m.nbundles ? POST_PLANAR : 0u) | (m.nrigid ? POST_RIGID : 0u) |
         (m.pose_iterations ? POST_REFINE : 0u) | (m.cov_sigma > 0.0 ? POST_COV : 0u) | (m.nrig ? POST_RIG : 0u);
}

// The launches: k_undistort_records, k_bundle_pose, k_bundle_rigid<cov>, k_pose_refine<cov>, k_bundle_rig.
enum PostKernel { POST_K_UNDISTORT, POST_K_PLANAR, POST_K_RIGID, POST_K_REFINE, POST_K_RIG };
// The pinned blocks they write: h_udets, h_bposes, h_xposes, h_xcovs, h_rposes, h_rcovs, h_gposes.
enum PostBlock { POST_B_UDETS, POST_B_BPOSES, POST_B_XPOSES, POST_B_XCOVS, POST_B_RPOSES, POST_B_RCOVS, POST_B_GPOSES };
// How a block is indexed: frame * per_frame + bundle, every entry written (h_gposes: group * per_frame + bundle, a group index per
// frame of the submission, every entry written); or frame * per_frame + record, the first min(nout, per_frame) of a frame written,
// as k_reconcile writes its own.
enum PostIndex { POST_BY_BUNDLE, POST_BY_RECORD };

constexpr uint32_t POST_UD_WAVES = 16;           // kernels_undistort.h: UD_WAVES_PER_FRAME
constexpr uint32_t POST_PR_RECORDS_PER_WAVE = 8;   // kernels_pose.h: PR_RECORDS_PER_WAVE (pose_refine_waves)

struct PostWrite {
  PostBlock block;
  PostIndex index;
  uint32_t per_frame;   // bundles of the mode, or the submission's record stride
};
struct PostStep {
  PostKernel kernel;
  bool cov;             // POST_K_RIGID, POST_K_REFINE: the covariance instance
  bool twins;           // the pose launches: reads the undistorted twins, not the raw records
  uint32_t gx, gy;      // grid, one block per (frame, gy index)
  int nwrites;
  PostWrite writes[2];
};
struct PostPlan {
  int nsteps;
  PostStep steps[5];    // in enqueue order, all on the submission stream
};

// What a submission of n frames with `ostride` record slots per frame launches behind k_reconcile.
static inline PostPlan plan_post(const PostMode& m, uint32_t n, uint32_t ostride) {
  PostPlan p = {};
  const bool cov = m.cov_sigma > 0.0, twins = m.nundist > 0;
  auto step = [&](PostKernel k, bool c, bool t, uint32_t gy) -> PostStep& {
    PostStep& s = p.steps[p.nsteps++];
    s = {k, c, t, n, gy, 0, {}};
    return s;
  };
  auto writes = [](PostStep& s, PostBlock b, PostIndex ix, uint32_t per_frame) { s.writes[s.nwrites++] = {b, ix, per_frame}; };
  if (twins) writes(step(POST_K_UNDISTORT, false, false, POST_UD_WAVES), POST_B_UDETS, POST_BY_RECORD, ostride);
  if (m.nbundles) writes(step(POST_K_PLANAR, false, twins, AMDAT_MAX_BUNDLES), POST_B_BPOSES, POST_BY_BUNDLE, m.nbundles);
  if (m.nrigid) {
    PostStep& s = step(POST_K_RIGID, cov, twins, AMDAT_MAX_BUNDLES);
    writes(s, POST_B_XPOSES, POST_BY_BUNDLE, m.nrigid);
    if (cov) writes(s, POST_B_XCOVS, POST_BY_BUNDLE, m.nrigid);
  }
  if (m.pose_iterations) {
    const uint32_t waves = (ostride + POST_PR_RECORDS_PER_WAVE - 1) / POST_PR_RECORDS_PER_WAVE;
    PostStep& s = step(POST_K_REFINE, cov, twins, waves < 1u ? 1u : waves);
    writes(s, POST_B_RPOSES, POST_BY_RECORD, ostride);
    if (cov) writes(s, POST_B_RCOVS, POST_BY_RECORD, ostride);
  }
  // the camera rig, behind the other pose launches and only beside the rigid kind: one block per (group, bundle) over every frame's
  // records, raw or twins as they read them, never a covariance
  if (m.nrig && m.nrigid) writes(step(POST_K_RIG, false, twins, AMDAT_MAX_BUNDLES), POST_B_GPOSES, POST_BY_BUNDLE, m.nrigid);
  return p;
}
