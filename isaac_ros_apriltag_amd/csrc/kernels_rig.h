// kernels_rig.h -- S13, the pose of a rigid 3-D tag bundle in the frame of a camera rig (amdAprilTagsSetRig).  The definition is
// rig_pose.h, instantiated as k_bundle_rigid instantiates rigid_pose.h: one observation per lane, the 64
// lanes of a wave being the 64 observation slots, every sum the in-lane (x0 + x1) + (x2 + x3) followed by RgSumWave's six-step
// butterfly.  A workgroup has two waves: wave 0 runs chain 0, wave 1 runs chain 1.  What differs is the gather: a workgroup serves one
// (group, bundle) and walks EVERY frame of the submission whose slot belongs to the group, in ascending batch-slot order, so a lane's
// observation comes with its own frame -- its intrinsics, its skew and its rig camera's extrinsics, all kept by the lane.  No LDS
// access and no barrier inside the iteration; chain 1's result crosses to wave 0 through LDS once, behind one barrier.  FP64
// throughout, one IEEE operation per operator (-ffp-contract=off).
#pragma once
#include "common.h"
#include "kernels_bundle.h"   // bundle_classify
#include "kernels_decode.h"   // pose_from_homography_dev
#include "kernels_rigid.h"    // RgSumWave
#include "rig_pose.h"

// One batch slot of a submission as the kernel reads it: the group it belongs to, its rig camera (AMDAT_RIG_NO_CAMERA: none, the
// slot belongs to no group) and that camera's extrinsics.  The host fills one per slot beside the frame descriptors.
struct RigSlotDev {
  double R[9], t[3];
  uint32_t group, camera;
};
// A rig record in the pinned host block: the public record and the stamp of the launch that wrote it, stored last.
struct RigPoseRec {
  amdAprilTagsRigBundlePose_t pose;
  uint32_t seq;
  uint32_t pad;
};

// grid (frames of the submission, AMDAT_MAX_BUNDLES), 128 threads: one workgroup per (group, bundle), a group index per frame, so
// that neither the layout nor the slot map changes a launch parameter (a captured graph stays valid); a group no slot belongs to
// writes the too-few-tags record.  Reads every frame's records (P.frame0 is not used), so it runs where they are all final.  Every
// lane of both waves stays active from the gather to the barrier, so that the cross-lane moves always read live lanes.
__global__ __launch_bounds__(128) void k_bundle_rig(const FrameDesc* __restrict__ frames, const DetRec* __restrict__ dets_all,
                                                    const FrameCounters* __restrict__ counters, const uint16_t* __restrict__ order_all,
                                                    const RigidHeadDev* __restrict__ head, const RigidMemberDev* __restrict__ members,
                                                    const uint16_t* __restrict__ table, const RigSlotDev* __restrict__ rig,
                                                    RigPoseRec* __restrict__ host_out, DetParams P) {
  const uint32_t b = blockIdx.y;
  const uint32_t nb = head->nbundles;
  if (b >= nb) return;
  const uint32_t g = blockIdx.x, nframes = gridDim.x;
  const int lane = (int)(threadIdx.x & 63u);
  const bool second = threadIdx.x >= 64u;   // wave 1: chain 1
  const RigidBundleDev B = head->b[b];
  const uint32_t seq = frames[g].seq;       // (every frame of the submission carries the launch's number)
  RigPoseRec* o = &host_out[(size_t)g * nb + b];

  __shared__ double s_sq[2][RG_SLOTS];   // the pixel reprojection sums per slot under chain 0's and chain 1's pose
  __shared__ double s_chain1[13];        // R, t, E of chain 1
  __shared__ int s_ok1;

  // ---- the gather: each wave classifies, for itself, every kept record of every frame of the group (k_bundle_rigid's statement per
  // frame) and compacts the used ones into the observation slots in slot-then-record order; the used ones beyond the slots are
  // counted and dropped ----
  uint32_t total = 0, nskipped = 0, ncams = 0;
  uint32_t my_frame = 0, my_rec = 0, my_mem = 0;
  for (uint32_t f = 0; f < nframes; f++) {
    if (rig[f].group != g || rig[f].camera == AMDAT_RIG_NO_CAMERA) continue;   // (the same on every thread of the block)
    uint32_t nout = counters[f].nout;
    if (nout > P.dcap) nout = P.dcap;
    const DetRec* dets = dets_all + (size_t)f * P.dcap;
    const uint16_t* order = order_all + (size_t)f * P.dcap;
    const uint32_t before = total;
    for (uint32_t base = 0; base < nout; base += 64) {
      const uint32_t i = base + (uint32_t)lane;
      uint32_t mi = 0;
      const int cls = i < nout ? bundle_classify(i, nout, dets, order, head, members, table, b, B, &mi) : 0;
      const unsigned long long used = __ballot(cls == 1);
      const uint32_t nu = (uint32_t)__popcll(used);
      nskipped += (uint32_t)__popcll(__ballot(cls == 2));
      const bool mine = (uint32_t)lane >= total && (uint32_t)lane < total + nu && (uint32_t)lane < RIG_SLOT_CUT;
      int src = 0;
      if (mine) {
        unsigned long long m = used;
        for (uint32_t k = (uint32_t)lane - total; k > 0; k--) m &= m - 1;
        src = __ffsll((long long)m) - 1;
      }
      const uint32_t mi_src = (uint32_t)__shfl((int)mi, src);
      if (mine) { my_frame = f; my_rec = base + (uint32_t)src; my_mem = mi_src; }
      total += nu;
    }
    if (total > before && before < RIG_SLOT_CUT) ncams++;   // (a (group, camera) pair names one slot: a frame is a camera)
  }
  const uint32_t nobs = total < RIG_SLOT_CUT ? total : RIG_SLOT_CUT;

  if (nobs < B.min_tags || nobs == 0) {   // (the same on every thread of the block)
    if (threadIdx.x == 0) {
      uint32_t* w = reinterpret_cast<uint32_t*>(&o->pose);
      for (uint32_t k = 0; k < sizeof(o->pose) / 4; k++) w[k] = 0u;
      o->pose.group = g;
      o->pose.bundle = b;
      o->pose.status = AMDAT_BUNDLE_TOO_FEW_TAGS;
      o->pose.nobs = nobs;
      o->pose.nskipped = nskipped;
      o->pose.ndropped = total - nobs;
      o->pose.ncams = ncams;
      __threadfence_system();
      __hip_atomic_store(&o->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }

  // ---- the lane's observation (an unused lane takes slot 0's, which exists, and contributes nothing) ----
  const bool used = (uint32_t)lane < nobs;
  {
    const uint32_t f0 = (uint32_t)__shfl((int)my_frame, 0), r0 = (uint32_t)__shfl((int)my_rec, 0), m0 = (uint32_t)__shfl((int)my_mem, 0);
    if (!used) { my_frame = f0; my_rec = r0; my_mem = m0; }
  }
  const DetRec* d = &dets_all[(size_t)my_frame * P.dcap + order_all[(size_t)my_frame * P.dcap + my_rec]];
  const RigidMemberDev* mem = &members[my_mem];
  const FrameDesc* fdp = &frames[my_frame];
  const RigSlotDev* rsp = &rig[my_frame];
  RigCam cam;
  cam.fx = fdp->fx; cam.fy = fdp->fy; cam.cx = fdp->cx; cam.cy = fdp->cy; cam.skew = fdp->skew;
#pragma unroll
  for (int e = 0; e < 9; e++) cam.R[e] = rsp->R[e];
#pragma unroll
  for (int e = 0; e < 3; e++) cam.t[e] = rsp->t[e];
  double pix[4][2], obj[4][3];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    pix[k][0] = d->p[k][0]; pix[k][1] = d->p[k][1];
    obj[k][0] = mem->P[k][0]; obj[k][1] = mem->P[k][1]; obj[k][2] = mem->P[k][2];
  }

  // ---- the seed: the used slot with the largest pixel area, a tie to the earlier slot; its homography pose under its own frame's
  // camera, composed with its member's inverse and moved into the rig frame ----
  double best = used ? rg_area2(pix) : -1.0;
  int seed = lane;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double oa = __shfl_xor(best, off);
    const int ol = __shfl_xor(seed, off);
    if (oa > best || (oa == best && ol < seed)) { best = oa; seed = ol; }
  }
  const uint32_t seed_frame = (uint32_t)__shfl((int)my_frame, seed);
  const uint32_t seed_rec = (uint32_t)__shfl((int)my_rec, seed);
  const uint32_t seed_mem = (uint32_t)__shfl((int)my_mem, seed);
  const DetRec* ds = &dets_all[(size_t)seed_frame * P.dcap + order_all[(size_t)seed_frame * P.dcap + seed_rec]];
  const RigidMemberDev* ms = &members[seed_mem];
  const FrameDesc* fds = &frames[seed_frame];
  const RigSlotDev* rss = &rig[seed_frame];
  double Rh[9], th[3], Rm[9], tm[3], Rcs[9], tcs[3];
  pose_from_homography_dev(ds->H, fds->fx, fds->fy, fds->cx, fds->cy, fds->skew, ms->size, Rh, th);
#pragma unroll
  for (int e = 0; e < 9; e++) { Rm[e] = ms->R[e]; Rcs[e] = rss->R[e]; }
#pragma unroll
  for (int e = 0; e < 3; e++) { tm[e] = ms->t[e]; tcs[e] = rss->t[e]; }
  double Rb0[9], tb0[3], Rmir[9], Rb1[9], Rs0[9], ts0[3], Rs1[9], Rs[9];
  rg_compose_start(Rh, th, Rm, tm, Rb0, tb0);
  pr_mirror_start(Rh, th, Rmir);
  rg_compose_start(Rmir, (const double*)0, Rm, tm, Rb1, (double*)0);
  rig_from_camera(Rcs, tcs, Rb0, tb0, Rs0, ts0);
  rig_from_camera(Rcs, tcs, Rb1, (const double*)0, Rs1, (double*)0);
#pragma unroll
  for (int e = 0; e < 9; e++) Rs[e] = second ? Rs1[e] : Rs0[e];

  // ---- the chain of this wave ----
  const RgSumWave sum = {used};
  const double npts = 4.0 * (double)nobs;
  uint32_t iterations = B.iterations;
  if (iterations > PR_MAX_ITERATIONS) iterations = PR_MAX_ITERATIONS;
  RigPoints<4> C;
  double Gi[6];
  rig_setup<4>(pix, obj, &cam, npts, sum, &C, Gi);
  const double Es = rig_error<4>(C, Rs0, ts0, sum);
  double R[9], t[3], E;
  const bool ok = rig_chain<4>(C, Gi, Rs, iterations, npts, sum, R, t, &E);

  // ---- the pixel reprojection sum of the lane's observation under this wave's pose; chain 1's result to wave 0 ----
#pragma unroll
  for (int k = 0; k < 4; k++) { pix[k][0] = d->p[k][0]; pix[k][1] = d->p[k][1]; }
  s_sq[second ? 1 : 0][lane] = rig_reprojection(pix, obj, R, t, cam);
  if (second && lane == 0) {
#pragma unroll
    for (int e = 0; e < 9; e++) s_chain1[e] = R[e];
#pragma unroll
    for (int e = 0; e < 3; e++) s_chain1[9 + e] = t[e];
    s_chain1[12] = E;
    s_ok1 = ok ? 1 : 0;
  }
  __syncthreads();

  // ---- the outcome and the record, straight to the pinned host block; the launch's stamp goes last, behind a system-wide fence ----
  if (threadIdx.x == 0) {
    double R1[9], t1[3];
    for (int e = 0; e < 9; e++) R1[e] = s_chain1[e];
    for (int e = 0; e < 3; e++) t1[e] = s_chain1[9 + e];
    double sq0 = 0.0, sq1 = 0.0;
    for (uint32_t s = 0; s < nobs; s++) { sq0 = sq0 + s_sq[0][s]; sq1 = sq1 + s_sq[1][s]; }
    o->pose.group = g;
    o->pose.bundle = b;
    o->pose.nobs = nobs;
    o->pose.nskipped = nskipped;
    o->pose.ndropped = total - nobs;
    o->pose.ncams = ncams;
    o->pose.seed_frame = seed_frame;
    o->pose.seed = seed_rec;
    rig_outcome(ok, R, t, E, sq0, s_ok1 != 0, R1, t1, s_chain1[12], sq1, Rs0, ts0, Es, &o->pose);
    __threadfence_system();
    __hip_atomic_store(&o->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
