// kernels_pose.h -- S11, the orthogonal-iteration tag pose with both minima (amdAprilTagsSetPoseRefinement).  The definition is
// pose_refine.h, instantiated here with one corner per lane: eight lanes per record -- lanes 0 .. 3 run
// chain 0 on corners 0 .. 3, lanes 4 .. 7 run chain 1 -- and every sum over the four corners is the two-step butterfly over the
// lanes of a quad on the DPP network (quad_perm), which leaves (x0 + x1) + (x2 + x3) on all four.  FP64 throughout, one IEEE
// operation per operator (-ffp-contract=off).  No LDS, no barrier, no scratch.
// k_pose_refine<true> (amdAprilTagsSetPoseCovariance, pose_covariance.h) adds, behind the chains, the Jacobian
// pass of each quad at its chain's pose -- 22 more sums on the same butterfly -- and the 6 x 6 inversion; k_pose_refine<false> is
// the kernel without any of it.
#pragma once
#include "common.h"
#include "kernels_decode.h"   // pose_from_homography_dev
#include "pose_covariance.h"
#include "pose_refine.h"

// A refined record in the pinned host block: the public record and the stamp of the launch that wrote it, stored last.
struct PoseRefineRec {
  amdAprilTagsRefinedPose_t pose;
  uint32_t seq;
  uint32_t pad;
};

// A covariance record in a pinned host block of its own, beside the pose record's: the public record and the launch's stamp.
struct PoseCovRec {
  amdAprilTagsPoseCovariance_t c;
  uint32_t seq;
  uint32_t pad;
};

#define PR_LANES_PER_RECORD 8
#define PR_RECORDS_PER_WAVE (64 / PR_LANES_PER_RECORD)

template <int CTRL>
__device__ __forceinline__ double pr_quad_perm(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

// Lane k of a quad holds x_k: (x0 + x1) + (x2 + x3) on every lane (addition commutes, so the four lanes form the same bits).
struct PrSumQuad {
  __device__ __forceinline__ double operator()(const double* x) const {
    const double a = x[0] + pr_quad_perm<0xB1>(x[0]);   // quad_perm [1, 0, 3, 2]: the lane across bit 0
    return a + pr_quad_perm<0x4E>(a);                   // quad_perm [2, 3, 0, 1]: the lane across bit 1
  }
};

// Waves per frame of the launch that hands out `ostride` records per frame (a host-side figure: the grid depends on no device count).
static inline uint32_t pose_refine_waves(uint32_t ostride) {
  const uint32_t w = (ostride + PR_RECORDS_PER_WAVE - 1) / PR_RECORDS_PER_WAVE;   // (ostride <= dcap <= 65 535: at most 8 192)
  return w < 1u ? 1u : w;
}

// grid (frames, pose_refine_waves(host_stride)), one wave per block: wave y of a frame refines records 8 y .. 8 y + 7 of the first
// min(nout, host_stride) -- the records k_reconcile handed out; a wave beyond them returns.  cfg[0]: the iteration count (device
// memory: changing it changes no launch argument).  Every lane of a wave that runs stays active through the iteration (a group
// beyond the last record repeats that record and stores nothing), so that the DPP moves always read live lanes.
// COV: cov_cfg[0] is sigma^2 (device memory, as the count), cov_out the covariance records, laid out as host_out.
// tag_table: the handle's tag table (tag_table.h), nullptr where none is set.
template <bool COV>
__global__ __launch_bounds__(64) void k_pose_refine(const FrameDesc* __restrict__ frames, const DetRec* __restrict__ dets_all,
                                                    const FrameCounters* __restrict__ counters, const uint16_t* __restrict__ order_all,
                                                    const uint32_t* __restrict__ cfg, PoseRefineRec* __restrict__ host_out,
                                                    uint32_t host_stride, DetParams P, const double* __restrict__ cov_cfg,
                                                    PoseCovRec* __restrict__ cov_out, const void* __restrict__ tag_table) {
  const int frame = (int)blockIdx.x + P.frame0;
  uint32_t nout = counters[frame].nout;
  if (nout > P.dcap) nout = P.dcap;
  if (nout > host_stride) nout = host_stride;
  uint32_t iterations = cfg[0];
  if (iterations > PR_MAX_ITERATIONS) iterations = PR_MAX_ITERATIONS;
  const FrameDesc fd = frames[frame];
  const DetRec* dets = dets_all + (size_t)frame * P.dcap;
  const uint16_t* order = order_all + (size_t)frame * P.dcap;
  const int lane = (int)threadIdx.x;
  const int k = lane & 3;
  const bool second = (lane & 4) != 0;
  const PrSumQuad sum;

  const uint32_t base = blockIdx.y * PR_RECORDS_PER_WAVE;
  if (base >= nout) return;   // (the same on every lane)
  const uint32_t i = base + (uint32_t)(lane / PR_LANES_PER_RECORD);
  const bool live = i < nout;
  const DetRec* d = &dets[order[live ? i : nout - 1]];
  // the record's tag size: the homography pose, the model points of the chains and, through them, of the covariance
  const double tag_size = PR_TAG_SIZE(P.tag_size, tt_size_dev(tag_table, (uint32_t)d->family, (uint32_t)d->id, P.tag_size));   // (tools_hooks.h: the table's)
  double Rh[9], th[3];
  pose_from_homography_dev(d->H, fd.fx, fd.fy, fd.cx, fd.cy, fd.skew, tag_size, Rh, th);

  const double pix[1][2] = {{d->p[k][0], d->p[k][1]}};
  PrPoints<1> C;
  double Gi[6];
  pr_setup<1>(pix, k, fd.fx, fd.fy, fd.cx, fd.cy, fd.skew, tag_size / 2.0, 4.0, sum, &C, Gi);
  const double Eh = pr_error<1>(C, Rh, th, sum);
  double Rm[9], Rs[9];
  pr_mirror_start(Rh, th, Rm);
#pragma unroll
  for (int e = 0; e < 9; e++) Rs[e] = second ? POSE_CHAIN1_START(Rm[e], Rh[e]) : Rh[e];
  double R[9], t[3], E;
  const bool ok = pr_chain<1>(C, Gi, Rs, iterations, 4.0, sum, R, t, &E);

  // the record's first lane takes chain 1's result from the lane four up, forms the outcome and stores the record; the stamp goes
  // last, behind a system-wide fence, as k_reconcile's
  const int src = (lane & ~7) | 4;
  double R1[9], t1[3];
#pragma unroll
  for (int e = 0; e < 9; e++) R1[e] = __shfl(R[e], src);
#pragma unroll
  for (int e = 0; e < 3; e++) t1[e] = __shfl(t[e], src);
  const double E1 = __shfl(E, src);
  const bool ok1 = __shfl((int)ok, src) != 0;
  if constexpr (COV) {
    // each quad at the pose the record reports for its chain: chain 0's, or the homography pose where chain 0 was degenerate; chain
    // 1's.  All lanes stay active through the sums and run the inversion; lanes 0 and 4 of a record store.
    const int lane0 = lane & ~7;
    double Re[9], te[3];
#pragma unroll
    for (int e = 0; e < 9; e++) { const double r1 = POSE_COV_CHAIN1_AT(R[e], lane0); Re[e] = second ? r1 : ok ? R[e] : Rh[e]; }
#pragma unroll
    for (int e = 0; e < 3; e++) { const double t1c = POSE_COV_CHAIN1_AT(t[e], lane0); te[e] = second ? t1c : ok ? t[e] : th[e]; }
    const double zero[1] = {0.0};
    double N[21], sq, cov[36];
    pc_normal<1>(C.px, C.py, zero, pix, Re, te, fd.fx, fd.fy, fd.cx, fd.cy, fd.skew, sum, N, &sq);
    const bool inv = pc_invert(N, cov_cfg[0], cov);
    // the outcome rule of pr_outcome on both storing lanes: chain 0's ok and E reach lane 4 by one shuffle each
    const bool ok0 = __shfl((int)ok, lane0) != 0;
    const double E0 = __shfl(E, lane0);
    const bool alt = ok0 && ok1;
    const bool chose1 = alt && E1 < E0;
    const bool to_alt = second != chose1;          // this lane's pose is the record's alternative ...
    const bool have = !to_alt || alt;              // ... which exists only where both chains ran
    const bool good = have && inv;
    PoseCovRec* co = &cov_out[(size_t)frame * host_stride + i];
    if (live && (lane & 3) == 0) {
      double* dst = to_alt ? co->c.cov_alt : co->c.cov;
#pragma unroll
      for (int e = 0; e < 36; e++) dst[e] = good ? cov[e] : 0.0;
      *(to_alt ? &co->c.sq_err_sum_alt : &co->c.sq_err_sum) = have ? sq : 0.0;
    }
    // the valid word is the first lane's: its own bit and lane 4's.  The stores above are earlier instructions of this wave, so the
    // fence below, which waits for the wave's outstanding stores, stands behind both lanes' doubles
    const bool good4 = __shfl((int)good, src) != 0;
    const bool to_alt4 = __shfl((int)to_alt, src) != 0;
    if (live && (lane & 7) == 0) {
      co->c.valid = (good ? (to_alt ? 2u : 1u) : 0u) | (good4 ? (to_alt4 ? 2u : 1u) : 0u);
      co->c.reserved = 0u;
      __threadfence_system();
      __hip_atomic_store(&co->seq, fd.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (live && (lane & 7) == 0) {
    PoseRefineRec* o = &host_out[(size_t)frame * host_stride + i];
    pr_outcome(ok, R, t, E, ok1, R1, t1, E1, Rh, th, Eh, &o->pose);
    __threadfence_system();
    __hip_atomic_store(&o->seq, fd.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
