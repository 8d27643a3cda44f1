// kernels_rigid.h -- S12, the pose of a rigid 3-D tag bundle (amdAprilTagsSetBundlesEx).  The definition is rigid_pose.h (DESIGN.md
// section 7f), instantiated here with one tag per lane: the 64 lanes of a wave are the 64 tag slots, each holds its tag's four
// points, and every sum over the points is the in-lane (x0 + x1) + (x2 + x3) followed by a six-step butterfly over the wave.  A
// workgroup has two waves: wave 0 runs chain 0, wave 1 runs chain 1, concurrently -- each one dependent FP64 chain.  The butterfly
// moves registers only: DPP quad_perm for the lanes across bits 0 and 1, DPP row_half_mirror and row_mirror for the groups of four
// and eight (a mirror pairs the same two groups as the exchange across that bit, and both hold one value by then), ds_swizzle for
// the rows across bit 4 and ds_bpermute for the halves across bit 5 -- the two DS instructions use the LDS crossbar, not its memory.
// No LDS access and no barrier inside the iteration; chain 1's result crosses to wave 0 through LDS once, behind one barrier.  FP64
// throughout, one IEEE operation per operator (-ffp-contract=off).
// k_bundle_rigid<true> (amdAprilTagsSetPoseCovariance, pose_covariance.h) adds, behind each wave's chain, the
// Jacobian pass at that wave's pose -- 22 more sums on the same butterfly -- and the 6 x 6 inversion; the waves then learn each
// other's outcome through LDS behind the same barrier, lane 0 of each stores its 36 doubles, and a second barrier puts the stamp
// behind both.  k_bundle_rigid<false> is the kernel without any of it.
#pragma once
#include "common.h"
#include "kernels_bundle.h"   // bundle_classify
#include "kernels_decode.h"   // pose_from_homography_dev
#include "kernels_pose.h"     // PoseCovRec
#include "pose_covariance.h"
#include "rigid_layout.h"
#include "rigid_pose.h"

template <int CTRL>
__device__ __forceinline__ double rg_dpp(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// the lane across bit 4: ds_swizzle in bit mode, and_mask 0x1F, or_mask 0, xor_mask 0x10
__device__ __forceinline__ double rg_swizzle16(double x) {
  const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(x), 0x401F);
  const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(x), 0x401F);
  return __hiloint2double(hi, lo);
}

// Lane s holds slot s's four values: the slot's (x0 + x1) + (x2 + x3), +0.0 for an unused slot, then the balanced tree over the 64
// slots on every lane (at each step both partners add the same two values, and addition commutes: the same bits everywhere).
struct RgSumWave {
  bool used;
  __device__ __forceinline__ double operator()(const double* x) const {
    double a = used ? (x[0] + x[1]) + (x[2] + x[3]) : 0.0;
    a = a + rg_dpp<0xB1>(a);      // quad_perm [1, 0, 3, 2]
    a = a + rg_dpp<0x4E>(a);      // quad_perm [2, 3, 0, 1]
    a = a + rg_dpp<0x141>(a);     // row_half_mirror: lane i of eight <-> 7 - i
    a = a + rg_dpp<0x140>(a);     // row_mirror: lane i of sixteen <-> 15 - i
    a = a + rg_swizzle16(a);
    return a + __shfl_xor(a, 32);
  }
};

// grid (frames, AMDAT_MAX_BUNDLES), 128 threads: one workgroup per (frame, bundle); the blocks beyond the layout's return, so that a
// change of the layout changes no launch parameter (a captured graph stays valid).  The iteration counts, the gates and the whole
// layout live in device memory.  Every lane of both waves stays active from the classification to the barrier, so that the
// cross-lane moves always read live lanes.
// COV: cov_cfg[0] is sigma^2 (device memory), cov_out the covariance records, laid out as host_out.
template <bool COV>
__global__ __launch_bounds__(128) void k_bundle_rigid(const FrameDesc* __restrict__ frames, const DetRec* __restrict__ dets_all,
                                                      const FrameCounters* __restrict__ counters, const uint16_t* __restrict__ order_all,
                                                      const RigidHeadDev* __restrict__ head, const RigidMemberDev* __restrict__ members,
                                                      const uint16_t* __restrict__ table, RigidPoseRec* __restrict__ host_out, DetParams P,
                                                      const double* __restrict__ cov_cfg, PoseCovRec* __restrict__ cov_out) {
  const uint32_t b = blockIdx.y;
  const uint32_t nb = head->nbundles;
  if (b >= nb) return;
  const int frame = (int)blockIdx.x + P.frame0;
  const int lane = (int)(threadIdx.x & 63u);
  const bool second = threadIdx.x >= 64u;   // wave 1: chain 1
  const FrameDesc fd = frames[frame];
  const RigidBundleDev B = head->b[b];
  uint32_t nout = counters[frame].nout;
  if (nout > P.dcap) nout = P.dcap;
  const DetRec* dets = dets_all + (size_t)frame * P.dcap;
  const uint16_t* order = order_all + (size_t)frame * P.dcap;
  RigidPoseRec* o = &host_out[(size_t)frame * nb + b];

  __shared__ double s_sq[2][RG_SLOTS];   // the pixel reprojection sums per slot under chain 0's and chain 1's pose
  __shared__ double s_chain1[13];        // R, t, E of chain 1
  __shared__ int s_ok1;
  __shared__ double s_E0;                // COV: what wave 1 needs of chain 0, and wave 0 of wave 1's inversion
  __shared__ int s_ok0, s_valid1;

  // ---- classification: each wave classifies every kept record for itself, in chunks of 64 (k_bundle_pose's statement), and compacts
  // the used ones into the tag slots in record order: lane s takes the (s - slots filled so far)-th used record of the chunk ----
  uint32_t ntags = 0, nskipped = 0;
  uint32_t my_rec = 0, my_mem = 0;
  for (uint32_t base = 0; base < nout; base += 64) {
    const uint32_t i = base + (uint32_t)lane;
    uint32_t mi = 0;
    const int cls = i < nout ? bundle_classify(i, nout, dets, order, head, members, table, b, B, &mi) : 0;
    const unsigned long long used = __ballot(cls == 1);
    const uint32_t nu = (uint32_t)__popcll(used);
    nskipped += (uint32_t)__popcll(__ballot(cls == 2));
    const bool mine = (uint32_t)lane >= ntags && (uint32_t)lane < ntags + nu;
    int src = 0;
    if (mine) {
      unsigned long long m = used;
      for (uint32_t k = (uint32_t)lane - ntags; k > 0; k--) m &= m - 1;
      src = __ffsll((long long)m) - 1;
    }
    const uint32_t mi_src = (uint32_t)__shfl((int)mi, src);
    if (mine) { my_rec = base + (uint32_t)src; my_mem = mi_src; }
    ntags += nu;
  }
  if (ntags > RG_SLOTS) ntags = RG_SLOTS;   // (a bundle has at most 64 members and a duplicated member uses none of its records)

  if (ntags < B.min_tags || ntags == 0) {   // (the same on every thread of the block)
    if (threadIdx.x == 0) {
      uint32_t* w = reinterpret_cast<uint32_t*>(&o->pose);
      for (uint32_t k = 0; k < sizeof(o->pose) / 4; k++) w[k] = 0u;
      o->pose.bundle = b;
      o->pose.status = AMDAT_BUNDLE_TOO_FEW_TAGS;
      o->pose.ntags = ntags;
      o->pose.nskipped = nskipped;
      if constexpr (COV) {   // a zeroed covariance record
        PoseCovRec* co = &cov_out[(size_t)frame * nb + b];
        uint32_t* cw = reinterpret_cast<uint32_t*>(&co->c);
        for (uint32_t k = 0; k < sizeof(co->c) / 4; k++) cw[k] = 0u;
        __threadfence_system();
        __hip_atomic_store(&co->seq, fd.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      }
      __threadfence_system();
      __hip_atomic_store(&o->seq, fd.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return;
  }

  // ---- the lane's tag (an unused lane reads record 0 and member 0, which exist, and contributes nothing) ----
  const bool used = (uint32_t)lane < ntags;
  const DetRec* d = &dets[order[my_rec]];
  const RigidMemberDev* mem = &members[my_mem];
  double pix[4][2], obj[4][3];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    pix[k][0] = d->p[k][0]; pix[k][1] = d->p[k][1];
    obj[k][0] = mem->P[k][0]; obj[k][1] = mem->P[k][1]; obj[k][2] = mem->P[k][2];
  }

  // ---- the seed: the used slot with the largest pixel area, a tie to the earlier slot ----
  double best = used ? rg_area2(pix) : -1.0;
  int seed = lane;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double oa = __shfl_xor(best, off);
    const int ol = __shfl_xor(seed, off);
    if (oa > best || (oa == best && ol < seed)) { best = oa; seed = ol; }
  }
  const uint32_t seed_rec = (uint32_t)__shfl((int)my_rec, seed);
  const uint32_t seed_mem = (uint32_t)__shfl((int)my_mem, seed);
  const DetRec* ds = &dets[order[seed_rec]];
  const RigidMemberDev* ms = &members[seed_mem];
  double Rh[9], th[3], Rm[9], tm[3];
  pose_from_homography_dev(ds->H, fd.fx, fd.fy, fd.cx, fd.cy, fd.skew, ms->size, Rh, th);
#pragma unroll
  for (int e = 0; e < 9; e++) Rm[e] = ms->R[e];
#pragma unroll
  for (int e = 0; e < 3; e++) tm[e] = ms->t[e];
  double Rs0[9], ts0[3], Rmir[9], Rs1[9], Rs[9];
  rg_compose_start(Rh, th, Rm, tm, Rs0, ts0);
  pr_mirror_start(Rh, th, Rmir);
  rg_compose_start(Rmir, (const double*)0, Rm, tm, Rs1, (double*)0);
#pragma unroll
  for (int e = 0; e < 9; e++) Rs[e] = second ? Rs1[e] : Rs0[e];

  // ---- the chain of this wave ----
  const RgSumWave sum = {used};
  const double npts = RIGID_NPTS(4.0 * (double)ntags);
  uint32_t iterations = B.iterations;
  if (iterations > PR_MAX_ITERATIONS) iterations = PR_MAX_ITERATIONS;
  RgPoints<4> C;
  double Gi[6];
  rg_setup<4>(pix, obj, fd.fx, fd.fy, fd.cx, fd.cy, fd.skew, npts, sum, &C, Gi);
  const double Es = rg_error<4>(C, Rs0, ts0, sum);
  double R[9], t[3], E;
  const bool ok = rg_chain<4>(C, Gi, Rs, iterations, npts, sum, R, t, &E);

  // ---- the pixel reprojection sum of the lane's tag under this wave's pose; chain 1's result to wave 0 ----
#pragma unroll
  for (int k = 0; k < 4; k++) { pix[k][0] = d->p[k][0]; pix[k][1] = d->p[k][1]; }
  s_sq[second ? 1 : 0][lane] = rg_reprojection(pix, obj, R, t, fd.fx, fd.fy, fd.cx, fd.cy, fd.skew);
  if (second && lane == 0) {
#pragma unroll
    for (int e = 0; e < 9; e++) s_chain1[e] = R[e];
#pragma unroll
    for (int e = 0; e < 3; e++) s_chain1[9 + e] = t[e];
    s_chain1[12] = E;
    s_ok1 = ok ? 1 : 0;
  }
  double cov[36];
  bool inv = false;
  if constexpr (COV) {
    // this wave's pose as the record reports it: its chain's, or -- wave 0 with a degenerate chain -- the seed start, which the
    // record reports where both chains were degenerate.  All lanes stay active through the sums and run the inversion.
    double Re[9], te[3], qx[4], qy[4], qz[4], N[21], sq;
#pragma unroll
    for (int e = 0; e < 9; e++) Re[e] = (second || ok) ? R[e] : Rs0[e];
#pragma unroll
    for (int e = 0; e < 3; e++) te[e] = (second || ok) ? t[e] : ts0[e];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      qx[k] = RIGID_COV_POINT(C.px[k], C.cx[k]); qy[k] = RIGID_COV_POINT(C.py[k], C.cy[k]); qz[k] = RIGID_COV_POINT(C.pz[k], C.cz[k]);
    }
    pc_normal<4>(qx, qy, qz, pix, Re, te, fd.fx, fd.fy, fd.cx, fd.cy, fd.skew, sum, N, &sq);
    inv = pc_invert(N, cov_cfg[0], cov);
    if (!second && lane == 0) { s_ok0 = ok ? 1 : 0; s_E0 = E; }
  }
  __syncthreads();
  if constexpr (COV) {
    // the outcome rule of rg_outcome on lane 0 of both waves; each stores its own 36 doubles into the half its pose went to
    PoseCovRec* co = &cov_out[(size_t)frame * nb + b];
    const bool ok0 = s_ok0 != 0, ok1 = s_ok1 != 0;
    const bool alt = ok0 && ok1;
    const bool chose1 = ok1 && (!ok0 || s_chain1[12] < s_E0);
    const bool to_alt = second != chose1;           // this wave's pose is the record's alternative (wave 0's seed start never is) ...
    const bool have = !to_alt || alt;               // ... which exists only where both chains ran
    const bool good = have && inv;
    if (lane == 0) {
      double* dst = to_alt ? co->c.cov_alt : co->c.cov;
#pragma unroll
      for (int e = 0; e < 36; e++) dst[e] = good ? cov[e] : 0.0;
      if (second) {
        s_valid1 = good ? (to_alt ? 2 : 1) : 0;
        __threadfence_system();   // wave 1's doubles are out before the barrier that the stamp stands behind
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      co->c.sq_err_sum = 0.0; co->c.sq_err_sum_alt = 0.0;
      co->c.valid = (good ? (to_alt ? 2u : 1u) : 0u) | (uint32_t)s_valid1;
      co->c.reserved = 0u;
      __threadfence_system();
      __hip_atomic_store(&co->seq, fd.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }

  // ---- the outcome and the record, straight to the pinned host block; the launch's stamp goes last, behind a system-wide fence ----
  if (threadIdx.x == 0) {
    double R1[9], t1[3];
    for (int e = 0; e < 9; e++) R1[e] = s_chain1[e];
    for (int e = 0; e < 3; e++) t1[e] = s_chain1[9 + e];
    double sq0 = 0.0, sq1 = 0.0;
    for (uint32_t s = 0; s < ntags; s++) { sq0 = sq0 + s_sq[0][s]; sq1 = sq1 + s_sq[1][s]; }
    o->pose.bundle = b;
    o->pose.ntags = ntags;
    o->pose.nskipped = nskipped;
    o->pose.seed = seed_rec;
    rg_outcome(ok, R, t, E, sq0, s_ok1 != 0, R1, t1, s_chain1[12], sq1, Rs0, ts0, Es, &o->pose);
    __threadfence_system();
    __hip_atomic_store(&o->seq, fd.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
