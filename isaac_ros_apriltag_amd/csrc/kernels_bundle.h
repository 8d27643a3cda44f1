// kernels_bundle.h -- S10, the board pose of a tag bundle (amdAprilTagsSetBundles): one joint least-squares homography over the
// corners of all used tags of a frame, and the single-tag pose routine on it.  DESIGN.md section 7d is the definition, statement by
// statement; tests/bundle_ref.py is the same in Python.  FP64 throughout, one IEEE operation per operator (-ffp-contract=off), every
// sum starts from +0.0.
#pragma once
#include "bundle_layout.h"
#include "common.h"
#include "kernels_decode.h"   // pose_from_homography_dev

#define BP_NE 44        // the 36 distinct entries of the symmetric 8 x 8 matrix M (upper triangle, row-major) and the 8 of b
#define BP_STRIDE 45    // doubles per record's partial in LDS: odd, so that the lanes of a wave land on distinct banks

// What record i of the frame's canonical order is to bundle b: 0 none of its members, 1 used, 2 skipped (a gate or the duplicate rule).
// One statement for both kinds of bundle: Head, Member, Gates are bundle_layout.h's structs for k_bundle_pose and rigid_layout.h's
// for k_bundle_rigid, which carry the fields read here under the same names.
template <class Head, class Member, class Gates>
__device__ __forceinline__ int bundle_classify(uint32_t i, uint32_t nout, const DetRec* __restrict__ dets, const uint16_t* __restrict__ order,
                                               const Head* __restrict__ head, const Member* __restrict__ members,
                                               const uint16_t* __restrict__ table, uint32_t b, const Gates& B, uint32_t* member) {
  const DetRec* d = &dets[order[i]];
  const uint32_t fam = (uint32_t)d->family, id = (uint32_t)d->id;
  if (fam >= BUNDLE_MAX_FAMILIES || id >= head->fam_ncodes[fam]) return 0;
  const uint32_t m = table[head->fam_base[fam] + id];
  if (m == 0 || m > head->nmembers || members[m - 1].bundle != b) return 0;
  *member = m - 1;
  // records of one (family, id) are contiguous in the canonical order: a neighbour with the same pair makes this one a duplicate
  bool dup = false;
  if (i > 0) { const DetRec* p = &dets[order[i - 1]]; dup = dup || (p->family == d->family && p->id == d->id); }
  if (i + 1 < nout) { const DetRec* n = &dets[order[i + 1]]; dup = dup || (n->family == d->family && n->id == d->id); }
  const bool gates = d->hamming <= B.max_hamming && d->decision_margin >= B.min_decision_margin;
  return (gates && !BUNDLE_DUPLICATE(dup)) ? 1 : 2;
}

// One 64-lane wave per (frame, bundle); the grid has AMDAT_MAX_BUNDLES bundles per frame and the blocks beyond the layout's return, so
// that a change of the layout changes no launch parameter (a captured graph stays valid).
__global__ __launch_bounds__(64) void k_bundle_pose(const FrameDesc* __restrict__ frames, const DetRec* __restrict__ dets_all,
                                                    const FrameCounters* __restrict__ counters, const uint16_t* __restrict__ order_all,
                                                    const BundleHeadDev* __restrict__ head, const BundleMemberDev* __restrict__ members,
                                                    const uint16_t* __restrict__ table, BundlePoseRec* __restrict__ host_out, DetParams P) {
  const uint32_t b = blockIdx.y;
  const uint32_t nb = head->nbundles;
  if (b >= nb) return;
  const int frame = (int)blockIdx.x + P.frame0;
  const int lane = (int)threadIdx.x;
  const FrameDesc fd = frames[frame];
  const BundleDev B = head->b[b];
  uint32_t nout = counters[frame].nout;
  if (nout > P.dcap) nout = P.dcap;
  const DetRec* dets = dets_all + (size_t)frame * P.dcap;
  const uint16_t* order = order_all + (size_t)frame * P.dcap;

  __shared__ double s_part[64 * BP_STRIDE];   // the partials M_d | b_d of a chunk of 64 records, later their squared errors
  __shared__ double s_A[72];                  // the 8 x 9 system [M | b]
  __shared__ double s_pose[12];               // R, t for the error pass
  __shared__ int s_status;

  // ---- pass 1: classify every kept record; the used ones form their partial sums in parallel, lane e adds entry e in record order ----
  uint32_t ntags = 0, nskipped = 0;
  double acc = 0.0;   // lane e < 44: entry e of M | b
  for (uint32_t base = 0; base < nout; base += 64) {
    const uint32_t i = base + (uint32_t)lane;
    uint32_t mi = 0;
    const int cls = i < nout ? bundle_classify(i, nout, dets, order, head, members, table, b, B, &mi) : 0;
    const unsigned long long used = __ballot(cls == 1);
    ntags += (uint32_t)__popcll(used);
    nskipped += (uint32_t)__popcll(__ballot(cls == 2));
    if (cls == 1) {
      const DetRec* d = &dets[order[i]];
      const BundleMemberDev mem = members[mi];
      double a[BP_NE];
#pragma unroll
      for (int e = 0; e < BP_NE; e++) a[e] = 0.0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const double ckx = (k == 0 || k == 3) ? -1.0 : 1.0, cky = k < 2 ? 1.0 : -1.0;
        const double xb = mem.x + mem.hs * ckx, yb = mem.y + mem.hs * cky;
        const double X = (xb - B.mx) / B.sc, Y = (yb - B.my) / B.sc;
        const double u = d->p[BUNDLE_PIXEL_CORNER(k)][0], v = d->p[BUNDLE_PIXEL_CORNER(k)][1];
        const double vn = (v - fd.cy) / fd.fy;
        const double un = ((u - fd.cx) - fd.skew * vn) / fd.fx;
        const double r0[9] = {X, Y, 1.0, 0.0, 0.0, 0.0, -X * un, -Y * un, un};
        const double r1[9] = {0.0, 0.0, 0.0, X, Y, 1.0, -X * vn, -Y * vn, vn};
#pragma unroll
        for (int row = 0; row < 2; row++) {
          const double* r = row == 0 ? r0 : r1;
          int e = 0;
#pragma unroll
          for (int p = 0; p < 8; p++) {
#pragma unroll
            for (int q = p; q < 8; q++) { a[e] = a[e] + r[p] * r[q]; e++; }
          }
#pragma unroll
          for (int p = 0; p < 8; p++) a[36 + p] = a[36 + p] + r[p] * r[8];
        }
      }
#pragma unroll
      for (int e = 0; e < BP_NE; e++) s_part[lane * BP_STRIDE + e] = a[e];
    }
    __syncthreads();
    if (lane < BP_NE) {
      unsigned long long m = used;
      while (m) {
        const int dd = __ffsll((long long)m) - 1;
        m &= m - 1;
        acc = acc + s_part[dd * BP_STRIDE + lane];
      }
    }
    __syncthreads();
  }

  // ---- the 8 x 9 system, its pivoted elimination in the wave, back-substitution and pose on lane 0 ----
  int status = (int)AMDAT_BUNDLE_SOLVED;
  if (ntags < B.min_tags) status = (int)AMDAT_BUNDLE_TOO_FEW_TAGS;
  if (status == (int)AMDAT_BUNDLE_SOLVED) {
    if (lane < 36) {   // entry e of the upper triangle is (p, q): mirrored into both halves
      int p = 0, e0 = 0;
      while (lane >= e0 + (8 - p)) { e0 += 8 - p; p++; }
      const int q = p + (lane - e0);
      s_A[p * 9 + q] = acc;
      s_A[q * 9 + p] = acc;
    } else if (lane < BP_NE) {
      s_A[(lane - 36) * 9 + 8] = acc;
    }
    __syncthreads();
    for (int col = 0; col < 8; col++) {
      double max_val = 0.0;
      int max_idx = -1;
      for (int row = col; row < 8; row++) {
        const double val = fabs(s_A[row * 9 + col]);
        if (val > max_val) { max_val = val; max_idx = row; }
      }
      if (max_val < 1e-10) { status = (int)AMDAT_BUNDLE_SINGULAR; break; }   // (the same value on every lane)
      if (max_idx != col) {
        double t0 = 0.0, t1 = 0.0;
        if (lane < 9) { t0 = s_A[col * 9 + lane]; t1 = s_A[max_idx * 9 + lane]; }
        __syncthreads();
        if (lane < 9) { s_A[col * 9 + lane] = t1; s_A[max_idx * 9 + lane] = t0; }
        __syncthreads();
      }
      const int ncols = 8 - col, nrows = 7 - col;   // entries (i, j), i = col + 1 .. 7, j = col + 1 .. 8: one per lane
      const bool mine = lane < nrows * ncols;
      const int i = col + 1 + (mine ? lane / ncols : 0), j = col + 1 + (mine ? lane % ncols : 0);
      double nv = 0.0;
      if (mine) {
        const double f = s_A[i * 9 + col] / s_A[col * 9 + col];
        nv = s_A[i * 9 + j] - f * s_A[col * 9 + j];
      }
      __syncthreads();
      if (mine) {
        s_A[i * 9 + j] = nv;
        if (j == col + 1) s_A[i * 9 + col] = 0.0;
      }
      __syncthreads();
    }
  }
  if (lane == 0) {
    double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0};
    if (status == (int)AMDAT_BUNDLE_SOLVED) {
      for (int col = 7; col >= 0; col--) {
        double sum = 0.0;
        for (int i = col + 1; i < 8; i++) sum += s_A[col * 9 + i] * s_A[i * 9 + 8];
        s_A[col * 9 + 8] = (s_A[col * 9 + 8] - sum) / s_A[col * 9 + col];
      }
      double h[9], tc[3];
      for (int i = 0; i < 8; i++) h[i] = s_A[i * 9 + 8];
      h[8] = 1.0;
      pose_from_homography_dev(h, 1.0, 1.0, 0.0, 0.0, 0.0, 2.0 * B.sc, R, tc);
      for (int i = 0; i < 3; i++) t[i] = tc[i] - (R[3 * i] * B.mx + R[3 * i + 1] * B.my);
    }
    for (int i = 0; i < 9; i++) s_pose[i] = R[i];
    for (int i = 0; i < 3; i++) s_pose[9 + i] = t[i];
    s_status = status;
  }
  __syncthreads();
  status = s_status;

  // ---- pass 2: the squared reprojection errors, per record in parallel, added in record order on lane 0 ----
  double sq = 0.0;
  if (status == (int)AMDAT_BUNDLE_SOLVED) {
    double R[9], t[3];
    for (int i = 0; i < 9; i++) R[i] = s_pose[i];
    for (int i = 0; i < 3; i++) t[i] = s_pose[9 + i];
    for (uint32_t base = 0; base < nout; base += 64) {
      const uint32_t i = base + (uint32_t)lane;
      uint32_t mi = 0;
      const int cls = i < nout ? bundle_classify(i, nout, dets, order, head, members, table, b, B, &mi) : 0;
      const unsigned long long used = __ballot(cls == 1);
      if (cls == 1) {
        const DetRec* d = &dets[order[i]];
        const BundleMemberDev mem = members[mi];
        double e[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const double ckx = (k == 0 || k == 3) ? -1.0 : 1.0, cky = k < 2 ? 1.0 : -1.0;
          const double xb = mem.x + mem.hs * ckx, yb = mem.y + mem.hs * cky;
          const double xc = (R[0] * xb + R[1] * yb) + t[0];
          const double yc = (R[3] * xb + R[4] * yb) + t[1];
          const double zc = (R[6] * xb + R[7] * yb) + t[2];
          const double xn = xc / zc, yn = yc / zc;
          const double u = (fd.fx * xn + fd.skew * yn) + fd.cx;
          const double v = fd.fy * yn + fd.cy;
          const double du = u - d->p[BUNDLE_PIXEL_CORNER(k)][0], dv = v - d->p[BUNDLE_PIXEL_CORNER(k)][1];
          e[k] = du * du + dv * dv;
        }
        s_part[lane] = ((e[0] + e[1]) + e[2]) + e[3];
      }
      __syncthreads();
      if (lane == 0) {
        unsigned long long m = used;
        while (m) {
          const int dd = __ffsll((long long)m) - 1;
          m &= m - 1;
          sq = sq + s_part[dd];
        }
      }
      __syncthreads();
    }
  }

  // ---- the record, straight to the pinned host block; the launch's stamp goes last, behind a system-wide fence, as k_reconcile's ----
  if (lane == 0) {
    BundlePoseRec* o = &host_out[(size_t)frame * nb + b];
    o->pose.bundle = b;
    o->pose.status = (uint32_t)status;
    o->pose.ntags = ntags;
    o->pose.nskipped = nskipped;
    for (int i = 0; i < 9; i++) o->pose.R[i] = s_pose[i];
    for (int i = 0; i < 3; i++) o->pose.t[i] = s_pose[9 + i];
    o->pose.sq_err_sum = sq;
    __threadfence_system();
    __hip_atomic_store(&o->seq, fd.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
