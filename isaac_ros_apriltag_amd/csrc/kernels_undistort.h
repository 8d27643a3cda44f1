// kernels_undistort.h -- S9b, the corner undistortion of raw-frame mode (amdAprilTagsSetCornerUndistortion):
// every kept record of every frame gets a twin whose corners are undistort(p[k]) (undistort.h), whose H is the exact four-point
// homography onto them, and whose centre and pose follow from that H.  One launch per submission, behind k_reconcile and ahead of
// the bundle, rigid and refinement launches, which then read the twins (d_dets_u) in the raw records' place.
// Eight lanes per record: lane j runs the Newton iteration of corner j / 2 and then holds row j of the 8 x 9 system -- rows 2k and
// 2k + 1 are corner k's -- so the pivoted elimination is a row per lane, the pivot row and the row exchange one shuffle inside the
// group of eight per entry.  FP64 throughout, one IEEE operation per operator (-ffp-contract=off).  No LDS, no barrier, no scratch:
// every array below is indexed by unrolled constants.
#pragma once
#include "common.h"
#include "kernels_decode.h"   // homography_project_dev, pose_from_homography_dev
#include "undistort.h"

// An undistorted record in the pinned host block: the public record and the stamp of the launch that wrote it, stored last.
struct UndistortRec {
  amdAprilTagsUndistortedDetection_t det;
  uint32_t seq;
  uint32_t pad;
};

#define UD_LANES_PER_RECORD 8
#define UD_RECORDS_PER_WAVE (64 / UD_LANES_PER_RECORD)
#define UD_WAVES_PER_FRAME 16   // the grid's second extent: wave y takes records 8 y .. 8 y + 7, then 128 further on, up to the kept count

__device__ __forceinline__ double ud_group_read(double x, int sub) { return __shfl(x, sub, UD_LANES_PER_RECORD); }

// grid (frames, UD_WAVES_PER_FRAME), one wave per block.  Every lane of a wave that enters a round stays active through it (a group
// beyond the last record repeats that record and stores nothing), so that the shuffles always read live lanes.  cams: one camera per
// batch slot, uploaded with the submission's descriptors.  dets_u_all is laid out and indexed as dets_all (order_all serves both);
// host_out holds host_stride records per frame in the order they are handed out.  tag_table: as k_reconcile's; the twin's pose takes
// the size of the record's tag.
__global__ __launch_bounds__(64) void k_undistort_records(const FrameDesc* __restrict__ frames, const DetRec* __restrict__ dets_all,
                                                          const FrameCounters* __restrict__ counters, const uint16_t* __restrict__ order_all,
                                                          const UndistortCam* __restrict__ cams, DetRec* __restrict__ dets_u_all,
                                                          UndistortRec* __restrict__ host_out, uint32_t host_stride, DetParams P,
                                                          const void* __restrict__ tag_table) {
  const int frame = (int)blockIdx.x + P.frame0;
  uint32_t nk = counters[frame].nout;
  if (nk > P.dcap) nk = P.dcap;
  const FrameDesc fd = frames[frame];
  const UndistortCam C = cams[frame];
  const DetRec* dets = dets_all + (size_t)frame * P.dcap;
  DetRec* dets_u = dets_u_all + (size_t)frame * P.dcap;
  const uint16_t* order = order_all + (size_t)frame * P.dcap;
  const int lane = (int)threadIdx.x;
  const int sub = lane & (UD_LANES_PER_RECORD - 1);
  const int k = sub >> 1;

  for (uint32_t base = blockIdx.y * UD_RECORDS_PER_WAVE; base < nk; base += UD_WAVES_PER_FRAME * UD_RECORDS_PER_WAVE) {   // (uniform)
    const uint32_t i = base + (uint32_t)(lane / UD_LANES_PER_RECORD);
    const bool live = i < nk;
    const uint32_t slot = order[live ? i : nk - 1];
    const DetRec* d = &dets[slot];

    // ---- the corner ------------------------------------------------------------------------------------------------------------
    double pu, pv;
    const bool corner_ok = ud_undistort(C, d->p[k][0], d->p[k][1], pu, pv);
    const unsigned long long oks = __ballot(corner_ok);
    bool ok = ((oks >> (lane & ~(UD_LANES_PER_RECORD - 1))) & 0xFFull) == 0xFFull;

    // ---- H_u: row `sub` of the system of kernels_decode_wave.h, with c_k for the tag's corner -------------------------------------
    const double x = (k == 0 || k == 3) ? -1.0 : 1.0, y = k < 2 ? 1.0 : -1.0;
    double r[9];
    if ((sub & 1) == 0) { r[0] = x; r[1] = y; r[2] = 1.0; r[3] = 0.0; r[4] = 0.0; r[5] = 0.0; r[6] = -x * pu; r[7] = -y * pu; r[8] = pu; }
    else { r[0] = 0.0; r[1] = 0.0; r[2] = 0.0; r[3] = x; r[4] = y; r[5] = 1.0; r[6] = -x * pv; r[7] = -y * pv; r[8] = pv; }
    bool singular = false;
#pragma unroll
    for (int col = 0; col < 8; col++) {
      // the first row at or below `col` with the largest |entry| (a later row must be strictly larger)
      const double val = fabs(r[col]);
      double max_val = 0.0;
      int max_idx = col;
#pragma unroll
      for (int row = col; row < 8; row++) {
        const double v = ud_group_read(val, row);
        if (v > max_val) { max_val = v; max_idx = row; }
      }
      singular = singular || max_val < 1e-10;
      // rows col and max_idx change places (entries left of `col` are zero in both or never read again)
      const int from = sub == col ? max_idx : sub == max_idx ? col : sub;
#pragma unroll
      for (int j = col; j < 9; j++) r[j] = ud_group_read(r[j], from);
      const double pivot = ud_group_read(r[col], col);
      const double f = r[col] / pivot;
#pragma unroll
      for (int j = col + 1; j < 9; j++) {
        const double pj = ud_group_read(r[j], col);
        const double nv = r[j] - f * pj;
        if (sub > col) r[j] = nv;
      }
    }
    double H[9];
#pragma unroll
    for (int col = 7; col >= 0; col--) {
      double sum = 0.0;
#pragma unroll
      for (int j = col + 1; j < 8; j++) sum += r[j] * H[j];
      H[col] = ud_group_read((r[8] - sum) / r[col], col);
    }
    H[8] = 1.0;
    ok = ok && !singular;

    // ---- centre, corners, pose: every lane forms them, two lanes store -----------------------------------------------------------------
    double c[2], p[4][2], R[9], t[3];
    homography_project_dev(H, 0.0, 0.0, &c[0], &c[1]);
#pragma unroll
    for (int q = 0; q < 4; q++) { p[q][0] = ud_group_read(pu, 2 * q); p[q][1] = ud_group_read(pv, 2 * q); }
    pose_from_homography_dev(H, fd.fx, fd.fy, fd.cx, fd.cy, fd.skew, tt_size_dev(tag_table, (uint32_t)d->family, (uint32_t)d->id, P.tag_size), R, t);
    bool fin = ud_finite(c[0]) && ud_finite(c[1]);
#pragma unroll
    for (int e = 0; e < 9; e++) fin = fin && ud_finite(H[e]) && ud_finite(R[e]);
#pragma unroll
    for (int e = 0; e < 3; e++) fin = fin && ud_finite(t[e]);
    ok = ok && fin;

    if (live && sub == 0) {   // the twin in device memory: what the pose launches read
      DetRec* o = &dets_u[slot];
      o->family = d->family; o->id = d->id; o->hamming = ok ? d->hamming : 0x7FFFFFFF; o->decision_margin = d->decision_margin;
#pragma unroll
      for (int e = 0; e < 9; e++) { o->H[e] = ok ? H[e] : 0.0; o->R[e] = ok ? R[e] : 0.0; }
#pragma unroll
      for (int e = 0; e < 2; e++) o->c[e] = ok ? c[e] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; q++) { o->p[q][0] = ok ? p[q][0] : 0.0; o->p[q][1] = ok ? p[q][1] : 0.0; }
#pragma unroll
      for (int e = 0; e < 3; e++) o->t[e] = ok ? t[e] : 0.0;
    }
    if (live && sub == 4 && i < host_stride) {   // the public record; the stamp goes last, behind a system-wide fence, as k_reconcile's
      UndistortRec* o = &host_out[(size_t)frame * host_stride + i];
      o->det.status = ok ? AMDAT_UNDISTORT_OK : AMDAT_UNDISTORT_INVALID;
      o->det.reserved = 0u;
#pragma unroll
      for (int e = 0; e < 9; e++) { o->det.H[e] = ok ? H[e] : 0.0; o->det.R[e] = ok ? R[e] : 0.0; }
#pragma unroll
      for (int e = 0; e < 2; e++) o->det.c[e] = ok ? c[e] : 0.0;
#pragma unroll
      for (int q = 0; q < 4; q++) { o->det.p[q][0] = ok ? p[q][0] : 0.0; o->det.p[q][1] = ok ? p[q][1] : 0.0; }
#pragma unroll
      for (int e = 0; e < 3; e++) o->det.t[e] = ok ? t[e] : 0.0;
      __threadfence_system();
      __hip_atomic_store(&o->seq, fd.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
