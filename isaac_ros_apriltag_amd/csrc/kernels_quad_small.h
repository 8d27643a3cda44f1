// kernels_quad_small.h -- S5 quad fitting for the SMALL clusters (at most 64 K boundary points, K = 2 or 4), the bulk of a
// noisy frame's clusters (inside cuAprilTagsDetect, reference src/apriltag_node.cpp:491-493).
// The statements of fit_statements.h and so the same results, bit for bit, as k_fit_quads (kernels_quad.h); what differs is where
// the data lives:
//   * a lane loads its K points ONCE and keeps them in registers through bounding box, border direction and slope keys;
//   * the keys never touch LDS: the bitonic network runs on the registers (partner keys over ds_bpermute), and after it
//     lane l holds the sorted positions l K .. l K + K - 1 -- exactly the lane-contiguous runs the moment sweep walks;
//   * the duplicate test takes the previous key from the neighbour lane over DPP, the sweep's per-point state (position,
//     squared gradient, kept flag) stays in registers between its two walks;
//   * the cumulative moments (48 bytes per kept point) live in LDS, not in a global scratch slot: the windowed errors, the
//     rows of the pair fits and the fits themselves never leave the CU (k_fit_quads sends them to HBM and back);
//   * box and border direction are reduced in 32-bit integers (gradient signs, scaled by 255 once);
//   * the pair tables keep (error, mse) for all 90 segments but line parameters only for the 45 forward ones: the
//     wrap-around segment's line is needed for the one chosen corner set only, and k_quad_finish computes it from the
//     six moments the candidate record carries; the corner search tests the four mse bits of a choice before it touches
//     normals or errors, with the pair indices of the 210 choices from a compile-time table.
// One wave per cluster, no workgroup barriers that synchronise anything (a one-wave workgroup's barrier is only a
// compiler fence).
// K = 2 (clusters up to 128 points) is the instance the library launches.  K = 4 (129 .. 256 points, its moments in a global
// scratch slot) measured no gain over k_fit_quads<64> for its sizes: class 1 of the class table
// (launch_plan.h) is empty.
#pragma once
#include "kernels_quad.h"

__device__ __forceinline__ int wave_sum_i(int v) {
#define OP(C, M) v += __builtin_amdgcn_update_dpp(0, v, C, M, 0xF, true);
  AT_DPP_STEPS(OP)
#undef OP
  return __builtin_amdgcn_readlane(v, 63);
}

#define FS_WPE 4   // waves per SIMD the register allocation must allow
#define FS_TAB_BYTES (FQT_DOUBLES * 8)   // pair tables + staged moment rows
// LDS of a workgroup: moments [64 K][6] | errors [64 K], the tables over the moments once they are dead
#define FS_LDS_BYTES(K) ((64 * (K) * 56) > FS_TAB_BYTES ? (64 * (K) * 56) : FS_TAB_BYTES)

template <int K>
__global__ __launch_bounds__(64, FS_WPE) void k_fit_small(const FrameDesc* __restrict__ frames, const uint8_t* __restrict__ gray_all,
                                                          const uint32_t* __restrict__ pts_all, const ClusterRec* __restrict__ clusters_all,
                                                          const uint32_t* __restrict__ work, const uint32_t* __restrict__ work_n, uint32_t work_cap,
                                                          uint32_t* __restrict__ work_cursor, FitCand* __restrict__ cands_all,
                                                          FrameCounters* __restrict__ counters, int pop, DetParams P) {
  constexpr int CAP = 64 * K;
  extern __shared__ __attribute__((aligned(16))) unsigned char fs_smem[];
  // [CAP][6] cumulative moments of the kept points
  double* const lds = reinterpret_cast<double*>(fs_smem);
  double* const rows = lds;
  // [CAP] windowed errors, then the smoothed ones, then the maxima list
  double* const errs = lds + CAP * 6;
  // the pair tables and the staged rows (FQT_* layout, kernels_quad.h): in the moments' place once the maxima are selected
  double* const s_tab = lds;
  double* const s_rows = s_tab + FQT_ROWS;
  static_assert(FQT_DOUBLES * 8 <= 64 * K * 56, "tables fit the moment region");
  __shared__ uint32_t s_cpairs[210];
  __shared__ int s_maxidx[16];

  const int lane = (int)threadIdx.x;
  const uint32_t nwork = min(*work_n, work_cap);
  for (int t = lane; t < 210; t += 64) s_cpairs[t] = g_combo_pairs.v[t];

  // Software pipeline over the work list: while cluster c is being fitted, the loads of cluster c + 1 are in flight -- its
  // work item (stage 1, issued before c's box reductions), its cluster record and frame (stage 2, before c's sort) and its
  // points (stage 3, before c's error pass).  A cluster used to start with four dependent global round trips (list cursor /
  // item / record / points) in front of its first instruction, a fifth of its time when the kernel runs alone.
  typedef const __attribute__((address_space(1))) uint32_t* gptr32;
  uint32_t next_item = blockIdx.x, chunk_left = 1;   // uniform; the first item is the workgroup's own index (no atomic), the cursor
                                                      // hands out the items from gridDim.x on (see k_fit_quads)
  auto next_index = [&]() -> uint32_t {
    if (chunk_left == 0) {
      uint32_t got = 0;
      if (lane == 0) got = gridDim.x + atomicAdd(work_cursor, (uint32_t)pop);
      next_item = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
      chunk_left = (uint32_t)pop;
    }
    chunk_left--;
    return next_item++;
  };
  struct Pending {      // cluster whose loads are in flight
    uint32_t item;      // uniform; >= nwork: none
    uint32_t wi_v;      // stage 1: work item (the same word in every lane)
    uint32_t rec_v[4];  // stage 2: cluster record {key lo, key hi, start, count}
    uint32_t img_v[4];  //          frame: image pointer lo / hi, pitch, working extents (W | H << 16)
    uint32_t pp[K];     // stage 3: the lane's points
  };
  auto stage1 = [&](Pending& n) {
    n.item = next_index();
    n.wi_v = 0;
    if (n.item < nwork) n.wi_v = ((gptr32)work)[n.item];
  };
  auto stage2 = [&](Pending& n) {
    if (n.item >= nwork) return;
    const uint32_t wi = (uint32_t)__builtin_amdgcn_readfirstlane((int)n.wi_v);
    const int frame = (int)(wi >> P.wshift);
    const gptr32 rec = (gptr32)(clusters_all + (size_t)frame * P.ccap + (wi & ((1u << P.wshift) - 1u)));
    const gptr32 fdp = (gptr32)(frames + frame);
#pragma unroll
    for (int j = 0; j < 4; j++) n.rec_v[j] = rec[j];
    n.img_v[0] = fdp[0]; n.img_v[1] = fdp[1]; n.img_v[2] = fdp[2]; n.img_v[3] = fdp[3];   // FrameDesc: img (8 bytes), pitch, wh
  };
  auto stage3 = [&](Pending& n) {
    if (n.item >= nwork) return;
    const uint32_t wi = (uint32_t)__builtin_amdgcn_readfirstlane((int)n.wi_v);
    const int frame = (int)(wi >> P.wshift);
    const uint32_t start = (uint32_t)__builtin_amdgcn_readfirstlane((int)n.rec_v[2]);
    const int sz = __builtin_amdgcn_readfirstlane((int)n.rec_v[3]);
    const gptr32 pts = (gptr32)(pts_all + (size_t)frame * P.pcap + start);
#pragma unroll
    for (int j = 0; j < K; j++) n.pp[j] = pts[min(lane + 64 * j, max(sz, 1) - 1)];
  };
  static_assert(offsetof(FrameDesc, img) == 0 && offsetof(FrameDesc, pitch) == 8 && offsetof(FrameDesc, wh) == 12 && sizeof(ClusterRec) == 16, "stage 2 reads raw words");
  Pending cur, nxt;
  stage1(cur); stage2(cur); stage3(cur);
  while (cur.item < nwork) {
    __syncthreads();   // (compiler fence: the previous cluster's LDS reads are done)
    int pf = 0;        // prefetch stages of the next cluster issued so far
    do {
    const uint32_t wi = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur.wi_v);
    const int frame = (int)(wi >> P.wshift);
    const uint8_t* gray = (P.decimate > 1) ? gray_all + (size_t)frame * P.H * P.WS
                                           : reinterpret_cast<const uint8_t*>(((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)cur.img_v[1]) << 32) |
                                                                              (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)cur.img_v[0]));
    const int gpitch = (P.decimate > 1) ? P.WS : __builtin_amdgcn_readfirstlane((int)cur.img_v[2]);
    const fit_gray_ptr ggray = (fit_gray_ptr)gray;
    const int wh = __builtin_amdgcn_readfirstlane((int)cur.img_v[3]);
    const int W = wh & 0xFFFF, H = (int)((uint32_t)wh >> 16);   // the frame's working extents: the image bounds of the fit
    const unsigned long long cl_key = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)cur.rec_v[1]) << 32) |
                                      (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)cur.rec_v[0]);
    const int sz = __builtin_amdgcn_readfirstlane((int)cur.rec_v[3]);
    stage1(nxt); pf = 1;
    if (sz < 24 || sz > CAP) break;   // (the work list only holds clusters of this class)

    AT_MARK("box")
    // ---- the lane's K points, bounding box and exact gradient dot -------------------------------------------------
    uint32_t pp[K];
#pragma unroll
    for (int j = 0; j < K; j++) pp[j] = cur.pp[j];
    FitBox box;
    int sxg = 0, sg = 0;   // sums of x sgn(gx) + y sgn(gy) and of the packed signs (sgn(gx) << 16) + sgn(gy): |sums| < 2^24, 2^9
#pragma unroll
    for (int j = 0; j < K; j++) {
      // a lane without a point in this slot repeats a point of the cluster with a zero gradient (neither box nor sums change)
      const uint32_t p = (lane + 64 * j < sz) ? pp[j] : fit_pad_point(pp[0]);
      const int x = fit_point_x(p), y = fit_point_y(p);
      const int gx = fit_point_sgx(p), gy = fit_point_sgy(p);
      box.xmin = min(box.xmin, x); box.xmax = max(box.xmax, x); box.ymin = min(box.ymin, y); box.ymax = max(box.ymax, y);
      sxg += __mul24(x, gx) + __mul24(y, gy);
      sg += gx * 65536 + gy;
    }
    box.xmin = wave_min_i(box.xmin); box.xmax = wave_max_i(box.xmax); box.ymin = wave_min_i(box.ymin); box.ymax = wave_max_i(box.ymax);
    sxg = wave_sum_i(sxg); sg = wave_sum_i(sg);
    if (fit_box_too_small(box, P)) break;
    const int sgy_s = (int)(short)(sg & 0xFFFF), sgx_s = (sg - sgy_s) >> 16;
    // (the gradients are +-255: the integer sums of k_fit_quads are 255 times these, exactly)
    const FitCentre ctr = fit_centre(box);
    const int q_reversed = fit_border_reversed(ctr, (double)(255LL * sxg), (double)(255 * sgx_s), (double)(255 * sgy_s));
    if (fit_border_unwanted(q_reversed, P)) break;

    stage2(nxt); pf = 2;
    AT_MARK("keys")
    // ---- slope keys and the sort, in registers -----------------------------------------------------------------------
    const float cx = (float)ctr.x, cy = (float)ctr.y;
    unsigned long long v[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
      const unsigned long long key = fit_sort_key(fit_slope(pp[j], cx, cy), pp[j]);
      v[j] = (lane + 64 * j < sz) ? key : AT_KEY_PAD;
    }
    AT_MARK("sort")
    fq_wave_sort_regs<K>(v);

    AT_MARK("walk1")
    // ---- moment sweep: walk 1 (terms of the lane's kept points), one scan, walk 2 (rounded prefixes to LDS) ------------
    // lane l owns the sorted positions l K + j; the key before its first one comes from lane l - 1 (wave_shr:1)
    unsigned long long prev;
    {
      const unsigned long long last = v[K - 1];
      const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)last, 0x138, 0xF, 0xF, false);
      const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(last >> 32), 0x138, 0xF, 0xF, false);
      prev = key_dec(((unsigned long long)hi << 32) | lo);
    }
    uint32_t st_xy[K], st_g[K];   // per point: kept flag << 31 | py << 14 | px; squared gradient magnitude
    D2 acc[6];
#pragma unroll
    for (int j = 0; j < 6; j++) { acc[j].hi = 0; acc[j].lo = 0; }
    int kept = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const int i = lane * K + j;
      const unsigned long long key = key_dec(v[j]);
      const bool keep = (i < sz) && ((i == 0) || fit_key_moved(key, prev));
      prev = key;
      const uint32_t px = fit_key_px(key), py = fit_key_py(key);
      uint32_t G = 0;
      if (keep) {
        G = fit_grad2(ggray, gpitch, px, py, W, H);
        fit_terms_add(acc, G, px, py);
        kept++;
      }
      st_xy[j] = ((keep ? 1u : 0u) << 31) | (py << 14) | px;
      st_g[j] = G;
    }
    AT_MARK("scan")
    D2 off[6];
    fit_scan_totals(acc, off);
#pragma unroll
    for (int j = 0; j < 6; j++) { off[j].hi -= acc[j].hi; off[j].lo -= acc[j].lo; }   // exclusive
    int kincl = kept;
#define OP(C, M) kincl += __builtin_amdgcn_update_dpp(0, kincl, C, M, 0xF, true);
    AT_DPP_STEPS(OP)
#undef OP
    AT_MARK("walk2")
    int pos = kincl - kept;
    const int szd = __builtin_amdgcn_readlane(kincl, 63);
    if (szd < 24) break;
#pragma unroll
    for (int j = 0; j < K; j++) {
      if (st_xy[j] >> 31) {
        fit_terms_add(off, st_g[j], st_xy[j] & 0x3FFFu, (st_xy[j] >> 14) & 0x3FFFu);
        double r[6];
#pragma unroll
        for (int m = 0; m < 6; m++) r[m] = off[m].hi + off[m].lo;
        double2* const o = reinterpret_cast<double2*>(rows + pos * 6);
        o[0] = make_double2(r[0], r[1]); o[1] = make_double2(r[2], r[3]); o[2] = make_double2(r[4], r[5]);
        pos++;
      }
    }
    __syncthreads();   // (fence: the rows are read by other lanes below)

    stage3(nxt); pf = 3;
    AT_MARK("errors")
    // ---- windowed line-fit error, smoothing, local maxima ------------------------------------------------------------
    const int ksz = min(20, szd / 12);
    double sm[K];
#pragma unroll
    for (int it = 0; it < K; it++) {
      const int i = lane + it * 64;
      if (i < szd) {
        double e;
        fit_line_dev(rows, szd, fit_window_i0(i, ksz, szd), fit_window_i1(i, ksz, szd), nullptr, &e, nullptr);
        errs[i] = e;
      }
    }
    __syncthreads();
    AT_MARK("smooth")
#pragma unroll
    for (int it = 0; it < K; it++) {
      const int i = lane + it * 64;
      sm[it] = 0;
      if (i < szd)
        sm[it] = fit_smooth7(errs[fit_wrap(i - 3, szd)], errs[fit_wrap(i - 2, szd)], errs[fit_wrap(i - 1, szd)], errs[i],
                             errs[fit_wrap(i + 1, szd)], errs[fit_wrap(i + 2, szd)], errs[fit_wrap(i + 3, szd)]);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < K; it++) {
      const int i = lane + it * 64;
      if (i < szd) errs[i] = sm[it];
    }
    __syncthreads();
    uint32_t mx = 0;
#pragma unroll
    for (int it = 0; it < K; it++) {
      const int i = lane + it * 64;
      if (i < szd && fit_is_max(sm[it], errs[fit_next(i, szd)], errs[fit_prev(i, szd)])) mx |= 1u << it;
    }
    __syncthreads();
    // the maxima, in ascending index order: values in errs[0 ..), indices behind them
    double* const cand_val = errs;
    int* const cand_idx = reinterpret_cast<int*>(errs + CAP / 2);   // (maxima are never neighbours: at most CAP / 2 of them)
    int nmaxima = 0;
#pragma unroll
    for (int it = 0; it < K; it++) {
      const bool is_max = (mx >> it) & 1u;
      const unsigned long long mm = __ballot(is_max);
      if (is_max) {
        const int k = nmaxima + (int)__popcll(mm & ((1ull << lane) - 1ull));
        cand_val[k] = sm[it];
        cand_idx[k] = lane + it * 64;
      }
      nmaxima += (int)__popcll(mm);
    }
    __syncthreads();
    if (nmaxima < 4) break;

    AT_MARK("top10")
    // ---- at most max_nmaxima corners: those whose value exceeds the (max_nmaxima + 1)-th largest --------------------------
    int m;
    if (nmaxima > P.max_nmaxima) {
      // KR candidates per lane as order-preserving keys (0 = none); rank of a key = keys above it (value descending,
      // position ascending among equals); the key of rank max_nmaxima is the threshold (FIT_CUT_RANK: tools_hooks.h, max_nmaxima)
      constexpr int KR = K <= 2 ? 1 : 2;
      unsigned long long myk[KR];
#pragma unroll
      for (int r = 0; r < KR; r++) {
        const int k = lane + 64 * r;
        myk[r] = (k < nmaxima) ? double_sortable(cand_val[k] + 0.0) : 0ull;
      }
      int rank[KR];
#pragma unroll
      for (int r = 0; r < KR; r++) rank[r] = 0;
#pragma unroll
      for (int r2 = 0; r2 < KR; r2++) {
        const int n2 = min(64, nmaxima - 64 * r2);
        for (int l = 0; l < n2; l++) {
          const unsigned long long ok = readlane_u64(myk[r2], l);
#pragma unroll
          for (int r = 0; r < KR; r++) rank[r] += (ok > myk[r] || (ok == myk[r] && (r2 < r || (r2 == r && l < lane)))) ? 1 : 0;
        }
      }
      // the threshold key: the one of rank max_nmaxima (exactly one candidate has it)
      unsigned long long tk = 0;
#pragma unroll
      for (int r = 0; r < KR; r++) {
        const unsigned long long tmask = __ballot(myk[r] != 0ull && rank[r] == FIT_CUT_RANK(0, P.max_nmaxima));
        if (tmask) {
          const int tl = (int)__ffsll((long long)tmask) - 1;
          tk = readlane_u64(myk[r], tl);
        }
      }
      m = 0;
#pragma unroll
      for (int r = 0; r < KR; r++) {
        const bool keepc = myk[r] != 0ull && rank[r] < FIT_CUT_RANK(0, P.max_nmaxima) && myk[r] > tk;
        const unsigned long long kmask = __ballot(keepc);
        if (keepc) s_maxidx[m + (int)__popcll(kmask & ((1ull << lane) - 1ull))] = cand_idx[lane + 64 * r];
        m += (int)__popcll(kmask);
      }
    } else {
      if (lane < nmaxima) s_maxidx[lane] = cand_idx[lane];
      m = nmaxima;
    }
    __syncthreads();
    if (m < 4) break;

    AT_MARK("rows")
    // ---- the 2 m + 1 moment rows the segment fits read, then the 45 + 45 fits ---------------------------------------------
    {
      double row[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      if (lane < 2 * m + 1) {
        const int src = fit_staged_row_src(lane, m, s_maxidx, szd);
        if (src >= 0) {
#pragma unroll
          for (int j = 0; j < 6; j++) row[j] = rows[src * 6 + j];
        }
      }
      __syncthreads();   // (every lane holds its row before the region is rewritten)
      if (lane < 2 * m + 1) {
#pragma unroll
        for (int j = 0; j < 6; j++) s_rows[lane * 6 + j] = row[j];
      }
    }
    __syncthreads();
    AT_MARK("pairfits")
    if (lane < 45) { fq_segment_fit(s_tab, s_maxidx, m, szd, lane, 0); fq_segment_fit(s_tab, s_maxidx, m, szd, lane, 1); }
    __syncthreads();
    AT_MARK("combos")
    fq_corner_search(s_tab, s_cpairs, m, szd, lane, P, cands_all, counters, frame, cl_key, q_reversed);
    AT_MARK("end")
    } while (0);
    if (pf < 1) stage1(nxt);
    if (pf < 2) stage2(nxt);
    if (pf < 3) stage3(nxt);
    cur = nxt;
  }
}
