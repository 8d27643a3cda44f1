// fit_statements.h -- the arithmetic of the quad fit that more than one kernel needs, each statement ONCE.
// k_fit_quads, k_fit_prefilter (kernels_quad.h) and k_fit_small (kernels_quad_small.h) must give the CPU oracle's results
// bit for bit, so every statement below is upstream's, in upstream's order of operations, and its comment names the function
// of oracle/apriltag_oracle.c it mirrors.  The kernels differ in where the data lives and in what order the points arrive;
// none of them retypes what is stated here.  Functions only: no kernels, no LDS, no barriers.
// Included by kernels_quad.h behind D2 / split_term / wave_scan_f64 / key_enc, which it uses.
//
// The SECOND WORDING: the general moment sweep of k_fit_quads<NT, false> (images beyond 2048 x 2048 working pixels, where the
// two-double sums do not hold) forms the weight as __dsqrt_rn of the squared gradient and addresses the image with 64-bit
// offsets, because neither sqrt_u18's argument range nor the 24-bit row multiply of fit_grad2 is checked for that path.  It
// shares fit_moment_terms and nothing else of the sweep.
#pragma once

// ---- the packed point word (unpack_point): x << 18 | y << 4 | (sgn gx + 1) << 2 | (sgn gy + 1), x and y in half pixels -------
__device__ __forceinline__ int fit_point_x(uint32_t p) { return (int)(p >> 18); }
__device__ __forceinline__ int fit_point_y(uint32_t p) { return (int)((p >> 4) & 0x3FFF); }
// gradient SIGNS (-1, 0, 1); the gradients themselves are 255 times these
__device__ __forceinline__ int fit_point_sgx(uint32_t p) { return (int)((p >> 2) & 3) - 1; }
__device__ __forceinline__ int fit_point_sgy(uint32_t p) { return (int)(p & 3) - 1; }
// what a lane without a point takes in its place: a point of the cluster with a zero gradient (neither box nor sums change)
__device__ __forceinline__ uint32_t fit_pad_point(uint32_t p0) { return (p0 & ~15u) | 5u; }

// ---- bounding box and exact gradient dot (fit_quad, first loop) --------------------------------------------------------------
struct FitBox { int xmin = 1 << 30, xmax = -1, ymin = 1 << 30, ymax = -1; };
// sums over a few points of x sgn(gx) + y sgn(gy), sgn(gx), sgn(gy) in 32 bits (24-bit multiplies); the caller scales by 255
struct FitDotPart { int xg = 0, gx = 0, gy = 0; };
__device__ __forceinline__ void fit_box_add(FitBox& b, FitDotPart& t, bool have, uint32_t p, uint32_t p0) {
  const uint32_t q = have ? p : fit_pad_point(p0);
  const int x = fit_point_x(q), y = fit_point_y(q);
  const int gx = fit_point_sgx(q), gy = fit_point_sgy(q);
  b.xmin = min(b.xmin, x); b.xmax = max(b.xmax, x); b.ymin = min(b.ymin, y); b.ymax = max(b.ymax, y);
  t.xg += __mul24(x, gx) + __mul24(y, gy);
  t.gx += gx; t.gy += gy;
}

// ---- box -> area test, centre, border direction and the border-acceptance tests (fit_quad) -------------------------------------
// Four statements, not one function with a verdict: a kernel leaves the cluster between them.  (As one function that forms the
// centre and the dot product ahead of the area test, and with the two border tests joined by ||, the k_fit_quads instances -- all
// at their 128-register limit -- came out with up to 52 bytes more scratch; in this form none has more than before.)
__device__ __forceinline__ bool fit_box_too_small(const FitBox& b, const DetParams& P) {
  return (b.xmax - b.xmin) * (b.ymax - b.ymin) < P.min_tag_width;
}
struct FitCentre { double x, y; };
__device__ __forceinline__ FitCentre fit_centre(const FitBox& b) {
  FitCentre c;
  c.x = (b.xmin + b.xmax) * 0.5 + 0.05118; c.y = (b.ymin + b.ymax) * 0.5 + -0.028581;
  return c;
}
// sxg, sgx, sgy: the exact sums of x gx + y gy, gx, gy over the cluster's points
__device__ __forceinline__ int fit_border_reversed(const FitCentre& c, double sxg, double sgx, double sgy) {
  const double dot = sxg - c.x * sgx - c.y * sgy;
  return dot < 0;
}
__device__ __forceinline__ bool fit_border_unwanted(int reversed, const DetParams& P) {
  if (!P.reversed_border && reversed) return true;
  if (FIT_NORMAL_UNWANTED(P, reversed)) return true;   // (tools_hooks.h: !P.normal_border && !reversed)
  return false;
}

// ---- slope of a point about the centre and its sort key (fit_quad, slope key) ---------------------------------------------------
// A band of the key per quadrant, FIT_BAND wide; fq_sector64 (kernels_quad.h) cuts its sectors inside the same bands.
constexpr float FIT_BAND = 65536.0f, FIT_BAND2 = 131072.0f;
__device__ __forceinline__ float fit_slope(uint32_t p, float cx, float cy) {
  float dx = (float)fit_point_x(p) - cx, dy = (float)fit_point_y(p) - cy;
  float quadrant;
  if (dy > 0) quadrant = (dx > 0) ? FIT_BAND : FIT_BAND2;
  else quadrant = (dx > 0) ? 0.0f : -FIT_BAND;
  if (dy < 0) { dy = -dy; dx = -dx; }
  if (dx < 0) { float tmp = dx; dx = dy; dy = -tmp; }
  return quadrant + __fdiv_rn(dy, dx);
}
// total order (slope, y, x, gradient signs), stored so that it sorts as an IEEE double (key_enc)
__device__ __forceinline__ unsigned long long fit_sort_key(float slope, uint32_t p) {
  return key_enc(((unsigned long long)float_sortable(slope) << 32) | ((unsigned long long)fit_point_y(p) << 18) |
                 ((unsigned long long)fit_point_x(p) << 4) | (unsigned long long)(p & 15u));
}

// ---- a decoded key: half-pixel position, and the duplicate test against the key before it (fit_quad, duplicate removal) -------
__device__ __forceinline__ uint32_t fit_key_px(unsigned long long key) { return (uint32_t)((key >> 4) & 0x3FFF); }
__device__ __forceinline__ uint32_t fit_key_py(unsigned long long key) { return (uint32_t)((key >> 18) & 0x3FFF); }
__device__ __forceinline__ bool fit_key_moved(unsigned long long key, unsigned long long prev) { return (key >> 4) != (prev >> 4); }
// coordinate of half-pixel position h: h / 2 + 1 / 2, exactly
__device__ __forceinline__ double fit_coord(uint32_t h) { return (int)(h + 1) * .5; }

// ---- squared gradient at a half-pixel position (fit_quad, compute_lfps); 0 on the image border, where no gradient is taken ----
// Its integer part and the image offset stay in 32-bit integers (rows below 2^14, pitches below 2^24, a frame below 2^31 bytes:
// check_images); the four neighbours are loaded before the first is used.
typedef const __attribute__((address_space(1))) uint8_t* fit_gray_ptr;   // global, not generic
__device__ __forceinline__ uint32_t fit_grad2(fit_gray_ptr ggray, int gpitch, uint32_t px, uint32_t py, int W, int H, bool have = true) {
  const int ix = (int)((px + 1) >> 1), iy = (int)((py + 1) >> 1);
  uint32_t G = 0;
  if (have & ((unsigned)(ix - 1) < (unsigned)(W - 2)) & ((unsigned)(iy - 1) < (unsigned)(H - 2))) {
    const uint32_t o = __umul24((uint32_t)iy, (uint32_t)gpitch) + (uint32_t)ix;
    const int g_r = ggray[o + 1], g_l = ggray[o - 1], g_d = ggray[o + (uint32_t)gpitch], g_u = ggray[o - (uint32_t)gpitch];
    const int grad_x = g_r - g_l, grad_y = g_d - g_u;
    G = (uint32_t)(grad_x * grad_x + grad_y * grad_y);
  }
  return G;
}

// ---- weight and the six moment terms of a point (fit_quad, compute_lfps), and their exact addition to six D2 sums --------------
__device__ __forceinline__ double fit_weight(uint32_t G) { return sqrt_u18(G) + 1; }
__device__ __forceinline__ void fit_moment_terms(double Wt, double x, double y, double (&tt)[6]) {
  tt[0] = Wt * x; tt[1] = Wt * y; tt[2] = Wt * x * x; tt[3] = Wt * x * y; tt[4] = Wt * y * y; tt[5] = Wt;
}
__device__ __forceinline__ void fit_terms_add(D2 (&sum)[6], uint32_t G, uint32_t px, uint32_t py) {
  double tt[6];
  fit_moment_terms(fit_weight(G), fit_coord(px), fit_coord(py), tt);
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const D2 t = split_term(tt[j]);
    sum[j].hi += t.hi; sum[j].lo += t.lo;
  }
}
// lane totals onto the grid (|lo| <= 2^-7, see split_term), then their inclusive scans over the wave
__device__ __forceinline__ void fit_scan_totals(D2 (&acc)[6], D2 (&incl)[6]) {
#pragma unroll
  for (int j = 0; j < 6; j++) {
    const double c = (acc[j].lo + AT_SPLIT_C) - AT_SPLIT_C;
    acc[j].hi += c; acc[j].lo -= c;
    incl[j].hi = wave_scan_f64(acc[j].hi);
    incl[j].lo = wave_scan_f64(acc[j].lo);
  }
}

// ---- windowed errors, smoothing, maxima (quad_segment_maxima) ---------------------------------------------------------------------
// cyclic index of k in [-szd, 2 szd) (compare / subtract: integer division by a run-time value costs ~40 instructions)
__device__ __forceinline__ int fit_wrap(int k, int szd) { return k < 0 ? k + szd : (k >= szd ? k - szd : k); }
// ends of the window of point i: i -+ ksz, cyclic
__device__ __forceinline__ int fit_window_i0(int i, int ksz, int szd) { return (i >= ksz) ? i - ksz : i - ksz + szd; }
__device__ __forceinline__ int fit_window_i1(int i, int ksz, int szd) { return (i + ksz < szd) ? i + ksz : i + ksz - szd; }
// the seven Gaussian taps (GAUSS7: floats, widened) over errors i - 3 .. i + 3, summed from zero in that order.  Takes the
// loaded values, not the array: handed a pointer and an index the one-wave kernels came out longer.
__device__ __forceinline__ double fit_smooth7(double em3, double em2, double em1, double e0, double ep1, double ep2, double ep3) {
  const float f0 = 0x1.6c0504p-7f, f1 = 0x1.152aaap-3f, f2 = 0x1.368b3p-1f;
  const double F0 = (double)f0, F1 = (double)f1, F2 = (double)f2;
  double a = 0;
  a += em3 * F0;
  a += em2 * F1;
  a += em1 * F2;
  a += e0 * 1.0;
  a += ep1 * F2;
  a += ep2 * F1;
  a += ep3 * F0;
  return a;
}
// local maximum: greater than both cyclic neighbours
__device__ __forceinline__ int fit_next(int i, int szd) { return i + 1 < szd ? i + 1 : 0; }
__device__ __forceinline__ int fit_prev(int i, int szd) { return i > 0 ? i - 1 : szd - 1; }
__device__ __forceinline__ bool fit_is_max(double e, double e_next, double e_prev) { return e > e_next && e > e_prev; }

// ---- source row of staged row r of the 2 m + 1 the segment fits read: rows 0 .. m-1 at the maxima, m .. 2m-1 before them (-1:
// before point 0, nothing), 2m the last row (fit_line's three row reads) ---------------------------------------------------------
__device__ __forceinline__ int fit_staged_row_src(int r, int m, const int* s_maxidx, int szd) {
  return r < m ? s_maxidx[r] : r < 2 * m ? s_maxidx[r - m] - 1 : szd - 1;
}
