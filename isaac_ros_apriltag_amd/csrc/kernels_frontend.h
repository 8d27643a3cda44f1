// kernels_frontend.h -- front steps that usually feed the detector: resize and rectify of mono8 frames
// (reference README.md:16-29 recommends resizing 4K input; launch/isaac_ros_apriltag_usb_cam.launch.py:43-63
// puts a RectifyNode in front of the AprilTag node).  HBM-streaming kernels; all sampling arithmetic is
// integer fixed point so that the CPU oracle reproduces the bytes exactly.
#pragma once
#include "common.h"
#include "camera_models.h"   // RectifyParams, and the general projection (three distortion models behind a rotation)

// ---- the resize statement (oracle: ato_resize_mono8), stated once for k_resize_mono8 and k_resize_frames.
// dst(x,y) = bilinear sample of src at ((x+0.5)*sw/dw - 0.5, (y+0.5)*sh/dh - 0.5), coordinates in 1/2048.  The position is the same
// statement along x and along y: the two source indices of destination index i and the 1/2048 weight of the second.
struct ResizePos { int i0, i1, w; };
__device__ __forceinline__ ResizePos resize_pos(int i, int sn, int dn) {
  // fixed-point source position: ((2i+1)*sn*1024/dn - 1024), exact in 64-bit integers (tools_hooks.h: RESIZE_FIXED)
  long long f = RESIZE_FIXED(i, sn, dn);
  if (f < 0) f = 0;
  ResizePos p;
  p.i0 = (int)(f >> 11);
  p.w = (int)(f & 2047);
  if (p.i0 >= sn - 1) { p.i0 = sn - 1; p.w = 0; }
  p.i1 = min(p.i0 + 1, sn - 1);
  return p;
}
// the 22-bit rounded blend of the four taps
__device__ __forceinline__ uint32_t resize_blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, int wx, int wy) {
  const uint32_t top = p00 * (2048 - wx) + p01 * wx, bot = p10 * (2048 - wx) + p11 * wx;
  const uint64_t v = (uint64_t)top * (2048 - wy) + (uint64_t)bot * wy;
  return (uint32_t)((v + (1ull << 21)) >> 22);
}

__global__ __launch_bounds__(256) void k_resize_mono8(const uint8_t* __restrict__ src, size_t spitch, int sw, int sh,
                                                      uint8_t* __restrict__ dst, size_t dpitch, int dw, int dh) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= dw || y >= dh) return;
  const ResizePos px = resize_pos(x, sw, dw), py = resize_pos(y, sh, dh);
  const uint8_t *r0 = src + (size_t)py.i0 * spitch, *r1 = src + (size_t)py.i1 * spitch;
  dst[(size_t)y * dpitch + x] = (uint8_t)resize_blend(r0[px.i0], r0[px.i1], r1[px.i0], r1[px.i1], px.w, py.w);
}

// ---- the rectification statement (oracle: ato_rectify_mono8), stated once for k_rectify_mono8 and k_rectify_frames.
// The projection of destination pixel (x, y) is split where its operands allow: what depends on x alone, what on y alone, and the
// rest.  Every operation below is the oracle's, on the oracle's operands, in the oracle's order (no re-association, and
// -ffp-contract=off keeps every product and sum its own IEEE operation): a term formed once and used for many pixels has the value
// it has when it is formed per pixel.
struct RectCol { double xn, xx, txx, p1x, p2x; };   // xn = (x - ncx) / nfx, xn * xn, 2.0 * xn * xn, 2.0 * p1 * xn, 2.0 * p2 * xn
struct RectRow { double yn, yy, tyy; };             // yn = (y - ncy) / nfy, yn * yn, 2.0 * yn * yn
// one sample: the four source pixels of a destination pixel and their 1/32 weights
struct RectTaps { int x0, y0, x1, y1, wx, wy; };

__device__ __forceinline__ RectCol rect_col(int x, const RectifyParams& R) {
  RectCol c;
  c.xn = ((double)x - R.ncx) / R.nfx;
  c.xx = c.xn * c.xn;
  c.txx = 2.0 * c.xn * c.xn;
  c.p1x = 2.0 * R.p1 * c.xn;
  c.p2x = 2.0 * R.p2 * c.xn;
  return c;
}
__device__ __forceinline__ RectRow rect_row(int y, const RectifyParams& R) {
  RectRow r;
  r.yn = ((double)y - R.ncy) / R.nfy;
  r.yy = r.yn * r.yn;
  r.tyy = 2.0 * r.yn * r.yn;
  return r;
}
// the bounds test, the 1/32-pixel position and the clamps of source position (u, v); false: outside the source (the pixel is 0)
__device__ __forceinline__ bool rect_taps_at(double u, double v, int w, int h, RectTaps& t) {
  if (!(u >= 0.0 && v >= 0.0 && u <= (double)(w - 1) && v <= (double)(h - 1))) return false;
  const int fu = RECT_FIXED(u), fv = RECT_FIXED(v);  // 1/32 pixel (tools_hooks.h: (int)(u * 32.0 + 0.5))
  t.x0 = fu >> 5; t.y0 = fv >> 5; t.wx = fu & 31; t.wy = fv & 31;
  if (t.x0 >= w - 1) { t.x0 = w - 1; t.wx = 0; }
  if (t.y0 >= h - 1) { t.y0 = h - 1; t.wy = 0; }
  t.x1 = min(t.x0 + 1, w - 1); t.y1 = min(t.y0 + 1, h - 1);
  return true;
}
// false: the pixel maps outside the source (its value is 0)
__device__ __forceinline__ bool rect_taps(const RectCol& c, const RectRow& r, const RectifyParams& R, int w, int h, RectTaps& t) {
  // normalised pinhole ray of the destination pixel, then the plumb_bob model, then source pixels
  const double xn = c.xn, yn = r.yn;
  const double r2 = c.xx + r.yy;
  const double radial = 1.0 + r2 * (R.k1 + r2 * (R.k2 + r2 * R.k3));
  const double xd = xn * radial + (c.p1x * yn + R.p2 * (r2 + c.txx));
  const double yd = yn * radial + (R.p1 * (r2 + r.tyy) + c.p2x * yn);
  const double u = R.fx * xd + R.cx, v = R.fy * yd + R.cy;
  return rect_taps_at(u, v, w, h, t);
}
// the same for a camera of any kind behind a rotation (camera_models.h), x's and y's terms of its projection given
__device__ __forceinline__ bool cam_taps(const CamCol& c, const CamRow& r, const RectifyParams& R, const CamGeneral& G, int w, int h, RectTaps& t) {
  double u, v;
  return cam_project(c, r, R, G, u, v) && rect_taps_at(u, v, w, h, t);
}
__device__ __forceinline__ uint32_t rect_blend(uint32_t p00, uint32_t p01, uint32_t p10, uint32_t p11, const RectTaps& t) {
  const uint32_t top = p00 * (32 - t.wx) + p01 * t.wx, bot = p10 * (32 - t.wx) + p11 * t.wx;
  return (top * (32 - t.wy) + bot * t.wy + 512) >> 10;
}

__global__ __launch_bounds__(256) void k_rectify_mono8(const uint8_t* __restrict__ src, size_t spitch, uint8_t* __restrict__ dst,
                                                       size_t dpitch, int w, int h, RectifyParams R) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  uint8_t out = 0;
  RectTaps t;
  if (rect_taps(rect_col(x, R), rect_row(y, R), R, w, h, t)) {
    const uint8_t *r0 = src + (size_t)t.y0 * spitch, *r1 = src + (size_t)t.y1 * spitch;
    out = (uint8_t)rect_blend(r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1], t);
  }
  dst[(size_t)y * dpitch + x] = out;
}

// The two statements behind one name, for the tile loops below: Proj<false> is the hoisted plumb_bob statement above (R the identity),
// Proj<true> the general projection of camera_models.h.
template <bool GEN> struct Proj;
template <> struct Proj<false> {
  typedef RectCol Col;
  typedef RectRow Row;
  static __device__ __forceinline__ Col col(int x, const RectifyParams& R, const CamGeneral&) { return rect_col(x, R); }
  static __device__ __forceinline__ Row row(int y, const RectifyParams& R, const CamGeneral&) { return rect_row(y, R); }
  static __device__ __forceinline__ bool taps(const Col& c, const Row& r, const RectifyParams& R, const CamGeneral&, int w, int h, RectTaps& t) {
    return rect_taps(c, r, R, w, h, t);
  }
};
template <> struct Proj<true> {
  typedef CamCol Col;
  typedef CamRow Row;
  static __device__ __forceinline__ Col col(int x, const RectifyParams& R, const CamGeneral& G) { return cam_col(x, R, G); }
  static __device__ __forceinline__ Row row(int y, const RectifyParams& R, const CamGeneral& G) { return cam_row(y, R, G); }
  static __device__ __forceinline__ bool taps(const Col& c, const Row& r, const RectifyParams& R, const CamGeneral& G, int w, int h, RectTaps& t) {
    return cam_taps(c, r, R, G, w, h, t);
  }
};

// amdAprilTagsRectifyMono8Ex: k_rectify_mono8 with the general projection
__global__ __launch_bounds__(256) void k_rectify_mono8_ex(const uint8_t* __restrict__ src, size_t spitch, uint8_t* __restrict__ dst,
                                                          size_t dpitch, int w, int h, RectifyParams R, CamGeneral G) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  uint8_t out = 0;
  RectTaps t;
  if (cam_taps(cam_col(x, R, G), cam_row(y, R, G), R, G, w, h, t)) {
    const uint8_t *r0 = src + (size_t)t.y0 * spitch, *r1 = src + (size_t)t.y1 * spitch;
    out = (uint8_t)rect_blend(r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1], t);
  }
  dst[(size_t)y * dpitch + x] = out;
}

// ---- the front stage of a submission: rectification (amdAprilTagsSetRectification) and resize (amdAprilTagsSetResize) ----------------
// One descriptor per batch slot, written by the host for every submission and uploaded by k_prologue beside the FrameDescs: the
// caller's frame (mono8 or interleaved colour, any base address and pitch) at its own size SW x SH, its camera, the size DW x DH it
// is detected at, and the slot of the handle's front plane it becomes.  Everything behind the front launch sees a mono8 submission
// whose images are those slots.  The slot is S = resize(G), G the frame's gray plane at the source size: convert(frame), or
// rectify(convert(frame)) with `rectify` set (section 7b's statement with w = SW, h = SH and `model`).  A rectify-only slot has
// DW = SW, DH = SH and `rectify` set: k_rectify_frames writes G itself; k_resize_frames never writes G (a tap of the resize that
// falls on G is computed where it is needed).
struct FrontDesc {
  const uint8_t* src;
  uint8_t* dst;          // 4-byte aligned, dst_pitch a multiple of 4 and >= DW rounded up to 4: whole dwords are stored
  uint32_t src_pitch, dst_pitch;
  uint32_t fmt;          // amdAprilTagsEncoding of `src`
  int32_t SW, SH, DW, DH;
  uint32_t rectify;      // 0: G = convert(frame); 1: G = rectify(convert(frame)) with `model`
  RectifyParams model;
  CamGeneral gen;        // gen.general: the slot's camera is not plumb_bob with R = I (the _general kernels switch on it, as on fmt)
};
static_assert(sizeof(FrontDesc) == 64 * 4, "k_prologue copies FrontDesc one word per thread");

// The gray value of source pixel x of a row: mono8 as it stands, colour through the fixed-point BT.601 statement of
// amdAprilTagsConvertToMono8 (k_to_mono8), so that R = rectify(convert(frame)).
template <int NCH, int RIDX, int BIDX, class Row>
__device__ __forceinline__ uint32_t rect_gray(Row row, int x) {
  if (NCH == 1) return row[x];
  const Row p = row + (size_t)x * NCH;
  return gray_bt601(p[RIDX], p[1], p[BIDX]);
}

#define RF_PX 4     // adjacent output pixels of a thread per row: one dword store
#define RF_ROWS 4   // rows of a thread: the column terms (one division each) serve all of them
#define RF_BW (64 * RF_PX)
#define RF_BH (4 * RF_ROWS)

// A block of 256 threads covers RF_BW x RF_BH output pixels of frame blockIdx.z: a wave is 256 pixels wide, a thread RF_PX
// columns by RF_ROWS rows.  The taps are gathered through the cache (neighbouring lanes read neighbouring source bytes).
template <int NCH, int RIDX, int BIDX, bool GEN>
__device__ __forceinline__ void rectify_frame_tile(const FrontDesc& d) {
  const int w = d.SW, h = d.SH;
  const int x4 = (int)blockIdx.x * RF_BW + (int)(threadIdx.x & 63) * RF_PX;
  const int ya = (int)blockIdx.y * RF_BH + (int)(threadIdx.x >> 6) * RF_ROWS;
  if (x4 >= w || ya >= h) return;
  const RectifyParams& R = d.model;
  const CamGeneral& G = d.gen;
  // (the descriptor's pointers are device memory: said so, the compiler addresses them as global, not flat)
  typedef __attribute__((address_space(1))) const uint8_t* GlobalSrc;
  typedef __attribute__((address_space(1))) uint32_t* GlobalDst;
  const GlobalSrc src = (GlobalSrc)d.src;
  typename Proj<GEN>::Col col[RF_PX];
#pragma unroll
  for (int k = 0; k < RF_PX; k++) col[k] = Proj<GEN>::col(x4 + k, R, G);   // (columns at or beyond w: computed, never sampled)
#pragma unroll
  for (int j = 0; j < RF_ROWS; j++) {
    const int y = ya + j;
    if (y >= h) break;
    const typename Proj<GEN>::Row row = Proj<GEN>::row(y, R, G);
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < RF_PX; k++) {
      RectTaps t;
      if (x4 + k < w && Proj<GEN>::taps(col[k], row, R, G, w, h, t)) {
        const GlobalSrc r0 = src + (size_t)t.y0 * d.src_pitch, r1 = src + (size_t)t.y1 * d.src_pitch;
        const uint32_t g = rect_blend(rect_gray<NCH, RIDX, BIDX>(r0, t.x0), rect_gray<NCH, RIDX, BIDX>(r0, t.x1),
                                      rect_gray<NCH, RIDX, BIDX>(r1, t.x0), rect_gray<NCH, RIDX, BIDX>(r1, t.x1), t);
        word |= g << (8 * k);
      }
    }
    *(GlobalDst)(d.dst + (size_t)y * d.dst_pitch + x4) = word;
  }
}

template <bool GEN>
__device__ __forceinline__ void rectify_frame_fmt(const FrontDesc& d) {
  switch (d.fmt) {   // amdAprilTagsEncoding: mono8, rgb8, bgr8, rgba8, bgra8
    case 0: rectify_frame_tile<1, 0, 0, GEN>(d); break;
    case 1: rectify_frame_tile<3, 0, 2, GEN>(d); break;
    case 2: rectify_frame_tile<3, 2, 0, GEN>(d); break;
    case 3: rectify_frame_tile<4, 0, 2, GEN>(d); break;
    default: rectify_frame_tile<4, 2, 0, GEN>(d); break;
  }
}

// every slot's camera is plumb_bob with R = I
__global__ __launch_bounds__(256) void k_rectify_frames(const FrontDesc* __restrict__ descs) {
  const FrontDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x * RF_BW >= d.SW || (int)blockIdx.y * RF_BH >= d.SH) return;   // blocks beyond this frame's extent
  rectify_frame_fmt<false>(d);
}

// Some slot's camera is of another kind or has a rotation: the same launch, with the general projection for the slots that say so.
// (A kernel of its own, chosen by the host per submission, so that k_rectify_frames keeps its registers and occupancy.)
__global__ __launch_bounds__(256) void k_rectify_frames_general(const FrontDesc* __restrict__ descs) {
  const FrontDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x * RF_BW >= d.SW || (int)blockIdx.y * RF_BH >= d.SH) return;
  if (d.gen.general) rectify_frame_fmt<true>(d);
  else rectify_frame_fmt<false>(d);
}

// ---- resize inside the submission, fused with the rectification where that is on ---------------------------------------------------
// G(x, y) with rectification on, x's and y's terms of the projection given: the rectified value, 0 where it maps outside the source
template <int NCH, int RIDX, int BIDX, bool GEN, class Src>
__device__ __forceinline__ uint32_t rectified_gray(Src src, uint32_t pitch, const typename Proj<GEN>::Col& c, const typename Proj<GEN>::Row& r,
                                                   const RectifyParams& R, const CamGeneral& G, int w, int h) {
  RectTaps t;
  if (!Proj<GEN>::taps(c, r, R, G, w, h, t)) return 0u;
  const Src r0 = src + (size_t)t.y0 * pitch, r1 = src + (size_t)t.y1 * pitch;
  return rect_blend(rect_gray<NCH, RIDX, BIDX>(r0, t.x0), rect_gray<NCH, RIDX, BIDX>(r0, t.x1), rect_gray<NCH, RIDX, BIDX>(r1, t.x0),
                    rect_gray<NCH, RIDX, BIDX>(r1, t.x1), t);
}

// The thread shape of rectify_frame_tile: RF_PX adjacent output pixels by RF_ROWS rows, one dword store a row.  What depends on the
// column alone -- the resize position, and with RECT the projection terms of its two source columns -- is formed once for the rows;
// what depends on the row alone once for the pixels.
template <int NCH, int RIDX, int BIDX, bool RECT, bool GEN>
__device__ __forceinline__ void resize_frame_tile(const FrontDesc& d) {
  const int sw = d.SW, sh = d.SH, dw = d.DW, dh = d.DH;
  const int x4 = (int)blockIdx.x * RF_BW + (int)(threadIdx.x & 63) * RF_PX;
  const int ya = (int)blockIdx.y * RF_BH + (int)(threadIdx.x >> 6) * RF_ROWS;
  if (x4 >= dw || ya >= dh) return;
  const RectifyParams& R = d.model;
  const CamGeneral& G = d.gen;
  typedef __attribute__((address_space(1))) const uint8_t* GlobalSrc;
  typedef __attribute__((address_space(1))) uint32_t* GlobalDst;
  const GlobalSrc src = (GlobalSrc)d.src;
  ResizePos px[RF_PX];
  typename Proj<GEN>::Col c0[RECT ? RF_PX : 1], c1[RECT ? RF_PX : 1];
#pragma unroll
  for (int k = 0; k < RF_PX; k++) {
    px[k] = resize_pos(min(x4 + k, dw - 1), sw, dw);   // (columns at or beyond dw: the last column's, never stored)
    if (RECT) { c0[k] = Proj<GEN>::col(px[k].i0, R, G); c1[k] = Proj<GEN>::col(px[k].i1, R, G); }
  }
#pragma unroll
  for (int j = 0; j < RF_ROWS; j++) {
    const int y = ya + j;
    if (y >= dh) break;
    const ResizePos py = resize_pos(y, sh, dh);
    uint32_t word = 0;
    if (RECT) {
      const typename Proj<GEN>::Row r0 = Proj<GEN>::row(py.i0, R, G), r1 = Proj<GEN>::row(py.i1, R, G);
#pragma unroll
      for (int k = 0; k < RF_PX; k++) {
        if (x4 + k >= dw) break;
        const uint32_t p00 = rectified_gray<NCH, RIDX, BIDX, GEN>(src, d.src_pitch, c0[k], r0, R, G, sw, sh);
        const uint32_t p01 = rectified_gray<NCH, RIDX, BIDX, GEN>(src, d.src_pitch, c1[k], r0, R, G, sw, sh);
        const uint32_t p10 = rectified_gray<NCH, RIDX, BIDX, GEN>(src, d.src_pitch, c0[k], r1, R, G, sw, sh);
        const uint32_t p11 = rectified_gray<NCH, RIDX, BIDX, GEN>(src, d.src_pitch, c1[k], r1, R, G, sw, sh);
        word |= resize_blend(p00, p01, p10, p11, px[k].w, py.w) << (8 * k);
      }
    } else {
      const GlobalSrc r0 = src + (size_t)py.i0 * d.src_pitch, r1 = src + (size_t)py.i1 * d.src_pitch;
#pragma unroll
      for (int k = 0; k < RF_PX; k++) {
        if (x4 + k >= dw) break;
        word |= resize_blend(rect_gray<NCH, RIDX, BIDX>(r0, px[k].i0), rect_gray<NCH, RIDX, BIDX>(r0, px[k].i1),
                             rect_gray<NCH, RIDX, BIDX>(r1, px[k].i0), rect_gray<NCH, RIDX, BIDX>(r1, px[k].i1), px[k].w, py.w) << (8 * k);
      }
    }
    *(GlobalDst)(d.dst + (size_t)y * d.dst_pitch + x4) = word;
  }
}

template <bool RECT, bool GEN>
__device__ __forceinline__ void resize_frame_fmt(const FrontDesc& d) {
  switch (d.fmt) {   // amdAprilTagsEncoding: mono8, rgb8, bgr8, rgba8, bgra8
    case 0: resize_frame_tile<1, 0, 0, RECT, GEN>(d); break;
    case 1: resize_frame_tile<3, 0, 2, RECT, GEN>(d); break;
    case 2: resize_frame_tile<3, 2, 0, RECT, GEN>(d); break;
    case 3: resize_frame_tile<4, 0, 2, RECT, GEN>(d); break;
    default: resize_frame_tile<4, 2, 0, RECT, GEN>(d); break;
  }
}

__global__ __launch_bounds__(256) void k_resize_frames(const FrontDesc* __restrict__ descs) {
  const FrontDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x * RF_BW >= d.DW || (int)blockIdx.y * RF_BH >= d.DH) return;   // blocks beyond this frame's target extent
  if (d.rectify) resize_frame_fmt<true, false>(d);
  else resize_frame_fmt<false, false>(d);
}

// as k_rectify_frames_general: chosen by the host when some slot's camera needs the general projection
__global__ __launch_bounds__(256) void k_resize_frames_general(const FrontDesc* __restrict__ descs) {
  const FrontDesc& d = descs[blockIdx.z];
  if ((int)blockIdx.x * RF_BW >= d.DW || (int)blockIdx.y * RF_BH >= d.DH) return;
  if (d.rectify && d.gen.general) resize_frame_fmt<true, true>(d);
  else if (d.rectify) resize_frame_fmt<true, false>(d);
  else resize_frame_fmt<false, false>(d);
}
