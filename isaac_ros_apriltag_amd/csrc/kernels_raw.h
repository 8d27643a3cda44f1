// kernels_raw.h -- Bayer and 16-bit frames to mono8 (the statement: raw_formats.h).  One HBM-streaming launch
// in front of a submission: frame blockIdx.z's source, whatever its base address and pitch, becomes its slot of the handle's plane
// d_raw, and everything behind sees a mono8 submission of those slots.  No LDS, no barrier, no scratch.
#pragma once
#include "raw_formats.h"

// One descriptor per batch slot, written by the host for every raw submission and uploaded by k_prologue beside the FrameDescs.
struct RawDesc {
  const uint8_t* src;    // any address and pitch for 8-bit samples; both even for 16-bit ones
  uint8_t* dst;
  uint32_t src_pitch, dst_pitch;
  uint32_t enc;          // amdAprilTagsEncoding of `src`, 5 .. 13
  uint32_t shift;        // 16-bit encodings: v = min(255, s >> shift)
  int32_t w, h;
  uint32_t store;        // RAW_STORE_*
  uint32_t pad;
};
static_assert(sizeof(RawDesc) % 4 == 0, "k_prologue copies words");
#define RAW_STORE_PLANE 0u   // a slot of d_raw: 4-byte aligned, the pitch a multiple of 4 and >= w rounded up to 4; whole dwords are stored
#define RAW_STORE_DWORD 1u   // a caller's plane, 4-byte aligned with a pitch that is a multiple of 4: dwords that lie inside w, bytes at the tail
#define RAW_STORE_BYTES 2u   // a caller's plane at any address and pitch: bytes

#define RAW_PX 4      // adjacent output pixels of a thread per row: one dword store (the shape of rectify_frame_tile)
#define RAW_ROWS 4    // rows of a thread: RAW_ROWS + 2 source rows are loaded for them
#define RAW_BW (64 * RAW_PX)
#define RAW_BH (4 * RAW_ROWS)

typedef __attribute__((address_space(1))) const uint8_t* RawSrc8;
typedef __attribute__((address_space(1))) const uint16_t* RawSrc16;

// sample x of a source row, BPS bytes per sample
template <int BPS>
__device__ __forceinline__ uint32_t raw_load(RawSrc8 row, int x, uint32_t shift) {
  if (BPS == 1) return row[x];
  return raw_sample16(((RawSrc16)row)[x], shift);   // (base and pitch are even: an aligned 16-bit load, little-endian as the device is)
}

// RAW_PX gray values of row y as one word, stored as the descriptor says
__device__ __forceinline__ void raw_store(const RawDesc& d, int x4, int y, uint32_t word) {
  uint8_t* const p = d.dst + (size_t)y * d.dst_pitch + x4;
  if (d.store == RAW_STORE_PLANE || (d.store == RAW_STORE_DWORD && x4 + RAW_PX <= d.w)) {
    *(__attribute__((address_space(1))) uint32_t*)p = word;
  } else {
#pragma unroll
    for (int k = 0; k < RAW_PX; k++)
      if (x4 + k < d.w) ((__attribute__((address_space(1))) uint8_t*)p)[k] = (uint8_t)(word >> (8 * k));
  }
}

// A thread's RAW_PX columns by RAW_ROWS rows of a Bayer frame, from output pixel (x4, ya).  Over its rows it keeps a sliding window of
// three source rows, RAW_PX + 2 samples each, so every source row is loaded once.  The columns' indices are formed once: only the
// threads on the frame's left and right edge meet the reflect rule (columns at or beyond w: an index inside the row, never stored).
template <int BPS>
__device__ __forceinline__ void raw_bayer_tile(const RawDesc& d, int x4, int ya) {
  const int w = d.w, h = d.h;
  if (x4 >= w || ya >= h) return;
  const uint32_t phase = raw_phase(d.enc);
  const uint32_t px = RAW_XPHASE(BPS, phase & 1u), py = phase >> 1;
  const RawSrc8 src = (RawSrc8)d.src;
  int cx[RAW_PX + 2];
  const bool edge = x4 == 0 || x4 + RAW_PX + 1 > w;
#pragma unroll
  for (int k = 0; k < RAW_PX + 2; k++) {
    int i = x4 - 1 + k;
    if (edge) i = max(0, min(raw_reflect(i, w), w - 1));
    cx[k] = i;
  }
  uint32_t a[RAW_PX + 2], b[RAW_PX + 2], c[RAW_PX + 2];   // rows y - 1, y, y + 1
  {
    const RawSrc8 ra = src + (size_t)raw_reflect(ya - 1, h) * d.src_pitch, rb = src + (size_t)ya * d.src_pitch;
#pragma unroll
    for (int k = 0; k < RAW_PX + 2; k++) { a[k] = raw_load<BPS>(ra, cx[k], d.shift); b[k] = raw_load<BPS>(rb, cx[k], d.shift); }
  }
#pragma unroll
  for (int j = 0; j < RAW_ROWS; j++) {
    const int y = ya + j;
    if (y >= h) break;
    const RawSrc8 rc = src + (size_t)raw_reflect(y + 1, h) * d.src_pitch;   // (y + 1 <= h: row h - 2 at the bottom edge, h >= 2)
#pragma unroll
    for (int k = 0; k < RAW_PX + 2; k++) c[k] = raw_load<BPS>(rc, cx[k], d.shift);
    const bool yr = (((uint32_t)y ^ py) & 1u) == 0u;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < RAW_PX; k++) {
      const bool xr = (((uint32_t)k ^ px) & 1u) == 0u;   // (x4 is a multiple of 4)
      word |= raw_bayer_gray(b[k + 1], a[k + 1], c[k + 1], b[k + 2], b[k], a[k + 2], a[k], c[k + 2], c[k], xr, yr) << (8 * k);
    }
    raw_store(d, x4, y, word);
#pragma unroll
    for (int k = 0; k < RAW_PX + 2; k++) { a[k] = b[k]; b[k] = c[k]; }
  }
}

// the plain path: mono16, gray = v
__device__ __forceinline__ void raw_mono16_tile(const RawDesc& d, int x4, int ya) {
  const int w = d.w, h = d.h;
  if (x4 >= w || ya >= h) return;
  const RawSrc8 src = (RawSrc8)d.src;
#pragma unroll
  for (int j = 0; j < RAW_ROWS; j++) {
    const int y = ya + j;
    if (y >= h) break;
    const RawSrc8 row = src + (size_t)y * d.src_pitch;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < RAW_PX; k++) word |= raw_load<2>(row, min(x4 + k, w - 1), d.shift) << (8 * k);
    raw_store(d, x4, y, word);
  }
}

#define RAW_KIND_BAYER8 1
#define RAW_KIND_MONO16 2
#define RAW_KIND_BAYER16 3
__host__ __device__ __forceinline__ int raw_kind(uint32_t enc) {
  return !raw_is_raw(enc) ? 0 : enc == RAW_ENC_MONO16 ? RAW_KIND_MONO16 : raw_is_16(enc) ? RAW_KIND_BAYER16 : RAW_KIND_BAYER8;
}

// One frame.  A block of 256 threads covers RAW_BW x RAW_BH output pixels: a wave is 256 pixels wide.  The blocks stride over the
// frame's tiles by the grid's extent, so a launch sized for the handle converts a larger source too (amdAprilTagsSetResize), and the
// blocks beyond a frame's own extent return.
template <int KIND>
__device__ __forceinline__ void raw_frame(const RawDesc& d) {
  const int tx = (int)(threadIdx.x & 63) * RAW_PX, ty = (int)(threadIdx.x >> 6) * RAW_ROWS;
  for (int by = (int)blockIdx.y * RAW_BH; by < d.h; by += (int)gridDim.y * RAW_BH)
    for (int bx = (int)blockIdx.x * RAW_BW; bx < d.w; bx += (int)gridDim.x * RAW_BW) {
      if (KIND == RAW_KIND_MONO16) raw_mono16_tile(d, bx + tx, by + ty);
      else raw_bayer_tile<KIND == RAW_KIND_BAYER16 ? 2 : 1>(d, bx + tx, by + ty);
    }
}

// the submission's launch: grid z is the batch slot
template <int KIND>
__global__ __launch_bounds__(256) void k_raw_to_mono8_frames(const RawDesc* __restrict__ descs) {
  const RawDesc d = descs[blockIdx.z];
  raw_frame<KIND>(d);
}

// amdAprilTagsConvertRawToMono8: the same device function for one frame
template <int KIND>
__global__ __launch_bounds__(256) void k_raw_to_mono8(const RawDesc d) {
  raw_frame<KIND>(d);
}
