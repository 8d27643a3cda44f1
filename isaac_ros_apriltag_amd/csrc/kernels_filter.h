// kernels_filter.h -- quad_sigma: the Gaussian blur (sigma > 0) or sharpen (sigma < 0) AprilRobotics applies to the working image
// before thresholding (apriltag_detector_detect / image_u8_gaussian_blur), as DESIGN.md section 7 defines it: integer taps k[0..ksz)
// (sum <= 255), one 1-D pass along the rows, one down the columns, each y[i] = (sum_j k[j] x[i-h+j]) >> 8 for h <= i <= n-h-2 and a copy
// of every other sample; sharpen is clamp(2 G - B, 0, 255).  All integer: the device result equals the CPU restatement bit for bit.
//
// HBM-bound streaming kernel, 2 B per working pixel algorithmic (the source samples read once, the plane written once):
//   * a 256-thread block owns a 128 x 32 pixel output tile; the source rows of the tile plus KH above and below land in LDS as 16-byte
//     units (one 16-pixel halo unit each side, KH <= 8), through the threshold pass's loader (th_load16: decimating gather, colour);
//   * the row pass reads 40 bytes of LDS per 16 output pixels and sums four taps per v_dot4_u32_u8 (taps fit in u8);
//   * the column pass sums 2 KH + 1 rows of the row pass with packed 16-bit multiply-adds (every sum is below 2^16: exact), then the
//     copy rule of the rows, the sharpen clamp, and one non-temporal 16-byte store per 16 pixels.
// KH (template) is the padded half width: taps are centred at KH and zero-padded, so one instance serves every h <= KH.
#pragma once
#include "common.h"
#include "kernels_threshold.h"

#define QS_TW 128                 // output tile, working pixels
#define QS_TH 32
#define QS_IW (QS_TW + 32)        // LDS row of the source tile: one 16-pixel halo unit each side
#define QS_MAX_KSZ 17             // |sigma| <= 4

struct QsTaps {
  uint32_t tk[5];   // taps k'[0 .. 2 KH] of the launched instance (k centred at KH, zeros around it), four per dword, low byte first
  int h;            // upstream's half width: ksz / 2
  int ksz;
  int sharpen;      // sigma < 0
  int kind;         // source: 0..4 decimate 1, amdAprilTagsEncoding of fd.src; 5, 6, 7 decimate 2, 3, 4, mono8 fd.img
};

typedef unsigned short qs_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void qs_load16(int kind, th_gimg_t img, uint32_t pitch, int W0, int H0, bool aligned, int x, int y, uint32_t v[4]) {
  switch (kind) {   // (uniform over the launch)
    case 0: th_load16<1, 0>(img, pitch, W0, H0, aligned, x, y, v); break;
    case 1: th_load16<1, 1>(img, pitch, W0, H0, aligned, x, y, v); break;
    case 2: th_load16<1, 2>(img, pitch, W0, H0, aligned, x, y, v); break;
    case 3: th_load16<1, 3>(img, pitch, W0, H0, aligned, x, y, v); break;
    case 4: th_load16<1, 4>(img, pitch, W0, H0, aligned, x, y, v); break;
    case 5: th_load16<2, 0>(img, pitch, W0, H0, aligned, x, y, v); break;
    case 6: th_load16<3, 0>(img, pitch, W0, H0, aligned, x, y, v); break;
    default: th_load16<4, 0>(img, pitch, W0, H0, aligned, x, y, v); break;
  }
}

// Launch: 1-D grid of 8 * ceil(T / 8) blocks, T = gx * gy * frames tiles, with k_threshold's XCD map (every XCD gets a contiguous run
// of tiles, x fastest, then y, then frame: the halo rows a tile re-reads from its vertical neighbours stay in that XCD's L2).
// Writes the filtered working image of every frame into its slot of gray_all (pitch P.WS).
template <int KH>
__global__ __launch_bounds__(256) void k_quad_sigma(const FrameDesc* __restrict__ frames, uint8_t* __restrict__ gray_all, int gx, int gy,
                                                    int nframes, QsTaps T, DetParams P) {
  constexpr int IH = QS_TH + 2 * KH;            // source rows of the tile
  constexpr int NG = (2 * KH + 1 + 3) / 4;      // dwords of taps
  __shared__ __attribute__((aligned(16))) uint8_t sg[IH * QS_IW];    // G: rows y0 - KH .., columns x0 - 16 ..
  __shared__ __attribute__((aligned(16))) uint8_t st[IH * QS_TW];    // the row pass: rows y0 - KH .., columns x0 ..

  const int ntiles = gx * gy * nframes;
  const int per_xcd = (int)(gridDim.x >> 3);
  const int tile = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
  if (tile >= ntiles) return;
  const int lframe = tile / (gx * gy);
  const int trem = tile - lframe * (gx * gy);
  const int frame = lframe + P.frame0;
  const int x0 = (trem % gx) * QS_TW, y0 = (trem / gx) * QS_TH;
  const FrameDesc fd = frames[frame];
  const int fW = fd.W, fH = fd.H;   // the frame's own working extents (the identity and edge-copy rules follow them); the grid is the handle's
  if (x0 >= fW || y0 >= fH) return;
  const th_gimg_t simg = (th_gimg_t)(T.kind < 5 ? fd.src : fd.img);
  const uint32_t spitch = T.kind < 5 ? fd.src_pitch : fd.pitch;
  const bool aligned = ((((uintptr_t)simg) | (uintptr_t)spitch) & 15) == 0;
  const int tid = threadIdx.x;

  // ---- source tile: IH rows x 10 units (pixels outside the working image are 0; no output that is computed reads them) ----------
  for (int u = tid; u < IH * 10; u += 256) {
    const int r = u / 10, c = u - r * 10;
    const int y = y0 - KH + r, x = x0 - 16 + 16 * c;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (y >= 0 && y < fH && x >= 0 && x < fW) qs_load16(T.kind, simg, spitch, fd.W0, fd.H0, aligned, x, y, v);
    th_u32x4 w; w.x = v[0]; w.y = v[1]; w.z = v[2]; w.w = v[3];
    *reinterpret_cast<th_u32x4*>(sg + r * QS_IW + 16 * c) = w;
  }
  __syncthreads();

  // ---- row pass: IH rows x 8 units of 16 pixels ------------------------------------------------------------------------------
  const bool rows_filter = fW > T.ksz, cols_filter = fH > T.ksz;
  for (int u = tid; u < IH * 8; u += 256) {
    const int r = u >> 3, c = u & 7;
    const int x = x0 + 16 * c;
    const uint2* src = reinterpret_cast<const uint2*>(sg + r * QS_IW + 16 * c + 8);   // bytes x - 8 .. x + 32
    uint32_t d[10];
#pragma unroll
    for (int q = 0; q < 5; q++) { const uint2 t = src[q]; d[2 * q] = t.x; d[2 * q + 1] = t.y; }
    const bool interior = rows_filter && x >= T.h && x + 15 <= fW - QS_FAR_EDGE_H(KH, T.h) - 2;   // (tools_hooks.h: T.h)
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int p = 0; p < 16; p++) {
      uint32_t acc = 0;
#pragma unroll
      for (int g = 0; g < NG; g++) {
        const int ob = 8 + p - KH + 4 * g;   // first source byte of tap group g
        const uint32_t w = (ob & 3) ? __builtin_amdgcn_alignbyte(d[ob / 4 + 1], d[ob / 4], ob & 3) : d[ob / 4];
        acc = __builtin_amdgcn_udot4(w, T.tk[g], acc, false);
      }
      uint32_t t = acc >> 8;
      if (!interior) {
        const int xp = x + p;
        if (!(rows_filter && xp >= T.h && xp <= fW - QS_FAR_EDGE_H(KH, T.h) - 2)) t = (d[(8 + p) / 4] >> (8 * ((8 + p) & 3))) & 0xFFu;
      }
      o[p >> 2] |= t << (8 * (p & 3));
    }
    th_u32x4 w; w.x = o[0]; w.y = o[1]; w.z = o[2]; w.w = o[3];
    *reinterpret_cast<th_u32x4*>(st + r * QS_TW + 16 * c) = w;
  }
  __syncthreads();

  // ---- column pass: 32 rows x 8 units, one per thread ---------------------------------------------------------------------------
  const int r = tid >> 3, c = tid & 7;
  const int y = y0 + r, x = x0 + 16 * c;
  if (y >= fH || x >= P.WS) return;
  uint32_t o[4];
  if (cols_filter && y >= T.h && y <= fH - QS_FAR_EDGE_H(KH, T.h) - 2) {
    qs_u16x2 lo[4], hi[4];
#pragma unroll
    for (int q = 0; q < 4; q++) { lo[q] = (qs_u16x2)(0); hi[q] = (qs_u16x2)(0); }
#pragma unroll
    for (int j = 0; j < 2 * KH + 1; j++) {
      const uint32_t kj = (T.tk[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      const qs_u16x2 tap = __builtin_bit_cast(qs_u16x2, kj * 0x00010001u);
      const th_u32x4 t = *reinterpret_cast<const th_u32x4*>(st + (r + j) * QS_TW + 16 * c);
      const uint32_t tw[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int q = 0; q < 4; q++) {
        lo[q] += tap * __builtin_bit_cast(qs_u16x2, tw[q] & 0x00FF00FFu);
        hi[q] += tap * __builtin_bit_cast(qs_u16x2, (tw[q] >> 8) & 0x00FF00FFu);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
      o[q] = ((__builtin_bit_cast(uint32_t, lo[q]) >> 8) & 0x00FF00FFu) | (__builtin_bit_cast(uint32_t, hi[q]) & 0xFF00FF00u);
  } else {   // a row the column pass copies
    const th_u32x4 t = *reinterpret_cast<const th_u32x4*>(st + (r + KH) * QS_TW + 16 * c);
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
  }
  if (T.sharpen) {
    const th_u32x4 g4 = *reinterpret_cast<const th_u32x4*>(sg + (r + KH) * QS_IW + 16 + 16 * c);
    const uint32_t gw[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
      uint32_t s = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int v = 2 * (int)((gw[q] >> (8 * b)) & 0xFFu) - (int)((o[q] >> (8 * b)) & 0xFFu);
        s |= (uint32_t)min(max(v, 0), 255) << (8 * b);
      }
      o[q] = s;
    }
  }
  th_u32x4 ov; ov.x = o[0]; ov.y = o[1]; ov.z = o[2]; ov.w = o[3];
  __builtin_nontemporal_store(ov, reinterpret_cast<th_u32x4*>(gray_all + (size_t)frame * P.H * P.WS + (size_t)y * P.WS + x));
}
