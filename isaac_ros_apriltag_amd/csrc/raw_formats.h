// raw_formats.h -- Bayer and 16-bit frames as gray: the one statement of DESIGN.md section 7k, for the device (kernels_raw.h) and
// the host (detector.hip: the checks at submit).  Reference for the tests: tests/raw_formats_ref.py.
//
// Encodings (amdAprilTagsEncoding, the names of sensor_msgs/image_encodings): 5 .. 8 bayer_rggb8, bayer_bggr8, bayer_gbrg8,
// bayer_grbg8; 9 mono16; 10 .. 13 bayer_rggb16, bayer_bggr16, bayer_gbrg16, bayer_grbg16.  A Bayer name lists the colours of pixels
// (0,0), (1,0) of row 0, then (0,1), (1,1) of row 1.  The four patterns are one pattern shifted: the red site's phase (px, py) is
// (0,0) for rggb, (1,0) for grbg, (0,1) for gbrg, (1,1) for bggr, and pixel (x, y) is a red site where x = px and y = py (mod 2),
// a blue site where neither holds, a green site of a red row where only y does, of a blue row where only x does.
//
// The sample v(x, y), 0 .. 255: the byte of an 8-bit encoding; min(255, s >> shift) of a 16-bit one, s the little-endian uint16 at
// byte 2x of the row and shift the handle's raw shift (0 .. 8, default 8; a 12-bit sensor sets 4).
//
// mono16: gray = v.  Bayer: bilinear, then the project's one gray statement (common.h: gray_bt601).  Neighbour indices are reflected
// about the border, r(i, n) = i < 0 ? -i : i >= n ? 2 (n - 1) - i : i, which keeps the colour parity and needs w, h >= 2.  With
// N, S, E, W, NE, NW, SE, SW the samples at the reflected neighbours:
//   red site                   R = v                        G = (N + S + E + W + 2) >> 2    B = (NE + NW + SE + SW + 2) >> 2
//   blue site                  R = (NE + NW + SE + SW + 2) >> 2   G = (N + S + E + W + 2) >> 2    B = v
//   green site in a red row    R = (E + W + 1) >> 1         G = v                           B = (N + S + 1) >> 1
//   green site in a blue row   R = (N + S + 1) >> 1         G = v                           B = (E + W + 1) >> 1
// Integer arithmetic throughout: the bytes are the same anywhere, and a flat region gives v back (the weights of gray_bt601 sum to 2^14).
//
// Composition (detector.hip: fill_raw).  The conversion is one launch of its own in front of everything; behind it the submission IS a
// mono8 submission of slots of the handle's plane d_raw.  So every record of a raw submission is exactly the record of the same handle
// given convert(frame) as a mono8 frame: at every decimate, tile size and quad_sigma, with per-frame sizes, with corner undistortion,
// bundles, refinement, covariance and rig on; and rectification and resize read the converted plane as their mono8 source,
// G = convert(frame) in section 7b / 7c.  A window into a Bayer image names the pattern at the window's first pixel: a window that
// starts at odd x turns rggb into grbg, one that starts at odd y turns it into gbrg.  All frames of a submission share one encoding.
#pragma once
#include "common.h"

#define RAW_ENC_FIRST 5u    // bayer_rggb8
#define RAW_ENC_MONO16 9u
#define RAW_ENC_LAST 13u    // bayer_grbg16
#define RAW_MAX_SHIFT 8u

__host__ __device__ __forceinline__ bool raw_is_raw(uint32_t enc) { return enc >= RAW_ENC_FIRST && enc <= RAW_ENC_LAST; }
__host__ __device__ __forceinline__ bool raw_is_16(uint32_t enc) { return enc >= RAW_ENC_MONO16 && enc <= RAW_ENC_LAST; }
__host__ __device__ __forceinline__ bool raw_is_bayer(uint32_t enc) { return raw_is_raw(enc) && enc != RAW_ENC_MONO16; }
__host__ __device__ __forceinline__ uint32_t raw_bytes_per_sample(uint32_t enc) { return raw_is_16(enc) ? 2u : 1u; }
// the red site's phase of a Bayer encoding, px | py << 1 (the order of the names: rggb, bggr, gbrg, grbg)
__host__ __device__ __forceinline__ uint32_t raw_phase(uint32_t enc) {
  const uint32_t k = (enc - RAW_ENC_FIRST) % 5u;   // 0 .. 3 for either sample width (4: mono16, no phase)
  return k == 0 ? 0u : k == 1 ? 3u : k == 2 ? 2u : k == 3 ? 1u : 0u;
}

// the sample of a 16-bit encoding (tools_hooks.h: RAW_SATURATE is min(s, 255))
__host__ __device__ __forceinline__ uint32_t raw_sample16(uint32_t s, uint32_t shift) {
  s >>= shift;
  return RAW_SATURATE(s);
}
// a neighbour index reflected about the border (tools_hooks.h: RAW_REFLECT_FAR is 2 (n - 1) - i)
__host__ __device__ __forceinline__ int raw_reflect(int i, int n) { return i < 0 ? -i : i >= n ? RAW_REFLECT_FAR(i, n) : i; }

// The gray value of one Bayer pixel from its sample v and its eight reflected neighbours; xr: its column is a red column
// (x = px mod 2), yr: its row is a red row (y = py mod 2).
__host__ __device__ __forceinline__ uint32_t raw_bayer_gray(uint32_t v, uint32_t N, uint32_t S, uint32_t E, uint32_t W, uint32_t NE,
                                                            uint32_t NW, uint32_t SE, uint32_t SW, bool xr, bool yr) {
  const uint32_t cross = (N + S + E + W + 2u) >> 2, diag = (NE + NW + SE + SW + 2u) >> 2;
  const uint32_t hor = (E + W + 1u) >> 1, ver = (N + S + 1u) >> 1;
  uint32_t R, G, B;
  if (xr == yr) {   // red or blue site
    G = cross;
    R = yr ? v : diag;
    B = yr ? diag : v;
  } else {          // green site: of a red row the red neighbours lie east and west, of a blue row north and south
    G = v;
    const bool red_hor = RAW_GREEN_RED_HORIZONTAL(yr);   // (tools_hooks.h: yr)
    R = red_hor ? hor : ver;
    B = red_hor ? ver : hor;
  }
  return gray_bt601(R, G, B);
}
