// code_index.h -- the pigeonhole code index of a large tag family: which codes of a family's table can lie within
// max_hamming bits of a word, found by exact match on pieces of the word instead of by a scan of the table.  Stated once, in plain
// integer operations, for host and device: every function here is __host__ __device__ under hipcc and an ordinary inline function
// under g++ (tests/aux_c/code_index_driver.cpp compiles these lines and prints what they give; tests/decode_lookup_ref.py states
// them in Python integers).  The statement and its host-tested build and lookup only: no kernel of the library includes this header
// yet, k_decode_wave still scans (DESIGN.md section 7l says why).
//
// The statement.  K = max_hamming + 1 chunks; chunk j covers the code's bits [floor(j * nbits / K), floor((j + 1) * nbits / K)),
// counted from the LSB; its key is the low min(chunk length, 16) bits of the chunk.  Per chunk one CSR table: offsets[2^keybits + 1],
// then the indices of the family's codes grouped by key, ascending inside a bucket.  A chunk of zero bits (nbits < K) has one bucket
// that holds every code.  A word's candidates are the codes of the K buckets at the word's keys; the answer is the smallest
// (hamming distance, index) among them, found iff that distance is at most max_hamming.
//
// Why that is the scan's answer: a code within K - 1 bit errors of the word agrees with it on at least one whole chunk (K - 1 errors
// cannot touch K disjoint chunks), hence on that chunk's key, so every code the scan could accept is a candidate, and the scan's own
// choice -- the lowest index at the smallest distance -- is the smallest (distance, index) among them.  Every other candidate is a
// code of the table and therefore no nearer than the scan's best; if that best exceeds max_hamming, no candidate qualifies.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CI_HD __host__ __device__ __forceinline__
#else
#define CI_HD static inline
#endif

// Families with at least this many codes are meant to be decoded through the index.  A floor with a reason, not a break-even: it sits
// above every built-in table (tag36h11: 587 codes) and below the smallest published large family (tagStandard41h12: 2 115), so that
// every handle of built-in families would run exactly what it runs now.  Never below 588.
#define AMDAT_INDEX_MIN_CODES 1024u

#define CI_MAX_CHUNKS 4        // max_hamming <= 3
#define CI_MAX_KEY_BITS 16
#define CI_MAX_CODES (1u << 28)   // a packed candidate carries its index in 28 bits (ci_pack)
#define CI_NONE 0xFFFFFFFFu       // a candidate beyond max_hamming, and the lookup's result when nothing qualifies

// Where the chunks lie and where their tables lie inside the index: one array of 32-bit words, per chunk j its offsets
// (2^keybits[j] + 1 words, relative to the chunk's own index list) at off[j], then its ncodes indices at ids[j].
struct CodeIndexShape {
  uint32_t K;
  uint32_t lo[CI_MAX_CHUNKS];        // the chunk's first bit
  uint32_t keybits[CI_MAX_CHUNKS];   // min(chunk length, 16)
  uint32_t off[CI_MAX_CHUNKS];       // word position of the chunk's offsets
  uint32_t ids[CI_MAX_CHUNKS];       // word position of the chunk's index list
  uint32_t words;                    // the whole index
};

// What a kernel reads: the shape and the table in device memory.
struct CodeIndexDev {
  const uint32_t* table;
  CodeIndexShape shape;
};

CI_HD CodeIndexShape ci_shape(uint32_t nbits, uint32_t max_hamming, uint32_t ncodes) {
  CodeIndexShape s;
  s.K = max_hamming + 1u;
  uint32_t at = 0;
  for (uint32_t j = 0; j < CI_MAX_CHUNKS; j++) {
    s.lo[j] = s.keybits[j] = s.off[j] = s.ids[j] = 0;
    if (j >= s.K) continue;
    const uint32_t lo = j * nbits / s.K, hi = (j + 1u) * nbits / s.K, len = hi - lo;
    s.lo[j] = lo;
    s.keybits[j] = len < CI_MAX_KEY_BITS ? len : CI_MAX_KEY_BITS;
    s.off[j] = at;
    s.ids[j] = at + (1u << s.keybits[j]) + 1u;
    at = s.ids[j] + ncodes;
  }
  s.words = at;
  return s;
}

// The key of a word on the chunk that starts at bit `lo` (lo < 64 whenever the chunk has bits; a chunk without bits has key 0).
CI_HD uint32_t ci_key(uint64_t w, uint32_t lo, uint32_t keybits) {
  return (uint32_t)(w >> lo) & ((1u << keybits) - 1u);
}

CI_HD int ci_popcount64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(x);
#else
  return __builtin_popcountll(x);
#endif
}

// One candidate as one integer, smaller = preferred: the rotation, then the distance, then the index.  CI_NONE beyond max_hamming
// (max_hamming <= 3: the distance takes two bits; index < CI_MAX_CODES - 1 keeps every packed value below CI_NONE).
CI_HD uint32_t ci_pack(uint32_t rotation, int hd, uint32_t index, int max_hamming) {
  return hd <= max_hamming ? (rotation << 30) | ((uint32_t)hd << 28) | index : CI_NONE;
}
CI_HD uint32_t ci_packed_rotation(uint32_t p) { return p >> 30; }
CI_HD uint32_t ci_packed_hamming(uint32_t p) { return (p >> 28) & 3u; }
CI_HD uint32_t ci_packed_index(uint32_t p) { return p & (CI_MAX_CODES - 1u); }

// (host only) The index of `codes` into table[shape.words]: a counting sort per chunk, so the indices of a bucket ascend.
static inline void ci_build(const uint64_t* codes, uint32_t ncodes, const CodeIndexShape& s, uint32_t* table) {
  for (uint32_t j = 0; j < s.K; j++) {
    uint32_t* const off = table + s.off[j];
    uint32_t* const ids = table + s.ids[j];
    const uint32_t nkeys = 1u << s.keybits[j];
    for (uint32_t k = 0; k <= nkeys; k++) off[k] = 0;
    for (uint32_t i = 0; i < ncodes; i++) off[ci_key(codes[i], s.lo[j], s.keybits[j]) + 1u]++;
    for (uint32_t k = 0; k < nkeys; k++) off[k + 1u] += off[k];   // off[k] = start of bucket k
    for (uint32_t k = nkeys; k > 0; k--) off[k] = off[k - 1u];    // moved up by one: off[k + 1] is bucket k's cursor, at its start
    off[0] = 0;
    for (uint32_t i = 0; i < ncodes; i++) ids[off[ci_key(codes[i], s.lo[j], s.keybits[j]) + 1u]++] = i;
    // every cursor has reached its bucket's end, the next bucket's start: off[] is the offsets table again
  }
}

// The lookup of the words of the four rotations, one candidate after the other (a wave's lanes would take them 64 at a time):
// the smallest packed candidate, CI_NONE if none is within max_hamming.
CI_HD uint32_t ci_lookup(const uint32_t* table, const CodeIndexShape& s, const uint64_t* codes, const uint64_t words[4], int max_hamming) {
  uint32_t best = CI_NONE;
  for (uint32_t r = 0; r < 4; r++) {
    for (uint32_t j = 0; j < s.K; j++) {
      const uint32_t* const off = table + s.off[j] + ci_key(words[r], s.lo[j], s.keybits[j]);
      for (uint32_t c = off[0]; c < off[1]; c++) {
        const uint32_t i = table[s.ids[j] + c];
        const uint32_t p = ci_pack(r, ci_popcount64(words[r] ^ codes[i]), i, max_hamming);
        if (p < best) best = p;
      }
    }
  }
  return best;
}
