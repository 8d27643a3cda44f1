// csrc/code_index.h under a host compiler (tests/test_decode_lookup_cpu.py): builds a family's code index and looks words up through
// it, with nothing but the header's own lines.
//
//   code_index_driver <in> <out>
//
// <in>, 64-bit little-endian words: nbits, max_hamming, ncodes, nwords, the codes, then per word its four rotations.
// <out>, 32-bit words: AMDAT_INDEX_MIN_CODES, the shape (K, lo[4], keybits[4], off[4], ids[4], words), the index, then per word the
// packed result of ci_lookup followed by its unpacked rotation, hamming distance and index (zeros for CI_NONE).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../isaac_ros_apriltag_amd/csrc/code_index.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 2;
  uint64_t head[4];
  if (fread(head, 8, 4, in) != 4) { fclose(in); return 2; }
  const uint32_t nbits = (uint32_t)head[0], max_hamming = (uint32_t)head[1], ncodes = (uint32_t)head[2], nwords = (uint32_t)head[3];
  if (nbits == 0 || nbits > 64 || max_hamming > 3 || ncodes == 0 || ncodes >= CI_MAX_CODES - 1u) { fclose(in); return 2; }
  std::vector<uint64_t> codes(ncodes), words((size_t)nwords * 4);
  const bool read_ok = fread(codes.data(), 8, ncodes, in) == ncodes && fread(words.data(), 8, words.size(), in) == words.size();
  fclose(in);
  if (!read_ok) return 2;

  const CodeIndexShape s = ci_shape(nbits, max_hamming, ncodes);
  std::vector<uint32_t> table(s.words);
  ci_build(codes.data(), ncodes, s, table.data());

  std::vector<uint32_t> out;
  out.push_back(AMDAT_INDEX_MIN_CODES);
  out.push_back(s.K);
  for (int j = 0; j < CI_MAX_CHUNKS; j++) out.push_back(s.lo[j]);
  for (int j = 0; j < CI_MAX_CHUNKS; j++) out.push_back(s.keybits[j]);
  for (int j = 0; j < CI_MAX_CHUNKS; j++) out.push_back(s.off[j]);
  for (int j = 0; j < CI_MAX_CHUNKS; j++) out.push_back(s.ids[j]);
  out.push_back(s.words);
  out.insert(out.end(), table.begin(), table.end());
  for (uint32_t i = 0; i < nwords; i++) {
    const uint32_t p = ci_lookup(table.data(), s, codes.data(), &words[(size_t)i * 4], (int)max_hamming);
    out.push_back(p);
    out.push_back(p == CI_NONE ? 0u : ci_packed_rotation(p));
    out.push_back(p == CI_NONE ? 0u : ci_packed_hamming(p));
    out.push_back(p == CI_NONE ? 0u : ci_packed_index(p));
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const bool write_ok = fwrite(out.data(), 4, out.size(), o) == out.size();
  return (fclose(o) == 0 && write_ok) ? 0 : 2;
}
