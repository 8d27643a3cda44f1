// tag_table_driver.cpp -- csrc/tag_table.h under a host compiler (tests/test_tag_table_cpu.py): builds the table of the entries in
// the input file, looks the file's queries up and writes what the header gave.  A program of its own, so that it can be built with
// -fsanitize=address,undefined and run as it stands.
//   input  (32-bit words): num_families, ncodes[4], default size (a double: low word, high word), n entries, q queries,
//                          n x (family_index, id, size as the bits of a float), q x (family, id)
//   output (64-bit words): tt_build's result (0, or 1 where it refused), n, n keys, n sizes (bits of the doubles),
//                          q x (listed, size as the bits of the double); after a refusal nothing follows the first word
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../isaac_ros_apriltag_amd/csrc/tag_table.h"

static uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> in;
  uint32_t w;
  while (fread(&w, 4, 1, f) == 1) in.push_back(w);
  fclose(f);
  if (in.size() < 9) return 2;
  const uint32_t num_families = in[0];
  const uint32_t* ncodes = &in[1];
  double default_size;
  memcpy(&default_size, &in[5], sizeof(default_size));
  const uint32_t n = in[7], q = in[8];
  if (in.size() != 9 + 3 * (size_t)n + 2 * (size_t)q) return 2;
  std::vector<TagTableEntry> entries(n);
  for (uint32_t i = 0; i < n; i++) {
    entries[i].family_index = in[9 + 3 * i];
    entries[i].id = in[10 + 3 * i];
    memcpy(&entries[i].size, &in[11 + 3 * i], sizeof(float));
  }
  // exactly as many slots as a table may have: an entry too many is refused before anything is written
  const uint32_t slots = n < AMDAT_MAX_TAG_ENTRIES ? n : AMDAT_MAX_TAG_ENTRIES;
  std::vector<uint32_t> keys(slots);
  std::vector<double> sizes(slots);
  std::vector<uint64_t> out;
  const int rc = tt_build(num_families, ncodes, n, entries.data(), keys.data(), sizes.data());
  out.push_back(rc ? 1u : 0u);
  if (!rc) {
    out.push_back(n);
    for (uint32_t i = 0; i < n; i++) out.push_back(keys[i]);
    for (uint32_t i = 0; i < n; i++) out.push_back(bits_of(sizes[i]));
    const uint32_t* qs = in.data() + 9 + 3 * (size_t)n;
    for (uint32_t i = 0; i < q; i++) {
      bool listed = false;
      const double s = tt_lookup(keys.data(), sizes.data(), n, qs[2 * i], qs[2 * i + 1], default_size, &listed);
      out.push_back(listed ? 1u : 0u);
      out.push_back(bits_of(s));
    }
  }
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  fwrite(out.data(), 8, out.size(), f);
  fclose(f);
  return 0;
}
