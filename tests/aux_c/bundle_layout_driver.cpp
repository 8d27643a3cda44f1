// Host driver of isaac_ros_apriltag_amd/csrc/bundle_layout.h for tests/test_bundles_cpu.py.  Compiled twice: as a small shared library
// (the extern "C" entry below, called through ctypes) and, with -DBUNDLE_LAYOUT_MAIN, as a stand-alone program that drives the same code
// through its refusals and its largest layout under -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>

#include "../../isaac_ros_apriltag_amd/csrc/bundle_layout.h"

// Builds the layout; on success norm[3 b ..] = mx, my, sc of bundle b, member_out[4 m ..] = x, y, hs, bundle of member m, table_out the
// lookup table (table_cap entries of room), counts[0] = members, counts[1] = table entries.
extern "C" int bundle_layout_probe(uint32_t nfam, const uint32_t* fam_ncodes, uint32_t nbundles, const amdAprilTagsBundle_t* bundles,
                                   double* norm, double* member_out, uint16_t* table_out, uint32_t table_cap, uint32_t* counts) {
  BundleLayout L;
  const int rc = bundle_layout_build(nfam, fam_ncodes, nbundles, bundles, &L);
  if (rc) return rc;
  if (L.table.size() > table_cap) return -1;
  for (uint32_t b = 0; b < L.head.nbundles; b++) { norm[3 * b] = L.head.b[b].mx; norm[3 * b + 1] = L.head.b[b].my; norm[3 * b + 2] = L.head.b[b].sc; }
  for (size_t m = 0; m < L.members.size(); m++) {
    member_out[4 * m] = L.members[m].x; member_out[4 * m + 1] = L.members[m].y; member_out[4 * m + 2] = L.members[m].hs;
    member_out[4 * m + 3] = (double)L.members[m].bundle;
  }
  for (size_t i = 0; i < L.table.size(); i++) table_out[i] = L.table[i];
  counts[0] = (uint32_t)L.members.size();
  counts[1] = (uint32_t)L.table.size();
  return 0;
}

extern "C" uint32_t bundle_layout_sizes(uint32_t which) {
  const uint32_t s[6] = {(uint32_t)sizeof(amdAprilTagsBundleMember_t), (uint32_t)sizeof(amdAprilTagsBundle_t), (uint32_t)sizeof(amdAprilTagsBundlePose_t),
                         (uint32_t)sizeof(BundlePoseRec), (uint32_t)sizeof(BundleMemberDev), (uint32_t)sizeof(BundleHeadDev)};
  return which < 6 ? s[which] : 0;
}

#ifdef BUNDLE_LAYOUT_MAIN
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)
int main(void) {
  const uint32_t ncodes[2] = {587, 35};
  // the largest layout: 8 bundles, 1024 members in all
  std::vector<amdAprilTagsBundleMember_t> mem(1025);
  for (uint32_t i = 0; i < 1025; i++) mem[i] = {i < 587 ? 0u : 1u, i < 587 ? i : (i - 587) % 35, 0.1 * (i % 32), 0.1 * (i / 32), 0.05};
  amdAprilTagsBundle_t B[9] = {};
  for (uint32_t b = 0; b < 9; b++) { B[b].members = &mem[b * 70]; B[b].nmembers = 70; B[b].max_hamming = 2; B[b].min_tags = 1; snprintf(B[b].name, 32, "b%u", b); }
  BundleLayout L;
  CHECK(bundle_layout_build(2, ncodes, 8, B, &L) == AMDAT_SUCCESS && L.members.size() == 560 && L.table.size() == 622);
  CHECK(L.table[0] == 1 && L.table[559] == 560 && L.table[560] == 0);
  CHECK(bundle_layout_build(2, ncodes, 0, nullptr, &L) == AMDAT_SUCCESS && L.members.empty() && L.head.nbundles == 0);
  CHECK(bundle_layout_build(2, ncodes, 9, B, &L) == AMDAT_INVALID_ARGUMENT);          // too many bundles
  CHECK(bundle_layout_build(2, ncodes, 1, nullptr, &L) == AMDAT_INVALID_ARGUMENT);    // null bundles
  CHECK(bundle_layout_build(2, ncodes, 1, B, nullptr) == AMDAT_INVALID_ARGUMENT);
  { amdAprilTagsBundle_t x = B[0]; x.members = nullptr; CHECK(bundle_layout_build(2, ncodes, 1, &x, &L) == AMDAT_INVALID_ARGUMENT); }
  { amdAprilTagsBundle_t x = B[0]; x.nmembers = 0; CHECK(bundle_layout_build(2, ncodes, 1, &x, &L) == AMDAT_INVALID_ARGUMENT); }
  { amdAprilTagsBundle_t x = B[0]; x.min_tags = 0; CHECK(bundle_layout_build(2, ncodes, 1, &x, &L) == AMDAT_INVALID_ARGUMENT); }
  { amdAprilTagsBundle_t x = B[0]; memset(x.name, 'n', 32); CHECK(bundle_layout_build(2, ncodes, 1, &x, &L) == AMDAT_INVALID_ARGUMENT); }
  { amdAprilTagsBundle_t x = B[0]; x.nmembers = 1025; CHECK(bundle_layout_build(2, ncodes, 1, &x, &L) == AMDAT_INVALID_ARGUMENT); }   // members in all
  { amdAprilTagsBundle_t x[2] = {B[0], B[0]}; x[0].nmembers = 600; x[1].members = &mem[600]; x[1].nmembers = 425;
    CHECK(bundle_layout_build(2, ncodes, 2, x, &L) == AMDAT_INVALID_ARGUMENT); }
  { amdAprilTagsBundle_t x[2] = {B[0], B[0]}; CHECK(bundle_layout_build(2, ncodes, 2, x, &L) == AMDAT_INVALID_ARGUMENT); }   // named twice, across bundles
  const amdAprilTagsBundleMember_t ok = {0, 5, 0.0, 0.0, 0.1};
  const double inf = HUGE_VAL, nan = NAN;
  const amdAprilTagsBundleMember_t bad[] = {{2, 5, 0, 0, 0.1}, {0, 587, 0, 0, 0.1}, {1, 35, 0, 0, 0.1}, {0, 5, inf, 0, 0.1}, {0, 5, 0, nan, 0.1},
                                            {0, 5, 0, 0, 0.0}, {0, 5, 0, 0, -0.1}, {0, 5, 0, 0, inf}, {0, 5, 0, 0, nan}};
  for (const auto& m : bad) {
    amdAprilTagsBundleMember_t two[2] = {{0, 4, 1.0, 1.0, 0.1}, m};
    amdAprilTagsBundle_t x = B[0]; x.members = two; x.nmembers = 2;
    CHECK(bundle_layout_build(2, ncodes, 1, &x, &L) == AMDAT_INVALID_ARGUMENT);
  }
  { amdAprilTagsBundleMember_t two[2] = {ok, ok}; amdAprilTagsBundle_t x = B[0]; x.members = two; x.nmembers = 2;
    CHECK(bundle_layout_build(2, ncodes, 1, &x, &L) == AMDAT_INVALID_ARGUMENT); }   // named twice, within a bundle
  { amdAprilTagsBundleMember_t two[2] = {ok, {1, 5, 1.0, 2.0, 0.3}}; amdAprilTagsBundle_t x = B[0]; x.members = two; x.nmembers = 2;
    CHECK(bundle_layout_build(2, ncodes, 1, &x, &L) == AMDAT_SUCCESS && L.table[5] == 1 && L.table[587 + 5] == 2);
    CHECK(L.head.b[0].mx == 0.5 && L.head.b[0].my == 1.0 && L.head.b[0].sc == 1.0 + 0.15); }
  printf("ok\n");
  return 0;
}
#endif
