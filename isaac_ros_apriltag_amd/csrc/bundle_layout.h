// bundle_layout.h -- the host side of amdAprilTagsSetBundles: what the call refuses, the normalisation constants of every bundle
//  and the (family, id) -> member lookup table k_bundle_pose reads.  Plain C++ without HIP, so that
// tests/test_bundles_cpu.py compiles it on the host (tests/aux_c/bundle_layout_driver.cpp); the device-side structs live here too.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/apriltag_amd.h"

#define BUNDLE_MAX_FAMILIES 4   // AT_MAX_FAMILIES (common.h)

// One member as the kernel reads it: the tag centre on the board plane, half its edge, and the bundle it belongs to.
struct BundleMemberDev {
  double x, y, hs;
  uint32_t bundle;
  uint32_t pad;
};
// One bundle: the normalisation centre and scale, and its gates.
struct BundleDev {
  double mx, my, sc;
  float min_decision_margin;
  int32_t max_hamming;
  uint32_t min_tags;
  uint32_t nmembers;
};
// The block at the head of the device layout.  table[fam_base[f] + id] is 1 + the member's index in the member array, 0 for a tag
// that belongs to no bundle; the table covers every code of every family of the handle, so its size never changes.
struct BundleHeadDev {
  uint32_t nbundles, nmembers;
  uint32_t fam_base[BUNDLE_MAX_FAMILIES], fam_ncodes[BUNDLE_MAX_FAMILIES];
  BundleDev b[AMDAT_MAX_BUNDLES];
};
// A bundle record in the pinned host block: the public record and the stamp of the launch that wrote it, stored last.
struct BundlePoseRec {
  amdAprilTagsBundlePose_t pose;
  uint32_t seq;
  uint32_t pad;
};

struct BundleLayout {
  BundleHeadDev head;
  std::vector<BundleMemberDev> members;
  std::vector<uint16_t> table;
};

inline uint32_t bundle_table_entries(uint32_t nfam, const uint32_t* fam_ncodes) {
  uint32_t n = 0;
  for (uint32_t f = 0; f < nfam; f++) n += fam_ncodes[f];
  return n;
}

// Validates `bundles` against the handle's families (nfam of them, fam_ncodes[f] codes each) and fills `out`; AMDAT_INVALID_ARGUMENT
// for everything include/apriltag_amd.h lists, with `out` in an unspecified state.  nbundles = 0 gives the empty layout.
inline int bundle_layout_build(uint32_t nfam, const uint32_t* fam_ncodes, uint32_t nbundles, const amdAprilTagsBundle_t* bundles,
                               BundleLayout* out) {
  if (!out || !fam_ncodes || nfam < 1 || nfam > BUNDLE_MAX_FAMILIES) return AMDAT_INVALID_ARGUMENT;
  if (nbundles > AMDAT_MAX_BUNDLES || (nbundles && !bundles)) return AMDAT_INVALID_ARGUMENT;
  memset(&out->head, 0, sizeof(out->head));
  out->members.clear();
  out->head.nbundles = nbundles;
  uint32_t base = 0;
  for (uint32_t f = 0; f < nfam; f++) { out->head.fam_base[f] = base; out->head.fam_ncodes[f] = fam_ncodes[f]; base += fam_ncodes[f]; }
  out->table.assign(base, 0);
  uint64_t total = 0;
  for (uint32_t b = 0; b < nbundles; b++) {
    if (!bundles[b].members || bundles[b].nmembers == 0) return AMDAT_INVALID_ARGUMENT;
    total += bundles[b].nmembers;
    if (total > AMDAT_MAX_BUNDLE_MEMBERS) return AMDAT_INVALID_ARGUMENT;
  }
  for (uint32_t b = 0; b < nbundles; b++) {
    const amdAprilTagsBundle_t& B = bundles[b];
    if (B.min_tags == 0 || !memchr(B.name, 0, sizeof(B.name))) return AMDAT_INVALID_ARGUMENT;
    // mx, my: the sequential means of the member centres
    double sx = 0.0, sy = 0.0;
    for (uint32_t i = 0; i < B.nmembers; i++) {
      const amdAprilTagsBundleMember_t& m = B.members[i];
      if (m.family_index >= nfam || m.id >= fam_ncodes[m.family_index]) return AMDAT_INVALID_ARGUMENT;
      if (!isfinite(m.x) || !isfinite(m.y) || !isfinite(m.size) || !(m.size > 0.0)) return AMDAT_INVALID_ARGUMENT;
      uint16_t& slot = out->table[out->head.fam_base[m.family_index] + m.id];
      if (slot) return AMDAT_INVALID_ARGUMENT;   // named twice, within this bundle or in an earlier one
      out->members.push_back({m.x, m.y, m.size / 2.0, b, 0u});
      slot = (uint16_t)out->members.size();
      sx = sx + m.x;
      sy = sy + m.y;
    }
    const double mx = sx / (double)B.nmembers, my = sy / (double)B.nmembers;
    // sc: the largest extent of a member from the centre, along either axis, out to its border
    double sc = 0.0;
    for (uint32_t i = 0; i < B.nmembers; i++) {
      const amdAprilTagsBundleMember_t& m = B.members[i];
      const double ax = fabs(m.x - mx), ay = fabs(m.y - my);
      const double e = (ax > ay ? ax : ay) + m.size / 2.0;
      if (e > sc) sc = e;
    }
    if (!isfinite(mx) || !isfinite(my) || !isfinite(sc)) return AMDAT_INVALID_ARGUMENT;   // (finite coordinates whose sums are not)
    BundleDev& d = out->head.b[b];
    d.mx = mx; d.my = my; d.sc = sc;
    d.min_decision_margin = B.min_decision_margin;
    d.max_hamming = B.max_hamming > 0x7FFFFFFEu ? 0x7FFFFFFE : (int32_t)B.max_hamming;   // (below INT32_MAX, the hamming of an invalid undistorted record: DESIGN.md section 7h)
    d.min_tags = B.min_tags;
    d.nmembers = B.nmembers;
  }
  out->head.nmembers = (uint32_t)out->members.size();
  return AMDAT_SUCCESS;
}
