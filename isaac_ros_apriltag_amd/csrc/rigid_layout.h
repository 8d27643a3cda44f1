// rigid_layout.h -- the host side of amdAprilTagsSetBundlesEx, the sibling of bundle_layout.h: what the call refuses, the four
// bundle-frame corners of every member (the object points of the iteration, computed once, here) and the
// (family, id) -> member lookup table k_bundle_rigid reads.  Plain C++ without HIP, so that tests/test_rigid_bundles_cpu.py compiles
// it on the host (tests/aux_c/rigid_pose_driver.cpp); the device-side structs live here too.  One IEEE operation per operator
// (-ffp-contract=off).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/apriltag_amd.h"
#include "bundle_layout.h"
#include "tools_hooks.h"

#define RIGID_MAX_MEMBERS (AMDAT_MAX_BUNDLES * AMDAT_MAX_RIGID_BUNDLE_MEMBERS)   // over all bundles of a handle

// One member as the kernel reads it: its four corners in the bundle frame (corner k is the record's p[k]), its pose in the bundle
// frame (the seed's start is composed with its inverse), its edge, and the bundle it belongs to.
struct RigidMemberDev {
  double P[4][3];
  double R[9], t[3];
  double size;
  uint32_t bundle;
  uint32_t pad;
};
// One bundle: its gates (bundle_classify reads max_hamming and min_decision_margin) and its iteration count.
struct RigidBundleDev {
  float min_decision_margin;
  int32_t max_hamming;
  uint32_t min_tags;
  uint32_t nmembers;
  uint32_t iterations;
  uint32_t pad;
};
// The block at the head of the device layout; the table is BundleHeadDev's.
struct RigidHeadDev {
  uint32_t nbundles, nmembers;
  uint32_t fam_base[BUNDLE_MAX_FAMILIES], fam_ncodes[BUNDLE_MAX_FAMILIES];
  RigidBundleDev b[AMDAT_MAX_BUNDLES];
};
// A rigid bundle record in the pinned host block: the public record and the stamp of the launch that wrote it, stored last.
struct RigidPoseRec {
  amdAprilTagsBundlePoseEx_t pose;
  uint32_t seq;
  uint32_t pad;
};

struct RigidLayout {
  RigidHeadDev head;
  std::vector<RigidMemberDev> members;
  std::vector<uint16_t> table;
};

// Whether R (row-major) is a rotation within the header's bound: max |R R^T - I| <= 1e-6 and det R > 0.
inline bool rigid_is_rotation(const double* R) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double d = ((R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2]) - (i == j ? 1.0 : 0.0);
      if (!(fabs(d) <= 1e-6)) return false;
    }
  const double det = (R[0] * (R[4] * R[8] - R[5] * R[7]) + R[1] * (R[5] * R[6] - R[3] * R[8])) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  return det > 0.0;
}

// Corner k of a member in the bundle frame: R (size / 2 * c_k.x, size / 2 * c_k.y, 0) + t.
inline void rigid_member_corner(const double* R, const double* t, double size, int k, double* P) {
  const double ckx = (k == 0 || k == 3) ? -1.0 : 1.0, cky = k < 2 ? 1.0 : -1.0;
  const double hs = size / 2.0;
  const double ax = hs * ckx, ay = hs * cky;
  for (int i = 0; i < 3; i++) P[i] = (RIGID_MEMBER_R(R, 3 * i) * ax + RIGID_MEMBER_R(R, 3 * i + 1) * ay) + t[i];
}

// Validates `bundles` against the handle's families and fills `out`; AMDAT_INVALID_ARGUMENT for everything include/apriltag_amd.h
// lists, with `out` in an unspecified state.  nbundles = 0 gives the empty layout.
inline int rigid_layout_build(uint32_t nfam, const uint32_t* fam_ncodes, uint32_t nbundles, const amdAprilTagsBundleEx_t* bundles,
                              RigidLayout* out) {
  if (!out || !fam_ncodes || nfam < 1 || nfam > BUNDLE_MAX_FAMILIES) return AMDAT_INVALID_ARGUMENT;
  if (nbundles > AMDAT_MAX_BUNDLES || (nbundles && !bundles)) return AMDAT_INVALID_ARGUMENT;
  memset(&out->head, 0, sizeof(out->head));
  out->members.clear();
  out->head.nbundles = nbundles;
  uint32_t base = 0;
  for (uint32_t f = 0; f < nfam; f++) { out->head.fam_base[f] = base; out->head.fam_ncodes[f] = fam_ncodes[f]; base += fam_ncodes[f]; }
  out->table.assign(base, 0);
  for (uint32_t b = 0; b < nbundles; b++)
    if (!bundles[b].members || bundles[b].nmembers == 0 || bundles[b].nmembers > AMDAT_MAX_RIGID_BUNDLE_MEMBERS) return AMDAT_INVALID_ARGUMENT;
  for (uint32_t b = 0; b < nbundles; b++) {
    const amdAprilTagsBundleEx_t& B = bundles[b];
    if (B.min_tags == 0 || !memchr(B.name, 0, sizeof(B.name))) return AMDAT_INVALID_ARGUMENT;
    if (B.iterations == 0 || B.iterations > AMDAT_MAX_POSE_ITERATIONS) return AMDAT_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < B.nmembers; i++) {
      const amdAprilTagsBundleMemberEx_t& m = B.members[i];
      if (m.family_index >= nfam || m.id >= fam_ncodes[m.family_index]) return AMDAT_INVALID_ARGUMENT;
      if (!isfinite(m.size) || !(m.size > 0.0)) return AMDAT_INVALID_ARGUMENT;
      for (int e = 0; e < 9; e++) if (!isfinite(m.R[e])) return AMDAT_INVALID_ARGUMENT;
      for (int e = 0; e < 3; e++) if (!isfinite(m.t[e])) return AMDAT_INVALID_ARGUMENT;
      if (!rigid_is_rotation(m.R)) return AMDAT_INVALID_ARGUMENT;
      uint16_t& slot = out->table[out->head.fam_base[m.family_index] + m.id];
      if (slot) return AMDAT_INVALID_ARGUMENT;   // named twice, within this bundle or in an earlier one
      RigidMemberDev d;
      memset(&d, 0, sizeof(d));
      for (int k = 0; k < 4; k++) {
        rigid_member_corner(m.R, m.t, m.size, k, d.P[k]);
        for (int e = 0; e < 3; e++) if (!isfinite(d.P[k][e])) return AMDAT_INVALID_ARGUMENT;   // (finite entries whose sums are not)
      }
      for (int e = 0; e < 9; e++) d.R[e] = m.R[e];
      for (int e = 0; e < 3; e++) d.t[e] = m.t[e];
      d.size = m.size;
      d.bundle = b;
      out->members.push_back(d);
      slot = (uint16_t)out->members.size();
    }
    RigidBundleDev& d = out->head.b[b];
    d.min_decision_margin = B.min_decision_margin;
    d.max_hamming = B.max_hamming > 0x7FFFFFFEu ? 0x7FFFFFFE : (int32_t)B.max_hamming;   // (below INT32_MAX, the hamming of an invalid undistorted record: DESIGN.md section 7h)
    d.min_tags = B.min_tags;
    d.nmembers = B.nmembers;
    d.iterations = B.iterations;
  }
  out->head.nmembers = (uint32_t)out->members.size();
  return AMDAT_SUCCESS;
}
