// Host driver of csrc/rigid_pose.h and csrc/rigid_layout.h for tests/test_rigid_bundles_cpu.py: the definition of the rigid bundle
// pose compiled by g++ (-ffp-contract=off), as a shared object that Python calls, and -- with -DRIGID_POSE_MAIN -- as a program of its
// own for the sanitizer run.
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../isaac_ros_apriltag_amd/csrc/rigid_layout.h"
#include "../../isaac_ros_apriltag_amd/csrc/rigid_pose.h"

extern "C" {

// Slot s < ntags: pix8 + 8 s the corners (u0, v0, u1, v1, ...), obj12 + 12 s the member's corners, Rh + 9 s, th + 3 s the record's
// homography pose, Rm + 9 s, tm + 3 s the member's pose.  out->seed comes back as the seed's slot.
int rigid_pose_probe(uint32_t ntags, const double* pix8, const double* obj12, const double* Rh, const double* th, const double* Rm,
                     const double* tm, double fx, double fy, double cx, double cy, double skew, uint32_t iterations,
                     amdAprilTagsBundlePoseEx_t* out) {
  if (ntags < 1 || ntags > RG_SLOTS) return 1;
  std::vector<double> pix(4 * RG_SLOTS * 2, 0.0), obj(4 * RG_SLOTS * 3, 0.0);
  memcpy(pix.data(), pix8, sizeof(double) * 8 * ntags);
  memcpy(obj.data(), obj12, sizeof(double) * 12 * ntags);
  memset(out, 0, sizeof(*out));
  rg_solve_host(ntags, reinterpret_cast<const double (*)[2]>(pix.data()), reinterpret_cast<const double (*)[3]>(obj.data()), Rh, th, Rm, tm, fx,
                fy, cx, cy, skew, iterations, out);
  return 0;
}

int rigid_polar_probe(const double* M, double* Rn) { return rg_polar(M, Rn) ? 1 : 0; }

// rigid_layout_build's return code; on success the members' corners (12 doubles each, in layout order) and their number.
int rigid_layout_probe(uint32_t nfam, const uint32_t* ncodes, uint32_t nbundles, const amdAprilTagsBundleEx_t* bundles, double* corners,
                       uint32_t capacity, uint32_t* nmembers) {
  RigidLayout L;
  const int rc = rigid_layout_build(nfam, ncodes, nbundles, bundles, &L);
  if (rc) return rc;
  if (nmembers) *nmembers = (uint32_t)L.members.size();
  for (size_t i = 0; i < L.members.size() && i < capacity; i++) memcpy(corners + 12 * i, L.members[i].P, sizeof(double) * 12);
  return 0;
}

uint32_t rigid_pose_sizes(uint32_t which) {
  switch (which) {
    case 0: return (uint32_t)sizeof(amdAprilTagsBundlePoseEx_t);
    case 1: return (uint32_t)sizeof(amdAprilTagsBundleEx_t);
    case 2: return (uint32_t)sizeof(amdAprilTagsBundleMemberEx_t);
    case 3: return RG_SLOTS;
    case 4: return RG_JACOBI_SWEEPS;
    case 5: return (uint32_t)sizeof(RigidMemberDev);
    default: return 0;
  }
}

}  // extern "C"

#ifdef RIGID_POSE_MAIN
// Two tags at right angles seen obliquely (a non-coplanar set), one of them alone (a coplanar set), one and two hundred iterations, a
// layout with a refused member, and the degenerate record (corners that are not numbers): every path of the two headers once, under
// the sanitizers.
int main(void) {
  int bad = 0;
  amdAprilTagsBundleMemberEx_t mem[2];
  memset(mem, 0, sizeof(mem));
  const double Ra[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1}, Rb[9] = {0, 0, -1, 1, 0, 0, 0, -1, 0};
  mem[0].id = 0; mem[0].size = 0.06; memcpy(mem[0].R, Ra, sizeof(Ra)); mem[0].t[0] = -0.05; mem[0].t[1] = -0.05;
  mem[1].id = 1; mem[1].size = 0.06; memcpy(mem[1].R, Rb, sizeof(Rb)); mem[1].t[1] = -0.05; mem[1].t[2] = -0.05;
  amdAprilTagsBundleEx_t B;
  memset(&B, 0, sizeof(B));
  B.members = mem; B.nmembers = 2; B.max_hamming = 2; B.min_tags = 1; B.iterations = 50;
  strcpy(B.name, "corner");
  const uint32_t ncodes[1] = {587};
  double corners[24];
  uint32_t nm = 0;
  if (rigid_layout_probe(1, ncodes, 1, &B, corners, 2, &nm) != 0 || nm != 2) bad++;
  amdAprilTagsBundleMemberEx_t skewed = mem[0];
  skewed.R[1] = 1e-3;
  amdAprilTagsBundleEx_t Bs = B;
  Bs.members = &skewed; Bs.nmembers = 1;
  if (rigid_layout_probe(1, ncodes, 1, &Bs, corners, 2, &nm) != AMDAT_INVALID_ARGUMENT) bad++;
  if (rigid_layout_probe(1, ncodes, 1, &B, corners, 2, &nm) != 0) bad++;
  // the bundle's true pose: looking at the corner along its diagonal
  const double Rt[9] = {-0.70710678118654757, 0.70710678118654757, 0.0, 0.40824829046386307, 0.40824829046386307, -0.81649658092772615,
                        -0.57735026918962584, -0.57735026918962584, -0.57735026918962584};
  const double tt[3] = {0.01, 0.02, 0.6};
  double pix[16], Rh[18], th[6], Rm[18], tm[6];
  for (int s = 0; s < 2; s++) {
    for (int k = 0; k < 4; k++) {
      const double* P = corners + 12 * s + 3 * k;
      const double x = Rt[0] * P[0] + Rt[1] * P[1] + Rt[2] * P[2] + tt[0], y = Rt[3] * P[0] + Rt[4] * P[1] + Rt[5] * P[2] + tt[1],
                   z = Rt[6] * P[0] + Rt[7] * P[1] + Rt[8] * P[2] + tt[2];
      pix[8 * s + 2 * k] = 600.0 * x / z + 0.5 * y / z + 320.0 + 0.2 * (k & 1);
      pix[8 * s + 2 * k + 1] = 600.0 * y / z + 240.0 - 0.1 * (k >> 1);
    }
    // the tag's pose in the camera: Rt Rm, Rt tm + tt (stands in for the homography pose)
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) Rh[9 * s + 3 * i + j] = Rt[3 * i] * mem[s].R[j] + Rt[3 * i + 1] * mem[s].R[3 + j] + Rt[3 * i + 2] * mem[s].R[6 + j];
      th[3 * s + i] = Rt[3 * i] * mem[s].t[0] + Rt[3 * i + 1] * mem[s].t[1] + Rt[3 * i + 2] * mem[s].t[2] + tt[i];
    }
    memcpy(Rm + 9 * s, mem[s].R, sizeof(Ra));
    memcpy(tm + 3 * s, mem[s].t, sizeof(double) * 3);
  }
  amdAprilTagsBundlePoseEx_t o;
  const uint32_t iters[3] = {1u, 50u, PR_MAX_ITERATIONS};
  for (uint32_t ntags = 1; ntags <= 2; ntags++)
    for (int i = 0; i < 3; i++) {
      memset(&o, 0xff, sizeof(o));
      if (rigid_pose_probe(ntags, pix, corners, Rh, th, Rm, tm, 600.0, 600.0, 320.0, 240.0, 0.5, iters[i], &o)) bad++;
      if (o.status != AMDAT_BUNDLE_SOLVED || o.chosen > 1u || o.seed >= ntags || !(o.err <= o.err_alt)) bad++;
      printf("%u tags, %u iterations: status %u chosen %u seed %u err %.3e err_alt %.3e sq_err_sum %.3e\n", ntags, iters[i], o.status, o.chosen,
             o.seed, o.err, o.err_alt, o.sq_err_sum);
    }
  double same[16];
  for (int k = 0; k < 16; k++) same[k] = nan("");
  memset(&o, 0xff, sizeof(o));
  rigid_pose_probe(2, same, corners, Rh, th, Rm, tm, 600.0, 600.0, 320.0, 240.0, 0.0, 50u, &o);
  printf("corners that are not numbers: status %u chosen %u\n", o.status, o.chosen);
  if (o.status != AMDAT_BUNDLE_DEGENERATE || o.chosen != 0u || o.err_alt != 0.0 || o.sq_err_sum != 0.0 || o.R_alt[0] != 0.0) bad++;
  const double Mz[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double Rn[9];
  if (rigid_polar_probe(Mz, Rn) != 0) bad++;
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
#endif
