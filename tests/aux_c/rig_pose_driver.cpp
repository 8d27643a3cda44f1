// Host driver of csrc/rig_pose.h for tests/test_rig_bundles_cpu.py: the definition of the rig pose compiled by g++
// (-ffp-contract=off), as a shared object that Python calls, and -- with -DRIG_POSE_MAIN -- as a program of its own for the
// sanitizer run.
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../isaac_ros_apriltag_amd/csrc/rig_pose.h"

extern "C" {

// Slot s < nobs: pix8 + 8 s the corners (u0, v0, u1, v1, ...), obj12 + 12 s the member's corners, cam17 + 17 s the observation's camera
// (fx, fy, cx, cy, skew, Rc row-major, tc), Rh + 9 s, th + 3 s the record's homography pose, Rm + 9 s, tm + 3 s the member's pose.
// out->seed comes back as the seed's slot.
int rig_pose_probe(uint32_t nobs, const double* pix8, const double* obj12, const double* cam17, const double* Rh, const double* th,
                   const double* Rm, const double* tm, uint32_t iterations, amdAprilTagsRigBundlePose_t* out) {
  if (nobs < 1 || nobs > RG_SLOTS) return 1;
  std::vector<double> pix(4 * RG_SLOTS * 2, 0.0), obj(4 * RG_SLOTS * 3, 0.0);
  memcpy(pix.data(), pix8, sizeof(double) * 8 * nobs);
  memcpy(obj.data(), obj12, sizeof(double) * 12 * nobs);
  std::vector<RigCam> cams(RG_SLOTS);
  for (uint32_t s = 0; s < RG_SLOTS; s++) {   // (an unused slot takes slot 0's camera and contributes nothing)
    const double* c = cam17 + 17 * (s < nobs ? s : 0);
    RigCam& k = cams[s];
    k.fx = c[0]; k.fy = c[1]; k.cx = c[2]; k.cy = c[3]; k.skew = c[4];
    for (int e = 0; e < 9; e++) k.R[e] = c[5 + e];
    for (int e = 0; e < 3; e++) k.t[e] = c[14 + e];
  }
  memset(out, 0, sizeof(*out));
  rig_solve_host(nobs, reinterpret_cast<const double (*)[2]>(pix.data()), reinterpret_cast<const double (*)[3]>(obj.data()), cams.data(), Rh, th,
                 Rm, tm, iterations, out);
  return 0;
}

uint32_t rig_pose_sizes(uint32_t which) {
  switch (which) {
    case 0: return (uint32_t)sizeof(amdAprilTagsRigBundlePose_t);
    case 1: return (uint32_t)sizeof(amdAprilTagsRigCamera_t);
    case 2: return (uint32_t)sizeof(amdAprilTagsRigSlot_t);
    case 3: return AMDAT_MAX_RIG_OBSERVATIONS;
    case 4: return AMDAT_MAX_RIG_CAMERAS;
    case 5: return RIG_SLOT_CUT;
    default: return 0;
  }
}

}  // extern "C"

#ifdef RIG_POSE_MAIN
// One tag seen by two cameras 0.2 m apart (two observations), one and two hundred iterations, and corners that are not numbers:
// every path of the header once, under the sanitizers.
int main(void) {
  int bad = 0;
  const double obj[24] = {-0.03, 0.03, 0, 0.03, 0.03, 0, 0.03, -0.03, 0, -0.03, -0.03, 0, -0.03, 0.03, 0, 0.03, 0.03, 0, 0.03, -0.03, 0, -0.03, -0.03, 0};
  const double Rt[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1}, tt[3] = {0.01, 0.02, 0.6};
  double cam[34] = {600, 600, 320, 240, 0.5, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, 0, 0, 610, 605, 318, 242, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, -0.1, 0, 0};
  double pix[16], Rh[18], th[6], Rm[18], tm[6];
  for (int s = 0; s < 2; s++) {
    const double* c = cam + 17 * s;
    for (int k = 0; k < 4; k++) {
      const double* P = obj + 12 * s + 3 * k;
      const double x = Rt[0] * P[0] + Rt[1] * P[1] + Rt[2] * P[2] + tt[0] + c[14], y = Rt[3] * P[0] + Rt[4] * P[1] + Rt[5] * P[2] + tt[1],
                   z = Rt[6] * P[0] + Rt[7] * P[1] + Rt[8] * P[2] + tt[2];
      pix[8 * s + 2 * k] = c[0] * x / z + c[4] * y / z + c[2] + 0.2 * (k & 1);
      pix[8 * s + 2 * k + 1] = c[1] * y / z + c[3] - 0.1 * (k >> 1);
    }
    memcpy(Rh + 9 * s, Rt, sizeof(Rt));
    for (int i = 0; i < 3; i++) th[3 * s + i] = tt[i] + c[14 + i];
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    memcpy(Rm + 9 * s, I, sizeof(I));
    memset(tm + 3 * s, 0, sizeof(double) * 3);
  }
  amdAprilTagsRigBundlePose_t o;
  const uint32_t iters[3] = {1u, 50u, PR_MAX_ITERATIONS};
  for (uint32_t nobs = 1; nobs <= 2; nobs++)
    for (int i = 0; i < 3; i++) {
      memset(&o, 0xff, sizeof(o));
      if (rig_pose_probe(nobs, pix, obj, cam, Rh, th, Rm, tm, iters[i], &o)) bad++;
      if (o.status != AMDAT_BUNDLE_SOLVED || o.chosen > 1u || o.seed >= nobs || !(o.err <= o.err_alt)) bad++;
      printf("%u observations, %u iterations: status %u chosen %u seed %u err %.3e err_alt %.3e sq_err_sum %.3e t %.4f %.4f %.4f\n", nobs, iters[i],
             o.status, o.chosen, o.seed, o.err, o.err_alt, o.sq_err_sum, o.t[0], o.t[1], o.t[2]);
    }
  double same[16];
  for (int k = 0; k < 16; k++) same[k] = nan("");
  memset(&o, 0xff, sizeof(o));
  rig_pose_probe(2, same, obj, cam, Rh, th, Rm, tm, 50u, &o);
  printf("corners that are not numbers: status %u chosen %u\n", o.status, o.chosen);
  if (o.status != AMDAT_BUNDLE_DEGENERATE || o.chosen != 0u || o.err_alt != 0.0 || o.sq_err_sum != 0.0 || o.R_alt[0] != 0.0) bad++;
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
#endif
