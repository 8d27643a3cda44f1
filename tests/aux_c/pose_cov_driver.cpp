// Host driver of csrc/pose_covariance.h for tests/test_pose_covariance_cpu.py: the definition of the pose covariance compiled by g++
// (-ffp-contract=off), as a shared object that Python calls, and -- with -DPOSE_COV_MAIN -- as a program of its own for the
// sanitizer run.
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../isaac_ros_apriltag_amd/csrc/pose_covariance.h"

extern "C" {

// p8: the four corners (u0, v0, u1, v1, ...); o: the tag's refined record
void pose_cov_tag_probe(const double* p8, double fx, double fy, double cx, double cy, double skew, double tag_size,
                        const amdAprilTagsRefinedPose_t* o, double sigma, amdAprilTagsPoseCovariance_t* out) {
  double p[4][2];
  for (int k = 0; k < 4; k++) { p[k][0] = p8[2 * k]; p[k][1] = p8[2 * k + 1]; }
  pc_tag_record(p, fx, fy, cx, cy, skew, tag_size, o, sigma * sigma, out);
}

// pix: ntags * 8 doubles, obj: ntags * 12 doubles, in slot order; o: the bundle's pose record
void pose_cov_bundle_probe(uint32_t ntags, const double* pix, const double* obj, double fx, double fy, double cx, double cy, double skew,
                           const amdAprilTagsBundlePoseEx_t* o, double sigma, amdAprilTagsPoseCovariance_t* out) {
  static thread_local double P[4 * RG_SLOTS][2], O[4 * RG_SLOTS][3];
  memset(P, 0, sizeof(P));
  memset(O, 0, sizeof(O));
  if (ntags > RG_SLOTS) ntags = RG_SLOTS;
  for (uint32_t j = 0; j < 4 * ntags; j++) {
    P[j][0] = pix[2 * j]; P[j][1] = pix[2 * j + 1];
    O[j][0] = obj[3 * j]; O[j][1] = obj[3 * j + 1]; O[j][2] = obj[3 * j + 2];
  }
  pc_bundle_record(ntags, P, O, fx, fy, cx, cy, skew, o, sigma * sigma, out);
}

uint32_t pose_cov_sizes(uint32_t which) {
  switch (which) {
    case 0: return (uint32_t)sizeof(amdAprilTagsPoseCovariance_t);
    case 1: return (uint32_t)offsetof(amdAprilTagsPoseCovariance_t, valid);
    default: return 0;
  }
}

}  // extern "C"

#ifdef POSE_COV_MAIN
// A tag seen obliquely under a skewed camera with an alternative, a record without one, four equal pixels, a NaN in the pose, and a
// two-tag bundle: every path of the header once, under the sanitizers.
int main(void) {
  amdAprilTagsRefinedPose_t o;
  memset(&o, 0, sizeof(o));
  const double R[9] = {0.8, -0.1, 0.59, 0.05, 0.99, 0.1, -0.6, -0.05, 0.8};
  const double Ra[9] = {0.8, 0.1, -0.59, -0.05, 0.99, 0.1, 0.6, -0.05, 0.8};
  const double t[3] = {0.05, -0.02, 0.9};
  for (int i = 0; i < 9; i++) { o.R[i] = R[i]; o.R_alt[i] = Ra[i]; }
  for (int i = 0; i < 3; i++) { o.t[i] = t[i]; o.t_alt[i] = t[i]; }
  o.status = AMDAT_POSE_REFINED;
  double p[8];
  const double s = 0.05, c[4][2] = {{-1, 1}, {1, 1}, {1, -1}, {-1, -1}};
  for (int k = 0; k < 4; k++) {
    const double x = R[0] * s * c[k][0] + R[1] * s * c[k][1] + t[0], y = R[3] * s * c[k][0] + R[4] * s * c[k][1] + t[1],
                 z = R[6] * s * c[k][0] + R[7] * s * c[k][1] + t[2];
    p[2 * k] = (600.0 * x + 0.5 * y) / z + 320.0 + 0.3 * c[k][0];
    p[2 * k + 1] = 600.0 * y / z + 240.0 - 0.2 * c[k][1];
  }
  int bad = 0;
  amdAprilTagsPoseCovariance_t out;
  memset(&out, 0xff, sizeof(out));
  pose_cov_tag_probe(p, 600.0, 600.0, 320.0, 240.0, 0.5, 0.1, &o, 0.3, &out);
  printf("tag: valid %u cov[0] %.3e cov[35] %.3e cov_alt[35] %.3e sq %.3e\n", out.valid, out.cov[0], out.cov[35], out.cov_alt[35], out.sq_err_sum);
  if (out.valid != 3u || !(out.cov[0] > 0.0) || !(out.cov[35] > 0.0) || out.cov[1] != out.cov[6] || out.reserved != 0u) bad++;
  o.status = AMDAT_POSE_REFINED_NO_ALT;
  memset(&out, 0xff, sizeof(out));
  pose_cov_tag_probe(p, 600.0, 600.0, 320.0, 240.0, 0.5, 0.1, &o, 0.3, &out);
  if (out.valid != 1u || out.cov_alt[0] != 0.0 || out.cov_alt[35] != 0.0 || out.sq_err_sum_alt != 0.0) bad++;
  const double same[8] = {100, 100, 100, 100, 100, 100, 100, 100};
  memset(&out, 0xff, sizeof(out));
  pose_cov_tag_probe(same, 600.0, 600.0, 320.0, 240.0, 0.0, 0.1, &o, 0.3, &out);
  printf("equal pixels: valid %u\n", out.valid);
  o.t[1] = NAN;
  memset(&out, 0xff, sizeof(out));
  pose_cov_tag_probe(p, 600.0, 600.0, 320.0, 240.0, 0.5, 0.1, &o, 0.3, &out);
  printf("NaN pose: valid %u\n", out.valid);
  if (out.valid != 0u || out.cov[0] != 0.0 || out.cov[35] != 0.0) bad++;
  // two tags of a bundle, side by side in the plane z = 0 and one lifted out of it
  amdAprilTagsBundlePoseEx_t b;
  memset(&b, 0, sizeof(b));
  for (int i = 0; i < 9; i++) b.R[i] = R[i];
  for (int i = 0; i < 3; i++) b.t[i] = t[i];
  b.status = AMDAT_BUNDLE_SOLVED;
  double obj[24], pix[16];
  for (int j = 0; j < 8; j++) {
    obj[3 * j] = s * c[j % 4][0] + (j < 4 ? -0.08 : 0.08); obj[3 * j + 1] = s * c[j % 4][1]; obj[3 * j + 2] = j < 4 ? 0.0 : 0.03;
    const double x = R[0] * obj[3 * j] + R[1] * obj[3 * j + 1] + R[2] * obj[3 * j + 2] + t[0],
                 y = R[3] * obj[3 * j] + R[4] * obj[3 * j + 1] + R[5] * obj[3 * j + 2] + t[1],
                 z = R[6] * obj[3 * j] + R[7] * obj[3 * j + 1] + R[8] * obj[3 * j + 2] + t[2];
    pix[2 * j] = 600.0 * x / z + 320.0; pix[2 * j + 1] = 600.0 * y / z + 240.0;
  }
  memset(&out, 0xff, sizeof(out));
  pose_cov_bundle_probe(2u, pix, obj, 600.0, 600.0, 320.0, 240.0, 0.0, &b, 0.3, &out);
  printf("bundle: valid %u cov[0] %.3e cov[35] %.3e\n", out.valid, out.cov[0], out.cov[35]);
  if (out.valid != 1u || !(out.cov[35] > 0.0) || out.cov_alt[7] != 0.0) bad++;
  b.status = AMDAT_BUNDLE_TOO_FEW_TAGS;
  memset(&out, 0xff, sizeof(out));
  pose_cov_bundle_probe(2u, pix, obj, 600.0, 600.0, 320.0, 240.0, 0.0, &b, 0.3, &out);
  if (out.valid != 0u || out.cov[0] != 0.0) bad++;
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
#endif
