// Host driver of csrc/pose_refine.h for tests/test_pose_refine_cpu.py: the definition of the orthogonal-iteration tag pose compiled by
// g++ (-ffp-contract=off), as a shared object that Python calls, and -- with -DPOSE_REFINE_MAIN -- as a program of its own for the
// sanitizer run.
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../isaac_ros_apriltag_amd/csrc/pose_refine.h"

extern "C" {

// p8: the four corners (u0, v0, u1, v1, ...); Rh row-major
void pose_refine_probe(const double* p8, double fx, double fy, double cx, double cy, double skew, double tag_size, const double* Rh,
                       const double* th, uint32_t iterations, amdAprilTagsRefinedPose_t* out) {
  double p[4][2];
  for (int k = 0; k < 4; k++) { p[k][0] = p8[2 * k]; p[k][1] = p8[2 * k + 1]; }
  pr_refine_tag(p, fx, fy, cx, cy, skew, tag_size, Rh, th, iterations, out);
}

uint32_t pose_refine_sizes(uint32_t which) {
  switch (which) {
    case 0: return (uint32_t)sizeof(amdAprilTagsRefinedPose_t);
    case 1: return (uint32_t)offsetof(amdAprilTagsRefinedPose_t, err_homography);
    case 2: return PR_MAX_ITERATIONS;
    default: return 0;
  }
}

}  // extern "C"

#ifdef POSE_REFINE_MAIN
// A tag of 0.1 m seen obliquely, its mirror-prone neighbour, a skewed camera, one iteration and two hundred, and the degenerate
// record (four equal corners): every path of the header once, under the sanitizers.
int main(void) {
  const double Rh[9] = {0.8, -0.1, 0.59, 0.05, 0.99, 0.1, -0.6, -0.05, 0.8};
  const double th[3] = {0.05, -0.02, 0.9};
  double p[8];
  const double s = 0.05, c[4][2] = {{-1, 1}, {1, 1}, {1, -1}, {-1, -1}};
  for (int k = 0; k < 4; k++) {
    const double x = Rh[0] * s * c[k][0] + Rh[1] * s * c[k][1] + th[0], y = Rh[3] * s * c[k][0] + Rh[4] * s * c[k][1] + th[1],
                 z = Rh[6] * s * c[k][0] + Rh[7] * s * c[k][1] + th[2];
    p[2 * k] = 600.0 * x / z + 0.5 * y / z + 320.0 + 0.3 * c[k][0];
    p[2 * k + 1] = 600.0 * y / z + 240.0 - 0.2 * c[k][1];
  }
  amdAprilTagsRefinedPose_t o;
  int bad = 0;
  const uint32_t iters[3] = {1u, 50u, PR_MAX_ITERATIONS};
  for (int i = 0; i < 3; i++) {
    memset(&o, 0xff, sizeof(o));
    pose_refine_probe(p, 600.0, 600.0, 320.0, 240.0, 0.5, 0.1, Rh, th, iters[i], &o);
    if (o.status != AMDAT_POSE_REFINED || o.chosen > 1u || !(o.err <= o.err_alt)) bad++;
    printf("iterations %u: status %u chosen %u err %.3e err_alt %.3e err_homography %.3e\n", iters[i], o.status, o.chosen, o.err, o.err_alt,
           o.err_homography);
  }
  const double same[8] = {100, 100, 100, 100, 100, 100, 100, 100};
  memset(&o, 0xff, sizeof(o));
  pose_refine_probe(same, 600.0, 600.0, 320.0, 240.0, 0.0, 0.1, Rh, th, 50u, &o);
  printf("equal corners: status %u chosen %u\n", o.status, o.chosen);
  if (o.status != AMDAT_POSE_DEGENERATE || o.chosen != 0u || o.err_alt != 0.0 || o.R[0] != Rh[0] || o.t[2] != th[2]) bad++;
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
#endif
