// undistort_driver.cpp -- the point map of csrc/undistort.h compiled by a host compiler (g++ -O2 -ffp-contract=off): the same lines
// k_undistort_records compiles.  tests/test_corner_undistortion_cpu.py compares what this prints with tests/undistort_ref.py, and
// builds it once more with -fsanitize=address,undefined.
//
//   undistort_driver KIND fx fy cx cy D0..D7 R0..R8 nfx nfy ncx ncy  u0 v0 u1 v1 ...      (doubles as C99 hex floats or decimals)
//
// prints, for every pixel (u, v), one line "ok uo vo": ok is 1 where the point converged inside the gate and looks towards the
// rectified camera, uo and vo the bit patterns of the ideal pixel as 16 hex digits (0 where ok is 0).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../isaac_ros_apriltag_amd/csrc/undistort.h"

static unsigned long long bits(double v) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  return b;
}

int main(int argc, char** argv) {
  const int fixed = 2 + 4 + 8 + 9 + 4;
  if (argc < fixed || ((argc - fixed) & 1)) {
    fprintf(stderr, "usage: undistort_driver KIND fx fy cx cy D[8] R[9] nfx nfy ncx ncy [u v]...\n");
    return 2;
  }
  std::vector<double> a(argc - 2);
  for (int i = 2; i < argc; i++) a[i - 2] = strtod(argv[i], nullptr);
  UndistortCam C;
  memset(&C, 0, sizeof(C));
  C.kind = (uint32_t)atoi(argv[1]);
  if (C.kind > CAM_EQUIDISTANT) return 2;
  C.fx = a[0]; C.fy = a[1]; C.cx = a[2]; C.cy = a[3];
  for (int j = 0; j < 8; j++) C.d[j] = a[4 + j];
  for (int j = 0; j < 9; j++) C.R[j] = a[12 + j];
  C.nfx = a[21]; C.nfy = a[22]; C.ncx = a[23]; C.ncy = a[24];
  for (size_t i = 25; i + 1 < a.size(); i += 2) {
    double uo = 0.0, vo = 0.0;
    const bool ok = ud_undistort(C, a[i], a[i + 1], uo, vo);
    printf("%d %016llx %016llx\n", ok ? 1 : 0, bits(uo), bits(vo));
  }
  return 0;
}
