// camera_models_driver.cpp -- the general projection of csrc/camera_models.h compiled by a host compiler (g++ -O2 -ffp-contract=off):
// the same lines the kernels compile.  tests/test_camera_models_cpu.py compares what this prints with tests/camera_models_ref.py.
//
//   camera_models_driver W H STEP KIND fx fy cx cy D0..D7 R0..R8 nfx nfy ncx ncy      (doubles as C99 hex floats or decimals)
//
// prints, for every pixel (x, y) with x % STEP == 0 and y % STEP == 0, one line "x y ok u v": ok is 1 where the ray points towards the
// camera, u and v the bit patterns of the source position as 16 hex digits (0 where ok is 0).  With W = 0 it reads nothing more and
// prints atan_s of the arguments that follow, one bit pattern a line.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../isaac_ros_apriltag_amd/csrc/camera_models.h"

static unsigned long long bits(double v) {
  unsigned long long b;
  memcpy(&b, &v, 8);
  return b;
}

int main(int argc, char** argv) {
  if (argc >= 2 && atoi(argv[1]) == 0) {
    for (int i = 2; i < argc; i++) printf("%016llx\n", bits(atan_s(strtod(argv[i], nullptr))));
    return 0;
  }
  if (argc != 5 + 4 + 8 + 9 + 4) {
    fprintf(stderr, "usage: camera_models_driver W H STEP KIND fx fy cx cy D[8] R[9] nfx nfy ncx ncy\n");
    return 2;
  }
  const int w = atoi(argv[1]), h = atoi(argv[2]), step = atoi(argv[3]);
  double a[25];
  for (int i = 0; i < 25; i++) a[i] = strtod(argv[5 + i], nullptr);
  const double *K = a, *D = a + 4, *Rm = a + 12, *Kn = a + 21;
  RectifyParams R = {K[0], K[1], K[2], K[3], D[0], D[1], D[2], D[3], D[4], Kn[0], Kn[1], Kn[2], Kn[3]};
  CamGeneral G;
  G.general = 1;
  G.kind = (uint32_t)atoi(argv[4]);
  G.k4 = D[5]; G.k5 = D[6]; G.k6 = D[7];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) G.Ri[3 * r + c] = Rm[3 * c + r];
  if (w <= 0 || h <= 0 || step <= 0 || G.kind > CAM_EQUIDISTANT) return 2;
  for (int y = 0; y < h; y += step) {
    const CamRow row = cam_row(y, R, G);
    for (int x = 0; x < w; x += step) {
      double u = 0.0, v = 0.0;
      const bool ok = cam_project(cam_col(x, R, G), row, R, G, u, v);
      printf("%d %d %d %016llx %016llx\n", x, y, ok ? 1 : 0, ok ? bits(u) : 0ull, ok ? bits(v) : 0ull);
    }
  }
  return 0;
}
