// undistort.h -- the inverse of the general projection: a raw pixel of a distorted camera to the pixel the
// rectified pinhole image would show it at, for amdAprilTagsSetCornerUndistortion.  Stated once, in plain double-precision operations,
// for k_undistort_records (kernels_undistort.h) and for a host compiler: every function here is __host__ __device__ under hipcc and an
// ordinary inline function under g++ (tests/aux_c/undistort_driver.cpp compiles these lines with -ffp-contract=off and prints what
// they give; tests/undistort_ref.py states them in numpy).
// Every operator is one IEEE operation in the order written: no re-association, no fused multiply-add, no library call but the
// correctly rounded square root and atan_s (camera_models.h).
#pragma once
#include <stdint.h>

#include "camera_models.h"

#define AMDAT_UNDISTORT_ITERATIONS 20
#define UD_GATE_PX 9.5367431640625e-07   // 2^-20 pixel: the round trip a converged point may miss by, per axis

// One batch slot's camera as the kernel reads it: amdAprilTagsCameraModelEx_t without what the statement never touches.
struct UndistortCam {
  uint32_t kind;               // CAM_*
  uint32_t pad;
  double fx, fy, cx, cy;       // K[0], K[4], K[2], K[5]
  double d[8];                 // D in CameraInfo's order (equidistant: k1 .. k4 in d[0 .. 3])
  double R[9];                 // row-major, as given: (X, Y, W) = R (x, y, 1)
  double nfx, nfy, ncx, ncy;   // Knew[0], Knew[4], Knew[2], Knew[5]
};

// x - x is +0.0 for every finite x and NaN for an infinity or a NaN
CAM_HD bool ud_finite(double x) { return x - x == 0.0; }

// The forward distortion of section 7b: normalised (x, y) -> (xd, yd), operation for operation what cam_project does between its
// division by W and its multiplication by K.
CAM_HD void ud_distort(const UndistortCam& C, double x, double y, double& xd, double& yd) {
  const double r2 = x * x + y * y;
  if (C.kind == CAM_EQUIDISTANT) {
    const double rr = cam_sqrt(r2);
    const double th = atan_s(rr);
    const double t2 = th * th;
    const double thd = th * (1.0 + t2 * (C.d[0] + t2 * (C.d[1] + t2 * (C.d[2] + t2 * C.d[3]))));
    const double s = rr > 1e-8 ? thd / rr : 1.0;
    xd = x * s; yd = y * s;
  } else {
    double radial = 1.0 + r2 * (C.d[0] + r2 * (C.d[1] + r2 * C.d[4]));
    if (C.kind == CAM_RATIONAL_POLYNOMIAL) radial = radial / (1.0 + r2 * (C.d[5] + r2 * (C.d[6] + r2 * C.d[7])));
    xd = x * radial + (2.0 * C.d[2] * x * y + C.d[3] * (r2 + 2.0 * x * x));
    yd = y * radial + (C.d[2] * (r2 + 2.0 * y * y) + 2.0 * C.d[3] * x * y);
  }
}

// One Newton step of plumb_bob / rational_polynomial on the unknowns (x, y): the residual e = distort(x, y) - (xd, yd), the analytic
// Jacobian J (the radial factor, its derivative by r^2, the tangential terms) and (x, y) -= J^-1 e by the closed 2 x 2 inverse.
CAM_HD void ud_newton_poly(const UndistortCam& C, double xd, double yd, double& x, double& y) {
  const double k1 = C.d[0], k2 = C.d[1], p1 = C.d[2], p2 = C.d[3], k3 = C.d[4];
  const double r2 = x * x + y * y;
  double radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
  double drad = k1 + r2 * (2.0 * k2 + r2 * (3.0 * k3));          // d radial / d r^2
  if (C.kind == CAM_RATIONAL_POLYNOMIAL) {                       // (N / Dn)' = (N' - (N / Dn) Dn') / Dn; plumb_bob divides by nothing
    const double den = 1.0 + r2 * (C.d[5] + r2 * (C.d[6] + r2 * C.d[7]));
    const double dden = C.d[5] + r2 * (2.0 * C.d[6] + r2 * (3.0 * C.d[7]));
    radial = radial / den;
    drad = (drad - radial * dden) / den;
  }
  const double ex = (x * radial + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) - xd;
  const double ey = (y * radial + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) - yd;
  const double cross = 2.0 * p1 * x + 2.0 * p2 * y;               // the tangential share of both off-diagonal entries
  const double J00 = (radial + 2.0 * (x * x) * drad) + (2.0 * p1 * y + 6.0 * p2 * x);
  const double J01 = 2.0 * (x * y) * drad + cross;
  const double J10 = J01;
  const double J11 = (radial + 2.0 * (y * y) * drad) + (6.0 * p1 * y + 2.0 * p2 * x);
  const double det = J00 * J11 - J01 * J10;
  x = x - (J11 * ex - J01 * ey) / det;
  y = y - (J00 * ey - J10 * ex) / det;
}

// One Newton step of equidistant on r = tan(theta): g(r) = theta_d(atan_s(r)) - thd.
CAM_HD double ud_newton_fisheye(const UndistortCam& C, double thd, double r) {
  const double th = atan_s(r);
  const double t2 = th * th;
  const double g = th * (1.0 + t2 * (C.d[0] + t2 * (C.d[1] + t2 * (C.d[2] + t2 * C.d[3])))) - thd;
  const double dg = (1.0 + t2 * (3.0 * C.d[0] + t2 * (5.0 * C.d[1] + t2 * (7.0 * C.d[2] + t2 * (9.0 * C.d[3]))))) / (1.0 + r * r);
  return r - g / dg;
}

// undistort(q): raw pixel (u, v) -> ideal pixel (uo, vo).  false (and uo = vo = 0): the iteration did not converge within the gate,
// some value is not finite, or the ray points away from the rectified camera (W > 0 is false).
CAM_HD bool ud_undistort(const UndistortCam& C, double u, double v, double& uo, double& vo) {
  const double xd = (u - C.cx) / C.fx;
  const double yd = (v - C.cy) / C.fy;
  double x = xd, y = yd;
  if (C.kind == CAM_EQUIDISTANT) {
    const double thd = cam_sqrt(xd * xd + yd * yd);
    if (thd > 1e-8) {
      double r = thd;
      for (int it = 0; it < AMDAT_UNDISTORT_ITERATIONS; it++) r = ud_newton_fisheye(C, thd, r);
      const double s = r / thd;
      x = xd * s; y = yd * s;
    }
  } else {
    for (int it = 0; it < AMDAT_UNDISTORT_ITERATIONS; it++) ud_newton_poly(C, xd, yd, x, y);
  }
  // the gate: the point pushed forward again lands on the pixel it came from
  double xf, yf;
  ud_distort(C, x, y, xf, yf);
  const double gx = C.fx * (xf - xd), gy = C.fy * (yf - yd);
  bool ok = ud_finite(x) && ud_finite(y) && ud_finite(gx) && ud_finite(gy);
  ok = ok && (gx < 0.0 ? -gx : gx) <= UD_GATE_PX && (gy < 0.0 ? -gy : gy) <= UD_GATE_PX;
  const double X = (UD_R(C.R, 0) * x + UD_R(C.R, 1) * y) + UD_R(C.R, 2);   // (tools_hooks.h: C.R[j] in the product build)
  const double Y = (UD_R(C.R, 3) * x + UD_R(C.R, 4) * y) + UD_R(C.R, 5);
  const double W = (UD_R(C.R, 6) * x + UD_R(C.R, 7) * y) + UD_R(C.R, 8);
  ok = ok && W > 0.0;
  const double uu = C.nfx * (X / W) + C.ncx;
  const double vv = C.nfy * (Y / W) + C.ncy;
  ok = ok && ud_finite(uu) && ud_finite(vv);
  uo = ok ? uu : 0.0;
  vo = ok ? vv : 0.0;
  return ok;
}
