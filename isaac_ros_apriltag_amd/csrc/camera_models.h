// camera_models.h -- the general projection of the rectification: the three distortion models of
// sensor_msgs/CameraInfo (plumb_bob, rational_polynomial, equidistant) behind a rectification rotation R.  Stated once, in plain
// double-precision operations, for k_rectify_frames_general, k_resize_frames_general and k_rectify_mono8_ex -- and for a host
// compiler: every function here is __host__ __device__ under hipcc and an ordinary inline function under g++
// (tests/aux_c/camera_models_driver.cpp compiles these lines with -ffp-contract=off and prints what they give).
// Every operator is one IEEE operation in the order written: no re-association, no fused multiply-add, no library call but the
// correctly rounded square root.  A term formed once per column or row has the value it has when it is formed per pixel.
#pragma once
#include <math.h>
#include <stdint.h>
#include "tools_hooks.h"

#if defined(__HIPCC__)
#define CAM_HD __host__ __device__ __forceinline__
#else
#define CAM_HD static inline
#endif

#define CAM_PLUMB_BOB 0u             // amdAprilTagsDistortion (include/apriltag_amd.h)
#define CAM_RATIONAL_POLYNOMIAL 1u
#define CAM_EQUIDISTANT 2u

struct RectifyParams {
  double fx, fy, cx, cy;        // source camera K
  double k1, k2, p1, p2, k3;    // plumb_bob
  double nfx, nfy, ncx, ncy;    // destination (pinhole) camera
};

// What the general projection needs beyond RectifyParams.  equidistant: RectifyParams' k1, k2, p1, p2 hold
// the fisheye's k1 .. k4 (D[0] .. D[3] of every kind sit in the same fields).
struct CamGeneral {
  uint32_t general;    // 0: plumb_bob with R exactly the identity -- the slot takes the hoisted plumb_bob statement (rect_taps)
  uint32_t kind;       // CAM_*
  double k4, k5, k6;   // rational_polynomial's denominator
  double Ri[9];        // the transpose of R, row-major
};

// ---- atan_s: the arctangent of r >= 0 in operations that every compiler rounds alike -------------------------------------------------
// Two reductions (1 / r above 1; (a - 1) / (a + 1) above tan(pi / 8)) leave |t| <= 0.41421356..., where the Maclaurin series to
// t^45 is cut below 2^-53 of its sum.  Largest distance from libm's atan over [0, 1000]: 2.3e-16.
#define CAM_ATAN_C(n) (((n) & 1 ? -1.0 : 1.0) / (double)(2 * (n) + 1))
CAM_HD double atan_s(double r) {
  const double a = r > 1.0 ? 1.0 / r : r;
  const bool reduced = a > 0.41421356237309503;
  const double t = reduced ? (a - 1.0) / (a + 1.0) : a;
  const double z = t * t;
  double p = CAM_ATAN_C(22);
  p = CAM_ATAN_C(21) + z * p; p = CAM_ATAN_C(20) + z * p; p = CAM_ATAN_C(19) + z * p; p = CAM_ATAN_C(18) + z * p;
  p = CAM_ATAN_C(17) + z * p; p = CAM_ATAN_C(16) + z * p; p = CAM_ATAN_C(15) + z * p; p = CAM_ATAN_C(14) + z * p;
  p = CAM_ATAN_C(13) + z * p; p = CAM_ATAN_C(12) + z * p; p = CAM_ATAN_C(11) + z * p; p = CAM_ATAN_C(10) + z * p;
  p = CAM_ATAN_C(9) + z * p; p = CAM_ATAN_C(8) + z * p; p = CAM_ATAN_C(7) + z * p; p = CAM_ATAN_C(6) + z * p;
  p = CAM_ATAN_C(5) + z * p; p = CAM_ATAN_C(4) + z * p; p = CAM_ATAN_C(3) + z * p; p = CAM_ATAN_C(2) + z * p;
  p = CAM_ATAN_C(1) + z * p; p = CAM_ATAN_C(0) + z * p;
  double s = t * p;
  if (reduced) s = 0.78539816339744830962 + s;   // M_PI_4
  if (r > 1.0) s = 1.57079632679489661923 - s;   // M_PI_2
  return s;
}

CAM_HD double cam_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return sqrt(x);
#endif
}

// ---- the projection of destination pixel (x, y), split where its operands allow ------------------------------------------------------
// xp = (x - ncx) / nfx and its three products with R^T's first column depend on the column alone; yp and its products with the
// second column on the row alone.  The ray (X, Y, W) = R^T (xp, yp, 1) is then three sums a pixel, and xn = X / W, yn = Y / W two
// divisions a pixel: with a rotation no part of xn is a column's alone.
struct CamCol { double a0, a3, a6; };   // Ri[0] * xp, Ri[3] * xp, Ri[6] * xp
struct CamRow { double b1, b4, b7; };   // Ri[1] * yp, Ri[4] * yp, Ri[7] * yp

CAM_HD CamCol cam_col(int x, const RectifyParams& R, const CamGeneral& G) {
  const double xp = ((double)x - R.ncx) / R.nfx;
  CamCol c;
  c.a0 = CAM_RI(G.Ri, 0) * xp; c.a3 = CAM_RI(G.Ri, 3) * xp; c.a6 = CAM_RI(G.Ri, 6) * xp;
  return c;
}
CAM_HD CamRow cam_row(int y, const RectifyParams& R, const CamGeneral& G) {
  const double yp = ((double)y - R.ncy) / R.nfy;
  CamRow r;
  r.b1 = CAM_RI(G.Ri, 1) * yp; r.b4 = CAM_RI(G.Ri, 4) * yp; r.b7 = CAM_RI(G.Ri, 7) * yp;
  return r;
}
// The source position (u, v) of the pixel, in pixels.  false: the ray points away from the camera (W <= 0 or NaN) -- the pixel is 0.
CAM_HD bool cam_project(const CamCol& c, const CamRow& r, const RectifyParams& R, const CamGeneral& G, double& u, double& v) {
  const double X = (c.a0 + r.b1) + CAM_RI(G.Ri, 2);
  const double Y = (c.a3 + r.b4) + CAM_RI(G.Ri, 5);
  const double W = (c.a6 + r.b7) + CAM_RI(G.Ri, 8);
  if (!(W > 0.0)) return false;
  const double xn = X / W, yn = Y / W;
  const double r2 = xn * xn + yn * yn;
  double xd, yd;
  if (G.kind == CAM_EQUIDISTANT) {   // OpenCV's fisheye model: D = k1 k2 k3 k4 in RectifyParams' k1, k2, p1, p2
    const double rr = cam_sqrt(r2);
    const double th = atan_s(rr);
    const double t2 = th * th;
    const double thd = th * (1.0 + t2 * (R.k1 + t2 * (R.k2 + t2 * (R.p1 + t2 * R.p2))));
    const double s = rr > 1e-8 ? thd / rr : 1.0;
    xd = xn * s; yd = yn * s;
  } else {
    double radial = 1.0 + r2 * (R.k1 + r2 * (R.k2 + r2 * R.k3));
    if (G.kind == CAM_RATIONAL_POLYNOMIAL) radial = radial / CAM_RATIONAL_DEN(1.0 + r2 * (G.k4 + r2 * (G.k5 + r2 * G.k6)));
    xd = xn * radial + (2.0 * R.p1 * xn * yn + R.p2 * (r2 + 2.0 * xn * xn));
    yd = yn * radial + (R.p1 * (r2 + 2.0 * yn * yn) + 2.0 * R.p2 * xn * yn);
  }
  u = R.fx * xd + R.cx;
  v = R.fy * yd + R.cy;
  return true;
}
