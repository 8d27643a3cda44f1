// rig_pose.h -- the pose of a rigid 3-D tag bundle in the frame of a camera rig (amdAprilTagsSetRig): the
// object-space iteration of rigid_pose.h over the observations of ALL cameras of one instant, every viewing ray carried into the rig
// frame with its camera's centre as its origin.  Stated once, in plain double-precision operations, for k_bundle_rig
// (kernels_rig.h) and for a host compiler, in the manner of rigid_pose.h, whose polar rotation, seed area, start composition and
// outcome rule are used as they stand: every function here is __host__ __device__ under hipcc and an ordinary inline function under
// g++ (tests/aux_c/rig_pose_driver.cpp compiles these lines with -ffp-contract=off; tests/rig_pose_ref.py states them in Python).
// Every operator is one IEEE operation in the order written: no re-association, no fused multiply-add, no library call but the
// correctly rounded square root.
//
// An observation is one used record of one camera; it fills one of the 64 slots of rigid_pose.h with its four corners, and the sums
// are rigid_pose.h's: (x0 + x1) + (x2 + x3) per slot, then the balanced tree over the slots (RgSumWave on the device, RgSumTree on
// the host).  A camera is (Rc, tc), the rig frame in the camera frame: X_cam = Rc X_rig + tc.  The statements are arranged so that a
// rig of one camera with Rc the exact identity and tc = 0 gives rigid_pose.h's bits: a product with an exact 1 or 0 and x - 0.0
// change no bit of x, and nothing but a -0.0 could tell the two apart.
#pragma once
#include "rigid_pose.h"

// The camera of an observation: the frame's intrinsics and skew, and the extrinsics of its rig camera.
struct RigCam {
  double fx, fy, cx, cy, skew;
  double R[9], t[3];
};

// RgPoints and the ray origin o = Rc^T (0 - tc) of each point: the camera's centre in the rig frame.
template <int NC>
struct RigPoints {
  RgPoints<NC> g;
  double ox[NC], oy[NC], oz[NC];
};

// pix[j]: the pixel of point j, obj[j]: its object point, cam[j / 4]: its observation's camera (a lane holds one observation: cam[0]).
// The ray v = (un, vn, 1) is rigid_pose.h's; its direction in the rig frame is d = Rc^T v (RIG_RAY_R, tools_hooks.h: entry (i, k) of
// Rc^T), and F = d d^T / (d^T d).  Fills the points and Gi as rg_setup does.
template <int NC, class Sum>
PR_HD void rig_setup(const double (*pix)[2], const double (*obj)[3], const RigCam* cam, double npts, const Sum& sum, RigPoints<NC>* C,
                     double* Gi) {
  for (int j = 0; j < NC; j++) {
    const RigCam& k = cam[j / 4];
    C->g.px[j] = obj[j][0]; C->g.py[j] = obj[j][1]; C->g.pz[j] = obj[j][2];
    const double vn = (pix[j][1] - k.cy) / k.fy;
    const double un = ((pix[j][0] - k.cx) - k.skew * vn) / k.fx;
    const double d0 = (RIG_RAY_R(k.R, 0, 0) * un + RIG_RAY_R(k.R, 0, 1) * vn) + RIG_RAY_R(k.R, 0, 2);
    const double d1 = (RIG_RAY_R(k.R, 1, 0) * un + RIG_RAY_R(k.R, 1, 1) * vn) + RIG_RAY_R(k.R, 1, 2);
    const double d2 = (RIG_RAY_R(k.R, 2, 0) * un + RIG_RAY_R(k.R, 2, 1) * vn) + RIG_RAY_R(k.R, 2, 2);
    const double nn = (d0 * d0 + d1 * d1) + d2 * d2;
    C->g.F00[j] = (d0 * d0) / nn; C->g.F01[j] = (d0 * d1) / nn; C->g.F02[j] = (d0 * d2) / nn;
    C->g.F11[j] = (d1 * d1) / nn; C->g.F12[j] = (d1 * d2) / nn; C->g.F22[j] = (d2 * d2) / nn;
    const double e0 = 0.0 - k.t[0], e1 = 0.0 - k.t[1], e2 = 0.0 - k.t[2];
    C->ox[j] = (k.R[0] * e0 + k.R[3] * e1) + k.R[6] * e2;
    C->oy[j] = (k.R[1] * e0 + k.R[4] * e1) + k.R[7] * e2;
    C->oz[j] = (k.R[2] * e0 + k.R[5] * e1) + k.R[8] * e2;
  }
  const double mx = sum(C->g.px) / npts, my = sum(C->g.py) / npts, mz = sum(C->g.pz) / npts;
  for (int j = 0; j < NC; j++) { C->g.cx[j] = C->g.px[j] - mx; C->g.cy[j] = C->g.py[j] - my; C->g.cz[j] = C->g.pz[j] - mz; }
  const double G00 = 1.0 - sum(C->g.F00) / npts, G01 = -(sum(C->g.F01) / npts), G02 = -(sum(C->g.F02) / npts);
  const double G11 = 1.0 - sum(C->g.F11) / npts, G12 = -(sum(C->g.F12) / npts), G22 = 1.0 - sum(C->g.F22) / npts;
  const double c00 = G11 * G22 - G12 * G12, c01 = G12 * G02 - G01 * G22, c02 = G01 * G12 - G11 * G02;
  const double c11 = G00 * G22 - G02 * G02, c12 = G01 * G02 - G00 * G12, c22 = G00 * G11 - G01 * G01;
  const double det = (G00 * c00 + G01 * c01) + G02 * c02;
  Gi[0] = c00 / det; Gi[1] = c01 / det; Gi[2] = c02 / det; Gi[3] = c11 / det; Gi[4] = c12 / det; Gi[5] = c22 / det;
}

// t(R) = G^-1 (sum (F_j - I)(R P_j - o_j)) / npts
template <int NC, class Sum>
PR_HD void rig_translation(const RigPoints<NC>& C, const double* Gi, const double* R, double npts, const Sum& sum, double* t) {
  double a0[NC], a1[NC], a2[NC];
  for (int j = 0; j < NC; j++) {
    RG_RP(R, C.g, j, r0, r1, r2)
    const double w0 = r0 - RIG_T_ORIGIN(C.ox[j]), w1 = r1 - RIG_T_ORIGIN(C.oy[j]), w2 = r2 - RIG_T_ORIGIN(C.oz[j]);
    a0[j] = ((C.g.F00[j] * w0 + C.g.F01[j] * w1) + C.g.F02[j] * w2) - w0;
    a1[j] = ((C.g.F01[j] * w0 + C.g.F11[j] * w1) + C.g.F12[j] * w2) - w1;
    a2[j] = ((C.g.F02[j] * w0 + C.g.F12[j] * w1) + C.g.F22[j] * w2) - w2;
  }
  const double b0 = sum(a0) / npts, b1 = sum(a1) / npts, b2 = sum(a2) / npts;
  t[0] = (Gi[0] * b0 + Gi[1] * b1) + Gi[2] * b2;
  t[1] = (Gi[1] * b0 + Gi[3] * b1) + Gi[4] * b2;
  t[2] = (Gi[2] * b0 + Gi[4] * b1) + Gi[5] * b2;
}

// R P_j + t - o_j for point j
#define RIG_X(R, t, C, j, x0, x1, x2)                                                      \
  RG_RP(R, C.g, j, x0##_w, x1##_w, x2##_w)                                                 \
  const double x0 = (x0##_w + t[0]) - C.ox[j], x1 = (x1##_w + t[1]) - C.oy[j], x2 = (x2##_w + t[2]) - C.oz[j];

// E(R, t) = sum |(I - F_j)(R P_j + t - o_j)|^2
template <int NC, class Sum>
PR_HD double rig_error(const RigPoints<NC>& C, const double* R, const double* t, const Sum& sum) {
  double e[NC];
  for (int j = 0; j < NC; j++) {
    RIG_X(R, t, C, j, x0, x1, x2)
    const double e0 = x0 - ((C.g.F00[j] * x0 + C.g.F01[j] * x1) + C.g.F02[j] * x2);
    const double e1 = x1 - ((C.g.F01[j] * x0 + C.g.F11[j] * x1) + C.g.F12[j] * x2);
    const double e2 = x2 - ((C.g.F02[j] * x0 + C.g.F12[j] * x1) + C.g.F22[j] * x2);
    e[j] = (e0 * e0 + e1 * e1) + e2 * e2;
  }
  return sum(e);
}

// The rotation of one iteration: q_j = o_j + F_j (R P_j + t - o_j), M = sum (q_j - mean q)(P_j - mean P)^T, and its rotation by
// rg_polar.
template <int NC, class Sum>
PR_HD bool rig_rotation(const RigPoints<NC>& C, const double* R, const double* t, double npts, const Sum& sum, double* Rn) {
  double q0[NC], q1[NC], q2[NC], m[NC], M[9];
  for (int j = 0; j < NC; j++) {
    RIG_X(R, t, C, j, x0, x1, x2)
    q0[j] = C.ox[j] + ((C.g.F00[j] * x0 + C.g.F01[j] * x1) + C.g.F02[j] * x2);
    q1[j] = C.oy[j] + ((C.g.F01[j] * x0 + C.g.F11[j] * x1) + C.g.F12[j] * x2);
    q2[j] = C.oz[j] + ((C.g.F02[j] * x0 + C.g.F12[j] * x1) + C.g.F22[j] * x2);
  }
  const double qb0 = sum(q0) / npts, qb1 = sum(q1) / npts, qb2 = sum(q2) / npts;
  for (int j = 0; j < NC; j++) { q0[j] = q0[j] - qb0; q1[j] = q1[j] - qb1; q2[j] = q2[j] - qb2; }
  for (int j = 0; j < NC; j++) m[j] = q0[j] * C.g.cx[j];
  M[0] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q0[j] * C.g.cy[j];
  M[1] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q0[j] * C.g.cz[j];
  M[2] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q1[j] * C.g.cx[j];
  M[3] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q1[j] * C.g.cy[j];
  M[4] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q1[j] * C.g.cz[j];
  M[5] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q2[j] * C.g.cx[j];
  M[6] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q2[j] * C.g.cy[j];
  M[7] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q2[j] * C.g.cz[j];
  M[8] = sum(m);
  return rg_polar(M, Rn);
}

// One chain, as rg_chain: t = t(R) at the start, `iterations` steps with no early exit, E at the end; false: degenerate.
template <int NC, class Sum>
PR_HD bool rig_chain(const RigPoints<NC>& C, const double* Gi, const double* Rstart, uint32_t iterations, double npts, const Sum& sum,
                     double* R, double* t, double* E) {
  for (int i = 0; i < 9; i++) R[i] = Rstart[i];
  rig_translation<NC>(C, Gi, R, npts, sum, t);
  bool ok = pr_pose_finite(R, t);
  for (uint32_t it = 0; it < iterations; it++) {
    double Rn[9];
    const bool pos = rig_rotation<NC>(C, R, t, npts, sum, Rn);
    for (int i = 0; i < 9; i++) R[i] = Rn[i];
    rig_translation<NC>(C, Gi, R, npts, sum, t);
    ok = ok && pos && pr_pose_finite(R, t);
  }
  *E = rig_error<NC>(C, R, t, sum);
  return ok && pr_finite(*E);
}

// A bundle pose in a camera's frame moved into the rig frame: Rc^T Rb, and (tr non-null) Rc^T (tb - tc).
PR_HD void rig_from_camera(const double* Rc, const double* tc, const double* Rb, const double* tb, double* Rr, double* tr) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Rr[3 * i + j] = (Rc[i] * Rb[j] + Rc[3 + i] * Rb[3 + j]) + Rc[6 + i] * Rb[6 + j];
  if (tr) {
    const double e0 = tb[0] - tc[0], e1 = tb[1] - tc[1], e2 = tb[2] - tc[2];
    for (int i = 0; i < 3; i++) tr[i] = (Rc[i] * e0 + Rc[3 + i] * e1) + Rc[6 + i] * e2;
  }
}

// The squared pixel reprojection errors of one observation's four corners under the rig pose (R, t): the point Rc (R P + t) + tc
// under the observation's camera, added as rg_reprojection's.
PR_HD double rig_reprojection(const double (*pix)[2], const double (*obj)[3], const double* R, const double* t, const RigCam& k) {
  double e[4];
  for (int c = 0; c < 4; c++) {
    const double X0 = ((R[0] * obj[c][0] + R[1] * obj[c][1]) + R[2] * obj[c][2]) + t[0];
    const double X1 = ((R[3] * obj[c][0] + R[4] * obj[c][1]) + R[5] * obj[c][2]) + t[1];
    const double X2 = ((R[6] * obj[c][0] + R[7] * obj[c][1]) + R[8] * obj[c][2]) + t[2];
    const double xc = ((k.R[0] * X0 + k.R[1] * X1) + k.R[2] * X2) + k.t[0];
    const double yc = ((k.R[3] * X0 + k.R[4] * X1) + k.R[5] * X2) + k.t[1];
    const double zc = ((k.R[6] * X0 + k.R[7] * X1) + k.R[8] * X2) + k.t[2];
    const double xn = xc / zc, yn = yc / zc;
    const double u = (k.fx * xn + k.skew * yn) + k.cx;
    const double v = k.fy * yn + k.cy;
    const double du = u - pix[c][0], dv = v - pix[c][1];
    e[c] = du * du + dv * dv;
  }
  return ((e[0] + e[1]) + e[2]) + e[3];
}

// rg_outcome's rule into the rig record: status, chosen and the pose fields; the counts and the seed are the caller's.
PR_HD void rig_outcome(bool ok0, const double* R0, const double* t0, double E0, double sq0, bool ok1, const double* R1, const double* t1,
                       double E1, double sq1, const double* Rs, const double* ts, double Es, amdAprilTagsRigBundlePose_t* o) {
  amdAprilTagsBundlePoseEx_t x;
  rg_outcome(ok0, R0, t0, E0, sq0, ok1, R1, t1, E1, sq1, Rs, ts, Es, &x);
  o->status = x.status;
  o->chosen = x.chosen;
  for (int i = 0; i < 9; i++) { o->R[i] = x.R[i]; o->R_alt[i] = x.R_alt[i]; }
  for (int i = 0; i < 3; i++) { o->t[i] = x.t[i]; o->t_alt[i] = x.t_alt[i]; }
  o->err = x.err; o->sq_err_sum = x.sq_err_sum;
  o->err_alt = x.err_alt; o->sq_err_sum_alt = x.sq_err_sum_alt;
}

#if !defined(__HIPCC__)
// One (group, bundle) on one host thread: slot s < nobs holds the observation's corners pix[4 s + k], its member's corners
// obj[4 s + k], its camera cam[s], and its homography pose under that camera (Rh + 9 s, th + 3 s) with its member's pose
// (Rm + 9 s, tm + 3 s).  Fills status, chosen and the pose fields; `seed` comes back as the SLOT of the seed.  nobs in 1 .. RG_SLOTS.
static inline void rig_solve_host(uint32_t nobs, const double (*pix)[2], const double (*obj)[3], const RigCam* cam, const double* Rh,
                                  const double* th, const double* Rm, const double* tm, uint32_t iterations,
                                  amdAprilTagsRigBundlePose_t* o) {
  uint32_t seed = 0;
  double best = -1.0;
  for (uint32_t s = 0; s < nobs; s++) {
    const double a = rg_area2(pix + 4 * s);
    if (a > best) { best = a; seed = s; }
  }
  double Rb0[9], tb0[3], Rmir[9], Rb1[9], Rs0[9], ts0[3], Rs1[9];
  rg_compose_start(Rh + 9 * seed, th + 3 * seed, Rm + 9 * seed, tm + 3 * seed, Rb0, tb0);
  pr_mirror_start(Rh + 9 * seed, th + 3 * seed, Rmir);
  rg_compose_start(Rmir, (const double*)0, Rm + 9 * seed, tm + 3 * seed, Rb1, (double*)0);
  rig_from_camera(cam[seed].R, cam[seed].t, Rb0, tb0, Rs0, ts0);
  rig_from_camera(cam[seed].R, cam[seed].t, Rb1, (const double*)0, Rs1, (double*)0);
  const RgSumTree sum = {nobs};
  const double npts = 4.0 * (double)nobs;
  static thread_local RigPoints<4 * RG_SLOTS> C;
  double Gi[6];
  rig_setup<4 * RG_SLOTS>(pix, obj, cam, npts, sum, &C, Gi);
  const double Es = rig_error<4 * RG_SLOTS>(C, Rs0, ts0, sum);
  double R0[9], t0[3], E0, R1[9], t1[3], E1;
  const bool ok0 = rig_chain<4 * RG_SLOTS>(C, Gi, Rs0, iterations, npts, sum, R0, t0, &E0);
  const bool ok1 = rig_chain<4 * RG_SLOTS>(C, Gi, Rs1, iterations, npts, sum, R1, t1, &E1);
  double sq0 = 0.0, sq1 = 0.0;
  for (uint32_t s = 0; s < nobs; s++) {
    sq0 = sq0 + rig_reprojection(pix + 4 * s, obj + 4 * s, R0, t0, cam[s]);
    sq1 = sq1 + rig_reprojection(pix + 4 * s, obj + 4 * s, R1, t1, cam[s]);
  }
  rig_outcome(ok0, R0, t0, E0, sq0, ok1, R1, t1, E1, sq1, Rs0, ts0, Es, o);
  o->seed = seed;
}
#endif
