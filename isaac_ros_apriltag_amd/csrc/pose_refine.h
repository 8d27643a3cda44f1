// pose_refine.h -- the orthogonal-iteration tag pose with both minima (amdAprilTagsSetPoseRefinement): the
// object-space iteration of Lu, Hager and Mjolsness on the four corners of one tag, run as two independent chains -- one from the
// homography pose, one from its mirror about the viewing ray -- and the outcome rule that picks between them.  Stated once, in plain
// double-precision operations, for k_pose_refine (kernels_pose.h) and for a host compiler: every function here is
// __host__ __device__ under hipcc and an ordinary inline function under g++ (tests/aux_c/pose_refine_driver.cpp compiles these lines
// with -ffp-contract=off; tests/pose_refine_ref.py states them in Python floats).
// Every operator is one IEEE operation in the order written: no re-association, no fused multiply-add, no library call but the
// correctly rounded square root.
//
// The per-point statements are loops over the NC points a thread holds, and every sum over the points goes through `sum`: the host
// holds all four corners (NC = 4, PrSumSerial: (x0 + x1) + (x2 + x3)); a lane of k_pose_refine holds one (NC = 1) and its `sum` is
// the two-step butterfly over the four lanes of a chain, which gives every lane those same bits.  The point count is the parameter
// `npts` (the divisor of the means) together with `sum`: a bundle of 4 * ntags corners needs another `sum`, and nothing else here.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/apriltag_amd.h"
#include "tools_hooks.h"

#if defined(__HIPCC__)
#define PR_HD __host__ __device__ __forceinline__
#define PR_HD_MEMBER __host__ __device__ __forceinline__
#else
#define PR_HD static inline
#define PR_HD_MEMBER inline
#endif

#define PR_MAX_ITERATIONS 200u

PR_HD double pr_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return sqrt(x);
#endif
}

// x - x is +0.0 for every finite x and NaN for an infinity or a NaN
PR_HD bool pr_finite(double x) { return x - x == 0.0; }

struct PrSumSerial {
  PR_HD_MEMBER double operator()(const double* x) const { return (x[0] + x[1]) + (x[2] + x[3]); }
};

// What a thread holds of its NC points: the ray (un, vn, 1), the six distinct entries of the projector F = v v^T / (v^T v), and the
// object point (px, py, 0).
template <int NC>
struct PrPoints {
  double F00[NC], F01[NC], F02[NC], F11[NC], F12[NC], F22[NC];
  double px[NC], py[NC];
};

// Corner k0 + j of the tag for j < NC: pix[j] is its pixel (u, v).  Fills the points and Gi, the six distinct entries
// (00, 01, 02, 11, 12, 22) of the inverse of G = I - (sum F) / npts, by cofactors.
template <int NC, class Sum>
PR_HD void pr_setup(const double (*pix)[2], int k0, double fx, double fy, double cx, double cy, double skew, double s, double npts,
                    const Sum& sum, PrPoints<NC>* C, double* Gi) {
  for (int j = 0; j < NC; j++) {
    const int k = k0 + j;
    const double ckx = (k == 0 || k == 3) ? -1.0 : 1.0, cky = k < 2 ? 1.0 : -1.0;
    C->px[j] = s * ckx;
    C->py[j] = s * cky;
    const double vn = (pix[j][1] - cy) / fy;
    const double un = ((pix[j][0] - cx) - skew * vn) / fx;
    const double nn = (un * un + vn * vn) + 1.0;
    C->F00[j] = (un * un) / nn; C->F01[j] = (un * vn) / nn; C->F02[j] = un / nn;
    C->F11[j] = (vn * vn) / nn; C->F12[j] = vn / nn; C->F22[j] = 1.0 / nn;
  }
  const double G00 = 1.0 - sum(C->F00) / npts, G01 = -(sum(C->F01) / npts), G02 = -(sum(C->F02) / npts);
  const double G11 = 1.0 - sum(C->F11) / npts, G12 = -(sum(C->F12) / npts), G22 = 1.0 - sum(C->F22) / npts;
  const double c00 = G11 * G22 - G12 * G12, c01 = G12 * G02 - G01 * G22, c02 = G01 * G12 - G11 * G02;
  const double c11 = G00 * G22 - G02 * G02, c12 = G01 * G02 - G00 * G12, c22 = G00 * G11 - G01 * G01;
  const double det = (G00 * c00 + G01 * c01) + G02 * c02;
  Gi[0] = c00 / det; Gi[1] = c01 / det; Gi[2] = c02 / det; Gi[3] = c11 / det; Gi[4] = c12 / det; Gi[5] = c22 / det;
}

// t(R) = G^-1 (sum (F_k - I) R P_k) / npts
template <int NC, class Sum>
PR_HD void pr_translation(const PrPoints<NC>& C, const double* Gi, const double* R, double npts, const Sum& sum, double* t) {
  double a0[NC], a1[NC], a2[NC];
  for (int j = 0; j < NC; j++) {
    const double w0 = R[0] * C.px[j] + R[1] * C.py[j], w1 = R[3] * C.px[j] + R[4] * C.py[j], w2 = R[6] * C.px[j] + R[7] * C.py[j];
    a0[j] = ((C.F00[j] * w0 + C.F01[j] * w1) + C.F02[j] * w2) - w0;
    a1[j] = ((C.F01[j] * w0 + C.F11[j] * w1) + C.F12[j] * w2) - w1;
    a2[j] = ((C.F02[j] * w0 + C.F12[j] * w1) + C.F22[j] * w2) - w2;
  }
  const double b0 = sum(a0) / npts, b1 = sum(a1) / npts, b2 = sum(a2) / npts;
  t[0] = (Gi[0] * b0 + Gi[1] * b1) + Gi[2] * b2;
  t[1] = (Gi[1] * b0 + Gi[3] * b1) + Gi[4] * b2;
  t[2] = (Gi[2] * b0 + Gi[4] * b1) + Gi[5] * b2;
}

// E(R, t) = sum |(I - F_k)(R P_k + t)|^2
template <int NC, class Sum>
PR_HD double pr_error(const PrPoints<NC>& C, const double* R, const double* t, const Sum& sum) {
  double e[NC];
  for (int j = 0; j < NC; j++) {
    const double x0 = (R[0] * C.px[j] + R[1] * C.py[j]) + t[0], x1 = (R[3] * C.px[j] + R[4] * C.py[j]) + t[1],
                 x2 = (R[6] * C.px[j] + R[7] * C.py[j]) + t[2];
    const double e0 = x0 - ((C.F00[j] * x0 + C.F01[j] * x1) + C.F02[j] * x2);
    const double e1 = x1 - ((C.F01[j] * x0 + C.F11[j] * x1) + C.F12[j] * x2);
    const double e2 = x2 - ((C.F02[j] * x0 + C.F12[j] * x1) + C.F22[j] * x2);
    e[j] = (e0 * e0 + e1 * e1) + e2 * e2;
  }
  return sum(e);
}

// The rotation of one iteration: q_k = F_k (R P_k + t), the 3 x 2 block A of sum (q_k - mean q) P_k^T, its polar factor by the
// closed-form square root of the 2 x 2 matrix S = A^T A, the third column by a cross product.  False where det S > 0 is false.
template <int NC, class Sum>
PR_HD bool pr_rotation(const PrPoints<NC>& C, const double* R, const double* t, double npts, const Sum& sum, double* Rn) {
  double q0[NC], q1[NC], q2[NC], m[NC];
  for (int j = 0; j < NC; j++) {
    const double x0 = (R[0] * C.px[j] + R[1] * C.py[j]) + t[0], x1 = (R[3] * C.px[j] + R[4] * C.py[j]) + t[1],
                 x2 = (R[6] * C.px[j] + R[7] * C.py[j]) + t[2];
    q0[j] = (C.F00[j] * x0 + C.F01[j] * x1) + C.F02[j] * x2;
    q1[j] = (C.F01[j] * x0 + C.F11[j] * x1) + C.F12[j] * x2;
    q2[j] = (C.F02[j] * x0 + C.F12[j] * x1) + C.F22[j] * x2;
  }
  const double qb0 = sum(q0) / npts, qb1 = sum(q1) / npts, qb2 = sum(q2) / npts;
  for (int j = 0; j < NC; j++) { q0[j] = q0[j] - qb0; q1[j] = q1[j] - qb1; q2[j] = q2[j] - qb2; }
  for (int j = 0; j < NC; j++) m[j] = q0[j] * C.px[j];
  const double A00 = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q0[j] * C.py[j];
  const double A01 = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q1[j] * C.px[j];
  const double A10 = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q1[j] * C.py[j];
  const double A11 = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q2[j] * C.px[j];
  const double A20 = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q2[j] * C.py[j];
  const double A21 = sum(m);
  const double S00 = (A00 * A00 + A10 * A10) + A20 * A20, S01 = (A00 * A01 + A10 * A11) + A20 * A21,
               S11 = (A01 * A01 + A11 * A11) + A21 * A21;
  const double d = S00 * S11 - S01 * S01;
  const double r = pr_sqrt(d);
  const double tau = pr_sqrt((S00 + S11) + 2.0 * r);
  const double T00 = (S00 + r) / tau, T01 = S01 / tau, T11 = (S11 + r) / tau;   // the square root of S
  const double dt = T00 * T11 - T01 * T01;
  const double I00 = T11 / dt, I01 = (-T01) / dt, I11 = T00 / dt;               // its inverse, by the adjugate
  const double Q00 = A00 * I00 + A01 * I01, Q01 = A00 * I01 + A01 * I11;
  const double Q10 = A10 * I00 + A11 * I01, Q11 = A10 * I01 + A11 * I11;
  const double Q20 = A20 * I00 + A21 * I01, Q21 = A20 * I01 + A21 * I11;
  Rn[0] = Q00; Rn[1] = Q01; Rn[2] = Q10 * Q21 - Q20 * Q11;
  Rn[3] = Q10; Rn[4] = Q11; Rn[5] = Q20 * Q01 - Q00 * Q21;
  Rn[6] = Q20; Rn[7] = Q21; Rn[8] = Q00 * Q11 - Q10 * Q01;
  return d > 0.0;
}

PR_HD bool pr_pose_finite(const double* R, const double* t) {
  bool ok = true;
  for (int i = 0; i < 9; i++) ok = ok && pr_finite(R[i]);
  for (int i = 0; i < 3; i++) ok = ok && pr_finite(t[i]);
  return ok;
}

// The start of chain 1: the homography pose mirrored about the viewing ray to the tag, (2 c c^T - I) R_h diag(-1, -1, 1) with
// c = t_h / |t_h|.
PR_HD void pr_mirror_start(const double* Rh, const double* th, double* R1) {
  const double n = pr_sqrt((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]);
  const double c[3] = {th[0] / n, th[1] / n, th[2] / n};
  for (int i = 0; i < 3; i++) {
    const double m0 = 2.0 * (c[i] * c[0]) - (i == 0 ? 1.0 : 0.0), m1 = 2.0 * (c[i] * c[1]) - (i == 1 ? 1.0 : 0.0),
                 m2 = 2.0 * (c[i] * c[2]) - (i == 2 ? 1.0 : 0.0);
    R1[3 * i + 0] = -((m0 * Rh[0] + m1 * Rh[3]) + m2 * Rh[6]);
    R1[3 * i + 1] = -((m0 * Rh[1] + m1 * Rh[4]) + m2 * Rh[7]);
    R1[3 * i + 2] = (m0 * Rh[2] + m1 * Rh[5]) + m2 * Rh[8];
  }
}

// One chain: t = t(R) at the start, `iterations` steps with no early exit, E at the end.  False: the chain is degenerate -- some
// step's det S > 0 was false, or an entry of R or t after the start or after a step, or E, is not finite.
template <int NC, class Sum>
PR_HD bool pr_chain(const PrPoints<NC>& C, const double* Gi, const double* Rstart, uint32_t iterations, double npts, const Sum& sum,
                    double* R, double* t, double* E) {
  for (int i = 0; i < 9; i++) R[i] = Rstart[i];
  pr_translation<NC>(C, Gi, R, npts, sum, t);
  bool ok = pr_pose_finite(R, t);
  for (uint32_t it = 0; it < iterations; it++) {
    double Rn[9];
    const bool pos = pr_rotation<NC>(C, R, t, npts, sum, Rn);
    for (int i = 0; i < 9; i++) R[i] = Rn[i];
    if (POSE_T_FOLLOWS_STEP(it, iterations)) pr_translation<NC>(C, Gi, R, npts, sum, t);
    ok = ok && pos && pr_pose_finite(R, t);
  }
  *E = pr_error<NC>(C, R, t, sum);
  return ok && pr_finite(*E);
}

// The outcome: the chain with the smaller E, a tie to chain 0; the record of amdAprilTagsGetRefinedPoses.
PR_HD void pr_outcome(bool ok0, const double* R0, const double* t0, double E0, bool ok1, const double* R1, const double* t1, double E1,
                      const double* Rh, const double* th, double Eh, amdAprilTagsRefinedPose_t* o) {
  const bool second = ok0 && ok1 && E1 < E0;
  const bool alt = ok0 && ok1;
  o->status = !ok0 ? AMDAT_POSE_DEGENERATE : !ok1 ? AMDAT_POSE_REFINED_NO_ALT : AMDAT_POSE_REFINED;
  o->chosen = second ? 1u : 0u;
  for (int i = 0; i < 9; i++) o->R[i] = !ok0 ? Rh[i] : second ? R1[i] : R0[i];
  for (int i = 0; i < 3; i++) o->t[i] = !ok0 ? th[i] : second ? t1[i] : t0[i];
  o->err = !ok0 ? Eh : second ? E1 : E0;
  for (int i = 0; i < 9; i++) o->R_alt[i] = !alt ? 0.0 : second ? R0[i] : R1[i];
  for (int i = 0; i < 3; i++) o->t_alt[i] = !alt ? 0.0 : second ? t0[i] : t1[i];
  o->err_alt = !alt ? 0.0 : second ? E0 : E1;
  o->err_homography = Eh;
}

// One tag on one thread: the record of the four corners p under the frame's camera, from the homography pose (Rh, th).
PR_HD void pr_refine_tag(const double (*p)[2], double fx, double fy, double cx, double cy, double skew, double tag_size,
                         const double* Rh, const double* th, uint32_t iterations, amdAprilTagsRefinedPose_t* o) {
  const PrSumSerial sum;
  PrPoints<4> C;
  double Gi[6];
  pr_setup<4>(p, 0, fx, fy, cx, cy, skew, tag_size / 2.0, 4.0, sum, &C, Gi);
  const double Eh = pr_error<4>(C, Rh, th, sum);
  double Rm[9], Rs1[9];
  pr_mirror_start(Rh, th, Rm);
  for (int i = 0; i < 9; i++) Rs1[i] = POSE_CHAIN1_START(Rm[i], Rh[i]);
  double R0[9], t0[3], E0, R1[9], t1[3], E1;
  const bool ok0 = pr_chain<4>(C, Gi, Rh, iterations, 4.0, sum, R0, t0, &E0);
  const bool ok1 = pr_chain<4>(C, Gi, Rs1, iterations, 4.0, sum, R1, t1, &E1);
  pr_outcome(ok0, R0, t0, E0, ok1, R1, t1, E1, Rh, th, Eh, o);
}
