// rigid_pose.h -- the pose of a rigid 3-D tag bundle (amdAprilTagsSetBundlesEx): the object-space iteration of
// Lu, Hager and Mjolsness over the n = 4 * ntags general points of the used tags, run as two independent chains -- one from the seed
// tag's homography pose, one from its mirror about the viewing ray, both composed with the inverse of the seed member's pose -- and
// the outcome rule that picks between them.  Stated once, in plain double-precision operations, for k_bundle_rigid
// (kernels_rigid.h) and for a host compiler, in the manner of pose_refine.h, whose square root, finiteness test and mirror start
// are used as they stand: every function here is __host__ __device__ under hipcc and an ordinary inline function under g++
// (tests/aux_c/rigid_pose_driver.cpp compiles these lines with -ffp-contract=off; tests/rigid_bundle_ref.py states them in Python).
// Every operator is one IEEE operation in the order written: no re-association, no fused multiply-add, no library call but the
// correctly rounded square root.
//
// The per-point statements are loops over the NC points a thread holds, and every sum over the points goes through `sum`.  The 64
// tag slots hold four corners each; slot s is used while s < ntags, and an unused slot contributes +0.0.  A lane of k_bundle_rigid
// holds one slot (NC = 4): its `sum` adds the slot's four values as (x0 + x1) + (x2 + x3) and then runs a six-step butterfly over
// the wave, which pairs the slots as a balanced binary tree and leaves the same bits on every lane (addition commutes).  The host
// holds all 64 slots (NC = 256, RgSumTree) and walks the same tree.
#pragma once
#include "pose_refine.h"

#define RG_SLOTS 64          // tag slots: AMDAT_MAX_RIGID_BUNDLE_MEMBERS, the lanes of a wave
#define RG_JACOBI_SWEEPS 5   // cyclic sweeps over the symmetric 3 x 3 matrix M^T M (DESIGN.md section 7f has the table behind the count)

struct RgSumTree {
  uint32_t ntags;
  PR_HD_MEMBER double operator()(const double* x) const {
    double v[RG_SLOTS];
    for (uint32_t s = 0; s < RG_SLOTS; s++) v[s] = s < ntags ? (x[4 * s] + x[4 * s + 1]) + (x[4 * s + 2] + x[4 * s + 3]) : 0.0;
    for (uint32_t n = RG_SLOTS / 2; n >= 1; n /= 2)
      for (uint32_t s = 0; s < n; s++) v[s] = v[2 * s] + v[2 * s + 1];
    return v[0];
  }
};

// What a thread holds of its NC points: the six distinct entries of the projector F = v v^T / (v^T v) onto the point's viewing ray
// v = (un, vn, 1), the object point P in the bundle frame, and P - mean P.
template <int NC>
struct RgPoints {
  double F00[NC], F01[NC], F02[NC], F11[NC], F12[NC], F22[NC];
  double px[NC], py[NC], pz[NC];
  double cx[NC], cy[NC], cz[NC];
};

// pix[j]: the pixel (u, v) of point j, obj[j]: its object point.  Fills the points and Gi, the six distinct entries
// (00, 01, 02, 11, 12, 22) of the inverse of G = I - (sum F) / npts, by cofactors.
template <int NC, class Sum>
PR_HD void rg_setup(const double (*pix)[2], const double (*obj)[3], double fx, double fy, double cx, double cy, double skew, double npts,
                    const Sum& sum, RgPoints<NC>* C, double* Gi) {
  for (int j = 0; j < NC; j++) {
    C->px[j] = obj[j][0]; C->py[j] = obj[j][1]; C->pz[j] = obj[j][2];
    const double vn = (pix[j][1] - cy) / fy;
    const double un = ((pix[j][0] - cx) - skew * vn) / fx;
    const double nn = (un * un + vn * vn) + 1.0;
    C->F00[j] = (un * un) / nn; C->F01[j] = (un * vn) / nn; C->F02[j] = un / nn;
    C->F11[j] = (vn * vn) / nn; C->F12[j] = vn / nn; C->F22[j] = 1.0 / nn;
  }
  const double mx = sum(C->px) / npts, my = sum(C->py) / npts, mz = sum(C->pz) / npts;
  for (int j = 0; j < NC; j++) { C->cx[j] = C->px[j] - mx; C->cy[j] = C->py[j] - my; C->cz[j] = C->pz[j] - mz; }
  const double G00 = 1.0 - sum(C->F00) / npts, G01 = -(sum(C->F01) / npts), G02 = -(sum(C->F02) / npts);
  const double G11 = 1.0 - sum(C->F11) / npts, G12 = -(sum(C->F12) / npts), G22 = 1.0 - sum(C->F22) / npts;
  const double c00 = G11 * G22 - G12 * G12, c01 = G12 * G02 - G01 * G22, c02 = G01 * G12 - G11 * G02;
  const double c11 = G00 * G22 - G02 * G02, c12 = G01 * G02 - G00 * G12, c22 = G00 * G11 - G01 * G01;
  const double det = (G00 * c00 + G01 * c01) + G02 * c02;
  Gi[0] = c00 / det; Gi[1] = c01 / det; Gi[2] = c02 / det; Gi[3] = c11 / det; Gi[4] = c12 / det; Gi[5] = c22 / det;
}

// R P_j for point j
#define RG_RP(R, C, j, w0, w1, w2)                                                          \
  const double w0 = (R[0] * C.px[j] + R[1] * C.py[j]) + R[2] * C.pz[j];                     \
  const double w1 = (R[3] * C.px[j] + R[4] * C.py[j]) + R[5] * C.pz[j];                     \
  const double w2 = (R[6] * C.px[j] + R[7] * C.py[j]) + R[8] * C.pz[j];

// t(R) = G^-1 (sum (F_j - I) R P_j) / npts
template <int NC, class Sum>
PR_HD void rg_translation(const RgPoints<NC>& C, const double* Gi, const double* R, double npts, const Sum& sum, double* t) {
  double a0[NC], a1[NC], a2[NC];
  for (int j = 0; j < NC; j++) {
    RG_RP(R, C, j, w0, w1, w2)
    a0[j] = ((C.F00[j] * w0 + C.F01[j] * w1) + C.F02[j] * w2) - w0;
    a1[j] = ((C.F01[j] * w0 + C.F11[j] * w1) + C.F12[j] * w2) - w1;
    a2[j] = ((C.F02[j] * w0 + C.F12[j] * w1) + C.F22[j] * w2) - w2;
  }
  const double b0 = sum(a0) / npts, b1 = sum(a1) / npts, b2 = sum(a2) / npts;
  t[0] = (Gi[0] * b0 + Gi[1] * b1) + Gi[2] * b2;
  t[1] = (Gi[1] * b0 + Gi[3] * b1) + Gi[4] * b2;
  t[2] = (Gi[2] * b0 + Gi[4] * b1) + Gi[5] * b2;
}

// E(R, t) = sum |(I - F_j)(R P_j + t)|^2
template <int NC, class Sum>
PR_HD double rg_error(const RgPoints<NC>& C, const double* R, const double* t, const Sum& sum) {
  double e[NC];
  for (int j = 0; j < NC; j++) {
    RG_RP(R, C, j, w0, w1, w2)
    const double x0 = w0 + t[0], x1 = w1 + t[1], x2 = w2 + t[2];
    const double e0 = x0 - ((C.F00[j] * x0 + C.F01[j] * x1) + C.F02[j] * x2);
    const double e1 = x1 - ((C.F01[j] * x0 + C.F11[j] * x1) + C.F12[j] * x2);
    const double e2 = x2 - ((C.F02[j] * x0 + C.F12[j] * x1) + C.F22[j] * x2);
    e[j] = (e0 * e0 + e1 * e1) + e2 * e2;
  }
  return sum(e);
}

// One Jacobi rotation in the (P, Q) plane of the symmetric S (all nine entries kept), K the third index; V collects the rotations.
// A fixed operation count: the angle's tangent is 0 where S_PQ is 0.
template <int P, int Q, int K>
PR_HD void rg_jacobi(double* S, double* V) {
  const double apq = S[3 * P + Q], app = S[3 * P + P], aqq = S[3 * Q + Q];
  const double theta = (aqq - app) / (2.0 * apq);
  const double at = theta < 0.0 ? -theta : theta;
  const double tm = 1.0 / (at + pr_sqrt(theta * theta + 1.0));
  const double ts = theta < 0.0 ? -tm : tm;
  const double tt = apq == 0.0 ? 0.0 : ts;
  const double c = 1.0 / pr_sqrt(tt * tt + 1.0);
  const double s = tt * c;
  S[3 * P + P] = app - tt * apq;
  S[3 * Q + Q] = aqq + tt * apq;
  S[3 * P + Q] = 0.0; S[3 * Q + P] = 0.0;
  const double akp = S[3 * K + P], akq = S[3 * K + Q];
  const double nkp = c * akp - s * akq, nkq = s * akp + c * akq;
  S[3 * K + P] = nkp; S[3 * P + K] = nkp;
  S[3 * K + Q] = nkq; S[3 * Q + K] = nkq;
  for (int k = 0; k < 3; k++) {
    const double vp = V[3 * k + P], vq = V[3 * k + Q];
    V[3 * k + P] = c * vp - s * vq;
    V[3 * k + Q] = s * vp + c * vq;
  }
}

// The rotation that maximises tr(R^T M), determinant +1 whatever M's: RG_JACOBI_SWEEPS cyclic sweeps diagonalise S = M^T M, the
// columns v1, v2 of V with the two largest eigenvalues (a tie to the lower index) give u1 = M v1 / |M v1| and u2 = M v2, made
// orthogonal to u1 and normalised; u3 = u1 x u2, v3 = v1 x v2, and R = sum u_i v_i^T.  The third pair never reads M: a rank-2 M (a
// coplanar point set) is served as it stands, and a negative determinant puts the reflection on the smallest singular value, where
// the maximiser has it.  False where |M v1| > 0 is false: the leading singular value vanishes.
PR_HD bool rg_polar(const double* M, double* Rn) {
  double S[9], V[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) S[3 * i + j] = (M[i] * M[j] + M[3 + i] * M[3 + j]) + M[6 + i] * M[6 + j];
  for (int sweep = 0; sweep < RG_JACOBI_SWEEPS; sweep++) {
    rg_jacobi<0, 1, 2>(S, V);
    rg_jacobi<0, 2, 1>(S, V);
    rg_jacobi<1, 2, 0>(S, V);
  }
  const double l0 = S[0], l1 = S[4], l2 = S[8];
  const bool b1 = l1 > l0;
  const bool b2 = l2 > (b1 ? l1 : l0);
  const int i1 = b2 ? 2 : (b1 ? 1 : 0);
  const double la = i1 == 0 ? l1 : l0, lb = i1 == 2 ? l1 : l2;   // the other two, lower index first
  const int ia = i1 == 0 ? 1 : 0, ib = i1 == 2 ? 1 : 2;
  const int i2 = lb > la ? ib : ia;
  double v1[3], v2[3], u1[3], u2[3], w[3];
  for (int k = 0; k < 3; k++) {
    v1[k] = i1 == 0 ? V[3 * k] : i1 == 1 ? V[3 * k + 1] : V[3 * k + 2];
    v2[k] = i2 == 0 ? V[3 * k] : i2 == 1 ? V[3 * k + 1] : V[3 * k + 2];
  }
  for (int i = 0; i < 3; i++) w[i] = (M[3 * i] * v1[0] + M[3 * i + 1] * v1[1]) + M[3 * i + 2] * v1[2];
  const double n1 = pr_sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  for (int i = 0; i < 3; i++) u1[i] = w[i] / n1;
  for (int i = 0; i < 3; i++) w[i] = (M[3 * i] * v2[0] + M[3 * i + 1] * v2[1]) + M[3 * i + 2] * v2[2];
  const double d = (u1[0] * w[0] + u1[1] * w[1]) + u1[2] * w[2];
  for (int i = 0; i < 3; i++) w[i] = w[i] - d * u1[i];
  const double n2 = pr_sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  for (int i = 0; i < 3; i++) u2[i] = w[i] / n2;
  const double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
  const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Rn[3 * i + j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j];
  return n1 > 0.0;
}

// The rotation of one iteration: q_j = F_j (R P_j + t), M = sum (q_j - mean q)(P_j - mean P)^T, and its rotation by rg_polar.
template <int NC, class Sum>
PR_HD bool rg_rotation(const RgPoints<NC>& C, const double* R, const double* t, double npts, const Sum& sum, double* Rn) {
  double q0[NC], q1[NC], q2[NC], m[NC], M[9];
  for (int j = 0; j < NC; j++) {
    RG_RP(R, C, j, w0, w1, w2)
    const double x0 = w0 + t[0], x1 = w1 + t[1], x2 = w2 + t[2];
    q0[j] = (C.F00[j] * x0 + C.F01[j] * x1) + C.F02[j] * x2;
    q1[j] = (C.F01[j] * x0 + C.F11[j] * x1) + C.F12[j] * x2;
    q2[j] = (C.F02[j] * x0 + C.F12[j] * x1) + C.F22[j] * x2;
  }
  const double qb0 = sum(q0) / npts, qb1 = sum(q1) / npts, qb2 = sum(q2) / npts;
  for (int j = 0; j < NC; j++) { q0[j] = q0[j] - qb0; q1[j] = q1[j] - qb1; q2[j] = q2[j] - qb2; }
  for (int j = 0; j < NC; j++) m[j] = q0[j] * C.cx[j];
  M[0] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q0[j] * C.cy[j];
  M[1] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q0[j] * C.cz[j];
  M[2] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q1[j] * C.cx[j];
  M[3] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q1[j] * C.cy[j];
  M[4] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q1[j] * C.cz[j];
  M[5] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q2[j] * C.cx[j];
  M[6] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q2[j] * C.cy[j];
  M[7] = sum(m);
  for (int j = 0; j < NC; j++) m[j] = q2[j] * C.cz[j];
  M[8] = sum(m);
  return rg_polar(M, Rn);
}

// One chain: t = t(R) at the start, `iterations` steps with no early exit, E at the end.  False: the chain is degenerate -- some
// step's leading singular value vanished, or an entry of R or t after the start or after a step, or E, is not finite.
template <int NC, class Sum>
PR_HD bool rg_chain(const RgPoints<NC>& C, const double* Gi, const double* Rstart, uint32_t iterations, double npts, const Sum& sum,
                    double* R, double* t, double* E) {
  for (int i = 0; i < 9; i++) R[i] = Rstart[i];
  rg_translation<NC>(C, Gi, R, npts, sum, t);
  bool ok = pr_pose_finite(R, t);
  for (uint32_t it = 0; it < iterations; it++) {
    double Rn[9];
    const bool pos = rg_rotation<NC>(C, R, t, npts, sum, Rn);
    for (int i = 0; i < 9; i++) R[i] = Rn[i];
    rg_translation<NC>(C, Gi, R, npts, sum, t);
    ok = ok && pos && pr_pose_finite(R, t);
  }
  *E = rg_error<NC>(C, R, t, sum);
  return ok && pr_finite(*E);
}

// Twice the signed shoelace area of a record's corners in pixels, as its magnitude: what the seed is chosen by.
PR_HD double rg_area2(const double (*p)[2]) {
  const double a = ((p[0][0] * p[1][1] - p[1][0] * p[0][1]) + (p[1][0] * p[2][1] - p[2][0] * p[1][1])) +
                   ((p[2][0] * p[3][1] - p[3][0] * p[2][1]) + (p[3][0] * p[0][1] - p[0][0] * p[3][1]));
  return a < 0.0 ? -a : a;
}

// A tag's rotation in the camera frame composed with the inverse of its member's pose in the bundle frame: the bundle's rotation
// Rc Rm^T, and (ts non-null) the bundle's translation tc - (Rc Rm^T) tm.
PR_HD void rg_compose_start(const double* Rc, const double* tc, const double* Rm, const double* tm, double* Rs, double* ts) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Rs[3 * i + j] = (Rc[3 * i] * Rm[3 * j] + Rc[3 * i + 1] * Rm[3 * j + 1]) + Rc[3 * i + 2] * Rm[3 * j + 2];
  if (ts)
    for (int i = 0; i < 3; i++) ts[i] = tc[i] - ((Rs[3 * i] * tm[0] + Rs[3 * i + 1] * tm[1]) + Rs[3 * i + 2] * tm[2]);
}

// The squared pixel reprojection errors of one tag's four corners under (R, t) and the frame's camera, added as the planar record's.
PR_HD double rg_reprojection(const double (*pix)[2], const double (*obj)[3], const double* R, const double* t, double fx, double fy,
                             double cx, double cy, double skew) {
  double e[4];
  for (int k = 0; k < 4; k++) {
    const double xc = ((R[0] * obj[k][0] + R[1] * obj[k][1]) + R[2] * obj[k][2]) + t[0];
    const double yc = ((R[3] * obj[k][0] + R[4] * obj[k][1]) + R[5] * obj[k][2]) + t[1];
    const double zc = ((R[6] * obj[k][0] + R[7] * obj[k][1]) + R[8] * obj[k][2]) + t[2];
    const double xn = xc / zc, yn = yc / zc;
    const double u = (fx * xn + skew * yn) + cx;
    const double v = fy * yn + cy;
    const double du = u - pix[k][0], dv = v - pix[k][1];
    e[k] = du * du + dv * dv;
  }
  return ((e[0] + e[1]) + e[2]) + e[3];
}

// The outcome: of the chains that are not degenerate the one with the smaller E, a tie to chain 0; the other beside it where both
// ran.  Both degenerate: the seed start (Rs, ts) with its E, everything else zero.  sq0, sq1: the chains' pixel reprojection sums.
// Fills status, chosen and the pose fields of the record of amdAprilTagsGetBundlePosesEx; the counts and the seed are the caller's.
PR_HD void rg_outcome(bool ok0, const double* R0, const double* t0, double E0, double sq0, bool ok1, const double* R1, const double* t1,
                      double E1, double sq1, const double* Rs, const double* ts, double Es, amdAprilTagsBundlePoseEx_t* o) {
  const bool none = !ok0 && !ok1;
  const bool alt = ok0 && ok1;
  const bool second = ok1 && (!ok0 || E1 < E0);
  o->status = none ? AMDAT_BUNDLE_DEGENERATE : AMDAT_BUNDLE_SOLVED;
  o->chosen = second ? 1u : 0u;
  for (int i = 0; i < 9; i++) o->R[i] = none ? Rs[i] : second ? R1[i] : R0[i];
  for (int i = 0; i < 3; i++) o->t[i] = none ? ts[i] : second ? t1[i] : t0[i];
  o->err = none ? Es : second ? E1 : E0;
  o->sq_err_sum = none ? 0.0 : second ? sq1 : sq0;
  for (int i = 0; i < 9; i++) o->R_alt[i] = !alt ? 0.0 : second ? R0[i] : R1[i];
  for (int i = 0; i < 3; i++) o->t_alt[i] = !alt ? 0.0 : second ? t0[i] : t1[i];
  o->err_alt = !alt ? 0.0 : second ? E0 : E1;
  o->sq_err_sum_alt = !alt ? 0.0 : second ? sq0 : sq1;
}

#if !defined(__HIPCC__)
// One bundle of one frame on one host thread: slot s < ntags holds the used record's corners pix[4 s + k], its member's corners
// obj[4 s + k], and its homography pose (Rh + 9 s, th + 3 s) with its member's pose (Rm + 9 s, tm + 3 s).  Fills everything of the
// record but bundle, ntags, nskipped; `seed` comes back as the SLOT of the seed.  ntags in 1 .. RG_SLOTS.
static inline void rg_solve_host(uint32_t ntags, const double (*pix)[2], const double (*obj)[3], const double* Rh, const double* th,
                                 const double* Rm, const double* tm, double fx, double fy, double cx, double cy, double skew,
                                 uint32_t iterations, amdAprilTagsBundlePoseEx_t* o) {
  uint32_t seed = 0;
  double best = -1.0;
  for (uint32_t s = 0; s < ntags; s++) {
    const double a = rg_area2(pix + 4 * s);
    if (a > best) { best = a; seed = s; }
  }
  double Rs0[9], ts0[3], Rmir[9], Rs1[9];
  rg_compose_start(Rh + 9 * seed, th + 3 * seed, Rm + 9 * seed, tm + 3 * seed, Rs0, ts0);
  pr_mirror_start(Rh + 9 * seed, th + 3 * seed, Rmir);
  rg_compose_start(Rmir, (const double*)0, Rm + 9 * seed, tm + 3 * seed, Rs1, (double*)0);
  const RgSumTree sum = {ntags};
  const double npts = RIGID_NPTS(4.0 * (double)ntags);
  static thread_local RgPoints<4 * RG_SLOTS> C;
  double Gi[6];
  rg_setup<4 * RG_SLOTS>(pix, obj, fx, fy, cx, cy, skew, npts, sum, &C, Gi);
  const double Es = rg_error<4 * RG_SLOTS>(C, Rs0, ts0, sum);
  double R0[9], t0[3], E0, R1[9], t1[3], E1;
  const bool ok0 = rg_chain<4 * RG_SLOTS>(C, Gi, Rs0, iterations, npts, sum, R0, t0, &E0);
  const bool ok1 = rg_chain<4 * RG_SLOTS>(C, Gi, Rs1, iterations, npts, sum, R1, t1, &E1);
  double sq0 = 0.0, sq1 = 0.0;
  for (uint32_t s = 0; s < ntags; s++) {
    sq0 = sq0 + rg_reprojection(pix + 4 * s, obj + 4 * s, R0, t0, fx, fy, cx, cy, skew);
    sq1 = sq1 + rg_reprojection(pix + 4 * s, obj + 4 * s, R1, t1, fx, fy, cx, cy, skew);
  }
  rg_outcome(ok0, R0, t0, E0, sq0, ok1, R1, t1, E1, sq1, Rs0, ts0, Es, o);
  o->seed = seed;
}
#endif
