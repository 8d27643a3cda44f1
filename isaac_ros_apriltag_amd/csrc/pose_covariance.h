// pose_covariance.h -- the first-order covariance of a reported pose (amdAprilTagsSetPoseCovariance): the
// Jacobian of the pixel projection of every point with respect to x = (dt_x, dt_y, dt_z, dtheta_x, dtheta_y, dtheta_z), the
// perturbation t' = t + dt, R' = Exp(dtheta) R of ROS' PoseWithCovariance in the camera optical frame; the normal matrix N = J^T J;
// and cov = sigma^2 N^-1 by a Cholesky factor and its inverse.  Stated once, in plain double-precision operations, for
// k_pose_refine<true> (kernels_pose.h), k_bundle_rigid<true> (kernels_rigid.h) and for a host compiler, in the manner of
// pose_refine.h and rigid_pose.h, whose square root and finiteness test are used as they stand: every function here is
// __host__ __device__ under hipcc and an ordinary inline function under g++ (tests/aux_c/pose_cov_driver.cpp compiles these lines
// with -ffp-contract=off; tests/pose_cov_ref.py states them in Python floats).
// Every operator is one IEEE operation in the order written: no re-association, no fused multiply-add, no library call but the
// correctly rounded square root.
//
// The per-point statements are loops over the NC points a thread holds, and every sum over the points goes through `sum`: the
// caller's PrSumSerial / PrSumQuad (a tag: four corners) or RgSumTree / RgSumWave (a bundle: 64 slots of four, an unused slot +0.0).
// The covariance is a pure function of (pose, points, camera, sigma): it is evaluated at whatever pose a record reports.
#pragma once
#include <string.h>

#include "rigid_pose.h"

#if defined(__HIPCC__)
#define PC_UNROLL _Pragma("unroll")
#else
#define PC_UNROLL
#endif

// entry (i, j), i >= j, of a symmetric or lower-triangular 6 x 6 matrix kept as its 21 distinct entries, row by row
#define PC_IX(i, j) ((i) * ((i) + 1) / 2 + (j))

// The 21 distinct entries of N = sum over the points of (J_u^T J_u + J_v^T J_v) at the pose (R, t), and *sq, the sum over the points
// of the squared pixel residual (u - pix_u)^2 + (v - pix_v)^2.  Point j: the object point (px[j], py[j], pz[j]), the pixel pix[j].
template <int NC, class Sum>
PR_HD void pc_normal(const double* px, const double* py, const double* pz, const double (*pix)[2], const double* R, const double* t,
                     double fx, double fy, double cx, double cy, double skew, const Sum& sum, double* N, double* sq) {
  double Ju[6][NC], Jv[6][NC], m[NC];
  PC_UNROLL
  for (int j = 0; j < NC; j++) {
    const double W0 = (R[0] * px[j] + R[1] * py[j]) + R[2] * pz[j];
    const double W1 = (R[3] * px[j] + R[4] * py[j]) + R[5] * pz[j];
    const double W2 = (R[6] * px[j] + R[7] * py[j]) + R[8] * pz[j];
    const double X0 = W0 + t[0], X1 = W1 + t[1], X2 = W2 + t[2];
    const double iz = 1.0 / X2;
    const double g = fx * X0 + skew * X1, h = fy * X1;
    const double a = fx * iz, b = skew * iz, c = fy * iz;
    const double d = -((g * iz) * iz), e = -((h * iz) * iz);
    const double bu = POSE_COV_JU_SKEW(b);
    Ju[0][j] = a; Ju[1][j] = bu; Ju[2][j] = d;
    Ju[3][j] = d * W1 - bu * W2; Ju[4][j] = a * W2 - d * W0; Ju[5][j] = bu * W0 - a * W1;
    Jv[0][j] = 0.0; Jv[1][j] = c; Jv[2][j] = e;
    Jv[3][j] = e * W1 - c * W2; Jv[4][j] = -(e * W0); Jv[5][j] = c * W0;
    const double du = (g / X2 + cx) - pix[j][0], dv = (h / X2 + cy) - pix[j][1];
    m[j] = du * du + dv * dv;
  }
  *sq = sum(m);
  PC_UNROLL
  for (int r = 0; r < 6; r++) {
    PC_UNROLL
    for (int s = 0; s <= r; s++) {
      PC_UNROLL
      for (int j = 0; j < NC; j++) m[j] = Ju[r][j] * Ju[s][j] + Jv[r][j] * Jv[s][j];
      N[PC_IX(r, s)] = sum(m);
    }
  }
}

// cov = sigma2 * N^-1, all 36 entries row-major and exactly symmetric: the Cholesky factor N = L L^T column by column, M = L^-1 by
// forward substitution, the 21 distinct entries of M^T M.  Every inner sum adds its terms in ascending k, starting from the first
// term.  A pivot is accepted only while pivot > 0.0 and it is finite.  False -- a refused pivot, or an entry of the result that is
// not finite --: cov is 36 zeros.  The operation count is fixed: a refused pivot only clears the outcome.
PR_HD bool pc_invert(const double* N, double sigma2, double* cov) {
  double L[21], M[21];
  bool ok = true;
  PC_UNROLL
  for (int j = 0; j < 6; j++) {
    double pivot = N[PC_IX(j, j)];
    if (j > 0) {
      double acc = L[PC_IX(j, 0)] * L[PC_IX(j, 0)];
      PC_UNROLL
      for (int k = 1; k < j; k++) acc = acc + L[PC_IX(j, k)] * L[PC_IX(j, k)];
      pivot = pivot - acc;
    }
    ok = ok && pivot > 0.0 && pr_finite(pivot);
    const double ljj = pr_sqrt(pivot);
    L[PC_IX(j, j)] = ljj;
    PC_UNROLL
    for (int i = j + 1; i < 6; i++) {
      double v = N[PC_IX(i, j)];
      if (j > 0) {
        double acc = L[PC_IX(i, 0)] * L[PC_IX(j, 0)];
        PC_UNROLL
        for (int k = 1; k < j; k++) acc = acc + L[PC_IX(i, k)] * L[PC_IX(j, k)];
        v = v - acc;
      }
      L[PC_IX(i, j)] = v / ljj;
    }
  }
  PC_UNROLL
  for (int j = 0; j < 6; j++) {
    M[PC_IX(j, j)] = 1.0 / L[PC_IX(j, j)];
    PC_UNROLL
    for (int i = j + 1; i < 6; i++) {
      double acc = L[PC_IX(i, j)] * M[PC_IX(j, j)];
      PC_UNROLL
      for (int k = j + 1; k < i; k++) acc = acc + L[PC_IX(i, k)] * M[PC_IX(k, j)];
      M[PC_IX(i, j)] = (-acc) / L[PC_IX(i, i)];
    }
  }
  double c[21];
  PC_UNROLL
  for (int r = 0; r < 6; r++) {
    PC_UNROLL
    for (int s = 0; s <= r; s++) {   // (M^T M)_rs = sum over k >= r of M_kr M_ks
      double acc = M[PC_IX(r, r)] * M[PC_IX(r, s)];
      PC_UNROLL
      for (int k = r + 1; k < 6; k++) acc = acc + M[PC_IX(k, r)] * M[PC_IX(k, s)];
      c[PC_IX(r, s)] = sigma2 * acc;
      ok = ok && pr_finite(c[PC_IX(r, s)]);
    }
  }
  PC_UNROLL
  for (int r = 0; r < 6; r++) {
    PC_UNROLL
    for (int s = 0; s < 6; s++) cov[6 * r + s] = ok ? (s <= r ? c[PC_IX(r, s)] : c[PC_IX(s, r)]) : 0.0;
  }
  return ok;
}

#if !defined(__HIPCC__)
// The covariance record of one tag on one host thread: at the refined record's (R, t), and at (R_alt, t_alt) where it has an
// alternative (status AMDAT_POSE_REFINED); elsewhere the alternative half is zero with its valid bit clear.
static inline void pc_tag_record(const double (*p)[2], double fx, double fy, double cx, double cy, double skew, double tag_size,
                                 const amdAprilTagsRefinedPose_t* o, double sigma2, amdAprilTagsPoseCovariance_t* c) {
  const PrSumSerial sum;
  const double s = tag_size / 2.0;
  const double px[4] = {s * -1.0, s * 1.0, s * 1.0, s * -1.0}, py[4] = {s * 1.0, s * 1.0, s * -1.0, s * -1.0}, pz[4] = {0.0, 0.0, 0.0, 0.0};
  double N[21];
  c->valid = 0u;
  c->reserved = 0u;
  pc_normal<4>(px, py, pz, p, o->R, o->t, fx, fy, cx, cy, skew, sum, N, &c->sq_err_sum);
  if (pc_invert(N, sigma2, c->cov)) c->valid |= 1u;
  if (o->status == AMDAT_POSE_REFINED) {
    pc_normal<4>(px, py, pz, p, o->R_alt, o->t_alt, fx, fy, cx, cy, skew, sum, N, &c->sq_err_sum_alt);
    if (pc_invert(N, sigma2, c->cov_alt)) c->valid |= 2u;
  } else {
    for (int i = 0; i < 36; i++) c->cov_alt[i] = 0.0;
    c->sq_err_sum_alt = 0.0;
  }
}

// The covariance record of one bundle of one frame on one host thread: slot s < ntags holds the used record's corners pix[4 s + k]
// and its member's corners obj[4 s + k], as rg_solve_host's; o: the bundle's pose record.  An alternative exists where both chains
// ran, which the record shows as a non-zero R_alt.  The two residual fields stay zero: the pose record carries them.
static inline void pc_bundle_record(uint32_t ntags, const double (*pix)[2], const double (*obj)[3], double fx, double fy, double cx, double cy,
                                    double skew, const amdAprilTagsBundlePoseEx_t* o, double sigma2, amdAprilTagsPoseCovariance_t* c) {
  memset(c, 0, sizeof(*c));
  if (o->status == AMDAT_BUNDLE_TOO_FEW_TAGS) return;
  const RgSumTree sum = {ntags};
  static thread_local double px[4 * RG_SLOTS], py[4 * RG_SLOTS], pz[4 * RG_SLOTS];
  for (int j = 0; j < 4 * RG_SLOTS; j++) { px[j] = obj[j][0]; py[j] = obj[j][1]; pz[j] = obj[j][2]; }
  double N[21], sq;
  pc_normal<4 * RG_SLOTS>(px, py, pz, pix, o->R, o->t, fx, fy, cx, cy, skew, sum, N, &sq);
  if (pc_invert(N, sigma2, c->cov)) c->valid |= 1u;
  bool alt = false;
  for (int i = 0; i < 9; i++) alt = alt || o->R_alt[i] != 0.0;
  if (alt) {
    pc_normal<4 * RG_SLOTS>(px, py, pz, pix, o->R_alt, o->t_alt, fx, fy, cx, cy, skew, sum, N, &sq);
    if (pc_invert(N, sigma2, c->cov_alt)) c->valid |= 2u;
  }
}
#endif
