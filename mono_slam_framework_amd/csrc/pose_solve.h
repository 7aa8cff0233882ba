// The arithmetic of Optimizer::PoseOptimization (slam_pipeline/src/Optimizer.cc:217-334) and of the parts of g2o it
// drives: a pose-only Levenberg-Marquardt over EdgeSE3ProjectXYZOnlyPose edges with a Huber kernel, four rounds with a
// chi2 re-classification of every correspondence between them.  Plain C++ shared by pose_kernels.hip and by a host
// build (tests/cpp/pose_solve_host.cpp), so every stage can be checked against float64 numpy without a GPU.  Both
// builds use -ffp-contract=off; libm: sqrt, fabs, sin, cos.  Every step is in f64; points, pixels, intrinsics and the
// entry pose are f32 and are promoted on load.
//
// How the work is spread is the Team of pnp_solve.h: the 21 + 6 + 1 sums of an iteration (the upper triangle of H, b
// and the cost) and the cost of a trial go through team.sum -- a plain loop (Serial), 64 strided partial sums joined
// by a butterfly on the device (pose_kernels.hip), the same partial sums in the same order on the host (Emu64).  What
// follows the sums (Cholesky, exp, the lambda logic) is the same scalar code on every lane.
//
// g2o is not available where this was written: what is marked [M] restates it from memory.
//  [M] SE3Quat(R, t): Eigen's Quaternion(R) (the trace branch, else the largest diagonal element), then
//      normalizeRotation: w < 0 flips every sign, then the division by the norm.
//  [M] SE3Quat::exp(omega, upsilon): theta = |omega|; below 1e-5 R = I + Omega + Omega^2 and V = R; else Rodrigues,
//      V = I + (1 - cos) / theta^2 Omega + (theta - sin) / theta^3 Omega^2; the result is SE3Quat(Quaternion(R), V upsilon).
//      oplus: estimate = exp(dx) * estimate, a quaternion product followed by normalizeRotation.
//  [M] EdgeSE3ProjectXYZOnlyPose: e = obs - (f X / Z + c) with X = T Xw, and the 2 x 6 Jacobian of linearizeOplus.
//  [M] RobustKernelHuber: rho = e2, rho' = 1 for e2 <= delta^2 (delta * delta, not 5.991), else 2 delta sqrt(e2) - delta^2
//      and delta / sqrt(e2); H += rho' J'J, b -= rho' J'e, no second-order term; the cost is sum(rho).
//  [M] OptimizationAlgorithmLevenberg: lambda = 1e-5 max|diag H| and ni = 2 at iteration 0; a trial solves
//      (H + lambda I) dx = b; gain = (cost - cost_trial) / (dx . (lambda dx + b) + 1e-3); accepted iff gain > 0 and the
//      trial cost is finite; then lambda *= max(1/3, min(2/3, 1 - (2 gain - 1)^3)), ni = 2; else lambda *= ni, ni *= 2;
//      at most 10 trials; the run ends on an iteration that accepts nothing.
//  [M] LinearSolverDense: a 6 x 6 Cholesky (LDLT there; LL' here).
//
// Defined divergences from the reference:
//  * Every correspondence is classified at the estimate the round keeps.  g2o's active edges may still hold the error
//    of a last rejected trial (computeError() is repeated at :306 for the inactive edges only).
//  * A non-finite H or b, or a pivot that is not positive, rejects the trial outright and the estimate does not move.
//    g2o sets the trial cost to DBL_MAX and still applies whatever the solver left in x before restoring.
//  * A NaN gain rejects the trial and the next trial runs (g2o's do-while leaves on it: "rho < 0" is false).
//  * The run ends on an iteration whose trials were all rejected (ten of them, a gain of exactly 0, or a non-finite
//    lambda).  g2o as recalled also ends when the accepted trial was the tenth [M].
//  * A NaN chi2 compares as the reference's ">" does: not an outlier.  Hence a NaN pose flags nothing.
//  * Every loop is bounded: 4 rounds x 10 iterations x 10 trials, ceil(n / lanes) strides.
//  * A round with no active correspondence keeps SE3Quat(Tcw0) (g2o's optimize returns before its first iteration).
#ifndef MSF_POSE_SOLVE_H
#define MSF_POSE_SOLVE_H

#include <math.h>
#include <stdint.h>

#include "pnp_solve.h"

// full unrolling of a loop with a constant trip count, for either compiler
#if defined(__clang__)
#define MSF_POSE_UNROLL _Pragma("unroll")
#else
#define MSF_POSE_UNROLL _Pragma("GCC unroll 32")
#endif

namespace msf {
namespace pose {

constexpr int kRounds = 4, kIterations = 10, kTrials = 10;
constexpr int kSums = 28;                         // 21 of H's upper triangle, row-major; 6 of b; the cost
constexpr double kHuberDelta2 = 5.991;            // deltaMono = sqrt(5.991), :246
constexpr double kSmallAngle = 1e-5;
constexpr double kDblMax = 1.7976931348623157e308;

using pnp::Cam;

// the unit quaternion (x, y, z, w) and the translation of g2o's SE3Quat
struct Estimate {
  double q[4];
  double t[3];
};

MSF_HD bool finite(double x) { return fabs(x) <= kDblMax; }

// ---- SE3Quat ----
MSF_HD void normalise_rotation(double* q) {
  const double sign = q[3] < 0 ? -1.0 : 1.0;
  const double norm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; k++) q[k] = sign * q[k] / norm;
}

// Eigen's Quaternion(Matrix3): r is row-major 3 x 3 with a row stride of `ld`
MSF_HD void quaternion_of(const double* r, int ld, double* q) {
  const double r00 = r[0], r11 = r[ld + 1], r22 = r[2 * ld + 2];
  const double trace = r00 + r11 + r22;
  if (trace > 0) {
    double s = sqrt(trace + 1.0);
    q[3] = 0.5 * s;
    s = 0.5 / s;
    q[0] = (r[2 * ld + 1] - r[ld + 2]) * s;
    q[1] = (r[2] - r[2 * ld]) * s;
    q[2] = (r[ld] - r[1]) * s;
    return;
  }
  // i: the largest diagonal element, j and k follow it cyclically; selected without indexing by a variable
  const bool i1 = r11 > r00, i2 = r22 > (i1 ? r11 : r00);
  double dii, djj, dkk, kj, ji_ij, ki_ik;
  if (i2) {        // i = 2, j = 0, k = 1
    dii = r22, djj = r00, dkk = r11;
    kj = r[ld] - r[1], ji_ij = r[2] + r[2 * ld], ki_ik = r[ld + 2] + r[2 * ld + 1];
  } else if (i1) { // i = 1, j = 2, k = 0
    dii = r11, djj = r22, dkk = r00;
    kj = r[2] - r[2 * ld], ji_ij = r[2 * ld + 1] + r[ld + 2], ki_ik = r[1] + r[ld];
  } else {         // i = 0, j = 1, k = 2
    dii = r00, djj = r11, dkk = r22;
    kj = r[2 * ld + 1] - r[ld + 2], ji_ij = r[ld] + r[1], ki_ik = r[2 * ld] + r[2];
  }
  double s = sqrt(dii - djj - dkk + 1.0);
  const double qi = 0.5 * s;
  s = 0.5 / s;
  const double w = kj * s, qj = ji_ij * s, qk = ki_ik * s;
  q[3] = w;
  q[0] = i2 ? qj : i1 ? qk : qi;
  q[1] = i2 ? qk : i1 ? qi : qj;
  q[2] = i2 ? qi : i1 ? qj : qk;
}

// Converter::toSE3Quat of the f32 pose: rows 0..2 of Tcw, R | t row-major
MSF_HD Estimate estimate_of(const float* tcw) {
  double rt[12];
  for (int k = 0; k < 12; k++) rt[k] = (double)tcw[k];
  Estimate e;
  quaternion_of(rt, 4, e.q);
  normalise_rotation(e.q);
  e.t[0] = rt[3], e.t[1] = rt[7], e.t[2] = rt[11];
  return e;
}

// to_homogeneous_matrix, rows 0..2: Eigen's toRotationMatrix | t
MSF_HD void matrix_of(const Estimate& e, double* rt) {
  const double x = e.q[0], y = e.q[1], z = e.q[2], w = e.q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
               tyz = tz * y, tzz = tz * z;
  rt[0] = 1 - (tyy + tzz), rt[1] = txy - twz, rt[2] = txz + twy, rt[3] = e.t[0];
  rt[4] = txy + twz, rt[5] = 1 - (txx + tzz), rt[6] = tyz - twx, rt[7] = e.t[1];
  rt[8] = txz - twy, rt[9] = tyz + twx, rt[10] = 1 - (txx + tyy), rt[11] = e.t[2];
}

// sin and cos of x >= 0 in plain f64 multiplies and adds, so that every build that keeps the order and does not fuse
// (-ffp-contract=off) gives the same bits -- libm's sin and cos do not: a device's and a host's round some arguments
// differently in the last bit.  Cody-Waite reduction by pi / 2 in three pieces (exact products for k < 2^20) and the
// customary minimax polynomials on [-pi / 4, pi / 4]; within 1 ulp of the host's libm (tests/cpp/sin_cos_main.cpp).
// Beyond 1e5 rad, and for what is not finite, libm's own (no step of an optimisation gets there, and no parity is
// claimed).
MSF_HD void sin_cos(double x, double* s, double* c) {
  if (!(x <= 1e5)) {
    *s = sin(x), *c = cos(x);
    return;
  }
  double r = x;
  long long k = 0;
  if (x > 0.78539816339744828) {
    k = (long long)(x * 6.36619772367581382433e-01 + 0.5);
    const double fk = (double)k;
    r = ((x - fk * 1.57079632673412561417e+00) - fk * 6.07710050630396597660e-11) - fk * 2.02226624871116645580e-21;
  }
  const double z = r * r;
  const double ps = 8.33333333332248946124e-03 +
                    z * (-1.98412698298579493134e-04 +
                         z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
  const double sr = r + (z * r) * (-1.66666666666666324348e-01 + z * ps);
  const double pc = z * (4.16666666666666019037e-02 +
                         z * (-1.38888888888741095749e-03 +
                              z * (2.48015872894767294178e-05 +
                                   z * (-2.75573143513906633035e-07 +
                                        z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
  const double cr = 1.0 - (0.5 * z - z * pc);
  switch (k & 3) {
    case 0: *s = sr, *c = cr; break;
    case 1: *s = cr, *c = -sr; break;
    case 2: *s = -sr, *c = -cr; break;
    default: *s = -cr, *c = sr; break;
  }
}

// SE3Quat::exp of dx = (omega, upsilon): r row-major 3 x 3, t = V upsilon.  kOwnTrig: sin_cos() above instead of libm's
// (the bundle adjustments, whose host build the device has to match bit for bit).
template <bool kOwnTrig = false>
MSF_HD void se3_exp(const double* dx, double* r, double* t) {
  const double a = dx[0], b = dx[1], c = dx[2];
  const double theta = sqrt(a * a + b * b + c * c);
  // Omega = [0 -c b; c 0 -a; -b a 0], Omega^2 = omega omega' - theta^2 I written out
  const double o[9] = {0, -c, b, c, 0, -a, -b, a, 0};
  const double o2[9] = {-(b * b + c * c), a * b, a * c, a * b, -(a * a + c * c), b * c, a * c, b * c, -(a * a + b * b)};
  double kr1, kr2, kv1, kv2;
  if (theta < kSmallAngle) {
    kr1 = 1, kr2 = 1, kv1 = 1, kv2 = 1;
  } else {
    double s, co;
    if (kOwnTrig) sin_cos(theta, &s, &co);
    else s = sin(theta), co = cos(theta);
    const double th2 = theta * theta;
    kr1 = s / theta, kr2 = (1 - co) / th2;
    kv1 = (1 - co) / th2, kv2 = (theta - s) / (th2 * theta);
  }
  double v[9];
  for (int k = 0; k < 9; k++) {
    const double eye = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
    r[k] = eye + kr1 * o[k] + kr2 * o2[k];
    v[k] = eye + kv1 * o[k] + kv2 * o2[k];
  }
  for (int i = 0; i < 3; i++) t[i] = v[3 * i] * dx[3] + v[3 * i + 1] * dx[4] + v[3 * i + 2] * dx[5];
}

// oplus: exp(dx) * e
template <bool kOwnTrig = false>
MSF_HD Estimate moved(const Estimate& e, const double* dx) {
  double r[9], t[3], d[4];
  se3_exp<kOwnTrig>(dx, r, t);
  quaternion_of(r, 3, d);
  normalise_rotation(d);
  const double* q = e.q;
  Estimate m;
  m.q[3] = d[3] * q[3] - d[0] * q[0] - d[1] * q[1] - d[2] * q[2];
  m.q[0] = d[3] * q[0] + d[0] * q[3] + d[1] * q[2] - d[2] * q[1];
  m.q[1] = d[3] * q[1] + d[1] * q[3] + d[2] * q[0] - d[0] * q[2];
  m.q[2] = d[3] * q[2] + d[2] * q[3] + d[0] * q[1] - d[1] * q[0];
  normalise_rotation(m.q);
  // the rotation of exp(dx) applied to t: through the unit quaternion d, as SE3Quat's product does
  const Estimate rot{{d[0], d[1], d[2], d[3]}, {0, 0, 0}};
  double rd[12];
  matrix_of(rot, rd);
  for (int i = 0; i < 3; i++) m.t[i] = rd[4 * i] * e.t[0] + rd[4 * i + 1] * e.t[1] + rd[4 * i + 2] * e.t[2] + t[i];
  return m;
}

// ---- the edge ----
// the camera point of p under rt (R | t row-major 3 x 4) and e = obs - project
MSF_HD void edge_error(const double* rt, const Cam& cam, const double* p, const double* u, double* xc, double* e) {
  for (int r = 0; r < 3; r++) xc[r] = rt[4 * r] * p[0] + rt[4 * r + 1] * p[1] + rt[4 * r + 2] * p[2] + rt[4 * r + 3];
  e[0] = u[0] - (xc[0] / xc[2] * cam.fu + cam.uc);
  e[1] = u[1] - (xc[1] / xc[2] * cam.fv + cam.vc);
}

// the unrobustified chi2 = e'e (information: the identity)
MSF_HD double chi2_of(const double* rt, const Cam& cam, const double* p, const double* u) {
  double xc[3], e[2];
  edge_error(rt, cam, p, u, xc, e);
  return e[0] * e[0] + e[1] * e[1];
}

// :311, chi2 > chi2Mono[it] with the f32 constant promoted; false for a NaN
MSF_HD bool flagged(const double* rt, const Cam& cam, float chi2_max, const double* p, const double* u) {
  return chi2_of(rt, cam, p, u) > (double)chi2_max;
}

// RobustKernelHuber::robustify, or the plain square
MSF_HD void robustify(bool huber, double e2, double* rho, double* weight) {
  const double delta = sqrt(kHuberDelta2), dsqr = delta * delta;
  if (!huber || e2 <= dsqr) {
    *rho = e2, *weight = 1.0;
    return;
  }
  const double sqrte = sqrt(e2);
  *rho = 2 * sqrte * delta - dsqr;
  *weight = delta / sqrte;
}

// one correspondence's 28 terms: rho' J'J (upper triangle, row-major), -rho' J'e, rho
MSF_HD void edge_terms(const double* rt, const Cam& cam, bool huber, const double* p, const double* u, double* add) {
  double xc[3], e[2];
  edge_error(rt, cam, p, u, xc, e);
  const double x = xc[0], y = xc[1], invz = 1.0 / xc[2], invz2 = invz * invz;
  const double j0[6] = {x * y * invz2 * cam.fu, -(1 + x * x * invz2) * cam.fu, y * invz * cam.fu, -invz * cam.fu, 0.0,
                        x * invz2 * cam.fu};
  const double j1[6] = {(1 + y * y * invz2) * cam.fv, -x * y * invz2 * cam.fv, -x * invz * cam.fv, 0.0, -invz * cam.fv,
                        y * invz2 * cam.fv};
  double rho, w;
  robustify(huber, e[0] * e[0] + e[1] * e[1], &rho, &w);
  int at = 0;
  for (int r = 0; r < 6; r++)
    for (int c = r; c < 6; c++) add[at++] = w * (j0[r] * j0[c] + j1[r] * j1[c]);
  for (int r = 0; r < 6; r++) add[21 + r] = -(w * (j0[r] * e[0] + j1[r] * e[1]));
  add[27] = rho;
}

MSF_HD double edge_cost(const double* rt, const Cam& cam, bool huber, const double* p, const double* u) {
  double rho, w;
  robustify(huber, chi2_of(rt, cam, p, u), &rho, &w);
  return rho;
}

// ---- the correspondences of a round ----
// The edges are the correspondences the mask lets in; a round's active edges are those the previous round's pose
// (`previous`, R | t, held by value so that it stays in registers; none in round 0) did not flag.  The flag is
// recomputed where it is needed (some twenty operations), so no lane ever reads a flag another lane wrote.
struct Edges {
  const float* p3d;
  const float* p2d;
  const uint8_t* mask;
  int n;
  Cam cam;
  float chi2_max;
  bool has_previous;
  double previous[12];
  MSF_HD int count() const { return n; }
  MSF_HD bool edge(int i, double* p, double* u) const {
    if (mask && !mask[i]) return false;
    p[0] = p3d[3 * i], p[1] = p3d[3 * i + 1], p[2] = p3d[3 * i + 2];
    u[0] = p2d[2 * i], u[1] = p2d[2 * i + 1];
    return true;
  }
  MSF_HD bool get(int i, double* p, double* u) const {
    if (!edge(i, p, u)) return false;
    return !(has_previous && flagged(previous, cam, chi2_max, p, u));
  }
};

// the same list with every edge taking part
MSF_HD Edges all_edges(const Edges& e) {
  Edges a = e;
  a.has_previous = false;
  return a;
}

template <class Team>
MSF_HD int count_edges(const Team& team, const Edges& edges) {
  double k;
  team.template sum<1>(edges, [](const double*, const double*, double* add) { add[0] = 1.0; }, &k);
  return (int)k;
}

// how many edges rt flags (:299-318: every edge, the inactive ones too)
template <class Team>
MSF_HD int count_flagged(const Team& team, const Edges& edges, const double* rt) {
  double k;
  const Cam cam = edges.cam;
  const float chi2_max = edges.chi2_max;
  team.template sum<1>(all_edges(edges),
                       [rt, cam, chi2_max](const double* p, const double* u, double* add) {
                         add[0] = flagged(rt, cam, chi2_max, p, u) ? 1.0 : 0.0;
                       },
                       &k);
  return (int)k;
}

// H (21), b (6) and the cost of the active edges at e
template <class Team>
MSF_HD void build_system(const Team& team, const Edges& edges, bool huber, const Estimate& e, double* sums) {
  double rt[12];
  matrix_of(e, rt);
  const double* at = rt;
  const Cam cam = edges.cam;
  team.template sum<kSums>(edges,
                           [at, cam, huber](const double* p, const double* u, double* add) {
                             edge_terms(at, cam, huber, p, u, add);
                           },
                           sums);
}

template <class Team>
MSF_HD double cost_at(const Team& team, const Edges& edges, bool huber, const Estimate& e) {
  double rt[12], cost;
  matrix_of(e, rt);
  const double* at = rt;
  const Cam cam = edges.cam;
  team.template sum<1>(edges,
                       [at, cam, huber](const double* p, const double* u, double* add) {
                         add[0] = edge_cost(at, cam, huber, p, u);
                       },
                       &cost);
  return cost;
}

// (H + lambda I) dx = b by Cholesky; false: a non-finite entry or a pivot that is not positive.  Every loop has a
// constant trip count and is unrolled, so that the indices are static and the factor stays in registers.
MSF_HD bool solve_step(const double* sums, double lambda, double* dx) {
  bool ok = finite(lambda);
  MSF_POSE_UNROLL
  for (int k = 0; k < 27; k++) ok = ok && finite(sums[k]);
  if (!ok) return false;
  double l[6][6];   // the lower triangle
  MSF_POSE_UNROLL
  for (int r = 0; r < 6; r++) {
    MSF_POSE_UNROLL
    for (int c = 0; c < 6; c++)
      if (c >= r) l[c][r] = sums[r * 6 - r * (r - 1) / 2 + (c - r)] + (r == c ? lambda : 0.0);
  }
  MSF_POSE_UNROLL
  for (int j = 0; j < 6; j++) {
    double d = l[j][j];
    MSF_POSE_UNROLL
    for (int k = 0; k < 6; k++)
      if (k < j) d -= l[j][k] * l[j][k];
    ok = ok && d > 0 && finite(d);
    d = sqrt(d);
    l[j][j] = d;
    MSF_POSE_UNROLL
    for (int i = 0; i < 6; i++) {
      if (i <= j) continue;
      double s = l[i][j];
      MSF_POSE_UNROLL
      for (int k = 0; k < 6; k++)
        if (k < j) s -= l[i][k] * l[j][k];
      l[i][j] = s / d;
    }
  }
  if (!ok) return false;   // after the factorisation: a failed pivot only poisons what follows it
  double y[6];
  MSF_POSE_UNROLL
  for (int i = 0; i < 6; i++) {
    double s = sums[21 + i];
    MSF_POSE_UNROLL
    for (int k = 0; k < 6; k++)
      if (k < i) s -= l[i][k] * y[k];
    y[i] = s / l[i][i];
  }
  MSF_POSE_UNROLL
  for (int i = 5; i >= 0; i--) {
    double s = y[i];
    MSF_POSE_UNROLL
    for (int k = 0; k < 6; k++)
      if (k > i) s -= l[k][i] * dx[k];
    dx[i] = s / l[i][i];
  }
  return true;
}

// Where a list's diagnostics go (msf_pose_result's per-round and per-iteration arrays at this list), any of them null.
// Only the team's `leader` stores.
struct Trace {
  double* round_pose_f64;      // [4][12]
  int32_t* round_n_bad;        // [4]
  int32_t* round_iterations;   // [4]
  int32_t* it_trials;          // [4][10]
  double* it_lambda_in;
  double* it_lambda_out;
  double* it_cost_in;
  double* it_cost_out;
  double* it_H;                // [4][10][21]
  double* it_b;                // [4][10][6]
  double* it_pose_out;         // [4][10][7]
  bool leader;
};

// One iteration of OptimizationAlgorithmLevenberg::solve: the system once at the entry estimate, then trials until one
// is accepted.  -> the number of trials, negated when none was accepted (the run ends).  `slot` = round * 10 + iteration.
template <class Team>
MSF_HD int iteration(const Team& team, const Edges& edges, bool huber, bool first, Estimate* e, double* lambda,
                     double* ni, const Trace& tr, int slot) {
  double sums[kSums];
  build_system(team, edges, huber, *e, sums);
  const double cost = sums[27];
  if (first) {
    double top = 0.0;
    const int diag[6] = {0, 6, 11, 15, 18, 20};
    for (int k = 0; k < 6; k++) top = fabs(sums[diag[k]]) > top ? fabs(sums[diag[k]]) : top;
    *lambda = 1e-5 * top;
    *ni = 2.0;
  }
  const double lambda_in = *lambda;
  double cost_out = cost;
  int trials = 0;
  bool accepted = false;
  while (trials < kTrials && !accepted) {
    trials++;
    double dx[6], gain = -1.0, trial_cost = kDblMax;
    Estimate trial = *e;
    const bool solved = solve_step(sums, *lambda, dx);
    if (solved) {
      trial = moved(*e, dx);
      trial_cost = cost_at(team, edges, huber, trial);
      double scale = 1e-3;
      for (int k = 0; k < 6; k++) scale += dx[k] * (*lambda * dx[k] + sums[21 + k]);
      gain = (cost - trial_cost) / scale;
    }
    if (solved && gain > 0 && finite(trial_cost)) {
      const double y = 2 * gain - 1;
      double alpha = 1.0 - y * y * y;
      alpha = alpha < 2.0 / 3.0 ? alpha : 2.0 / 3.0;
      *lambda *= alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0;
      *ni = 2.0;
      *e = trial;
      cost_out = trial_cost;
      accepted = true;
    } else {
      *lambda *= *ni;
      *ni *= 2.0;
      if (!finite(*lambda) || gain == 0) break;
    }
  }
  if (tr.leader) {
    if (tr.it_trials) tr.it_trials[slot] = trials;
    if (tr.it_lambda_in) tr.it_lambda_in[slot] = lambda_in;
    if (tr.it_lambda_out) tr.it_lambda_out[slot] = *lambda;
    if (tr.it_cost_in) tr.it_cost_in[slot] = cost;
    if (tr.it_cost_out) tr.it_cost_out[slot] = cost_out;
    if (tr.it_H)
      for (int k = 0; k < 21; k++) tr.it_H[slot * 21 + k] = sums[k];
    if (tr.it_b)
      for (int k = 0; k < 6; k++) tr.it_b[slot * 6 + k] = sums[21 + k];
    if (tr.it_pose_out) {
      for (int k = 0; k < 4; k++) tr.it_pose_out[slot * 7 + k] = e->q[k];
      for (int k = 0; k < 3; k++) tr.it_pose_out[slot * 7 + 4 + k] = e->t[k];
    }
  }
  return accepted ? trials : -trials;
}

// optimizer.optimize(10) -> the iterations run
template <class Team>
MSF_HD int optimize(const Team& team, const Edges& edges, bool huber, Estimate* e, const Trace& tr, int round) {
  double lambda = 0.0, ni = 2.0;
  int it = 0;
  while (it < kIterations) {
    const int trials = iteration(team, edges, huber, it == 0, e, &lambda, &ni, tr, round * kIterations + it);
    it++;
    if (trials < 0) break;
  }
  return it;
}

struct Outcome {
  int n_good;
  int n_edges;
  int rounds_run;
  double pose[12];   // R | t of the last round's estimate; Tcw0 promoted when no round ran
};

// PoseOptimization on one list.  The flags of the result are flagged(pose, ...) of every edge when rounds_run > 0, and
// clear otherwise: the caller writes them, each index by the lane that owns it.
template <class Team>
MSF_HD Outcome pose_optimization(const Team& team, Edges edges, const float* tcw0, const Trace& tr) {
  Outcome out;
  edges.has_previous = false;
  out.n_edges = count_edges(team, edges);
  out.rounds_run = 0;
  out.n_good = 0;
  for (int k = 0; k < 12; k++) out.pose[k] = (double)tcw0[k];
  if (tr.leader) {
    for (int k = 0; k < kRounds * kIterations; k++)
      if (tr.it_trials) tr.it_trials[k] = 0;
    for (int k = 0; k < kRounds; k++) {
      if (tr.round_n_bad) tr.round_n_bad[k] = 0;
      if (tr.round_iterations) tr.round_iterations[k] = 0;
    }
  }
  if (out.n_edges < 3) return out;                       // :285
  const int rounds = out.n_edges < 10 ? 1 : kRounds;     // :323
  for (int round = 0; round < rounds; round++) {
    Estimate e = estimate_of(tcw0);                      // :295
    const int active = count_edges(team, edges);
    const int its = active ? optimize(team, edges, round < 3, &e, tr, round) : 0;
    matrix_of(e, out.pose);
    const int n_bad = count_flagged(team, edges, out.pose);
    for (int k = 0; k < 12; k++) edges.previous[k] = out.pose[k];
    edges.has_previous = true;
    out.n_good = out.n_edges - n_bad;
    out.rounds_run = round + 1;
    if (tr.leader) {
      if (tr.round_pose_f64)
        for (int k = 0; k < 12; k++) tr.round_pose_f64[round * 12 + k] = out.pose[k];
      if (tr.round_n_bad) tr.round_n_bad[round] = n_bad;
      if (tr.round_iterations) tr.round_iterations[round] = its;
    }
  }
  return out;
}

// ---- the whole call on the host, one thread: what tests/cpp/pose_solve_host.cpp exports ----
struct HostOut {
  int32_t* n_edges;
  int32_t* rounds_run;
  float* Tcw;          // [12]
  double* pose_f64;    // [12]
  uint8_t* outliers;   // [n], written where masked in
  Trace trace;
};

template <class Team>
inline int optimize_host(const Team& team, int n, const float* p3d, const float* p2d, const uint8_t* mask,
                         const Cam& cam, float chi2_max, const float* tcw0, const HostOut& o) {
  const Edges edges{p3d, p2d, mask, n, cam, chi2_max, false, {}};
  const Outcome r = pose_optimization(team, edges, tcw0, o.trace);
  if (o.n_edges) *o.n_edges = r.n_edges;
  if (o.rounds_run) *o.rounds_run = r.rounds_run;
  for (int k = 0; k < 12; k++) {
    if (o.pose_f64) o.pose_f64[k] = r.pose[k];
    if (o.Tcw) o.Tcw[k] = r.rounds_run ? (float)r.pose[k] : tcw0[k];
  }
  if (o.outliers)
    for (int i = 0; i < n; i++) {
      double p[3], u[2];
      if (!edges.edge(i, p, u)) continue;
      o.outliers[i] = r.rounds_run && flagged(r.pose, cam, chi2_max, p, u) ? 1 : 0;
    }
  return r.n_good;
}

}  // namespace pose
}  // namespace msf
#endif  // MSF_POSE_SOLVE_H
