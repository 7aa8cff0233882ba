// The arithmetic of Optimizer::LocalBundleAdjustment (slam_pipeline/src/Optimizer.cc:336-574) and
// Optimizer::BundleAdjustment (:71-215) and of the parts of g2o they drive: a Levenberg-Marquardt over SE3 poses and
// 3-D points joined by EdgeSE3ProjectXYZ edges, the points eliminated by a Schur complement.  Plain C++ shared by
// ba_kernels.hip and by a host build (tests/cpp/ba_solve_host.cpp), so every stage can be checked against float64
// numpy without a GPU.  Both builds use -ffp-contract=off; libm: sqrt, fabs (sin and cos of a pose update are
// pose::sin_cos, plain multiplies and adds: a device's and a host's libm round some arguments differently, and the host
// build is what both device paths have to match bit for bit).  Every step is in f64; poses,
// points, pixels and intrinsics are f32 and are promoted on load.  Estimate, estimate_of, matrix_of, se3_exp, the
// oplus (moved), the edge error and the Huber kernel are those of pose_solve.h.
//
// How the work is spread is a team: every phase is team.each(n, f) -- "f(i) for every i in [0, n)", then a join.  The
// device strides a workgroup over the indices and joins with __syncthreads (ba_kernels.hip); Serial is a plain loop.
// Every output of a phase has one owner, which adds its terms in an order fixed by the problem's own arrays: a point's
// Hpp, b_p and cost in edge order (the edges are sorted by point), a camera's Hcc, b_c and its rows of S in the order of
// a camera-side CSR built stably from the edge list, every total as a pairwise tree over a per-point (per-camera)
// array whose shape depends on the count alone.  So both builds add in the same order, there are no floating-point
// atomics, and a problem's result depends on nothing but the problem.
//
// g2o is not available where this was written: what is marked [M] restates it from memory.
//  [M] EdgeSE3ProjectXYZ: e = obs - (f X / Z + c) with X = T Xw; the 2 x 6 pose Jacobian of
//      EdgeSE3ProjectXYZOnlyPose; the 2 x 3 point Jacobian -(1 / Z) [fx 0 -fx X / Z; 0 fy -fy Y / Z] R;
//      isDepthPositive: Z > 0; information: the identity; H += rho' J'J, b -= rho' J'e for both vertices and the cross
//      block W = rho' Jc'Jp; an edge whose camera is fixed contributes to its point only.
//  [M] RobustKernelHuber with delta = sqrt(huber_delta2): pose::robustify holds delta^2 = 5.991; another delta^2 goes
//      through it by scaling, rho_d(e2) = rho_0(s e2) / s and rho_d' = rho_0'(s e2) with s = 5.991 / delta^2, which is
//      exactly 1 for 5.991.
//  [M] BlockSolver_6_3: lambda on every diagonal entry of the pose and of the point blocks; Hpp^-1 of every 3 x 3 point
//      block (the cofactor inverse); S = Hcc - sum_p W_p Hpp^-1 W_p', b_S = b_c - sum_p W_p Hpp^-1 b_p over the free
//      cameras; S dx_c = b_S by a dense Cholesky; dx_p = Hpp^-1 (b_p - W_p' dx_c).
//  [M] OptimizationAlgorithmLevenberg as in pose_solve.h, over all dimensions: lambda_0 = 1e-5 max|diag| over pose and
//      point blocks, gain = (cost - cost_trial) / (sum dx (lambda dx + b) + 1e-3), at most 10 trials, the run ends on
//      an iteration that accepts nothing; lambda and ni restart at the first iteration of each round.
//
// Schedule: up to two rounds.  LocalBundleAdjustment: 5 iterations with Huber, then 10 without a kernel over the edges
// that :507-518 keeps (chi2 <= chi2_max and depth positive at the end of round 0).  BundleAdjustment: one round.  The
// final flags restate :530-540: an edge of the last round is classified at the kept estimate; an edge that left after
// round 0 is flagged iff its chi2 of the end of round 0 exceeds the threshold or its depth is not positive at the
// final estimate (g2o never recomputes a level-1 edge's error, but isDepthPositive() reads the current vertices).
//
// Defined divergences from the reference:
//  * Every edge is classified at the estimate a round keeps (g2o's edges may hold the error of a rejected trial).
//  * A point or camera with no active edge in a round does not move (g2o leaves it out of initializeOptimization(0)).
//  * A NaN chi2 is no outlier (">" is false); the depth clause stays literal, !(Z > 0).
//  * A non-finite entry or a pivot that is not positive (in a point block or in S) rejects the trial outright.
//  * A NaN gain rejects the trial and the next one runs; the run ends on an iteration whose trials were all rejected.
//  * Every loop is bounded: 2 rounds x 32 iterations x 10 trials, strides over the problem's own counts.
//  * One set of intrinsics per problem (the reference reads them per key frame; there is one camera).
//  * The stop word (pbStopFlag) is read once before every round and at the top of every iteration; non-zero ends the
//    run and skips round 1 (:502-505).  The final flags and estimates are still written.
#ifndef MSF_BA_SOLVE_H
#define MSF_BA_SOLVE_H

#include <math.h>
#include <stdint.h>

#include "carve.h"
#include "pose_solve.h"

namespace msf {
namespace ba {

using pose::Cam;
using pose::Estimate;
using pose::finite;
using pose::kDblMax;

constexpr int kMaxFreeCams = 64;     // MSF_BA_MAX_FREE_CAMS
constexpr int kRounds = 2, kMaxIterations = 32, kSlots = kRounds * kMaxIterations, kTrials = 10;
constexpr int kLin = 22;             // per edge: j0[6], j1[6] (pose), p0[3], p1[3] (point), e[2], rho', rho

struct Params {
  Cam cam;
  int n_rounds;
  int iterations[kRounds];
  int robust[kRounds];
  double huber_delta2;
  double chi2;
};

// One problem.  Edge indices are local to it; the edges are sorted by point.
struct Problem {
  int n_cams, n_points, n_edges;
  const float* cam_tcw;       // [n_cams][12]
  const uint8_t* cam_fixed;   // [n_cams]
  const float* points;        // [n_points][3]
  const int32_t* edge_cam;
  const int32_t* edge_point;
  const float* edge_obs;      // [n_edges][2]
};

// The scratch of a call: arrays over the call's cameras, points and edges (a problem's piece starts at its cam0,
// point0, edge0) and one dense system per problem.
struct Scratch {
  Estimate* cam;          // [cams] the estimates
  Estimate* cam_trial;
  double* pt;             // [points][3]
  double* pt_trial;
  int32_t* free_of;       // [cams] index among the problem's free cameras, -1: fixed
  int32_t* free_cam;      // [cams] camera of a free index
  // Every array over cameras, points or edges has exactly one row per camera, point or edge, so that the pieces of
  // two problems are disjoint wherever their ranges are, in whatever order the descriptors list them.
  int32_t* cam_start;     // [cams] the camera-side CSR: camera c's edges are cam_edges[cam_start[c] .. cam_end[c])
  int32_t* cam_end;       // [cams]
  int32_t* cam_edges;     // [edges]
  int32_t* cam_active;    // [cams] active edges of the round
  int32_t* pt_start;      // [points] point q's edges are [pt_start[q], pt_end[q])
  int32_t* pt_end;        // [points]
  int32_t* pt_active;     // [points]
  int32_t* word;          // [problems] one word per problem through which the leader tells the team a count
  uint8_t* active;        // [edges]
  double* chi2_0;         // [edges] chi2 at the estimate round 0 kept
  double* lin;            // [edges][kLin]
  double* W;              // [edges][18] row-major 6 x 3
  double* Hpp;            // [points][6] upper triangle, row-major
  double* bp;             // [points][3]
  double* inv;            // [points][6] (Hpp + lambda I)^-1
  double* dxp;            // [points][3]
  double* redp;           // [points] what a tree reduces
  double* redq;           // [points]
  double* redc;           // [cams]
  double* Hcc;            // [problems][max_free][27]: 21 of the upper triangle, 6 of b_c
  double* S;              // [problems][6 F][6 F + 1] column-major with b_S as row 6 F; F = max_free
  double* diag;           // [problems][6 F]
  double* x;              // [problems][6 F] dx_c
  int32_t max_free;
};

// The one layout of the scratch: measured on a null base, placed on the block.
inline Scratch layout(Carver& c, size_t problems, size_t cams, size_t points, size_t edges, int max_free) {
  const size_t f = (size_t)max_free, n = 6 * f;
  Scratch s{};
  s.cam = c.take<Estimate>(cams), s.cam_trial = c.take<Estimate>(cams);
  s.pt = c.take<double>(points * 3), s.pt_trial = c.take<double>(points * 3);
  s.free_of = c.take<int32_t>(cams), s.free_cam = c.take<int32_t>(cams);
  s.cam_start = c.take<int32_t>(cams), s.cam_end = c.take<int32_t>(cams), s.cam_edges = c.take<int32_t>(edges);
  s.pt_end = c.take<int32_t>(points), s.word = c.take<int32_t>(problems);
  s.cam_active = c.take<int32_t>(cams);
  s.pt_start = c.take<int32_t>(points), s.pt_active = c.take<int32_t>(points);
  s.active = c.take<uint8_t>(edges);
  s.chi2_0 = c.take<double>(edges), s.lin = c.take<double>(edges * kLin), s.W = c.take<double>(edges * 18);
  s.Hpp = c.take<double>(points * 6), s.bp = c.take<double>(points * 3), s.inv = c.take<double>(points * 6);
  s.dxp = c.take<double>(points * 3), s.redp = c.take<double>(points), s.redq = c.take<double>(points);
  s.redc = c.take<double>(cams);
  s.Hcc = c.take<double>(problems * f * 27), s.S = c.take<double>(problems * n * (n + 1));
  s.diag = c.take<double>(problems * n), s.x = c.take<double>(problems * n);
  s.max_free = max_free;
  return s;
}

// a problem's piece of the scratch
MSF_HD Scratch piece(const Scratch& s, long long problem, long long cam0, long long point0, long long edge0) {
  const long long f = s.max_free, n = 6 * f;
  Scratch w = s;
  w.cam += cam0, w.cam_trial += cam0, w.pt += point0 * 3, w.pt_trial += point0 * 3;
  w.free_of += cam0, w.free_cam += cam0, w.cam_start += cam0, w.cam_end += cam0, w.cam_edges += edge0, w.cam_active += cam0;
  w.pt_start += point0, w.pt_end += point0, w.pt_active += point0, w.word += problem, w.active += edge0;
  w.chi2_0 += edge0, w.lin += edge0 * kLin, w.W += edge0 * 18;
  w.Hpp += point0 * 6, w.bp += point0 * 3, w.inv += point0 * 6, w.dxp += point0 * 3;
  w.redp += point0, w.redq += point0, w.redc += cam0;
  w.Hcc += problem * f * 27, w.S += problem * n * (n + 1), w.diag += problem * n, w.x += problem * n;
  return w;
}

// Where a problem's results go (msf_ba_result's arrays at this problem), any of them null but status.
struct Out {
  int32_t* status;
  float* cam_tcw;              // [n_cams][12]
  float* points;               // [n_points][3]
  uint8_t* outliers;           // [n_edges]
  double* cam_pose_f64;        // [n_cams][12]
  double* points_f64;          // [n_points][3]
  uint8_t* round_flags;        // [n_edges][2]
  int32_t* round_iterations;   // [2]
  int32_t* it_trials;          // [kSlots]
  double* it_lambda_in;
  double* it_lambda_out;
  double* it_cost_in;
  double* it_cost_out;
  double* it_cam_in;           // [kSlots][n_cams][7]
  double* it_point_in;         // [kSlots][n_points][3]
  double* it_cam_out;
  double* it_point_out;
  double* it_Hcc;              // [kSlots][n_cams][21]
  double* it_bc;               // [kSlots][n_cams][6]
  double* it_Hpp;              // [kSlots][n_points][6]
  double* it_bp;               // [kSlots][n_points][3]
};

// the host's team: one thread
struct Serial {
  template <class F>
  void each(int n, F f) const {
    for (int i = 0; i < n; i++) f(i);
  }
  bool any(bool b) const { return b; }
  bool leader() const { return true; }
  void join() const {}
};

// a[0] = the sum (the largest) of a[0..n) as a pairwise tree whose shape depends on n alone; a is used up
template <bool kMax, class Team>
MSF_HD double tree(const Team& team, double* a, int n) {
  for (long long s = 1; s < n; s <<= 1) {
    const int pairs = (int)((n - s + 2 * s - 1) / (2 * s));
    team.each(pairs, [&](int t) {
      const long long i = 2 * s * t;
      if (kMax) a[i] = a[i + s] > a[i] ? a[i + s] : a[i];
      else a[i] = a[i] + a[i + s];
    });
  }
  const double r = n > 0 ? a[0] : 0.0;
  team.join();   // every member has read a[0] before a later phase writes it
  return r;
}

MSF_HD int tri(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }   // (r, c), r <= c, of a 6 x 6 upper triangle

// RobustKernelHuber of delta^2 = delta2 through pose::robustify (see the header comment)
MSF_HD void robustify(bool huber, double delta2, double e2, double* rho, double* weight) {
  const double s = pose::kHuberDelta2 / delta2;
  pose::robustify(huber, e2 * s, rho, weight);
  *rho = *rho / s;
}

// camera point and error of edge e at the given estimates
MSF_HD void edge_at(const Problem& p, const Cam& cam, const Estimate* cams, const double* pts, int e, double* rt,
                    double* xc, double* err) {
  pose::matrix_of(cams[p.edge_cam[e]], rt);
  const double u[2] = {(double)p.edge_obs[2 * e], (double)p.edge_obs[2 * e + 1]};
  pose::edge_error(rt, cam, pts + 3 * (long long)p.edge_point[e], u, xc, err);
}

// :507-518 / :530-540 on a fresh error: chi2 > chi2_max || !isDepthPositive(); *chi2 gets e'e
MSF_HD bool flagged_at(const Problem& p, const Params& prm, const Estimate* cams, const double* pts, int e, double* chi2) {
  double rt[12], xc[3], err[2];
  edge_at(p, prm.cam, cams, pts, e, rt, xc, err);
  *chi2 = err[0] * err[0] + err[1] * err[1];
  return *chi2 > prm.chi2 || !(xc[2] > 0);
}

MSF_HD double edge_cost(const Problem& p, const Params& prm, bool huber, const Estimate* cams, const double* pts, int e) {
  double rt[12], xc[3], err[2], rho, w;
  edge_at(p, prm.cam, cams, pts, e, rt, xc, err);
  robustify(huber, prm.huber_delta2, err[0] * err[0] + err[1] * err[1], &rho, &w);
  return rho;
}

// linearizeOplus and robustify of edge e at the estimates: lin and, for a free camera, W
MSF_HD void linearize(const Problem& p, const Params& prm, bool huber, const Scratch& w, int e) {
  double rt[12], xc[3], err[2];
  edge_at(p, prm.cam, w.cam, w.pt, e, rt, xc, err);
  const Cam& cam = prm.cam;
  const double x = xc[0], y = xc[1], invz = 1.0 / xc[2], invz2 = invz * invz;
  double* l = w.lin + (long long)e * kLin;
  const double j0[6] = {x * y * invz2 * cam.fu, -(1 + x * x * invz2) * cam.fu, y * invz * cam.fu, -invz * cam.fu, 0.0,
                        x * invz2 * cam.fu};
  const double j1[6] = {(1 + y * y * invz2) * cam.fv, -x * y * invz2 * cam.fv, -x * invz * cam.fv, 0.0, -invz * cam.fv,
                        y * invz2 * cam.fv};
  for (int k = 0; k < 6; k++) l[k] = j0[k], l[6 + k] = j1[k];
  const double t02 = -x * invz * cam.fu, t12 = -y * invz * cam.fv;
  for (int k = 0; k < 3; k++) {
    l[12 + k] = -invz * (cam.fu * rt[k] + t02 * rt[8 + k]);
    l[15 + k] = -invz * (cam.fv * rt[4 + k] + t12 * rt[8 + k]);
  }
  l[18] = err[0], l[19] = err[1];
  robustify(huber, prm.huber_delta2, err[0] * err[0] + err[1] * err[1], &l[21], &l[20]);
  if (w.free_of[p.edge_cam[e]] < 0) return;
  double* W = w.W + (long long)e * 18;
  for (int r = 0; r < 6; r++)
    for (int k = 0; k < 3; k++) W[3 * r + k] = l[20] * (l[r] * l[12 + k] + l[6 + r] * l[15 + k]);
}

// (a + lambda I)^-1 of a symmetric 3 x 3 given as its upper triangle; false: a leading minor that is not positive
MSF_HD bool invert3(const double* a, double lambda, double* inv) {
  const double a00 = a[0] + lambda, a01 = a[1], a02 = a[2], a11 = a[3] + lambda, a12 = a[4], a22 = a[5] + lambda;
  const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
  const double m2 = a00 * a11 - a01 * a01;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  if (!(a00 > 0 && m2 > 0 && det > 0 && finite(det))) return false;
  inv[0] = c00 / det, inv[1] = c01 / det, inv[2] = c02 / det;
  inv[3] = (a00 * a22 - a02 * a02) / det, inv[4] = (a01 * a02 - a00 * a12) / det, inv[5] = m2 / det;
  return true;
}

// y = m x for a symmetric 3 x 3 given as its upper triangle
MSF_HD void sym3_mul(const double* m, const double* x, double* y) {
  y[0] = m[0] * x[0] + m[1] * x[1] + m[2] * x[2];
  y[1] = m[1] * x[0] + m[3] * x[1] + m[4] * x[2];
  y[2] = m[2] * x[0] + m[4] * x[1] + m[5] * x[2];
}

// The bodies of the phases, one index each: the teams of this file and the grid-wide launches of gba_solve.h /
// gba_kernels.hip call the same code.

// an edge whose indices may not be used: out of range, or its point below the edge before it
MSF_HD bool edge_malformed(const Problem& p, int e) {
  const int c = p.edge_cam[e], q = p.edge_point[e];
  return c < 0 || c >= p.n_cams || q < 0 || q >= p.n_points || (e > 0 && p.edge_point[e - 1] > q);
}

// the free cameras in camera order (one thread) -> their count
MSF_HD int map_free_cameras(const Problem& p, const Scratch& w) {
  int nf = 0;
  for (int c = 0; c < p.n_cams; c++) {
    const bool fixed = p.cam_fixed[c] != 0;
    w.free_of[c] = fixed ? -1 : nf;
    if (!fixed) w.free_cam[nf++] = c;
  }
  return nf;
}

// camera c: how many edges it has (into cam_active) and its entry estimate
MSF_HD void count_camera_edges(const Problem& p, const Scratch& w, int c) {
  int k = 0;
  for (int e = 0; e < p.n_edges; e++) k += p.edge_cam[e] == c;
  w.cam_active[c] = k;
  w.cam[c] = pose::estimate_of(p.cam_tcw + 12 * (long long)c);
}

// camera c collects its edges in edge order from cam_start[c] on
MSF_HD void collect_camera_edges(const Problem& p, const Scratch& w, int c) {
  int at = w.cam_start[c];
  for (int e = 0; e < p.n_edges; e++)
    if (p.edge_cam[e] == c) w.cam_edges[at++] = e;
}

// point q: its edges [pt_start[q], pt_end[q]) by two lower bounds in the sorted edge_point, and its entry estimate
MSF_HD void prepare_point(const Problem& p, const Scratch& w, int q) {
  for (int side = 0; side < 2; side++) {
    int lo = 0, hi = p.n_edges;
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (p.edge_point[mid] < q + side) lo = mid + 1;
      else hi = mid;
    }
    (side ? w.pt_end : w.pt_start)[q] = lo;
  }
  for (int k = 0; k < 3; k++) w.pt[3 * (long long)q + k] = (double)p.points[3 * (long long)q + k];
}

// Checks every index before use and builds what does not change: the free-camera map, both CSRs and the estimates.
// false: malformed (nothing but the scratch was written).  *n_free: the free cameras.
template <class Team>
MSF_HD bool prepare(const Team& team, const Problem& p, const Scratch& w, int* n_free) {
  bool bad = false;
  team.each(p.n_edges, [&](int e) {
    if (edge_malformed(p, e)) bad = true;
  });
  if (team.any(bad)) return false;
  // the free cameras in camera order; the count travels through the problem's word
  if (team.leader()) *w.word = map_free_cameras(p, w);
  team.join();
  const int nf = *w.word;
  team.join();
  *n_free = nf;
  if (nf > w.max_free) return false;
  // the camera-side CSR: counts, the leader's prefix sum, then every camera collects its edges in edge order
  team.each(p.n_cams, [&](int c) { count_camera_edges(p, w, c); });
  if (team.leader()) {
    int at = 0;
    for (int c = 0; c < p.n_cams; c++) {
      w.cam_start[c] = at;
      at += w.cam_active[c];
      w.cam_end[c] = at;
    }
  }
  team.join();
  team.each(p.n_cams, [&](int c) { collect_camera_edges(p, w, c); });
  team.each(p.n_points, [&](int q) { prepare_point(p, w, q); });
  return true;
}

MSF_HD void count_active_camera(const Scratch& w, int c) {
  int k = 0;
  for (int at = w.cam_start[c]; at < w.cam_end[c]; at++) k += w.active[w.cam_edges[at]];
  w.cam_active[c] = k;
}

MSF_HD void count_active_point(const Scratch& w, int q) {
  int k = 0;
  for (int e = w.pt_start[q]; e < w.pt_end[q]; e++) k += w.active[e];
  w.pt_active[q] = k;
}

// how many active edges every camera and point has in the round
template <class Team>
MSF_HD void count_active(const Team& team, const Problem& p, const Scratch& w) {
  team.each(p.n_cams, [&](int c) { count_active_camera(w, c); });
  team.each(p.n_points, [&](int q) { count_active_point(w, q); });
}

// Hpp, b_p, cost (redp) and largest |diagonal| (redq) of point q over its active edges, in edge order
MSF_HD void point_system(const Scratch& w, int q) {
  double h[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, cost = 0.0;
  for (int e = w.pt_start[q]; e < w.pt_end[q]; e++) {
    if (!w.active[e]) continue;
    const double* l = w.lin + (long long)e * kLin;
    int at = 0;
    for (int r = 0; r < 3; r++)
      for (int c = r; c < 3; c++) h[at++] += l[20] * (l[12 + r] * l[12 + c] + l[15 + r] * l[15 + c]);
    for (int r = 0; r < 3; r++) b[r] += -(l[20] * (l[12 + r] * l[18] + l[15 + r] * l[19]));
    cost += l[21];
  }
  for (int k = 0; k < 6; k++) w.Hpp[6 * (long long)q + k] = h[k];
  for (int k = 0; k < 3; k++) w.bp[3 * (long long)q + k] = b[k];
  w.redp[q] = cost;
  double top = fabs(h[0]);
  top = fabs(h[3]) > top ? fabs(h[3]) : top;
  w.redq[q] = fabs(h[5]) > top ? fabs(h[5]) : top;
}

// entry i = (free camera, one of the 21 of Hcc's upper triangle or the 6 of b_c) over the camera's CSR, in its order
MSF_HD void camera_system(const Scratch& w, int i) {
  const int f = i / 27, k = i % 27, c = w.free_cam[f];
  int r = 0, cc = k - 21;
  if (k < 21) {
    int left = k;
    while (left >= 6 - r) left -= 6 - r, r++;
    cc = r + left;
  }
  double sum = 0.0;
  for (int at = w.cam_start[c]; at < w.cam_end[c]; at++) {
    const int e = w.cam_edges[at];
    if (!w.active[e]) continue;
    const double* l = w.lin + (long long)e * kLin;
    if (k < 21) sum += l[20] * (l[r] * l[cc] + l[6 + r] * l[6 + cc]);
    else sum += -(l[20] * (l[cc] * l[18] + l[6 + cc] * l[19]));
  }
  w.Hcc[i] = sum;
}

// H and b of the active edges at the estimates; -> the cost.  redq is left holding every point's largest |diagonal|.
template <class Team>
MSF_HD double build_system(const Team& team, const Problem& p, const Params& prm, bool huber, const Scratch& w, int nf) {
  team.each(p.n_edges, [&](int e) {
    if (w.active[e]) linearize(p, prm, huber, w, e);
  });
  team.each(p.n_points, [&](int q) { point_system(w, q); });
  team.each(nf * 27, [&](int i) { camera_system(w, i); });
  return tree<false>(team, w.redp, p.n_points);
}

// what column c of the 6 x 3 block W2 takes from an entry of S, y being Hpp^-1 times the row's own row of W
MSF_HD double schur_term(const double* y, const double* W2, int c) {
  return y[0] * W2[3 * c] + y[1] * W2[3 * c + 1] + y[2] * W2[3 * c + 2];
}

// row `row` of S (lower triangle, column-major, ld = n + 1) and its entry of b_S (row n) at lambda
MSF_HD void schur_row(const Problem& p, const Scratch& w, int nf, double lambda, int row) {
  const int n = 6 * nf;
  const long long ld = n + 1;
  const int fi = row / 6, r = row % 6, ci = w.free_cam[fi];
  const double* H = w.Hcc + 27 * (long long)fi;
  const bool moves = w.cam_active[ci] > 0;
  for (int col = 0; col <= row; col++) {
    double v = 0.0;
    if (col / 6 == fi) {
      const int c = col % 6;
      v = moves ? H[tri(c, r)] + (c == r ? lambda : 0.0) : (c == r ? 1.0 : 0.0);
    }
    w.S[col * ld + row] = v;
  }
  double bs = moves ? H[21 + r] : 0.0;
  for (int at = w.cam_start[ci]; at < w.cam_end[ci]; at++) {
    const int e = w.cam_edges[at];
    if (!w.active[e]) continue;
    const int q = p.edge_point[e];
    const double* We = w.W + 18 * (long long)e + 3 * r;
    double y[3];
    sym3_mul(w.inv + 6 * (long long)q, We, y);
    const double* b = w.bp + 3 * (long long)q;
    bs -= y[0] * b[0] + y[1] * b[1] + y[2] * b[2];
    for (int e2 = w.pt_start[q]; e2 < w.pt_end[q]; e2++) {
      if (!w.active[e2]) continue;
      const int fj = w.free_of[p.edge_cam[e2]];
      if (fj < 0 || fj > fi) continue;
      const double* W2 = w.W + 18 * (long long)e2;
      const int last = fj == fi ? r : 5;
      for (int c = 0; c <= last; c++)
        w.S[(6 * fj + c) * ld + row] -= schur_term(y, W2, c);
    }
  }
  w.S[row * ld + n] = bs;
}

// S and b_S at lambda; every row by its owner
template <class Team>
MSF_HD void build_schur(const Team& team, const Problem& p, const Scratch& w, int nf, double lambda) {
  team.each(6 * nf, [&](int row) { schur_row(p, w, nf, lambda, row); });
}

// L L' = S in place, left-looking, with b_S as row n, so that row n ends as y = L^-1 b_S; the diagonal of L goes to
// `diag`.  false: a pivot that is not positive or not finite.
template <class Team>
MSF_HD bool cholesky(const Team& team, double* S, int n, double* diag) {
  const long long ld = n + 1;
  for (int j = 0; j < n; j++) {
    team.each(n + 1 - j, [&](int t) {
      const int i = j + t;
      double s = S[j * ld + i];
      for (int k = 0; k < j; k++) s -= S[k * ld + i] * S[k * ld + j];
      S[j * ld + i] = s;
    });
    const double pivot = S[j * ld + j];   // never written again
    if (!(pivot > 0 && finite(pivot))) return false;
    team.each(n + 1 - j, [&](int t) {
      const int i = j + t;
      const double d = sqrt(S[j * ld + j]);
      if (i == j) diag[j] = d;
      else S[j * ld + i] = S[j * ld + i] / d;
    });
  }
  return true;
}

// L' x = y, y being row n of S
template <class Team>
MSF_HD void back_substitute(const Team& team, double* S, int n, const double* diag, double* x) {
  const long long ld = n + 1;
  for (int j = n - 1; j >= 0; j--)
    team.each(j + 1, [&](int i) {
      const double xj = S[j * ld + n] / diag[j];
      if (i == j) x[j] = xj;
      else S[i * ld + n] -= S[i * ld + j] * xj;
    });
}

MSF_HD void write_camera(const Scratch& w, double* cam_out, int c) {
  for (int k = 0; k < 4; k++) cam_out[7 * (long long)c + k] = w.cam[c].q[k];
  for (int k = 0; k < 3; k++) cam_out[7 * (long long)c + 4 + k] = w.cam[c].t[k];
}

template <class Team>
MSF_HD void write_estimates(const Team& team, const Problem& p, const Scratch& w, double* cam_out, double* pt_out) {
  if (cam_out)
    team.each(p.n_cams, [&](int c) { write_camera(w, cam_out, c); });
  if (pt_out)
    team.each(p.n_points * 3, [&](int k) { pt_out[k] = w.pt[k]; });
}

// it_Hcc / it_bc of camera c in `slot`: 0 for a fixed camera
MSF_HD void write_camera_system(const Problem& p, const Scratch& w, const Out& o, int slot, int c) {
  const long long nc = p.n_cams;
  const int f = w.free_of[c];
  for (int k = 0; k < 21; k++)
    if (o.it_Hcc) o.it_Hcc[(slot * nc + c) * 21 + k] = f < 0 ? 0.0 : w.Hcc[27 * (long long)f + k];
  for (int k = 0; k < 6; k++)
    if (o.it_bc) o.it_bc[(slot * nc + c) * 6 + k] = f < 0 ? 0.0 : w.Hcc[27 * (long long)f + 21 + k];
}

// the largest |diagonal| of free camera f's block, into redc
MSF_HD void camera_top(const Scratch& w, int f) {
  double top = 0.0;
  for (int r = 0; r < 6; r++) {
    const double d = fabs(w.Hcc[27 * (long long)f + tri(r, r)]);
    top = d > top ? d : top;
  }
  w.redc[f] = top;
}

// (Hpp + lambda I)^-1 of point q, 0 for a point without an active edge; false: the block failed
MSF_HD bool invert_point(const Scratch& w, double lam, int q) {
  double* inv = w.inv + 6 * (long long)q;
  if (!w.pt_active[q]) {
    for (int k = 0; k < 6; k++) inv[k] = 0.0;
    return true;
  }
  return invert3(w.Hpp + 6 * (long long)q, lam, inv);
}

// dx_p, the trial point and the point's part of the gain's denominator (redq)
MSF_HD void point_step(const Problem& p, const Scratch& w, double lam, int q) {
  const double* b = w.bp + 3 * (long long)q;
  double t[3] = {b[0], b[1], b[2]}, dx[3];
  for (int e = w.pt_start[q]; e < w.pt_end[q]; e++) {
    if (!w.active[e]) continue;
    const int f = w.free_of[p.edge_cam[e]];
    if (f < 0) continue;
    const double* We = w.W + 18 * (long long)e;
    const double* xc = w.x + 6 * f;
    for (int k = 0; k < 3; k++)
      for (int r = 0; r < 6; r++) t[k] -= We[3 * r + k] * xc[r];
  }
  sym3_mul(w.inv + 6 * (long long)q, t, dx);
  double scale = 0.0;
  for (int k = 0; k < 3; k++) {
    w.dxp[3 * (long long)q + k] = dx[k];
    w.pt_trial[3 * (long long)q + k] = w.pt_active[q] ? w.pt[3 * (long long)q + k] + dx[k] : w.pt[3 * (long long)q + k];
    scale += dx[k] * (lam * dx[k] + b[k]);
  }
  w.redq[q] = scale;
}

// the trial estimate of camera c and, for a free one, its part of the gain's denominator (redc)
MSF_HD void camera_step(const Scratch& w, double lam, int c) {
  const int f = w.free_of[c];
  w.cam_trial[c] = w.cam[c];
  if (f < 0) return;
  double scale = 0.0;
  if (w.cam_active[c] > 0) {
    const double* dx = w.x + 6 * f;
    w.cam_trial[c] = pose::moved<true>(w.cam[c], dx);
    for (int k = 0; k < 6; k++) scale += dx[k] * (lam * dx[k] + w.Hcc[27 * (long long)f + 21 + k]);
  }
  w.redc[f] = scale;
}

// the cost of point q's active edges at the trial estimates, in edge order, into redp
MSF_HD void point_trial_cost(const Problem& p, const Params& prm, bool huber, const Scratch& w, int q) {
  double c = 0.0;
  for (int e = w.pt_start[q]; e < w.pt_end[q]; e++)
    if (w.active[e]) c += edge_cost(p, prm, huber, w.cam_trial, w.pt_trial, e);
  w.redp[q] = c;
}

// a trial's verdict from its figures: the expressions of OptimizationAlgorithmLevenberg
MSF_HD double gain_of(double cost, double trial_cost, double scale_c, double scale_p) {
  return (cost - trial_cost) / ((1e-3 + scale_c) + scale_p);
}

// lambda and ni after a trial; -> the run of trials ends without an accepted one
MSF_HD bool next_lambda(bool accepted, double gain, double* lambda, double* ni) {
  if (accepted) {
    const double y = 2 * gain - 1;
    double alpha = 1.0 - y * y * y;
    alpha = alpha < 2.0 / 3.0 ? alpha : 2.0 / 3.0;
    *lambda *= alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0;
    *ni = 2.0;
    return false;
  }
  *lambda *= *ni;
  *ni *= 2.0;
  return !finite(*lambda) || gain == 0;
}

// One iteration of OptimizationAlgorithmLevenberg::solve over BlockSolver_6_3: the system once at the entry estimate,
// then trials until one is accepted.  -> the number of trials, negated when none was accepted (the run ends).
template <class Team>
MSF_HD int iteration(const Team& team, const Problem& p, const Params& prm, const Scratch& w, int nf, int round,
                     bool first, double* lambda, double* ni, const Out& o, int slot) {
  const bool huber = prm.robust[round] != 0;
  const int n = 6 * nf;
  const long long nc = p.n_cams, np = p.n_points;
  write_estimates(team, p, w, o.it_cam_in ? o.it_cam_in + slot * nc * 7 : nullptr,
                  o.it_point_in ? o.it_point_in + slot * np * 3 : nullptr);
  const double cost = build_system(team, p, prm, huber, w, nf);
  if (o.it_Hcc || o.it_bc)
    team.each(p.n_cams, [&](int c) { write_camera_system(p, w, o, slot, c); });
  if (o.it_Hpp) team.each(p.n_points * 6, [&](int k) { o.it_Hpp[slot * np * 6 + k] = w.Hpp[k]; });
  if (o.it_bp) team.each(p.n_points * 3, [&](int k) { o.it_bp[slot * np * 3 + k] = w.bp[k]; });
  if (first) {
    team.each(nf, [&](int f) { camera_top(w, f); });
    const double top_p = tree<true>(team, w.redq, p.n_points), top_c = tree<true>(team, w.redc, nf);
    *lambda = 1e-5 * (top_c > top_p ? top_c : top_p);
    *ni = 2.0;
  }
  const double lambda_in = *lambda;
  double cost_out = cost;
  int trials = 0;
  bool accepted = false;
  while (trials < kTrials && !accepted) {
    trials++;
    const double lam = *lambda;
    double gain = -1.0, trial_cost = kDblMax;
    bool bad = false;
    team.each(p.n_points, [&](int q) {
      if (!invert_point(w, lam, q)) bad = true;
    });
    bool solved = !team.any(bad) && finite(lam);
    if (solved) {
      build_schur(team, p, w, nf, lam);
      solved = cholesky(team, w.S, n, w.diag);
    }
    if (solved) {
      back_substitute(team, w.S, n, w.diag, w.x);
      team.each(p.n_points, [&](int q) { point_step(p, w, lam, q); });
      team.each(p.n_cams, [&](int c) { camera_step(w, lam, c); });
      team.each(p.n_points, [&](int q) { point_trial_cost(p, prm, huber, w, q); });
      trial_cost = tree<false>(team, w.redp, p.n_points);
      const double scale_c = tree<false>(team, w.redc, nf), scale_p = tree<false>(team, w.redq, p.n_points);
      gain = gain_of(cost, trial_cost, scale_c, scale_p);
    }
    if (solved && gain > 0 && finite(trial_cost)) {
      next_lambda(true, gain, lambda, ni);
      team.each(p.n_cams, [&](int c) { w.cam[c] = w.cam_trial[c]; });
      team.each(p.n_points * 3, [&](int k) { w.pt[k] = w.pt_trial[k]; });
      cost_out = trial_cost;
      accepted = true;
    } else if (next_lambda(false, gain, lambda, ni)) {
      break;
    }
  }
  write_estimates(team, p, w, o.it_cam_out ? o.it_cam_out + slot * nc * 7 : nullptr,
                  o.it_point_out ? o.it_point_out + slot * np * 3 : nullptr);
  if (team.leader()) {
    if (o.it_trials) o.it_trials[slot] = trials;
    if (o.it_lambda_in) o.it_lambda_in[slot] = lambda_in;
    if (o.it_lambda_out) o.it_lambda_out[slot] = *lambda;
    if (o.it_cost_in) o.it_cost_in[slot] = cost;
    if (o.it_cost_out) o.it_cost_out[slot] = cost_out;
  }
  return accepted ? trials : -trials;
}

// :507-518: the edges round 1 keeps, and every edge's chi2 at the estimate round 0 kept
MSF_HD void reclassify_edge(const Problem& p, const Params& prm, const Scratch& w, int e) {
  const bool f = flagged_at(p, prm, w.cam, w.pt, e, &w.chi2_0[e]);
  w.active[e] = f ? 0 : 1;
}

MSF_HD void write_round0_flag(const Problem& p, const Params& prm, const Scratch& w, const Out& o, int e) {
  double chi2;
  o.round_flags[2 * (long long)e] = flagged_at(p, prm, w.cam, w.pt, e, &chi2) ? 1 : 0;
}

// :530-540
MSF_HD void write_final_flag(const Problem& p, const Params& prm, const Scratch& w, const Out& o, int rounds_run, int e) {
  double chi2;
  bool f = flagged_at(p, prm, w.cam, w.pt, e, &chi2);
  if (rounds_run == 2 && !w.active[e]) {
    double rt[12], xc[3], err[2];
    edge_at(p, prm.cam, w.cam, w.pt, e, rt, xc, err);
    f = w.chi2_0[e] > prm.chi2 || !(xc[2] > 0);
  }
  if (o.outliers) o.outliers[e] = f ? 1 : 0;
  if (o.round_flags && rounds_run == 2) o.round_flags[2 * (long long)e + 1] = f ? 1 : 0;
}

MSF_HD void write_final_camera(const Problem& p, const Scratch& w, const Out& o, int rounds_run, int c) {
  double rt[12];
  pose::matrix_of(w.cam[c], rt);
  const bool as_came = w.free_of[c] < 0 || rounds_run == 0;
  for (int k = 0; k < 12; k++) {
    const float in = p.cam_tcw[12 * (long long)c + k];
    const double v = as_came ? (double)in : rt[k];
    if (o.cam_pose_f64) o.cam_pose_f64[12 * (long long)c + k] = v;
    if (o.cam_tcw) o.cam_tcw[12 * (long long)c + k] = as_came ? in : (float)v;
  }
}

MSF_HD void write_final_point(const Scratch& w, const Out& o, int k) {
  if (o.points_f64) o.points_f64[k] = w.pt[k];
  if (o.points) o.points[k] = (float)w.pt[k];
}

// the stop word, read by the leader alone and agreed on by the team
template <class Team>
MSF_HD bool stop_set(const Team& team, const int32_t* stop) {
  return team.any(team.leader() && stop && *(const volatile int32_t*)stop != 0);
}

// The whole schedule on one problem -> its status: -1 (malformed or too many free cameras; nothing else is written)
// or the rounds run.
template <class Team>
MSF_HD int bundle_adjust(const Team& team, const Problem& p, const Params& prm, const int32_t* stop, const Scratch& w,
                         const Out& o) {
  int nf = 0;
  if (!prepare(team, p, w, &nf)) return -1;
  if (team.leader()) {
    for (int k = 0; k < kSlots; k++)
      if (o.it_trials) o.it_trials[k] = 0;
    for (int k = 0; k < kRounds; k++)
      if (o.round_iterations) o.round_iterations[k] = 0;
  }
  team.each(p.n_edges, [&](int e) { w.active[e] = 1; });
  int rounds_run = 0;
  bool stopped = false;
  for (int round = 0; round < prm.n_rounds && !stopped; round++) {
    if (stop_set(team, stop)) break;
    if (round == 1) {   // :507-518
      team.each(p.n_edges, [&](int e) { reclassify_edge(p, prm, w, e); });
    }
    count_active(team, p, w);
    double lambda = 0.0, ni = 2.0;
    int it = 0;
    while (it < prm.iterations[round]) {
      if (stop_set(team, stop)) {
        stopped = true;
        break;
      }
      const int trials = iteration(team, p, prm, w, nf, round, it == 0, &lambda, &ni, o, round * kMaxIterations + it);
      it++;
      if (trials < 0) break;
    }
    rounds_run = round + 1;
    if (team.leader() && o.round_iterations) o.round_iterations[round] = it;
    if (o.round_flags && round == 0)
      team.each(p.n_edges, [&](int e) { write_round0_flag(p, prm, w, o, e); });
  }
  // :530-540
  if (o.outliers || o.round_flags)
    team.each(p.n_edges, [&](int e) { write_final_flag(p, prm, w, o, rounds_run, e); });
  team.each(p.n_cams, [&](int c) { write_final_camera(p, w, o, rounds_run, c); });
  team.each(p.n_points * 3, [&](int k) { write_final_point(w, o, k); });
  return rounds_run;
}

}  // namespace ba
}  // namespace msf
#endif  // MSF_BA_SOLVE_H
