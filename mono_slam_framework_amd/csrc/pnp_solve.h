// The arithmetic of PnPsolver (slam_pipeline/src/PnPsolver.cc): one EPnP pose from n >= 4 correspondences
// (compute_pose, :453-500, and everything it calls), CheckInliers (:302-331) and the draw of a minimum set (:196-210).
// Plain C++ shared by pnp_kernels.hip and by a host build (tests/cpp/pnp_solve_host.cpp), so every stage can be checked
// against float64 numpy without a GPU.  Both builds use -ffp-contract=off; libm: sqrt, fabs, copysign only.  Every step
// is in f64, the type the reference's expressions have; points and intrinsics enter as f32 and are promoted on load.
//
// How the work is spread is a parameter (a "team"): the sums over the correspondences -- centroid, PW0'PW0, M'M, pc0,
// AB', the reprojection error -- go through team.sum, which is a plain loop for the four points of a minimum set
// (Serial), 64 strided partial sums joined by a butterfly on the device (pnp_kernels.hip) and the same 64 partial sums
// in the same order on the host (Emu64).  The symmetric 12 x 12 eigenproblem is a one-sided Jacobi on M'M itself: the
// device keeps row r of [M'M ; V] in lane r of a 16-lane group and gets the three dot products of a rotation as
// butterfly sums over the group; eig12_host does the same sums in the same order.
//
// Singular values: every SVD here is a one-sided (Hestenes) Jacobi, A V = B with mutually orthogonal columns b_j, so
// w_j = |b_j|, u_j = b_j / w_j.  A pair is rotated while |b_p . b_q| > 2^-52 |b_p| |b_q|; at most kMaxSweeps sweeps; a NaN
// makes every comparison false, so nothing rotates and NaN flows to the pose.
//
// Defined divergences from the reference:
//  * rep_errors[N].  :495 reads rep_errors[N] with N the member "number of all correspondences" where EPnP has
//    rep_errors[n], an out-of-bounds read for N > 3.  Here it is rep_errors[n].
//  * Singular qr_solve.  On a singular matrix the reference returns without writing X (stale or uninitialised); here
//    that Gauss-Newton step adds zero.
//  * Pseudo-inverse and least squares (cvInvert / cvSolve with CV_SVD): singular values at or below
//    2 DBL_EPSILON sum(w) are dropped, OpenCV's SVBkSb rule as recalled, not verifiable here [M].  Where none is
//    dropped the 3 x 3 pseudo-inverse is the inverse and is formed by cofactors (see pinv3).
//  * Null space of dimension above one.  A minimum set gives an 8 x 12 M, so M'M has a 4-dimensional null space and the
//    reference takes whatever basis cv::SVD leaves; the P4P pose depends on that basis, so there is no hypothesis-by-
//    hypothesis parity with any other SVD.  The canonical choice here: Ut's rows ordered by computed eigenvalue
//    descending, ties by column index, signs as the Jacobi leaves them; rows 8..11 then orthonormalised by one
//    Gram-Schmidt pass from row 11 upwards (row 11 keeps its direction).  The same holds for the signs of the PCA axes
//    of the control points (choose_control_points takes V's columns: for a symmetric positive semi-definite matrix U = V).
//  * estimate_R_and_t with a rank-2 AB' (coplanar camera points): U's third column is the cross product of the other
//    two, where cv::SVD completes the basis in its own way.  Rank below 2 gives a NaN pose.
//  * Non-finite poses score 0 inliers, since every comparison is false: as the reference.
#ifndef MSF_PNP_SOLVE_H
#define MSF_PNP_SOLVE_H

#include <math.h>
#include <stdint.h>

#include "ransac_solve.h"

namespace msf {
namespace pnp {

constexpr int kMaxSweeps = 30;
constexpr double kTol = 2.220446049250313e-16;   // 2^-52

struct Cam {
  double fu, fv, uc, vc;
};

// what one EPnP leaves behind: R | t row-major 3 x 4, and the diagnostics of msf_pnp_result
struct Solution {
  double pose[12];
  double cws[12];       // [4][3]
  double ut_tail[48];   // [4][12]: rows 8..11 of Ut
  double betas[12];     // [3][4]
  double rep[3];
  double pca[9];       // [3][3]: the unit PCA axes behind cws, by descending eigenvalue
};

// the Jacobi rotation that makes two columns with these dot products orthogonal; false: leave them
MSF_HD bool rotation(double alpha, double beta, double gamma, double* c, double* s) {
  if (!(fabs(gamma) > kTol * sqrt(alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  *c = 1.0 / sqrt(1.0 + t * t);
  *s = *c * t;
  return true;
}

// a: row-major R x N.  -> b[j * R + r] (column j of A V), v[j * N + r] (component r of v_j), w2[j] = |b_j|^2
template <int R, int N>
MSF_HD void svd_small(const double* a, double* b, double* v, double* w2) {
  for (int j = 0; j < N; j++) {
    for (int r = 0; r < R; r++) b[j * R + r] = a[r * N + j];
    for (int r = 0; r < N; r++) v[j * N + r] = r == j ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
    int rotated = 0;
    for (int p = 0; p < N - 1; p++) {
      for (int q = p + 1; q < N; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int r = 0; r < R; r++) {
          const double x = b[p * R + r], y = b[q * R + r];
          alpha += x * x;
          beta += y * y;
          gamma += x * y;
        }
        double c, s;
        if (!rotation(alpha, beta, gamma, &c, &s)) continue;
        for (int r = 0; r < R; r++) {
          const double x = b[p * R + r], y = b[q * R + r];
          b[p * R + r] = c * x - s * y;
          b[q * R + r] = s * x + c * y;
        }
        for (int r = 0; r < N; r++) {
          const double x = v[p * N + r], y = v[q * N + r];
          v[p * N + r] = c * x - s * y;
          v[q * N + r] = s * x + c * y;
        }
        rotated++;
      }
    }
    if (!rotated) break;
  }
  for (int j = 0; j < N; j++) {
    double sum = 0.0;
    for (int r = 0; r < R; r++) sum += b[j * R + r] * b[j * R + r];
    w2[j] = sum;
  }
}

// the cut of cvInvert / cvSolve(CV_SVD): singular values at or below it are dropped
template <int N>
MSF_HD double sv_cut(const double* w2) {
  double sum = 0.0;
  for (int j = 0; j < N; j++) sum += sqrt(w2[j]);
  return 2.0 * kTol * sum;
}

// cvSolve(A, rhs, x, CV_SVD): the minimum-norm least-squares solution of the R x N system
template <int R, int N>
MSF_HD void lstsq(const double* a, const double* rhs, double* x) {
  double b[N * R], v[N * N], w2[N];
  svd_small<R, N>(a, b, v, w2);
  const double cut = sv_cut<N>(w2);
  for (int r = 0; r < N; r++) x[r] = 0.0;
  for (int j = 0; j < N; j++) {
    if (!(sqrt(w2[j]) > cut)) continue;
    double dot = 0.0;
    for (int r = 0; r < R; r++) dot += b[j * R + r] * rhs[r];
    const double k = dot / w2[j];
    for (int r = 0; r < N; r++) x[r] += k * v[j * N + r];
  }
}

// cvInvert(CC, CC_inv, CV_SVD) of a 3 x 3.  The SVD decides the rank.  With no singular value cut the pseudo-inverse
// is the inverse, and it is taken by cofactors: CC's columns are the scaled PCA axes, orthogonal up to rounding, so the
// cross products and the determinant have no cancellation and the inverse is accurate to a few eps whatever the ratio
// of the axes' lengths; V W^-1 U' would leave eps cond(CC) in the alphas of a nearly coplanar set.
MSF_HD void pinv3(const double* a, double* inv) {
  double b[9], v[9], w2[3];
  svd_small<3, 3>(a, b, v, w2);
  const double cut = sv_cut<3>(w2);
  if (sqrt(w2[0]) > cut && sqrt(w2[1]) > cut && sqrt(w2[2]) > cut) {
    const double c0[3] = {a[4] * a[8] - a[5] * a[7], a[5] * a[6] - a[3] * a[8], a[3] * a[7] - a[4] * a[6]};
    const double det = a[0] * c0[0] + a[1] * c0[1] + a[2] * c0[2];
    inv[0] = c0[0] / det, inv[3] = c0[1] / det, inv[6] = c0[2] / det;
    inv[1] = (a[2] * a[7] - a[1] * a[8]) / det, inv[4] = (a[0] * a[8] - a[2] * a[6]) / det, inv[7] = (a[1] * a[6] - a[0] * a[7]) / det;
    inv[2] = (a[1] * a[5] - a[2] * a[4]) / det, inv[5] = (a[2] * a[3] - a[0] * a[5]) / det, inv[8] = (a[0] * a[4] - a[1] * a[3]) / det;
    return;
  }
  for (int k = 0; k < 9; k++) inv[k] = 0.0;
  for (int j = 0; j < 3; j++) {
    if (!(sqrt(w2[j]) > cut)) continue;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) inv[3 * r + c] += v[j * 3 + r] * b[j * 3 + c] / w2[j];
  }
}

// ---- the correspondences and the teams that sum over them ----
// A point source has count() and get(i, p, u) -> "point i takes part"; p = (X, Y, Z), u = (u, v), promoted from f32.

// the four points of a minimum set
struct SetPoints {
  const float* p3d;
  const float* p2d;
  const int32_t* set;
  MSF_HD int count() const { return 4; }
  MSF_HD bool get(int k, double* p, double* u) const {
    const int i = set[k];
    p[0] = p3d[3 * i], p[1] = p3d[3 * i + 1], p[2] = p3d[3 * i + 2];
    u[0] = p2d[2 * i], u[1] = p2d[2 * i + 1];
    return true;
  }
};

// where `pose` (R | t, row-major 3 x 4) sees the world point p: the pixel, through 1 / depth as the reference divides
MSF_HD void reproject(const double* pose, const Cam& cam, const double* p, double* pixel) {
  double c[3];
  for (int r = 0; r < 3; r++) c[r] = pose[4 * r] * p[0] + pose[4 * r + 1] * p[1] + pose[4 * r + 2] * p[2] + pose[4 * r + 3];
  const double inverse_depth = 1 / c[2];
  pixel[0] = cam.uc + cam.fu * c[0] * inverse_depth;
  pixel[1] = cam.vc + cam.fv * c[1] * inverse_depth;
}

// the squared pixel distance between the observation u and the reprojection of p
MSF_HD double reprojection2(const double* pose, const Cam& cam, const double* p, const double* u) {
  double pixel[2];
  reproject(pose, cam, p, pixel);
  const double du = u[0] - pixel[0], dv = u[1] - pixel[1];
  return du * du + dv * dv;
}

// CheckInliers for one point: strictly inside th2, a float promoted to double; a NaN is outside
MSF_HD bool is_inlier(const double* pose, const Cam& cam, float th2, const double* p, const double* u) {
  return reprojection2(pose, cam, p, u) < (double)th2;
}

// Refine's correspondences: the points of the list that are inliers of `pose`.  The flag is recomputed where it is
// needed (some twenty operations) instead of being stored.
struct InlierPoints {
  const float* p3d;
  const float* p2d;
  int n;
  const double* pose;
  Cam cam;
  float th2;
  MSF_HD int count() const { return n; }
  MSF_HD bool get(int i, double* p, double* u) const {
    p[0] = p3d[3 * i], p[1] = p3d[3 * i + 1], p[2] = p3d[3 * i + 2];
    u[0] = p2d[2 * i], u[1] = p2d[2 * i + 1];
    return is_inlier(pose, cam, th2, p, u);
  }
};

// out[k] = sum over the points of f(p, u, add)[k], in index order
struct Serial {
  template <int K, class Pts, class F>
  MSF_HD void sum(const Pts& pts, F f, double* out) const {
    for (int k = 0; k < K; k++) out[k] = 0.0;
    const int n = pts.count();
    for (int i = 0; i < n; i++) {
      double p[3], u[2], add[K];
      if (!pts.get(i, p, u)) continue;
      f(p, u, add);
      for (int k = 0; k < K; k++) out[k] += add[k];
    }
  }
  template <class Pts>
  MSF_HD int first(const Pts& pts) const {
    const int n = pts.count();
    double p[3], u[2];
    for (int i = 0; i < n; i++)
      if (pts.get(i, p, u)) return i;
    return -1;
  }
};

// the value every lane of a 2^k-lane butterfly ends with: x[i] + x[i ^ 1], then ^ 2, ...
template <int LANES>
inline double butterfly(double* x) {
  for (int m = 1; m < LANES; m <<= 1) {
    double y[LANES];
    for (int i = 0; i < LANES; i++) y[i] = x[i] + x[i ^ m];
    for (int i = 0; i < LANES; i++) x[i] = y[i];
  }
  return x[0];
}

// the host's restatement of the device's 64-lane team: lane l sums the points l, l + 64, ..., then the butterfly
struct Emu64 {
  template <int K, class Pts, class F>
  void sum(const Pts& pts, F f, double* out) const {
    double part[K][64];
    for (int k = 0; k < K; k++)
      for (int l = 0; l < 64; l++) part[k][l] = 0.0;
    const int n = pts.count();
    for (int i = 0; i < n; i++) {
      double p[3], u[2], add[K];
      if (!pts.get(i, p, u)) continue;
      f(p, u, add);
      for (int k = 0; k < K; k++) part[k][i & 63] += add[k];
    }
    for (int k = 0; k < K; k++) out[k] = butterfly<64>(part[k]);
  }
  template <class Pts>
  int first(const Pts& pts) const {
    return Serial().first(pts);
  }
};

// ---- choose_control_points (:362-392) ----
// -> the number of correspondences; cws [4][3]; pca [3][3]: the unit axes as the Jacobi leaves them, before they are
// scaled and folded into c0 + k axis
template <class Team, class Pts>
MSF_HD double choose_control_points(const Team& team, const Pts& pts, double* cws, double* pca) {
  double s[4];
  team.template sum<4>(pts, [](const double* p, const double*, double* add) {
    add[0] = p[0], add[1] = p[1], add[2] = p[2], add[3] = 1.0;
  }, s);
  const double n = s[3];
  double c0[3];
  for (int j = 0; j < 3; j++) c0[j] = s[j] / n;
  double m[6];   // PW0' PW0: xx xy xz yy yz zz
  team.template sum<6>(pts, [c0](const double* p, const double*, double* add) {
    const double x = p[0] - c0[0], y = p[1] - c0[1], z = p[2] - c0[2];
    add[0] = x * x, add[1] = x * y, add[2] = x * z, add[3] = y * y, add[4] = y * z, add[5] = z * z;
  }, m);
  const double a[9] = {m[0], m[1], m[2], m[1], m[3], m[4], m[2], m[4], m[5]};
  double b[9], v[9], w2[3];
  svd_small<3, 3>(a, b, v, w2);
  // rows of UCt by descending singular value, ties by column index
  int order[3];
  for (int j = 0; j < 3; j++) {
    int rank = 0;
    for (int k = 0; k < 3; k++) rank += (w2[k] > w2[j] || (w2[k] == w2[j] && k < j)) ? 1 : 0;
    order[j] = rank;
  }
  for (int j = 0; j < 3; j++) cws[j] = c0[j];
  for (int i = 1; i < 4; i++)
    for (int j = 0; j < 3; j++) cws[3 * i + j] = pca[3 * (i - 1) + j] = c0[j] * 0.0;   // NaN when no column has the rank (a NaN matrix)
  for (int col = 0; col < 3; col++) {
    const int i = order[col] + 1;
    const double k = sqrt(sqrt(w2[col]) / n);
    for (int j = 0; j < 3; j++) {
      cws[3 * i + j] = c0[j] + k * v[col * 3 + j];
      pca[3 * (i - 1) + j] = v[col * 3 + j];
    }
  }
  return n;
}

// cc and its pseudo-inverse (:395-402)
MSF_HD void control_inverse(const double* cws, double* ci) {
  double cc[9];
  for (int i = 0; i < 3; i++)
    for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[3 * j + i] - cws[i];
  pinv3(cc, ci);
}

// the alphas of one point (:404-413)
MSF_HD void barycentric(const double* ci, const double* cws, const double* p, double* a) {
  for (int j = 0; j < 3; j++)
    a[1 + j] = ci[3 * j] * (p[0] - cws[0]) + ci[3 * j + 1] * (p[1] - cws[1]) + ci[3 * j + 2] * (p[2] - cws[2]);
  a[0] = 1.0 - a[1] - a[2] - a[3];
}

// fill_M (:416-430): entry c of the two rows of M that a point contributes
MSF_HD void m_entry(const double* a, const double* u, const Cam& cam, int c, double* m1, double* m2) {
  const int j = c / 3, k = c - 3 * j;
  const double aj = j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3];
  *m1 = k == 0 ? aj * cam.fu : k == 1 ? 0.0 : aj * (cam.uc - u[0]);
  *m2 = k == 0 ? 0.0 : k == 1 ? aj * cam.fv : aj * (cam.vc - u[1]);
}

// row r of M'M gains what one point contributes (cvMulTransposed: the rows of M in order)
MSF_HD void mtm_row_add(const double* a, const double* u, const Cam& cam, int r, double* row) {
  double r1, r2;
  m_entry(a, u, cam, r, &r1, &r2);
  for (int c = 0; c < 12; c++) {
    double c1, c2;
    m_entry(a, u, cam, c, &c1, &c2);
    row[c] = row[c] + r1 * c1;
    row[c] = row[c] + r2 * c2;
  }
}

// Ut's row of column c: the number of columns in front of it (larger eigenvalue, or equal and a lower index)
MSF_HD int eig_rank(const double* norms, int c) {
  int rank = 0;
  for (int k = 0; k < 12; k++) rank += (norms[k] > norms[c] || (norms[k] == norms[c] && k < c)) ? 1 : 0;
  return rank;
}

// rows 8..11 of Ut made orthonormal: row 11 first, each earlier row against the later ones
MSF_HD void orthonormalise_tail(double* t) {
  for (int i = 3; i >= 0; i--) {
    for (int k = 3; k > i; k--) {
      double dot = 0.0;
      for (int c = 0; c < 12; c++) dot += t[12 * i + c] * t[12 * k + c];
      for (int c = 0; c < 12; c++) t[12 * i + c] -= dot * t[12 * k + c];
    }
    double norm2 = 0.0;
    for (int c = 0; c < 12; c++) norm2 += t[12 * i + c] * t[12 * i + c];
    const double norm = sqrt(norm2);
    for (int c = 0; c < 12; c++) t[12 * i + c] = t[12 * i + c] / norm;
  }
}

// The eigenvectors of the four smallest eigenvalues of the symmetric 12 x 12 `mtm`, as the device computes them: 16
// lanes, lane r holds row r of [M'M ; V] (lanes 12..15 hold zeros), the dot products of a pair are butterfly sums.
inline void eig12_host(const double* mtm, double* ut_tail) {
  double a[16][12], v[16][12];
  for (int r = 0; r < 16; r++)
    for (int c = 0; c < 12; c++) {
      a[r][c] = r < 12 ? mtm[12 * r + c] : 0.0;
      v[r][c] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < kMaxSweeps; sweep++) {
    int rotated = 0;
    for (int p = 0; p < 11; p++) {
      for (int q = p + 1; q < 12; q++) {
        double xa[16], xb[16], xg[16];
        for (int r = 0; r < 16; r++) xa[r] = a[r][p] * a[r][p], xb[r] = a[r][q] * a[r][q], xg[r] = a[r][p] * a[r][q];
        const double alpha = butterfly<16>(xa), beta = butterfly<16>(xb), gamma = butterfly<16>(xg);
        double c, s;
        if (!rotation(alpha, beta, gamma, &c, &s)) continue;
        for (int r = 0; r < 16; r++) {
          const double x = a[r][p], y = a[r][q], vx = v[r][p], vy = v[r][q];
          a[r][p] = c * x - s * y, a[r][q] = s * x + c * y;
          v[r][p] = c * vx - s * vy, v[r][q] = s * vx + c * vy;
        }
        rotated++;
      }
    }
    if (!rotated) break;
  }
  double norms[12], poison = 0.0;
  for (int c = 0; c < 12; c++) {
    double x[16];
    for (int r = 0; r < 16; r++) x[r] = a[r][c] * a[r][c];
    norms[c] = butterfly<16>(x);
    poison += norms[c] * 0.0;
  }
  for (int k = 0; k < 48; k++) ut_tail[k] = poison;
  for (int c = 0; c < 12; c++) {
    const int rank = eig_rank(norms, c);
    if (rank >= 8)
      for (int r = 0; r < 12; r++) ut_tail[12 * (rank - 8) + r] = v[r][c];
  }
  orthonormalise_tail(ut_tail);
}

// ---- everything behind the basis ----

// The six pairs of control points (a, b) with a < b, and the ten products beta_a beta_b with a <= b in the order EPnP
// numbers them: (0,0) (0,1) (1,1) (0,2) (1,2) (2,2) (0,3) (1,3) (2,3) (3,3).  kProduct[a][b] is the place of beta_a beta_b.
struct Tables {
  int pair[6][2];
  int factor[10][2];
  int product[4][4];
};
MSF_HD Tables tables() {
  return Tables{{{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}},
                {{0, 0}, {0, 1}, {1, 1}, {0, 2}, {1, 2}, {2, 2}, {0, 3}, {1, 3}, {2, 3}, {3, 3}},
                {{0, 1, 3, 6}, {1, 2, 4, 7}, {3, 4, 5, 8}, {6, 7, 8, 9}}};
}

MSF_HD double dot3(const double* x, const double* y) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// The 6 x 10 system of the distance constraints: row = a pair of control points, column = a product of two betas.  The
// basis vector of beta_i is row 11 - i of Ut; edge[i][row] is the difference of that vector's two control points, and an
// entry is the scalar product of two edges, doubled for a mixed product.
MSF_HD void compute_l(const double* ut_tail, double* l) {
  const Tables t = tables();
  double edge[4][6][3];
  for (int i = 0; i < 4; i++) {
    const double* basis = ut_tail + 12 * (3 - i);
    for (int row = 0; row < 6; row++)
      for (int k = 0; k < 3; k++) edge[i][row][k] = basis[3 * t.pair[row][0] + k] - basis[3 * t.pair[row][1] + k];
  }
  for (int row = 0; row < 6; row++)
    for (int col = 0; col < 10; col++) {
      const int a = t.factor[col][0], b = t.factor[col][1];
      const double sp = dot3(edge[a][row], edge[b][row]);
      l[10 * row + col] = a == b ? sp : 2.0 * sp;
    }
}

// the right-hand side: the squared distances of the world control points, pair by pair
MSF_HD void compute_rho(const double* cws, double* rho) {
  const Tables t = tables();
  for (int row = 0; row < 6; row++) {
    const double* p = cws + 3 * t.pair[row][0];
    const double* q = cws + 3 * t.pair[row][1];
    const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
    rho[row] = dx * dx + dy * dy + dz * dz;
  }
}

// the least-squares solution of the 6 x N system made of the columns `cols` of l
template <int N>
MSF_HD void solve_columns(const double* l, const int* cols, const double* rho, double* x) {
  double a[6 * N];
  for (int row = 0; row < 6; row++)
    for (int k = 0; k < N; k++) a[N * row + k] = l[10 * row + cols[k]];
  lstsq<6, N>(a, rho, x);
}

// The three starting points of the betas, which = 0, 1, 2: the linear system restricted to the products
//   0: b00 b01 b02 b03        1: b00 b01 b11        2: b00 b01 b11 b02 b12
// and the betas read off the solution x.  With s the sign that makes x[0] = b00 non-negative: beta0 = sqrt(s x[0]);
// which = 0: beta_k = s x[k] / beta0; else beta1 = sqrt(s x[2]) where that is positive (0 otherwise), beta0 takes the
// sign of x[1] = b01, and beta2 = x[3] / beta0 for which = 2.
MSF_HD void find_betas(int which, const double* l, const double* rho, double* betas) {
  double x[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  const int first[4] = {0, 1, 3, 6}, lower[5] = {0, 1, 2, 3, 4};
  if (which == 0)
    solve_columns<4>(l, first, rho, x);
  else if (which == 1)
    solve_columns<3>(l, lower, rho, x);
  else
    solve_columns<5>(l, lower, rho, x);
  const double s = x[0] < 0 ? -1.0 : 1.0;
  const double root = sqrt(s * x[0]);
  if (which == 0) {
    betas[0] = root;
    for (int k = 1; k < 4; k++) betas[k] = (s * x[k]) / root;
    return;
  }
  const double square1 = s * x[2];
  betas[0] = x[1] < 0 ? -root : root;
  betas[1] = square1 > 0 ? sqrt(square1) : 0.0;
  betas[2] = which == 2 ? x[3] / betas[0] : 0.0;
  betas[3] = 0.0;
}

// Householder QR solve of the 6 x 4 Gauss-Newton system, overwriting a and rhs.  Kept from EPnP's own solver because the
// bits depend on it: a column is scaled by its largest magnitude before its norm is taken, and the search for that
// magnitude looks at rows k .. 4 only -- never at the last row.  A column whose scale is 0 makes the system singular:
// x = 0 (defined divergence).  Reflector k is v = column k below the diagonal (after the update of its head), applied as
// y -= (v . y / denom[k]) v to the later columns and to the right-hand side.
MSF_HD void qr_solve(double* a, double* rhs, double* x) {
  constexpr int rows = 6, cols = 4;
  double denom[cols], diag[cols];
  auto reflect = [a](int k, double d, double* y, int stride) {
    double sp = 0;
    for (int i = k; i < rows; i++) sp += a[i * cols + k] * y[i * stride];
    const double f = sp / d;
    for (int i = k; i < rows; i++) y[i * stride] -= f * a[i * cols + k];
  };
  for (int k = 0; k < cols; k++) {
    double scale = fabs(a[k * cols + k]);
    for (int i = k; i < rows - 1; i++) {
      const double m = fabs(a[i * cols + k]);
      if (m > scale) scale = m;
    }
    if (scale == 0) {
      for (int i = 0; i < cols; i++) x[i] = 0.0;
      return;
    }
    const double shrink = 1. / scale;
    double norm2 = 0.0;
    for (int i = k; i < rows; i++) {
      a[i * cols + k] *= shrink;
      norm2 += a[i * cols + k] * a[i * cols + k];
    }
    const double length = a[k * cols + k] < 0 ? -sqrt(norm2) : sqrt(norm2);
    a[k * cols + k] += length;
    denom[k] = length * a[k * cols + k];
    diag[k] = -scale * length;
    for (int j = k + 1; j < cols; j++) reflect(k, denom[k], a + j, cols);
  }
  for (int k = 0; k < cols; k++) reflect(k, denom[k], rhs, 1);
  for (int i = cols - 1; i >= 0; i--) {
    double known = 0;
    for (int j = i + 1; j < cols; j++) known += a[i * cols + j] * x[j];
    x[i] = i == cols - 1 ? rhs[i] / diag[i] : (rhs[i] - known) / diag[i];
  }
}

// Five Gauss-Newton steps on f_row(beta) = sum over the ten products of l[row][.] beta_a beta_b - rho[row].
// d f_row / d beta_i = sum over m of l[row][product(i, m)] beta_m, the term m = i doubled; both sums run in the order of
// m and of the product numbering, which is what fixes the bits.
MSF_HD void gauss_newton(const double* l, const double* rho, double* betas) {
  const Tables t = tables();
  for (int step = 0; step < 5; step++) {
    double jac[24], res[6], dx[4];
    for (int row = 0; row < 6; row++) {
      const double* lr = l + 10 * row;
      for (int i = 0; i < 4; i++) {
        double sum = 0.0;
        for (int m = 0; m < 4; m++) {
          const double coef = lr[t.product[i][m]];
          const double term = (m == i ? 2 * coef : coef) * betas[m];
          sum = m == 0 ? term : sum + term;
        }
        jac[4 * row + i] = sum;
      }
      double model = 0.0;
      for (int col = 0; col < 10; col++) {
        const double term = lr[col] * betas[t.factor[col][0]] * betas[t.factor[col][1]];
        model = col == 0 ? term : model + term;
      }
      res[row] = rho[row] - model;
    }
    qr_solve(jac, res, dx);
    for (int i = 0; i < 4; i++) betas[i] += dx[i];
  }
}


// compute_R_and_t (:614-624): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error.
// `first`: the index of the first correspondence (pcs[2] is its depth).  -> the reprojection error; pose = R | t
template <class Team, class Pts>
MSF_HD double compute_r_and_t(const Team& team, const Pts& pts, int first, double n, const Cam& cam, const double* cws,
                              const double* ci, const double* ut_tail, const double* betas, double* pose) {
  double ccs[12];
  for (int k = 0; k < 12; k++) ccs[k] = 0.0;
  for (int i = 0; i < 4; i++) {
    const double* v = ut_tail + 12 * (3 - i);
    for (int k = 0; k < 12; k++) ccs[k] += betas[i] * v[k];
  }
  {
    double p[3] = {0.0, 0.0, 0.0}, u[2], a[4];
    if (first >= 0) pts.get(first, p, u);
    barycentric(ci, cws, p, a);
    const double z = a[0] * ccs[2] + a[1] * ccs[5] + a[2] * ccs[8] + a[3] * ccs[11];
    if (z < 0.0)
      for (int k = 0; k < 12; k++) ccs[k] = -ccs[k];
  }
  const double* cc = ccs;
  auto camera_point = [cc, ci, cws](const double* p, double* pc) {
    double a[4];
    barycentric(ci, cws, p, a);
    for (int j = 0; j < 3; j++) pc[j] = a[0] * cc[j] + a[1] * cc[3 + j] + a[2] * cc[6 + j] + a[3] * cc[9 + j];
  };
  double c[6];
  team.template sum<6>(pts, [&camera_point](const double* p, const double*, double* add) {
    camera_point(p, add);
    add[3] = p[0], add[4] = p[1], add[5] = p[2];
  }, c);
  double pc0[3], pw0[3];
  for (int j = 0; j < 3; j++) pc0[j] = c[j] / n, pw0[j] = c[3 + j] / n;
  double abt[9];
  team.template sum<9>(pts, [&camera_point, &pc0, &pw0](const double* p, const double*, double* add) {
    double pc[3];
    camera_point(p, pc);
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) add[3 * j + k] = (pc[j] - pc0[j]) * (p[k] - pw0[k]);
  }, abt);
  // AB' = U W V': AB' V = B, u_k = b_k / w_k
  double b[9], v[9], w2[3], w[3], uu[9];   // uu[k * 3 + i] = U[i][k]
  svd_small<3, 3>(abt, b, v, w2);
  const double cut = sv_cut<3>(w2);
  int lost = 0, which = 0;
  for (int k = 0; k < 3; k++) {
    w[k] = sqrt(w2[k]);
    if (w[k] <= cut) lost++, which = k;
    for (int i = 0; i < 3; i++) uu[3 * k + i] = b[3 * k + i] / w[k];
  }
  if (lost == 1) {
    const double* x = uu + 3 * ((which + 1) % 3);
    const double* y = uu + 3 * ((which + 2) % 3);
    uu[3 * which] = x[1] * y[2] - x[2] * y[1];
    uu[3 * which + 1] = x[2] * y[0] - x[0] * y[2];
    uu[3 * which + 2] = x[0] * y[1] - x[1] * y[0];
  }
  double R[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[3 * i + j] = uu[i] * v[j] + uu[3 + i] * v[3 + j] + uu[6 + i] * v[6 + j];
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] -
                     R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
  if (det < 0) {
    R[6] = -R[6];
    R[7] = -R[7];
    R[8] = -R[8];
  }
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) pose[4 * i + j] = R[3 * i + j];
    pose[4 * i + 3] = pc0[i] - dot3(R + 3 * i, pw0);
  }
  double err[1];
  const double* ps = pose;
  team.template sum<1>(pts, [ps, cam](const double* p, const double* u, double* add) {
    add[0] = sqrt(reprojection2(ps, cam, p, u));
  }, err);
  return err[0] / n;
}

// compute_pose behind cvSVD (:471-499): given the control points and rows 8..11 of Ut.  Fills sol->pose, betas, rep;
// -> the chosen candidate 0..2
template <class Team, class Pts>
MSF_HD int epnp_from(const Team& team, const Pts& pts, double n, const Cam& cam, Solution* sol) {
  double ci[9], l[60], rho[6];
  control_inverse(sol->cws, ci);
  compute_l(sol->ut_tail, l);
  compute_rho(sol->cws, rho);
  const int first = team.first(pts);
  double poses[3][12];
  for (int cand = 0; cand < 3; cand++) {
    double* betas = sol->betas + 4 * cand;
    find_betas(cand, l, rho, betas);
    gauss_newton(l, rho, betas);
    sol->rep[cand] = compute_r_and_t(team, pts, first, n, cam, sol->cws, ci, sol->ut_tail, betas, poses[cand]);
  }
  int chosen = 0;
  if (sol->rep[1] < sol->rep[0]) chosen = 1;
  if (sol->rep[2] < sol->rep[chosen]) chosen = 2;
  for (int k = 0; k < 12; k++) sol->pose[k] = chosen == 0 ? poses[0][k] : chosen == 1 ? poses[1][k] : poses[2][k];
  return chosen;
}

// ---- the draw of a minimum set (:196-210): four draws, swap with the last, without replacement; the generator and
// the key (seed, list, iteration, draw) of ransac::draw_set.  n >= 4, it < 2^20 ----
MSF_HD void draw_set4(uint64_t seed, int list, int it, int n, int32_t* set) {
  int pos[4], val[4];
  int size = n;
  for (int j = 0; j < 4; j++) {
    const uint64_t counter = (((uint64_t)(uint32_t)list << 20) + (uint64_t)(uint32_t)it) * 8 + (uint64_t)j;
    const uint64_t word = ransac::mix64(seed ^ ransac::mix64(counter + 0x9E3779B97F4A7C15ull));
    const int randi = (int)ransac::mulhi64(word, (uint64_t)size);
    int idx = randi, last = size - 1;
    for (int k = 0; k < j; k++) {
      if (pos[k] == randi) idx = val[k];
      if (pos[k] == size - 1) last = val[k];
    }
    set[j] = idx;
    pos[j] = randi;
    val[j] = last;
    size--;
  }
}

// a set is usable when its four indices lie inside the list (a caller's set may not)
MSF_HD bool set_in_range(const int32_t* set, int n) {
  bool ok = true;
  for (int k = 0; k < 4; k++) ok = ok && set[k] >= 0 && set[k] < n;
  return ok;
}

// ---- the host's whole solver: what the two kernels compute, list by list ----

// every array of one list; any pointer may be null
struct HostOut {
  int32_t* counts;         // [n_iterations]
  int32_t* sets;           // [n_iterations][4]
  double* pose_f64;        // [n_iterations][12]
  double* cws;             // [n_iterations][12]
  double* ut_tail;         // [n_iterations][48]
  double* betas;           // [n_iterations][12]
  double* rep_errors;      // [n_iterations][3]
  double* pca;             // [n_iterations][9]
  int32_t* iteration;      // [max_records]
  int32_t* n_inliers;      // [max_records]
  int32_t* refined_ok;     // [max_records]
  int32_t* n_refined;      // [max_records]
  float* tcw_best;         // [max_records][12]
  float* tcw_refined;      // [max_records][12]
  uint8_t* inliers_best;   // [max_records][cap]
  uint8_t* inliers_refined;
  double* rec_pose_f64;    // [max_records][12] ... the refine's own diagnostics
  double* rec_cws;
  double* rec_ut_tail;
  double* rec_betas;
  double* rec_rep_errors;
  double* rec_pca;
};

template <class Pts>
inline void full_mtm_serial(const Pts& pts, const Cam& cam, const double* cws, const double* ci, double* mtm) {
  for (int k = 0; k < 144; k++) mtm[k] = 0.0;
  const int n = pts.count();
  for (int i = 0; i < n; i++) {
    double p[3], u[2], a[4];
    if (!pts.get(i, p, u)) continue;
    barycentric(ci, cws, p, a);
    for (int r = 0; r < 12; r++) mtm_row_add(a, u, cam, r, mtm + 12 * r);
  }
}

// the device's order for Refine: the points i = g (mod 4) in group g, then (g0 + g1) + (g2 + g3)
template <class Pts>
inline void full_mtm_groups(const Pts& pts, const Cam& cam, const double* cws, const double* ci, double* mtm) {
  double part[4][144];
  for (int g = 0; g < 4; g++)
    for (int k = 0; k < 144; k++) part[g][k] = 0.0;
  const int n = pts.count();
  for (int i = 0; i < n; i++) {
    double p[3], u[2], a[4];
    if (!pts.get(i, p, u)) continue;
    barycentric(ci, cws, p, a);
    for (int r = 0; r < 12; r++) mtm_row_add(a, u, cam, r, part[i & 3] + 12 * r);
  }
  for (int k = 0; k < 144; k++) mtm[k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
}

// one hypothesis: P4P EPnP on the set (with `given` = {cws, ut_tail} the basis is taken, not computed)
inline void p4p_host(const float* p3d, const float* p2d, const int32_t* set, const Cam& cam, Solution* sol) {
  const SetPoints pts{p3d, p2d, set};
  const Serial team;
  const double n = choose_control_points(team, pts, sol->cws, sol->pca);
  double ci[9], mtm[144];
  control_inverse(sol->cws, ci);
  full_mtm_serial(pts, cam, sol->cws, ci, mtm);
  eig12_host(mtm, sol->ut_tail);
  epnp_from(team, pts, n, cam, sol);
}

// Refine's EPnP (:259-281) over the inliers of `best`
inline void refine_host(const float* p3d, const float* p2d, int n, const double* best, const Cam& cam, float th2,
                        Solution* sol) {
  const InlierPoints pts{p3d, p2d, n, best, cam, th2};
  const Emu64 team;
  const double m = choose_control_points(team, pts, sol->cws, sol->pca);
  double ci[9], mtm[144];
  control_inverse(sol->cws, ci);
  full_mtm_groups(pts, cam, sol->cws, ci, mtm);
  eig12_host(mtm, sol->ut_tail);
  epnp_from(team, pts, m, cam, sol);
}

inline int count_inliers(const float* p3d, const float* p2d, int n, const double* pose, const Cam& cam, float th2,
                         uint8_t* flags) {
  int count = 0;
  for (int i = 0; i < n; i++) {
    const double p[3] = {p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]}, u[2] = {p2d[2 * i], p2d[2 * i + 1]};
    const bool in = is_inlier(pose, cam, th2, p, u);
    if (flags) flags[i] = in ? 1 : 0;
    count += in ? 1 : 0;
  }
  return count;
}

// iterations [0, n_iterations) of one list and its records.  -> the true number of records, -1 for n < 4.
inline int ransac_host(int n, const float* p3d, const float* p2d, const Cam& cam, float th2, int min_inliers,
                       int n_iterations, int max_records, uint64_t seed, int list, const int32_t* sets, int cap,
                       const HostOut& o) {
  if (n < 4) return -1;
  int records = 0, best = 0;
  for (int it = 0; it < n_iterations; it++) {
    int32_t set[4];
    if (sets)
      for (int k = 0; k < 4; k++) set[k] = sets[4 * it + k];
    else
      draw_set4(seed, list, it, n, set);
    if (o.sets && !sets)
      for (int k = 0; k < 4; k++) o.sets[4 * it + k] = set[k];
    Solution sol;
    int count = 0;
    if (set_in_range(set, n)) {
      p4p_host(p3d, p2d, set, cam, &sol);
      count = count_inliers(p3d, p2d, n, sol.pose, cam, th2, nullptr);
    } else {
      double* all = sol.pose;   // Solution is six arrays of doubles
      for (size_t k = 0; k < sizeof(Solution) / sizeof(double); k++) all[k] = NAN;
    }
    if (o.counts) o.counts[it] = count;
    if (o.pose_f64) for (int k = 0; k < 12; k++) o.pose_f64[12 * it + k] = sol.pose[k];
    if (o.cws) for (int k = 0; k < 12; k++) o.cws[12 * it + k] = sol.cws[k];
    if (o.ut_tail) for (int k = 0; k < 48; k++) o.ut_tail[48 * it + k] = sol.ut_tail[k];
    if (o.betas) for (int k = 0; k < 12; k++) o.betas[12 * it + k] = sol.betas[k];
    if (o.rep_errors) for (int k = 0; k < 3; k++) o.rep_errors[3 * it + k] = sol.rep[k];
    if (o.pca) for (int k = 0; k < 9; k++) o.pca[9 * it + k] = sol.pca[k];
    if (count < min_inliers || count <= best) continue;
    best = count;
    const int rec = records++;
    if (rec >= max_records) continue;
    Solution ref;
    refine_host(p3d, p2d, n, sol.pose, cam, th2, &ref);
    if (o.inliers_best) count_inliers(p3d, p2d, n, sol.pose, cam, th2, o.inliers_best + (size_t)rec * cap);
    const int n_refined =
        count_inliers(p3d, p2d, n, ref.pose, cam, th2, o.inliers_refined ? o.inliers_refined + (size_t)rec * cap : nullptr);
    if (o.iteration) o.iteration[rec] = it;
    if (o.n_inliers) o.n_inliers[rec] = count;
    if (o.n_refined) o.n_refined[rec] = n_refined;
    if (o.refined_ok) o.refined_ok[rec] = n_refined > min_inliers ? 1 : 0;
    if (o.tcw_best) for (int k = 0; k < 12; k++) o.tcw_best[12 * rec + k] = (float)sol.pose[k];
    if (o.tcw_refined) for (int k = 0; k < 12; k++) o.tcw_refined[12 * rec + k] = (float)ref.pose[k];
    if (o.rec_pose_f64) for (int k = 0; k < 12; k++) o.rec_pose_f64[12 * rec + k] = ref.pose[k];
    if (o.rec_cws) for (int k = 0; k < 12; k++) o.rec_cws[12 * rec + k] = ref.cws[k];
    if (o.rec_ut_tail) for (int k = 0; k < 48; k++) o.rec_ut_tail[48 * rec + k] = ref.ut_tail[k];
    if (o.rec_betas) for (int k = 0; k < 12; k++) o.rec_betas[12 * rec + k] = ref.betas[k];
    if (o.rec_rep_errors) for (int k = 0; k < 3; k++) o.rec_rep_errors[3 * rec + k] = ref.rep[k];
    if (o.rec_pca) for (int k = 0; k < 9; k++) o.rec_pca[9 * rec + k] = ref.pca[k];
  }
  return records;
}

}  // namespace pnp
}  // namespace msf

#endif  // MSF_PNP_SOLVE_H
