// The arithmetic of the loop body of LocalMapping::CreateNewMapPoints (slam_pipeline/src/LocalMapping.cc:195-265): one
// match of one list -> a new map point or the stage that rejects it.  Plain C++ shared by triangulate_kernels.hip and by
// a host build (tests/cpp/new_points_host.cpp), so every stage can be checked against a float64 SVD without a GPU.  Both
// builds use -ffp-contract=off: every expression rounds once per operation, in the order written.
//
// Types are those of the reference's expressions, and the conventions are the ones reconstruct_solve.h fixed for the
// same expressions:
//   * kp = (float) of the match's integers (cv::Point2f from cv::Point2i); invfx = 1.0f / fx; xn = ((kp.x - cx) * invfx,
//     (kp.y - cy) * invfy, 1) in f32, per view;
//   * ray = Rwc xn = Rcw' xn: f32 products summed left to right, as check_match does R p;
//   * cosParallaxRays in f64 on the f32 rays: Mat::dot and cv::norm return double -- products of the f32 entries in f64,
//     summed left to right, as check_match's cosParallax;
//   * the 4 x 4 matrix in f32 and its null vector by reconstruct::triangulate with P = [Rcw | tcw] and the normalised
//     coordinates; x3D = hom[0..2] / hom[3] in f32;
//   * from z1 on f64 arithmetic on f32 entries: Mat::dot returns double, invz = 1.0 / z is double, u = fx * x * invz + cx
//     promotes to double from the first product, and 5.991 is a double.
// Defined divergence: the reference's comparisons let a NaN point through every check and would store it; a non-finite
// x3D is rejected at stage 3 here, as check_match rejects it.  mMinParallax is compared with the COSINE exactly as the
// reference does (SlamParameters sets 1.1, so stage 2 rejects nothing by default); it is a parameter.
// Every loop is bounded (ransac::kMaxSweeps Jacobi sweeps): new_point ends on any input.
#ifndef MSF_TRIANGULATE_SOLVE_H
#define MSF_TRIANGULATE_SOLVE_H

#include "reconstruct_solve.h"

namespace msf {
namespace triangulate {

// msf_view / msf_match of include/msf_local_mapping.h, restated so that the host build needs no other header
struct View {
  float Rcw[9], tcw[3];
  float fx, fy, cx, cy;
};

struct Match {
  int32_t x1, y1, x2, y2;
};

constexpr int kNewPoint = 0;       // a new map point
constexpr int kCosNotPositive = 1; // !(cos > 0), a NaN cosine included
constexpr int kCosNotBelow = 2;    // !(cos < max_cos)
constexpr int kNoPoint = 3;        // hom[3] == 0, or a non-finite x3D
constexpr int kBehind1 = 4;        // z1 <= 0
constexpr int kBehind2 = 5;        // z2 <= 0
constexpr int kReprojection1 = 6;  // errX1^2 + errY1^2 > chi2
constexpr int kReprojection2 = 7;  // errX2^2 + errY2^2 > chi2

// xn and ray of one end point (:200-206)
MSF_HD void normalised_ray(float kx, float ky, const View& v, float* xn, float* ray) {
  const float invfx = 1.0f / v.fx, invfy = 1.0f / v.fy;
  xn[0] = (kx - v.cx) * invfx;
  xn[1] = (ky - v.cy) * invfy;
  xn[2] = 1.0f;
  for (int r = 0; r < 3; r++) {   // Rwc = Rcw'
    float sum = 0.0f;
    for (int k = 0; k < 3; k++) sum += v.Rcw[3 * k + r] * xn[k];
    ray[r] = sum;
  }
}

// row `r` of Rcw times x3D plus tcw[r]: Mat::dot (f64) + a float
MSF_HD double camera_coord(const View& v, int r, const float* x) {
  return ((double)v.Rcw[3 * r] * x[0] + (double)v.Rcw[3 * r + 1] * x[1] + (double)v.Rcw[3 * r + 2] * x[2]) + (double)v.tcw[r];
}

// errX^2 + errY^2 of x3D in view v against the key point (:243-251, :256-264); z is the depth already computed
MSF_HD double reprojection_error(const View& v, const float* x, double z, float kx, float ky) {
  const double xc = camera_coord(v, 0, x), yc = camera_coord(v, 1, x);
  const double invz = 1.0 / z;
  const double u = (double)v.fx * xc * invz + (double)v.cx;
  const double w = (double)v.fy * yc * invz + (double)v.cy;
  const double ex = u - (double)kx, ey = w - (double)ky;
  return ex * ex + ey * ey;
}

// The body of the loop for one match: returns 0 (a new map point) or the rejecting stage 1..7.  x3d [3]: the point,
// zero unless the status is 0.  hom [4]: the null vector before the division (zero for stages 1 and 2).  *cos:
// cosParallaxRays.
MSF_HD int new_point(const Match& m, const View& v1, const View& v2, double max_cos, double chi2, float* x3d, float* hom,
                     double* cos) {
  for (int k = 0; k < 3; k++) x3d[k] = 0.0f;
  for (int k = 0; k < 4; k++) hom[k] = 0.0f;
  const float k1x = (float)m.x1, k1y = (float)m.y1, k2x = (float)m.x2, k2y = (float)m.y2;
  float xn1[3], xn2[3], ray1[3], ray2[3];
  normalised_ray(k1x, k1y, v1, xn1, ray1);
  normalised_ray(k2x, k2y, v2, xn2, ray2);
  const double dot = (double)ray1[0] * ray2[0] + (double)ray1[1] * ray2[1] + (double)ray1[2] * ray2[2];
  const double n1 = sqrt((double)ray1[0] * ray1[0] + (double)ray1[1] * ray1[1] + (double)ray1[2] * ray1[2]);
  const double n2 = sqrt((double)ray2[0] * ray2[0] + (double)ray2[1] * ray2[1] + (double)ray2[2] * ray2[2]);
  const double c = dot / (n1 * n2);
  *cos = c;
  if (!(c > 0.0)) return kCosNotPositive;
  if (!(c < max_cos)) return kCosNotBelow;

  float T1[12], T2[12];   // Tcw = [Rcw | tcw]
  for (int r = 0; r < 3; r++)
    for (int col = 0; col < 4; col++) {
      T1[4 * r + col] = col < 3 ? v1.Rcw[3 * r + col] : v1.tcw[r];
      T2[4 * r + col] = col < 3 ? v2.Rcw[3 * r + col] : v2.tcw[r];
    }
  float p[3];
  reconstruct::triangulate(xn1[0], xn1[1], xn2[0], xn2[1], T1, T2, hom, p);
  if (hom[3] == 0.0f) return kNoPoint;
  if (!reconstruct::finite32(p[0]) || !reconstruct::finite32(p[1]) || !reconstruct::finite32(p[2])) return kNoPoint;

  const double z1 = camera_coord(v1, 2, p);
  if (z1 <= 0.0) return kBehind1;
  const double z2 = camera_coord(v2, 2, p);
  if (z2 <= 0.0) return kBehind2;
  if (reprojection_error(v1, p, z1, k1x, k1y) > chi2) return kReprojection1;
  if (reprojection_error(v2, p, z2, k2x, k2y) > chi2) return kReprojection2;
  for (int k = 0; k < 3; k++) x3d[k] = p[k];
  return kNewPoint;
}

}  // namespace triangulate
}  // namespace msf

#endif  // MSF_TRIANGULATE_SOLVE_H
