// PnPsolver (slam_pipeline/src/PnPsolver.cc) on the device, for one list of 3-D / 2-D correspondences or a batch:
//   k_pnp_hypotheses  one RANSAC iteration per 16-lane group: the draw (or the caller's set), P4P EPnP, the inlier count
//   k_pnp_records     one wave per list: the record-setting iterations, and for each Refine (:259-300) -- EPnP over the
//                     record's inliers, then CheckInliers
// Two launches ordered by the stream.  The arithmetic is pnp_solve.h, shared with a host build that is checked against
// float64 without a GPU.  Every loop is bounded (pnp::kMaxSweeps Jacobi sweeps, ceil(n / lanes) strides,
// n_iterations); no workgroup waits on another; nothing is exchanged through LDS: a group's lanes talk by ds_bpermute.
//
// The 12 x 12 eigenproblem: a one-sided Jacobi on M'M whose [M'M ; V] is 24 x 12 doubles.  Lane r
// of a 16-lane group keeps row r of M'M and row r of V in registers (lanes 12..15 keep zeros); the pair loops are fully
// unrolled, so the register indices are static; alpha, beta and gamma of a pair are butterfly sums over the group
// (__shfl_xor 1, 2, 4, 8), which leave the same bits in every lane, so the group takes every branch together.
//
// Order independence: a hypothesis is a function of (seed, list, iteration) or of its given set and of the list alone;
// a record of the list's counts and points alone.  The sums over a record's inliers have a fixed shape (lane l takes
// the points l, l + 64, ...; then the butterfly), so a list gives the same bits alone or in any batch.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pnp_pipeline.h"
#include "pnp_solve.h"

namespace msf {

namespace {

__device__ inline double sum16(double x) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) x += __shfl_xor(x, m);
  return x;
}

__device__ inline int isum(int x, int lanes) {
  for (int m = 1; m < lanes; m <<= 1) x += __shfl_xor(x, m);
  return x;
}

// the device's 64-lane team of pnp_solve.h: lane l sums the points l, l + 64, ..., then the butterfly (pnp::Emu64 is
// its host restatement)
struct Wave64 {
  int lane;
  template <int K, class Pts, class F>
  __device__ void sum(const Pts& pts, F f, double* out) const {
    for (int k = 0; k < K; k++) out[k] = 0.0;
    const int n = pts.count();
    for (int i = lane; i < n; i += 64) {
      double p[3], u[2], add[K];
      if (!pts.get(i, p, u)) continue;
      f(p, u, add);
      for (int k = 0; k < K; k++) out[k] += add[k];
    }
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) out[k] += __shfl_xor(out[k], m);
  }
  template <class Pts>
  __device__ int first(const Pts& pts) const {
    const int n = pts.count();
    int mine = 0x7fffffff;
    double p[3], u[2];
    for (int i = lane; i < n; i += 64)
      if (pts.get(i, p, u)) {
        mine = i;
        break;
      }
    for (int m = 1; m < 64; m <<= 1) {
      const int other = __shfl_xor(mine, m);
      mine = other < mine ? other : mine;
    }
    return mine == 0x7fffffff ? -1 : mine;
  }
};

// rows 8..11 of Ut from row r (r = lane & 15; zeros for r >= 12) of the symmetric 12 x 12 matrix; every lane of the
// group gets all of ut_tail.  pnp::eig12_host is the same arithmetic.
__device__ inline void eig12_group(int r, double* a, double* ut_tail) {
  double v[12];
#pragma unroll
  for (int c = 0; c < 12; c++) v[c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < pnp::kMaxSweeps; sweep++) {
    int rotated = 0;
#pragma unroll
    for (int p = 0; p < 11; p++) {
#pragma unroll
      for (int q = p + 1; q < 12; q++) {
        const double alpha = sum16(a[p] * a[p]), beta = sum16(a[q] * a[q]), gamma = sum16(a[p] * a[q]);
        double c, s;
        if (!pnp::rotation(alpha, beta, gamma, &c, &s)) continue;
        const double x = a[p], y = a[q], vx = v[p], vy = v[q];
        a[p] = c * x - s * y, a[q] = s * x + c * y;
        v[p] = c * vx - s * vy, v[q] = s * vx + c * vy;
        rotated++;
      }
    }
    if (!rotated) break;
  }
  double norms[12], poison = 0.0;
#pragma unroll
  for (int c = 0; c < 12; c++) {
    norms[c] = sum16(a[c] * a[c]);
    poison += norms[c] * 0.0;
  }
  double mine[4] = {poison, poison, poison, poison};
#pragma unroll
  for (int c = 0; c < 12; c++) {
    const int rank = pnp::eig_rank(norms, c);
#pragma unroll
    for (int t = 0; t < 4; t++) mine[t] = rank == 8 + t ? v[c] : mine[t];
  }
#pragma unroll
  for (int t = 0; t < 4; t++)
#pragma unroll
    for (int k = 0; k < 12; k++) ut_tail[12 * t + k] = __shfl(mine[t], k, 16);
  pnp::orthonormalise_tail(ut_tail);
}

__device__ inline pnp::Cam camera(const PnpParams& prm) {
  return pnp::Cam{(double)prm.fx, (double)prm.fy, (double)prm.cx, (double)prm.cy};
}

// the length of list `list`, or -1 when it has no valid result
__device__ inline int list_length(const PnpLists& in, int list) {
  const int given = in.n ? in.n[list] : in.n_single;
  const int n = given < in.cap ? given : in.cap;
  return n < 4 ? -1 : n;
}

__device__ inline void store12(double* dst, const double* src) {
  if (!dst) return;
  for (int k = 0; k < 12; k++) dst[k] = src[k];
}

}  // namespace

// 64 threads = four 16-lane groups, one hypothesis (list, iteration) per group; grid: ceil(n_lists * n_iterations / 4).
// The four points, the control points and everything behind the basis are computed by every lane of the group (the
// same values in each: no exchange needed); the Jacobi is spread over the group; the inlier count is strided over it.
__global__ __launch_bounds__(64) void k_pnp_hypotheses(PnpLists in, PnpParams prm, PnpOut out, long long total) {
  const int tid = threadIdx.x, r = tid & 15;
  const long long hyp = (long long)blockIdx.x * 4 + (tid >> 4);
  if (hyp >= total) return;   // a whole group
  const int list = (int)(hyp / prm.n_iterations), it = (int)(hyp % prm.n_iterations);
  const int n = list_length(in, list);
  if (n < 0) return;          // a whole group; k_pnp_records reports the list
  const float* p3d = in.p3d + (long long)list * in.cap * 3;
  const float* p2d = in.p2d + (long long)list * in.cap * 2;
  const pnp::Cam cam = camera(prm);
  int32_t set[4];
  if (in.sets) {
    for (int k = 0; k < 4; k++) set[k] = in.sets[hyp * 4 + k];
  } else {
    pnp::draw_set4(prm.seed, list, it, n, set);
    if (out.sets && r == 0)
      for (int k = 0; k < 4; k++) out.sets[hyp * 4 + k] = set[k];
  }
  pnp::Solution sol;
  int count = 0;
  if (pnp::set_in_range(set, n)) {
    const pnp::SetPoints pts{p3d, p2d, set};
    const pnp::Serial team;
    const double m = pnp::choose_control_points(team, pts, sol.cws, sol.pca);
    double ci[9], row[12];
    pnp::control_inverse(sol.cws, ci);
#pragma unroll
    for (int c = 0; c < 12; c++) row[c] = 0.0;
    for (int k = 0; k < 4; k++) {
      double p[3], u[2], a[4];
      pts.get(k, p, u);
      pnp::barycentric(ci, sol.cws, p, a);
      pnp::mtm_row_add(a, u, cam, r < 12 ? r : 0, row);
    }
#pragma unroll
    for (int c = 0; c < 12; c++) row[c] = r < 12 ? row[c] : 0.0;
    eig12_group(r, row, sol.ut_tail);
    pnp::epnp_from(team, pts, m, cam, &sol);
    for (int i = r; i < n; i += 16) {
      const double p[3] = {p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]}, u[2] = {p2d[2 * i], p2d[2 * i + 1]};
      count += pnp::is_inlier(sol.pose, cam, prm.th2, p, u) ? 1 : 0;
    }
    count = isum(count, 16);
  } else {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int k = 0; k < 12; k++) sol.pose[k] = sol.cws[k] = sol.betas[k] = nan;
    for (int k = 0; k < 48; k++) sol.ut_tail[k] = nan;
    for (int k = 0; k < 3; k++) sol.rep[k] = nan;
    for (int k = 0; k < 9; k++) sol.pca[k] = nan;
  }
  if (r != 0) return;
  out.counts[hyp] = count;
  store12(out.pose_f64 + hyp * 12, sol.pose);
  store12(out.cws ? out.cws + hyp * 12 : nullptr, sol.cws);
  store12(out.betas ? out.betas + hyp * 12 : nullptr, sol.betas);
  if (out.ut_tail)
    for (int k = 0; k < 48; k++) out.ut_tail[hyp * 48 + k] = sol.ut_tail[k];
  if (out.rep_errors)
    for (int k = 0; k < 3; k++) out.rep_errors[hyp * 3 + k] = sol.rep[k];
  if (out.pca)
    for (int k = 0; k < 9; k++) out.pca[hyp * 9 + k] = sol.pca[k];
}

// One wave per list; grid: n_lists.  The wave walks the list's counts (uniform loads) and, at every record, refines it:
// the sums over the record's inliers go through Wave64; row r of M'M is gathered by the lanes (g, r), g = lane / 16
// taking the points i = g (mod 4), and joined across the four groups, which then run the same Jacobi on the same bits.
__global__ __launch_bounds__(64) void k_pnp_records(PnpLists in, PnpParams prm, PnpOut out) {
  const int list = blockIdx.x, lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int n = list_length(in, list);
  if (n < 0) {   // uniform
    if (lane == 0) out.n_records[list] = -1;
    return;
  }
  const float* p3d = in.p3d + (long long)list * in.cap * 3;
  const float* p2d = in.p2d + (long long)list * in.cap * 2;
  const pnp::Cam cam = camera(prm);
  const long long hyp0 = (long long)list * prm.n_iterations;
  int records = 0, best = 0;
  for (int it = 0; it < prm.n_iterations; it++) {
    const int count = out.counts[hyp0 + it];
    if (count < prm.min_inliers || count <= best) continue;
    best = count;
    const int rec = records++;
    if (rec >= prm.max_records) continue;
    const long long at = (long long)list * prm.max_records + rec;
    double pose[12];
    for (int k = 0; k < 12; k++) pose[k] = out.pose_f64[(hyp0 + it) * 12 + k];
    const pnp::InlierPoints pts{p3d, p2d, n, pose, cam, prm.th2};
    const Wave64 team{lane};
    pnp::Solution sol;
    const double m = pnp::choose_control_points(team, pts, sol.cws, sol.pca);
    double ci[9], row[12];
    pnp::control_inverse(sol.cws, ci);
#pragma unroll
    for (int c = 0; c < 12; c++) row[c] = 0.0;
    for (int i = g; i < n; i += 4) {
      double p[3], u[2], a[4];
      if (!pts.get(i, p, u)) continue;
      pnp::barycentric(ci, sol.cws, p, a);
      pnp::mtm_row_add(a, u, cam, r < 12 ? r : 0, row);
    }
#pragma unroll
    for (int c = 0; c < 12; c++) {
      row[c] += __shfl_xor(row[c], 16);
      row[c] += __shfl_xor(row[c], 32);
      row[c] = r < 12 ? row[c] : 0.0;
    }
    eig12_group(r, row, sol.ut_tail);
    pnp::epnp_from(team, pts, m, cam, &sol);
    int n_refined = 0;
    for (int i = lane; i < n; i += 64) {
      const double p[3] = {p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]}, u[2] = {p2d[2 * i], p2d[2 * i + 1]};
      const bool was = pnp::is_inlier(pose, cam, prm.th2, p, u), is = pnp::is_inlier(sol.pose, cam, prm.th2, p, u);
      if (out.inliers_best) out.inliers_best[at * in.cap + i] = was ? 1 : 0;
      if (out.inliers_refined) out.inliers_refined[at * in.cap + i] = is ? 1 : 0;
      n_refined += is ? 1 : 0;
    }
    n_refined = isum(n_refined, 64);
    if (lane != 0) continue;
    if (out.iteration) out.iteration[at] = it;
    if (out.n_inliers) out.n_inliers[at] = count;
    if (out.n_refined) out.n_refined[at] = n_refined;
    if (out.refined_ok) out.refined_ok[at] = n_refined > prm.min_inliers ? 1 : 0;
    if (out.tcw_best)
      for (int k = 0; k < 12; k++) out.tcw_best[at * 12 + k] = (float)pose[k];
    if (out.tcw_refined)
      for (int k = 0; k < 12; k++) out.tcw_refined[at * 12 + k] = (float)sol.pose[k];
    store12(out.rec_pose_f64 ? out.rec_pose_f64 + at * 12 : nullptr, sol.pose);
    store12(out.rec_cws ? out.rec_cws + at * 12 : nullptr, sol.cws);
    store12(out.rec_betas ? out.rec_betas + at * 12 : nullptr, sol.betas);
    if (out.rec_ut_tail)
      for (int k = 0; k < 48; k++) out.rec_ut_tail[at * 48 + k] = sol.ut_tail[k];
    if (out.rec_rep_errors)
      for (int k = 0; k < 3; k++) out.rec_rep_errors[at * 3 + k] = sol.rep[k];
    if (out.rec_pca)
      for (int k = 0; k < 9; k++) out.rec_pca[at * 9 + k] = sol.pca[k];
  }
  if (lane == 0) out.n_records[list] = records;
}

hipError_t pnp_ransac(int n_lists, const PnpLists& in, const PnpParams& prm, const PnpOut& out, hipStream_t st) {
  if (n_lists <= 0) return hipSuccess;
  const long long total = (long long)n_lists * prm.n_iterations;
  hipLaunchKernelGGL(k_pnp_hypotheses, dim3((unsigned)((total + 3) / 4)), dim3(64), 0, st, in, prm, out, total);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_pnp_records, dim3(n_lists), dim3(64), 0, st, in, prm, out);
  return hipGetLastError();
}

}  // namespace msf
