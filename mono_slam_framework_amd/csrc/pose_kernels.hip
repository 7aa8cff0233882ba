// Optimizer::PoseOptimization (slam_pipeline/src/Optimizer.cc:217-334) on the device, for one list of 3-D / 2-D
// correspondences or a batch:
//   k_pose_optimize   one wave per list: four rounds of a pose-only Levenberg-Marquardt (Huber in rounds 0..2), every
//                     correspondence re-flagged by chi2 after each round
// One launch.  The arithmetic is pose_solve.h, shared with a host build that is checked against float64 without a GPU.
// Every loop is bounded (4 rounds x 10 iterations x 10 trials, ceil(n / 64) strides); no workgroup waits on another;
// no LDS, no atomics: the lanes talk by __shfl_xor.
//
// Lane l takes the correspondences l, l + 64, ... and accumulates the 21 + 6 + 1 sums of an iteration (a trial: the
// cost alone); the butterfly leaves the same bits in every lane, so the Cholesky, exp and the lambda logic run on all
// lanes redundantly and the wave takes every branch together.  Whether a correspondence is active in a round is
// recomputed from the previous round's pose wherever it is needed, and its outlier flag is stored by the lane that
// owns its index.
//
// Order independence: a list's result is a function of its points, mask and entry pose alone, and its sums have a fixed
// shape, so a list gives the same bits alone or in any row of any batch.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "pose_pipeline.h"
#include "pose_solve.h"

namespace msf {

namespace {

// the device's 64-lane team of pnp_solve.h (pnp::Emu64 is its host restatement)
struct PoseWave64 {
  int lane;
  template <int K, class Pts, class F>
  __device__ void sum(const Pts& pts, F f, double* out) const {
#pragma unroll
    for (int k = 0; k < K; k++) out[k] = 0.0;
    const int n = pts.count();
    for (int i = lane; i < n; i += 64) {
      double p[3], u[2], add[K];
      if (!pts.get(i, p, u)) continue;
      f(p, u, add);
#pragma unroll
      for (int k = 0; k < K; k++) out[k] += add[k];
    }
#pragma unroll
    for (int k = 0; k < K; k++)
#pragma unroll
      for (int m = 1; m < 64; m <<= 1) out[k] += __shfl_xor(out[k], m);
  }
};

}  // namespace

// 64 threads = one wave = one list; grid: n_lists.
__global__ __launch_bounds__(64) void k_pose_optimize(PoseLists in, PoseParams prm, PoseOut out) {
  const int list = blockIdx.x, lane = threadIdx.x;
  const int given = in.n ? in.n[list] : in.n_single;
  if (given < 0) {   // uniform
    if (lane == 0) out.n_good[list] = -1;
    return;
  }
  const int n = given < in.cap ? given : in.cap;
  const long long row = (long long)list * in.cap;
  const float* tcw0 = in.tcw0 + (long long)list * in.tcw0_stride;
  const pose::Edges edges{in.p3d + row * 3,
                          in.p2d + row * 2,
                          in.mask ? in.mask + (long long)list * in.mask_stride : nullptr,
                          n,
                          pose::Cam{(double)prm.fx, (double)prm.fy, (double)prm.cx, (double)prm.cy},
                          prm.chi2,
                          false,
                          {}};
  const long long r4 = (long long)list * pose::kRounds, i40 = r4 * pose::kIterations;
  const pose::Trace tr{out.round_pose_f64 ? out.round_pose_f64 + r4 * 12 : nullptr,
                       out.round_n_bad ? out.round_n_bad + r4 : nullptr,
                       out.round_iterations ? out.round_iterations + r4 : nullptr,
                       out.it_trials ? out.it_trials + i40 : nullptr,
                       out.it_lambda_in ? out.it_lambda_in + i40 : nullptr,
                       out.it_lambda_out ? out.it_lambda_out + i40 : nullptr,
                       out.it_cost_in ? out.it_cost_in + i40 : nullptr,
                       out.it_cost_out ? out.it_cost_out + i40 : nullptr,
                       out.it_H ? out.it_H + i40 * 21 : nullptr,
                       out.it_b ? out.it_b + i40 * 6 : nullptr,
                       out.it_pose_out ? out.it_pose_out + i40 * 7 : nullptr,
                       lane == 0};
  const PoseWave64 team{lane};
  const pose::Outcome r = pose::pose_optimization(team, edges, tcw0, tr);
  if (out.outliers)
    for (int i = lane; i < n; i += 64) {
      double p[3], u[2];
      if (!edges.edge(i, p, u)) continue;
      out.outliers[row + i] = r.rounds_run && pose::flagged(r.pose, edges.cam, prm.chi2, p, u) ? 1 : 0;
    }
  if (lane != 0) return;
  out.n_good[list] = r.n_good;
  if (out.n_edges) out.n_edges[list] = r.n_edges;
  if (out.rounds_run) out.rounds_run[list] = r.rounds_run;
  for (int k = 0; k < 12; k++) {
    if (out.pose_f64) out.pose_f64[(long long)list * 12 + k] = r.pose[k];
    if (out.tcw) out.tcw[(long long)list * 12 + k] = r.rounds_run ? (float)r.pose[k] : tcw0[k];
  }
}

hipError_t pose_optimize(int n_lists, const PoseLists& in, const PoseParams& prm, const PoseOut& out, hipStream_t st) {
  if (n_lists <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pose_optimize, dim3(n_lists), dim3(64), 0, st, in, prm, out);
  return hipGetLastError();
}

}  // namespace msf
