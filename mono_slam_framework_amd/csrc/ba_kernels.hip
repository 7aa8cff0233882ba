// Optimizer::LocalBundleAdjustment (slam_pipeline/src/Optimizer.cc:336-574) and Optimizer::BundleAdjustment (:71-215)
// on the device, for one problem or a batch:
//   k_bundle_adjust   one workgroup of 256 threads per problem: up to two rounds of a Schur-complement
//                     Levenberg-Marquardt over poses and points, the edges re-classified by chi2 and depth between them
// One launch.  The arithmetic is ba_solve.h, shared with a host build that is checked against float64 without a GPU.
// Every loop is bounded (2 rounds x 32 iterations x 10 trials, strides over the problem's own counts); the workgroup
// joins with __syncthreads only: no wait on another workgroup, no spin on memory, no atomics, and no LDS but the 256
// bytes the compiler keeps for __syncthreads_or.
//
// Every phase of ba_solve.h is "for every index in [0, n)" and a join: thread t takes the indices t, t + 256, ... and
// each index writes what it alone owns, so the sums have the order the host build gives them.  What the team decides
// on (a trial's cost, a pivot, the stop word) every thread reads from the same scratch word after a join, or agrees on
// with __syncthreads_or, so the workgroup takes every branch together.  The scratch is global memory (a problem's S is
// up to 385 x 384 doubles); it stays in the L2 of the problem's XCD.
//
// A malformed problem -- an index out of range, edge_point decreasing, a negative count, a range beyond the call's
// totals, more free cameras than max_free_cams -- gets status -1 and nothing else; no index is used before it is checked.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ba_pipeline.h"
#include "ba_solve.h"

namespace msf {

namespace {

constexpr int kBaThreads = 256;

struct Block256 {
  int tid;
  template <class F>
  __device__ void each(int n, F f) const {
    for (int i = tid; i < n; i += kBaThreads) f(i);
    __syncthreads();
  }
  __device__ bool any(bool b) const { return __syncthreads_or(b ? 1 : 0) != 0; }
  __device__ bool leader() const { return tid == 0; }
  __device__ void join() const { __syncthreads(); }
};

template <class T>
__device__ T* at(T* p, long long i) {
  return p ? p + i : nullptr;
}

}  // namespace

// 256 threads = one problem; grid: n_problems.
__global__ __launch_bounds__(kBaThreads) void k_bundle_adjust(BaBatch in, ba::Params prm, ba::Scratch scratch, BaOut out) {
  const int problem = blockIdx.x, tid = threadIdx.x;
  const msf_ba_problem d = in.problems[problem];
  const long long nc = d.n_cams, np = d.n_points, ne = d.n_edges, c0 = d.cam0, p0 = d.point0, e0 = d.edge0;
  // uniform: the descriptor is the same for every thread
  const bool in_range = nc >= 0 && np >= 0 && ne >= 0 && c0 >= 0 && p0 >= 0 && e0 >= 0 && c0 + nc <= in.total_cams &&
                        p0 + np <= in.total_points && e0 + ne <= in.total_edges;
  if (!in_range) {
    if (tid == 0) out.status[problem] = -1;
    return;
  }
  const ba::Problem p{d.n_cams,          d.n_points,         d.n_edges,           in.cam_tcw + c0 * 12, in.cam_fixed + c0,
                      in.points + p0 * 3, in.edge_cam + e0,  in.edge_point + e0, in.edge_obs + e0 * 2};
  const ba::Scratch w = ba::piece(scratch, problem, c0, p0, e0);
  const long long s = ba::kSlots;
  const BaOut o{out.status + problem,
                at(out.cam_tcw, c0 * 12),
                at(out.points, p0 * 3),
                at(out.outliers, e0),
                at(out.cam_pose_f64, c0 * 12),
                at(out.points_f64, p0 * 3),
                at(out.round_flags, e0 * 2),
                at(out.round_iterations, (long long)problem * ba::kRounds),
                at(out.it_trials, problem * s),
                at(out.it_lambda_in, problem * s),
                at(out.it_lambda_out, problem * s),
                at(out.it_cost_in, problem * s),
                at(out.it_cost_out, problem * s),
                at(out.it_cam_in, c0 * s * 7),
                at(out.it_point_in, p0 * s * 3),
                at(out.it_cam_out, c0 * s * 7),
                at(out.it_point_out, p0 * s * 3),
                at(out.it_Hcc, c0 * s * 21),
                at(out.it_bc, c0 * s * 6),
                at(out.it_Hpp, p0 * s * 6),
                at(out.it_bp, p0 * s * 3)};
  const Block256 team{tid};
  const int status = ba::bundle_adjust(team, p, prm, in.stop, w, o);
  if (tid == 0) *o.status = status;
}

hipError_t bundle_adjust(int n_problems, const BaBatch& in, const ba::Params& prm, const ba::Scratch& scratch,
                         const BaOut& out, hipStream_t st) {
  if (n_problems <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_bundle_adjust, dim3(n_problems), dim3(kBaThreads), 0, st, in, prm, scratch, out);
  return hipGetLastError();
}

}  // namespace msf
