// Optimizer::GlobalBundleAdjustemnt (slam_pipeline/src/Optimizer.cc:62-69) on the device: one bundle adjustment of up
// to 1024 free cameras as a sequence of launches, each spread over the whole device.  The arithmetic is ba_solve.h's
// through gba_solve.h; the host drives the Levenberg-Marquardt loop (gba::levenberg_marquardt) and reads one record per
// trial and one per iteration.
//   k_gba_check            every edge index, the order of edge_point, the free cameras, the stop word
//   k_gba_prepare          the free-camera map, edge counts and entry estimates per camera, edge ranges per point
//   k_gba_collect          the camera-side CSR
//   k_gba_reclassify, k_gba_count_active                                  per round
//   k_gba_linearize, k_gba_system, k_gba_system_out, k_gba_reduce_system  per iteration
//   k_gba_invert, k_gba_schur, k_gba_chol_panel / k_gba_chol_solve per tile column, k_gba_back_substitute, k_gba_step,
//   k_gba_trial_cost, k_gba_reduce_trial                                  per trial
//   k_gba_end_iteration, k_gba_end_round, k_gba_stop_word, k_gba_finish, k_gba_status
// The joins are the kernel boundaries of one stream: no cooperative launch, no workgroup waits for another, nothing
// spins on memory, no floating-point atomics (the one atomic counts free cameras, an integer).  Every output has one
// owner that adds in the order ba_solve.h fixes, so the result is k_bundle_adjust's and the host build's bit for bit
// (sin and cos are pose::sin_cos, not libm's).  A kernel of a trial in
// which a point block or a pivot has already failed finds the trial's number in the record and returns.
//
// The Cholesky (gba_solve.h has the schedule and why it keeps every bit).  k_gba_chol_panel: one workgroup of 256 per
// tile (I, J) of the column; operand tiles of 64 rows x 16 columns of L go through LDS, a thread keeps 4 x 4 entries in
// registers and subtracts the products k ascending, a multiply and a subtract each (-ffp-contract=off, no MFMA); the
// workgroup of the diagonal tile then factors it in LDS, one thread per row.  k_gba_chol_solve: one wave per tile below,
// the factored diagonal tile and the tile's own rows in LDS, a thread per row.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "gba_pipeline.h"
#include "gba_solve.h"

#pragma STDC FP_CONTRACT OFF

namespace msf {

namespace {

constexpr int kThreads = 256;       // the per-index phases
constexpr int kReduceThreads = 1024;   // the one-workgroup phases: ba::tree as it is
constexpr int kT = gba::kTile;
constexpr int kChunk = 16;          // columns of L per LDS stage of k_gba_chol_panel

static_assert(kT == 64, "k_gba_chol_panel deals 4 x 4 entries to 256 threads; k_gba_chol_solve is one wave per tile");

template <int kSize>
struct Block {
  int tid;
  template <class F>
  __device__ void each(int n, F f) const {
    for (int i = tid; i < n; i += kSize) f(i);
    __syncthreads();
  }
  __device__ bool any(bool b) const { return __syncthreads_or(b ? 1 : 0) != 0; }
  __device__ bool leader() const { return tid == 0; }
  __device__ void join() const { __syncthreads(); }
};

__device__ int index() { return blockIdx.x * kThreads + threadIdx.x; }
__device__ int32_t stop_now(const GbaCall& a) { return a.d_stop ? *(const volatile int32_t*)a.d_stop : 0; }
__device__ bool failed(const GbaCall& a, int number) { return a.s.rec->failed == number; }

}  // namespace

// grid: max(n_edges, n_cams, 1) threads.  The record was cleared before.
__global__ __launch_bounds__(kThreads) void k_gba_check(GbaCall a) {
  const int i = index();
  if (i < a.p.n_edges && ba::edge_malformed(a.p, i)) a.s.rec->malformed = 1;
  if (i < a.p.n_cams && a.p.cam_fixed[i] == 0) atomicAdd(&a.s.rec->n_free, 1);
  if (i == 0) a.s.rec->stop = stop_now(a);
}

// grid: max(n_cams, n_points, n_edges, 64) threads
__global__ __launch_bounds__(kThreads) void k_gba_prepare(GbaCall a) {
  const int i = index();
  if (i == 0) ba::map_free_cameras(a.p, a.s.w);
  if (i < a.p.n_cams) ba::count_camera_edges(a.p, a.s.w, i);
  if (i < a.p.n_points) ba::prepare_point(a.p, a.s.w, i);
  if (i < a.p.n_edges) a.s.w.active[i] = 1;
  if (i < ba::kSlots && a.out.it_trials) a.out.it_trials[i] = 0;
  if (i < ba::kRounds && a.out.round_iterations) a.out.round_iterations[i] = 0;
}

// grid: n_cams threads.  A camera's start is the sum of the counts before it (integers: any order gives the leader's
// prefix sum of ba::prepare).
__global__ __launch_bounds__(kThreads) void k_gba_collect(GbaCall a) {
  const int c = index();
  if (c >= a.p.n_cams) return;
  int at = 0;
  for (int k = 0; k < c; k++) at += a.s.w.cam_active[k];
  a.s.w.cam_start[c] = at;
  a.s.w.cam_end[c] = at + a.s.w.cam_active[c];
  ba::collect_camera_edges(a.p, a.s.w, c);
}

__global__ __launch_bounds__(kThreads) void k_gba_reclassify(GbaCall a) {
  const int e = index();
  if (e < a.p.n_edges) ba::reclassify_edge(a.p, a.prm, a.s.w, e);
}

// grid: max(n_cams, n_points) threads
__global__ __launch_bounds__(kThreads) void k_gba_count_active(GbaCall a) {
  const int i = index();
  if (i < a.p.n_cams) ba::count_active_camera(a.s.w, i);
  if (i < a.p.n_points) ba::count_active_point(a.s.w, i);
}

// grid: max(n_edges, n_cams, 3 n_points) threads: the edges, and the entry estimates of the slot
__global__ __launch_bounds__(kThreads) void k_gba_linearize(GbaCall a, int huber, int slot) {
  const int i = index();
  const ba::Scratch& w = a.s.w;
  if (i < a.p.n_edges && w.active[i]) ba::linearize(a.p, a.prm, huber != 0, w, i);
  if (a.out.it_cam_in && i < a.p.n_cams) ba::write_camera(w, a.out.it_cam_in + (long long)slot * a.p.n_cams * 7, i);
  if (a.out.it_point_in && i < a.p.n_points * 3) a.out.it_point_in[(long long)slot * a.p.n_points * 3 + i] = w.pt[i];
}

// grid: max(n_points, 27 n_free) threads
__global__ __launch_bounds__(kThreads) void k_gba_system(GbaCall a, int nf) {
  const int i = index();
  if (i < a.p.n_points) ba::point_system(a.s.w, i);
  if (i < nf * 27) ba::camera_system(a.s.w, i);
}

// grid: max(n_cams, 6 n_points) threads: it_Hcc, it_bc, it_Hpp, it_bp of the slot
__global__ __launch_bounds__(kThreads) void k_gba_system_out(GbaCall a, int slot) {
  const int i = index();
  const long long np = a.p.n_points;
  if ((a.out.it_Hcc || a.out.it_bc) && i < a.p.n_cams) ba::write_camera_system(a.p, a.s.w, a.out, slot, i);
  if (a.out.it_Hpp && i < np * 6) a.out.it_Hpp[slot * np * 6 + i] = a.s.w.Hpp[i];
  if (a.out.it_bp && i < np * 3) a.out.it_bp[slot * np * 3 + i] = a.s.w.bp[i];
}

// one workgroup: the cost, and at a round's first iteration lambda_0; the stop word
__global__ __launch_bounds__(kReduceThreads) void k_gba_reduce_system(GbaCall a, int nf, int first) {
  const Block<kReduceThreads> team{(int)threadIdx.x};
  const ba::Scratch& w = a.s.w;
  const double cost = ba::tree<false>(team, w.redp, a.p.n_points);
  double lambda0 = 0.0;
  if (first) {
    team.each(nf, [&](int f) { ba::camera_top(w, f); });
    const double top_p = ba::tree<true>(team, w.redq, a.p.n_points), top_c = ba::tree<true>(team, w.redc, nf);
    lambda0 = 1e-5 * (top_c > top_p ? top_c : top_p);
  }
  if (team.leader()) {
    a.s.rec->cost = cost;
    a.s.rec->lambda0 = lambda0;
    a.s.rec->stop = stop_now(a);
  }
}

__global__ __launch_bounds__(kThreads) void k_gba_invert(GbaCall a, double lambda, int number) {
  const int q = index();
  if (q < a.p.n_points && !ba::invert_point(a.s.w, lambda, q)) a.s.rec->failed = number;
}

// grid: 6 n_free x n_free threads, the row fastest
__global__ __launch_bounds__(kThreads) void k_gba_schur(GbaCall a, int nf, double lambda, int number) {
  if (failed(a, number)) return;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int n = 6 * nf;
  if (i < (long long)n * nf) gba::schur_block(a.p, a.s.w, nf, lambda, (int)(i % n), (int)(i / n));
}

// Steps 1 and 2 of tile column J.  grid: the row tiles J .. row_tiles(n) - 1; 256 threads; thread (tx, ty) owns rows
// row0 + 4 tx .. + 3 and columns col0 + 4 ty .. + 3 of its tile.
__global__ __launch_bounds__(256) void k_gba_chol_panel(double* __restrict__ S, int n, int J, double* __restrict__ diag,
                                                        gba::Record* rec, int number) {
  if (rec->failed == number) return;
  __shared__ double As[kChunk][kT];   // As[k][r] = L(row0 + r, k0 + k)
  __shared__ double Bs[kChunk][kT];   // Bs[k][r] = L(col0 + r, k0 + k)
  __shared__ double Ts[kT][kT];       // the diagonal tile, Ts[j][i]
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int I = J + blockIdx.x;
  const long long ld = n + 1;
  const int c0 = gba::col0(J), c1 = gba::col1(n, J), r0 = gba::row0(I), r1 = gba::row1(n, I);
  double acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int i = r0 + 4 * tx + a, j = c0 + 4 * ty + b;
      acc[a][b] = i < r1 && j < c1 && i >= j ? S[j * ld + i] : 0.0;
    }
  for (int k0 = 0; k0 < c0; k0 += kChunk) {   // c0 is a multiple of the tile edge, and so of kChunk
#pragma unroll
    for (int m = 0; m < kChunk * kT / 256; m++) {
      const int at = tid + 256 * m, k = at >> 6, r = at & 63;
      As[k][r] = r0 + r < r1 ? S[(k0 + k) * ld + r0 + r] : 0.0;
      Bs[k][r] = c0 + r < c1 ? S[(k0 + k) * ld + c0 + r] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kChunk; k++) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; a++) av[a] = As[k][4 * tx + a], bv[a] = Bs[k][4 * ty + a];
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = acc[a][b] - av[a] * bv[b];
    }
    __syncthreads();
  }
  if (I != J) {
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const int i = r0 + 4 * tx + a, j = c0 + 4 * ty + b;
        if (i < r1 && j < c1) S[j * ld + i] = acc[a][b];
      }
    return;
  }
  // the diagonal tile: k goes on inside the panel, column by column; thread t < rows owns row r0 + t
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) Ts[4 * ty + b][4 * tx + a] = acc[a][b];
  __syncthreads();
  const int cols = c1 - c0, rows = r1 - r0;
  for (int j = 0; j < cols; j++) {
    if (tid >= j && tid < rows) {
      double s = Ts[j][tid];
#pragma unroll 8
      for (int k = 0; k < j; k++) s -= Ts[k][tid] * Ts[k][j];   // unrolled so that the LDS reads run ahead of the chain
      Ts[j][tid] = s;
    }
    __syncthreads();
    const double pivot = Ts[j][j];
    if (!(pivot > 0 && ba::finite(pivot))) {   // uniform: every thread reads the same word
      if (tid == 0) rec->failed = number;
      return;
    }
    const double d = sqrt(pivot);
    if (tid == j) diag[c0 + j] = d;
    else if (tid > j && tid < rows) Ts[j][tid] = Ts[j][tid] / d;
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int i = 4 * tx + a, j = 4 * ty + b;
      if (i < rows && j < cols && i >= j) S[(c0 + j) * ld + r0 + i] = Ts[j][i];
    }
}

// Step 3 of tile column J.  grid: the row tiles J + 1 .. row_tiles(n) - 1 (the column is then a full one); one wave;
// thread t owns row row0 + t.
__global__ __launch_bounds__(kT) void k_gba_chol_solve(double* __restrict__ S, int n, int J, const double* __restrict__ diag,
                                                       const gba::Record* rec, int number) {
  if (rec->failed == number) return;
  __shared__ double Ls[kT][kT];   // Ls[k][j] = L(col0 + j, col0 + k), k < j
  __shared__ double Rs[kT][kT];   // Rs[j][t] = entry (row0 + t, col0 + j)
  const int t = threadIdx.x, I = J + 1 + blockIdx.x;
  const long long ld = n + 1;
  const int c0 = gba::col0(J), cols = gba::col1(n, J) - c0, r0 = gba::row0(I), r1 = gba::row1(n, I);
  const bool mine = r0 + t < r1;
  for (int k = 0; k < cols; k++) {
    Ls[k][t] = t < cols && t > k ? S[(c0 + k) * ld + c0 + t] : 0.0;
    Rs[k][t] = mine ? S[(c0 + k) * ld + r0 + t] : 0.0;
  }
  __syncthreads();
  if (!mine) return;
  for (int j = 0; j < cols; j++) {
    double s = Rs[j][t];
#pragma unroll 8
    for (int k = 0; k < j; k++) s -= Rs[k][t] * Ls[k][j];
    s = s / diag[c0 + j];
    Rs[j][t] = s;
    S[(c0 + j) * ld + r0 + t] = s;
  }
}

// gba::back_substitute in one workgroup: a block of 64 columns is solved by one wave, a lane per row, y in a register
// and x_j passed by a shuffle; then every thread takes a row above the block through the block's updates.
__global__ __launch_bounds__(kReduceThreads) void k_gba_back_substitute(double* __restrict__ S, int n,
                                                                        const double* __restrict__ diag,
                                                                        double* __restrict__ x, const gba::Record* rec,
                                                                        int number) {
  if (rec->failed == number) return;
  __shared__ double Lb[kT][kT + 1];   // Lb[i][j] = L(b0 + j, b0 + i), i < j
  __shared__ double xb[kT];
  const int tid = threadIdx.x;
  const long long ld = n + 1;
  for (int B = gba::panels(n) - 1; B >= 0; B--) {
    const int b0 = gba::col0(B), b1 = gba::col1(n, B), m = b1 - b0;
    for (int at = tid; at < kT * kT; at += kReduceThreads) {
      const int i = at >> 6, j = at & 63;
      if (i < j && j < m) Lb[i][j] = S[(b0 + i) * ld + b0 + j];
    }
    __syncthreads();
    if (tid < kT) {   // exactly the first wave
      double y = tid < m ? S[(b0 + tid) * ld + n] : 0.0;
      for (int j = m - 1; j >= 0; j--) {
        const double xj = __shfl(y, j) / diag[b0 + j];
        if (tid == j) x[b0 + j] = xj, xb[j] = xj;
        else if (tid < j) y -= Lb[tid][j] * xj;
      }
    }
    __syncthreads();
    for (int i = tid; i < b0; i += kReduceThreads) {
      double y = S[i * ld + n];
#pragma unroll 8
      for (int j = m - 1; j >= 0; j--) y -= S[i * ld + b0 + j] * xb[j];
      S[i * ld + n] = y;
    }
    __syncthreads();
  }
}

// grid: max(n_points, n_cams) threads
__global__ __launch_bounds__(kThreads) void k_gba_step(GbaCall a, double lambda, int number) {
  if (failed(a, number)) return;
  const int i = index();
  if (i < a.p.n_points) ba::point_step(a.p, a.s.w, lambda, i);
  if (i < a.p.n_cams) ba::camera_step(a.s.w, lambda, i);
}

__global__ __launch_bounds__(kThreads) void k_gba_trial_cost(GbaCall a, int huber, int number) {
  if (failed(a, number)) return;
  const int q = index();
  if (q < a.p.n_points) ba::point_trial_cost(a.p, a.prm, huber != 0, a.s.w, q);
}

// one workgroup: the trial's cost and the two denominators of the gain; the stop word
__global__ __launch_bounds__(kReduceThreads) void k_gba_reduce_trial(GbaCall a, int nf, int number) {
  const Block<kReduceThreads> team{(int)threadIdx.x};
  const ba::Scratch& w = a.s.w;
  if (team.leader()) a.s.rec->stop = stop_now(a);
  if (failed(a, number)) return;   // uniform: the word was written by an earlier launch
  const double trial_cost = ba::tree<false>(team, w.redp, a.p.n_points);
  const double scale_c = ba::tree<false>(team, w.redc, nf), scale_p = ba::tree<false>(team, w.redq, a.p.n_points);
  if (team.leader()) a.s.rec->trial_cost = trial_cost, a.s.rec->scale_c = scale_c, a.s.rec->scale_p = scale_p;
}

// grid: max(n_cams, 3 n_points, 1) threads: the kept estimates and the figures of the slot
__global__ __launch_bounds__(kThreads) void k_gba_end_iteration(GbaCall a, int slot, int trials, double lambda_in,
                                                                double lambda_out, double cost_in, double cost_out) {
  const int i = index();
  const ba::Out& o = a.out;
  if (o.it_cam_out && i < a.p.n_cams) ba::write_camera(a.s.w, o.it_cam_out + (long long)slot * a.p.n_cams * 7, i);
  if (o.it_point_out && i < a.p.n_points * 3) o.it_point_out[(long long)slot * a.p.n_points * 3 + i] = a.s.w.pt[i];
  if (i == 0) {
    if (o.it_trials) o.it_trials[slot] = trials;
    if (o.it_lambda_in) o.it_lambda_in[slot] = lambda_in;
    if (o.it_lambda_out) o.it_lambda_out[slot] = lambda_out;
    if (o.it_cost_in) o.it_cost_in[slot] = cost_in;
    if (o.it_cost_out) o.it_cost_out[slot] = cost_out;
  }
}

// grid: max(n_edges, 1) threads
__global__ __launch_bounds__(kThreads) void k_gba_end_round(GbaCall a, int round, int iterations) {
  const int e = index();
  if (e == 0 && a.out.round_iterations) a.out.round_iterations[round] = iterations;
  if (round == 0 && a.out.round_flags && e < a.p.n_edges) ba::write_round0_flag(a.p, a.prm, a.s.w, a.out, e);
}

__global__ void k_gba_stop_word(GbaCall a) { a.s.rec->stop = stop_now(a); }

// grid: max(n_edges, n_cams, 3 n_points, 1) threads: :530-540, the estimates and the status
__global__ __launch_bounds__(kThreads) void k_gba_finish(GbaCall a, int rounds_run) {
  const int i = index();
  if ((a.out.outliers || a.out.round_flags) && i < a.p.n_edges) ba::write_final_flag(a.p, a.prm, a.s.w, a.out, rounds_run, i);
  if (i < a.p.n_cams) ba::write_final_camera(a.p, a.s.w, a.out, rounds_run, i);
  if (i < a.p.n_points * 3) ba::write_final_point(a.s.w, a.out, i);
  if (i == 0) *a.out.status = rounds_run;
}

__global__ void k_gba_status(int32_t* status, int32_t value) { *status = value; }

namespace {

int max3(long long a, long long b, long long c) {
  const long long m = a > b ? (a > c ? a : c) : (b > c ? b : c);
  return (int)(m > 1 ? m : 1);
}

// The device's side of gba::levenberg_marquardt.  Every method enqueues on the stream; the ones that hand back a record
// copy it to pinned memory and wait.  `call` changes in one way: accept() swaps the estimates with the trial estimates
// (k_gba_step writes every trial camera and point, so the swap is the copy of ba::iteration).
struct Driver {
  GbaCall call;
  int nf;
  gba::Record* pinned;
  hipStream_t st;
  hipError_t error = hipSuccess;

  template <class... Params, class... Args>
  void launch(void (*kernel)(Params...), long long threads, int block, Args... args) {
    if (error != hipSuccess) return;
    const unsigned grid = (unsigned)((threads + block - 1) / block);
    hipLaunchKernelGGL(kernel, dim3(grid > 0 ? grid : 1), dim3(block), 0, st, args...);
    error = hipGetLastError();
  }
  bool fetch(gba::Record* r) {
    if (error == hipSuccess) error = hipMemcpyAsync(pinned, call.s.rec, sizeof(gba::Record), hipMemcpyDeviceToHost, st);
    if (error == hipSuccess) error = hipStreamSynchronize(st);
    if (error != hipSuccess) return false;
    *r = *pinned;
    return true;
  }
  bool ok() const { return error == hipSuccess; }

  bool prepare() {
    const ba::Problem& p = call.p;
    launch(k_gba_prepare, max3(max3(p.n_cams, p.n_points, p.n_edges), ba::kSlots, 0), kThreads, call);
    if (p.n_cams > 0) launch(k_gba_collect, p.n_cams, kThreads, call);
    return ok();
  }
  bool stop_word(int32_t* stop) {
    launch(k_gba_stop_word, 1, 1, call);
    gba::Record r;
    if (!fetch(&r)) return false;
    *stop = r.stop;
    return true;
  }
  bool reclassify() {
    if (call.p.n_edges > 0) launch(k_gba_reclassify, call.p.n_edges, kThreads, call);
    return ok();
  }
  bool count_active() {
    if (call.p.n_cams > 0 || call.p.n_points > 0) launch(k_gba_count_active, max3(call.p.n_cams, call.p.n_points, 0), kThreads, call);
    return ok();
  }
  bool linearize(int round, int slot, bool first, gba::Record* r) {
    const ba::Problem& p = call.p;
    const ba::Out& o = call.out;
    launch(k_gba_linearize, max3(p.n_edges, p.n_cams, 3LL * p.n_points), kThreads, call, call.prm.robust[round], slot);
    if (p.n_points > 0 || nf > 0) launch(k_gba_system, max3(p.n_points, 27LL * nf, 0), kThreads, call, nf);
    if (o.it_Hcc || o.it_bc || o.it_Hpp || o.it_bp)
      launch(k_gba_system_out, max3(p.n_cams, 6LL * p.n_points, 0), kThreads, call, slot);
    launch(k_gba_reduce_system, kReduceThreads, kReduceThreads, call, nf, first ? 1 : 0);
    return fetch(r);
  }
  bool trial(int round, double lambda, int number, gba::Record* r) {
    const ba::Problem& p = call.p;
    const ba::Scratch& w = call.s.w;
    const int n = 6 * nf;
    if (p.n_points > 0) launch(k_gba_invert, p.n_points, kThreads, call, lambda, number);
    if (nf > 0) {
      launch(k_gba_schur, (long long)n * nf, kThreads, call, nf, lambda, number);
      for (int J = 0; J < gba::panels(n); J++) {
        const int tiles = gba::row_tiles(n) - J;
        launch(k_gba_chol_panel, 256LL * tiles, 256, w.S, n, J, w.diag, call.s.rec, number);
        if (tiles > 1) launch(k_gba_chol_solve, (long long)kT * (tiles - 1), kT, w.S, n, J, w.diag, call.s.rec, number);
      }
      launch(k_gba_back_substitute, kReduceThreads, kReduceThreads, w.S, n, w.diag, w.x, call.s.rec, number);
    }
    if (p.n_points > 0 || p.n_cams > 0) launch(k_gba_step, max3(p.n_points, p.n_cams, 0), kThreads, call, lambda, number);
    if (p.n_points > 0) launch(k_gba_trial_cost, p.n_points, kThreads, call, call.prm.robust[round], number);
    launch(k_gba_reduce_trial, kReduceThreads, kReduceThreads, call, nf, number);
    return fetch(r);
  }
  void accept() {
    ba::Scratch& w = call.s.w;
    ba::Estimate* cam = w.cam;
    w.cam = w.cam_trial, w.cam_trial = cam;
    double* pt = w.pt;
    w.pt = w.pt_trial, w.pt_trial = pt;
  }
  bool end_iteration(int slot, int trials, double lambda_in, double lambda_out, double cost_in, double cost_out) {
    const ba::Out& o = call.out;
    if (o.it_cam_out || o.it_point_out || o.it_trials || o.it_lambda_in || o.it_lambda_out || o.it_cost_in || o.it_cost_out)
      launch(k_gba_end_iteration, max3(call.p.n_cams, 3LL * call.p.n_points, 0), kThreads, call, slot, trials, lambda_in,
             lambda_out, cost_in, cost_out);
    return ok();
  }
  bool end_round(int round, int iterations) {
    if (call.out.round_iterations || (round == 0 && call.out.round_flags))
      launch(k_gba_end_round, max3(call.p.n_edges, 0, 0), kThreads, call, round, iterations);
    return ok();
  }
  bool finish(int rounds_run) {
    launch(k_gba_finish, max3(call.p.n_edges, call.p.n_cams, 3LL * call.p.n_points), kThreads, call, rounds_run);
    if (error == hipSuccess) error = hipStreamSynchronize(st);
    return ok();
  }
};

}  // namespace

hipError_t gba_check(const GbaCall& call, gba::Record* verdict, hipStream_t st) {
  Driver d{call, 0, verdict, st};
  d.error = hipMemsetAsync(call.s.rec, 0, sizeof(gba::Record), st);
  d.launch(k_gba_check, max3(call.p.n_edges, call.p.n_cams, 0), kThreads, call);
  gba::Record r;
  d.fetch(&r);
  return d.error;
}

hipError_t gba_solve(const GbaCall& call, int n_free, int32_t stop_at_entry, gba::Record* pinned,
                     const volatile int32_t* host_stop, hipStream_t st, int* status) {
  Driver d{call, n_free, pinned, st};
  // The record may lie in a block allocated after gba_check (the device entry carves again once the free cameras are
  // counted): no trial number may be found in it before a kernel of that trial has written it.
  d.error = hipMemsetAsync(call.s.rec, 0, sizeof(gba::Record), st);
  *status = gba::levenberg_marquardt(d, call.prm, stop_at_entry, host_stop);
  if (d.error == hipSuccess && *status == -2) return hipErrorUnknown;
  return d.error;
}

hipError_t gba_refuse(const GbaCall& call, hipStream_t st) {
  hipLaunchKernelGGL(k_gba_status, dim3(1), dim3(1), 0, st, call.out.status, -1);
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}

}  // namespace msf
