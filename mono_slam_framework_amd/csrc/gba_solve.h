// Optimizer::GlobalBundleAdjustemnt (slam_pipeline/src/Optimizer.cc:62-69): BundleAdjustment (:71-215) over the whole
// map, as LoopClosing::RunGlobalBundleAdjustment calls it after a loop, for one problem of up to 1024 free cameras.  The
// arithmetic is ba_solve.h's, entry for entry: what is here is how one problem is spread over the whole device instead
// of one workgroup -- the phases as launches over their index (gba_kernels.hip calls the one-index bodies of
// ba_solve.h), the host's Levenberg-Marquardt loop around them, and the dense solve as tiles.
//
// The solve.  ba::cholesky is left-looking: entry (i, j) of L is S_ij - sum_{k < j} L_ik L_jk with k ascending, an
// unfused multiply and subtract each, then / sqrt(pivot_j).  A tiled left-looking factorisation with tile edge kTile
// performs that operation sequence per entry whatever the tile edge is: for tile column (panel) J
//   step 1  every tile (I, J), I >= J, subtracts the products of the columns of panels 0 .. J - 1, k ascending;
//   step 2  the diagonal tile continues k inside the panel and is factored column by column;
//   step 3  every tile below continues k inside the panel against the factored diagonal tile, row by row.
// b_S travels as row n, so the row tiles cover rows 0 .. n.  Steps 1 and 2 are one launch (the workgroup of the diagonal
// tile goes on to factor it), step 3 another; the tiles of a step share nothing and are spread over the grid.  No FMA
// and no MFMA, so the result equals ba::cholesky bit for bit; the functions below are that schedule run serially
// (tests/cpp/gba_solve_host.cpp), and gba_kernels.hip stages the same tiles through LDS.
//
// The back substitution.  ba::back_substitute gives y_i its updates y_i -= L_ji x_j in descending j.  By blocks of
// kTile columns from the last: the block is solved in itself (x_j = y_j / d_j, then the rows of the block above j),
// then every row above the block takes the block's updates, j descending.  The same sequence per y_i.
#ifndef MSF_GBA_SOLVE_H
#define MSF_GBA_SOLVE_H

#include "ba_solve.h"

namespace msf {
namespace gba {

constexpr int kMaxFreeCams = 1024;   // MSF_GBA_MAX_FREE_CAMS: S is at most 6144 x 6145
constexpr int kTile = 64;            // msf_global_ba_tile_rows()

// What the host reads after a launch sequence: the checking kernel's verdict, then an iteration's cost and first
// lambda, then a trial's figures.  The kernels write the device copy; one copy to pinned memory per host wait.
struct Record {
  int32_t malformed;   // the checking kernel: an edge index out of range or edge_point decreasing
  int32_t n_free;      // the checking kernel: the free cameras
  int32_t failed;      // == the trial's number: a point block or a pivot failed in it
  int32_t stop;        // the stop word as the last launch of the sequence read it
  double cost, lambda0;                  // the iteration: sum(rho) at the entry estimate; 1e-5 max|diag|
  double trial_cost, scale_c, scale_p;   // the trial
};

// The scratch of one problem: the record and ba::Scratch for one problem whose max_free is the problem's own count.
struct Scratch {
  Record* rec;
  ba::Scratch w;
};

// The one layout.  n_free = 0 before the count is known: the record and the per-camera, per-point and
// per-edge arrays only.
inline Scratch layout(Carver& c, size_t cams, size_t points, size_t edges, int n_free) {
  Scratch s{};
  s.rec = c.take<Record>(1);
  s.w = ba::layout(c, 1, cams, points, edges, n_free);
  return s;
}

// ba::schur_row dealt out by (row, free camera fj <= the row's own): the row's up to six entries under camera fj, each
// kept in a register from its first value to its last term, and b_S with the row's own block.  An entry receives the
// terms ba::schur_row gives it, in its order: ascending position in the row camera's CSR, ascending edge in a point.
MSF_HD void schur_block(const ba::Problem& p, const ba::Scratch& w, int nf, double lambda, int row, int fj) {
  const int n = 6 * nf;
  const long long ld = n + 1;
  const int fi = row / 6, r = row % 6, ci = w.free_cam[fi];
  if (fj > fi) return;
  const bool own = fj == fi;
  const double* H = w.Hcc + 27 * (long long)fi;
  const bool moves = w.cam_active[ci] > 0;
  const int last = own ? r : 5;
  double v[6] = {0, 0, 0, 0, 0, 0};
  if (own)
    for (int c = 0; c <= last; c++) v[c] = moves ? H[ba::tri(c, r)] + (c == r ? lambda : 0.0) : (c == r ? 1.0 : 0.0);
  double bs = moves ? H[21 + r] : 0.0;
  for (int at = w.cam_start[ci]; at < w.cam_end[ci]; at++) {
    const int e = w.cam_edges[at];
    if (!w.active[e]) continue;
    const int q = p.edge_point[e];
    double y[3];
    ba::sym3_mul(w.inv + 6 * (long long)q, w.W + 18 * (long long)e + 3 * r, y);
    const double* b = w.bp + 3 * (long long)q;
    if (own) bs -= y[0] * b[0] + y[1] * b[1] + y[2] * b[2];
    for (int e2 = w.pt_start[q]; e2 < w.pt_end[q]; e2++) {
      if (!w.active[e2] || w.free_of[p.edge_cam[e2]] != fj) continue;
      const double* W2 = w.W + 18 * (long long)e2;
      for (int c = 0; c <= last; c++) v[c] -= ba::schur_term(y, W2, c);
    }
  }
  for (int c = 0; c <= last; c++) w.S[(6 * fj + c) * ld + row] = v[c];
  if (own) w.S[row * ld + n] = bs;
}

// ---- the tile schedule: panel J is columns [col0(J), col1(n, J)), row tile I is rows [row0(I), row1(n, I)) of 0 .. n
MSF_HD int panels(int n) { return (n + kTile - 1) / kTile; }
MSF_HD int row_tiles(int n) { return n / kTile + 1; }
MSF_HD int col0(int J) { return J * kTile; }
MSF_HD int col1(int n, int J) { return (J + 1) * kTile < n ? (J + 1) * kTile : n; }
MSF_HD int row0(int I) { return I * kTile; }
MSF_HD int row1(int n, int I) { return (I + 1) * kTile < n + 1 ? (I + 1) * kTile : n + 1; }

// s - sum_{k0 <= k < k1} L_ik L_jk, k ascending
MSF_HD double minus_products(const double* S, long long ld, int i, int j, int k0, int k1, double s) {
  for (int k = k0; k < k1; k++) s -= S[k * ld + i] * S[k * ld + j];
  return s;
}

// step 1 on tile (I, J), I >= J
MSF_HD void update_tile(double* S, int n, int I, int J) {
  const long long ld = n + 1;
  const int c0 = col0(J);
  for (int j = c0; j < col1(n, J); j++)
    for (int i = row0(I) > j ? row0(I) : j; i < row1(n, I); i++) S[j * ld + i] = minus_products(S, ld, i, j, 0, c0, S[j * ld + i]);
}

// step 2 on tile (J, J) -> -1, or the column whose pivot is not positive or not finite (nothing of it is written)
MSF_HD int factor_tile(double* S, int n, int J, double* diag) {
  const long long ld = n + 1;
  const int c0 = col0(J), r1 = row1(n, J);
  for (int j = c0; j < col1(n, J); j++) {
    for (int i = j; i < r1; i++) S[j * ld + i] = minus_products(S, ld, i, j, c0, j, S[j * ld + i]);
    const double pivot = S[j * ld + j];
    if (!(pivot > 0 && ba::finite(pivot))) return j;
    const double d = sqrt(pivot);
    diag[j] = d;
    for (int i = j + 1; i < r1; i++) S[j * ld + i] = S[j * ld + i] / d;
  }
  return -1;
}

// step 3 on tile (I, J), I > J
MSF_HD void solve_tile(double* S, int n, int I, int J, const double* diag) {
  const long long ld = n + 1;
  const int c0 = col0(J);
  for (int i = row0(I); i < row1(n, I); i++)
    for (int j = c0; j < col1(n, J); j++) S[j * ld + i] = minus_products(S, ld, i, j, c0, j, S[j * ld + i]) / diag[j];
}

// ba::cholesky by tiles, serially -> -1 or the failing column
inline int cholesky(double* S, int n, double* diag) {
  for (int J = 0; J < panels(n); J++) {
    if (J > 0)
      for (int I = J; I < row_tiles(n); I++) update_tile(S, n, I, J);
    const int fail = factor_tile(S, n, J, diag);
    if (fail >= 0) return fail;
    for (int I = J + 1; I < row_tiles(n); I++) solve_tile(S, n, I, J, diag);
  }
  return -1;
}

// the block [b0, b1) in itself: x_j = y_j / d_j, then the rows of the block above j, j descending
MSF_HD void back_substitute_block(double* S, int n, const double* diag, double* x, int b0, int b1) {
  const long long ld = n + 1;
  for (int j = b1 - 1; j >= b0; j--) {
    const double xj = S[j * ld + n] / diag[j];
    x[j] = xj;
    for (int i = b0; i < j; i++) S[i * ld + n] -= S[i * ld + j] * xj;
  }
}

// row i < b0 takes the updates of the block [b0, b1), j descending
MSF_HD void back_substitute_row(double* S, int n, const double* x, int b0, int b1, int i) {
  const long long ld = n + 1;
  double y = S[i * ld + n];
  for (int j = b1 - 1; j >= b0; j--) y -= S[i * ld + j] * x[j];
  S[i * ld + n] = y;
}

// ba::back_substitute by blocks, serially
inline void back_substitute(double* S, int n, const double* diag, double* x) {
  for (int B = panels(n) - 1; B >= 0; B--) {
    const int b0 = col0(B), b1 = col1(n, B);
    back_substitute_block(S, n, diag, x, b0, b1);
    for (int i = 0; i < b0; i++) back_substitute_row(S, n, x, b0, b1, i);
  }
}

// ---- the host's side of the Levenberg-Marquardt loop.  A Driver runs launch sequences and hands back the record:
//   bool prepare()                                  the CSRs, the estimates, active = 1, the counters at 0
//   bool stop_word(int32_t* stop)                   the stop word now
//   bool reclassify()  bool count_active()
//   bool linearize(int round, int slot, bool first, Record* r)        r->cost, r->lambda0, r->stop
//   bool trial(int round, double lambda, int number, Record* r)       r->failed == number, r->trial_cost, ...
//   void accept()                                   the trial estimates become the estimates
//   bool end_iteration(int slot, int trials, double lambda_in, double lambda_out, double cost_in, double cost_out)
//   bool end_round(int round, int iterations)  bool finish(int rounds_run)
// each false: the launch or the wait failed and the run ends.  Serial drives the same loop over ba_solve.h's bodies
// (tests/cpp/gba_solve_host.cpp); the device's is in gba_kernels.hip.  -> the rounds run, or -2 when the driver failed.
template <class Driver>
int levenberg_marquardt(Driver& d, const ba::Params& prm, int32_t stop_at_entry, const volatile int32_t* host_stop) {
  using ba::finite;
  if (!d.prepare()) return -2;
  int rounds_run = 0, number = 0;
  int32_t stop = stop_at_entry;
  bool stopped = false;
  const auto stop_set = [&]() { return stop != 0 || (host_stop && *host_stop != 0); };
  for (int round = 0; round < prm.n_rounds && !stopped; round++) {
    if (round > 0 && !d.stop_word(&stop)) return -2;
    if (stop_set()) break;
    if (round == 1 && !d.reclassify()) return -2;
    if (!d.count_active()) return -2;
    double lambda = 0.0, ni = 2.0;
    int it = 0;
    while (it < prm.iterations[round]) {
      if (stop_set()) {
        stopped = true;
        break;
      }
      // ba::iteration: the system once at the entry estimate, then trials until one is accepted
      const int slot = round * ba::kMaxIterations + it;
      Record r{};
      if (!d.linearize(round, slot, it == 0, &r)) return -2;
      stop = r.stop;
      const double cost = r.cost;
      if (it == 0) lambda = r.lambda0, ni = 2.0;
      const double lambda_in = lambda;
      double cost_out = cost;
      int trials = 0;
      bool accepted = false;
      while (trials < ba::kTrials && !accepted) {
        trials++;
        double gain = -1.0, trial_cost = ba::kDblMax;
        bool solved = finite(lambda);
        if (solved) {
          number++;
          if (!d.trial(round, lambda, number, &r)) return -2;
          stop = r.stop;
          solved = r.failed != number;
        }
        if (solved) {
          trial_cost = r.trial_cost;
          gain = ba::gain_of(cost, trial_cost, r.scale_c, r.scale_p);
        }
        if (solved && gain > 0 && finite(trial_cost)) {
          ba::next_lambda(true, gain, &lambda, &ni);
          d.accept();
          cost_out = trial_cost;
          accepted = true;
        } else if (ba::next_lambda(false, gain, &lambda, &ni)) {
          break;
        }
      }
      if (!d.end_iteration(slot, trials, lambda_in, lambda, cost, cost_out)) return -2;
      it++;
      if (!accepted) break;
    }
    rounds_run = round + 1;
    if (!d.end_round(round, it)) return -2;
  }
  if (!d.finish(rounds_run)) return -2;
  return rounds_run;
}

}  // namespace gba
}  // namespace msf
#endif  // MSF_GBA_SOLVE_H
