// Host build of csrc/gba_solve.h for tests/test_gba_solve_host.py, tests/test_gba_gpu.py and tools/bench_gba.py:
// g++ -ffp-contract=off into a plain shared object (no HIP, no GPU).  The tiled Cholesky and back substitution run
// serially next to ba::cholesky / ba::back_substitute, and the phases chained as gba_kernels.hip chains them -- one
// index at a time under gba::levenberg_marquardt -- next to ba::bundle_adjust (tests/cpp/ba_solve_host.cpp).
#include <cstdlib>
#include <cstring>

#include "gba_solve.h"

using namespace msf;

// S: (n + 1) x n column-major with b_S as row n, in place -> -1, or the column whose pivot failed
extern "C" int gba_host_solve_tiled(int n, double* S, double* diag, double* x) {
  const int fail = gba::cholesky(S, n, diag);
  if (fail < 0) gba::back_substitute(S, n, diag, x);
  return fail;
}

// the same through ba::cholesky / ba::back_substitute -> 1: factored
extern "C" int gba_host_solve_reference(int n, double* S, double* diag, double* x) {
  if (!ba::cholesky(ba::Serial(), S, n, diag)) return 0;
  ba::back_substitute(ba::Serial(), S, n, diag, x);
  return 1;
}

extern "C" int gba_host_tile_rows(void) { return gba::kTile; }

namespace {

// gba_kernels.hip's Driver with every launch as a loop over its indices
struct SerialDriver {
  ba::Problem p;
  ba::Params prm;
  ba::Scratch w;
  ba::Out o;
  int nf;
  const int32_t* stop;
  int failed = 0;

  int32_t stop_now() const { return stop ? *(const volatile int32_t*)stop : 0; }
  bool prepare() {
    ba::map_free_cameras(p, w);
    for (int c = 0; c < p.n_cams; c++) ba::count_camera_edges(p, w, c);
    for (int q = 0; q < p.n_points; q++) ba::prepare_point(p, w, q);
    for (int e = 0; e < p.n_edges; e++) w.active[e] = 1;
    for (int k = 0; k < ba::kSlots; k++)
      if (o.it_trials) o.it_trials[k] = 0;
    for (int k = 0; k < ba::kRounds; k++)
      if (o.round_iterations) o.round_iterations[k] = 0;
    for (int c = 0; c < p.n_cams; c++) {   // k_gba_collect
      int at = 0;
      for (int k = 0; k < c; k++) at += w.cam_active[k];
      w.cam_start[c] = at, w.cam_end[c] = at + w.cam_active[c];
      ba::collect_camera_edges(p, w, c);
    }
    return true;
  }
  bool stop_word(int32_t* s) {
    *s = stop_now();
    return true;
  }
  bool reclassify() {
    for (int e = 0; e < p.n_edges; e++) ba::reclassify_edge(p, prm, w, e);
    return true;
  }
  bool count_active() {
    for (int c = 0; c < p.n_cams; c++) ba::count_active_camera(w, c);
    for (int q = 0; q < p.n_points; q++) ba::count_active_point(w, q);
    return true;
  }
  bool linearize(int round, int slot, bool first, gba::Record* r) {
    const bool huber = prm.robust[round] != 0;
    const long long nc = p.n_cams, np = p.n_points;
    for (int e = 0; e < p.n_edges; e++)
      if (w.active[e]) ba::linearize(p, prm, huber, w, e);
    for (int c = 0; c < p.n_cams; c++)
      if (o.it_cam_in) ba::write_camera(w, o.it_cam_in + slot * nc * 7, c);
    for (int k = 0; k < np * 3; k++)
      if (o.it_point_in) o.it_point_in[slot * np * 3 + k] = w.pt[k];
    for (int q = 0; q < p.n_points; q++) ba::point_system(w, q);
    for (int i = 0; i < nf * 27; i++) ba::camera_system(w, i);
    for (int c = 0; c < p.n_cams; c++)
      if (o.it_Hcc || o.it_bc) ba::write_camera_system(p, w, o, slot, c);
    for (int k = 0; k < np * 6; k++)
      if (o.it_Hpp) o.it_Hpp[slot * np * 6 + k] = w.Hpp[k];
    for (int k = 0; k < np * 3; k++)
      if (o.it_bp) o.it_bp[slot * np * 3 + k] = w.bp[k];
    const ba::Serial team;
    r->cost = ba::tree<false>(team, w.redp, p.n_points);
    r->lambda0 = 0.0;
    if (first) {
      for (int f = 0; f < nf; f++) ba::camera_top(w, f);
      const double top_p = ba::tree<true>(team, w.redq, p.n_points), top_c = ba::tree<true>(team, w.redc, nf);
      r->lambda0 = 1e-5 * (top_c > top_p ? top_c : top_p);
    }
    r->stop = stop_now();
    r->failed = failed;
    return true;
  }
  bool trial(int round, double lambda, int number, gba::Record* r) {
    const bool huber = prm.robust[round] != 0;
    const int n = 6 * nf;
    for (int q = 0; q < p.n_points; q++)
      if (!ba::invert_point(w, lambda, q)) failed = number;
    if (failed != number && nf > 0) {
      for (int fj = 0; fj < nf; fj++)
        for (int row = 0; row < n; row++) gba::schur_block(p, w, nf, lambda, row, fj);
      if (gba::cholesky(w.S, n, w.diag) >= 0) failed = number;
      else gba::back_substitute(w.S, n, w.diag, w.x);
    }
    if (failed != number) {
      for (int q = 0; q < p.n_points; q++) ba::point_step(p, w, lambda, q);
      for (int c = 0; c < p.n_cams; c++) ba::camera_step(w, lambda, c);
      for (int q = 0; q < p.n_points; q++) ba::point_trial_cost(p, prm, huber, w, q);
      const ba::Serial team;
      r->trial_cost = ba::tree<false>(team, w.redp, p.n_points);
      r->scale_c = ba::tree<false>(team, w.redc, nf);
      r->scale_p = ba::tree<false>(team, w.redq, p.n_points);
    }
    r->stop = stop_now();
    r->failed = failed;
    return true;
  }
  void accept() {
    ba::Estimate* cam = w.cam;
    w.cam = w.cam_trial, w.cam_trial = cam;
    double* pt = w.pt;
    w.pt = w.pt_trial, w.pt_trial = pt;
  }
  bool end_iteration(int slot, int trials, double lambda_in, double lambda_out, double cost_in, double cost_out) {
    const long long nc = p.n_cams, np = p.n_points;
    for (int c = 0; c < p.n_cams; c++)
      if (o.it_cam_out) ba::write_camera(w, o.it_cam_out + slot * nc * 7, c);
    for (int k = 0; k < np * 3; k++)
      if (o.it_point_out) o.it_point_out[slot * np * 3 + k] = w.pt[k];
    if (o.it_trials) o.it_trials[slot] = trials;
    if (o.it_lambda_in) o.it_lambda_in[slot] = lambda_in;
    if (o.it_lambda_out) o.it_lambda_out[slot] = lambda_out;
    if (o.it_cost_in) o.it_cost_in[slot] = cost_in;
    if (o.it_cost_out) o.it_cost_out[slot] = cost_out;
    return true;
  }
  bool end_round(int round, int iterations) {
    if (o.round_iterations) o.round_iterations[round] = iterations;
    if (round == 0 && o.round_flags)
      for (int e = 0; e < p.n_edges; e++) ba::write_round0_flag(p, prm, w, o, e);
    return true;
  }
  bool finish(int rounds_run) {
    if (o.outliers || o.round_flags)
      for (int e = 0; e < p.n_edges; e++) ba::write_final_flag(p, prm, w, o, rounds_run, e);
    for (int c = 0; c < p.n_cams; c++) ba::write_final_camera(p, w, o, rounds_run, c);
    for (int k = 0; k < p.n_points * 3; k++) ba::write_final_point(w, o, k);
    return true;
  }
};

}  // namespace

// Arguments as ba_host_adjust without max_free: the scratch is gba::layout() for the problem's own free cameras.
// -> status, or -2 without memory.
extern "C" int gba_host_adjust(int n_cams, const float* cam_tcw, const uint8_t* cam_fixed, int n_points, const float* points,
                               int n_edges, const int32_t* edge_cam, const int32_t* edge_point, const float* edge_obs,
                               const int32_t* stop, const float* K, const int32_t* schedule, double huber_delta2, double chi2,
                               void* const* outs) {
  const ba::Params prm{ba::Cam{(double)K[0], (double)K[1], (double)K[2], (double)K[3]},
                       schedule[0],
                       {schedule[1], schedule[2]},
                       {schedule[3], schedule[4]},
                       huber_delta2,
                       chi2};
  const ba::Out o{(int32_t*)outs[0], (float*)outs[1],   (float*)outs[2],   (uint8_t*)outs[3], (double*)outs[4],  (double*)outs[5],
                  (uint8_t*)outs[6], (int32_t*)outs[7], (int32_t*)outs[8], (double*)outs[9],  (double*)outs[10], (double*)outs[11],
                  (double*)outs[12], (double*)outs[13], (double*)outs[14], (double*)outs[15], (double*)outs[16], (double*)outs[17],
                  (double*)outs[18], (double*)outs[19], (double*)outs[20]};
  if (n_cams < 0 || n_points < 0 || n_edges < 0) return *o.status = -1;
  const ba::Problem p{n_cams, n_points, n_edges, cam_tcw, cam_fixed, points, edge_cam, edge_point, edge_obs};
  // k_gba_check
  int n_free = 0;
  for (int e = 0; e < n_edges; e++)
    if (ba::edge_malformed(p, e)) return *o.status = -1;
  for (int c = 0; c < n_cams; c++) n_free += cam_fixed[c] == 0;
  if (n_free > gba::kMaxFreeCams) return *o.status = -1;
  Carver measure;
  gba::layout(measure, n_cams, n_points, n_edges, n_free);
  uint8_t* block = (uint8_t*)std::calloc(measure.off + 256, 1);
  if (!block) return -2;
  Carver place{block};
  const gba::Scratch s = gba::layout(place, n_cams, n_points, n_edges, n_free);
  SerialDriver d{p, prm, s.w, o, n_free, stop};
  const int status = gba::levenberg_marquardt(d, prm, d.stop_now(), nullptr);
  *o.status = status;
  std::free(block);
  return status;
}
