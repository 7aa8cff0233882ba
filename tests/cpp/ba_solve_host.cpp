// Host build of csrc/ba_solve.h for tests/test_ba_solve_host.py and tools/bench_ba.py: g++ -ffp-contract=off into a
// plain shared object (no HIP, no GPU).  What k_bundle_adjust computes for one problem, on one thread.
#include <cstdlib>
#include <cstring>

#include "ba_solve.h"

using namespace msf::ba;

// K = (fx, fy, cx, cy); schedule = n_rounds, iterations[2], robust[2]; outs: the 21 arrays of Out in its order, any of
// them null but the first.  The scratch is ba::layout() on a block of its own.  -> status, or -2 without memory.
extern "C" int ba_host_adjust(int n_cams, const float* cam_tcw, const uint8_t* cam_fixed, int n_points, const float* points,
                              int n_edges, const int32_t* edge_cam, const int32_t* edge_point, const float* edge_obs,
                              const int32_t* stop, const float* K, const int32_t* schedule, double huber_delta2, double chi2,
                              int max_free, void* const* outs) {
  const Params prm{Cam{(double)K[0], (double)K[1], (double)K[2], (double)K[3]},
                   schedule[0],
                   {schedule[1], schedule[2]},
                   {schedule[3], schedule[4]},
                   huber_delta2,
                   chi2};
  const Out o{(int32_t*)outs[0], (float*)outs[1],   (float*)outs[2],   (uint8_t*)outs[3], (double*)outs[4],  (double*)outs[5],
              (uint8_t*)outs[6], (int32_t*)outs[7], (int32_t*)outs[8], (double*)outs[9],  (double*)outs[10], (double*)outs[11],
              (double*)outs[12], (double*)outs[13], (double*)outs[14], (double*)outs[15], (double*)outs[16], (double*)outs[17],
              (double*)outs[18], (double*)outs[19], (double*)outs[20]};
  if (n_cams < 0 || n_points < 0 || n_edges < 0) return *o.status = -1;
  msf::Carver measure;
  layout(measure, 1, n_cams, n_points, n_edges, max_free);
  uint8_t* block = (uint8_t*)std::calloc(measure.off + 256, 1);
  if (!block) return -2;
  msf::Carver place{block};
  const Scratch w = layout(place, 1, n_cams, n_points, n_edges, max_free);
  const Problem p{n_cams, n_points, n_edges, cam_tcw, cam_fixed, points, edge_cam, edge_point, edge_obs};
  const int status = bundle_adjust(Serial(), p, prm, stop, w, o);
  *o.status = status;
  std::free(block);
  return status;
}
