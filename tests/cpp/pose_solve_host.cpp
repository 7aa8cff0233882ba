// Host build of csrc/pose_solve.h for tests/test_pose_solve_host.py and tools/bench_pose.py: g++ -ffp-contract=off into
// a plain shared object (no HIP, no GPU).  What k_pose_optimize computes for one list, on one thread.
#include <cstring>

#include "pose_solve.h"

using namespace msf::pose;

// outs: n_edges, rounds_run, Tcw, pose_f64, outliers, then the eleven arrays of Trace in its order, any of them null.
// K = (fx, fy, cx, cy).  emu64: the sums in the device's order (64 strided partial sums and the butterfly), else in
// index order.  -> n_good
extern "C" int pose_host_optimize(int n, const float* p3d, const float* p2d, const uint8_t* mask, const float* K,
                                  float chi2, const float* tcw0, int emu64, void* const* outs) {
  HostOut o{};
  o.n_edges = (int32_t*)outs[0], o.rounds_run = (int32_t*)outs[1], o.Tcw = (float*)outs[2];
  o.pose_f64 = (double*)outs[3], o.outliers = (uint8_t*)outs[4];
  o.trace = Trace{(double*)outs[5],  (int32_t*)outs[6], (int32_t*)outs[7], (int32_t*)outs[8],
                  (double*)outs[9],  (double*)outs[10], (double*)outs[11], (double*)outs[12],
                  (double*)outs[13], (double*)outs[14], (double*)outs[15], true};
  const Cam cam{(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
  if (emu64) return optimize_host(msf::pnp::Emu64(), n, p3d, p2d, mask, cam, chi2, tcw0, o);
  return optimize_host(msf::pnp::Serial(), n, p3d, p2d, mask, cam, chi2, tcw0, o);
}

// se3_exp alone: dx (omega, upsilon) -> R row-major 3 x 3 and t
extern "C" void pose_host_exp(const double* dx, double* r, double* t) { se3_exp(dx, r, t); }

// moved alone: est (quaternion x y z w, t) -> exp(dx) * est
extern "C" void pose_host_moved(const double* est, const double* dx, double* out) {
  Estimate e;
  std::memcpy(e.q, est, 32), std::memcpy(e.t, est + 4, 24);
  const Estimate m = moved(e, dx);
  std::memcpy(out, m.q, 32), std::memcpy(out + 4, m.t, 24);
}
