// Host build of csrc/pnp_solve.h for tests/test_pnp_solve_host.py and tools/bench_pnp.py: g++ -ffp-contract=off into a
// plain shared object (no HIP, no GPU).  What the two kernels of pnp_kernels.hip compute, list by list, on one thread.
#include <cstring>

#include "pnp_solve.h"

using namespace msf::pnp;

// outs: the twenty-two arrays of HostOut in its order, any of them null.  K = (fx, fy, cx, cy).
// -> the true number of records, -1 for n < 4
extern "C" int pnp_host_ransac(int n, const float* p3d, const float* p2d, const float* K, float th2, int min_inliers,
                               int n_iterations, int max_records, uint64_t seed, int list, const int32_t* sets, int cap,
                               void* const* outs) {
  static_assert(sizeof(HostOut) == 22 * sizeof(void*), "HostOut is twenty-two pointers");
  HostOut o;
  std::memcpy(&o, outs, sizeof o);
  const Cam cam{(double)K[0], (double)K[1], (double)K[2], (double)K[3]};
  return ransac_host(n, p3d, p2d, cam, th2, min_inliers, n_iterations, max_records, seed, list, sets, cap, o);
}

// SetPoints / draw_set4 alone, for the test of the draw
extern "C" void pnp_host_draw(uint64_t seed, int list, int it, int n, int32_t* set) { draw_set4(seed, list, it, n, set); }

// eig12_host alone: rows 8..11 of Ut of a symmetric 12 x 12 matrix
extern "C" void pnp_host_eig12(const double* mtm, double* ut_tail) { eig12_host(mtm, ut_tail); }
