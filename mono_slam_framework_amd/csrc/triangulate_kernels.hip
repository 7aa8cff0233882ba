// The loop body of LocalMapping::CreateNewMapPoints (slam_pipeline/src/LocalMapping.cc:195-265) on the device, for one
// match list or a batch of them, directly behind the matcher:
//   k_new_points   per match: ray parallax, the 4 x 4 linear triangulation, two depth signs, two reprojection errors;
//                  per list: the accepted matches appended to a packed array in match order, and their count
// One launch.  The arithmetic is triangulate_solve.h, shared with a host build that is checked against float64 without a
// GPU.  Every loop is bounded (ransac::kMaxSweeps Jacobi sweeps, ceil(n / 256) chunks); no workgroup waits on another.
//
// Order independence: every per-match value is a function of that match and the list's two views alone, and a record's
// place in the packed array is the number of accepted matches in front of it (ballot + prefix inside a wave, one LDS
// word per wave across the waves, a running offset across the chunks) -- neither depends on which lane handled which
// match, so a list gives the same bits alone or in any batch.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "triangulate_pipeline.h"
#include "triangulate_solve.h"

namespace msf {

namespace tr = triangulate;

static_assert(sizeof(tr::View) == sizeof(msf_view) && sizeof(msf_view) == 64, "msf_view layout");
static_assert(sizeof(tr::Match) == sizeof(msf_match), "msf_match layout");
static_assert(sizeof(msf_new_point) == 16, "msf_new_point layout");

// One 256-thread workgroup per list; grid: n_lists.  The workgroup walks its list in chunks of 256 matches: lane `tid`
// takes match chunk * 256 + tid; its 4 x 4 [A; V] of the triangulation stays in registers (reconstruct::triangulate
// unrolls completely: no LDS tile, no scratch).  Per chunk the accepted flags are counted by ballot: a lane's record goes
// to offset + (accepted in earlier waves) + (accepted in lower lanes of its wave), so the packed array is in match order.
// Code object (gfx950): 149 vector registers (3 waves per SIMD), 16 B of static LDS, 0 B of scratch; the list's two views
// are uniform and sit in scalar registers.
__global__ __launch_bounds__(256) void k_new_points(NewPointLists in, NewPointParams prm, NewPointOut out) {
  __shared__ int wave_count[4];
  const int list = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int given = in.n_out ? in.n_out[list] : in.n_single;
  if (given < 0) {   // uniform: the matcher's "no valid result"
    if (tid == 0) out.n_new[list] = -1;
    return;
  }
  int n = given < in.cap ? given : in.cap;
  n = n < in.limit ? n : in.limit;
  const long long row = (long long)list * in.cap;
  const msf_match* m = in.matches + row;
  const tr::View v1 = *reinterpret_cast<const tr::View*>(in.view1 + list);
  const tr::View v2 = *reinterpret_cast<const tr::View*>(in.view2 + list);
  int offset = 0;
  const int chunks = (n + 255) / 256;
  for (int chunk = 0; chunk < chunks; chunk++) {
    const int i = chunk * 256 + tid;
    bool accepted = false;
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (i < n) {
      const msf_match mm = m[i];
      const tr::Match q{mm.x1, mm.y1, mm.x2, mm.y2};
      float hom[4];
      double cosp = 0.0;
      const int status = tr::new_point(q, v1, v2, prm.max_cos, prm.chi2, p, hom, &cosp);
      accepted = status == tr::kNewPoint;
      if (out.status) out.status[row + i] = (uint8_t)status;
      if (out.points)
        for (int k = 0; k < 3; k++) out.points[(row + i) * 3 + k] = p[k];
      if (out.hom)
        for (int k = 0; k < 4; k++) out.hom[(row + i) * 4 + k] = hom[k];
      if (out.cos_parallax) out.cos_parallax[row + i] = cosp;
    }
    const unsigned long long ballot = __ballot(accepted);
    if (lane == 0) wave_count[wave] = __popcll(ballot);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < 4; w++) {
      const int c = wave_count[w];
      before += w < wave ? c : 0;
      total += c;
    }
    if (accepted && out.packed) {
      const int at = offset + before + __popcll(ballot & ((1ull << lane) - 1ull));   // < n <= cap
      out.packed[row + at] = msf_new_point{i, p[0], p[1], p[2]};
    }
    offset += total;
    __syncthreads();   // wave_count is rewritten by the next chunk
  }
  if (tid == 0) out.n_new[list] = offset;
}

hipError_t new_points(int n_lists, const NewPointLists& in, const NewPointParams& prm, const NewPointOut& out,
                      hipStream_t st) {
  if (n_lists <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_new_points, dim3(n_lists), dim3(256), 0, st, in, prm, out);
  return hipGetLastError();
}

}  // namespace msf
