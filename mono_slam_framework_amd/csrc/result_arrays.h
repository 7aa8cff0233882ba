// The arrays of the geometry calls' result structs (msf_pnp_result, msf_pose_result, msf_motion_result,
// msf_new_points_result) as one table each, and the two functions that read it: carve_result() gives the arrays of a
// call their pieces of the workspace, copy_result() moves the arrays of one list back to the caller.  A shape is written
// down here once; mono_slam_framework_amd/_lib.py holds the same table for numpy and tests/test_result_arrays_host.py
// compares the two.  No HIP in here: any C++17 compiler takes it (tests/cpp/result_arrays_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "carve.h"
#include "msf_initializer.h"
#include "msf_local_mapping.h"
#include "msf_pnp.h"
#include "msf_pose.h"

namespace msf {

// One array of a result struct: [lists][units[unit]] rows of `tail` elements, or of cap * tail elements when per_cap
// (a row that runs along the list, cap being the lists' stride).  Unit 0 is the list itself: one row per list.
struct ResultArray {
  const char* name;
  size_t offset;   // of the pointer member in the public struct
  size_t elem;     // bytes per element
  int unit;        // index into the call's unit counts
  size_t tail;     // elements per row (per entry of the list when per_cap)
  bool per_cap;
  bool required;   // the kernel needs the array whether the caller wants it or not
};

// offset and element size come from the member itself
#define MSF_RESULT_ROW(S, member, unit, tail, per_cap, required) \
  ::msf::ResultArray { #member, offsetof(S, member), sizeof(*S{}.member), unit, tail, per_cap, required }

// A result struct is struct_size, reserved and then nothing but pointers: one row per pointer, in declaration order.
template <class S, size_t N>
constexpr bool covers(const ResultArray (&table)[N]) {
  if (N != (sizeof(S) - 8) / sizeof(void*)) return false;
  for (size_t i = 0; i < N; i++)
    if (table[i].offset != 8 + i * sizeof(void*)) return false;
  return true;
}

// unit counts of a PnP call: {n_lists, n_iterations, max_records}
enum { kPerList = 0, kPerHyp = 1, kPerRec = 2 };
constexpr ResultArray kPnpArrays[] = {
    MSF_RESULT_ROW(msf_pnp_result, n_records, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_pnp_result, counts, kPerHyp, 1, false, true),
    MSF_RESULT_ROW(msf_pnp_result, iteration, kPerRec, 1, false, false),
    MSF_RESULT_ROW(msf_pnp_result, n_inliers, kPerRec, 1, false, false),
    MSF_RESULT_ROW(msf_pnp_result, refined_ok, kPerRec, 1, false, false),
    MSF_RESULT_ROW(msf_pnp_result, n_refined, kPerRec, 1, false, false),
    MSF_RESULT_ROW(msf_pnp_result, Tcw_best, kPerRec, 12, false, false),
    MSF_RESULT_ROW(msf_pnp_result, Tcw_refined, kPerRec, 12, false, false),
    MSF_RESULT_ROW(msf_pnp_result, inliers_best, kPerRec, 1, true, false),
    MSF_RESULT_ROW(msf_pnp_result, inliers_refined, kPerRec, 1, true, false),
    MSF_RESULT_ROW(msf_pnp_result, sets, kPerHyp, 4, false, false),
    MSF_RESULT_ROW(msf_pnp_result, pose_f64, kPerHyp, 12, false, true),
    MSF_RESULT_ROW(msf_pnp_result, cws, kPerHyp, 12, false, false),
    MSF_RESULT_ROW(msf_pnp_result, ut_tail, kPerHyp, 48, false, false),
    MSF_RESULT_ROW(msf_pnp_result, betas, kPerHyp, 12, false, false),
    MSF_RESULT_ROW(msf_pnp_result, rep_errors, kPerHyp, 3, false, false),
    MSF_RESULT_ROW(msf_pnp_result, pca, kPerHyp, 9, false, false),
    MSF_RESULT_ROW(msf_pnp_result, rec_pose_f64, kPerRec, 12, false, false),
    MSF_RESULT_ROW(msf_pnp_result, rec_cws, kPerRec, 12, false, false),
    MSF_RESULT_ROW(msf_pnp_result, rec_ut_tail, kPerRec, 48, false, false),
    MSF_RESULT_ROW(msf_pnp_result, rec_betas, kPerRec, 12, false, false),
    MSF_RESULT_ROW(msf_pnp_result, rec_rep_errors, kPerRec, 3, false, false),
    MSF_RESULT_ROW(msf_pnp_result, rec_pca, kPerRec, 9, false, false),
};
static_assert(covers<msf_pnp_result>(kPnpArrays), "one row per pointer of msf_pnp_result, in its order");

// unit counts of a pose call: {n_lists, 4 rounds, 4 x 10 iterations}
enum { kPerRound = 1, kPerIt = 2 };
constexpr size_t kPoseRounds = 4, kPoseIterations = 40;
constexpr ResultArray kPoseArrays[] = {
    MSF_RESULT_ROW(msf_pose_result, n_good, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_pose_result, Tcw, kPerList, 12, false, false),
    MSF_RESULT_ROW(msf_pose_result, outliers, kPerList, 1, true, false),
    MSF_RESULT_ROW(msf_pose_result, n_edges, kPerList, 1, false, false),
    MSF_RESULT_ROW(msf_pose_result, rounds_run, kPerList, 1, false, false),
    MSF_RESULT_ROW(msf_pose_result, pose_f64, kPerList, 12, false, false),
    MSF_RESULT_ROW(msf_pose_result, round_pose_f64, kPerRound, 12, false, false),
    MSF_RESULT_ROW(msf_pose_result, round_n_bad, kPerRound, 1, false, false),
    MSF_RESULT_ROW(msf_pose_result, round_iterations, kPerRound, 1, false, false),
    MSF_RESULT_ROW(msf_pose_result, it_trials, kPerIt, 1, false, false),
    MSF_RESULT_ROW(msf_pose_result, it_lambda_in, kPerIt, 1, false, false),
    MSF_RESULT_ROW(msf_pose_result, it_lambda_out, kPerIt, 1, false, false),
    MSF_RESULT_ROW(msf_pose_result, it_cost_in, kPerIt, 1, false, false),
    MSF_RESULT_ROW(msf_pose_result, it_cost_out, kPerIt, 1, false, false),
    MSF_RESULT_ROW(msf_pose_result, it_H, kPerIt, 21, false, false),
    MSF_RESULT_ROW(msf_pose_result, it_b, kPerIt, 6, false, false),
    MSF_RESULT_ROW(msf_pose_result, it_pose_out, kPerIt, 7, false, false),
};
static_assert(covers<msf_pose_result>(kPoseArrays), "one row per pointer of msf_pose_result, in its order");

// unit counts of a reconstruct call: {n_lists}.  The three launches hand the candidates on through these arrays.
constexpr ResultArray kMotionArrays[] = {
    MSF_RESULT_ROW(msf_motion_result, ok, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_motion_result, model, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_motion_result, R21, kPerList, 9, false, false),
    MSF_RESULT_ROW(msf_motion_result, t21, kPerList, 3, false, false),
    MSF_RESULT_ROW(msf_motion_result, points, kPerList, 3, true, false),
    MSF_RESULT_ROW(msf_motion_result, triangulated, kPerList, 1, true, false),
    MSF_RESULT_ROW(msf_motion_result, n_cand, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_motion_result, cand_R, kPerList, 72, false, true),
    MSF_RESULT_ROW(msf_motion_result, cand_t, kPerList, 24, false, true),
    MSF_RESULT_ROW(msf_motion_result, cand_good, kPerList, 8, false, true),
    MSF_RESULT_ROW(msf_motion_result, cand_parallax, kPerList, 8, false, true),
    MSF_RESULT_ROW(msf_motion_result, winner, kPerList, 1, false, true),
};
static_assert(covers<msf_motion_result>(kMotionArrays), "one row per pointer of msf_motion_result, in its order");

// unit counts of a new-points call: {n_lists}
constexpr ResultArray kNewPointsArrays[] = {
    MSF_RESULT_ROW(msf_new_points_result, n_new, kPerList, 1, false, true),
    MSF_RESULT_ROW(msf_new_points_result, packed, kPerList, 1, true, false),
    MSF_RESULT_ROW(msf_new_points_result, status, kPerList, 1, true, false),
    MSF_RESULT_ROW(msf_new_points_result, points, kPerList, 3, true, false),
    MSF_RESULT_ROW(msf_new_points_result, hom, kPerList, 4, true, false),
    MSF_RESULT_ROW(msf_new_points_result, cos_parallax, kPerList, 1, true, false),
};
static_assert(covers<msf_new_points_result>(kNewPointsArrays), "one row per pointer of msf_new_points_result, in its order");

// keeps a parameter out of template deduction: carve_result(..., nullptr, wanted, &dev) takes S from the other two
template <class T>
struct same_as {
  using type = T;
};

// The pointer of array `a` in a result struct, read and written as bytes: the members have different pointer types.
template <class S>
uint8_t* slot(const S& s, const ResultArray& a) {
  uint8_t* p;
  std::memcpy(&p, reinterpret_cast<const uint8_t*>(&s) + a.offset, sizeof p);
  return p;
}

template <class S>
void set_slot(S* s, const ResultArray& a, uint8_t* p) {
  std::memcpy(reinterpret_cast<uint8_t*>(s) + a.offset, &p, sizeof p);
}

// rows of unit `unit` in one list: units[0] counts the lists themselves
inline size_t rows_per_list(const size_t* units, int unit) { return unit == kPerList ? 1 : units[unit]; }

// bytes of one row on a side whose lists have the stride `cap`
inline size_t row_bytes(const ResultArray& a, size_t cap) { return a.tail * a.elem * (a.per_cap ? cap : 1); }

// bytes of array `a` for the whole call
inline size_t array_bytes(const ResultArray& a, const size_t* units, size_t cap) {
  return units[kPerList] * rows_per_list(units, a.unit) * row_bytes(a, cap);
}

// Fills `dev` with the device pointers of one call; units[0] = n_lists, units[k] = rows of unit k per list.
// Host call (given == nullptr): an array gets a piece iff it is required or `wanted` has a pointer for it.
// Device call: the caller's pointer where there is one, else a piece iff required, else null.
template <class S, size_t N>
void carve_result(Carver& c, const ResultArray (&table)[N], const size_t* units, size_t cap,
                  const typename same_as<S>::type* given, const S& wanted, S* dev) {
  static_assert(N == (sizeof(S) - 8) / sizeof(void*), "the table of another struct");
  for (const ResultArray& a : table) {
    uint8_t* p = given ? slot(*given, a) : nullptr;
    if (!p && (a.required || (!given && slot(wanted, a)))) p = c.take<uint8_t>(array_bytes(a, units, cap));
    set_slot(dev, a, p);
  }
}

// What copy_result moves of one list: rows[k] rows of unit k (rows[0] = 1) out of units[k] per list, and of every
// per-cap row its first n entries; the device lists have the stride dcap, the caller's hcap.
struct Extent {
  size_t list;
  size_t dcap, hcap;
  size_t n;
  const size_t* units;
  const size_t* rows;
};

// Every array that `out` has a pointer for, from `dev`: copy(dst, src, bytes) -> 0 or a status that ends the call.
// Rows that are full on both sides (n == dcap == hcap), and rows that do not run along the list, go as one copy.
template <class S, size_t N, class Copier>
int copy_result(const ResultArray (&table)[N], const S& dev, const S& out, const Extent& e, Copier&& copy) {
  static_assert(N == (sizeof(S) - 8) / sizeof(void*), "the table of another struct");
  for (const ResultArray& a : table) {
    uint8_t* dst = slot(out, a);
    const uint8_t* src = slot(dev, a);
    if (!dst || !src) continue;
    const size_t first = e.list * rows_per_list(e.units, a.unit), rows = e.rows[a.unit];
    const size_t drow = row_bytes(a, e.dcap), hrow = row_bytes(a, e.hcap), w = row_bytes(a, e.n);
    dst += first * hrow;
    src += first * drow;
    if (!rows || !w) continue;
    if (w == drow && w == hrow) {
      if (int rc = copy(dst, src, rows * w)) return rc;
      continue;
    }
    for (size_t r = 0; r < rows; r++)
      if (int rc = copy(dst + r * hrow, src + r * drow, w)) return rc;
  }
  return 0;
}

}  // namespace msf
