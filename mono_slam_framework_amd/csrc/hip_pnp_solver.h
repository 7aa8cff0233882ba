// hip_pnp_solver.h -- C++ host mirror of SLAM_PIPELINE::PnPsolver (slam_pipeline/include/PnPsolver.h,
// slam_pipeline/src/PnPsolver.cc:69-331) above the C ABI: the surface Tracking::Relocalization (Tracking.cc:738-864)
// uses -- the constructor, SetRansacParameters, iterate, find -- with every EPnP solve, inlier count and Refine done by
// msf_pnp_ransac / msf_pnp_ransac_device (include/msf_pnp.h).
//
// The reference solves one hypothesis per loop turn on the CPU.  Here a solver keeps a cache of what the stateless
// device call returned for iterations [0, cached): the inlier count of every iteration and the records (the iterations
// at which mvbBestInliers is replaced) with their refined poses; iterate() replays :172-257 over that cache, the
// count of iterations done and the best state included.  The loop runs while fewer than mRansacMaxIts iterations have
// been done in total or fewer than nIterations in this call, as the reference's does, so the first call runs to
// mRansacMaxIts.  When a call needs iterations beyond the
// cache, the stateless call is issued again with a larger n_iterations: the sets are drawn here from (seed, key,
// iteration), so the earlier iterations come out as they were.  Relocalization round-robins over the candidates'
// solvers: PnPsolver::Prefetch fills all their caches with ONE msf_pnp_ransac_device call.
//
// Header-only and OpenCV-free, like hip_initializer.h: a 3-D point is three floats, a 2-D point two, Tcw a row-major
// float[16], "no pose" (the reference's empty cv::Mat) a false return.  The gather of the 3-D points (:80-112:
// GetMapPoint2(i), isBad(), GetWorldPos()) stays with the caller, who passes what the reference's constructor builds:
// mvP3Dw, mvP2D, mvKeyPointIndices and the number of matches.  See INTEGRATION.md.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "hip_device_block.h"
#include "hip_mirror_types.h"
#include "msf_pnp.h"
#include "pnp_solve.h"   // draw_set4: the minimum sets are drawn here and handed to the call

namespace msf {

class PnPsolver {
 public:
  // What PnPsolver::PnPsolver(matchResult) leaves in mvP3Dw, mvP2D, mvKeyPointIndices; nMatches =
  // matchResult.keyPoints2.size(); the intrinsics of the current frame.  `seed` and `key` name this solver's draws.
  PnPsolver(msf_handle* handle, const std::vector<Point3f>& vP3Dw, const std::vector<Point2f>& vP2D,
            const std::vector<size_t>& vKeyPointIndices, size_t nMatches, float fx, float fy, float cx, float cy,
            uint64_t seed = 0, int32_t key = 0)
      : h_(handle), p3d_(vP3Dw), p2d_(vP2D), idx_(vKeyPointIndices), n_matches_(nMatches), fx_(fx), fy_(fy), cx_(cx),
        cy_(cy), seed_(seed), key_(key) {
    SetRansacParameters();
  }

  // The adjustment of the reference's SetRansacParameters, in its types: the floor is the larger of minInliers, minSet
  // and epsilon N truncated (a float product); epsilon is raised to floor / N (a float quotient); the iteration count is
  // 1 when every correspondence has to be an inlier, else ceil(log(1 - probability) / log(1 - epsilon^3)) in double
  // with epsilon promoted -- the cube, not the fourth power, although minSet is 4 -- clamped to [1, maxIterations].
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                           float epsilon = 0.4f, float th2 = 5.991f) {
    n_ = static_cast<int>(p2d_.size());
    floor_ = std::max(std::max(static_cast<int>(n_ * epsilon), minInliers), minSet);
    const float share = static_cast<float>(floor_) / n_;
    const float eps = epsilon < share ? share : epsilon;
    int wanted = 1;
    if (floor_ != n_) {
      const double miss = 1 - std::pow(static_cast<double>(eps), 3);
      wanted = static_cast<int>(std::ceil(std::log(1 - probability) / std::log(miss)));
    }
    max_its_ = std::max(1, std::min(wanted, maxIterations));
    th2_ = th2;
    cached_ = 0;   // the floor and the threshold are part of what the cache holds
  }

  bool find(std::vector<bool>& vbInliers, int& nInliers, float Tcw[16]) {
    bool ignored;
    return iterate(max_its_, ignored, vbInliers, nInliers, Tcw);
  }

  // The reference's iterate over the cache.  It keeps going while fewer than max_its_ iterations have been done in
  // total OR fewer than nIterations in this call (so the first call runs to max_its_).  An iteration below the floor
  // changes nothing; one at or above it first replaces the best record if its count is strictly larger, then asks
  // whether the CURRENT best record's refine succeeded (more refined inliers than the floor, strictly): if so that is
  // the return.  When the loop ends, bNoMore is set and the best record, if there is one, is returned unrefined.
  // true: Tcw holds a pose; false: the reference's empty matrix.
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float Tcw[16]) {
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (n_ < floor_) {
      bNoMore = true;
      return false;
    }
    for (int here = 0; done_ < max_its_ || here < nIterations; here++) {
      const int it = done_++;
      if (it >= cached_ && !Fill(std::max(std::max(2 * cached_, it + 1), max_its_))) {
        bNoMore = true;   // the device call failed: msf_last_error(handle) has the text
        return false;
      }
      const int count = counts_[it];
      if (count < floor_) continue;
      if (count > best_count_) {
        best_count_ = count;
        best_ = RecordOf(it);
      }
      const Record& r = records_[best_];
      if (r.n_refined > floor_) return Report(r.n_refined, r.inliers_refined, r.Tcw_refined, vbInliers, nInliers, Tcw);
    }
    bNoMore = done_ >= max_its_;
    if (!bNoMore || best_count_ < floor_) return false;
    const Record& r = records_[best_];
    return Report(best_count_, r.inliers_best, r.Tcw_best, vbInliers, nInliers, Tcw);
  }

  // Fills the caches of all the solvers (the candidates of one Relocalization) for iterations [0, their largest
  // max_its_) with one msf_pnp_ransac_device call on a block allocated here.  The calling thread's current HIP
  // device must be the handle's.  false: a failed call, or solvers that do not share handle, intrinsics and th2 (nothing is
  // filled then; each solver still fills its own cache when iterate needs it).
  static bool Prefetch(const std::vector<PnPsolver*>& solvers) {
    if (solvers.empty()) return true;
    msf_handle* h = solvers[0]->h_;
    for (const PnPsolver* s : solvers) {   // one call has one handle, one camera and one threshold
      const PnPsolver* f = solvers[0];
      if (!s || s->h_ != h || s->fx_ != f->fx_ || s->fy_ != f->fy_ || s->cx_ != f->cx_ || s->cy_ != f->cy_ ||
          !(s->th2_ == f->th2_))
        return false;
    }
    const size_t L = solvers.size();
    int its = 1, floor = 0x7fffffff;
    size_t cap = 1;
    for (const PnPsolver* s : solvers) {
      its = std::max(its, s->max_its_);
      floor = std::min(floor, s->floor_);
      cap = std::max(cap, s->p3d_.size());
    }
    const int max_records = kMaxRecords;
    const size_t recs = L * max_records;
    // one block: the lists, their lengths and minimum sets, then the outputs the cache keeps
    struct View {
      float *p3d, *p2d;
      int32_t *n, *sets;
      size_t inputs_end;
      msf_pnp_result out;
    };
    DeviceBlock mem;
    View dev, host;
    const auto layout = [&](Carver& c) {
      View v;
      v.p3d = c.take<float>(L * cap * 3);
      v.p2d = c.take<float>(L * cap * 2);
      v.n = c.take<int32_t>(L);
      v.sets = c.take<int32_t>(L * its * 4);
      v.inputs_end = c.off;
      v.out = sized<msf_pnp_result>();
      v.out.n_records = c.take<int32_t>(L);
      v.out.counts = c.take<int32_t>(L * its);
      v.out.iteration = c.take<int32_t>(recs);
      v.out.n_inliers = c.take<int32_t>(recs);
      v.out.n_refined = c.take<int32_t>(recs);
      v.out.Tcw_best = c.take<float>(recs * 12);
      v.out.Tcw_refined = c.take<float>(recs * 12);
      v.out.inliers_best = c.take<uint8_t>(recs * cap);
      v.out.inliers_refined = c.take<uint8_t>(recs * cap);
      return v;
    };
    if (!mem.place(layout, &dev, &host)) return false;
    for (size_t l = 0; l < L; l++) {
      const PnPsolver* s = solvers[l];
      const int32_t n = host.n[l] = static_cast<int32_t>(s->p3d_.size());
      if (n) std::memcpy(host.p3d + l * cap * 3, s->p3d_.data(), n * sizeof(Point3f));
      if (n) std::memcpy(host.p2d + l * cap * 2, s->p2d_.data(), n * sizeof(Point2f));
      if (n >= 4)
        for (int it = 0; it < its; it++) pnp::draw_set4(s->seed_, s->key_, it, n, host.sets + (l * its + it) * 4);
    }
    msf_pnp_params prm = solvers[0]->Params(its, max_records);
    prm.min_inliers = floor;
    if (!mem.upload() ||
        msf_pnp_ransac_device(h, static_cast<int32_t>(L), dev.p3d, dev.p2d, static_cast<int32_t>(cap), dev.n, &prm,
                              dev.sets, &dev.out, nullptr) != MSF_OK ||
        !mem.download())
      return false;
    const msf_pnp_result& got = host.out;
    for (size_t l = 0; l < L; l++) {
      PnPsolver* s = solvers[l];
      if (got.n_records[l] < 0 || got.n_records[l] > max_records) continue;   // no list, or too many records: the solver asks itself
      s->counts_.assign(got.counts + l * its, got.counts + (l + 1) * its);
      s->sets_.assign(host.sets + l * its * 4, host.sets + (l + 1) * its * 4);
      s->records_.clear();
      for (int r = 0; r < got.n_records[l]; r++) {
        const size_t at = l * max_records + r;
        if (got.n_inliers[at] >= s->floor_) s->records_.push_back(s->RecordAt(got, at, cap));   // else: of the call's lower floor only
      }
      s->cached_ = its;
    }
    return true;
  }

  int minInliers() const { return floor_; }
  int maxIterations() const { return max_its_; }
  int iterations() const { return done_; }
  int cached() const { return cached_; }
  const std::vector<int32_t>& sets() const { return sets_; }       // [cached][4]
  const std::vector<int32_t>& counts() const { return counts_; }   // [cached]

 private:
  static constexpr int kMaxRecords = 16;

  struct Record {
    int32_t iteration, n_inliers, n_refined;
    float Tcw_best[12], Tcw_refined[12];
    std::vector<uint8_t> inliers_best, inliers_refined;
  };

  msf_pnp_params Params(int its, int max_records) const {
    msf_pnp_params prm = sized<msf_pnp_params>();
    prm.fx = fx_, prm.fy = fy_, prm.cx = cx_, prm.cy = cy_;
    prm.th2 = th2_;
    prm.min_inliers = floor_;
    prm.n_iterations = its;
    prm.max_records = max_records;
    prm.seed = seed_;
    return prm;
  }

  // the stateless call for iterations [0, its) of this solver alone
  bool Fill(int its) {
    if (!h_ || n_ < 4 || its >= (1 << 20)) return false;
    std::vector<int32_t> sets(static_cast<size_t>(its) * 4);
    for (int it = 0; it < its; it++) pnp::draw_set4(seed_, key_, it, n_, &sets[it * 4]);
    for (int max_records = kMaxRecords;; max_records *= 2) {
      std::vector<int32_t> counts(its), iteration(max_records), n_inliers(max_records), n_refined(max_records);
      std::vector<float> tb(max_records * 12), tr(max_records * 12);
      std::vector<uint8_t> ib(static_cast<size_t>(max_records) * n_), ir(static_cast<size_t>(max_records) * n_);
      int32_t n_records = 0;
      const msf_pnp_params prm = Params(its, max_records);
      msf_pnp_result out = sized<msf_pnp_result>();
      out.n_records = &n_records, out.counts = counts.data(), out.iteration = iteration.data();
      out.n_inliers = n_inliers.data(), out.n_refined = n_refined.data(), out.Tcw_best = tb.data();
      out.Tcw_refined = tr.data(), out.inliers_best = ib.data(), out.inliers_refined = ir.data();
      const int rc = msf_pnp_ransac(h_, n_, &p3d_[0].x, &p2d_[0].x, &prm, sets.data(), &out);
      if (rc == MSF_ERR_CAPACITY && max_records < (1 << 16)) continue;
      if (rc != MSF_OK) return false;
      records_.clear();
      for (int r = 0; r < n_records; r++) records_.push_back(RecordAt(out, r, n_));
      counts_.swap(counts);
      sets_.swap(sets);
      cached_ = its;
      return true;
    }
  }

  // record `at` of a result in host memory whose inlier rows have the stride `stride`
  Record RecordAt(const msf_pnp_result& res, size_t at, size_t stride) const {
    Record rec{res.iteration[at], res.n_inliers[at], res.n_refined[at], {}, {}, {}, {}};
    std::memcpy(rec.Tcw_best, res.Tcw_best + at * 12, 48);
    std::memcpy(rec.Tcw_refined, res.Tcw_refined + at * 12, 48);
    rec.inliers_best.assign(res.inliers_best + at * stride, res.inliers_best + at * stride + n_);
    rec.inliers_refined.assign(res.inliers_refined + at * stride, res.inliers_refined + at * stride + n_);
    return rec;
  }

  size_t RecordOf(int it) const {
    for (size_t r = 0; r < records_.size(); r++)
      if (records_[r].iteration == it) return r;
    return 0;   // not reached: every iteration that raises the best count is a record
  }

  // the inlier flags scattered through mvKeyPointIndices over all matches, and rows 0..2 of Tcw completed to 4 x 4
  bool Report(int count, const std::vector<uint8_t>& flags, const float* rt, std::vector<bool>& vbInliers, int& nInliers,
              float Tcw[16]) const {
    nInliers = count;
    vbInliers.assign(n_matches_, false);
    for (int i = 0; i < n_; i++)
      if (flags[i]) vbInliers[idx_[i]] = true;
    std::memcpy(Tcw, rt, 48);
    Tcw[12] = Tcw[13] = Tcw[14] = 0.0f;
    Tcw[15] = 1.0f;
    return true;
  }

  msf_handle* h_;
  std::vector<Point3f> p3d_;
  std::vector<Point2f> p2d_;
  std::vector<size_t> idx_;
  size_t n_matches_;
  float fx_, fy_, cx_, cy_, th2_ = 5.991f;
  uint64_t seed_;
  int32_t key_;
  // what SetRansacParameters works out, and how far iterate has come
  int n_ = 0, floor_ = 8, max_its_ = 300;
  int done_ = 0, best_count_ = 0;
  // the cache
  int cached_ = 0;
  size_t best_ = 0;
  std::vector<int32_t> counts_, sets_;
  std::vector<Record> records_;
};

}  // namespace msf
