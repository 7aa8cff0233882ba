// extern "C" boundary of libmsf.so, the initializer: msf_check_hypotheses, msf_find_models*, msf_reconstruct*
// (declarations: include/msf_abi.h and include/msf_initializer.h; what the files of the boundary share: abi_core.h).
#include "abi_core.h"

#include <cmath>

#include "msf_initializer.h"
#include "ransac_solve.h"
#include "reconstruct_pipeline.h"

namespace msf {
hipError_t check_hypotheses(int model, int n_hyp, const float* d_m21, const float* d_m12, int n,
                            const msf_match* d_matches, float sigma, float* d_scores, uint8_t* d_inliers,
                            hipStream_t st);
hipError_t find_models(int n_lists, const msf_match* d_matches, int cap, const int32_t* d_n_out, int n_single, int n_hyp,
                       const int32_t* d_sets, float sigma, float4* d_pn, float* d_T, float* const* d_m21,
                       float* const* d_aux, float* const* d_null, float* const* d_scores, int32_t* const* d_best,
                       uint8_t* const* d_inliers, hipStream_t st);
hipError_t ransac_sets(int n_lists, int n_hyp, const int32_t* d_n_out, int cap, uint64_t seed, int32_t* d_sets,
                       hipStream_t st);
}

using namespace msf::abi;

namespace {

msf::MotionOut to_out(const msf_motion_result& r) {   // n_inliers is no result: the entry point adds its piece
  return msf::MotionOut{r.model, nullptr, r.n_cand, r.cand_R, r.cand_t, r.cand_good, r.cand_parallax, r.winner, r.ok,
                        r.R21, r.t21, r.points, r.triangulated};
}

}  // namespace

extern "C" {

namespace {

// The device arrays of one msf_check_hypotheses call, all pieces of the workspace: m21 / m12 [hc][9], scores [hc],
// inliers [hc * mc] (the call indexes it with its own n_matches), matches [mc].
struct HypothesesPlan {
  float* m21 = nullptr, *m12 = nullptr, *scores = nullptr;
  uint8_t* inliers = nullptr;
  msf_match* matches = nullptr;
};

}  // namespace

int msf_check_hypotheses(msf_handle* h, int32_t model, int32_t n_hyp, const float* m21, const float* m12,
                         int32_t n_matches, const msf_match* matches, float sigma, float* scores, int32_t* best,
                         uint8_t* best_inliers) {
  return guarded(h, "msf_check_hypotheses", [&]() -> int {
    const bool homography = model == MSF_MODEL_HOMOGRAPHY;
    if ((!homography && model != MSF_MODEL_FUNDAMENTAL) || n_hyp < 0 || n_matches < 0 || n_matches > 8192 ||
        (n_hyp > 0 && (!m21 || !scores || (homography && !m12))) || (n_matches > 0 && !matches) || !best ||
        (n_matches > 0 && !best_inliers))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_check_hypotheses: bad argument (models 0/1, at most 8192 matches)");
    *best = -1;
    for (int i = 0; i < n_matches; i++) best_inliers[i] = 0;   // FindHomography: vbMatchesInliers(N, false) (Initializer.cc:167)
    if (n_hyp == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    // sized for at least 256 hypotheses and 2048 matches: no allocation in the steady state
    const size_t hc = n_hyp > 256 ? n_hyp : 256, mc = n_matches > 2048 ? n_matches : 2048;
    HypothesesPlan p;
    if (int rc = carve(h, h->d_hyp, 0, "hipMalloc", [&](msf::Carver& c) {
          p.m21 = c.take<float>(hc * 9);
          p.m12 = c.take<float>(hc * 9);
          p.scores = c.take<float>(hc);
          p.inliers = c.take<uint8_t>(hc * mc);
          p.matches = c.take<msf_match>(mc);
        }))
      return rc;
    hipStream_t st = cs.st;
    const size_t mat_bytes = (size_t)n_hyp * 9 * sizeof(float);
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.m21, m21, mat_bytes, hipMemcpyHostToDevice, st));
    if (homography) HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.m12, m12, mat_bytes, hipMemcpyHostToDevice, st));
    if (n_matches)
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.matches, matches, (size_t)n_matches * sizeof(msf_match), hipMemcpyHostToDevice, st));
    HIP_TRY(h, "check_hypotheses", msf::check_hypotheses(model, n_hyp, p.m21, p.m12, n_matches, p.matches, sigma, p.scores, p.inliers, st));
    if (int rc = fetch(h, st, scores, p.scores, (size_t)n_hyp * sizeof(float))) return rc;
    if (int rc = cs.finish()) return rc;
    // FindHomography / FindFundamental keep the first hypothesis whose score beats every earlier one (:190-194, :236-240)
    float score = 0.0f;
    for (int i = 0; i < n_hyp; i++)
      if (scores[i] > score) { score = scores[i]; *best = i; }
    if (*best >= 0 && n_matches)
      HIP_TRY(h, "hipMemcpy", hipMemcpy(best_inliers, p.inliers + (size_t)*best * n_matches, (size_t)n_matches, hipMemcpyDeviceToHost));
    return MSF_OK;
  });
}

namespace {

// The device arrays of one find-models call: the caller's where it gave one, else a piece of the handle's workspace.
struct FindModelsPlan {
  float4* pn = nullptr;
  float* T = nullptr;
  int32_t* sets = nullptr;
  msf_match* matches = nullptr;   // single-list call only
  float* m21[2] = {}, *aux[2] = {}, *null_vec[2] = {}, *scores[2] = {};
  int32_t* best[2] = {};
  uint8_t* inliers[2] = {};
};

// user: the device pointers the caller supplied.  host_call: the host entry point -- `user` is empty, and the match list
// and every output get a piece of the workspace.  Returns MSF_OK or an error.
int plan_find_models(msf_handle* h, int n_lists, int cap, int n_hyp, bool host_call, const msf_ransac_batch* user,
                     FindModelsPlan* p) {
  const size_t L = (size_t)n_lists, LH = L * (size_t)n_hyp;
  const msf_ransac_result* res[2] = {&user->homography, &user->fundamental};
  return carve(h, h->d_fm, (size_t)1 << 20, "hipMalloc(find-models workspace)", [&](msf::Carver& c) {
    p->pn = c.take<float4>(L * cap);
    p->T = c.take<float>(L * 18);
    p->sets = c.take(user->sets, LH * 8);
    p->matches = host_call ? c.take<msf_match>(cap) : nullptr;
    for (int m = 0; m < 2; m++) {
      p->m21[m] = c.take(res[m]->m21, LH * 9);
      p->aux[m] = c.take(m == 0 ? res[m]->m12 : res[m]->fn, LH * 9);
      p->null_vec[m] = host_call ? c.take<float>(LH * 9) : res[m]->null_vec;
      p->scores[m] = c.take(res[m]->scores, LH ? LH : 1);
      p->best[m] = host_call ? c.take<int32_t>(1) : res[m]->best;
      p->inliers[m] = host_call ? c.take<uint8_t>(cap) : res[m]->best_inliers;
    }
  });
}

bool ransac_result_ok(const msf_ransac_result* r) {
  return r && r->struct_size == sizeof(msf_ransac_result) && r->best;
}

}  // namespace

int msf_find_models(msf_handle* h, int32_t n_matches, const msf_match* matches, int32_t n_hyp, const int32_t* sets,
                    float sigma, msf_ransac_result* homography, msf_ransac_result* fundamental) {
  return guarded(h, "msf_find_models", [&]() -> int {
    if (!ransac_result_ok(homography) || !ransac_result_ok(fundamental) || n_hyp < 0 || n_hyp > (1 << 20) ||
        n_matches < 0 || n_matches > 8192 || (n_matches > 0 && !matches) ||
        (n_hyp > 0 && (n_matches < 8 || !sets || !homography->scores || !fundamental->scores)))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_find_models: bad argument (8 to 8192 matches, sets, best and scores "
                                          "required, struct_size = sizeof(msf_ransac_result))");
    for (long long i = 0; i < 8ll * n_hyp; i++)
      if (sets[i] < 0 || sets[i] >= n_matches)
        return fail(h, MSF_ERR_INVALID_ARG, "msf_find_models: a set holds an index outside [0, n_matches)");
    msf_ransac_result* res[2] = {homography, fundamental};
    for (int m = 0; m < 2; m++) {
      *res[m]->best = -1;
      if (res[m]->best_inliers)
        for (int i = 0; i < n_matches; i++) res[m]->best_inliers[i] = 0;
    }
    if (n_hyp == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    // device side: every array is a piece of the workspace
    msf_ransac_batch dev{};
    FindModelsPlan p;
    if (int rc = plan_find_models(h, 1, n_matches, n_hyp, true, &dev, &p)) return rc;
    hipStream_t st = cs.st;
    Drain drain{st};
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.matches, matches, (size_t)n_matches * sizeof(msf_match), hipMemcpyHostToDevice, st));
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.sets, sets, (size_t)n_hyp * 8 * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(h, "find_models", msf::find_models(1, p.matches, n_matches, nullptr, n_matches, n_hyp, p.sets, sigma, p.pn, p.T, p.m21,
                                               p.aux, p.null_vec, p.scores, p.best, p.inliers, st));
    const size_t mat_bytes = (size_t)n_hyp * 9 * sizeof(float);
    for (int m = 0; m < 2; m++) {
      if (int rc = fetch(h, st, res[m]->m21, p.m21[m], mat_bytes)) return rc;
      if (int rc = fetch(h, st, m == 0 ? res[m]->m12 : res[m]->fn, p.aux[m], mat_bytes)) return rc;
      if (int rc = fetch(h, st, res[m]->null_vec, p.null_vec[m], mat_bytes)) return rc;
      if (int rc = fetch(h, st, res[m]->scores, p.scores[m], (size_t)n_hyp * sizeof(float))) return rc;
      if (int rc = fetch(h, st, res[m]->best, p.best[m], sizeof(int32_t))) return rc;
      if (int rc = fetch(h, st, res[m]->best_inliers, p.inliers[m], (size_t)n_matches)) return rc;
      if (int rc = fetch(h, st, res[m]->T1, p.T, 9 * sizeof(float))) return rc;
      if (int rc = fetch(h, st, res[m]->T2, p.T + 9, 9 * sizeof(float))) return rc;
    }
    drain.armed = false;
    return cs.finish();   // the one wait of the call
  });
}

int msf_find_models_device(msf_handle* h, int32_t n_lists, const msf_match* d_matches, int32_t cap_per_pair,
                           const int32_t* d_n_out, int32_t n_hyp, uint64_t seed, float sigma, msf_ransac_batch* out,
                           void* stream) {
  return guarded(h, "msf_find_models_device", [&]() -> int {
    if (!out || out->struct_size != sizeof(msf_ransac_batch) || !ransac_result_ok(&out->homography) ||
        !ransac_result_ok(&out->fundamental) || n_lists < 0 || n_lists > 65535 || n_hyp < 0 || n_hyp > (1 << 20) ||
        cap_per_pair < 1 || (n_lists > 0 && (!d_matches || !d_n_out)))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_find_models_device: bad argument (at most 65535 lists, best required, "
                                          "struct_size = sizeof(msf_ransac_batch))");
    if (n_lists == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    FindModelsPlan p;
    if (int rc = plan_find_models(h, n_lists, cap_per_pair, n_hyp, false, out, &p)) return rc;
    hipStream_t st = cs.st;
    HIP_TRY(h, "ransac_sets", msf::ransac_sets(n_lists, n_hyp, d_n_out, cap_per_pair, seed, p.sets, st));
    HIP_TRY(h, "find_models", msf::find_models(n_lists, d_matches, cap_per_pair, d_n_out, 0, n_hyp, p.sets, sigma, p.pn, p.T, p.m21,
                                               p.aux, p.null_vec, p.scores, p.best, p.inliers, st));
    const msf_ransac_result* res[2] = {&out->homography, &out->fundamental};
    for (int m = 0; m < 2; m++) {   // T lives as [n_lists][2][9] in the workspace; the caller's T1 / T2 are [n_lists][9] each
      if (res[m]->T1) HIP_TRY(h, "hipMemcpy2DAsync", hipMemcpy2DAsync(res[m]->T1, 36, p.T, 72, 36, n_lists, hipMemcpyDeviceToDevice, st));
      if (res[m]->T2) HIP_TRY(h, "hipMemcpy2DAsync", hipMemcpy2DAsync(res[m]->T2, 36, p.T + 9, 72, 36, n_lists, hipMemcpyDeviceToDevice, st));
    }
    return cs.finish();
  });
}

// ---- msf_initializer.h: the tail of Initializer::Initialize ----
namespace {

// What a reconstruct call keeps in the workspace besides its result arrays (result_arrays.h: kMotionArrays).
struct ReconstructPlan {
  int32_t* n_inliers = nullptr;   // MotionOut::n_inliers [n_lists]: handed from launch to launch, no result
  msf_match* matches = nullptr;   // host call only: the list, its inlier flags and its matrix
  uint8_t* inliers = nullptr;
  float* m21 = nullptr;
};

// nullptr when the parameters are usable, else what is wrong with them
const char* motion_params_fault(const msf_motion_params* prm) {
  if (!prm) return "params is NULL";
  if (prm->struct_size != sizeof(msf_motion_params)) return "params->struct_size is not sizeof(msf_motion_params)";
  bool finite = std::isfinite(prm->sigma) && std::isfinite(prm->min_parallax);
  for (int k = 0; k < 9; k++) finite = finite && std::isfinite(prm->K[k]);
  if (!finite) return "K, sigma and min_parallax must be finite";
  float inv[9];
  msf::ransac::inv3(prm->K, inv);
  bool zero = true;
  for (int k = 0; k < 9; k++) zero = zero && inv[k] == 0.0f;
  if (zero) return "K is singular";
  return nullptr;
}

msf::MotionParams motion_params(const msf_motion_params* prm) {
  msf::MotionParams d{};
  for (int k = 0; k < 9; k++) d.K[k] = prm->K[k];
  d.th2 = 4.0f * (prm->sigma * prm->sigma);   // 4.0f * mSigma2
  d.min_triangulated = prm->min_triangulated;
  d.min_parallax = prm->min_parallax;
  return d;
}

}  // namespace

int msf_initializer_version(void) { return MSF_INITIALIZER_VERSION; }

int msf_reconstruct(msf_handle* h, int32_t model, const float* m21, int32_t n_matches, const msf_match* matches,
                    const uint8_t* inliers, const msf_motion_params* params, msf_motion_result* out) {
  return guarded(h, "msf_reconstruct", [&]() -> int {
    if (!out || out->struct_size != sizeof(msf_motion_result))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct: out is NULL or out->struct_size is not sizeof(msf_motion_result)");
    if (!out->ok || !m21 || (n_matches > 0 && (!matches || !inliers)))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct: a required pointer is NULL (m21, matches, inliers, out->ok)");
    if (n_matches < 0 || n_matches > msf::kMaxReconstructMatches)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct: n_matches outside [0, 8192]");
    if (model != MSF_MODEL_HOMOGRAPHY && model != MSF_MODEL_FUNDAMENTAL)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct: model is neither MSF_MODEL_HOMOGRAPHY nor MSF_MODEL_FUNDAMENTAL");
    if (const char* fault = motion_params_fault(params))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_reconstruct: ") + fault);
    CallScope cs{h};
    if (int rc = cs.enter()) return rc;
    const int cap = n_matches > 0 ? n_matches : 1;
    const size_t units[] = {1};
    msf_motion_result dev{};
    ReconstructPlan p;
    if (int rc = carve(h, h->d_rc, (size_t)1 << 16, "hipMalloc(reconstruct workspace)", [&](msf::Carver& c) {
          msf::carve_result(c, msf::kMotionArrays, units, (size_t)cap, nullptr, *out, &dev);
          p.n_inliers = c.take<int32_t>(1);
          p.matches = c.take<msf_match>(cap);
          p.inliers = c.take<uint8_t>(cap);
          p.m21 = c.take<float>(9);
        }))
      return rc;
    msf::MotionOut o = to_out(dev);
    o.n_inliers = p.n_inliers;
    hipStream_t st = cs.st;
    Drain drain{st};
    if (n_matches > 0) {
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.matches, matches, (size_t)n_matches * sizeof(msf_match), hipMemcpyHostToDevice, st));
      HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.inliers, inliers, (size_t)n_matches, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(h, "hipMemcpyAsync", hipMemcpyAsync(p.m21, m21, 9 * sizeof(float), hipMemcpyHostToDevice, st));
    msf::MotionLists in{};
    in.matches = p.matches;
    in.cap = cap;
    in.n_single = n_matches;
    in.n_hyp = 1;
    in.forced_model = model;
    in.m21[model] = p.m21;
    in.inliers[model] = p.inliers;
    HIP_TRY(h, "reconstruct_motion", msf::reconstruct_motion(1, in, motion_params(params), o, st));
    const msf::Extent all{0, (size_t)cap, (size_t)cap, (size_t)n_matches, units, units};
    if (int rc = fetch_result(h, st, msf::kMotionArrays, dev, *out, all)) return rc;
    drain.armed = false;
    return cs.finish();   // the one wait of the call
  });
}

int msf_reconstruct_device(msf_handle* h, int32_t n_lists, const msf_match* d_matches, int32_t cap_per_pair,
                           const int32_t* d_n_out, int32_t n_hyp, const msf_ransac_batch* found,
                           const msf_motion_params* params, msf_motion_result* out, void* stream) {
  return guarded(h, "msf_reconstruct_device", [&]() -> int {
    if (!out || out->struct_size != sizeof(msf_motion_result))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: out is NULL or out->struct_size is not sizeof(msf_motion_result)");
    if (!found || found->struct_size != sizeof(msf_ransac_batch))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: found is NULL or found->struct_size is not sizeof(msf_ransac_batch)");
    const msf_ransac_result* res[2] = {&found->homography, &found->fundamental};
    bool complete = out->ok && (n_lists <= 0 || (d_matches && d_n_out));
    for (int m = 0; m < 2; m++)
      complete = complete && res[m]->m21 && res[m]->scores && res[m]->best && res[m]->best_inliers;
    if (!complete)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: a required pointer is NULL (d_matches, d_n_out, out->ok; "
                                          "m21, scores, best and best_inliers of both models of found)");
    if (n_lists < 0 || n_lists > 65535)
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: n_lists outside [0, 65535]");
    if (cap_per_pair < 1 || n_hyp < 1 || n_hyp > (1 << 20))
      return fail(h, MSF_ERR_INVALID_ARG, "msf_reconstruct_device: cap_per_pair < 1 or n_hyp outside [1, 2^20]");
    if (const char* fault = motion_params_fault(params))
      return fail(h, MSF_ERR_INVALID_ARG, std::string("msf_reconstruct_device: ") + fault);
    if (n_lists == 0) return MSF_OK;
    CallScope cs{h};
    if (int rc = cs.enter(stream)) return rc;
    const size_t units[] = {(size_t)n_lists};
    msf_motion_result dev{};
    ReconstructPlan p;
    if (int rc = carve(h, h->d_rc, (size_t)1 << 16, "hipMalloc(reconstruct workspace)", [&](msf::Carver& c) {
          msf::carve_result(c, msf::kMotionArrays, units, (size_t)cap_per_pair, out, *out, &dev);
          p.n_inliers = c.take<int32_t>(n_lists);
        }))
      return rc;
    msf::MotionOut o = to_out(dev);
    o.n_inliers = p.n_inliers;
    msf::MotionLists in{};
    in.matches = d_matches;
    in.cap = cap_per_pair;
    in.n_out = d_n_out;
    in.n_hyp = n_hyp;
    in.forced_model = -1;
    for (int m = 0; m < 2; m++) {
      in.m21[m] = res[m]->m21;
      in.scores[m] = res[m]->scores;
      in.best[m] = res[m]->best;
      in.inliers[m] = res[m]->best_inliers;
    }
    HIP_TRY(h, "reconstruct_motion", msf::reconstruct_motion(n_lists, in, motion_params(params), o, cs.st));
    return cs.finish();
  });
}

}  // extern "C"
