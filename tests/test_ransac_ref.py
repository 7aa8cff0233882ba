"""CPU: the inputs and the reference of tests/test_ransac_gpu.py on their own (tests/ransac_ref.py), so that no GPU test
can pass by leaving cases out: the conditioning of every DLT matrix of every scene and seed, the float64 reference reaching
the planted model, the end-to-end margin being what the CPU shows, the ctypes mirrors of the result structs, and the new
ABI symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import initializer as oracle_init
from tests import ransac_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, s) for k in rr.SCENES for s in rr.SEEDS]


@pytest.mark.parametrize("kind,seed", CASES)
def test_scene_shape_and_conditioning(kind, seed):
    m, bad = rr.scene(kind, seed)
    assert m.shape == (rr.N_MATCHES, 4) and m.dtype == np.int32
    assert 0.2 < bad.mean() < 0.4                                         # 30 % outliers
    assert np.abs(m).max() < 2 * rr.W                                     # integer pixels around a 640 x 480 frame
    sets = rr.draw_sets(len(m), rr.N_HYP, seed)
    assert sets.shape == (rr.N_HYP, 8) and all(len(set(s)) == 8 for s in sets.tolist())
    n1, _ = rr.normalize_seq(m[:, :2])
    n2, _ = rr.normalize_seq(m[:, 2:])
    for model in (0, 1):
        bounds = []
        for idx in sets:
            _, s = rr.null64(rr.build_a(model, n1, n2, idx))
            bounds.append(16 * rr.EPS * s[0] / (s[7] - s[8]))
            if model == 1:
                assert s[8] == 0                                          # 8 x 9: the null vector is exact
        share = np.mean(np.array(bounds) > rr.UNINFORMATIVE)
        print("%s seed %d model %d: largest null-vector bound %.2e, uninformative share %.3f"
              % (kind, seed, model, max(bounds), share))
        assert share <= rr.MAX_UNINFORMATIVE_SHARE


def test_normalize_restatement_is_sequential_f32():
    """the restatement differs from a pairwise (numpy) f32 mean on some input -- it is the loop, not a formula"""
    m, _ = rr.scene("planar", 1)
    pn, T = rr.normalize_seq(m[:, :2])
    assert pn.dtype == np.float32 and T.dtype == np.float32 and T[2].tolist() == [0, 0, 1]
    p = m[:, :2].astype(np.float64)
    mean = p.mean(0)
    s = 1 / np.abs(p - mean).mean(0)
    assert np.allclose(T[[0, 1], [0, 1]], s, rtol=1e-5) and np.allclose(T[:2, 2], -mean * s, rtol=1e-5)
    assert np.allclose(pn, (p - mean) * s, atol=1e-4)
    acc = np.float32(0)
    for v in m[:, 0].astype(np.float32):
        acc = np.float32(acc + v)
    assert T[0, 2] == np.float32(-np.float32(acc / np.float32(len(m)))) * T[0, 0]


def _best_scores(kind, seed, solve):
    m, bad = rr.scene(kind, seed)
    sets = rr.draw_sets(len(m), rr.N_HYP, seed)
    H21, H12, F21 = solve(m, sets)
    model = rr.model_of(kind)
    best, scores, inl = oracle_init.find_best(model, H21 if model == 0 else F21, H12 if model == 0 else None, m, 1.0)
    return m, bad, best, scores, inl


@pytest.mark.parametrize("kind,seed", CASES)
def test_reference_recovers_the_planted_model(kind, seed):
    """float64 hypotheses, rounded to f32, scored by the oracle: the kept one explains the planted inliers"""
    m, bad, best, scores, inl = _best_scores(kind, seed, rr.solve64)
    assert best >= 0
    planted = ~bad
    recall = (inl & planted).sum() / planted.sum()
    print("%s seed %d: best score %.2f, %d inliers, recall of planted inliers %.3f, outliers accepted %d"
          % (kind, seed, scores[best], inl.sum(), recall, (inl & bad).sum()))
    assert recall >= 0.8
    # a homography explains an outlier only by chance; an epipolar line passes near a random point far more often
    assert (inl & bad).sum() <= (0.05 if kind == "planar" else 0.25) * bad.sum()


def test_margin_is_what_the_cpu_shows():
    """rr.MARGIN = twice the largest relative difference between the best score of the float64 solve and of numpy's
    float32 SVD solve of the same sets (neither is code under test)"""
    spread = 0.0
    for kind, seed in CASES:
        _, _, b64, s64, _ = _best_scores(kind, seed, rr.solve64)
        _, _, b32, s32, _ = _best_scores(kind, seed, rr.solve32)
        rel = abs(float(s64[b64]) - float(s32[b32])) / float(s64[b64])
        print("%s seed %d: best score f64 %.4f (hyp %d), f32 SVD %.4f (hyp %d), relative difference %.3e"
              % (kind, seed, s64[b64], b64, s32[b32], b32, rel))
        spread = max(spread, rel)
    print("largest relative difference %.3e" % spread)
    assert spread <= rr.MEASURED_CPU_SPREAD
    assert rr.MARGIN == 2 * rr.MEASURED_CPU_SPREAD


def test_result_structs_match_the_header(tmp_path):
    from mono_slam_framework_amd import _lib
    assert C.sizeof(_lib.RansacResult) == 80 and C.sizeof(_lib.RansacBatch) == 176
    assert _lib.RansacBatch.homography.offset == 16 and _lib.RansacBatch.fundamental.offset == 96
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include "msf_abi.h"\n'
                   "_Static_assert(sizeof(msf_ransac_result) == 80, \"result\");\n"
                   "_Static_assert(sizeof(msf_ransac_batch) == 176, \"batch\");\n"
                   "_Static_assert(offsetof(msf_ransac_result, best) == 48, \"best\");\n"
                   "_Static_assert(offsetof(msf_ransac_result, T2) == 72, \"T2\");\n"
                   "_Static_assert(offsetof(msf_ransac_batch, fundamental) == 96, \"fundamental\");\n"
                   "int main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])
    assert _lib.RansacResult.best.offset == 48 and _lib.RansacResult.T2.offset == 72


def test_new_symbols_exist():
    from mono_slam_framework_amd import _lib
    L = _lib.load()
    for name in ("msf_find_models", "msf_find_models_device"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name)
    hdr = open(os.path.join(ROOT, "include", "msf_abi.h")).read()
    assert "msf_find_models_device(" in hdr and "msf_ransac_batch" in hdr
