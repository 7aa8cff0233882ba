"""CPU: csrc/reconstruct_solve.h -- the arithmetic of reconstruct_kernels.hip (svd3, decompose_e / decompose_h,
triangulate, check_match, the selection rules) -- compiled for the host (g++ -ffp-contract=off,
tests/cpp/reconstruct_host.cpp) and held to the bars of test_reconstruct_gpu.py against the float64 reference of
tests/initializer_ref.py on all nine cases.  The device build runs the same expressions in the same order; what only the
GPU can show (the kernels' indexing, the radix selection, the batch) is in test_reconstruct_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import initializer_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("reconstruct_host") / "libreconstruct_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I",
                           os.path.join(ROOT, "mono_slam_framework_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "reconstruct_host.cpp"), "-o", so])
    L = C.CDLL(so)
    L.reconstruct_host_svd3.argtypes = [C.c_void_p] * 4
    L.reconstruct_host_svd3.restype = None
    L.reconstruct_host_run.argtypes = ([C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_float, C.c_int] +
                                       [C.c_void_p] * 13)
    L.reconstruct_host_run.restype = C.c_int
    L.reconstruct_host_pick.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]
    L.reconstruct_host_pick.restype = C.c_int
    L.reconstruct_host_key.argtypes = [C.c_double]
    L.reconstruct_host_key.restype = C.c_uint64
    L.reconstruct_host_unkey.argtypes = [C.c_uint64]
    L.reconstruct_host_unkey.restype = C.c_double
    return L


def run_host(L, model, m21, matches, inliers, Kf=ir.K, sigma=ir.SIGMA, min_tri=ir.MIN_TRIANGULATED,
             min_par=ir.MIN_PARALLAX):
    m = np.ascontiguousarray(matches, np.int32).reshape(-1, 4)
    n = len(m)
    inl = np.ascontiguousarray(inliers, np.uint8)
    m21 = np.ascontiguousarray(m21, np.float32).reshape(9)
    Kf = np.ascontiguousarray(Kf, np.float32).reshape(9)
    o = dict(w=np.zeros(3, np.float32), n_cand=np.zeros(1, np.int32), cand_R=np.zeros((8, 3, 3), np.float32),
             cand_t=np.zeros((8, 3), np.float32), cand_good=np.zeros(8, np.int32), cand_parallax=np.zeros(8, np.float32),
             flags=np.zeros((8, max(n, 1)), np.uint8), pts=np.zeros((8, max(n, 1), 3), np.float32),
             hom=np.zeros((8, max(n, 1), 4), np.float32), winner=np.zeros(1, np.int32), early=np.zeros(1, np.int32))
    ok = L.reconstruct_host_run(model, m21.ctypes.data, Kf.ctypes.data, sigma, min_tri, min_par, n, m.ctypes.data,
                                inl.ctypes.data, *[o[k].ctypes.data for k in
                                                   ("w", "n_cand", "cand_R", "cand_t", "cand_good", "cand_parallax", "flags",
                                                    "pts", "hom", "winner", "early")])
    o.update(ok=ok, n_cand=int(o["n_cand"][0]), winner=int(o["winner"][0]), early=int(o["early"][0]))
    return o


@pytest.mark.parametrize("kind,seed", ir.CASES)
def test_host_build_meets_the_float64_bars(host, kind, seed):
    c = ir.case(kind, seed)
    name = "H" if c["model"] == 0 else "F"
    ref = ir.case_reference(kind, seed)
    got = run_host(host, c["model"], c[name]["m21"], c["matches"], c[name]["inliers"])
    ir.check_result(ref, got, c["matches"], c[name]["inliers"], label="host %s seed %d" % (kind, seed))
    assert got["ok"] == ir.EXPECT_OK[(kind, seed)]
    if got["ok"]:   # vP3D of the winner against the float64 points, relative to the point's norm
        chk = ref["checks"][ref["winner"]]
        both = chk["counted"] & ((got["flags"][got["winner"]] & 1) != 0)
        err = np.linalg.norm(got["pts"][got["winner"]][both] - chk["points"][both], axis=1)
        rel = err / np.linalg.norm(chk["points"][both], axis=1)
        print("host %s seed %d: relative point error %.3e" % (kind, seed, rel.max()))


@pytest.mark.parametrize("kind", ("two_view", "wide"))
def test_planted_f_gives_every_inlier_to_one_candidate(host, kind):
    F, _, _ = ir.planted_f(kind)
    for seed in (1, 2, 3):
        m, bad = ir.scene(kind, seed)
        got = run_host(host, 1, F, m, ~bad)
        ref = ir.reconstruct(1, F, m, ~bad)
        ir.check_result(ref, got, m, ~bad, label="planted %s seed %d" % (kind, seed))
        assert got["ok"] == 1 and got["cand_good"][got["winner"]] >= 0.97 * (~bad).sum()


def test_svd3_factors_its_input(host):
    """a = u diag(w) v' with w descending, orthogonal u and v, on random, rank-2 and rank-1 matrices"""
    r = np.random.RandomState(0)
    mats = [r.randn(3, 3) for _ in range(20)]
    u0, _, vt0 = np.linalg.svd(r.randn(3, 3))
    mats.append(u0 @ np.diag([3.0, 2.9, 0.0]) @ vt0)          # an essential matrix's spectrum
    mats.append(np.diag([1.0, 1.0, 1.0]))
    for a in mats:
        a = np.ascontiguousarray(a, np.float32)
        u, w, v = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros((3, 3), np.float32)
        host.reconstruct_host_svd3(a.ctypes.data, u.ctypes.data, w.ctypes.data, v.ctypes.data)
        s1 = np.linalg.svd(a.astype(np.float64), compute_uv=False)
        assert np.abs(w - s1).max() <= 16 * ir.EPS * s1[0]
        assert w[0] >= w[1] >= w[2]
        u64, v64 = u.astype(np.float64), v.astype(np.float64)
        assert np.abs(u64 @ np.diag(w.astype(np.float64)) @ v64.T - a).max() <= 16 * ir.EPS * s1[0]
        assert np.abs(u64.T @ u64 - np.eye(3)).max() <= 16 * ir.EPS
        assert np.abs(v64.T @ v64 - np.eye(3)).max() <= 16 * ir.EPS


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
@pytest.mark.parametrize("model", (0, 1))
def test_non_finite_models_terminate_with_no_result(host, model, bad):
    c = ir.case("planar" if model == 0 else "wide", 2)
    name = "H" if model == 0 else "F"
    for where in (0, 4, 8, None):
        m21 = c[name]["m21"].copy().reshape(9)
        if where is None:
            m21[:] = bad
        else:
            m21[where] = bad
        got = run_host(host, model, m21, c["matches"], c[name]["inliers"])
        assert got["ok"] == 0 and got["winner"] == -1
        for k in range(got["n_cand"]):   # a candidate with a non-finite entry is never counted on
            if not (np.isfinite(got["cand_R"][k]).all() and np.isfinite(got["cand_t"][k]).all()):
                assert got["cand_good"][k] == 0 and got["cand_parallax"][k] == 0


def test_rank_one_h_and_identity_h(host):
    c = ir.case("planar", 1)
    inl = c["H"]["inliers"]
    rank1 = np.outer([1.0, 0.5, 0.001], [0.2, 0.1, 1.0]).astype(np.float32)
    got = run_host(host, 0, rank1, c["matches"], inl)
    assert got["ok"] == 0 and got["winner"] == -1      # rounded to f32 the matrix has full rank: it ends, with no result
    eye = run_host(host, 0, np.eye(3, dtype=np.float32), c["matches"], inl)
    assert eye["early"] == 1 and eye["ok"] == 0 and eye["n_cand"] == 0      # d1 / d2 < 1.00001


def test_singular_k_gives_no_result(host):
    c = ir.case("planar", 1)
    K0 = ir.K.copy()
    K0[0, 0] = 0
    for model, name in ((0, "H"), (1, "F")):
        got = run_host(host, model, c[name]["m21"], c["matches"], c[name]["inliers"], Kf=K0)
        assert got["ok"] == 0 and got["winner"] == -1


def test_selection_rules_equal_the_reference_restatement(host):
    r = np.random.RandomState(3)
    for _ in range(2000):
        model = int(r.randint(2))
        k = 8 if model == 0 else 4
        good = r.choice([0, 1, 40, 49, 50, 51, 70, 71, 100, 180, 181, 200], k).astype(np.int32)
        par = r.choice([0.0, 0.5, 1.0, 1.5, 8.0], k).astype(np.float32)
        N = int(r.choice([0, 10, 55, 56, 100, 200, 223]))
        min_tri = int(r.choice([0, 50, 100]))
        exp = (ir.pick_h if model == 0 else ir.pick_f)(list(good), list(par), N, min_tri, np.float32(1.0))
        got = host.reconstruct_host_pick(model, good.ctypes.data, par.ctypes.data, N, min_tri, 1.0)
        assert got == exp, (model, good, par, N, min_tri)


def test_keys_keep_the_order_of_the_doubles(host):
    vals = np.array([-np.inf, -1.0, -1e-300, -0.0, 0.0, 1e-300, 0.5, 0.99998, 1.0, np.nextafter(1.0, 2), np.inf])
    keys = [host.reconstruct_host_key(float(v)) for v in vals]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for v, k in zip(vals, keys):
        back = host.reconstruct_host_unkey(k)
        assert back == v and np.signbit(back) == np.signbit(v)
    nan = host.reconstruct_host_key(float("nan"))
    assert keys[-1] < nan < 2 ** 64 - 1
