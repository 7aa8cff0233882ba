"""CPU: csrc/ransac_solve.h -- the arithmetic k_solve_models and k_ransac_sets run per hypothesis -- compiled for the
host (g++ -ffp-contract=off, tests/cpp/ransac_solve_host.cpp) and held to the bars of test_ransac_gpu.py against a
float64 SVD: null vector, rank-2 step, denormalisation, inverse, on every scene and seed.  The device build runs the same
expressions in the same order; what only the GPU can show (the kernels' indexing, the fusion with the scorer, the batch)
is in test_ransac_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import ransac_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ransac_host") / "libransac_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I",
                           os.path.join(ROOT, "mono_slam_framework_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ransac_solve_host.cpp"), "-o", so])
    L = C.CDLL(so)
    L.ransac_host_solve.argtypes = [C.c_int] + [C.c_void_p] * 8
    L.ransac_host_solve.restype = None
    L.ransac_host_draw.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.ransac_host_draw.restype = None
    return L


def solve_host(L, model, n1, n2, T1, T2, sets):
    """-> null_vec, m21, m12, fn, each f32 [n_hyp, 9]"""
    out = [np.zeros((len(sets), 9), np.float32) for _ in range(4)]
    T1 = np.ascontiguousarray(T1, np.float32)
    T2 = np.ascontiguousarray(T2, np.float32)
    for k, idx in enumerate(sets):
        a = np.ascontiguousarray(n1[idx], np.float32)
        b = np.ascontiguousarray(n2[idx], np.float32)
        L.ransac_host_solve(model, a.ctypes.data, b.ctypes.data, T1.ctypes.data, T2.ctypes.data,
                            *[o[k:].ctypes.data for o in out])
    return out


@pytest.mark.parametrize("kind", rr.SCENES)
@pytest.mark.parametrize("seed", rr.SEEDS)
def test_host_build_meets_the_float64_bars(host, kind, seed):
    m, _ = rr.scene(kind, seed)
    sets = rr.draw_sets(len(m), rr.N_HYP, seed)
    n1, T1 = rr.normalize_seq(m[:, :2])
    n2, T2 = rr.normalize_seq(m[:, 2:])
    for model in (0, 1):
        nv, m21, m12, fn = solve_host(host, model, n1, n2, T1, T2, sets)
        rr.check_solver_output(sets, model, n1, n2, T1, T2, nv, m21, m12, fn, label="host %s seed %d" % (kind, seed))


def test_non_finite_input_gives_non_finite_models(host):
    """an infinite scale (all x equal) makes NaN points: the solver ends and every output entry is non-finite"""
    n1 = np.full((8, 2), np.nan, np.float32)
    n2 = np.random.RandomState(0).randn(8, 2).astype(np.float32)
    T = np.eye(3, dtype=np.float32)
    Tinf = T.copy()
    Tinf[0, 0] = np.inf
    Tinf[0, 2] = np.nan
    sets = np.arange(8)[None]
    for model in (0, 1):
        nv, m21, m12, fn = solve_host(host, model, n1, n2, Tinf, T, sets)
        assert not np.isfinite(nv).any() and not np.isfinite(m21).any()
        if model == 0:
            assert not np.isfinite(m12).any()


def test_degenerate_but_finite_sets_terminate(host):
    """eight collinear points, and one match repeated eight times: finite A of rank < 8; the solver returns a unit vector"""
    t = np.linspace(-1, 1, 8, dtype=np.float32)
    line = np.stack([t, 2 * t], 1).astype(np.float32)
    same = np.tile(np.array([[0.3, -0.7]], np.float32), (8, 1))
    T = np.eye(3, dtype=np.float32)
    for pts in (line, same):
        for model in (0, 1):
            nv, m21, _, _ = solve_host(host, model, pts, pts[::-1].copy(), T, T, np.arange(8)[None])
            assert abs(np.linalg.norm(nv[0].astype(np.float64)) - 1) < 1e-6
            A = rr.build_a(model, pts, pts[::-1].copy(), np.arange(8)).astype(np.float64)
            s1 = np.linalg.svd(A, compute_uv=False)[0]
            assert np.linalg.norm(A @ nv[0]) <= 32 * rr.EPS * s1      # some vector of the (larger) null space


def test_draw_is_the_reference_procedure(host):
    """draw_set = the reference's draw (copy the index list; eight times: randi, take avail[randi], move the last element
    in) with randi from the documented counter-based generator, restated here in Python integers"""
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    for seed, lst, it, n in ((0, 0, 0, 8), (7, 3, 199, 9), (2 ** 63 + 5, 1023, 17, 300), (99, 5, 1, 8192)):
        avail = list(range(n))
        exp = []
        for j in range(8):
            word = mix(seed ^ mix(((((lst << 20) + it) * 8 + j) + 0x9E3779B97F4A7C15) & M))
            randi = (word * len(avail)) >> 64
            exp.append(avail[randi])
            avail[randi] = avail[-1]
            avail.pop()
        got = np.zeros(8, np.int32)
        host.ransac_host_draw(seed, lst, it, n, got.ctypes.data)
        assert got.tolist() == exp
        assert len(set(exp)) == 8
