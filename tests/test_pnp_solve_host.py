"""CPU: csrc/pnp_solve.h -- the arithmetic of pnp_kernels.hip (control points, barycentric coordinates, M'M, the 12 x 12
Jacobi in the device's 16-lane order, betas, Gauss-Newton, R and t, CheckInliers, the records and Refine) -- compiled for
the host (g++ -ffp-contract=off, tests/cpp/pnp_solve_host.cpp) and held to the bars of test_pnp_gpu.py against the
float64 reference of tests/pnp_ref.py.  What only the GPU can show (the kernels' indexing, the lanes' exchange, the
batch) is in test_pnp_gpu.py.  The edge inputs run in a stand-alone sanitized executable, never inside python."""
import os
import subprocess

import numpy as np
import pytest

from tests import pnp_host
from tests import pnp_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [4, 5, 15, 16, 17, 63, 64, 65, 96, 257]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pnp_host.build(tmp_path_factory.mktemp("pnp_solve_host"))


@pytest.mark.parametrize("kind,seed", pr.CASES)
def test_host_build_meets_the_float64_bars(host, kind, seed):
    sc = pr.scene(kind, seed)
    sets = pr.draw_sets(seed, pr.N_SCENE, pr.N_ITERATIONS)
    m, its = pr.set_ransac_parameters(pr.N_SCENE)
    assert (m, its) == (48, pr.N_ITERATIONS)
    got = pnp_host.run(host, sc["p3d"], sc["p2d"], sc["K"], m, its, sets=sets)
    ok = pr.check_result(got, sc, sets, m, 8, "host %s seed %d" % (kind, seed))
    if kind == "few":
        assert ok is None
    if kind == "base":                                # a record whose Refine succeeds, so bar 6 was evaluated
        assert ok is not None and got["n_refined"][ok] >= 60


@pytest.mark.parametrize("n", SIZES)
def test_sizes(host, n):
    sc = pr.scene("base", 2, n)
    m, _ = pr.set_ransac_parameters(n, min_inliers=4)
    sets = pr.draw_sets(n, n, 12)
    got = pnp_host.run(host, sc["p3d"], sc["p2d"], sc["K"], m, 12, sets=sets)
    pr.check_result(got, sc, sets, m, 8, "host n %d" % n)


def test_the_draw_is_without_replacement_and_keyed(host):
    seen = set()
    for n in (4, 5, 96):
        for it in range(40):
            s = np.zeros(4, np.int32)
            host.pnp_host_draw(7, 2, it, n, s.ctypes.data)
            assert len(set(s)) == 4 and s.min() >= 0 and s.max() < n
            seen.add((n, tuple(s)))
    assert len(seen) > 60
    a, b, c = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.int32)
    host.pnp_host_draw(7, 2, 3, 96, a.ctypes.data)
    host.pnp_host_draw(7, 2, 3, 96, b.ctypes.data)
    host.pnp_host_draw(8, 2, 3, 96, c.ctypes.data)
    assert (a == b).all() and (a != c).any()


def test_drawn_sets_are_returned_and_replay(host):
    sc = pr.scene("base", 1)
    a = pnp_host.run(host, sc["p3d"], sc["p2d"], sc["K"], 48, 35, seed=11)
    b = pnp_host.run(host, sc["p3d"], sc["p2d"], sc["K"], 48, 35, sets=a["sets"])
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    pr.check_result(a, sc, a["sets"], 48, 8, "host drawn")


def test_max_records_keeps_the_first(host):
    sc = pr.scene("wide", 1)
    sets = pr.draw_sets(1, pr.N_SCENE, pr.N_ITERATIONS)
    full = pnp_host.run(host, sc["p3d"], sc["p2d"], sc["K"], 48, 35, sets=sets)
    one = pnp_host.run(host, sc["p3d"], sc["p2d"], sc["K"], 48, 35, sets=sets, max_records=1)
    assert full["n_records"] >= 2 and one["n_records"] == full["n_records"] and one["capacity"]
    assert one["Tcw_refined"].tobytes() == full["Tcw_refined"][:1].tobytes()


def test_fewer_than_four_points(host):
    sc = pr.scene("base", 1, 3)
    assert pnp_host.run(host, sc["p3d"], sc["p2d"], sc["K"], 4, 5)["n_records"] == -1


def test_edge_inputs_in_a_sanitized_executable(tmp_path):
    """coplanar, coincident, a point at the camera centre, NaN / Inf, n = 4 with min_inliers = 4: every call ends with
    finite-or-NaN poses and counts in [0, n]"""
    exe = str(tmp_path / "pnp_edge")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", pnp_host.CSRC,
                           os.path.join(ROOT, "tests", "cpp", "pnp_edge_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
