"""GPU: csrc/hip_pnp_solver.h (msf::PnPsolver), built with plain g++ against libmsf.so: iterate(5, ...) called until
bNoMore gives the sequence of returns (empty / pose, nInliers, vbInliers scattered through mvKeyPointIndices, bNoMore)
that a Python replay of PnPsolver.cc:172-257 gives over the counts and records of pnp_ransac on the same sets -- for
solvers whose caches one Prefetch filled, for calls after a success, and for calls that reach beyond the cache."""
import os
import subprocess

import numpy as np
import pytest

from tests import pnp_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _build(tmp_path):
    from mono_slam_framework_amd import build
    lib = build.lib_path()
    exe = str(tmp_path / "test_pnp_mirror")
    pkg = os.path.join(ROOT, "mono_slam_framework_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(pkg, "csrc"), "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pnp_mirror.cpp"), lib,
                           "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-L" + os.path.join(rocm, "lib"),
                           "-lamdhip64", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pnp_mirror"))


def _iterate_all(exe, tmp_path, scenes):
    """Runs the program on `scenes` (one Prefetch) and holds every iterate call of every solver to the replay.
    -> the calls by solver, how many solvers reached beyond their cache, how many succeeded twice"""
    from mono_slam_framework_amd.matcher import FeatureMatcher
    f_in, f_out = str(tmp_path / "lists.bin"), str(tmp_path / "log.txt")
    with open(f_in, "wb") as f:
        f.write(np.int32(len(scenes)).tobytes())
        for sc in scenes:
            f.write(np.int32(len(sc["p3d"])).tobytes() + sc["p3d"].tobytes() + sc["p2d"].tobytes())
    r = subprocess.run([exe, f_in, f_out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    calls, solvers = {}, {}
    for line in open(f_out):
        head, *rest = line.split("|")
        w = head.split()
        if w[0] == "solver":
            solvers[int(w[1])] = dict(floor=int(w[2]), its=int(w[3]), prefetched=int(w[4]), cached=int(w[5]),
                                      sets=np.array(rest[0].split(), np.int32).reshape(-1, 4))
        else:
            idx = [int(x) for x in rest[1].split()]
            calls.setdefault(int(w[1]), []).append(dict(ok=int(w[2]), n=int(w[3]), no_more=int(w[4]), its=int(w[5]),
                                                        Tcw=np.array(rest[0].split(), np.uint32), size=idx[0], true=idx[1:]))
    assert (solvers[0]["floor"], solvers[0]["its"]) == (48, 35)             # SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991f), N = 96
    fm = FeatureMatcher(0.7, 640, 480)
    reached_beyond = succeeded_twice = 0
    for s, sc in enumerate(scenes):
        n, info = len(sc["p3d"]), solvers[s]
        assert (info["floor"], info["its"]) == pr.set_ransac_parameters(n)
        replay = pr.IterateReplay(n, 2 * n + 3, 2 * np.arange(n) + 1, info["floor"], info["its"])
        if n >= info["floor"]:
            got = fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], info["floor"], info["cached"], sets=info["sets"], max_records=64)
            assert not got["capacity"]
            replay.results = got
            reached_beyond += info["cached"] > info["prefetched"]
        want = [replay.iterate(5) for _ in calls[s]]
        for c, w in zip(calls[s], want):
            assert (c["ok"], c["n"], c["no_more"], c["its"]) == (w["ok"], w["n"], w["no_more"], w["its"]), (s, c, w)
            assert c["size"] == w["size"] and c["true"] == w["true"], s
            assert c["Tcw"].tobytes() == w["Tcw"].view(np.uint32).tobytes(), s
        assert calls[s][-1]["no_more"] or len(calls[s]) == 12
        succeeded_twice += sum(c["ok"] for c in calls[s]) >= 2
        print("solver %d (N %d): %d calls, returns %s" % (s, n, len(calls[s]), [(c["ok"], c["n"], c["no_more"]) for c in calls[s]]))
    fm.close()
    return calls, reached_beyond, succeeded_twice


def test_iterate_equals_the_replay(exe, tmp_path):
    """solvers of 96, 96, 63 and 9 correspondences and, between them, one of 3: too short for a minimum set, so no sets
    are drawn for its row of the block and its list gives no records"""
    scenes = [pr.scene("base", 1), pr.scene("few", 1), pr.scene("wide", 3, 63), pr.scene("base", 2, 3), pr.scene("base", 2, 9)]
    calls, reached_beyond, succeeded_twice = _iterate_all(exe, tmp_path, scenes)
    assert succeeded_twice >= 1 and reached_beyond >= 1
    # 55 % outliers of 96 cannot reach the floor of 48: empty returns to the end; N = 9 is below its floor of 10
    assert [c["ok"] for c in calls[1]] == [0] * len(calls[1]) and calls[1][-1]["no_more"] and calls[4][0]["no_more"]
    # N = 3: false with bNoMore at the first call, as for a solver that fills its own cache
    assert [(c["ok"], c["n"], c["no_more"], c["size"]) for c in calls[3]] == [(0, 0, 1, 0)]


def test_a_prefetch_of_one_solver(exe, tmp_path):
    calls, _, _ = _iterate_all(exe, tmp_path, [pr.scene("base", 1)])
    assert any(c["ok"] for c in calls[0])
