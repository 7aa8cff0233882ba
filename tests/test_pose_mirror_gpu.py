"""GPU: csrc/hip_optimizer.h (msf::Optimizer), built with plain g++ against libmsf.so: PoseOptimization on every list
alone and PoseOptimizationBatch on all of them give, bit for bit, what FeatureMatcher.pose_optimize gives -- the return
value, Tcw replaced in place with its last row 0 0 0 1, the flags of every correspondence -- and with fewer than 3
correspondences 0, an untouched Tcw and cleared flags, as Optimizer.cc:285 and :312-333 do."""
import os
import subprocess

import numpy as np
import pytest

from tests import pose_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _build(tmp_path):
    from mono_slam_framework_amd import build
    lib = build.lib_path()
    exe = str(tmp_path / "test_pose_mirror")
    pkg = os.path.join(ROOT, "mono_slam_framework_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(pkg, "csrc"), "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pose_mirror.cpp"), lib,
                           "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-L" + os.path.join(rocm, "lib"),
                           "-lamdhip64", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("pose_mirror"))


def _single_and_batch(exe, tmp_path, scenes):
    """Runs the program on `scenes` (one batch) and holds every "single" and "batch" line to pose_optimize of its list.
    -> the lines, by (kind, list)"""
    from mono_slam_framework_amd.matcher import FeatureMatcher
    entry = []
    f_in, f_out = str(tmp_path / "lists.bin"), str(tmp_path / "log.txt")
    with open(f_in, "wb") as f:
        f.write(np.int32(len(scenes)).tobytes())
        for i, sc in enumerate(scenes):
            T = np.concatenate([sc["Tcw0"], np.array([0, 0, 0, 1 if i % 2 else 7], np.float32)])   # a row 3 to be replaced
            entry.append(T)
            f.write(np.int32(len(sc["p3d"])).tobytes() + T.tobytes() + sc["p3d"].tobytes() + sc["p2d"].tobytes())
    r = subprocess.run([exe, f_in, f_out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {}
    for line in open(f_out):
        head, tcw, idx = line.split("|")
        kind, s, good = head.split()
        idx = [int(x) for x in idx.split()]
        seen[kind, int(s)] = (int(good), np.array(tcw.split(), np.uint32), idx[0], idx[1:])
    fm = FeatureMatcher(0.7, 640, 480)
    for s, sc in enumerate(scenes):
        n = len(sc["p3d"])
        want = fm.pose_optimize(sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"], diagnostics=False)
        if n < 3:
            tcw, flags = entry[s], []
            assert want["n_good"] == 0
        else:
            tcw, flags = np.concatenate([want["Tcw"], np.array([0, 0, 0, 1], np.float32)]), np.flatnonzero(want["outliers"]).tolist()
            assert want["n_good"] == n - len(flags)
        for kind in ("single", "batch"):
            good, bits, size, true = seen[kind, s]
            assert good == want["n_good"] and size == n and true == flags, (kind, s)
            assert bits.tobytes() == tcw.view(np.uint32).tobytes(), (kind, s)
    fm.close()
    return seen


def test_the_mirror_equals_the_python_call(exe, tmp_path):
    """lists of 96, 63, 9 (one round), 2 and 130 correspondences and, between two ordinary ones, a candidate with none:
    an empty row in the middle of the block"""
    scenes = [pr.scene("base", 1), pr.scene("few", 1), pr.scene("wide", 3, 63), pr.scene("base", 1, 0),
              pr.scene("base", 2, 9), pr.scene("base", 2, 2), pr.scene("shallow", 1, 130)]
    seen = _single_and_batch(exe, tmp_path, scenes)
    assert seen["single", 0][0] == int((~scenes[0]["outlier"]).sum())
    assert [len(sc["p3d"]) for sc in scenes[2:5]] == [63, 0, 9]
    good, bits, size, true = seen["batch", 3]
    assert (good, size, true) == (0, 0, []) == (seen["single", 3][0],) + seen["single", 3][2:]
    assert bits.tobytes() == seen["single", 3][1].tobytes()                 # Tcw as it came in, row 3 included


def test_a_batch_of_one_candidate(exe, tmp_path):
    sc = pr.scene("wide", 3, 63)
    seen = _single_and_batch(exe, tmp_path, [sc])
    assert seen["batch", 0][0] == seen["single", 0][0] > 0
