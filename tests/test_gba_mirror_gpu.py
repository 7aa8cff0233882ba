"""GPU: msf::BundleAdjuster::GlobalBundleAdjustment (csrc/hip_bundle_adjustment.h), built with plain g++ against
libmsf.so, on the (80 + 2) x 400 scene: with and without the stop word it gives, bit for bit, what
FeatureMatcher.global_bundle_adjust gives, and a malformed problem is a failed call that leaves the problem alone."""
import os
import subprocess

import numpy as np
import pytest

from tests import gba_scenes as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_the_mirror_equals_the_python_call(tmp_path):
    from mono_slam_framework_amd import build
    from mono_slam_framework_amd.matcher import FeatureMatcher
    lib = build.lib_path()
    exe = str(tmp_path / "test_gba_mirror")
    pkg = os.path.join(ROOT, "mono_slam_framework_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(pkg, "csrc"), "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_gba_mirror.cpp"), lib,
                           "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-L" + os.path.join(rocm, "lib"),
                           "-lamdhip64", "-o", exe])
    sc, schedule = gs.scene("g80")
    nc, npt, ne = len(sc["cam_Tcw"]), len(sc["points"]), len(sc["edge_cam"])
    T16 = np.concatenate([sc["cam_Tcw"].reshape(nc, 12), np.tile(np.array([0, 0, 0, 7], np.float32), (nc, 1))], 1)
    f_in, f_out = str(tmp_path / "problem.bin"), str(tmp_path / "log.txt")
    with open(f_in, "wb") as f:
        f.write(np.array([nc, npt, ne], np.int32).tobytes() + T16.tobytes() + sc["cam_fixed"].tobytes() + sc["points"].tobytes()
                + sc["edge_cam"].tobytes() + sc["edge_point"].tobytes() + sc["edge_obs"].tobytes())
    r = subprocess.run([exe, f_in, f_out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    seen = {}
    for line in open(f_out):
        head, tcw, pts, idx = line.split("|")
        kind, rounds = head.split()
        idx = [int(x) for x in idx.split()]
        seen[kind] = (int(rounds), np.array(tcw.split(), np.uint32), np.array(pts.split(), np.uint32), idx[0], idx[1:])
    fm = FeatureMatcher(0.7, 640, 480)
    call = lambda **kw: fm.global_bundle_adjust(sc["cam_Tcw"], sc["cam_fixed"], sc["points"], sc["edge_cam"], sc["edge_point"],
                                                sc["edge_obs"], sc["K"], schedule=schedule, diagnostics=False, **kw)
    want = {"global": call(), "stopped": call(stop=1)}
    for kind, w in want.items():
        rounds, tcw_bits, pts_bits, size, flagged = seen[kind]
        assert rounds == w["status"] == {"global": 1, "stopped": 0}[kind], kind
        T = np.concatenate([w["cam_Tcw"], T16[:, 12:]], 1)
        assert tcw_bits.tobytes() == T.view(np.uint32).tobytes(), kind
        assert pts_bits.tobytes() == w["points"].view(np.uint32).tobytes(), kind
        assert size == ne and flagged == np.flatnonzero(w["outliers"]).tolist(), kind
    assert (want["global"]["cam_Tcw"] != sc["cam_Tcw"].reshape(nc, 12)).any()
    fm.close()
