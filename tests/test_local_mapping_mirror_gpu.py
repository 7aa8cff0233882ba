"""GPU: csrc/hip_local_mapping.h (msf::NewMapPoints), built with plain g++ against libmsf.so, gives for a query and its
neighbours what create_map_points gives through the Python wrapper: the same records in the same order."""
import os
import subprocess

import numpy as np
import pytest

from tests import local_mapping_ref as lm
from tests.test_create_map_points_gpu import H, SHIFTS, W, plane_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RECORD = np.dtype([("neighbour", "<i4"), ("match", "<i4"), ("kp1", "<i4", (2,)), ("kp2", "<i4", (2,)), ("x3D", "<f4", (3,))])


def _build(tmp_path):
    from mono_slam_framework_amd import build
    lib = build.lib_path()
    exe = str(tmp_path / "test_local_mapping_mirror")
    pkg = os.path.join(ROOT, "mono_slam_framework_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(pkg, "csrc"), "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_local_mapping_mirror.cpp"), lib,
                           "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-L" + os.path.join(rocm, "lib"),
                           "-lamdhip64", "-o", exe])
    return exe


def test_new_map_points_equals_create_map_points(tmp_path):
    from mono_slam_framework_amd import synth
    from mono_slam_framework_amd.matcher import FeatureMatcher
    exe = _build(tmp_path)
    frames = [synth.synth_pair(3, W, H, shift=(0, 0))[0]] + [synth.synth_pair(3, W, H, shift=s)[1] for s in SHIFTS]
    views = np.array([lm.make_view(np.eye(3), np.zeros(3))] + [plane_view(*s) for s in SHIFTS], lm.VIEW_DTYPE)
    f_frames, f_views, f_out = str(tmp_path / "frames.bin"), str(tmp_path / "views.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(np.stack(frames)).tofile(f_frames)
    views.tofile(f_views)
    r = subprocess.run([exe, f_frames, f_views, f_out, str(len(SHIFTS))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(f_out, RECORD)

    fm = FeatureMatcher(0.8, W, H, max_batch_pairs=8)
    for i, f in enumerate(frames):
        fm.store_frame(i, f)
    num, lists, new = fm.create_map_points(0, views[0], list(range(1, len(frames))), views[1:], cap=2048)
    fm.close()
    exp = []
    for i, e in enumerate(new):
        for p in e["packed"]:
            m = lists[i][p["match"]]
            exp.append((i, p["match"], m[:2], m[2:], (p["x"], p["y"], p["z"])))
    exp = np.array(exp, RECORD)
    print(r.stdout.strip(), "| wrapper: %d" % len(exp))
    assert len(got) == len(exp) > 0
    assert got.tobytes() == exp.tobytes()
