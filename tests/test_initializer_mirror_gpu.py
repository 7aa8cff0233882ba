"""GPU: csrc/hip_initializer.h (msf::Initialize), built with plain g++ against libmsf.so, gives for one match list what
find_models_device + reconstruct_device give for it through the Python wrappers: the same bits."""
import os
import subprocess

import numpy as np
import pytest

from tests import initializer_ref as ir
from tests import ransac_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _build(tmp_path):
    from mono_slam_framework_amd import build
    lib = build.lib_path()
    exe = str(tmp_path / "test_initializer_mirror")
    pkg = os.path.join(ROOT, "mono_slam_framework_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(pkg, "csrc"), "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_initializer_mirror.cpp"), lib,
                           "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-L" + os.path.join(rocm, "lib"),
                           "-lamdhip64", "-o", exe])
    return exe


@pytest.mark.parametrize("kind,seed", (("planar", 1), ("wide", 3), ("two_view", 2)))
def test_initialize_equals_the_two_device_calls(tmp_path, kind, seed):
    import torch
    from mono_slam_framework_amd.matcher import FeatureMatcher
    exe = _build(tmp_path)
    m = np.ascontiguousarray(ir.case(kind, seed)["matches"], np.int32)
    src, dst = str(tmp_path / "matches.bin"), str(tmp_path / "out.bin")
    m.tofile(src)
    r = subprocess.run([exe, src, dst, "200", "41"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(dst, "rb").read()
    ok, n_pts = np.frombuffer(raw, np.int32, 2)
    R21, t21 = np.frombuffer(raw, np.float32, 9, 8), np.frombuffer(raw, np.float32, 3, 44)

    fm = FeatureMatcher(0.7, rr.W, rr.H)
    d_m = torch.from_numpy(m[None]).cuda()
    d_n = torch.tensor([len(m)], dtype=torch.int32, device="cuda")
    found = fm.find_models_device(d_m, d_n, n_hyp=200, seed=41)
    exp = {k: v.cpu().numpy()[0] for k, v in fm.reconstruct_device(d_m, d_n, found, ir.K).items()}
    fm.close()
    print("%s seed %d: ok %d (wrappers %d), model %d" % (kind, seed, ok, exp["ok"], exp["model"]))
    assert ok == exp["ok"]
    np.testing.assert_array_equal(R21.view(np.uint32), exp["R21"].reshape(9).view(np.uint32))
    np.testing.assert_array_equal(t21.view(np.uint32), exp["t21"].view(np.uint32))
    if ok:
        assert n_pts == len(m)
        pts = np.frombuffer(raw, np.float32, 3 * n_pts, 56).reshape(-1, 3)
        tri = np.frombuffer(raw, np.uint8, n_pts, 56 + 12 * n_pts)
        np.testing.assert_array_equal(pts.view(np.uint32), exp["points"].view(np.uint32))
        np.testing.assert_array_equal(tri, exp["triangulated"])
    else:
        assert n_pts == 0
