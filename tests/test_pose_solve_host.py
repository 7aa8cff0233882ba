"""CPU: csrc/pose_solve.h -- the arithmetic of pose_kernels.hip (SE3Quat, exp, the edge and its Jacobian, Huber, the
6 x 6 Cholesky, the Levenberg-Marquardt trials, the rounds and the flags) -- compiled for the host (g++
-ffp-contract=off, tests/cpp/pose_solve_host.cpp) and held to the bars of test_pose_gpu.py against the float64
reference of tests/pose_ref.py, with the sums in the device's order (Emu64) and in index order (Serial).  What only the
GPU can show (the kernel's indexing, the lanes' exchange, the batch, the strides) is in test_pose_gpu.py.  The edge
inputs run in a stand-alone sanitized executable, never inside python."""
import os
import subprocess

import numpy as np
import pytest

from tests import pose_host
from tests import pose_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 2, 3, 9, 10, 63, 64, 65, 128, 129, 257]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return pose_host.build(tmp_path_factory.mktemp("pose_solve_host"))


@pytest.mark.parametrize("emu64", [True, False])
@pytest.mark.parametrize("kind,seed", pr.CASES)
def test_host_build_meets_the_float64_bars(host, kind, seed, emu64):
    sc = pr.scene(kind, seed)
    got = pose_host.run(host, sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"], emu64=emu64)
    clear, run = pr.check_result(got, sc, "host %s seed %d" % (kind, seed), scene_conditions=True)
    print("%s seed %d: %d clear iterations of %d" % (kind, seed, clear, run))
    assert (got["outliers"].astype(bool) == sc["outlier"]).all()


@pytest.mark.parametrize("n", SIZES)
def test_sizes(host, n):
    sc = pr.scene("base", 2, n)
    got = pose_host.run(host, sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"])
    pr.check_result(got, sc, "host n %d" % n)


def test_mask_with_every_third_entry_out(host):
    sc = pr.scene("wide", 2)
    mask = (np.arange(pr.N_SCENE) % 3 != 0).astype(np.uint8)
    got = pose_host.run(host, sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"], mask=mask)
    pr.check_result(got, sc, "host masked", mask=mask)
    assert got["n_edges"] == 64 and not got["outliers"][mask == 0].any()
    # the masked list equals the list of the edges alone, up to the order of the sums
    keep = mask.astype(bool)
    cut = dict(sc, p3d=sc["p3d"][keep], p2d=sc["p2d"][keep])
    alone = pose_host.run(host, cut["p3d"], cut["p2d"], sc["K"], sc["Tcw0"], emu64=False)
    masked = pose_host.run(host, sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"], mask=mask, emu64=False)
    assert alone["pose_f64"].tobytes() == masked["pose_f64"].tobytes() and alone["n_good"] == masked["n_good"]


def test_exp_and_the_update_against_numpy(host):
    rng = np.random.default_rng(3)
    for scale in (1.0, 1e-3, 3e-6, 0.0):
        dx = rng.normal(size=6) * scale
        R, t = np.zeros(9), np.zeros(3)
        host.pose_host_exp(dx.ctypes.data, R.ctypes.data, t.ctypes.data)
        Rn, tn = pr.se3_exp(dx)
        assert np.abs(R.reshape(3, 3) - Rn).max() <= 8 * pr.EPS and np.abs(t - tn).max() <= 8 * pr.EPS * max(scale, 1e-300)
        sc = pr.scene("base", 1)
        est = pr.estimate_of(sc["Tcw0"])
        flat, out = np.concatenate(est), np.zeros(7)
        host.pose_host_moved(flat.ctypes.data, dx.ctypes.data, out.ctypes.data)
        want = pr.moved(est, dx)
        assert np.abs(out - np.concatenate(want)).max() <= 16 * pr.EPS * max(1.0, np.abs(flat).max())


def test_edge_inputs_in_a_sanitized_executable(tmp_path):
    """points on or behind the camera plane, identical points, n in {0, 2, 3, 9, 10}, a NaN pose, an all-zero mask:
    every call ends with n_good in range and no Inf in the pose"""
    exe = str(tmp_path / "pose_edge")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", pose_host.CSRC,
                           os.path.join(ROOT, "tests", "cpp", "pose_edge_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
