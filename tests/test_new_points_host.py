"""CPU: csrc/triangulate_solve.h -- the arithmetic of triangulate_kernels.hip (new_point: ray parallax, the 4 x 4
triangulation, depth signs, reprojection errors) -- compiled for the host (g++ -ffp-contract=off,
tests/cpp/new_points_host.cpp) and held to the bars of test_new_points_gpu.py against the float64 reference of
tests/local_mapping_ref.py on all six scene cases and the hand-made matches.  The device build runs the same expressions
in the same order; what only the GPU can show (the kernel's indexing, the scan, the batch) is in test_new_points_gpu.py.
The edge inputs run in a stand-alone sanitized executable, never inside python."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import local_mapping_ref as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
PACKED = np.dtype([("match", "<i4"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4")])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("new_points_host") / "libnew_points_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "new_points_host.cpp"), "-o", so])
    L = C.CDLL(so)
    L.new_points_host_run.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double] + [C.c_void_p] * 5
    L.new_points_host_run.restype = C.c_int
    return L


def run_host(L, matches, v1, v2, max_cos=1.1, chi2=lm.CHI2):
    m = np.ascontiguousarray(matches, np.int32).reshape(-1, 4)
    n = len(m)
    v1, v2 = np.array(v1, lm.VIEW_DTYPE).reshape(1), np.array(v2, lm.VIEW_DTYPE).reshape(1)
    o = dict(status=np.zeros(n, np.uint8), points=np.zeros((n, 3), np.float32), hom=np.zeros((n, 4), np.float32),
             cos_parallax=np.zeros(n, np.float64), packed=np.zeros(n, PACKED))
    o["n_new"] = L.new_points_host_run(n, m.ctypes.data, v1.ctypes.data, v2.ctypes.data, max_cos, chi2,
                                       *[o[k].ctypes.data for k in ("status", "points", "hom", "cos_parallax", "packed")])
    o["packed"] = o["packed"][:o["n_new"]]
    return o


@pytest.mark.parametrize("seed,max_cos", lm.CASES)
def test_host_build_meets_the_float64_bars(host, seed, max_cos):
    view1, views2, matches = lm.scene(seed)
    refs = lm.scene_reference(seed, max_cos)
    worst = 0.0
    for i in range(lm.N_NEIGHBOURS):
        got = run_host(host, matches[i], view1, views2[i], max_cos)
        w, _ = lm.check_result(refs[i], got, matches[i], view1, views2[i], max_cos,
                               label="host seed %d max_cos %g list %d" % (seed, max_cos, i))
        worst = max(worst, w)
    print("host seed %d max_cos %g: null vector worst err / bound %.3f" % (seed, max_cos, worst))


def test_handmade_matches(host):
    v1, v2, m = lm.handmade()
    got = run_host(host, m, v1, v2)
    lm.check_result(lm.handmade_reference(), got, m, v1, v2, label="host handmade")
    assert list(got["status"]) == [3, 1, 0]
    assert got["hom"][0, 3] == 0 and abs(got["hom"][0, 2]) == 1       # the zero column: exact
    assert np.allclose(got["points"][2], [0.5, 0.0, 5.0], atol=1e-5)


def test_max_cos_zero_rejects_everything_at_stage_two(host):
    view1, views2, matches = lm.scene(1)
    got = run_host(host, matches[0], view1, views2[0], 0.0)
    assert got["n_new"] == 0 and set(got["status"]) <= {1, 2} and not got["points"].any()


def test_edge_inputs_in_a_sanitized_executable(tmp_path):
    """identical views, NaN / Inf poses, all-zero views, INT32 extremes: new_point ends with a status in 0..7"""
    exe = str(tmp_path / "new_points_edge")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "new_points_edge_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
