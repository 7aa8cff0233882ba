"""The host build of csrc/pose_solve.h (tests/cpp/pose_solve_host.cpp) behind ctypes: g++ -ffp-contract=off, no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
# the arrays pose_host_optimize writes, in its order: name -> (dtype, shape; "n" = the list's length)
ARRAYS = [("n_edges", "int32", (1,)), ("rounds_run", "int32", (1,)), ("Tcw", "float32", (12,)), ("pose_f64", "float64", (12,)),
          ("outliers", "uint8", ("n",)), ("round_pose_f64", "float64", (4, 12)), ("round_n_bad", "int32", (4,)),
          ("round_iterations", "int32", (4,)), ("it_trials", "int32", (4, 10)), ("it_lambda_in", "float64", (4, 10)),
          ("it_lambda_out", "float64", (4, 10)), ("it_cost_in", "float64", (4, 10)), ("it_cost_out", "float64", (4, 10)),
          ("it_H", "float64", (4, 10, 21)), ("it_b", "float64", (4, 10, 6)), ("it_pose_out", "float64", (4, 10, 7))]


def build(directory, optimise="-O2"):
    so = os.path.join(str(directory), "libpose_solve_host.so")
    subprocess.check_call(["g++", "-std=c++17", optimise, "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "pose_solve_host.cpp"), "-o", so])
    L = C.CDLL(so)
    L.pose_host_optimize.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                     C.c_int, C.c_void_p]
    L.pose_host_optimize.restype = C.c_int
    L.pose_host_exp.argtypes = [C.c_void_p] * 3
    L.pose_host_exp.restype = None
    L.pose_host_moved.argtypes = [C.c_void_p] * 3
    L.pose_host_moved.restype = None
    return L


def run(L, p3d, p2d, K, Tcw0, mask=None, chi2=5.991, emu64=True):
    """-> the dict that _Matcher.pose_optimize returns, computed on the host"""
    p3 = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
    p2 = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
    t0 = np.ascontiguousarray(Tcw0, np.float32).reshape(12)
    n = len(p3)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(n)
    d = {name: np.zeros(tuple(max(n, 1) if t == "n" else t for t in shape), dt) for name, dt, shape in ARRAYS}
    ptrs = (C.c_void_p * len(ARRAYS))(*[d[a[0]].ctypes.data for a in ARRAYS])
    k = np.ascontiguousarray(K, np.float32)
    good = L.pose_host_optimize(n, p3.ctypes.data, p2.ctypes.data, m.ctypes.data if m is not None else None,
                                k.ctypes.data, chi2, t0.ctypes.data, 1 if emu64 else 0, ptrs)
    out = dict(d, n_good=good, n_edges=int(d["n_edges"][0]), rounds_run=int(d["rounds_run"][0]))
    out["outliers"] = out["outliers"][:n]
    return out
