"""The host build of csrc/pnp_solve.h (tests/cpp/pnp_solve_host.cpp) behind ctypes: g++ -ffp-contract=off, no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
# HostOut's arrays in its order: name -> (dtype, per iteration / record, trailing shape)
ARRAYS = [("counts", "int32", "it", ()), ("sets", "int32", "it", (4,)), ("pose_f64", "float64", "it", (12,)),
          ("cws", "float64", "it", (4, 3)), ("ut_tail", "float64", "it", (4, 12)), ("betas", "float64", "it", (3, 4)),
          ("rep_errors", "float64", "it", (3,)), ("pca", "float64", "it", (3, 3)),
          ("iteration", "int32", "rec", ()), ("n_inliers", "int32", "rec", ()),
          ("refined_ok", "int32", "rec", ()), ("n_refined", "int32", "rec", ()), ("Tcw_best", "float32", "rec", (12,)),
          ("Tcw_refined", "float32", "rec", (12,)), ("inliers_best", "uint8", "rec", ("n",)),
          ("inliers_refined", "uint8", "rec", ("n",)), ("rec_pose_f64", "float64", "rec", (12,)),
          ("rec_cws", "float64", "rec", (4, 3)), ("rec_ut_tail", "float64", "rec", (4, 12)),
          ("rec_betas", "float64", "rec", (3, 4)), ("rec_rep_errors", "float64", "rec", (3,)),
          ("rec_pca", "float64", "rec", (3, 3))]


def build(directory, optimise="-O2"):
    so = os.path.join(str(directory), "libpnp_solve_host.so")
    subprocess.check_call(["g++", "-std=c++17", optimise, "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "pnp_solve_host.cpp"), "-o", so])
    L = C.CDLL(so)
    L.pnp_host_ransac.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int,
                                  C.c_uint64, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.pnp_host_ransac.restype = C.c_int
    L.pnp_host_draw.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.pnp_host_draw.restype = None
    return L


def run(L, p3d, p2d, K, min_inliers, n_iterations, th2=5.991, max_records=8, seed=0, sets=None, list_index=0):
    """-> the dict that _Matcher.pnp_ransac returns, computed on the host"""
    p3 = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
    p2 = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
    n = len(p3)
    cap = max(n, 1)
    lead = {"it": n_iterations, "rec": max_records}
    d = {name: np.zeros((lead[per],) + tuple(cap if t == "n" else t for t in tail), dt) for name, dt, per, tail in ARRAYS}
    s = None
    if sets is not None:
        s = np.ascontiguousarray(sets, np.int32).reshape(n_iterations, 4)
        d["sets"][:] = s
    ptrs = (C.c_void_p * len(ARRAYS))(*[d[a[0]].ctypes.data for a in ARRAYS])
    k = np.ascontiguousarray(K, np.float32)
    records = L.pnp_host_ransac(n, p3.ctypes.data, p2.ctypes.data, k.ctypes.data, th2, min_inliers, n_iterations,
                                max_records, seed, list_index, s.ctypes.data if s is not None else None, cap, ptrs)
    kept = min(max(records, 0), max_records)
    out = dict(n_records=records, capacity=records > max_records)
    for name, _, per, _ in ARRAYS:
        out[name] = d[name][:kept] if per == "rec" else d[name]
    out["inliers_best"], out["inliers_refined"] = out["inliers_best"][:, :n], out["inliers_refined"][:, :n]
    return out
