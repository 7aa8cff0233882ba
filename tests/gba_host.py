"""The host build of csrc/gba_solve.h (tests/cpp/gba_solve_host.cpp) behind ctypes: g++ -ffp-contract=off, no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import ba_host

ROOT = ba_host.ROOT
CSRC = ba_host.CSRC


def build(directory, optimise="-O2"):
    so = os.path.join(str(directory), "libgba_solve_host.so")
    subprocess.check_call(["g++", "-std=c++17", optimise, "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror", "-I", CSRC,
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "gba_solve_host.cpp"), "-o", so])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.gba_host_adjust.argtypes = [C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_double, C.c_double, vp]
    L.gba_host_adjust.restype = C.c_int
    for f in (L.gba_host_solve_tiled, L.gba_host_solve_reference):
        f.argtypes = [C.c_int, vp, vp, vp]
        f.restype = C.c_int
    return L


def solve(L, S, tiled):
    """S: float64 [n, n + 1], row j = column j of the system with b_S as its last entry (column-major, ld = n + 1).
    -> (S after, diag, x, verdict); diag and x start as NaN, so what was not written stays NaN"""
    n = S.shape[0]
    S = np.ascontiguousarray(S, np.float64).copy()
    diag, x = np.full(n, np.nan), np.full(n, np.nan)
    f = L.gba_host_solve_tiled if tiled else L.gba_host_solve_reference
    return S, diag, x, f(n, S.ctypes.data, diag.ctypes.data, x.ctypes.data)


def run(L, sc, schedule, stop=None, huber_delta2=5.991, chi2=5.991, diagnostics=True):
    """as ba_host.run, through the phases chained as the device chains them"""
    from mono_slam_framework_amd import _lib
    nc, npt, ne = len(sc["cam_Tcw"]), len(sc["points"]), len(sc["edge_cam"])
    d = {k: np.zeros(shape, dt) for k, (shape, dt) in _lib.ba_shapes(1, nc, npt, ne).items()}
    given = [a[0] for a in _lib.BA_ARRAYS if diagnostics or not a[0].startswith("it_")]
    ptrs = (C.c_void_p * len(_lib.BA_ARRAYS))(*[d[a[0]].ctypes.data if a[0] in given and d[a[0]].size else None
                                                for a in _lib.BA_ARRAYS])
    ptrs[0] = d["status"].ctypes.data
    tcw = np.ascontiguousarray(sc["cam_Tcw"], np.float32).reshape(-1, 12)
    fixed = np.ascontiguousarray(sc["cam_fixed"], np.uint8)
    pts = np.ascontiguousarray(sc["points"], np.float32)
    ec, ep = np.ascontiguousarray(sc["edge_cam"], np.int32), np.ascontiguousarray(sc["edge_point"], np.int32)
    obs = np.ascontiguousarray(sc["edge_obs"], np.float32)
    k = np.ascontiguousarray(sc["K"], np.float32)
    sched = np.array([schedule[0], schedule[1][0], schedule[1][1], schedule[2][0], schedule[2][1]], np.int32)
    st = None if stop is None else np.array([stop], np.int32)
    status = L.gba_host_adjust(nc, tcw.ctypes.data, fixed.ctypes.data, npt, pts.ctypes.data, ne, ec.ctypes.data,
                               ep.ctypes.data, obs.ctypes.data, st.ctypes.data if st is not None else None, k.ctypes.data,
                               sched.ctypes.data, huber_delta2, chi2, ptrs)
    assert status != -2
    return ba_host.shape_result(d, nc, npt)


def _bits(x):
    """the bytes of an array with every NaN as one NaN: IEEE 754 leaves a NaN's sign and payload open, and an x86 host
    and the GPU fill them differently (0 * inf is -NaN on one and +NaN on the other); where the NaNs are is compared"""
    x = np.ascontiguousarray(x)
    if x.dtype.kind == "f":
        x = np.where(np.isnan(x), np.array(np.nan, x.dtype), x)
    return np.ascontiguousarray(x).tobytes()


def same(a, b, names=None):
    """-> the arrays of two result dicts that differ in a byte"""
    from mono_slam_framework_amd import _lib
    out = []
    for name in names or [x[0] for x in _lib.BA_ARRAYS]:
        if name not in a and name not in b:
            continue
        x, y = np.asarray(a[name]), np.asarray(b[name])
        if x.shape != y.shape or (x.ndim and x.dtype != y.dtype) or _bits(x) != _bits(y.astype(x.dtype)):
            out.append(name)
    return out
