"""The host build of csrc/frame_tracking_solve.h (tests/cpp/frame_tracking_host.cpp) behind ctypes, for the CPU and the
GPU tests, and the comparison of a build's outputs with tests/frame_tracking_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import frame_tracking_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
_KEYS = ("points", "observed", "ref_key", "ref_point", "cur_key", "cur_point")


class Map(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("n_ref", C.c_int32), ("n_cur", C.c_int32)] + [(k, C.c_void_p) for k in _KEYS]


def build(directory):
    so = os.path.join(str(directory), "libframe_tracking_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "frame_tracking_host.cpp"), "-o", so])
    L = C.CDLL(so)
    L.frame_tracking_host_carry.argtypes = [C.POINTER(Map), C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int32, C.c_int, C.c_int] + \
                                           [C.c_void_p] * 7
    L.frame_tracking_host_cut.argtypes = [C.POINTER(Map), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    return L


def _c_map(fmap):
    fmap = {k: None if fmap.get(k) is None else np.ascontiguousarray(fmap[k]) for k in _KEYS}
    m = Map(len(fmap["points"]), len(fmap["ref_key"]), len(fmap["cur_key"]),
            *[None if fmap[k] is None else fmap[k].ctypes.data for k in _KEYS])
    return m, fmap          # the arrays live as long as the caller keeps `fmap`


def pad_list(matches, cap):
    """int [k, 4] -> int32 [cap, 4]: clipped to cap, the rest -7 (never read)"""
    out = np.full((cap, 4), -7, np.int32)
    k = min(len(matches), cap)
    out[:k] = matches[:k]
    return out


def carry(L, fmap, matches, n, corr_cap, min_matches=0, width=fr.W, height=fr.H):
    """matches int32 [cap, 4] -> dict as frame_tracking_ref.carry gives it; the arrays are [corr_cap] / [cap], 255 / -7
    where nothing was written"""
    m, keep = _c_map(fmap)
    matches = np.ascontiguousarray(matches, np.int32)
    cap, n_cur = len(matches), len(fmap["cur_key"])
    o = dict(n_map=np.full(1, -7, np.int32), map=np.full((corr_cap, 4), -7, np.int32), carry_status=np.full(cap, 255, np.uint8),
             cur_status=np.full(n_cur, 255, np.uint8), corr_p3d=np.full((corr_cap, 3), -7, np.float32),
             corr_p2d=np.full((corr_cap, 2), -7, np.float32), corr_point=np.full(corr_cap, -7, np.int32))
    o["status"] = L.frame_tracking_host_carry(C.byref(m), width, height, matches.ctypes.data, cap, int(n), min_matches, corr_cap,
                                              *[o[k].ctypes.data for k in ("n_map", "map", "carry_status", "cur_status",
                                                                           "corr_p3d", "corr_p2d", "corr_point")])
    return o


def cut(L, fmap, carried, outliers, min_map_matches):
    """Steps 5-6 on the dict `carried` that carry() returned (its map gets the flags) -> dict of the cut's outputs"""
    m, keep = _c_map(fmap)
    n_map = int(carried["n_map"][0])
    cap = max(len(carried["map"]), 1)
    out = np.ascontiguousarray(np.asarray(outliers, np.uint8).reshape(-1))
    assert len(out) >= n_map
    o = dict(n_kept=np.zeros(1, np.int32), kept_key=np.full(cap, -7, np.int32), kept_point=np.full(cap, -7, np.int32),
             n_removed=np.zeros(1, np.int32), removed=np.full((cap, 2), -7, np.int32), n_matches_map=np.zeros(1, np.int32))
    o["track_status"] = L.frame_tracking_host_cut(C.byref(m), carried["status"], n_map, carried["map"].ctypes.data,
                                                  out.ctypes.data, min_map_matches,
                                                  *[o[k].ctypes.data for k in ("n_kept", "kept_key", "kept_point", "n_removed",
                                                                               "removed", "n_matches_map")])
    return o


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def check_carry(got, ref, label=""):
    """a build's carry outputs (numpy or CUDA tensors; `got["status"]` or track_status) against frame_tracking_ref.carry,
    exactly; what the reference does not write must be untouched (the arrays were filled with 255 / -7)"""
    status = got["status"] if "status" in got else int(_np(got["track_status"]).reshape(-1)[0])
    assert status == ref["status"], (label, status, ref["status"])
    if ref["status"] < 0:
        for k in ("n_map", "map", "carry_status", "cur_status", "corr_p3d", "corr_p2d", "corr_point"):
            a = _np(got[k])
            assert (a == (255 if a.dtype == np.uint8 else -7)).all(), (label, k)
        return
    n = ref["n_map"]
    assert int(_np(got["n_map"]).reshape(-1)[0]) == n, label
    assert np.array_equal(_np(got["map"])[:n], ref["map"]), label
    assert np.array_equal(_np(got["carry_status"]), ref["carry_status"]), label       # 255 beyond the list: untouched
    assert np.array_equal(_np(got["cur_status"]), ref["cur_status"]), label
    assert np.array_equal(_np(got["corr_point"])[:n], ref["corr_point"]), label
    assert np.array_equal(_np(got["corr_p2d"])[:n], ref["corr_p2d"]), label
    assert _np(got["corr_p3d"])[:n].tobytes() == ref["corr_p3d"].tobytes(), label
    for k in ("map", "corr_p3d", "corr_p2d", "corr_point"):                               # untouched beyond n_map
        assert (_np(got[k])[n:] == -7).all(), (label, k)


def check_cut(got, ref, label=""):
    """a build's cut outputs against frame_tracking_ref.order_independent run on the same outlier bytes, exactly"""
    first = lambda k: int(_np(got[k]).reshape(-1)[0])
    assert first("track_status") == ref["track_status"], (label, first("track_status"), ref["track_status"])
    assert (first("n_kept"), first("n_removed"), first("n_matches_map")) == (ref["n_kept"], ref["n_removed"], ref["n_matches_map"]), label
    assert np.array_equal(_np(got["kept_key"])[:ref["n_kept"]], ref["kept_key"]), label
    assert np.array_equal(_np(got["kept_point"])[:ref["n_kept"]], ref["kept_point"]), label
    assert np.array_equal(_np(got["removed"])[:ref["n_removed"]], ref["removed"]), label
    if "map" in got:
        assert np.array_equal(_np(got["map"])[:ref["n_map"]], ref["map"]), label      # with the flags
