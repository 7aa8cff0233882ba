"""GPU: the four geometry host entry points (msf_pnp_ransac, msf_pose_optimize, msf_new_points, msf_reconstruct) asked
for subsets of their result arrays, through _lib directly (the matcher wrappers always ask for everything).  An array
nobody asks for gets no piece of the workspace and a null pointer in the kernel (csrc/result_arrays.h), so: one call
with every array, then one with the required pointer alone and one per further array on its own; whatever comes back
must equal the all-arrays call bit for bit.  Every buffer is its documented extent plus a canary tail that must come
back intact."""
import ctypes as C

import numpy as np
import pytest

from mono_slam_framework_amd import _lib
from tests import initializer_ref as ir
from tests import local_mapping_ref as lm
from tests import pnp_ref
from tests import pose_ref

pytestmark = pytest.mark.gpu

CANARY, TAIL = 0xA5, 64


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.7, 640, 480)
    yield m
    m.close()


def _list_shapes(arrays, cap):
    return {name: ((1,) + tuple(cap if t == "cap" else t for t in tail), dt) for name, dt, _, tail in arrays}


def _call(struct, shapes, names, invoke):
    """One call that asks for `names`: each in a buffer of its documented bytes + TAIL, all of it CANARY beforehand.
    -> (status, {name: the documented bytes})"""
    size = {k: int(np.prod(shapes[k][0])) * np.dtype(shapes[k][1]).itemsize for k in names}
    bufs = {k: np.full(size[k] + TAIL, CANARY, np.uint8) for k in names}
    res = struct(struct_size=C.sizeof(struct))
    for k in names:
        setattr(res, k, bufs[k].ctypes.data)
    rc = invoke(res)
    for k in names:
        assert (bufs[k][size[k]:] == CANARY).all(), "%s: written beyond its documented extent" % k
    return rc, {k: bufs[k][:size[k]].copy() for k in names}


def _subsets_equal_the_whole(label, struct, arrays, shapes, required, invoke, ok=(_lib.MSF_OK,)):
    names = [a[0] for a in arrays]
    rc_all, whole = _call(struct, shapes, names, invoke)
    assert rc_all in ok, (label, rc_all)
    written = sum(int((whole[k] != CANARY).any()) for k in names)
    print("%s: status %d, %d of %d arrays written, %s = %s" % (label, rc_all, written, len(names), required,
                                                               whole[required].view(np.int32).tolist()))
    for subset in [[required]] + [[required, k] for k in names if k != required]:
        rc, got = _call(struct, shapes, subset, invoke)
        assert rc == rc_all, (label, subset, rc)
        for k in subset:
            assert got[k].tobytes() == whole[k].tobytes(), "%s: %s alone differs from the all-arrays call" % (label, k)
    return whole


def test_pnp_with_drawn_and_with_given_sets(fm):
    n, its, recs = 6, 8, 2
    sc = pnp_ref.scene("base", 2, n)
    p3, p2 = np.ascontiguousarray(sc["p3d"], np.float32), np.ascontiguousarray(sc["p2d"], np.float32)
    prm = fm._pnp_params(sc["K"], 5.991, 4, its, recs, 7)
    shapes = _lib.pnp_shapes(1, its, recs, n)
    ok = (_lib.MSF_OK, _lib.MSF_ERR_CAPACITY)   # more than two records is no failure: the first two are complete

    def drawn(res):
        return fm._L.msf_pnp_ransac(fm._h, n, p3.ctypes.data, p2.ctypes.data, C.byref(prm), None, C.byref(res))

    whole = _subsets_equal_the_whole("pnp, drawn sets", _lib.PnpResult, _lib.PNP_ARRAYS, shapes, "n_records", drawn, ok)
    sets = np.ascontiguousarray(whole["sets"].view(np.int32).reshape(its, 4))
    assert sets.min() >= 0 and sets.max() < n

    def given(res):
        return fm._L.msf_pnp_ransac(fm._h, n, p3.ctypes.data, p2.ctypes.data, C.byref(prm), sets.ctypes.data, C.byref(res))

    again = _subsets_equal_the_whole("pnp, given sets", _lib.PnpResult, _lib.PNP_ARRAYS, shapes, "n_records", given, ok)
    assert (again["sets"] == CANARY).all()   # sets come back only when they were drawn here
    for k in whole:
        if k != "sets":
            assert again[k].tobytes() == whole[k].tobytes(), k


@pytest.mark.parametrize("masked", (False, True))
def test_pose_with_and_without_a_mask(fm, masked):
    n = 8
    sc = pose_ref.scene("base", 1, n)
    p3, p2 = np.ascontiguousarray(sc["p3d"], np.float32), np.ascontiguousarray(sc["p2d"], np.float32)
    t0 = np.ascontiguousarray(sc["Tcw0"], np.float32)
    mask = np.array([1, 1, 0, 1, 1, 1, 0, 1], np.uint8)
    prm = fm._pose_params(sc["K"], 5.991)

    def invoke(res):
        return fm._L.msf_pose_optimize(fm._h, n, p3.ctypes.data, p2.ctypes.data, t0.ctypes.data,
                                       mask.ctypes.data if masked else None, C.byref(prm), C.byref(res))

    whole = _subsets_equal_the_whole("pose, mask %s" % masked, _lib.PoseResult, _lib.POSE_ARRAYS, _lib.pose_shapes(1, n),
                                     "n_good", invoke)
    if masked:   # an outlier byte outside the mask stays as the caller had it
        assert (whole["outliers"][mask == 0] == CANARY).all() and (whole["outliers"][mask != 0] <= 1).all()


def test_new_points(fm):
    v1, v2, m = lm.handmade()
    n = len(m)
    assert n == 3
    m = np.ascontiguousarray(m, np.int32)
    a1, a2 = fm.make_views(v1), fm.make_views(v2)
    prm = fm._new_points_params(1.1, lm.CHI2)

    def invoke(res):
        return fm._L.msf_new_points(fm._h, n, m.ctypes.data, a1.ctypes.data, a2.ctypes.data, C.byref(prm), C.byref(res))

    whole = _subsets_equal_the_whole("new points", _lib.NewPointsResult, _lib.NEW_POINTS_ARRAYS,
                                     _list_shapes(_lib.NEW_POINTS_ARRAYS, n), "n_new", invoke)
    assert whole["n_new"].view(np.int32)[0] == 1 and list(whole["status"]) == [3, 1, 0]


def test_reconstruct_from_eight_inliers_of_one_model(fm):
    c = ir.case("planar", 3)
    keep = np.flatnonzero(c["H"]["inliers"])[:8]
    m = np.ascontiguousarray(c["matches"][keep], np.int32)
    inl = np.ones(8, np.uint8)
    m21 = np.ascontiguousarray(c["H"]["m21"], np.float32).reshape(9)
    prm = fm._motion_params(ir.K, ir.SIGMA, 0, ir.MIN_PARALLAX)

    def invoke(res):
        return fm._L.msf_reconstruct(fm._h, 0, m21.ctypes.data, 8, m.ctypes.data, inl.ctypes.data, C.byref(prm),
                                     C.byref(res))

    whole = _subsets_equal_the_whole("reconstruct", _lib.MotionResult, _lib.MOTION_ARRAYS,
                                     _list_shapes(_lib.MOTION_ARRAYS, 8), "ok", invoke)
    assert whole["n_cand"].view(np.int32)[0] == 8   # the homography's eight candidates went through CheckRT
