"""GPU: msf_create_map_points -- the loop of LocalMapping::CreateNewMapPoints in one call: the stored query frame
matched against its stored neighbours (the launch sequence of msf_match_one_to_many) and every list triangulated by
k_new_points directly behind it.  Counts and lists equal msf_match_one_to_many's, the new points equal msf_new_points
run on those lists bit for bit, the geometry convention puts the points of a fronto-parallel plane at its depth, and the
refusals are those of the documentation.  Once on an ORB handle, once on a LoFTR handle."""
import ctypes as C

import numpy as np
import pytest

from tests import initializer_ref as ir
from tests import local_mapping_ref as lm

pytestmark = pytest.mark.gpu

W, H = 640, 480
PLANE_Z = 5.0
SHIFTS = ((12, 0), (-20, 6), (8, -16), (24, 10), (-6, -22))


def plane_view(dx, dy):
    """Frame b of synth_pair shows the canvas from (dx, dy) further right / down: a feature at (x, y) of the query sits
    at (x - dx, y - dy).  For the plane z = PLANE_Z in front of an identity query view that is a camera translated by
    tcw = (-dx, -dy, 0) * PLANE_Z / f."""
    f = float(ir.K[0, 0])
    return lm.make_view(np.eye(3), np.array([-dx, -dy, 0.0]) * PLANE_Z / f)


def check_against_two_calls(fm, frames, views, cap, label, want_depth):
    qv = lm.make_view(np.eye(3), np.zeros(3))
    for i, f in enumerate(frames):
        fm.store_frame(i, f)
    slots = list(range(1, len(frames)))
    v = np.array(views, lm.VIEW_DTYPE)
    num, lists, new = fm.create_map_points(0, qv, slots, v, cap=cap, diagnostics=True)
    num2, _, lists2 = fm.match_one_to_many(0, slots, cap=cap)
    # ORB: every neighbour shares texture with the query.  LoFTR on the repeating pattern matches only some shifts
    # (measured: 41, 42 and 1 matches for (32, 16), (16, 0), (-16, 8)); an empty list in the batch is a case of its own
    assert np.array_equal(num, num2) and (num >= 0).all(), (num, num2)
    assert (num > 0).all() if want_depth else (num > 0).sum() >= 2, num
    near_plane = 0
    for i in range(len(slots)):
        assert np.array_equal(lists[i], lists2[i])
        two = fm.new_points(lists2[i], qv, v[i])
        for k in ("status", "points", "hom", "cos_parallax", "packed"):
            assert np.ascontiguousarray(new[i][k]).tobytes() == np.ascontiguousarray(two[k]).tobytes(), (label, i, k)
        assert new[i]["n_new"] == two["n_new"] == int((two["status"] == 0).sum())
        z = new[i]["packed"]["z"]
        good = int((np.abs(z - PLANE_Z) <= 0.05 * PLANE_Z).sum())
        print("%s neighbour %d: %d matches, %d new points, %d within 5 %% of the plane's depth"
              % (label, i, len(lists[i]), new[i]["n_new"], good))
        near_plane = max(near_plane, good)
    if want_depth:
        assert near_plane >= 20
    return num, lists, new


@pytest.fixture(scope="module")
def orb():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.8, W, H, max_batch_pairs=8)
    yield m
    m.close()


@pytest.fixture(scope="module")
def orb_frames():
    from mono_slam_framework_amd import synth
    frames = [synth.synth_pair(3, W, H, shift=(0, 0))[0]]
    for s in SHIFTS:
        a, b = synth.synth_pair(3, W, H, shift=s)
        assert np.array_equal(a, frames[0])
        frames.append(b)
    return frames


def test_orb_create_map_points_equals_the_two_call_path(orb, orb_frames):
    views = [plane_view(*s) for s in SHIFTS]
    check_against_two_calls(orb, orb_frames, views, 2048, "orb", want_depth=True)


def test_small_capacity_triangulates_what_it_delivers(orb, orb_frames):
    """cap_per_pair below the lists' lengths: the first cap matches are delivered, and exactly those are triangulated"""
    qv = lm.make_view(np.eye(3), np.zeros(3))
    v = np.array([plane_view(*s) for s in SHIFTS], lm.VIEW_DTYPE)
    for i, f in enumerate(orb_frames):
        orb.store_frame(i, f)
    num, lists, new = orb.create_map_points(0, qv, [1, 2, 3, 4, 5], v, cap=70)
    num2, _, lists2 = orb.match_one_to_many(0, [1, 2, 3, 4, 5], cap=70)
    assert np.array_equal(num, num2) and (num > 70).all()
    for i in range(5):
        assert len(lists[i]) == 70 and np.array_equal(lists[i], lists2[i])
        two = orb.new_points(lists[i], qv, v[i])
        assert new[i]["status"].tobytes() == two["status"].tobytes() and new[i]["packed"].tobytes() == two["packed"].tobytes()
        assert new[i]["points"].tobytes() == two["points"].tobytes()


def test_refusals(orb, orb_frames):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import MsfError
    qv = lm.make_view(np.eye(3), np.zeros(3))
    v = np.array([plane_view(*s) for s in SHIFTS], lm.VIEW_DTYPE)
    for i, f in enumerate(orb_frames):
        orb.store_frame(i, f)
    num, lists, new = orb.create_map_points(0, qv, [], v[:0])                       # n = 0: no error, nothing
    assert len(num) == 0 and lists == [] and new == []
    with pytest.raises(MsfError) as e:
        orb.create_map_points(0, qv, [1, 16], v[:2])
    assert e.value.code == _lib.MSF_ERR_INVALID_ARG and "msf_create_map_points: bad slot" in str(e.value)
    with pytest.raises(MsfError) as e:
        orb.create_map_points(-1, qv, [1], v[:1])
    assert e.value.code == _lib.MSF_ERR_INVALID_ARG and "bad query slot" in str(e.value)
    with pytest.raises(MsfError) as e:
        orb.create_map_points(0, qv, list(range(9)), np.repeat(v[:1], 9))
    assert "n exceeds max_batch_pairs" in str(e.value)
    # a wrong struct_size, through the raw entry point
    L, h = orb._L, orb._h
    slots, n_new, num = np.array([1], np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    q = orb.make_views(np.array([qv]))
    prm = _lib.NewPointsParams(struct_size=C.sizeof(_lib.NewPointsParams), max_cos_parallax=1.1, chi2=lm.CHI2)
    res = _lib.NewPointsResult(struct_size=C.sizeof(_lib.NewPointsResult) - 8, n_new=n_new.ctypes.data)
    args = (h, 0, q.ctypes.data, 1, slots.ctypes.data, v.ctypes.data)
    assert L.msf_create_map_points(*args, C.byref(prm), num.ctypes.data, None, 64, C.byref(res)) == _lib.MSF_ERR_INVALID_ARG
    assert "struct_size" in orb.last_error()
    res.struct_size = C.sizeof(_lib.NewPointsResult)
    assert L.msf_create_map_points(*args, C.byref(prm), num.ctypes.data, None, 0, C.byref(res)) == _lib.MSF_ERR_INVALID_ARG
    assert L.msf_create_map_points(*args, C.byref(prm), num.ctypes.data, None, 64, C.byref(res)) == _lib.MSF_OK
    assert num[0] > 0 and 0 <= n_new[0] <= min(num[0], 64)
    fresh_cls = type(orb)
    fresh = fresh_cls(0.8, W, H, max_batch_pairs=2)
    try:
        with pytest.raises(MsfError) as e:
            fresh.create_map_points(0, qv, [1], v[:1])
        assert "msf_create_map_points: no frame was stored" in str(e.value)
    finally:
        fresh.close()


def test_loftr_create_map_points_equals_the_two_call_path():
    """the same on a LoFTR handle at 640 x 480 (the coarse-grid matches of the repeating test pattern say nothing about
    depth: lists and points only)"""
    from mono_slam_framework_amd import synth
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    shifts = ((0, 0), (32, 16), (16, 0), (-16, 8), (16, 16), (0, 16))
    frames = [synth.kat_pattern(W, H, sx, sy) for sx, sy in shifts]
    dm = DNNFeatureMatcher(threshold=0.15, image_width=W, image_height=H, max_batch_pairs=5)
    try:
        views = [plane_view(*s) for s in shifts[1:]]
        check_against_two_calls(dm, frames, views, 4096, "loftr", want_depth=False)
    finally:
        dm.close()
