"""CPU: mono_slam_framework_amd/results.py -- the one place that says how a result dict of the geometry calls is laid
out -- against what the wrappers returned before there was such a place.  No GPU and no libmsf.so.  The expected values
are frozen: tests/test_binding_results.json holds what _lib.pnp_shapes(3, 5, 2, 7), pose_shapes(3, 7), ba_shapes(2, 5,
9, 20) and tracking_shapes(table, 6, 3, 7, 25) returned at the commit before the layer; the motion, new-points and
RANSAC shapes below are read off that commit's reconstruct_device, new_points_device and find_models_device."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from mono_slam_framework_amd import _lib, results
from tests import ba_host

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_binding_results.json")) as f:
    FROZEN = {family: [(name, tuple(shape), dt if isinstance(dt, str) else np.dtype([tuple(x) for x in dt]))
                       for name, shape, dt in rows] for family, rows in json.load(f).items()}
CPU = torch.device("cpu")
N_HYP = 5


def motion_rows(L, cap):
    i32, f32 = "int32", "float32"
    return [("ok", (L,), i32), ("model", (L,), i32), ("R21", (L, 3, 3), f32), ("t21", (L, 3), f32),
            ("points", (L, cap, 3), f32), ("triangulated", (L, cap), "uint8"), ("n_cand", (L,), i32),
            ("cand_R", (L, 8, 3, 3), f32), ("cand_t", (L, 8, 3), f32), ("cand_good", (L, 8), i32),
            ("cand_parallax", (L, 8), f32), ("winner", (L,), i32)]


def new_points_rows(L, cap):
    return [("n_new", (L,), "int32"), ("packed", (L, cap), _lib.NEW_POINT_DTYPE), ("status", (L, cap), "uint8"),
            ("points", (L, cap, 3), "float32"), ("hom", (L, cap, 4), "float32"), ("cos_parallax", (L, cap), "float64")]


def ransac_rows(L, cap, own):
    f32 = "float32"
    return [("m21", (L, N_HYP, 3, 3), f32), ("null_vec", (L, N_HYP, 3, 3), f32), ("scores", (L, N_HYP), f32),
            ("best", (L,), "int32"), ("best_inliers", (L, cap), "uint8"), ("T1", (L, 3, 3), f32), ("T2", (L, 3, 3), f32),
            (own, (L, N_HYP, 3, 3), f32)]


def check_layout(d, rows, device, flat=()):
    """d: what the allocator made; rows: (name, shape, dtype) as the host has them"""
    assert list(d) == [r[0] for r in rows]
    for name, shape, dt in rows:
        a = d[name]
        if name in flat:
            shape = (int(np.prod(shape)),)
        if device is None:
            assert isinstance(a, np.ndarray) and a.shape == shape and a.dtype == np.dtype(dt), name
        else:   # a record of four 4-byte fields is int32 [..., 4] on a device
            if np.dtype(dt).fields:
                shape, dt = shape + (4,), "int32"
            assert a.device == device and tuple(a.shape) == shape and a.dtype == getattr(torch, dt), name
            assert a.is_contiguous()
        assert not np.asarray(a).view(np.uint8).any() or name == "best", name


def test_the_shape_functions_return_what_they_returned():
    got = {"pnp": _lib.pnp_shapes(3, 5, 2, 7), "pose": _lib.pose_shapes(3, 7), "ba": _lib.ba_shapes(2, 5, 9, 20),
           "frustum": _lib.tracking_shapes(_lib.FRUSTUM_ARRAYS, points=6, kfs=3, cap=7, corr_cap=25),
           "claim": _lib.tracking_shapes(_lib.CLAIM_ARRAYS, points=6, kfs=3, cap=7, corr_cap=25)}
    assert set(got) == set(FROZEN)
    for family, rows in FROZEN.items():
        assert [(k, s, dt) for k, (s, dt) in got[family].items()] == rows, family


@pytest.mark.parametrize("device", (None, CPU), ids=("numpy", "torch-cpu"))
def test_allocator_layout_of_the_frozen_tables(device):
    shapes = {family: {name: (shape, dt) for name, shape, dt in rows} for family, rows in FROZEN.items()}
    for family, rows in FROZEN.items():
        flat = ("claims",) if family == "claim" else ()
        check_layout(results.alloc(shapes[family], device, flat=flat), rows, device, flat)
    claims = results.alloc(shapes["claim"], device, flat=("claims",))["claims"]
    assert tuple(claims.shape) == ((21,) if device is None else (21, 4))
    assert claims.dtype == (_lib.LOCAL_CLAIM_DTYPE if device is None else torch.int32)


@pytest.mark.parametrize("device", (None, CPU), ids=("numpy", "torch-cpu"))
@pytest.mark.parametrize("L", (1, 3))
@pytest.mark.parametrize("cap", (1, 7))
def test_allocator_layout_of_motion_new_points_and_ransac(device, L, cap):
    check_layout(results.alloc(_lib.list_shapes(_lib.MOTION_ARRAYS, L, cap), device), motion_rows(L, cap), device)
    d = results.alloc(_lib.list_shapes(_lib.NEW_POINTS_ARRAYS, L, cap), device)
    check_layout(d, new_points_rows(L, cap), device)
    assert tuple(d["packed"].shape) == ((L, cap) if device is None else (L, cap, 4))
    both = results.alloc_ransac(_lib.ransac_shapes(L, N_HYP, cap), device)
    assert list(both) == ["H", "F"]
    for model, own, other in (("H", "m12", "fn"), ("F", "fn", "m12")):
        check_layout(both[model], ransac_rows(L, cap, own), device)
        assert other not in both[model]
        best = np.asarray(both[model]["best"])
        assert best.shape == (L,) and (best == -1).all()
    assert [f[0] for f in _lib.RansacResult._fields_[2:]] == [a[0] for a in _lib.RANSAC_ARRAYS] \
        == ["m21", "m12", "fn", "null_vec", "scores", "best", "best_inliers", "T1", "T2"]


def test_subsets_are_those_the_wrappers_asked_for():
    names = {family: [r[0] for r in rows] for family, rows in FROZEN.items()}
    expect = {"pnp": ["n_records", "counts", "iteration", "n_inliers", "refined_ok", "n_refined", "Tcw_best",
                      "Tcw_refined", "inliers_best", "inliers_refined"],
              "pose": ["n_good", "Tcw", "outliers", "n_edges", "rounds_run", "pose_f64"],
              "ba": ["status", "cam_Tcw", "points", "outliers", "cam_pose_f64", "points_f64", "round_flags",
                     "round_iterations"],
              "new_points": ["n_new", "packed", "status", "points"],
              "search": ["status_word", "n_claims", "n_claimed", "claims", "claim_status", "n_corr"]}
    tables = {"pnp": (_lib.PNP_ARRAYS, _lib.pnp_shapes(3, 5, 2, 7)), "pose": (_lib.POSE_ARRAYS, _lib.pose_shapes(3, 7)),
              "ba": (_lib.BA_ARRAYS, _lib.ba_shapes(2, 5, 9, 20)),
              "new_points": (_lib.NEW_POINTS_ARRAYS, _lib.list_shapes(_lib.NEW_POINTS_ARRAYS, 3, 7)),
              "search": (_lib.CLAIM_ARRAYS, _lib.tracking_shapes(_lib.CLAIM_ARRAYS, 6, 3, 7, 25))}
    for family, (table, shapes) in tables.items():
        assert list(results.alloc(shapes, leave_out=results.left_out(family, table))) == expect[family], family
        assert list(results.alloc(shapes, CPU, results.left_out(family, table))) == expect[family], family
        assert results.left_out(family, table, whole=True) == set()
        assert list(results.alloc(shapes, leave_out=results.left_out(family, table, True))) == [a[0] for a in table]
    # the per-record pnp arrays without rec_*, the pose "list" arrays, the ba units that do not start with "it"
    assert expect["pnp"] == [n for n in names["pnp"] if not n.startswith("rec_")][:10]
    assert expect["pose"] == [a[0] for a in _lib.POSE_ARRAYS if a[2] == "list"]
    assert expect["ba"] == [a[0] for a in _lib.BA_ARRAYS if not a[2].startswith("it")]


def test_fill_points_the_struct_at_the_arrays_given_and_at_nothing_else():
    d = results.alloc(_lib.pose_shapes(2, 5), leave_out=results.left_out("pose", _lib.POSE_ARRAYS))
    res = results.fill(_lib.PoseResult(), d)
    assert res.struct_size == C.sizeof(_lib.PoseResult) and res.reserved == 0
    for name, _, _, _ in _lib.POSE_ARRAYS:
        assert getattr(res, name) == (d[name].ctypes.data if name in d else None), name
    whole = results.alloc(_lib.ba_shapes(1, 3, 4, 6))
    res = results.fill(_lib.BaResult(), whole)
    assert res.struct_size == C.sizeof(_lib.BaResult)
    assert all(getattr(res, a[0]) == whole[a[0]].ctypes.data for a in _lib.BA_ARRAYS)
    with pytest.raises(AssertionError):   # a device form takes CUDA tensors only
        results.fill(_lib.PoseResult(), results.alloc(_lib.pose_shapes(2, 5), CPU))


def _arange(shapes):
    return {k: np.arange(int(np.prod(s)), dtype=np.float64).reshape(s).astype(dt) for k, (s, dt) in shapes.items()}


@pytest.mark.parametrize("diagnostics", (True, False))
def test_ba_host_view(diagnostics):
    nc, npt = 3, 4
    d = _arange(_lib.ba_shapes(1, nc, npt, 6))
    if not diagnostics:
        d = {k: v for k, v in d.items() if not k.startswith("it_")}
    expect = dict(d)
    expect["status"] = int(d["status"][0])
    expect["round_iterations"] = d["round_iterations"][0]
    if diagnostics:
        for k in ("it_trials", "it_lambda_in", "it_lambda_out", "it_cost_in", "it_cost_out"):
            expect[k] = d[k][0]
        for k in ("it_cam_in", "it_cam_out", "it_Hcc", "it_bc"):
            expect[k] = d[k].reshape((64, nc) + d[k].shape[1:])
        for k in ("it_point_in", "it_point_out", "it_Hpp", "it_bp"):
            expect[k] = d[k].reshape((64, npt) + d[k].shape[1:])
    for got in (results.view_ba(d, _lib.BA_ARRAYS, _lib.BA_SLOTS, nc, npt), ba_host.shape_result(d, nc, npt)):
        assert list(got) == list(expect) and type(got["status"]) is int
        for k, v in expect.items():
            assert np.shape(got[k]) == np.shape(v) and np.array_equal(got[k], v), k
    assert expect["round_iterations"].shape == (2,)
    if diagnostics:
        assert expect["it_trials"].shape == (64,) and expect["it_Hcc"].shape == (64, 3, 21) and expect["it_bp"].shape == (64, 4, 3)


def _same(got, expect):
    assert list(got) == list(expect)
    for k, v in expect.items():
        assert type(got[k]) is type(v), k
        if isinstance(v, np.ndarray):
            assert got[k].dtype == v.dtype and got[k].shape == v.shape and np.array_equal(got[k], v), k
        else:
            assert got[k] == v, k


@pytest.mark.parametrize("n", (0, 3))
def test_host_views_cut_and_convert(n):
    rows = max(n, 1)   # a host form allocates max(n, 1) rows
    d = _arange(_lib.list_shapes(_lib.MOTION_ARRAYS, 1, rows))
    expect = {k: v[0] for k, v in d.items()}
    for k in ("ok", "model", "n_cand", "winner"):
        expect[k] = int(d[k][0])
    expect["points"], expect["triangulated"] = d["points"][0, :n], d["triangulated"][0, :n].astype(bool)
    _same(results.view_motion(d, n), expect)
    assert expect["R21"].shape == (3, 3) and expect["cand_R"].shape == (8, 3, 3) and expect["points"].shape == (n, 3)

    d = results.alloc(_lib.list_shapes(_lib.NEW_POINTS_ARRAYS, 1, rows))
    d["n_new"][0] = n - 1   # -1: packed is cut to nothing
    d["status"][0], d["cos_parallax"][0] = np.arange(rows), np.arange(rows)
    d["packed"]["match"][0] = np.arange(rows)
    expect = dict(n_new=n - 1, packed=d["packed"][0, :max(n - 1, 0)], status=d["status"][0, :n], points=d["points"][0, :n],
                  hom=d["hom"][0, :n], cos_parallax=d["cos_parallax"][0, :n])
    _same(results.view_new_points(d, n), expect)
    del d["hom"], d["cos_parallax"], expect["hom"], expect["cos_parallax"]
    _same(results.view_new_points(d, n), expect)

    its, recs = 5, 4
    for records in (-1, 2, 9):   # 9: more than max_records, the first max_records are kept
        d = _arange(_lib.pnp_shapes(1, its, recs, rows))
        d["n_records"][0] = records
        kept = min(max(records, 0), recs)
        expect = {"n_records": records}
        for name, _, per, _ in _lib.PNP_ARRAYS[1:]:
            expect[name] = d[name][0, :kept] if per == "rec" else d[name][0]
        expect["inliers_best"], expect["inliers_refined"] = expect["inliers_best"][:, :n], expect["inliers_refined"][:, :n]
        _same(results.view_pnp(d, _lib.PNP_ARRAYS, n, recs), expect)
        assert expect["inliers_best"].shape == (kept, n) and expect["counts"].shape == (its,)

    for diagnostics in (True, False):
        d = _arange(_lib.pose_shapes(1, rows))
        if not diagnostics:
            d = {k: d[k] for k in ("n_good", "Tcw", "outliers", "n_edges", "rounds_run", "pose_f64")}
        expect = {k: v[0] for k, v in d.items()}
        for k in ("n_good", "n_edges", "rounds_run"):
            expect[k] = int(d[k][0])
        expect["outliers"] = d["outliers"][0, :n]
        _same(results.view_pose(d, n), expect)

    both = results.alloc_ransac(_lib.ransac_shapes(1, N_HYP, rows))
    for model, own in (("H", "m12"), ("F", "fn")):
        d = both[model]
        d["best_inliers"][0, ::2] = 1
        got = results.view_ransac(d, n)
        expect = {k: v[0] for k, v in d.items()}
        expect["best"], expect["best_inliers"] = -1, d["best_inliers"][0, :n].astype(bool)
        _same(got, expect)
        assert list(got)[-1] == own and got["m21"].shape == (N_HYP, 3, 3) and got["T1"].shape == (3, 3)
