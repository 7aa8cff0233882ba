"""GPU: k_new_points (csrc/triangulate_kernels.hip) through msf_new_points_device / msf_new_points -- the loop body of
LocalMapping::CreateNewMapPoints -- against the float64 reference of tests/local_mapping_ref.py, step by step (cosine,
null vector, division, the checks from the device's own point, status end to end, the packed records); the shapes at
which the chunked scan can go wrong; inputs on which a loop must still end."""
import ctypes as C

import numpy as np
import pytest

from tests import local_mapping_ref as lm

pytestmark = pytest.mark.gpu

SENTINEL_U8 = 0xAB
SENTINEL_F = np.float32(-12345.5)
KEYS = ("n_new", "packed", "status", "points", "hom", "cos_parallax")


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.7, 640, 480)
    yield m
    m.close()


def _views(v):
    import torch
    v = np.ascontiguousarray(np.asarray(v, lm.VIEW_DTYPE).reshape(-1))
    return torch.from_numpy(v.view(np.uint8).reshape(len(v), 64).copy()).cuda()


def _sentinel_out(L, cap):
    import torch
    return dict(n_new=torch.full((L,), -77, dtype=torch.int32, device="cuda"),
                packed=torch.full((L, cap, 4), -77, dtype=torch.int32, device="cuda"),
                status=torch.full((L, cap), SENTINEL_U8, dtype=torch.uint8, device="cuda"),
                points=torch.full((L, cap, 3), float(SENTINEL_F), dtype=torch.float32, device="cuda"),
                hom=torch.full((L, cap, 4), float(SENTINEL_F), dtype=torch.float32, device="cuda"),
                cos_parallax=torch.full((L, cap), float(SENTINEL_F), dtype=torch.float64, device="cuda"))


def run_device(fm, lists, n_out, v1, v2, cap, max_cos=1.1):
    """lists: [L] of int32 [k, 4] (k <= cap rows are stored) -> dict of numpy arrays, outputs pre-filled with sentinels"""
    import torch
    L = len(lists)
    m = np.zeros((L, cap, 4), np.int32)
    for i, l in enumerate(lists):
        m[i, :len(l)] = l
    d_m = torch.from_numpy(m).cuda()
    d_n = torch.tensor(list(n_out), dtype=torch.int32, device="cuda")
    out = fm.new_points_device(d_m, d_n, _views(v1), _views(v2), max_cos, lm.CHI2, out=_sentinel_out(L, cap))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["packed"] = np.ascontiguousarray(got["packed"]).view(lm_packed()).reshape(L, cap)
    return got


def lm_packed():
    from mono_slam_framework_amd import _lib
    return _lib.NEW_POINT_DTYPE


def one_list(got, i, n):
    n_new = int(got["n_new"][i])
    return dict(n_new=n_new, packed=got["packed"][i, :max(n_new, 0)], status=got["status"][i, :n],
                points=got["points"][i, :n], hom=got["hom"][i, :n], cos_parallax=got["cos_parallax"][i, :n])


def assert_untouched_beyond(got, i, n, n_new):
    assert (got["status"][i, n:] == SENTINEL_U8).all()
    assert (got["points"][i, n:] == SENTINEL_F).all() and (got["hom"][i, n:] == SENTINEL_F).all()
    assert (got["cos_parallax"][i, n:] == float(SENTINEL_F)).all()
    assert (got["packed"][i, max(n_new, 0):].view(np.int32) == -77).all()


def same_bits(a, b):
    for k in ("status", "points", "hom", "cos_parallax", "packed"):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert int(a["n_new"]) == int(b["n_new"])


# ---- 1. against float64, per step ----
@pytest.mark.parametrize("seed,max_cos", lm.CASES)
def test_device_meets_the_float64_bars(fm, seed, max_cos):
    view1, views2, matches = lm.scene(seed)
    refs = lm.scene_reference(seed, max_cos)
    cap = lm.N_MATCHES + 64            # a stride that is not the length
    got = run_device(fm, list(matches), [lm.N_MATCHES] * lm.N_NEIGHBOURS, [view1] * lm.N_NEIGHBOURS, views2, cap, max_cos)
    worst = 0.0
    for i in range(lm.N_NEIGHBOURS):
        g = one_list(got, i, lm.N_MATCHES)
        w, _ = lm.check_result(refs[i], g, matches[i], view1, views2[i], max_cos,
                               label="device seed %d max_cos %g list %d" % (seed, max_cos, i))
        worst = max(worst, w)
        assert_untouched_beyond(got, i, lm.N_MATCHES, g["n_new"])
    print("device seed %d max_cos %g: null vector worst err / bound %.3f" % (seed, max_cos, worst))


def test_handmade_matches(fm):
    v1, v2, m = lm.handmade()
    got = fm.new_points(m, v1, v2)
    lm.check_result(lm.handmade_reference(), got, m, v1, v2, label="device handmade")
    assert list(got["status"]) == [3, 1, 0]
    assert got["hom"][0, 3] == 0 and abs(got["hom"][0, 2]) == 1
    assert np.allclose(got["points"][2], [0.5, 0.0, 5.0], atol=1e-5)


# ---- 2. shapes ----
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 513)
CAP = 600


@pytest.fixture(scope="module")
def shaped(fm):
    """the lists of the shape test, cut from scene 1: list j holds LENGTHS[j] matches of neighbour j % 8 (tiled where
    the length exceeds 320), then one list of 600 matches that claims 700, then one that claims -1"""
    view1, views2, matches = lm.scene(1)
    lists, n_out, v2 = [], [], []
    for j, n in enumerate(LENGTHS + (CAP, CAP)):
        k = j % lm.N_NEIGHBOURS
        lists.append(np.tile(matches[k], (2, 1))[:n].copy())
        v2.append(views2[k])
        n_out.append(n)
    n_out[-2], n_out[-1] = 700, -1
    got = run_device(fm, lists, n_out, [view1] * len(lists), v2, CAP)
    return dict(view1=view1, lists=lists, n_out=n_out, v2=v2, got=got)


def test_list_lengths_around_the_chunk_and_wave_sizes(fm, shaped):
    got, L = shaped["got"], len(shaped["lists"])
    for j in range(L):
        claimed = shaped["n_out"][j]
        if claimed < 0:
            assert got["n_new"][j] == -1
            assert_untouched_beyond(got, j, 0, 0)
            continue
        n = min(claimed, CAP)
        g = one_list(got, j, n)
        ref = lm.new_points(shaped["lists"][j][:n], shaped["view1"], shaped["v2"][j])
        lm.check_result(ref, g, shaped["lists"][j][:n], shaped["view1"], shaped["v2"][j], label="length %d" % claimed)
        assert_untouched_beyond(got, j, n, g["n_new"])
    assert got["n_new"][0] == 0 and got["n_new"][-2] > 256


def test_lists_do_not_depend_on_their_neighbours_in_the_call(fm, shaped):
    got, L = shaped["got"], len(shaped["lists"])
    order = list(range(L))[::-1]
    rev = run_device(fm, [shaped["lists"][j] for j in order], [shaped["n_out"][j] for j in order],
                     [shaped["view1"]] * L, [shaped["v2"][j] for j in order], CAP)
    for pos, j in enumerate(order):
        n = max(min(shaped["n_out"][j], CAP), 0)
        same_bits(one_list(got, j, n), one_list(rev, pos, n))
        alone = run_device(fm, [shaped["lists"][j]], [shaped["n_out"][j]], [shaped["view1"]], [shaped["v2"][j]], CAP)
        same_bits(one_list(got, j, n), one_list(alone, 0, n))
        if shaped["n_out"][j] < 0:
            assert rev["n_new"][pos] == -1 and alone["n_new"][0] == -1


def test_every_list_equals_the_host_entry_point(fm, shaped):
    got = shaped["got"]
    for j, l in enumerate(shaped["lists"]):
        if shaped["n_out"][j] < 0:
            continue
        n = min(shaped["n_out"][j], CAP)
        host = fm.new_points(l[:n], shaped["view1"], shaped["v2"][j])
        same_bits(one_list(got, j, n), host)


# ---- 3. inputs that must not hang ----
def test_degenerate_inputs_end_with_a_status(fm):
    view1, views2, matches = lm.scene(2)
    bad = views2[1].copy()
    bad["Rcw"][4] = np.nan
    for v2, max_cos, label in ((view1, 1.1, "identical views"), (bad, 1.1, "NaN in Rcw"), (views2[0], 0.0, "max_cos = 0")):
        got = run_device(fm, [matches[0]], [lm.N_MATCHES], [view1], [v2], lm.N_MATCHES, max_cos)
        g = one_list(got, 0, lm.N_MATCHES)
        print("%s: status histogram %s" % (label, np.bincount(g["status"], minlength=8)))
        assert ((g["status"] >= 0) & (g["status"] <= 7)).all()
        assert g["n_new"] == int((g["status"] == 0).sum()) and np.isfinite(g["points"]).all()
        assert not g["points"][g["status"] != 0].any()
        if max_cos == 0.0:
            assert g["n_new"] == 0 and set(g["status"]) <= {1, 2}
        if label == "NaN in Rcw":
            assert g["n_new"] == 0


# ---- the refusals of msf_new_points / msf_new_points_device ----
def test_refusals_and_an_empty_list(fm):
    from mono_slam_framework_amd import _lib
    L, h = fm._L, fm._h
    INV = _lib.MSF_ERR_INVALID_ARG
    v1, v2, m = lm.handmade()
    v1, v2 = fm.make_views(np.array([v1])), fm.make_views(np.array([v2]))
    m = np.ascontiguousarray(m)
    n_new = np.full(1, -5, np.int32)

    def call(n=3, matches=m, prm_size=None, res_size=None, max_cos=1.1, chi2=lm.CHI2, n_new_ptr=True):
        prm = _lib.NewPointsParams(struct_size=C.sizeof(_lib.NewPointsParams) if prm_size is None else prm_size,
                                   max_cos_parallax=max_cos, chi2=chi2)
        res = _lib.NewPointsResult(struct_size=C.sizeof(_lib.NewPointsResult) if res_size is None else res_size)
        res.n_new = n_new.ctypes.data if n_new_ptr else None
        return L.msf_new_points(h, n, None if matches is None else matches.ctypes.data, v1.ctypes.data, v2.ctypes.data,
                                C.byref(prm), C.byref(res))

    assert call(prm_size=8) == INV and "struct_size" in fm.last_error()
    assert call(res_size=8) == INV and "struct_size" in fm.last_error()
    assert call(n_new_ptr=False) == INV and "n_new" in fm.last_error()
    assert call(n=-1) == INV and "negative" in fm.last_error()
    assert call(matches=None) == INV
    assert call(max_cos=float("nan")) == INV and "NaN" in fm.last_error()
    assert call(chi2=float("nan")) == INV
    assert call(n=0, matches=None) == _lib.MSF_OK and n_new[0] == 0
    assert call() == _lib.MSF_OK and n_new[0] == 1          # a good call after the refusals
    prm = _lib.NewPointsParams(struct_size=C.sizeof(_lib.NewPointsParams), max_cos_parallax=1.1, chi2=lm.CHI2)
    res = _lib.NewPointsResult(struct_size=C.sizeof(_lib.NewPointsResult))
    assert L.msf_new_points_device(h, 1, None, 8, None, None, None, C.byref(prm), C.byref(res), None) == INV
    res.n_new = n_new.ctypes.data
    assert L.msf_new_points_device(h, 70000, None, 8, None, None, None, C.byref(prm), C.byref(res), None) == INV
    assert "65535" in fm.last_error()
    assert L.msf_new_points_device(h, 1, None, 8, None, None, None, C.byref(prm), C.byref(res), None) == INV
    assert L.msf_new_points_device(h, 0, None, 8, None, None, None, C.byref(prm), C.byref(res), None) == _lib.MSF_OK
