"""GPU: msfx_track_frame -- TrackWithMotionModel / TrackReferenceKeyFrame in one call, once on an ORB and once on a
LoFTR handle with synthetic frames.  The count and the list equal msf_match_one_to_many on the two slots, and every
output equals msfx_track_list_device on that list bit for bit; with MSFX_TRACK_KEEP_ON_DEVICE the device pointers hold
the bytes of the copy-back, still do after a following msf_search_local_points, and msf_pose_optimize_device on the kept
correspondences gives the call's own pose; the refusals are those of the documentation."""
import ctypes as C

import numpy as np
import pytest

from tests import frame_tracking_host as fh
from tests import frame_tracking_ref as fr
from tests import tracking_ref as tr
from tests.test_create_map_points_gpu import H, W

pytestmark = pytest.mark.gpu

CAP = 2048


def frame_map_from_list(lst, prm, seed=0):
    """A train map with a point under the train end of every second match, placed where the current frame sees the
    query end of that match -- a carried point is a consistent correspondence for the pose -- and a current-frame map
    with an arbitrary point under the query end of every fifth match (replaced where the match carries one) and under
    a few pixels that no match ends on."""
    rng = np.random.default_rng(seed)
    R, t = prm["Rcw"].reshape(3, 3).astype(np.float64), prm["tcw"].astype(np.float64)
    seen_at = {}
    for (x1, y1, x2, y2) in lst[::2]:
        seen_at.setdefault(int(y2) * W + int(x2), (int(x1), int(y1)))
    pts = np.zeros(len(seen_at) + 1, tr.MAP_POINT)
    ref_key = np.array(sorted(seen_at), np.int32)
    for p, k in enumerate(ref_key):
        z = rng.uniform(2, 8)
        px, py = seen_at[int(k)]
        pc = np.array([(px - 320) / 500 * z, (py - 240) / 500 * z, z])
        pts["pos"][p] = (R.T @ (pc - t)).astype(np.float32)
    pts["pos"][-1] = (R.T @ (np.array([0.3, -0.2, 5.0]) - t)).astype(np.float32)
    cur = {int(y1) * W + int(x1): len(pts) - 1 for (x1, y1, _, _) in lst[::5]}
    used = set(int(m[1]) * W + int(m[0]) for m in lst)
    for k in rng.choice(W * H, 6, replace=False):
        if int(k) not in used:
            cur[int(k)] = len(pts) - 1
    observed = np.ones(len(pts), np.uint8)
    observed[::7] = 0
    return dict(points=pts, ref_key=ref_key, ref_point=np.arange(len(ref_key), dtype=np.int32),
                cur_key=np.array(sorted(cur), np.int32), cur_point=np.array([cur[k] for k in sorted(cur)], np.int32),
                observed=observed)


def peek(fm, address, dtype, count):
    """`count` elements at a device address, through the HIP runtime libmsf.so is linked against"""
    out = np.zeros(count, dtype)
    if count:
        fm._L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert fm._L.hipMemcpy(out.ctypes.data, address, out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return out


def check_track_frame(fm, frames, label, min_carried):
    import torch
    from mono_slam_framework_amd import _lib, results
    for i, f in enumerate(frames):
        fm.store_frame(i, f)
    num0, _, lists0 = fm.match_one_to_many(0, [1], cap=CAP)
    n = int(num0[0])
    assert n >= 15, (label, n)
    prm = tr.camera(1)
    fmap = frame_map_from_list(lists0[0], prm)
    Tcw0 = np.concatenate([prm["Rcw"].reshape(3, 3), prm["tcw"].reshape(3, 1)], 1).astype(np.float32).reshape(12)
    K = (float(prm["fx"]), float(prm["fy"]), float(prm["cx"]), float(prm["cy"]))
    got = fm.track_frame(0, 1, fmap, K, Tcw0, cap=CAP)
    assert got["num_matches"] == n and not got["capacity"] and np.array_equal(got["list"], lists0[0]), label
    # the same by the device entry on the returned list
    n_cur = len(fmap["cur_key"])
    corr_cap = n_cur + CAP
    d_m = torch.from_numpy(fh.pad_list(lists0[0], CAP)).cuda()
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    d, pd = fm.track_list_device(fm.frame_map_to_device(fmap), d_m, d_n, corr_cap, K, Tcw0)
    torch.cuda.synchronize()
    two = results.view_track({k: v.cpu().numpy() for k, v in d.items()}, n)
    for k in ("track_status", "n_map", "n_good", "n_kept", "n_removed", "n_matches_map"):
        assert got[k] == two[k], (label, k, got[k], two[k])
    for k in ("map", "carry_status", "cur_status", "corr_p3d", "corr_p2d", "corr_point", "Tcw", "kept_key", "kept_point", "removed"):
        assert np.ascontiguousarray(got[k]).view(np.uint8).tobytes() == np.ascontiguousarray(two[k]).view(np.uint8).tobytes(), (label, k)
    n_map = got["n_map"]
    assert got["pose"]["n_good"] == got["n_good"] == int(pd["n_good"].cpu()[0])
    assert np.array_equal(got["pose"]["outliers"], pd["outliers"].cpu().numpy()[0, :n_map])
    assert got["pose"]["pose_f64"].tobytes() == pd["pose_f64"].cpu().numpy()[0].tobytes()
    # and by the reference, on the call's own outlier bytes
    flags = got["pose"]["outliers"] != 0
    ref = fr.order_independent(fmap, lists0[0], n, CAP, corr_cap, 15, 10, lambda keys, points: (flags, {}))
    assert got["track_status"] == ref["track_status"] and n_map == ref["n_map"]
    assert np.array_equal(got["map"].view(np.int32).reshape(-1, 4), ref["map"])
    assert np.array_equal(got["kept_key"], ref["kept_key"]) and np.array_equal(got["removed"].view(np.int32).reshape(-1, 2), ref["removed"])
    assert np.array_equal(got["carry_status"], ref["carry_status"][:n]) and np.array_equal(got["cur_status"], ref["cur_status"])
    carried = int((ref["carry_status"][:n] == 0).sum())
    print("%s: %d matches, %d carried, %d replaced, n_map %d, kept %d, removed %d, n_good %d, n_matches_map %d, track_status %d" % (
        label, n, carried, int((ref["cur_status"] == 1).sum()), n_map, got["n_kept"], got["n_removed"], got["n_good"],
        got["n_matches_map"], got["track_status"]))
    assert carried >= min_carried and (ref["cur_status"] == 1).sum() >= 1 and (ref["cur_status"] == 0).sum() >= 1
    # keep_on_device: the pointers hold the bytes of the copy-back
    kept = fm.track_frame(0, 1, fmap, K, Tcw0, cap=CAP, keep_on_device=True, want_list=False)
    keep = kept["keep"]
    assert kept["track_status"] == got["track_status"] and kept["n_map"] == n_map and all(keep.values())

    def same_bytes(when):
        assert int(peek(fm, keep["d_track_status"], np.int32, 1)[0]) == got["track_status"], when
        assert int(peek(fm, keep["d_n_kept"], np.int32, 1)[0]) == got["n_kept"] and int(peek(fm, keep["d_n_map"], np.int32, 1)[0]) == n_map, when
        assert np.array_equal(peek(fm, keep["d_kept_key"], np.int32, got["n_kept"]), got["kept_key"]), when
        assert np.array_equal(peek(fm, keep["d_kept_point"], np.int32, got["n_kept"]), got["kept_point"]), when
        assert peek(fm, keep["d_corr_p3d"], np.float32, n_map * 3).tobytes() == got["corr_p3d"].tobytes(), when
        assert peek(fm, keep["d_corr_p2d"], np.float32, n_map * 2).tobytes() == got["corr_p2d"].tobytes(), when
        assert np.array_equal(peek(fm, keep["d_corr_point"], np.int32, n_map), got["corr_point"]), when
        assert np.array_equal(peek(fm, keep["d_outliers"], np.uint8, n_map), got["pose"]["outliers"]), when
        assert peek(fm, keep["d_Tcw"], np.float32, 12).tobytes() == got["Tcw"].tobytes(), when
    same_bytes("after the call")
    # a following msf_search_local_points (another family, its own workspace) leaves them alone; its current-frame map
    # is the kept map
    lmap = fm.make_local_map(fmap["points"], [0, len(fmap["ref_key"])], fmap["ref_key"], fmap["ref_point"],
                             got["kept_key"], got["kept_point"])
    search = fm.search_local_points(0, [1], lmap, tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), 0.5, cap=CAP)
    assert search["frustum"]["status_word"] == 0 and search["n_corr"] >= got["n_kept"]
    same_bytes("after msf_search_local_points")
    # msf_pose_optimize_device on the kept correspondences: the call's own pose
    z = lambda shape, dt="float32": torch.zeros(shape, dtype=getattr(torch, dt), device="cuda")
    pdev = dict(n_good=z((1,), "int32"), Tcw=z((1, 12)), outliers=z((1, keep["corr_cap"]), "uint8"))
    res = _lib.PoseResult(struct_size=C.sizeof(_lib.PoseResult), **{k: v.data_ptr() for k, v in pdev.items()})
    pp = fm._pose_params(K, 5.991)
    d_T = torch.from_numpy(Tcw0).cuda()
    fm._check(fm._L.msf_pose_optimize_device(fm._h, 1, keep["d_corr_p3d"], keep["d_corr_p2d"], keep["corr_cap"], keep["d_n_map"],
                                             d_T.data_ptr(), 12, None, 0, C.byref(pp), C.byref(res), None))
    if got["track_status"] in (0, 2):
        assert int(pdev["n_good"].cpu()[0]) == got["n_good"] and pdev["Tcw"].cpu().numpy()[0].tobytes() == got["Tcw"].tobytes()
    return fmap, K, Tcw0


@pytest.fixture(scope="module")
def orb():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.8, W, H, max_batch_pairs=2)
    yield m
    m.close()


@pytest.fixture(scope="module")
def orb_frames():
    from mono_slam_framework_amd import synth
    a, b = synth.synth_pair(3, W, H, shift=(12, 4))
    return [b, a]          # the current frame, then its predecessor


def test_orb_track_frame(orb, orb_frames):
    check_track_frame(orb, orb_frames, "orb", min_carried=40)


def test_loftr_track_frame():
    from mono_slam_framework_amd import synth
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    frames = [synth.kat_pattern(W, H, 32, 16), synth.kat_pattern(W, H, 0, 0)]
    dm = DNNFeatureMatcher(threshold=0.15, image_width=W, image_height=H, max_batch_pairs=2)
    try:
        check_track_frame(dm, frames, "loftr", min_carried=5)
    finally:
        dm.close()


def test_refusals_and_the_gate(orb, orb_frames):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import MsfError
    for i, f in enumerate(orb_frames):
        orb.store_frame(i, f)
    _, _, lists0 = orb.match_one_to_many(0, [1], cap=CAP)
    prm = tr.camera(1)
    fmap = frame_map_from_list(lists0[0], prm)
    Tcw0 = np.concatenate([prm["Rcw"].reshape(3, 3), prm["tcw"].reshape(3, 1)], 1).astype(np.float32).reshape(12)
    K = (float(prm["fx"]), float(prm["fy"]), float(prm["cx"]), float(prm["cy"]))

    def refused(text, *a, **kw):
        with pytest.raises(MsfError) as e:
            orb.track_frame(*a, **kw)
        assert e.value.code == _lib.MSF_ERR_INVALID_ARG and "msfx_track_frame: " in str(e.value) and text in str(e.value), str(e.value)
    refused("bad slot", 0, 4, fmap, K, Tcw0)
    refused("bad query slot", -1, 1, fmap, K, Tcw0)
    refused("cap_per_pair < 1", 0, 1, fmap, K, Tcw0, cap=0)
    refused("NaN", 0, 1, fmap, K, Tcw0, chi2=float("nan"))
    refused("negative", 0, 1, fmap, K, Tcw0, min_matches=-1)
    for what, bad in fr.malformed(fmap):
        refused("strictly increasing", 0, 1, bad, K, Tcw0)
    # the gate: more matches asked for than there are
    n = len(lists0[0])
    got = orb.track_frame(0, 1, fmap, K, Tcw0, min_matches=n + 1, cap=CAP)
    assert got["track_status"] == 1 and got["n_good"] == -1 and got["n_removed"] == 0 and got["pose"]["n_good"] == -1
    assert np.array_equal(got["kept_key"], fmap["cur_key"]) and np.array_equal(got["kept_point"], fmap["cur_point"])
    assert got["Tcw"].tobytes() == Tcw0.tobytes() and len(got["carry_status"]) == 0
    # a list longer than cap_per_pair: MSF_ERR_CAPACITY, as msf_match_one_to_many reports it
    short = orb.track_frame(0, 1, fmap, K, Tcw0, cap=16)
    assert short["capacity"] and short["num_matches"] == n and len(short["list"]) == 16
    # unknown flag bits and a missing keep, through the raw entry point
    m = orb._frame_map(fmap)
    prm_c = orb._track_params(K, Tcw0, 5.991, 15, 10)
    word, num = np.zeros(1, np.int32), np.zeros(1, np.int32)
    res = _lib.TrackResult(struct_size=C.sizeof(_lib.TrackResult), track_status=word.ctypes.data)
    call = lambda flags, keep: orb._L.msfx_track_frame(orb._h, 0, 1, C.byref(m), C.byref(prm_c), flags, num.ctypes.data, None,
                                                        64, C.byref(res), None, keep)
    assert call(2, None) == _lib.MSF_ERR_INVALID_ARG and "unknown flag bits" in orb.last_error()
    assert call(1, None) == _lib.MSF_ERR_INVALID_ARG and "keep" in orb.last_error()
    res.struct_size -= 8
    assert call(0, None) == _lib.MSF_ERR_INVALID_ARG and "struct_size" in orb.last_error()
