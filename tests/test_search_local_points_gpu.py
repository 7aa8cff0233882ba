"""GPU: msf_search_local_points -- the loop of Tracking::SearchLocalPoints in one call, once on an ORB and once on a
LoFTR handle with the frames of test_create_map_points_gpu.py.  Counts and lists of the matched key frames equal
msf_match_one_to_many on those slots; a key frame whose points are all behind the camera is not matched
(n_to_match == 0, num_matches == -1) and does not disturb its neighbours' lists; the rest equals msf_frustum_device +
msf_claim_points_device on the same lists bit for bit; with keep_on_device, msf_pose_optimize_device on the returned
pointers equals msf_pose_optimize on the host-gathered correspondences bit for bit; the refusals are those of the
documentation."""
import ctypes as C

import numpy as np
import pytest

from tests import tracking_host as th
from tests import tracking_ref as tr
from tests.test_create_map_points_gpu import SHIFTS, H, W

pytestmark = pytest.mark.gpu

CAP = 2048
GATED = 2          # the key frame whose points all lie behind the camera


def local_map_from_lists(lists, prm, seed=0, pad=0):
    """A local map whose key frames hold a point under the train end of every second match and whose frame holds one
    under the query end of every fifth, so that the extracted lists give claims, occupied pixels and misses.  The points
    of key frame GATED lie behind the camera; all others in front of it, seen head-on, where the frame sees the query
    end of their match: a claim is a consistent correspondence for the pose, the frame's own entries are not.
    pad: so many more points in every key frame, under train keys that no match of its list ends at (visible, but
    behind the camera in key frame GATED: the gate stays shut), and so many more entries of the frame's own map under
    keys that no match of any list starts at, each with a point of its own that projects there.  With pad = 0 nothing
    is drawn for them."""
    rng = np.random.default_rng(seed)
    R, t = prm["Rcw"].reshape(3, 3).astype(np.float64), prm["tcw"].astype(np.float64)
    pts, kf_start, kf_key, kf_point, cur = [], [0], [], [], {}

    def add_point(px, py, z):
        pc = np.array([(px - 320) / 500 * abs(z), (py - 240) / 500 * abs(z), z])
        pos = (R.T @ (pc - t)).astype(np.float32)
        po = pos.astype(np.float64) - prm["Ow"].astype(np.float64)
        p = np.zeros((), tr.MAP_POINT)
        p["pos"], p["normal"], p["max_distance"] = pos, po / np.linalg.norm(po), 100.0
        pts.append(p)
        return len(pts) - 1
    for i, l in enumerate(lists):
        seen_at = {}     # train key -> the query end of the first match that has it: the point projects there
        for (x1, y1, x2, y2) in l[::2]:
            seen_at.setdefault(int(y2) * W + int(x2), (int(x1), int(y1)))
        entries = []
        for k in sorted(seen_at):
            z = -4.0 if i == GATED else rng.uniform(2, 8)
            px, py = seen_at[k]
            entries.append((k, add_point(px, py, z)))
        last = len(pts) - 1 if pts else 0
        if pad:
            free = np.setdiff1d(np.arange(W * H), [int(y2) * W + int(x2) for (_, _, x2, y2) in l])
            for k in rng.choice(free, pad, replace=False):
                z = -4.0 if i == GATED else rng.uniform(2, 8)
                entries.append((int(k), add_point(rng.uniform(20, W - 20), rng.uniform(20, H - 20), z)))
        for k, p in sorted(entries):
            kf_key.append(k)
            kf_point.append(p)
        kf_start.append(len(kf_key))
        for (x1, y1, _, _) in l[::5]:
            cur.setdefault(int(y1) * W + int(x1), last)
    if pad:
        starts = [int(y1) * W + int(x1) for l in lists for (x1, y1, _, _) in l]
        free = np.setdiff1d(np.arange(W * H), starts + list(cur))
        for k in rng.choice(free, pad, replace=False):
            cur[int(k)] = add_point(int(k) % W, int(k) // W, rng.uniform(2, 8))
    pts = np.array(pts, tr.MAP_POINT)
    cur_key = np.array(sorted(cur), np.int32)
    cur_point = np.array([cur[k] for k in sorted(cur)], np.int32)
    pts["flags"][cur_point] |= tr.SEEN
    return dict(points=pts, kf_start=np.array(kf_start, np.int32), kf_key=np.array(kf_key, np.int32),
                kf_point=np.array(kf_point, np.int32), cur_key=cur_key, cur_point=cur_point)


def check_search(fm, frames, label, need_claims, pad=0):
    import torch
    from mono_slam_framework_amd import _lib
    for i, f in enumerate(frames):
        fm.store_frame(i, f)
    slots = list(range(1, len(frames)))
    n_kf = len(slots)
    num0, _, lists0 = fm.match_one_to_many(0, slots, cap=CAP)
    assert (num0 >= 0).all() and num0[GATED] > 0, num0     # the gate has a list to withhold
    prm = tr.camera(1)
    lmap = local_map_from_lists(lists0, prm, pad=pad)
    if pad:      # every run and the frame's own map pass one chunk of 256
        assert np.diff(lmap["kf_start"]).min() > 256 and len(lmap["cur_key"]) > 256
    args = (tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), 0.5)
    got = fm.search_local_points(0, slots, lmap, *args, cap=CAP)
    fr = got["frustum"]
    open_ = [i for i in range(n_kf) if fr["n_to_match"][i] > 0]
    assert fr["status_word"] == 0 and fr["n_to_match"][GATED] == 0 and got["num_matches"][GATED] == -1
    assert len(got["lists"][GATED]) == 0 and got["n_claimed"][GATED] == 0
    for i in open_:     # the gated key frame does not disturb its neighbours
        assert got["num_matches"][i] == num0[i] and np.array_equal(got["lists"][i], lists0[i]), (label, i)
    assert len(open_) >= (2 if need_claims else 1)
    # the same by the device entries on the same lists
    dmap = fm.local_map_to_device(lmap)
    fd = fm.frustum_device(dmap, *args)
    for k in ("n_to_match", "status", "visible", "owner_kf", "u", "v", "dist", "view_cos"):
        assert fd[k].cpu().numpy().tobytes() == fr[k].tobytes(), (label, k)
    matched = (fr["n_to_match"] > 0).astype(np.uint8)
    n_out = np.where(matched > 0, num0, -1).astype(np.int32)
    corr_cap = len(lmap["cur_key"]) + n_kf * CAP
    d_m = torch.from_numpy(th.pad_lists(lists0, CAP)).cuda()
    cd = fm.claim_points_device(dmap, d_m, torch.from_numpy(n_out).cuda(), torch.from_numpy(matched).cuda(), corr_cap)
    n_claims = int(cd["n_claims"].cpu()[0])
    assert got["n_claims"] == n_claims and np.array_equal(cd["n_claimed"].cpu().numpy(), got["n_claimed"])
    assert np.array_equal(cd["claims"].cpu().numpy()[:n_claims], got["claims"].view(np.int32).reshape(-1, 4))
    for i in open_:
        k = len(lists0[i])
        assert np.array_equal(cd["claim_status"].cpu().numpy()[i, :k], got["claim_status"][i, :k]), (label, i)
    n_corr = int(cd["n_corr"].cpu()[0])
    assert got["n_corr"] == n_corr == len(lmap["cur_key"]) + n_claims
    for k in ("corr_p3d", "corr_p2d", "corr_point"):
        assert cd[k].cpu().numpy()[:n_corr].tobytes() == got[k].tobytes(), (label, k)
    # and by the reference
    ref = tr.order_independent(lmap, prm, lists0, n_out, CAP, corr_cap)
    th.check_claims(dict(got, claims=got["claims"].view(np.int32).reshape(-1, 4),
                         claim_status=np.where(ref["claim_status"] == 255, 255, got["claim_status"])), ref, n_out, CAP, label)
    print("%s: matches %s, n_to_match %s, %d claims, %d correspondences" % (label, list(got["num_matches"]),
                                                                           list(fr["n_to_match"]), n_claims, n_corr))
    assert n_claims >= (20 if need_claims else 1)     # the claim and correspondence comparisons above are not vacuous
    # keep_on_device: the pose straight from the workspace equals the pose from the host-gathered correspondences
    kept = fm.search_local_points(0, slots, lmap, *args, cap=CAP, keep_on_device=True, want_lists=False)
    d_p3d, d_p2d, d_point, d_n, cap = kept["keep"]
    assert kept["n_corr"] == n_corr and cap == corr_cap and d_p3d and d_p2d and d_point and d_n
    Tcw0 = np.concatenate([prm["Rcw"].reshape(3, 3), prm["tcw"].reshape(3, 1)], 1).astype(np.float32).reshape(12)
    K = (float(prm["fx"]), float(prm["fy"]), float(prm["cx"]), float(prm["cy"]))
    want = fm.pose_optimize(got["corr_p3d"], got["corr_p2d"], K, Tcw0, diagnostics=False)
    z = lambda shape, dt="float32": torch.zeros(shape, dtype=getattr(torch, dt), device="cuda")
    d = dict(n_good=z((1,), "int32"), Tcw=z((1, 12)), outliers=z((1, cap), "uint8"), n_edges=z((1,), "int32"),
             rounds_run=z((1,), "int32"), pose_f64=z((1, 12), "float64"))
    res = _lib.PoseResult(struct_size=C.sizeof(_lib.PoseResult), **{k: v.data_ptr() for k, v in d.items()})
    pp = fm._pose_params(K, 5.991)
    d_T = torch.from_numpy(Tcw0).cuda()
    fm._check(fm._L.msf_pose_optimize_device(fm._h, 1, d_p3d, d_p2d, cap, d_n, d_T.data_ptr(), 12, None, 0, C.byref(pp),
                                             C.byref(res), None))
    assert int(d["n_good"].cpu()[0]) == want["n_good"] and int(d["n_edges"].cpu()[0]) == want["n_edges"] == n_corr
    if need_claims:
        assert 20 <= want["n_good"] < n_corr and want["rounds_run"] == 4      # inliers and outliers: the pose is a real one
    assert d["Tcw"].cpu().numpy().tobytes() == want["Tcw"].tobytes()
    assert d["pose_f64"].cpu().numpy().tobytes() == want["pose_f64"].tobytes()
    assert np.array_equal(d["outliers"].cpu().numpy()[0, :n_corr], want["outliers"])
    return lmap, prm, slots


@pytest.fixture(scope="module")
def orb():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.8, W, H, max_batch_pairs=8)
    yield m
    m.close()


@pytest.fixture(scope="module")
def orb_frames():
    from mono_slam_framework_amd import synth
    return [synth.synth_pair(3, W, H, shift=(0, 0))[0]] + [synth.synth_pair(3, W, H, shift=s)[1] for s in SHIFTS]


def test_orb_search_local_points(orb, orb_frames):
    check_search(orb, orb_frames, "orb", need_claims=True)


def test_orb_search_local_points_past_one_chunk(orb, orb_frames):
    """the fused call with every key frame's run and the frame's own map longer than 256: the checking kernel's loop
    and third block range, the claims' lookups in long runs, the correspondences of the frame's map from more than
    one workgroup -- behind the same comparisons"""
    check_search(orb, orb_frames, "orb padded", need_claims=True, pad=300)


def test_loftr_search_local_points():
    from mono_slam_framework_amd import synth
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    shifts = ((0, 0), (32, 16), (-16, 8), (16, 0), (16, 16), (0, 16))     # the gated key frame is one that matches
    frames = [synth.kat_pattern(W, H, sx, sy) for sx, sy in shifts]
    dm = DNNFeatureMatcher(threshold=0.15, image_width=W, image_height=H, max_batch_pairs=8)
    try:
        check_search(dm, frames, "loftr", need_claims=False)
    finally:
        dm.close()


def test_refusals(orb, orb_frames):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher, MsfError
    for i, f in enumerate(orb_frames):
        orb.store_frame(i, f)
    prm = tr.camera(1)
    lmap, _, lists, _ = tr.scene(5, n_points=80, n_kf=2, per_kf=30, n_cur=6, list_len=10)
    args = (tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), 0.5)

    def refused(text, *a, **kw):
        with pytest.raises(MsfError) as e:
            orb.search_local_points(*a, **kw)
        assert e.value.code == _lib.MSF_ERR_INVALID_ARG and "msf_search_local_points: " in str(e.value) and text in str(e.value), str(e.value)
    refused("bad slot", 0, [1, 16], lmap, *args)
    refused("bad query slot", -1, [1, 2], lmap, *args)
    refused("cap_per_pair < 1", 0, [1, 2], lmap, *args, cap=0)
    refused("NaN", 0, [1, 2], lmap, tr.view_of(prm), prm["Ow"], (0.0, 640.0, float("nan"), 480.0), 0.5)
    bad = dict(lmap, kf_key=lmap["kf_key"].copy())
    bad["kf_key"][1] = bad["kf_key"][0]
    refused("strictly increasing", 0, [1, 2], bad, *args)
    bad = dict(lmap, kf_point=lmap["kf_point"].copy())
    bad["kf_point"][0] = 80
    refused("kf_point is out of range", 0, [1, 2], bad, *args)
    many, _, _, _ = tr.scene(5, n_points=80, n_kf=9, per_kf=10, n_cur=6, list_len=10)
    refused("n exceeds max_batch_pairs", 0, list(range(1, 10)), many, *args)
    with pytest.raises(ValueError):
        orb.search_local_points(0, [1], lmap, *args)
    # zero key frames: no error, the frame's own correspondences
    none = orb.make_local_map(lmap["points"], [], [], [], lmap["cur_key"], lmap["cur_point"])
    got = orb.search_local_points(0, [], none, *args, cap=16)
    assert got["n_claims"] == 0 and got["n_corr"] == 6 and np.array_equal(got["corr_point"], lmap["cur_point"])
    assert (got["frustum"]["status"] == 9).all()
    # unknown flag bits and a missing keep, through the raw entry point
    m, n_points, n_kf = orb._local_map(lmap)
    fr = _lib.FrustumResult(struct_size=C.sizeof(_lib.FrustumResult))
    cl = _lib.ClaimResult(struct_size=C.sizeof(_lib.ClaimResult))
    word, ntm, ncl, nclk, num = (np.zeros(4, np.int32) for _ in range(5))
    fr.status_word, fr.n_to_match = word.ctypes.data, ntm.ctypes.data
    cl.status_word, cl.n_claims, cl.n_claimed = word.ctypes.data + 4, ncl.ctypes.data, nclk.ctypes.data
    slots = np.array([1, 2], np.int32)
    pp = orb._frustum_params(*args)
    call = lambda flags, keep: orb._L.msf_search_local_points(orb._h, 0, slots.ctypes.data, C.byref(m), C.byref(pp), flags,
                                                               num.ctypes.data, None, 64, C.byref(fr), C.byref(cl), keep)
    assert call(2, None) == _lib.MSF_ERR_INVALID_ARG and "unknown flag bits" in orb.last_error()
    assert call(1, None) == _lib.MSF_ERR_INVALID_ARG and "keep" in orb.last_error()
    assert call(0, None) == _lib.MSF_OK and word[0] == 0
    fr.struct_size -= 8
    assert call(0, None) == _lib.MSF_ERR_INVALID_ARG and "struct_size" in orb.last_error()
    fresh = FeatureMatcher(0.8, W, H, max_batch_pairs=2)
    try:
        with pytest.raises(MsfError) as e:
            fresh.search_local_points(0, [1, 2], lmap, *args)
        assert "msf_search_local_points: no frame was stored" in str(e.value)
    finally:
        fresh.close()
