"""GPU: msfx_track_list_device -- the carry, k_pose_optimize and the cut as three launches on one injected list.  The
scenes are those of tests/pose_ref.py (96 correspondences with outliers) dressed as a train map plus a match list in
which a few matches repeat a k1 and a few carry no point.  Every integer output equals tests/frame_tracking_ref.py run
on the device's own outlier bytes; Tcw, n_good, outliers and pose_f64 equal msf_pose_optimize on the host-gathered,
key-ordered list BIT FOR BIT (the equality include/msf_pose.h already promises of its device form: no tolerance here);
the kept map is a current-frame map that msf_claim_points_device accepts.  The gate on both sides of min_matches, n_map
of 2 / 3 / 9 / 10, an invalid list, and track_status 2 with nothing observed.  Past one chunk of the cut: n_map on both
sides of 256, 512 and 1024, scenes of 1500 and 3000 correspondences, and a gated call on a frame map of 600 entries."""
import numpy as np
import pytest

from tests import frame_tracking_host as fh
from tests import frame_tracking_ref as fr
from tests.test_frame_tracking_ref import dressed

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.8, fr.W, fr.H, max_batch_pairs=2)
    yield m
    m.close()


def run(fm, fmap, matches, n, sc, min_matches=15, min_map_matches=10, cap=None, corr_cap=None):
    """-> (track dict, pose dict) of numpy arrays; the outputs were filled with 255 / -7 before the call"""
    import torch
    from mono_slam_framework_amd import _lib, results
    cap = len(matches) if cap is None else cap
    n_cur = len(fmap["cur_key"])
    corr_cap = n_cur + cap if corr_cap is None else corr_cap
    d = results.alloc(_lib.track_shapes(cap, n_cur, corr_cap), "cuda")
    for v in d.values():
        v.fill_(255 if v.dtype == torch.uint8 else -7)
    d_m = torch.from_numpy(fh.pad_list(matches, cap)).cuda()
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    _, pd = fm.track_list_device(fm.frame_map_to_device(fmap), d_m, d_n, corr_cap, tuple(float(k) for k in sc["K"]),
                                 sc["Tcw0"], min_matches=min_matches, min_map_matches=min_map_matches, out=d)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}, {k: v.cpu().numpy() for k, v in pd.items()}


def check(fm, fmap, matches, n, sc, label, **kw):
    """one call against the reference on the device's own outlier bytes and against msf_pose_optimize; -> (track, ref)"""
    got, pose = run(fm, fmap, matches, n, sc, **kw)
    cap = kw.get("cap") or len(matches)
    corr_cap = kw.get("corr_cap") or len(fmap["cur_key"]) + cap
    min_matches, min_map = kw.get("min_matches", 15), kw.get("min_map_matches", 10)
    carried = fr.carry(fmap, matches, n, cap, corr_cap, min_matches)
    status = int(got["track_status"][0])
    if carried["status"] < 0:
        assert status == carried["status"], label
        for k, v in got.items():           # nothing else is written
            if k != "track_status":
                assert (v == (255 if v.dtype == np.uint8 else -7)).all(), (label, k)
        assert int(pose["n_good"][0]) == -1
        return got, carried
    n_map = carried["n_map"]
    flags = pose["outliers"][0, :n_map] if carried["status"] == 0 else np.zeros(n_map, np.uint8)
    ref = fr.order_independent(fmap, matches, n, cap, corr_cap, min_matches, min_map,
                               lambda keys, points: (flags != 0, {}))
    # the carry's outputs (the records without the cut's flags) and the cut's
    plain = dict(got, map=got["map"].copy())
    plain["map"][:n_map, 3] = 0
    fh.check_carry(dict(plain, status=carried["status"]), carried, label)
    fh.check_cut(got, ref, label)
    if carried["status"] == 1:
        assert status == 1 and int(got["n_good"][0]) == -1 and int(pose["n_good"][0]) == -1, label
        assert got["Tcw"][0].tobytes() == np.asarray(sc["Tcw0"], np.float32).tobytes(), label
        return got, ref
    # the optimiser: bit for bit msf_pose_optimize on the host-gathered list
    want = fm.pose_optimize(got["corr_p3d"][:n_map], got["corr_p2d"][:n_map], tuple(float(k) for k in sc["K"]), sc["Tcw0"],
                            diagnostics=False)
    assert int(got["n_good"][0]) == int(pose["n_good"][0]) == want["n_good"], label
    assert int(pose["n_edges"][0]) == want["n_edges"] == n_map and int(pose["rounds_run"][0]) == want["rounds_run"], label
    assert got["Tcw"][0].tobytes() == pose["Tcw"][0].tobytes() == want["Tcw"].tobytes(), label
    assert pose["pose_f64"][0].tobytes() == want["pose_f64"].tobytes(), label
    assert np.array_equal(pose["outliers"][0, :n_map], want["outliers"]), label
    assert (pose["outliers"][0, n_map:] == 0).all(), label            # beyond the list: as allocated
    return got, ref


@pytest.mark.parametrize("kind,seed", [("base", 1), ("few", 2), ("wide", 3), ("shallow", 1)])
def test_scenes(fm, kind, seed):
    import torch
    fmap, matches, sc = dressed(kind, seed)
    got, ref = check(fm, fmap, matches, len(matches), sc, "%s %d" % (kind, seed))
    print("%s %d: n_map %d, kept %d, removed %d, n_good %d, track_status %d" % (
        kind, seed, ref["n_map"], ref["n_kept"], ref["n_removed"], int(got["n_good"][0]), ref["track_status"]))
    assert ref["track_status"] == 0 and ref["n_removed"] > 0 and (ref["carry_status"] == 4).sum() >= 4 and (ref["carry_status"] == 3).sum() >= 5
    # the kept map is a current-frame map for msf_claim_points_device
    n_kept = ref["n_kept"]
    lmap = fm.make_local_map(fmap["points"], [0, len(fmap["ref_key"])], fmap["ref_key"], fmap["ref_point"],
                             got["kept_key"][:n_kept], got["kept_point"][:n_kept])
    d_m = torch.from_numpy(fh.pad_list(matches, len(matches))[None]).cuda()
    cd = fm.claim_points_device(fm.local_map_to_device(lmap), d_m, torch.tensor([len(matches)], dtype=torch.int32, device="cuda"),
                                torch.ones(1, dtype=torch.uint8, device="cuda"), n_kept + len(matches))
    assert int(cd["status_word"].cpu()[0]) == 0 and int(cd["n_corr"].cpu()[0]) >= n_kept


def test_frame_with_entries_of_its_own(fm):
    """TrackReferenceKeyFrame as the fallback: the frame holds entries, some of which the carry replaces"""
    fmap, matches, sc = dressed("base", 2)
    rng = np.random.default_rng(5)
    own = sorted(set(int(m[1]) * fr.W + int(m[0]) for m in matches[10:20]) | set(int(k) for k in rng.choice(fr.W * fr.H, 20)))
    fmap = dict(fmap, cur_key=np.array(own, np.int32), cur_point=rng.integers(0, len(fmap["points"]), len(own)).astype(np.int32))
    got, ref = check(fm, fmap, matches, len(matches), sc, "with entries")
    assert (ref["cur_status"] == 1).sum() >= 8 and (ref["cur_status"] == 0).sum() >= 15 and ref["track_status"] == 0


def test_gate_invalid_list_and_capacity(fm):
    fmap, matches, sc = dressed("base", 3)
    _, ref = check(fm, fmap, matches, 14, sc, "n = min_matches - 1")
    assert ref["track_status"] == 1 and ref["n_map"] == 0 and ref["n_kept"] == 0
    _, ref = check(fm, fmap, matches, 15, sc, "n = min_matches")
    assert ref["track_status"] in (0, 2) and ref["n_map"] > 0
    _, ref = check(fm, fmap, matches, -1, sc, "invalid list")
    assert ref["status"] == -3
    _, ref = check(fm, fmap, matches, len(matches), sc, "corr_cap one short", corr_cap=len(matches) - 1)
    assert ref["status"] == -2
    bad = dict(fmap, ref_point=fmap["ref_point"].copy())
    bad["ref_point"][5] = len(fmap["points"])
    _, ref = check(fm, bad, matches, len(matches), sc, "malformed")
    assert ref["status"] == -1


@pytest.mark.parametrize("n_map", (2, 3, 9, 10))
def test_short_maps(fm, n_map):
    """the optimiser's own thresholds: fewer than 3 edges (no round), fewer than 10 (one round), 10 (four)"""
    fmap, matches, sc = dressed("base", 1, repeat=0, blind=0)
    inl = np.flatnonzero(~sc["outlier"])[:n_map]              # distinct pixels: inliers of the scene
    m = matches[inl]
    assert len(set((int(a), int(b)) for a, b in m[:, :2])) == n_map
    got, ref = check(fm, fmap, m, n_map, sc, "n_map %d" % n_map, min_matches=0, min_map_matches=2)
    assert ref["n_map"] == n_map and ref["track_status"] == 0


# ---- past one chunk of the cut: maps of more than 256 records, lanes of the optimiser with up to 47 strides --------------

CUT_SIZES = (256, 257, 512, 513, 1024, 1025)
_LONG = {}


def observed_mask(n, seed=11):
    return (np.random.default_rng(seed).random(n) < 0.8).astype(np.uint8)


def long_scene():
    """("base", 2) with 1100 correspondences, no match repeated or blind, 80 % of the points observed; computed once"""
    if not _LONG:
        _LONG["scene"] = dressed("base", 2, n=1100, repeat=0, blind=0, observed=observed_mask(1100))
    return _LONG["scene"]


def window(matches, sc, n_map):
    """Rows of the list (row i is correspondence i) with pairwise distinct (x1, y1), so that the map has exactly n_map
    records: n_map of them that are consecutive in key order and end at an outlier of the scene.  The one record of
    the last chunk of 257 / 513 / 1025 is then one the optimiser flags."""
    key = matches[:, 1] * fr.W + matches[:, 0]
    _, first = np.unique(key, return_index=True)                  # one row per pixel, in key order
    last = max(i for i in np.flatnonzero(sc["outlier"][first]) if i >= n_map - 1)
    return np.sort(first[last - n_map + 1:last + 1])


def check_chunks(ref, label):
    """No pass on an empty case: on the device's own outlier bytes every chunk of 256 records of the map holds a removed
    and a kept record -- but a last chunk of one record, which can hold one of the two and holds a removed one --, some
    kept points are not observed, and the frame is tracked."""
    chunks = fr.cut_chunks(ref["outliers"])
    print("%s: n_map %d, (kept, removed) per chunk of the cut %s, n_matches_map %d of %d kept" % (
        label, ref["n_map"], chunks, ref["n_matches_map"], ref["n_kept"]))
    assert len(chunks) == -(-ref["n_map"] // 256) >= 1, label
    for kept, removed in chunks:
        assert removed >= 1 and (kept >= 1 or kept + removed == 1), (label, chunks)
    assert ref["n_matches_map"] < ref["n_kept"] and ref["track_status"] == 0, label


@pytest.mark.parametrize("n_map", CUT_SIZES)
def test_maps_at_the_chunk_edges_of_the_cut(fm, n_map):
    fmap, matches, sc = long_scene()
    m = matches[window(matches, sc, n_map)]
    assert len(set((int(a), int(b)) for a, b in m[:, :2])) == len(m) == n_map
    got, ref = check(fm, fmap, m, n_map, sc, "n_map %d" % n_map)
    assert ref["n_map"] == n_map
    check_chunks(ref, "n_map %d" % n_map)


@pytest.mark.parametrize("kind,seed,n,n_map", [("wide", 3, 1500, 1497), ("base", 2, 3000, 2982)])
def test_scenes_of_thousands(fm, kind, seed, n, n_map):
    """6 and 12 chunks of the cut behind a carry of two chunks / three chunks of step 3"""
    fmap, matches, sc = dressed(kind, seed, n=n, observed=observed_mask(n))
    label = "%s %d n %d" % (kind, seed, n)
    got, ref = check(fm, fmap, matches, len(matches), sc, label)
    print("%s: n_good %d" % (label, int(got["n_good"][0])))
    assert ref["n_map"] == n_map and (ref["carry_status"] == 4).sum() >= 4 and (ref["carry_status"] == 3).sum() >= 5
    check_chunks(ref, label)


def test_gated_call_keeps_a_frame_map_of_three_chunks(fm):
    fmap, matches, sc = dressed("base", 3)
    rng = np.random.default_rng(6)
    own = np.sort(rng.choice(fr.W * fr.H, 600, replace=False)).astype(np.int32)
    fmap = dict(fmap, cur_key=own, cur_point=rng.integers(0, len(fmap["points"]), 600).astype(np.int32))
    got, ref = check(fm, fmap, matches, 14, sc, "n = min_matches - 1, 600 entries")
    assert ref["track_status"] == 1 and ref["n_map"] == ref["n_kept"] == 600 and ref["n_removed"] == 0
    assert np.array_equal(got["kept_key"][:600], own) and np.array_equal(got["kept_point"][:600], fmap["cur_point"])
    assert (got["map"][:600, 3] == 0).all() and got["Tcw"][0].tobytes() == np.asarray(sc["Tcw0"], np.float32).tobytes()


def test_nothing_observed_is_status_2(fm):
    fmap, matches, sc = dressed("base", 1, observed=False)
    got, ref = check(fm, fmap, matches, len(matches), sc, "nothing observed")
    assert ref["track_status"] == 2 and ref["n_matches_map"] == 0 and ref["n_kept"] >= 10
    assert int(got["n_good"][0]) >= 10                           # the pose is written either way
