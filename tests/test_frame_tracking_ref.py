"""CPU: the two statements of tests/frame_tracking_ref.py -- the sequential code of TrackWithMotionModel /
TrackReferenceKeyFrame and the order-independent statement of include/msf_frame_tracking.h -- are equal on random scenes
and on the tied case, the scenes reach every status value, and with pose_ref.pose_optimization behind the carry every
track_status of a call that runs occurs.  Both statements also agree at the sizes of a real frame (8192 words; the
boundary case, whose runs of equal keys lie where the kernel's chunks of 1024 words meet)."""
import numpy as np
import pytest

from tests import frame_tracking_ref as fr
from tests import pose_ref

SEEDS = (0, 1, 2, 3)


def flag_some(rate, seed):
    """an optimiser that flags a fixed pseudo-random subset of the keys: a function of the key alone, so that both
    statements see the same flags"""
    def optimise(keys, points):
        return np.array([((k * 2654435761 + seed) >> 7) % 1000 < rate * 1000 for k in keys], bool), {}
    return optimise


@pytest.mark.parametrize("seed", SEEDS)
def test_literal_equals_order_independent(seed):
    fmap, matches = fr.scene(seed)                    # 300 ref entries, 150 cur entries, 160 matches
    assert (len(fmap["ref_key"]), len(fmap["cur_key"]), len(matches)) == (300, 150, 160)
    for opt in (fr.no_optimiser, flag_some(0.3, seed), flag_some(0.97, seed)):
        for n, cap, min_matches in ((160, 160, 15), (160, 120, 15), (200, 160, 15), (14, 160, 15), (15, 160, 15), (0, 160, 0)):
            lit = fr.literal(fmap, matches, n, cap, min_matches, 10, opt)
            oi = fr.order_independent(fmap, matches, n, cap, 150 + cap, min_matches, 10, opt)
            fr.agree(lit, oi)
    oi = fr.order_independent(fmap, matches, 160, 160, 310, 15, 10)
    counts = {s: int((oi["carry_status"][:160] == s).sum()) for s in (0, 1, 3, 4)}
    cur_counts = {s: int((oi["cur_status"] == s).sum()) for s in (0, 1)}
    print("seed %d: carry_status %s, cur_status %s, n_map %d" % (seed, counts, cur_counts, oi["n_map"]))
    assert min(counts.values()) >= 5 and min(cur_counts.values()) >= 5 and sum(counts.values()) == 160
    assert oi["n_map"] == 150 + counts[0] - cur_counts[1]


def test_tied_case():
    fmap, matches = fr.tied_case()
    n = len(matches)
    oi = fr.order_independent(fmap, matches, n, n, 3 + n, 0, 0, flag_some(0.4, 1))
    fr.agree(fr.literal(fmap, matches, n, n, 0, 0, flag_some(0.4, 1)), oi)
    assert list(oi["carry_status"]) == [4, 4, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 3, 3, 3, 3, 3]
    key = lambda x, y: y * fr.W + x
    assert list(oi["cur_status"]) == [1, 1, 0]                     # (0, 0) and (100, 100) replaced, (200, 100) stays
    rec = {int(r[0]): (int(r[1]), int(r[2])) for r in oi["map"]}
    assert rec[key(8, 8)] == (2, 3) and rec[key(100, 100)] == (0, 4) and rec[key(200, 100)] == (9, -1)
    assert rec[0] == (7, 5) and rec[key(fr.W - 1, fr.H - 1)] == (4, 8) and oi["n_map"] == 8


def large_scene():
    """8192 words, none of them padding: 3000 entries of the frame and a list of 5192"""
    return fr.scene(7, n_points=3000, n_ref=6000, n_cur=3000, n_matches=5192)


def test_boundary_case_lies_on_the_chunk_edges():
    fmap, matches = fr.boundary_case()
    runs = fr.boundary_runs(fmap, matches)
    n_cur, n = len(fmap["cur_key"]), len(matches)
    c = fr.carry(fmap, matches, n, n, n_cur + n)
    assert (c["carry_status"] == 1).sum() == 7 and (c["carry_status"] == 3).sum() == 9
    assert len(fr.sorted_words(fmap, matches, n, n)) == fr.BOUNDARY_WORDS == n_cur + n - 16
    entry, *three = runs[1022]
    assert c["cur_status"][entry] == 1 and sorted(c["carry_status"][r - n_cur] for r in three) == [0, 4, 4]
    assert c["carry_status"][max(three) - n_cur] == 0                       # the largest j wins
    assert c["carry_status"][runs[2047][0] - n_cur] == 0
    entry, match = runs[3071]
    assert c["cur_status"][entry] == 1 and c["carry_status"][match - n_cur] == 0
    ranks = np.array([r for _, r in fr.sorted_words(fmap, matches, n, n) if r >= n_cur])
    assert (np.diff(ranks) < 0).sum() > len(ranks) // 3                     # shuffled: rank order is not key order


@pytest.mark.parametrize("case", ("boundary", "large"))
def test_literal_equals_order_independent_past_one_chunk(case):
    fmap, matches = fr.boundary_case() if case == "boundary" else large_scene()
    n, n_cur = len(matches), len(fmap["cur_key"])
    if case == "large":
        assert (n_cur, n) == (3000, 5192)
    for opt in (fr.no_optimiser, flag_some(0.3, 7)):
        fr.agree(fr.literal(fmap, matches, n, n, 15, 10, opt), fr.order_independent(fmap, matches, n, n, n_cur + n, 15, 10, opt))


def test_refused_inputs():
    fmap, matches = fr.scene(0)
    assert fr.carry(fmap, matches, -1, 160, 400)["status"] == -3
    assert fr.carry(fmap, matches, 160, 160, 309)["status"] == -2 and fr.carry(fmap, matches, 160, 160, 310)["status"] == 0
    assert fr.carry(fmap, matches, 14, 160, 150, 15)["status"] == 1      # gated: only the frame's entries need room
    bad = fr.malformed(fmap)
    assert len(bad) == 12
    for what, m in bad:
        assert fr.carry(m, matches, 160, 160, 400)["status"] == -1, what


def dressed(kind, seed, observed=True, repeat=4, blind=5, n=pose_ref.N_SCENE):
    """A pose_ref scene of n correspondences as a train map plus a match list: correspondence i is match i from the pixel
    of p2d to a train pixel of its own that holds point i; `repeat` more matches repeat an earlier k1 with another point
    and `blind` carry no point.  observed: True (no table: every point counts), False (none does) or a uint8 [n] table.
    -> (fmap, matches, sc)"""
    from tests import tracking_ref as tr
    sc = pose_ref.scene(kind, seed, n)
    assert n == len(sc["p3d"])
    rng = np.random.default_rng(seed)
    pts = np.zeros(n, tr.MAP_POINT)
    pts["pos"] = sc["p3d"]
    ref_key = np.sort(rng.choice(fr.W * fr.H, n, replace=False)).astype(np.int32)
    rows = [(int(sc["p2d"][i, 0]), int(sc["p2d"][i, 1]), int(ref_key[i] % fr.W), int(ref_key[i] // fr.W)) for i in range(n)]
    for r in range(repeat):
        rows.insert(3 * r, (rows[-1 - r][0], rows[-1 - r][1], rows[r][2], rows[r][3]))    # overwritten by the later match
    for b in range(blind):
        rows.append((10 + b, 10, 3 + b, 1) if (1 * fr.W + 3 + b) not in set(ref_key) else (10 + b, 10, -1, 1))
    if isinstance(observed, np.ndarray):
        assert observed.dtype == np.uint8 and observed.shape == (n,)
    else:
        observed = None if observed else np.zeros(n, np.uint8)
    fmap = dict(points=pts, ref_key=ref_key, ref_point=np.arange(n, dtype=np.int32), cur_key=np.zeros(0, np.int32),
                cur_point=np.zeros(0, np.int32), observed=observed)
    return fmap, np.array(rows, np.int32), sc


def reference_optimiser(fmap, sc):
    def optimise(keys, points):
        p2d = np.array([(k % fr.W, k // fr.W) for k in keys], np.float32).reshape(-1, 2)
        r = pose_ref.pose_optimization(fmap["points"]["pos"][points].reshape(-1, 3), p2d, sc["K"], sc["Tcw0"])
        return r["outliers"], dict(n_good=r["n_good"], pose_f64=r["pose_f64"])
    return optimise


def test_every_track_status_with_the_reference_optimiser():
    seen = set()
    for observed, n_given in ((True, None), (False, None), (True, 14)):
        fmap, matches, sc = dressed("base", 1, observed)
        n = len(matches) if n_given is None else n_given
        opt = reference_optimiser(fmap, sc)
        oi = fr.order_independent(fmap, matches, n, len(matches), len(matches), 15, 10, opt, sc["Tcw0"])
        fr.agree(fr.literal(fmap, matches, n, len(matches), 15, 10, opt), oi)
        seen.add(oi["track_status"])
        if oi["track_status"] == 0:
            assert 10 <= oi["n_kept"] < oi["n_map"] and oi["n_removed"] > 0 and (oi["carry_status"][:n] == 4).sum() >= 4
    assert seen == {0, 1, 2}
