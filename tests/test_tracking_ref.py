"""CPU: tests/tracking_ref.py -- the literal sequential restatement of Tracking::SearchLocalPoints (Tracking.cc:594-632)
equals the order-independent statement of include/msf_tracking.h (owner = smallest entry, gate, smallest ordinal) on
random scenes and on the tied cases: every status, count, record and correspondence.  It also asserts the scene
conditions the GPU tests rely on: every frustum code 0..9 and every claim status 0..4 at least five times per seed, and
at most 1 % of a scene's points inside a threshold band.  The second half does the same for the scenes past one chunk of
256 (tracking_ref.CHUNK_CASES) and asserts, on the reference's output, that each of them reaches the code it is there
for: owners, claims, key frames and the frame's own map past 256, winners and losers in different chunks, 64 owners in
every aligned group of 64 points."""
import numpy as np
import pytest

from tests import tracking_ref as tr

SEEDS = (1, 2, 3)


def both(lmap, prm, lists, n_out, cap):
    oi = tr.order_independent(lmap, prm, lists, n_out, cap, corr_cap=1 << 30)
    lit = tr.literal(lmap, prm, lists, n_out, cap)
    assert lit["visible"] == list(np.flatnonzero(oi["status"] == 0))
    assert np.array_equal(lit["n_to_match"], oi["n_to_match"])
    assert np.array_equal(lit["matched"], oi["matched"])
    assert np.array_equal(lit["calls"], oi["claims"])          # the same SetMapPoint calls in the same order
    final = {int(k): int(p) for k, p in zip(lmap["cur_key"], lmap["cur_point"])}
    final.update({int(c[0]): int(c[1]) for c in oi["claims"]})
    assert lit["cur_map"] == final
    # the correspondences are the frame's map in key order, then the claims in call order
    n_cur = len(lmap["cur_key"])
    assert oi["n_corr"] == n_cur + len(lit["calls"])
    assert np.array_equal(oi["corr_point"][n_cur:], lit["calls"][:, 1])
    assert np.array_equal(oi["corr_p2d"][n_cur:, 0], lit["calls"][:, 0] % tr.W)
    assert np.array_equal(oi["corr_p2d"][n_cur:, 1], lit["calls"][:, 0] // tr.W)
    assert np.array_equal(oi["corr_p3d"], lmap["points"]["pos"][oi["corr_point"]], equal_nan=True)
    return oi


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("cap", [128, 256])
def test_literal_equals_order_independent_on_scenes(seed, cap):
    both(*tr.scene(seed), cap)


@pytest.mark.parametrize("seed", SEEDS)
def test_small_and_empty_scenes(seed):
    both(*tr.scene(seed, n_points=65, n_kf=3, per_kf=30, n_cur=10, list_len=40, empty_kf=1), 64)
    both(*tr.scene(seed, n_points=1, n_kf=1, per_kf=12, n_cur=0, list_len=30), 64)
    both(*tr.scene(seed, n_points=5, n_kf=0, n_cur=3), 64)


def test_tied_cases():
    lmap, prm, lists, n_out = tr.tied_case()
    oi = both(lmap, prm, lists, n_out, 16)
    assert list(oi["n_to_match"]) == [3, 0, 4, 0, 0]            # point 3 is bad; key frames 3, 4 hold owned points only
    assert list(oi["matched"]) == [1, 0, 1, 0, 0]
    assert list(oi["claim_status"][0, :13]) == [0, 4, 4, 0, 0, 1, 1, 1, 1, 2, 3, 3, 3]
    assert list(oi["claim_status"][2, :4]) == [4, 0, 4, 0]
    assert (oi["claim_status"][[1, 3, 4]] == 255).all()
    assert [tuple(c) for c in oi["claims"][:3]] == [(8 * tr.W + 8, 0, 0, 0), (0, 3, 0, 3), ((tr.H - 1) * tr.W + tr.W - 1, 0, 0, 4)]
    # with the gate forced open the same pixel is contested by three key frames and an invalid list stays out
    forced = tr.order_independent(lmap, prm, lists, n_out, 16, 1 << 30, matched=np.ones(5, np.uint8))
    assert list(forced["claim_status"][3, :4]) == [4, 4, 0, 0] and (forced["claim_status"][4] == 255).all()
    assert list(forced["n_claimed"]) == [3, 1, 1, 2, 0]      # key frame 1 now takes (50, 50) from key frame 2
    short = tr.order_independent(lmap, prm, lists, n_out, 16, corr_cap=2 + oi["n_claims"] - 1)
    assert short["n_corr"] == -1 and np.array_equal(short["claims"], oi["claims"]) and "corr_p3d" not in short


@pytest.mark.parametrize("seed", SEEDS)
def test_scene_conditions(seed):
    lmap, prm, lists, n_out = tr.scene(seed)
    oi = tr.order_independent(lmap, prm, lists, n_out, 256, 1 << 30)
    counts = np.bincount(oi["status"], minlength=10)
    assert (counts >= 5).all(), counts
    claim_counts = np.bincount(oi["claim_status"][oi["claim_status"] != 255], minlength=5)
    assert (claim_counts >= 5).all(), claim_counts
    assert len(lmap["kf_start"]) == 9 and 850 <= len(lmap["points"]) <= 950
    flagged = oi["status"] >= 7
    worst, in_band = tr.check_against_f64(lmap["points"], prm, oi["status"], oi["diag"], flagged, "numpy f32 seed %d" % seed)
    print("seed %d: codes %s, claim statuses %s, worst fraction of a bar %.3f, %.2f %% of the points in a band"
          % (seed, list(counts), list(claim_counts), worst, 100 * in_band))
    assert in_band <= 0.01


# ---- past one chunk of 256: the scenes of tracking_ref.CHUNK_CASES ----------------------------------------------------

def test_the_default_scenes_are_what_they_were_before_kf_sizes():
    """sha256 over scene(1)'s integer arrays, taken before scene() learnt kf_sizes.  The generator's draws are one
    sequence and the lists are drawn last, so any added, dropped or changed draw changes this digest; the float
    arrays are left out of it because their last bits belong to the linear algebra library, not to the draws."""
    import hashlib
    lmap, prm, lists, n_out = tr.scene(1)
    h = hashlib.sha256()
    for k in ("kf_start", "kf_key", "kf_point", "cur_key", "cur_point"):
        h.update(np.ascontiguousarray(lmap[k], np.int32).tobytes())
    h.update(np.ascontiguousarray(lmap["points"]["flags"], np.uint32).tobytes())
    for l in lists:
        h.update(np.ascontiguousarray(l, np.int32).tobytes())
    h.update(np.ascontiguousarray(n_out, np.int32).tobytes())
    assert h.hexdigest() == "9329a2ce56757c4c5a9750c16b9c0799ca95c9aa94a9c90aa204a5377cd04a86"


@pytest.mark.parametrize("name", list(tr.CHUNK_CASES))
def test_literal_equals_order_independent_past_one_chunk(name):
    lmap, prm, lists, n_out, cap = tr.chunk_case(name)
    oi = both(lmap, prm, lists, n_out, cap)
    ref = tr.chunk_reference(name)       # what the host build and the device are held to
    for k in ("status", "owner_kf", "n_to_match", "matched", "claim_status", "claims", "n_claimed"):
        assert np.array_equal(oi[k], ref[k]), k
    assert ref["n_corr"] == oi["n_corr"] == len(lmap["cur_key"]) + ref["n_claims"]


def lost_matches(ref, lists):
    """-> [((kf, match) of a lost match, (kf, match) of the match that took its pixel)]"""
    winner = {int(c[0]): (int(c[2]), int(c[3])) for c in ref["claims"]}
    return [((int(i), int(j)), winner[int(lists[i][j][1]) * tr.W + int(lists[i][j][0])])
            for i, j in zip(*np.nonzero(ref["claim_status"] == 4))]


def test_the_long_runs_scene_reaches_past_one_chunk():
    lmap, prm, lists, n_out, cap = tr.chunk_case("long")
    ref = tr.chunk_reference("long")
    assert np.diff(lmap["kf_start"]).max() > 768 and len(lmap["cur_key"]) == 700 and (n_out > 1025).all()
    _, _, offset = tr.owner_entries(lmap)
    assert (offset >= 256).sum() >= 100 and (offset >= 768).any()
    assert ref["n_claimed"].max() > 512
    st = ref["claim_status"]
    assert (st[:, 256:] == 0).sum() >= 100 and (st[:, 256:] == 4).sum() >= 50
    lost = lost_matches(ref, lists)
    assert sum(1 for (i, j), (wi, wj) in lost if wi == i and wj // 256 != j // 256) >= 5
    assert sum(1 for (i, j), (wi, wj) in lost if wi != i) >= 5
    late = np.bincount(st[:, 512:][st[:, 512:] != 255], minlength=5)
    assert (late > 0).all(), late
    counts = np.bincount(ref["status"], minlength=10)
    assert (counts >= 5).all(), counts
    print("long runs: %d owners at offset >= 256, longest run %d, largest n_claimed %d, %d won and %d lost at j >= 256"
          % ((offset >= 256).sum(), np.diff(lmap["kf_start"]).max(), ref["n_claimed"].max(), (st[:, 256:] == 0).sum(),
             (st[:, 256:] == 4).sum()))
    # clipped at 512 and at 513: n_out stays above the cap, every list is cut there, winners on both sides of 256
    for name, cap in (("long-cap512", 512), ("long-cap513", 513)):
        clipped = tr.chunk_reference(name)
        assert tr.chunk_case(name)[4] == cap and (n_out > cap).all()
        assert clipped["claim_status"].shape == (4, cap) and (clipped["claim_status"] != 255).all()
        assert (clipped["claim_status"][:, cap - 1] == 0).any() and clipped["n_claimed"].min() > 256


def test_the_few_points_scene_leaves_the_owner_to_the_smallest_entry():
    lmap, prm, lists, n_out, cap = tr.chunk_case("few-points")
    points, first, offset = tr.owner_entries(lmap)
    assert (offset >= 256).sum() >= 50
    e = np.arange(len(lmap["kf_point"]))
    kf = np.searchsorted(lmap["kf_start"], e, side="right") - 1
    chunk = kf * 16 + (e - lmap["kf_start"][kf]) // 256           # a run has fewer than 16 chunks
    chunks_of = [len(set(chunk[lmap["kf_point"] == p])) for p in points]
    assert sum(c >= 2 for c in chunks_of) >= 50
    assert (n_out <= cap).all() and n_out.max() > 256
    print("few points: %d owners at offset >= 256, %d points referred to from two or more chunks"
          % ((offset >= 256).sum(), sum(c >= 2 for c in chunks_of)))


@pytest.mark.parametrize("n_cur", [255, 256, 257])
def test_the_exact_edges_scenes_have_the_sizes_they_name(n_cur):
    lmap, prm, lists, n_out, cap = tr.chunk_case("edges-cur%d" % n_cur)
    assert tuple(np.diff(lmap["kf_start"])) == tr.EDGE_SIZES and len(lmap["cur_key"]) == n_cur
    assert tuple(n_out) == tr.EDGE_N_OUT and cap == 1100 and all(len(l) >= 1100 for l in lists)
    forced = tr.chunk_reference("edges-cur%d" % n_cur, forced=True)
    assert tuple((forced["claim_status"] != 255).sum(1)) == tr.EDGE_N_OUT
    assert forced["n_claimed"][3] == 0 and forced["n_claimed"][[0, 1, 2, 4, 5]].min() > 0
    # winners past the first chunk of every list that has one: the running offset of the pack is used
    assert all((forced["claim_status"][i, 256:] == 0).any() for i in (0, 1, 2, 4, 5))


def test_the_many_key_frames_scene_reaches_both_sides_of_256():
    lmap, prm, lists, n_out, cap = tr.chunk_case("many-kf")
    assert tuple(np.diff(lmap["kf_start"])) == tr.MANY_SIZES and len(lmap["kf_start"]) == 301 and (n_out <= cap).all()
    for forced in (False, True):
        ref = tr.chunk_reference("many-kf", forced)
        ntm, ncl = ref["n_to_match"], ref["n_claimed"]
        for side in (slice(0, 256), slice(256, 300)):
            assert (ntm[side] > 0).any() and (ntm[side] == 0).any() and (ncl[side] > 0).any()
        assert (ncl[257:] > 0).any() and (ncl[:256] > 0).sum() > 1    # `front` of a late key frame sums over both strides
        n_cur = len(lmap["cur_key"])
        assert n_cur == 300 and ref["n_corr"] == n_cur + ref["n_claims"] and ref["n_claims"] == ncl.sum()
    gated = tr.chunk_reference("many-kf")
    assert (gated["matched"] == 0).any() and (gated["n_to_match"] > 0).sum() >= 200
    # a pixel contested across index 256
    lost = lost_matches(tr.chunk_reference("many-kf", True), lists)
    assert any(i >= 256 > wi for (i, _), (wi, _) in lost)
    print("many key frames: %d of 300 with n_to_match > 0" % (gated["n_to_match"] > 0).sum())


@pytest.mark.parametrize("n_kf,runs", tr.LADDERS)
def test_the_ladder_is_what_it_says(n_kf, runs):
    name = "ladder-%d" % n_kf + ("-empty" if runs else "")
    lmap, prm, lists, n_out, cap = tr.chunk_case(name)
    ref = tr.chunk_reference(name)
    rounds, start = tr.LADDER_ROUNDS, lmap["kf_start"]
    empty = np.zeros(n_kf, bool)
    for a, k in tr.ladder_empty_runs(n_kf, runs):
        empty[a:a + k] = True
        assert (start[a:a + k + 1] == start[a]).all()                # repeated values in kf_start
    live = np.flatnonzero(~empty)
    n_points = len(lmap["points"])
    assert len(start) == n_kf + 1 and n_points == len(live) * rounds
    assert (ref["status"] == 0).all()
    assert np.array_equal(ref["owner_kf"], live[np.arange(n_points) % len(live)])
    _, first, offset = tr.owner_entries(lmap)
    assert np.array_equal(offset, np.arange(n_points) // len(live))
    assert np.array_equal(ref["n_to_match"], np.where(empty, 0, rounds))
    flagged = np.zeros(n_points, bool)
    worst, in_band = tr.check_against_f64(lmap["points"], prm, ref["status"], ref["diag"], flagged, name)
    assert in_band == 0
    if len(live) >= 64:
        groups = ref["owner_kf"][:n_points // 64 * 64].reshape(-1, 64)
        assert len(groups) and all(len(set(g)) == 64 for g in groups)
    for a, k in tr.ladder_empty_runs(n_kf, runs):
        if a + k < n_kf:      # the point just after the stretch: owned by the first key frame behind it
            q = int(np.searchsorted(live, a + k))
            assert live[q] == a + k and live[q - 1] == a - 1 and ref["owner_kf"][q] == a + k and ref["owner_kf"][q - 1] == a - 1
    if runs:
        assert empty[n_kf - 1] and (runs < 2 or n_kf < 270 or (empty[254:259].all() and not empty[253] and not empty[259]))
        assert n_kf != 257 or empty[256]
    forced = tr.chunk_reference(name, forced=True)
    lost = lost_matches(forced, lists)
    # the repeat inside a list of six loses to the list's first match; the k1 shared with key frame i - 256 loses to it
    assert sum(1 for (i, j), (wi, wj) in lost if wi == i) >= sum(1 for i in live if i < 256 and i % 3 == 2)
    across = sum(1 for i in live if i >= 256 and not empty[i - 256])
    assert sum(1 for (i, j), (wi, _) in lost if j == 0 and wi == i - 256) == across and (n_kf < 320 or across >= 50)
    assert all(np.bincount(forced["claim_status"][forced["claim_status"] != 255], minlength=5) > 0)
