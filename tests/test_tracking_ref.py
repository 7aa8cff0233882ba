"""CPU: tests/tracking_ref.py -- the literal sequential restatement of Tracking::SearchLocalPoints (Tracking.cc:594-632)
equals the order-independent statement of include/msf_tracking.h (owner = smallest entry, gate, smallest ordinal) on
random scenes and on the tied cases: every status, count, record and correspondence.  It also asserts the scene
conditions the GPU tests rely on: every frustum code 0..9 and every claim status 0..4 at least five times per seed, and
at most 1 % of a scene's points inside a threshold band."""
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
