"""Finish units of the one-launch walker (k_walk, finish_unit): per (frame, level) one wave that waits for the level's
strips and then does, inside the launch, what k_fast_check, k_thr_harris and k_harris_flat do behind it -- the
completeness check, the retainBest(2N) cut, the stage-1 list and its Harris responses -- or hands a level that must be
redone densely over to those launches.  Stage 1, key points and descriptors against the CPU oracle on the smallest
frames that reach every case; the hand-over of redone levels; the run-time switch (MSF_ORB_WALK_FINISH=0) against the
default.  Every batch has at least 10 frames, so that it takes the one-launch walker."""
import numpy as np
import pytest

from mono_slam_framework_amd import synth
from oracle import orb as oracle_orb

pytestmark = pytest.mark.gpu

# (name, width, height, pairs)
CASES = [
    ("two_strips_ten_frames", 200, 250, 5),
    # 18 frames: XCDs with 3 and with 2 frames, surplus workgroups without a unit
    ("xcds_with_different_frame_counts", 300, 260, 9),
    # the smallest levels fall inside the 31-px border: their finish units find no candidates
    ("width_72_levels_inside_the_border", 72, 100, 64),
]


def _handle(w, h, n):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher
    return FeatureMatcher(0.7, w, h, max_batch_pairs=n, flags=_lib.MSF_FLAG_NO_FRAME_CACHE | _lib.MSF_FLAG_PROFILE)


def _ran_one_launch(fm):
    assert "pyramid_fast" in fm.stage_times(), "the walker did not make the pyramid: the case tests nothing"
    assert fm.walk_mode() == (False, 0)


def _by_yx(s1):
    return s1[np.lexsort((s1["lx"], s1["ly"]))]


def _has_rectangle(fm, l):
    w, h = (int(v) for v in fm.level_sizes()[l][:2])
    return w > 62 and h > 62


def _expected_mask(fm, slot):
    """levels a finish unit must have finished, from the thresholds: the final threshold is the first one or its
    refinement (never 20 after a failed check), and the level was not dense from the start -- a level at fastThreshold
    that has a key point rectangle takes the dense pass, which runs behind the launch; one without is finished empty"""
    taus = fm.fast_tau(slot)
    mask = 0
    for l in range(8):
        if taus[l][0] > 20 or (taus[l][0] == 20 and taus[l][1] == 20 and not _has_rectangle(fm, l)):
            mask |= 1 << l
    return mask, taus


def _assert_slot_is_the_oracles(fm, slot, img, w, h, where):
    orc = oracle_orb.OrbOracle(w, h)
    ko, do = orc.extract(img)
    s1o = orc.stage1_keypoints()
    for l in range(8):
        got = _by_yx(fm.stage1(slot, l))
        exp = s1o[s1o["octave"] == l]
        assert len(got) == len(exp), "%s L%d: stage 1 %d, oracle %d" % (where, l, len(got), len(exp))
        for f in ("lx", "ly", "fast_score"):
            np.testing.assert_array_equal(got[f], exp[f], err_msg="%s L%d %s" % (where, l, f))
        np.testing.assert_array_equal(got["response"].view(np.uint32), exp["response"].view(np.uint32),
                                      err_msg="%s L%d Harris" % (where, l))
    kg, dg = fm.keypoints(slot), fm.descriptors(slot)
    assert len(kg) == len(ko), where
    for f in ("lx", "ly", "octave", "fast_score"):
        np.testing.assert_array_equal(kg[f], ko[f], err_msg="%s %s" % (where, f))
    for f in ("x", "y", "response", "angle"):
        np.testing.assert_array_equal(kg[f].view(np.uint32), ko[f].view(np.uint32), err_msg="%s %s" % (where, f))
    np.testing.assert_array_equal(dg, do, err_msg=where + " descriptors")


@pytest.mark.parametrize("name,w,h,n", CASES, ids=[c[0] for c in CASES])
def test_levels_finished_inside_the_launch_are_the_oracles(name, w, h, n):
    """two calls on one handle (the finished words are reset per call); frames A and B of the first, a middle and the
    last pair: the mask of levels finished inside the launch covers every level the thresholds say it must, and stage 1
    (with the response bits), key points and descriptors are the oracle's"""
    fm = _handle(w, h, n)
    check = sorted({0, n // 2, n - 1, n, n + n // 2, 2 * n - 1})
    for call, mode in enumerate((0, 2)):
        A, B = synth.synth_batch(5200 + 300 * call, n, w, h, mode=mode)
        fm.match_batch(list(A), list(B), cap=1024)
        _ran_one_launch(fm)
        for s in check:
            where = "%s call %d slot %d" % (name, call, s)
            want, taus = _expected_mask(fm, s)
            mask = fm.walk_finished(s)
            print(where, "mask %02x expected %02x tau" % (mask, want), taus.tolist())
            assert mask & want == want, "%s: finished %02x, the thresholds say %02x" % (where, mask, want)
            assert mask & ~want == 0, "%s: finished %02x beyond %02x" % (where, mask, want)
            if call == 0:
                assert mask != 0, where
            _assert_slot_is_the_oracles(fm, s, A[s] if s < n else B[s - n], w, h, where)
    fm.close()


def _everything(fm, n):
    out = []
    for s in range(2 * n):
        out.append(([_by_yx(fm.stage1(s, l)).tobytes() for l in range(8)], fm.keypoints(s).tobytes(),
                    fm.descriptors(s).tobytes()))
    return out


REDO_SEED = 5800


def test_levels_that_fail_the_check_are_handed_to_the_dense_pass(monkeypatch):
    """MSF_ORB_TAU2_MARGIN_PCT=3 makes the refined threshold overshoot: some levels, not all, fail the check in their
    finish unit, are queued from there and redone behind the launch.  The mask is clear exactly on those levels; stage 1,
    key points and match lists are those of the default run; one pair is the oracle's.
    That the input sends some levels and not all through the dense pass is read from the handle's own thresholds
    (fast_tau): the CPU oracle is dense throughout and has no thresholds to ask.  Whether a level was queued by its finish
    unit or by k_fast_check is not told apart; a hand-over gone wrong shows in the lists."""
    w, h, n = 300, 260, 9
    A, B = synth.synth_batch(REDO_SEED, n, w, h, mode=0)
    fm = _handle(w, h, n)
    ref_lists = fm.match_batch(list(A), list(B), cap=1024)
    _ran_one_launch(fm)
    ref = _everything(fm, n)
    fm.close()
    monkeypatch.setenv("MSF_ORB_TAU2_MARGIN_PCT", "3")
    alt = _handle(w, h, n)
    got_lists = alt.match_batch(list(A), list(B), cap=1024)
    _ran_one_launch(alt)
    taus = np.stack([alt.fast_tau(s) for s in range(2 * n)])                   # [slot, level, (final, first)]
    redone = (taus[:, :, 0] == 20) & (taus[:, :, 1] > 20)
    print("levels redone per slot", redone.sum(axis=1).tolist())
    # the input must exercise the hand-over: a slot with levels that were redone and levels that were not (else: another seed)
    mixed = [s for s in range(2 * n) if redone[s].any() and (taus[s, :, 0] > 20).any()]
    assert mixed, "no slot with both redone and finished levels: %s" % taus[:, :, 0].tolist()
    for s in range(2 * n):
        mask = alt.walk_finished(s)
        for l in range(8):
            if redone[s, l]:
                assert not (mask >> l) & 1, "slot %d L%d was redone densely and is marked finished" % (s, l)
            elif taus[s, l, 0] > 20:
                assert (mask >> l) & 1, "slot %d L%d passed its check and is not marked finished" % (s, l)
    got = _everything(alt, n)
    for s in range(2 * n):
        assert got[s] == ref[s], "slot %d differs from the default run" % s
    for i in range(n):
        np.testing.assert_array_equal(got_lists[i], ref_lists[i], err_msg="pair %d" % i)
    i = mixed[0] % n
    np.testing.assert_array_equal(got_lists[i], oracle_orb.FeatureMatcherOracle(0.7).MatchFrames(A[i], B[i]))
    alt.close()


def test_switched_off_equals_switched_on(monkeypatch):
    """MSF_ORB_WALK_FINISH=0 leaves every level to the launches behind the walker (no level is marked), =2 places the
    finish units behind the next level's sampled quarter: stage 1, key points, descriptors and match lists of every
    slot are those of the default"""
    w, h, n = 300, 260, 9
    A, B = synth.synth_batch(6100, n, w, h, mode=0)
    fm = _handle(w, h, n)
    ref_lists = fm.match_batch(list(A), list(B), cap=1024)
    _ran_one_launch(fm)
    assert any(fm.walk_finished(s) for s in range(2 * n))
    ref = _everything(fm, n)
    fm.close()
    for value in ("0", "2"):
        monkeypatch.setenv("MSF_ORB_WALK_FINISH", value)
        alt = _handle(w, h, n)
        got_lists = alt.match_batch(list(A), list(B), cap=1024)
        _ran_one_launch(alt)
        masks = [alt.walk_finished(s) for s in range(2 * n)]
        assert any(masks) == (value != "0"), masks
        got = _everything(alt, n)
        for s in range(2 * n):
            assert got[s] == ref[s], "MSF_ORB_WALK_FINISH=%s: slot %d differs" % (value, s)
        for i in range(n):
            np.testing.assert_array_equal(got_lists[i], ref_lists[i], err_msg="MSF_ORB_WALK_FINISH=%s pair %d" % (value, i))
        alt.close()
