"""Two index spaces of the ORB pipeline: frame i of a call works in row i of the per-call arrays (pyramid, candidate
lists, thresholds, walker state, stage-1 lists), whatever feature slot first_slot + i its key points and descriptors go
to.  An extraction into the cache slots at first_slot > 0 must therefore show, in every per-row view, the bytes of the
same frames extracted at first_slot = 0 -- streaming calls (ten frames: the one-launch walker with finish units), dense
calls (three frames), and streaming calls whose levels take the dense second pass -- and must leave the slots outside
the call alone.  The other ORB tests reach slot0 = 0 and slot0 = 2P only.

Candidate lists are compared sorted by (y, x): their order in memory is that of the appends.  At 200 x 250 every
level's primary list is its full-capacity list (orb_plan.h: lists of at most 16 K entries are not cut), so the candidate
view returns a redone level's list as it stands; the last test takes 1280 x 720 frames, where a redone level holds only
its retainBest(2N) cut and the view makes the complete list again with a dense pass of its own (debug_get)."""
import numpy as np
import pytest

from mono_slam_framework_amd import synth
from oracle import orb as oracle_orb

pytestmark = pytest.mark.gpu

W, H, PAIRS, SEED = 200, 250, 8, 7300
N = 10                      # frames of a streaming call (at least 8: below that a call is dense)
N_DENSE = 3


def _frames():
    A, B = synth.synth_batch(SEED, 5, W, H)
    return np.ascontiguousarray(np.concatenate([A, B], 0))


def _handle():
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher
    return FeatureMatcher(0.7, W, H, max_batch_pairs=PAIRS, flags=_lib.MSF_FLAG_NO_FRAME_CACHE | _lib.MSF_FLAG_PROFILE)


def _on_device(frames):
    """device frames with a row pitch that is a multiple of 16 (the device entry points take only such)"""
    import torch
    d = torch.zeros((len(frames), H, (W + 15) & ~15), dtype=torch.uint8, device="cuda")
    d[:, :, :W] = torch.from_numpy(frames).cuda()
    return d


def _stage_times(fm, first):
    """the stage times of the extraction just made: a handle reports a call's times once a match has closed the call"""
    import torch
    sa = torch.tensor([first], dtype=torch.int32, device="cuda")
    sb = torch.tensor([first + 5], dtype=torch.int32, device="cuda")      # frames 0 and 5: pair 0 of the synthetic batch
    out = torch.zeros((1, 1024, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    fm.match_slots_device(sa, sb, out, cnt)
    assert int(cnt[0]) > 0
    return fm.stage_times()


def _by_yx(s1):
    return s1[np.lexsort((s1["lx"], s1["ly"]))]


def _sorted_cands(c):
    c = np.asarray(c).reshape(-1, 3)
    return c[np.lexsort((c[:, 0], c[:, 1]))]


def _features(fm, slot):
    return {"keypoints": fm.keypoints(slot, cache=True).tobytes(), "descriptors": fm.descriptors(slot, cache=True).tobytes()}


def _cands(fm, slot):
    return {"fast_candidates L%d" % l: _sorted_cands(fm.fast_candidates(slot, l, cache=True)).tobytes() for l in range(8)}


def _views(fm, slot):
    """every view of one frame of the last extraction: the per-slot ones and the per-row ones"""
    v = _features(fm, slot)
    v.update(_cands(fm, slot))
    for l in range(8):
        v["stage1 L%d" % l] = _by_yx(fm.stage1(slot, l, cache=True)).tobytes()
    for l in range(1, 8):
        v["level_pixels L%d" % l] = fm.level_pixels(slot, l, cache=True).tobytes()
    v["fast_tau"] = fm.fast_tau(slot, cache=True).tobytes()
    v["walk_finished"] = fm.walk_finished(slot, cache=True)
    return v


def _assert_same(got, exp, where):
    assert got.keys() == exp.keys()
    for k in exp:
        assert got[k] == exp[k], "%s: %s differs" % (where, k)


@pytest.fixture(scope="module")
def runs():
    """one handle, every call of the streaming and the dense case, recorded once"""
    from mono_slam_framework_amd.matcher import MsfError
    frames = _frames()
    d = _on_device(frames)
    fm = _handle()
    r = {"frames": frames, "stream": {}, "dense": {}, "stage_times": {}}
    for first in (0, 3, 6):
        if first == 6:
            r["before_6"] = [_features(fm, s) for s in range(6)]
        fm.extract_device(d, first_slot=first)
        r["stage_times"][first] = _stage_times(fm, first)
        assert fm.walk_mode() == (False, 0)
        r["stream"][first] = [_views(fm, first + i) for i in range(N)]
        if first == 0:
            r["oracle_stage1"] = [_by_yx(fm.stage1(0, l, cache=True)) for l in range(8)]
            r["oracle_kp"], r["oracle_desc"] = fm.keypoints(0, cache=True), fm.descriptors(0, cache=True)
    r["after_6"] = [_features(fm, s) for s in range(6)]
    try:
        fm.stage1(0, 0, cache=True)
        r["slot0_error"] = None
    except MsfError as e:
        r["slot0_error"] = e
    for first in (0, 5):
        fm.extract_device(d[:N_DENSE], first_slot=first)
        r["dense"][first] = [_views(fm, first + i) for i in range(N_DENSE)]
    fm.close()
    return r


def test_streaming_call_into_other_slots_gives_the_same_views(runs):
    """ten frames at first_slot 0, 3 and 6 (the last that fits 16 slots) on one handle: frame i in slot first_slot + i
    gives the same bytes in every view; the calls ran the one-launch walker, with finish units"""
    for first in (0, 3, 6):
        assert "pyramid_fast" in runs["stage_times"][first], "the walker did not make the pyramid: the case tests nothing"
    assert any(v["walk_finished"] for v in runs["stream"][0]), "no level was finished inside the launch"
    assert all(len(v["keypoints"]) > 0 for v in runs["stream"][0])
    for first in (3, 6):
        for i in range(N):
            _assert_same(runs["stream"][first][i], runs["stream"][0][i], "first_slot %d frame %d" % (first, i))


def test_slots_outside_the_call_are_left_alone(runs):
    """after the call into slots 6 .. 15: slots 0 .. 5 hold the earlier calls' key points and descriptors byte for byte
    (frames 0 .. 2 twice), and slot 0 is no frame of the last extraction: it has no per-row view"""
    from mono_slam_framework_amd.matcher import MsfError
    for s in range(6):
        _assert_same(runs["after_6"][s], runs["before_6"][s], "slot %d" % s)
        exp = runs["stream"][0][s % 3]
        for k in ("keypoints", "descriptors"):
            assert runs["after_6"][s][k] == exp[k], "slot %d %s is not frame %d's" % (s, k, s % 3)
    assert isinstance(runs["slot0_error"], MsfError), "stage1 of a slot outside the last extraction did not raise"


def test_dense_call_into_other_slots_gives_the_same_views(runs):
    """three frames (a dense call: k_resize and the tile kernel, lists in the pool) at first_slot 5 and at 0; the
    features are those of the streaming call"""
    for i in range(N_DENSE):
        assert runs["dense"][0][i]["walk_finished"] == 0
        assert (np.frombuffer(runs["dense"][0][i]["fast_tau"], np.int32) == 20).all()
        _assert_same(runs["dense"][5][i], runs["dense"][0][i], "dense first_slot 5 frame %d" % i)
        for k in ("keypoints", "descriptors"):
            assert runs["dense"][0][i][k] == runs["stream"][0][i][k], "dense frame %d %s" % (i, k)


def test_dense_second_pass_into_other_slots(runs, monkeypatch):
    """MSF_ORB_TAU2_MARGIN_PCT=3: the refined thresholds overshoot and levels are redone by the dense second pass (its
    histogram, cut and queue are per-call arrays too).  Ten frames at first_slot 6 against first_slot 0: key points,
    descriptors and the candidate lists of every level; the key points are those of the default handle"""
    monkeypatch.setenv("MSF_ORB_TAU2_MARGIN_PCT", "3")
    d = _on_device(runs["frames"])
    fm = _handle()
    got = {}
    for first in (0, 6):
        fm.extract_device(d, first_slot=first)
        assert "pyramid_fast" in _stage_times(fm, first)
        got[first] = []
        for i in range(N):
            v = _features(fm, first + i)
            v.update(_cands(fm, first + i))
            got[first].append(v)
        taus = np.stack([fm.fast_tau(first + i, cache=True) for i in range(N)])      # [frame, level, (final, first)]
        redone = (taus[:, :, 0] == 20) & (taus[:, :, 1] > 20)
        print("first_slot %d: levels redone per frame" % first, redone.sum(axis=1).tolist())
        assert redone.any(), "no level took the dense second pass: the case tests nothing"
    fm.close()
    for i in range(N):
        _assert_same(got[6][i], got[0][i], "margin 3, first_slot 6 frame %d" % i)
        assert got[0][i]["keypoints"] == runs["stream"][0][i]["keypoints"], "margin 3 frame %d: key points" % i


def test_frame_0_is_the_oracles(runs):
    """stage 1 (with the response bits), key points and descriptors of frame 0 of the streaming call at first_slot 0"""
    orc = oracle_orb.OrbOracle(W, H)
    ko, do = orc.extract(runs["frames"][0])
    s1o = orc.stage1_keypoints()
    for l in range(8):
        got = runs["oracle_stage1"][l]
        exp = s1o[s1o["octave"] == l]
        assert len(got) == len(exp), "L%d: stage 1 %d, oracle %d" % (l, len(got), len(exp))
        for f in ("lx", "ly", "fast_score"):
            np.testing.assert_array_equal(got[f], exp[f], err_msg="L%d %s" % (l, f))
        np.testing.assert_array_equal(got["response"].view(np.uint32), exp["response"].view(np.uint32), err_msg="L%d Harris" % l)
    kg, dg = runs["oracle_kp"], runs["oracle_desc"]
    assert len(kg) == len(ko)
    for f in ("lx", "ly", "octave", "fast_score"):
        np.testing.assert_array_equal(kg[f], ko[f], err_msg=f)
    for f in ("x", "y", "response", "angle"):
        np.testing.assert_array_equal(kg[f].view(np.uint32), ko[f].view(np.uint32), err_msg=f)
    np.testing.assert_array_equal(dg, do, err_msg="descriptors")


def test_complete_list_view_of_a_cut_level_in_other_slots(monkeypatch):
    """1280 x 720, MSF_ORB_TAU2_MARGIN_PCT=3: levels are redone by the dense second pass, and those with more maxima
    than their primary list holds keep only the retainBest(2N) cut.  The candidate view of such a level runs the dense
    pass again into buffers of its own, with one row of counts and of the list map per frame of the last call: frame 0
    and the last frame, at first_slot 0 and 6, against the oracle's complete lists"""
    import torch
    w, h = 1280, 720
    monkeypatch.setenv("MSF_ORB_TAU2_MARGIN_PCT", "3")
    A, B = synth.synth_batch(9300, 5, w, h, mode=0)
    frames = np.concatenate([A, B], 0)
    d = torch.from_numpy(frames).cuda()
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher
    fm = FeatureMatcher(0.7, w, h, max_batch_pairs=PAIRS, flags=_lib.MSF_FLAG_NO_FRAME_CACHE)
    sizes = fm.level_sizes()
    # a level's list is cut when its full capacity (w h / 8) exceeds 16 K entries: to max(w h / 64, 8192) (orb_plan.h)
    prim = [max((int(sizes[l][0]) * int(sizes[l][1]) // 64 + 15) & ~15, 8192) if int(sizes[l][0]) * int(sizes[l][1]) // 8 > 16384
            else None for l in range(8)]
    orcs = {}
    for i in (0, N - 1):
        orcs[i] = oracle_orb.OrbOracle(w, h)
        orcs[i].extract(frames[i])
    for first in (0, 6):
        fm.extract_device(d, first_slot=first)
        rebuilt = 0
        for i, orc in orcs.items():
            taus = fm.fast_tau(first + i, cache=True)
            for l in range(1, 8):
                if not (taus[l][0] == 20 and taus[l][1] > 20):
                    continue
                exp = _sorted_cands(orc.fast_candidates(l))
                rebuilt += prim[l] is not None and len(exp) > prim[l]
                np.testing.assert_array_equal(_sorted_cands(fm.fast_candidates(first + i, l, cache=True)), exp,
                                              err_msg="first_slot %d frame %d L%d" % (first, i, l))
        print("first_slot %d: views of cut levels" % first, rebuilt)
        assert rebuilt >= 2, "no redone level with more maxima than its primary list holds: the case tests nothing"
    fm.close()
