"""GPU: the two Hamming 2-NN kernels of csrc/orb_kernels.hip -- k_match_split (calls of at most 128 pairs) and k_match
(larger calls: what bench.py times) -- alone, on features the test writes into a handle's slots
(msf_debug_orb_set_features), against the numpy restatement of featurematcher.cpp:23-42 in tests/orb_match_ref.py.
Which kernel a call launched is asked of the handle (MSF_DBG_ORB_MATCH_FORM) and asserted, so a later change of the
128-pair threshold cannot turn the tests of one kernel into tests of the other.

Match lists are bit-exact by contract: every comparison is array equality with the reference's list, n_out included.
Every output buffer is pre-filled with a sentinel, and every row a call has no business writing -- past a pair's count,
past cap, the pairs of a bad slot, one guard pair behind the call's last -- must still hold it.

What the inputs reach (ties of the best, both chunks, all wave quarters, f32 ratio edges) is asserted on the CPU in
tests/test_orb_match_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import orb_match_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7777
SPLIT, ONE_PER_PAIR = 1, 2                    # MSF_DBG_ORB_MATCH_FORM
N = len(R.SIZES)
BIG, EMPTY = N - 1, 0                         # the slots of the 2048-row and the 0-row set


def _handle(threshold=0.8, pairs=8, width=640, height=480):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher
    return FeatureMatcher(threshold, width, height, max_batch_pairs=pairs, flags=_lib.MSF_FLAG_NO_FRAME_CACHE)


def _load_grid(fm, slots=range(N)):
    sets = R.grid_sets()
    for s in slots:
        fm.set_features(s, *sets[s])


def _enqueue(fm, pairs, cap=R.KP_CAP, stream=None):
    """one match_slots_device call on sentinel-filled buffers with a guard pair behind the last -> device (out, cnt)"""
    import torch
    p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2).astype(np.int32))
    sa, sb = torch.from_numpy(p[:, 0].copy()).cuda(), torch.from_numpy(p[:, 1].copy()).cuda()
    out = torch.full((len(p) + 1, cap, 4), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((len(p) + 1,), SENT, dtype=torch.int32, device="cuda")
    fm.match_slots_device(sa, sb, out[:len(p)], cnt[:len(p)], stream=stream)
    return out, cnt, (sa, sb)


def _run(fm, pairs, cap=R.KP_CAP):
    out, cnt, _ = _enqueue(fm, pairs, cap)
    return out.cpu().numpy(), cnt.cpu().numpy()


def _check(pairs, out, cnt, expect, label):
    """expect(a, b) -> the reference's list, or None for a pair that must come back with n_out = -1"""
    n = len(pairs)
    cap = out.shape[1]
    assert cnt[n] == SENT and (out[n] == SENT).all(), label + ": wrote behind the last pair"
    for i, (a, b) in enumerate(pairs):
        exp = expect(int(a), int(b))
        where = "%s: pair %d = slots (%d, %d)" % (label, i, a, b)
        if exp is None:
            assert cnt[i] == -1, where
            assert (out[i] == SENT).all(), where + ": rows of a refused pair written"
            continue
        assert cnt[i] == len(exp), where + ": n_out %d, reference %d" % (cnt[i], len(exp))
        k = min(len(exp), cap)
        np.testing.assert_array_equal(out[i, :k], exp[:k], err_msg=where)
        assert (out[i, k:] == SENT).all(), where + ": rows past the list written"


def _grid_expect(ratio):
    return lambda a, b: R.grid_ref(a, b, ratio)


def test_set_features_round_trip():
    """keypoints / descriptors of a slot return the bytes set_features wrote -- n = 0 and n = 2048 included, every field of
    the key point, a slot set twice, the last caller slot -- and neighbouring slots are left alone"""
    fm = _handle()
    sets = R.grid_sets()
    rng = np.random.default_rng(3)
    full_kp = np.frombuffer(rng.integers(0, 256, R.KP_CAP * 32, dtype=np.uint8).tobytes(), R.KP_DTYPE).copy()
    full_kp["x"], full_kp["y"] = sets[BIG][0]["x"], sets[BIG][0]["y"]
    plan = [(5, (full_kp, sets[BIG][1])), (4, sets[3]), (6, sets[8]), (15, sets[9]), (0, sets[1]), (1, sets[EMPTY])]
    for slot, (kp, desc) in plan:
        fm.set_features(slot, kp, desc)
    for slot, (kp, desc) in plan:
        got_k, got_d = fm.keypoints(slot, cache=True), fm.descriptors(slot, cache=True)
        assert got_k.shape == kp.shape and got_d.shape == desc.shape, slot
        assert got_k.tobytes() == kp.tobytes(), slot
        np.testing.assert_array_equal(got_d, desc, err_msg=str(slot))
    assert len(fm.keypoints(2, cache=True)) == 0                         # never set
    # a shorter set over a longer one: the count is what was set last
    fm.set_features(5, *sets[2])
    assert fm.keypoints(5, cache=True).tobytes() == sets[2][0].tobytes()
    np.testing.assert_array_equal(fm.descriptors(5, cache=True), sets[2][1])
    np.testing.assert_array_equal(fm.descriptors(4, cache=True), sets[3][1])
    np.testing.assert_array_equal(fm.descriptors(6, cache=True), sets[8][1])
    # float [n, 2] points in place of key point records
    xy = np.stack([sets[4][0]["x"], sets[4][0]["y"]], axis=1)
    fm.set_features(7, xy, sets[4][1])
    got = fm.keypoints(7, cache=True)
    assert got["x"].tobytes() == sets[4][0]["x"].tobytes() and got["y"].tobytes() == sets[4][0]["y"].tobytes()
    assert fm.match_form()[0] == 0                                       # nothing was matched yet
    fm.close()


def test_size_grid_both_kernels():
    """all 121 ordered pairs of the 11 sizes and 39 repeats: as one call (k_match), as calls of 128, 32 and 1
    (k_match_split), and at the threshold itself, 128 and 129 pairs"""
    fm = _handle()
    _load_grid(fm)
    pairs = R.pair_list()
    expect = _grid_expect(0.8)
    for part, form, label in ((pairs, ONE_PER_PAIR, "160"), (pairs[:128], SPLIT, "128"), (pairs[128:], SPLIT, "32"),
                              (pairs[:1], SPLIT, "1"), (pairs[:129], ONE_PER_PAIR, "129"),
                              (pairs[-128:], SPLIT, "last 128"), (pairs[-129:], ONE_PER_PAIR, "last 129")):
        out, cnt = _run(fm, part)
        assert fm.match_form() == (form, R.CHUNK), label
        _check(part, out, cnt, expect, label + " pairs")
    fm.close()


def test_ratio_above_one_shows_the_kept_index():
    """SetThreshold(1.5): two equal bests pass, and the list shows which train row was kept -- the lowest index, across
    wave quarters and across the 1024 chunk"""
    fm = _handle()
    _load_grid(fm)
    fm.SetThreshold(1.5)
    pairs = R.pair_list()
    expect = _grid_expect(1.5)
    for part, form, label in ((pairs, ONE_PER_PAIR, "160"), (pairs[:128], SPLIT, "128"), (pairs[128:], SPLIT, "32")):
        out, cnt = _run(fm, part)
        assert fm.match_form()[0] == form, label
        _check(part, out, cnt, expect, "ratio 1.5, %s pairs" % label)
    fm.close()


@pytest.mark.parametrize("ratio", (0.8, 0.6))
def test_ratio_edges(ratio):
    """planted (d0, d1) on which float(d0) < ratio * float(d1) rounds: f32 decides, in both kernels"""
    fm = _handle(threshold=ratio)
    kq, dq, kt, dt, _ = R.ratio_edge_set(ratio)
    fm.set_features(0, kq, dq)
    fm.set_features(1, kt, dt)
    exp = R.ref_match(kq, dq, kt, dt, ratio)
    back = R.ref_match(kt, dt, kq, dq, ratio)
    expect = lambda a, b: exp if (a, b) == (0, 1) else back                 # noqa: E731
    for pairs, form in (([(0, 1)], SPLIT), ([(0, 1), (1, 0)], SPLIT), ([(0, 1)] * 129, ONE_PER_PAIR),
                        ([(0, 1), (1, 0)] * 65, ONE_PER_PAIR)):
        out, cnt = _run(fm, pairs, cap=256)
        assert fm.match_form()[0] == form
        _check(pairs, out, cnt, expect, "ratio %.1f edges, %d pairs" % (ratio, len(pairs)))
    fm.close()


def test_more_matches_than_cap():
    """2048 x 2048 with cap = 7: n_out is the full count, the seven rows are the reference's first seven, and nothing
    lands behind them -- the next pair's rows (n_out = 0) and the guard still hold the sentinel"""
    fm = _handle()
    _load_grid(fm, (EMPTY, BIG))
    full = R.grid_ref(BIG, BIG, 0.8)
    assert len(full) > 1000
    expect = _grid_expect(0.8)
    for pairs, form in (([(BIG, BIG), (EMPTY, BIG)], SPLIT), ([(BIG, BIG)], SPLIT),
                        ([(BIG, BIG), (EMPTY, BIG)] * 65, ONE_PER_PAIR), ([(EMPTY, BIG)] * 128 + [(BIG, BIG)], ONE_PER_PAIR)):
        out, cnt = _run(fm, pairs, cap=7)
        assert fm.match_form()[0] == form
        _check(pairs, out, cnt, expect, "cap 7, %d pairs" % len(pairs))
        assert cnt[pairs.index((BIG, BIG))] == len(full)
    fm.close()


def test_bad_slots_in_a_one_per_pair_call():
    """slot indices -1, 16 (the first past the caller's), 2^30 and one of the handle's scratch range among 160 good
    pairs of a k_match call: those pairs give n_out = -1 and write nothing, every other pair equals the reference"""
    fm = _handle()
    _load_grid(fm)
    pairs = R.pair_list().copy()
    bad = {5: (0, -1), 17: (1, 16), 40: (0, 1 << 30), 77: (1, 20), 120: (0, 16), 131: (1, -1), 159: (0, 31), 0: (1, 1 << 30)}
    for at, (col, slot) in bad.items():
        pairs[at, col] = slot
    ok = set(range(2 * 8))
    expect = lambda a, b: R.grid_ref(a, b, 0.8) if a in ok and b in ok else None      # noqa: E731
    out, cnt = _run(fm, pairs)
    assert fm.match_form()[0] == ONE_PER_PAIR
    assert sorted(np.flatnonzero(cnt[:160] == -1).tolist()) == sorted(bad)
    _check(pairs, out, cnt, expect, "bad slots, 160 pairs")
    # the same through the other kernel: the first 128 pairs hold six of them
    out, cnt = _run(fm, pairs[:128])
    assert fm.match_form()[0] == SPLIT
    _check(pairs[:128], out, cnt, expect, "bad slots, 128 pairs")
    fm.close()


def test_back_to_back_on_one_stream():
    """split, one-per-pair, split, split on one handle and one stream with nothing waiting in between: every list equals
    the reference, so each split launch found its ticket counters at zero"""
    import torch
    fm = _handle()
    _load_grid(fm)
    pairs = R.pair_list()
    parts = [pairs[:128], pairs, pairs[128:], pairs[:128]]
    stream = torch.cuda.Stream()
    keep = []
    with torch.cuda.stream(stream):
        for part in parts:
            keep.append(_enqueue(fm, part, stream=stream.cuda_stream))
    stream.synchronize()
    expect = _grid_expect(0.8)
    for i, (part, (out, cnt, _)) in enumerate(zip(parts, keep)):
        _check(part, out.cpu().numpy(), cnt.cpu().numpy(), expect, "call %d of 4 (%d pairs)" % (i + 1, len(part)))
    assert fm.match_form()[0] == SPLIT
    fm.close()


def test_position_independence():
    """a seeded permutation of the 160-pair call: a pair's list does not depend on its place in the grid"""
    fm = _handle()
    _load_grid(fm)
    pairs = R.pair_list()
    perm = np.random.default_rng(8).permutation(len(pairs))
    assert (perm != np.arange(len(pairs))).sum() > 150
    out, cnt = _run(fm, pairs[perm])
    assert fm.match_form()[0] == ONE_PER_PAIR
    _check(pairs[perm], out, cnt, _grid_expect(0.8), "permuted 160 pairs")
    fm.close()


def test_null_slot_arrays_through_one_per_pair():
    """match_batch_device of 130 pairs: extraction, then k_match with no slot arrays (pair i = slots base + i and
    base + 130 + i); every list equals the CPU matcher's"""
    import torch
    from mono_slam_framework_amd import synth
    from oracle import orb as oracle_orb
    n, w, h = 130, 160, 120
    A, B = synth.synth_batch(900, n, w, h)
    orc = oracle_orb.FeatureMatcherOracle(0.8)
    exp = [orc.MatchFrames(A[i], B[i]) for i in range(n)]
    assert min(len(e) for e in exp) >= 59 and np.median([len(e) for e in exp]) >= 100
    fm = _handle(pairs=n, width=w, height=h)
    out = torch.full((n + 1, 512, 4), SENT, dtype=torch.int32, device="cuda")
    cnt = torch.full((n + 1,), SENT, dtype=torch.int32, device="cuda")
    fm.match_batch_device(torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda(), out[:n], cnt[:n])
    assert fm.match_form()[0] == ONE_PER_PAIR
    _check([(i, i) for i in range(n)], out.cpu().numpy(), cnt.cpu().numpy(), lambda a, b: exp[a], "130 frame pairs")
    fm.close()


def _small_chunk_child(chunk):
    """runs in a process of its own, started with MSF_ORB_TRAIN_CHUNK = chunk: the pairs of the size grid with at most 257
    rows on both sides, in both kernels"""
    fm = _handle()
    small = [i for i, n in enumerate(R.SIZES) if n <= 257]
    _load_grid(fm, small)
    pairs = np.array([p for p in R.pair_list() if p[0] in small and p[1] in small], np.int32)
    assert 64 <= len(pairs) <= 128
    twice = np.concatenate([pairs, pairs[::-1]])
    expect = _grid_expect(0.8)
    for part, form in ((pairs, SPLIT), (twice, ONE_PER_PAIR), (pairs[:1], SPLIT)):
        out, cnt = _run(fm, part, cap=512)
        assert fm.match_form() == (form, chunk), fm.match_form()
        _check(part, out, cnt, expect, "chunk %d, %d pairs" % (chunk, len(part)))
    fm.close()
    print("small chunk child ok")


@pytest.mark.parametrize("chunk", (96, 16))
def test_small_chunks(chunk):
    """MSF_ORB_TRAIN_CHUNK is read once per process: a child with chunk 96 (257 rows = 3 chunks, the last of 65) and one
    with 16 (the smallest; quarters of four rows, a last chunk of one row)"""
    code = "import sys; sys.path.insert(0, %r); from tests.test_orb_match_gpu import _small_chunk_child as f; f(%d)" % (ROOT, chunk)
    env = dict(os.environ, MSF_ORB_TRAIN_CHUNK=str(chunk))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "small chunk child ok" in r.stdout, r.stdout + r.stderr
