"""CPU: the reference and the inputs of tests/test_orb_match_gpu.py.  The numpy restatement of the matching step
(tests/orb_match_ref.py) equals oracle.orb.knn_match -- written independently, in C -- bit for bit on every input the GPU
tests use, and those inputs do reach what they are made for: ties of the best, second-bests at a lower index, bests and
second-bests on two sides of the 1024-row chunk and in two wave quarters, ratio products that round in f32.  A generator
weakened until one of these is gone fails here instead of letting the GPU tests pass on nothing."""
import numpy as np
import pytest

from oracle import orb as oracle_orb
from tests import orb_match_ref as R

RATIOS = (0.6, 0.75, 0.8, 1.5)
BIG = [i for i, n in enumerate(R.SIZES) if n >= 63]
N = len(R.SIZES)


def _xy(kp, rows):
    return np.stack([np.trunc(kp["x"][rows]), np.trunc(kp["y"][rows])], axis=1).astype(np.int32)


def test_layouts():
    from mono_slam_framework_amd import _lib
    assert R.KP_DTYPE == _lib.KP_DTYPE == oracle_orb.KP_DTYPE
    sets = R.grid_sets()
    assert [len(k) for k, _ in sets] == R.SIZES == [len(d) for _, d in sets]
    for k, d in sets:
        assert d.dtype == np.uint8 and d.shape == (len(k), 32)
        assert (k["x"] >= 0).all() and (k["x"] < 640).all() and (k["y"] >= 0).all() and (k["y"] < 480).all()
    pairs = R.pair_list()
    assert pairs.shape == (160, 2) and len({tuple(p) for p in pairs}) == 121
    assert len({tuple(p) for p in pairs[:128]} & {tuple(p) for p in pairs[128:]}) > 0     # repeats across the 128 / 32 cut


@pytest.mark.parametrize("ratio", RATIOS)
def test_reference_equals_oracle_on_the_grid(ratio):
    sets = R.grid_sets()
    total = 0
    for a in range(N):
        for b in range(N):
            (k1, d1), (k2, d2) = sets[a], sets[b]
            exp = oracle_orb.knn_match(k1, d1, k2, d2, ratio)
            got = R.grid_ref(a, b, ratio)
            assert got.dtype == np.int32 and got.shape == exp.shape, (R.SIZES[a], R.SIZES[b])
            np.testing.assert_array_equal(got, exp, err_msg="%d x %d" % (R.SIZES[a], R.SIZES[b]))
            if R.SIZES[a] == 0 or R.SIZES[b] < 2:
                assert len(got) == 0
            total += len(got)
    assert total > 5000


@pytest.mark.parametrize("edge", (0.8, 0.6))
def test_reference_equals_oracle_on_the_edge_sets(edge):
    kq, dq, kt, dt, _ = R.ratio_edge_set(edge)
    for ratio in RATIOS:
        np.testing.assert_array_equal(R.ref_match(kq, dq, kt, dt, ratio), oracle_orb.knn_match(kq, dq, kt, dt, ratio))


def test_grid_reaches_ties_close_seconds_and_both_chunks():
    sets = R.grid_sets()
    lower_second = 0
    straddle_tie = {i: 0 for i in BIG if R.SIZES[i] > R.CHUNK}
    straddle_pass = dict(straddle_tie)
    for a in BIG:
        for b in BIG:
            d0, i0, d1, i1 = R.grid_knn(a, b)
            label = "%d x %d" % (R.SIZES[a], R.SIZES[b])
            passing, tie = R.ratio_pass(d0, d1, 0.8), d0 == d1
            assert passing.sum() >= 1, label
            assert tie.sum() >= 6, label
            lower_second += int((passing & (i1 < i0)).sum())
            across = (i0 < R.CHUNK) != (i1 < R.CHUNK)
            if R.SIZES[b] == 2048:
                assert (passing & across).sum() >= 14, label
            if b in straddle_tie:
                straddle_tie[b] += int((tie & across).sum())
                straddle_pass[b] += int((passing & across).sum())
            if a != b:
                # ratio 1.5: a tie of the best passes, and the two equal bests show different points -- a kernel that
                # keeps the higher train index, or the one its merge met first, gives another row
                shown = tie & R.ratio_pass(d0, d1, 1.5)
                kt = sets[b][0]
                differ = (_xy(kt, i0[shown]) != _xy(kt, i1[shown])).any(axis=1)
                assert differ.sum() >= 4, label
                q0 = np.array([R.quarter_of(int(t), R.SIZES[b]) for t in i0[shown]]).reshape(-1, 2)
                q1 = np.array([R.quarter_of(int(t), R.SIZES[b]) for t in i1[shown]]).reshape(-1, 2)
                if R.SIZES[b] >= 255:
                    assert ((q0[:, 0] == q1[:, 0]) & (q0[:, 1] != q1[:, 1]) & differ).any(), label + ": quarters"
                if R.SIZES[b] == 2048:
                    assert ((q0[:, 0] != q1[:, 0]) & differ).any(), label + ": chunks"
    assert lower_second >= 200
    assert set(R.SIZES[b] for b in straddle_tie) == {1025, 2048}
    for b in straddle_tie:
        assert straddle_tie[b] >= 1 and straddle_pass[b] >= 1, R.SIZES[b]
    # the n_out > cap case and its neighbour
    assert len(R.grid_ref(N - 1, N - 1, 0.8)) > 1000 and len(R.grid_ref(0, N - 1, 0.8)) == 0


@pytest.mark.parametrize("ratio", (0.8, 0.6))
def test_edge_sets_hold_what_was_planted(ratio):
    pairs = R.ratio_edge_pairs(ratio)
    k = 4 if ratio == 0.8 else 3
    assert [(p[0], p[1]) for p in pairs] == [(k * i, 5 * i) for i in range(1, 13)]
    kq, dq, kt, dt, planted = R.ratio_edge_set(ratio)
    assert len(dt) == R.EDGE_TRAIN_ROWS > R.CHUNK and len(planted) == 12
    d0, i0, d1, i1 = R.ref_knn(dq, dt)
    D = R.hamming(dq, dt)
    for (q, p0, p1, best, second), pair in zip(planted, pairs):
        assert (d0[q], i0[q], d1[q], i1[q]) == (p0, best, p1, second) == (pair[0], best, pair[1], second)
        assert (D[q] <= p1).sum() == 2                                   # no filler inside the planted distances
    quarters = [(R.quarter_of(b, len(dt)), R.quarter_of(s, len(dt))) for _, _, _, b, s in planted]
    assert sum(qb != qs for qb, qs in quarters) == 6
    assert sum(qb[0] != qs[0] for qb, qs in quarters) == 2               # two of them across the 1024 chunk
    assert sum(s < b for _, _, _, b, s in planted) == 6
    assert len({q // 64 for q, *_ in planted}) == 3                      # three query blocks
    # the best and the second-best of a planted query show different points
    for q, _, _, b, s in planted:
        assert (_xy(kt, [b]) != _xy(kt, [s])).any()


def test_edge_sets_separate_f32_from_float64():
    """over the two sets: a planted pair that passes in f32 and fails in float64, and one that fails in f32 and passes in
    float64 (with the ratio the matcher holds, an f32).  At 0.8 the f32 product 0.8f * 5k rounds down to 4k for every k."""
    p = R.ratio_edge_pairs(0.8) + R.ratio_edge_pairs(0.6)
    assert (15, 25, True, False, True) in p
    assert any(p32 and not p64 for _, _, p32, p64, _ in p)
    assert any(not p32 and p64r for _, _, p32, _, p64r in p)
    assert all(not p32 and not p64 and p64r for _, _, p32, p64, p64r in R.ratio_edge_pairs(0.8))
    # the reference applies the f32 rule to the planted queries
    for ratio in (0.8, 0.6):
        kq, dq, kt, dt, planted = R.ratio_edge_set(ratio)
        got = {tuple(r) for r in R.ref_match(kq, dq, kt, dt, ratio)}
        for (q, d0, d1, best, _), pair in zip(planted, R.ratio_edge_pairs(ratio)):
            row = tuple(np.concatenate([_xy(kq, [q])[0], _xy(kt, [best])[0]]))
            assert (row in got) == pair[2], (ratio, d0, d1)
