"""The walker's pyramid stores (walk_strip, RZ_EMIT) are issued for every source row and every lane: a row without an
output row and a lane without an output group store at an offset the buffer range check drops.  Such a store must never
land anywhere.  Pyramid pixels of levels 1-7 and the FAST candidate lists against the CPU oracle, on the smallest frames
that reach every emit case, and the bytes of a level that no store may touch (between a row's last group of four pixels
and its pitch) unchanged by a whole call."""
import numpy as np
import pytest

from mono_slam_framework_amd import synth
from oracle import orb as oracle_orb

pytestmark = pytest.mark.gpu

# (name, width, height, pairs).  64 pairs and more: strips of up to 240 rows (all four blocks of a strip's emit table);
# fewer: strips of at most 80 rows.  Every batch has at least 9 frames, so it takes the one-launch walker, not the dense kernel.
CASES = [
    # one 256-px window; two vertical strips of 128 and 122 rows, the second ends in a partial group of four rows
    ("one_window_two_strips", 200, 250, 64),
    # two windows, the second one 44 px to the right of the first; strips of 240 and 239 rows
    ("narrow_last_window_tall_strips", 300, 479, 64),
    # the narrowest frames (69 .. 80 px): levels of 60 .. 20 px, output groups for 15 .. 5 lanes
    ("width_72_most_lanes_idle", 72, 100, 64),
    # a small handle: short strips (four of 68 rows at level 0, with a partial last one), 10 frames
    ("short_strips_ten_frames", 300, 260, 5),
]


def _sorted_cands(c):
    c = np.asarray(c).reshape(-1, 3)
    return c[np.lexsort((c[:, 0], c[:, 1]))]


def _padded_level(fm, slot, level):
    from mono_slam_framework_amd import _lib
    w, h, pitch, _ = (int(v) for v in fm.level_sizes()[level])
    raw = fm._debug(_lib.DBG_LEVEL_PIXELS, fm._slot(slot, False), level, np.uint8, pitch * h).reshape(h, pitch)
    return raw, w


def _untouched(fm, slots):
    """the bytes no store of the walker may write: columns from the end of a row's last group of four to its pitch"""
    out = []
    for s in slots:
        for l in range(1, 8):
            raw, w = _padded_level(fm, s, l)
            out.append(raw[:, (w + 3) & ~3:].copy())
    return out


@pytest.mark.parametrize("name,w,h,n", CASES, ids=[c[0] for c in CASES])
def test_every_emit_case_writes_its_level_and_nothing_else(name, w, h, n):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher
    fm = FeatureMatcher(0.7, w, h, max_batch_pairs=n, flags=_lib.MSF_FLAG_NO_FRAME_CACHE | _lib.MSF_FLAG_PROFILE)
    check = sorted({0, n // 2, n - 1, n, n + n // 2, 2 * n - 1})      # frames A and B of the first, a middle and the last pair
    guard = None
    for call, mode in enumerate((0, 2)):
        A, B = synth.synth_batch(4100 + 300 * call, n, w, h, mode=mode)
        fm.match_batch(list(A), list(B), cap=1024)
        assert "pyramid_fast" in fm.stage_times(), "the walker did not make the pyramid: the case tests nothing"
        assert fm.walk_mode() == (False, 0)
        orc = oracle_orb.OrbOracle(w, h)
        for s in check:
            orc.extract(A[s] if s < n else B[s - n])
            taus = fm.fast_tau(s)
            for l in range(1, 8):
                raw, lw = _padded_level(fm, s, l)
                np.testing.assert_array_equal(raw[:, :lw], orc.level_pixels(l), err_msg="call %d slot %d pyramid L%d" % (call, s, l))
            for l in range(8):
                exp = np.asarray(orc.fast_candidates(l)).reshape(-1, 3)
                np.testing.assert_array_equal(_sorted_cands(fm.fast_candidates(s, l)), _sorted_cands(exp[exp[:, 2] >= taus[l][0]]),
                                              err_msg="call %d slot %d FAST candidates L%d (tau %d)" % (call, s, l, taus[l][0]))
        # other frames, another texture: a store that strayed into these bytes would have left other pixels there
        now = _untouched(fm, check)
        if guard is not None:
            for g, x in zip(guard, now):
                np.testing.assert_array_equal(x, g, err_msg="bytes between a level's rows changed during a call")
        guard = now
    fm.close()
