"""ORB on inputs at the edge of the fixed-capacity device lists (tests/orb_capacity.py): a pair comes back loud
(n_out = -1) exactly when the oracle's own counts exceed a documented cap, bit-exact otherwise -- in every call form
(match_batch, match_batch_device, extract_device + match_slots_device), at every batch size and position, whatever
the other frames of the call are.  Default settings throughout: no MSF_ORB_* overrides."""
import numpy as np
import pytest

from mono_slam_framework_amd import synth
from tests import orb_capacity as oc

pytestmark = pytest.mark.gpu
RATIO = 0.8
PAIR_COUNTS = (1, 3, 4, 8, 64)
MAX_PAIRS = 64
WITHIN = [n for n in oc.GENERATORS if oc.kind(n) != "over"]
NOISE = [n for n in oc.DENSE_PASS if n.startswith("noise")]


def _handle(w, h, pairs=MAX_PAIRS):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher
    return FeatureMatcher(RATIO, w, h, max_batch_pairs=pairs, flags=_lib.MSF_FLAG_NO_FRAME_CACHE)


class _Frames:
    """The frames of one size: every generator (noise also with a second seed) and ordinary synthetic frames."""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.img = {n: oc.frame(n, w, h) for n in oc.GENERATORS}
        for s in NOISE:
            self.img[s + "b"] = oc.noise(w, h, int(s[5:]), seed=1)
        A, B = synth.synth_batch(4100, 6, w, h)
        for i in range(6):
            self.img["synth%da" % i], self.img["synth%db" % i] = A[i], B[i]
        self.synth = [n for n in self.img if n.startswith("synth")]
        self.noise = [n for n in self.img if n.startswith("noise")]
        self.hard = [n for n in self.img if n in WITHIN or n in self.noise]
        self.orc = oc.OracleMatcher(RATIO)
        self._cap = {}

    def over(self, name):
        if name not in self._cap:
            self._cap[name] = oc.capacity(self.img[name])
        return bool(self._cap[name].loud)

    def expected(self, a, b):
        """the oracle's list, or None for a pair that must be loud"""
        if self.over(a) or self.over(b):
            return None
        return self.orc.match(self.img[a], self.img[b])


_FRAMES = {}


def _frames(w, h):
    if (w, h) not in _FRAMES:
        _FRAMES[(w, h)] = _Frames(w, h)
    return _FRAMES[(w, h)]


def _mixed_pairs(F, n, seed, noise_share=0.0):
    """n pairs: hard frames at varying positions interleaved with synthetic ones; noise_share of the frames noise"""
    rng = np.random.default_rng(seed)
    pairs = []
    for i in range(n):
        pick = []
        for side in range(2):
            r = rng.random()
            if r < noise_share:
                pick.append(F.noise[int(rng.integers(len(F.noise)))])
            elif (i + side) % 2 == 0:
                pick.append(F.hard[int(rng.integers(len(F.hard)))])
            else:
                pick.append(F.synth[int(rng.integers(len(F.synth)))])
        pairs.append(tuple(pick))
    return pairs


def _run_all_forms(fm, F, pairs, cap=2048):
    """n_out and lists of the pairs through match_batch, match_batch_device and extract_device + match_slots_device"""
    import torch
    A = np.stack([F.img[a] for a, _ in pairs])
    B = np.stack([F.img[b] for _, b in pairs])
    n = len(pairs)
    res = {}
    num, lists = fm.match_batch_raw(list(A), list(B), cap=cap)
    res["match_batch"] = (np.asarray(num), lists)
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    out = torch.zeros((n, cap, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((n,), dtype=torch.int32, device="cuda")
    try:
        fm.match_batch_device(dA, dB, out, cnt, stream=torch.cuda.current_stream().cuda_stream)
    except Exception as e:      # MSF_ERR_CAPACITY is reported through n_out; anything else is a failure below
        if getattr(e, "code", None) != -4:
            raise
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    o = out.cpu().numpy()
    res["match_batch_device"] = (c, [o[i, :max(int(c[i]), 0)] for i in range(n)])
    frames = torch.cat([dA, dB], 0)
    try:
        fm.extract_device(frames, first_slot=0)
    except Exception as e:
        if getattr(e, "code", None) != -4:
            raise
    sa = torch.arange(n, dtype=torch.int32, device="cuda")
    sb = sa + n
    out.zero_()
    cnt.zero_()
    try:
        fm.match_slots_device(sa, sb, out, cnt)
    except Exception as e:
        if getattr(e, "code", None) != -4:
            raise
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    o = out.cpu().numpy()
    res["extract+match_slots"] = (c, [o[i, :max(int(c[i]), 0)] for i in range(n)])
    return res


def _check(F, pairs, res, what):
    bad = []
    for form, (num, lists) in res.items():
        for i, (a, b) in enumerate(pairs):
            exp = F.expected(a, b)
            if exp is None:
                if num[i] != -1:
                    bad.append("%s %s pair %d (%s, %s): n_out %d, expected -1 (over caps)" % (what, form, i, a, b, num[i]))
            elif num[i] != len(exp) or not np.array_equal(lists[i], exp):
                bad.append("%s %s pair %d (%s, %s): n_out %d, oracle %d matches" % (what, form, i, a, b, num[i], len(exp)))
    assert not bad, "\n".join(bad[:40]) + ("\n... %d in all" % len(bad) if len(bad) > 40 else "")


def _outcome(num, lists, F, pairs, i):
    return "loud" if num[i] == -1 else ("exact" if np.array_equal(lists[i], F.orc.match(*[F.img[x] for x in pairs[i]]))
                                        else "WRONG(%d)" % num[i])


@pytest.mark.parametrize("w,h", [(640, 480), (1280, 720)], ids=["640x480", "1280x720"])
def test_within_caps_is_exact_in_every_call_form_and_batch_size(w, h):
    """Mixed batches of 1, 3, 4, 8 and 64 pairs (calls of fewer than eight frames take the dense kernel, the others the
    streaming pass and its dense second pass), and one batch of max_batch_pairs pairs at least half of whose frames are
    noise (most levels need more than their primary list at fastThreshold): every pair is the oracle's."""
    F = _frames(w, h)
    fm = _handle(w, h)
    for n in PAIR_COUNTS:
        pairs = _mixed_pairs(F, n, seed=100 * n + w)
        _check(F, pairs, _run_all_forms(fm, F, pairs), "%d pairs" % n)
    pairs = _mixed_pairs(F, MAX_PAIRS, seed=7 + w, noise_share=0.6)
    assert sum(x in F.noise for p in pairs for x in p) >= MAX_PAIRS
    _check(F, pairs, _run_all_forms(fm, F, pairs), "noise-heavy %d pairs" % MAX_PAIRS)
    fm.close()


def test_over_caps_is_loud_and_does_not_touch_the_rest_of_the_batch():
    """A pair with a frame over a cap (dots4, salt: stage 1 of level 0 > kS1Cap) is n_out = -1 in every call form -- never
    a short or wrong list -- and the within-caps pairs of the same batch, noise among them, stay exact."""
    w, h = 640, 480
    F = _frames(w, h)
    fm = _handle(w, h, pairs=8)
    pairs = [("dots4", "synth0b"), ("noise30", "noise30b"), ("synth1a", "synth1b"), ("synth2a", "salt"),
             ("weak_dots", "noise45"), ("salt", "dots4"), ("checker2", "synth3a"), ("noise16b", "noise20")]
    assert [F.expected(a, b) is None for a, b in pairs] == [True, False, False, True, False, True, False, False]
    _check(F, pairs, _run_all_forms(fm, F, pairs), "8 pairs")
    fm.close()


def test_outcome_of_a_pair_does_not_depend_on_the_batch():
    """The same pairs alone, in a batch of 8 and in batches of 64 at two positions (the rest noise): the same outcome
    each time, and the one the oracle's counts call for."""
    w, h = 640, 480
    F = _frames(w, h)
    fm = _handle(w, h)
    probe = [("noise45", "noise45b"), ("dots4", "synth0a"), ("weak_dots", "synth2b"), ("noise30", "checker2"),
             ("synth4a", "synth4b"), ("salt", "noise20b")]
    want = ["loud" if F.expected(a, b) is None else "exact" for a, b in probe]
    seen = {}
    for i, p in enumerate(probe):
        num, lists = fm.match_batch_raw([F.img[p[0]]], [F.img[p[1]]], cap=2048)
        seen.setdefault(i, []).append(("alone", _outcome(num, lists, F, [p], 0)))
    batch8 = probe + [("noise16", "noise45"), ("saturated", "synth5a")]
    num, lists = fm.match_batch_raw([F.img[a] for a, _ in batch8], [F.img[b] for _, b in batch8], cap=2048)
    for i in range(len(probe)):
        seen[i].append(("batch of 8", _outcome(num, lists, F, batch8, i)))
    fill = _mixed_pairs(F, MAX_PAIRS - len(probe), seed=31, noise_share=0.7)
    for at in (0, 41):
        batch = fill[:at] + probe + fill[at:]
        num, lists = fm.match_batch_raw([F.img[a] for a, _ in batch], [F.img[b] for _, b in batch], cap=2048)
        for i in range(len(probe)):
            seen[i].append(("batch of 64 at %d" % at, _outcome(num, lists, F, batch, at + i)))
    bad = ["%s: want %s, got %s" % (probe[i], want[i], seen[i]) for i in seen if any(o != want[i] for _, o in seen[i])]
    assert not bad, "\n".join(bad)
    fm.close()


def test_noise_batches_take_the_dense_pass_with_more_maxima_than_the_primary_list():
    """What makes the tests above cover the dense second pass of a streaming call: in a batch of noise (and weak-dot)
    frames, levels end up listed at fastThreshold (fast_tau = 20: the dense pass) while the oracle counts more maxima
    there than the level's primary list holds -- and the pairs are still the oracle's."""
    w, h = 1280, 720
    F = _frames(w, h)
    names = F.noise + ["weak_dots"]
    pairs = [(names[i % len(names)], names[(i + 3) % len(names)]) for i in range(8)]
    fm = _handle(w, h, pairs=8)
    num, lists = fm.match_batch_raw([F.img[a] for a, _ in pairs], [F.img[b] for _, b in pairs], cap=2048)
    frames = [a for a, _ in pairs] + [b for _, b in pairs]
    tau = np.stack([fm.fast_tau(s) for s in range(len(frames))])               # [frame, level, (final, first)]
    dense_over = []
    for s, name in enumerate(frames):
        c = oc.capacity(F.img[name])
        lv = [l for l in c.primary_overflow if tau[s, l, 0] == 20]
        dense_over += [(name, l) for l in lv]
    print("levels at fastThreshold per frame:", (tau[:, :, 0] == 20).sum(1).tolist())
    print("first thresholds:", tau[:, :, 1].tolist())
    print("(frame, level) at fastThreshold with more maxima than the primary list:", dense_over)
    assert ((tau[:, :, 0] == 20).sum(1) >= 1).all()
    assert len(dense_over) >= 4, dense_over
    for i, (a, b) in enumerate(pairs):
        exp = F.orc.match(F.img[a], F.img[b])
        assert num[i] == len(exp) and np.array_equal(lists[i], exp), (i, a, b, num[i], len(exp))
    fm.close()
