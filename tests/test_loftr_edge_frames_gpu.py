"""GPU: the whole LoFTR path on edge-case frames against the CPU restatement (oracle/loftr.py) -- flat frames, noise, a
1-px checkerboard, a ramp, a frame against itself and against its negative -- as single calls on the split and the
exact-f32 handle, and at positions 0 and 8 of a 9-pair batch of synth pairs.  The existing bars: confidences of pair 0
within 1e-3 of the oracle, lists identical wherever no confidence is within 1e-3 of the threshold."""
import numpy as np
import pytest

from mono_slam_framework_amd import synth
from oracle import loftr as oracle_loftr
from tests.test_loftr_gpu import CONF_TOL, _check_lists

pytestmark = pytest.mark.gpu

H, W = 480, 640


def _frames(name):
    rng = np.random.default_rng(NAMES.index(name) + 31)
    a, _ = synth.synth_pair(77, W, H, mode=1)
    if name == "black":
        return np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    if name == "white":
        return np.full((H, W), 255, np.uint8), np.full((H, W), 255, np.uint8)
    if name == "grey":
        return np.full((H, W), 128, np.uint8), np.full((H, W), 128, np.uint8)
    if name == "noise":
        return rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    if name == "checker":
        c = ((np.add.outer(np.arange(H), np.arange(W)) & 1) * 255).astype(np.uint8)
        return c, c.copy()
    if name == "ramp":
        r = np.tile((np.arange(W) * 255 // (W - 1)).astype(np.uint8), (H, 1))
        return r, r.copy()
    if name == "self":
        return a, a.copy()
    if name == "negative":
        return a, (255 - a).astype(np.uint8)
    raise KeyError(name)


NAMES = ["black", "white", "grey", "noise", "checker", "ramp", "self", "negative"]
_ORACLE = {}


def _oracle_conf(name):
    if name not in _ORACLE:
        a, b = _frames(name)
        _ORACLE[name] = oracle_loftr.DNNFeatureMatcherOracle(0.15).run(a, b)["conf"]
    return _ORACLE[name]


def _dm(pairs, f32=False):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    f = _lib.MSF_FLAG_KEEP_DEBUG | _lib.MSF_FLAG_NO_FRAME_CACHE | (_lib.MSF_FLAG_LOFTR_F32 if f32 else 0)
    return DNNFeatureMatcher(threshold=0.15, max_batch_pairs=pairs, flags=f)


@pytest.mark.parametrize("name", NAMES)
def test_edge_frames_match_the_oracle(name):
    a, b = _frames(name)
    ref = _oracle_conf(name)
    worst = {}
    for label, f32 in (("split", False), ("f32", True)):
        dm = _dm(1, f32)
        got = dm.MatchFrames(a, b, cap=8192)
        d = float(np.abs(dm.conf_matrix() - ref).max())
        worst[label] = d
        assert d <= CONF_TOL, (label, d)
        _check_lists(got, ref, 0.15)
    A, B = synth.synth_batch(5200, 9, W, H, mode=1)
    for pos in (0, 8):
        fa, fb = list(A), list(B)
        fa[pos], fb[pos] = a, b
        dm = _dm(9)
        lists = dm.match_batch(fa, fb, cap=8192)
        _check_lists(lists[pos], ref, 0.15)
        if pos == 0:
            d = float(np.abs(dm.conf_matrix() - ref).max())
            worst["batch@0"] = d
            assert d <= CONF_TOL, d
    print("\n[%s] worst |dconf| %s, %d oracle matches" % (name, ", ".join("%s %.2e" % kv for kv in worst.items()),
                                                        int((ref > 0.15).sum())))
