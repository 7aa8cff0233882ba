"""CPU: pins the float64 matching-head reference (oracle/loftr_head.py) that tests/test_loftr_head_gpu.py holds the GPU
head to.  On the golden features it must reproduce the ONNX graph's confidences (tests/golden/loftr_kat.npz), and on
a synth pair the CPU restatement's (oracle/libloftr_oracle.so) from that restatement's own features."""
import os

import numpy as np
import pytest

from oracle import loftr_head

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "loftr_kat.npz"))


@pytest.mark.parametrize("name", ["i", "ii", "iii", "synth"])
def test_reference_reproduces_the_onnx_golden(name):
    f0, f1 = G["feat0_" + name], G["feat1_" + name]
    _, conf, ij = loftr_head.head(f0, f1, 0.15)
    si, sv = G["samp_ij_" + name].astype(int), G["samp_v_" + name]
    bi, bv = G["big_ij_" + name].astype(int), G["big_v_" + name]
    assert np.abs(conf[si[:, 0], si[:, 1]] - sv).max() <= 3e-6
    if len(bv):
        assert np.abs(conf[bi[:, 0], bi[:, 1]] - bv).max() <= 3e-6
    assert np.abs(conf.sum(1) - G["rowsum_" + name]).max() <= 3e-6
    assert np.abs(conf.sum(0) - G["colsum_" + name]).max() <= 3e-6
    # the golden lists (no golden confidence sits within 1e-5 of these thresholds)
    for thr, tag in ((0.15, "015"), (0.1, "010")):
        _, _, ij = loftr_head.head(f0, f1, thr)
        np.testing.assert_array_equal(loftr_head.cells(ij), G["matches_%s_%s" % (name, tag)])


@pytest.mark.parametrize("name", ["i", "ii", "iii", "synth"])
def test_band_is_ten_times_tighter_than_the_end_to_end_bar(name):
    """rho at thr = 0.15 must stay below 1e-4 absolute on realistic features (the end-to-end bar is 1e-3)"""
    r = loftr_head.rho(G["feat0_" + name], G["feat1_" + name])
    assert 0.15 * np.expm1(r) < 1e-4, r


def test_reference_reproduces_the_c_restatement():
    from mono_slam_framework_amd import synth
    from oracle import loftr
    a, b = synth.synth_pair(3, 640, 480, mode=1)
    r = loftr.DNNFeatureMatcherOracle(0.15).run(a, b)
    _, conf, ij = loftr_head.head(r["feat0"], r["feat1"], 0.15)
    assert np.abs(conf - r["conf"]).max() <= 3e-6
    assert len(ij) > 10


def test_reference_on_flat_features():
    """equal tokens: every confidence is 1 / 1200^2; rho is finite and small"""
    f = np.ones((1200, 32), np.float32)
    s, conf, ij = loftr_head.head(f, f, 6.9e-7)
    np.testing.assert_allclose(conf, 1.0 / 1200 ** 2, rtol=1e-12)
    assert len(ij) == 1200 * 1200
    assert loftr_head.head(np.zeros_like(f), f, 0.05)[2].shape == (0, 2)
    flagged, clear = loftr_head.single_pass_flagged(f, f)
    assert not flagged and clear
