"""CPU pins for tests/orb_capacity.py: every hard-input generator is what the GPU tests (tests/test_orb_capacity_gpu.py)
take it for, and the helper's capacities are the pipeline's.  If a generator is retuned so that it no longer sits where
it should, these fail before the GPU tests go vacuous."""
import os
import re

import numpy as np
import pytest

from mono_slam_framework_amd import synth
from tests import orb_capacity as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(640, 480), (1280, 720)]


def test_helper_caps_are_the_pipeline_caps():
    src = open(os.path.join(ROOT, "mono_slam_framework_amd", "csrc", "orb_plan.h")).read()
    assert int(re.search(r"constexpr int kKpCap = (\d+);", src).group(1)) == oc.KP_CAP
    assert int(re.search(r"constexpr int kS1Cap = (\d+);", src).group(1)) == oc.S1_CAP
    # the list sizes plan_orb computes, at the sizes the GPU tests use (tests/test_orb_plan_host.py holds the helper to
    # the compiled plan, level by level)
    assert [oc.full_list(w, h) for (w, h) in [(1280, 720), (1067, 600), (357, 201), (100, 60)]] == [115200, 80032, 8976, 4096]
    assert [oc.primary_list(w, h) for (w, h) in [(1280, 720), (1067, 600), (889, 500), (640, 480), (444, 333), (429, 241)]] == \
        [14400, 10016, 8192, 8192, 8192, 12928]


@pytest.mark.parametrize("w,h", SIZES, ids=["640x480", "1280x720"])
@pytest.mark.parametrize("name", sorted(oc.GENERATORS))
def test_generator_is_what_it_is_for(name, w, h):
    img = oc.frame(name, w, h)
    assert img.shape == (h, w) and img.dtype == np.uint8
    np.testing.assert_array_equal(img, oc.frame(name, w, h))           # deterministic
    c = oc.capacity(img)
    # the oracle's level sizes are the ones the helper's list sizes are computed for
    assert c.sizes[0] == (w, h) and len(c.sizes) == 8
    kind = oc.kind(name)
    if kind == "over":
        # over a cap that every call form meets: these must come back loud everywhere
        assert c.loud, c
    else:
        assert not c.over, c
    if name in oc.DENSE_PASS:
        # many maxima at fastThreshold, few stage-1 key points: a level that takes the dense pass in a streaming call
        # holds more maxima than its primary list, and its stage 1 still fits
        assert c.primary_overflow, c
        assert max(c.stage1) < 1000, c
    if kind == "flat":
        assert min(c.maxima) == 0, c                                  # some levels without a corner
    if name == "constant" or name == "gradient":
        assert sum(c.maxima) == 0 and c.kp == 0, c
    if name == "weak_dots":
        # most corners just above fastThreshold (scores 20..23), a thin strong tail
        o = oc._oracle(w, h)
        s = o.fast_candidates(0)[:, 2]
        assert (s <= 23).mean() > 0.9 and (s > 30).sum() > 0, np.bincount(s)[20:40]


@pytest.mark.parametrize("w,h", SIZES, ids=["640x480", "1280x720"])
def test_synth_frames_are_within_caps(w, h):
    A, B = synth.synth_batch(700, 3, w, h)
    for img in list(A) + list(B):
        c = oc.capacity(img)
        assert not c.over, c


def test_capacity_names_the_cap_that_is_exceeded():
    c = oc.capacity(oc.frame("dots4", 640, 480))
    # dots on a 4 px lattice: every dot a tied FAST maximum of level 0
    assert c.stage1[0] > oc.S1_CAP and c.kp > oc.KP_CAP
    assert any(r.startswith("L0 stage 1") for r in c.loud) and any(r.startswith("key points") for r in c.loud)
    assert not c.dense_only
    c = oc.Capacity([(640, 480)] + [(100, 60)] * 7, [40000] + [0] * 7, [10] + [0] * 7, 10)
    assert c.over and not c.loud and c.dense_only == ["L0 maxima 40000 > full list 38400"]
