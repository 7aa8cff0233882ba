"""CPU: the reference of the new-map-point tests alone (tests/local_mapping_ref.py).  The caps are conditions on the
inputs, not measurements: the scenes must leave few matches at a threshold and few null vectors without an informative
bar, must exercise every stage, and a numpy float32 SVD of the same matrices must agree with the float64 one on every
match that is not borderline -- otherwise a comparison of f32 device code against float64 would say nothing."""
import numpy as np
import pytest

from tests import initializer_ref as ir
from tests import local_mapping_ref as lm
from tests import ransac_ref as rr


@pytest.mark.parametrize("seed,max_cos", lm.CASES)
def test_scene_conditions(seed, max_cos):
    refs = lm.scene_reference(seed, max_cos)
    n = lm.N_NEIGHBOURS * lm.N_MATCHES
    border = sum(int(r["borderline"].sum()) for r in refs)
    unin = sum(int(r["uninformative"].sum()) for r in refs)
    reached = sum(int(r["reached"].sum()) for r in refs)
    accepted = sum(r["n_new"] for r in refs)
    worst = max(float(np.nanmax(np.where(r["uninformative"], 0, np.where(r["reached"], r["bound"], 0)))) for r in refs)
    print("seed %d max_cos %g: accepted %.3f, borderline %.4f, uninformative %.4f of %d reached, largest informative bound %.2e"
          % (seed, max_cos, accepted / n, border / n, unin / max(reached, 1), reached, worst))
    print("  status histogram:", np.bincount(np.concatenate([r["status"] for r in refs]), minlength=8))
    assert border <= ir.MAX_BORDERLINE_SHARE * n
    assert unin <= rr.MAX_UNINFORMATIVE_SHARE * max(reached, 1)
    assert accepted >= 0.2 * n                      # the scene is no degenerate one: a good part becomes map points


def test_every_status_occurs():
    seen = set()
    for seed, max_cos in lm.CASES:
        for r in lm.scene_reference(seed, max_cos):
            seen |= set(int(s) for s in r["status"])
    hand = lm.handmade_reference()
    assert list(hand["status"]) == [3, 1, 0], hand["status"]
    assert hand["hom"][0, 3] == 0                   # the zero column: exactly (0, 0, +-1, 0) in float64 too
    seen |= set(int(s) for s in hand["status"])
    assert seen == set(range(8)), seen


@pytest.mark.parametrize("seed,max_cos", lm.CASES)
def test_float32_svd_agrees_off_the_borderline(seed, max_cos):
    r64, r32 = lm.scene_reference(seed, max_cos), lm.scene_reference(seed, max_cos, True)
    worst = 0.0
    for a, b in zip(r64, r32):
        keep = ~a["borderline"]
        assert np.array_equal(a["status"][keep], b["status"][keep]), np.flatnonzero(keep & (a["status"] != b["status"]))
        rows = a["reached"] & ~a["uninformative"]
        h = b["hom"][rows].astype(np.float64)
        h /= np.linalg.norm(h, axis=1, keepdims=True)
        v = a["hom"][rows]
        err = np.minimum(np.linalg.norm(h - v, axis=1), np.linalg.norm(h + v, axis=1))
        worst = max(worst, float((err / a["bound"][rows]).max()))
    print("seed %d max_cos %g: numpy float32 null vector worst err / bound %.3f" % (seed, max_cos, worst))
    assert worst <= 1.0


def test_handmade_point_is_where_it_was_put():
    v1, v2, m = lm.handmade()
    ref = lm.handmade_reference()
    assert np.allclose(ref["points"][2], [0.5, 0.0, 5.0], atol=1e-5)
