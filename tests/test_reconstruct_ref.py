"""CPU: the reference side of the reconstruction tests (tests/initializer_ref.py) against planted motion, the
preconditions the GPU and host tests rest on, the float64 / float32 spread that sizes the parallax bar, and the literal
quirks of the two selection rules (slam_pipeline/src/Initializer.cc:524-582, 700-741) on hand-made counts."""
import os

import numpy as np
import pytest

from tests import initializer_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ("two_view", "wide"))
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_planted_f_gives_every_inlier_to_one_candidate(kind, seed):
    F, R, t = ir.planted_f(kind)
    m, bad = ir.scene(kind, seed)
    ref = ir.reconstruct(1, F, m, ~bad)
    goods = [c["nGood"] for c in ref["checks"]]
    n_in = int((~bad).sum())
    print("%s seed %d: nGood %s of %d planted inliers, parallax %s" % (kind, seed, goods, n_in,
                                                                      [round(float(c["parallax"]), 3) for c in ref["checks"]]))
    assert ref["ok"] == 1 and sorted(goods)[:3] == [0, 0, 0] and max(goods) >= 0.97 * n_in
    Rw, tw = ref["cands"][ref["winner"]]
    assert np.abs(Rw - R).max() < 1e-4 and np.abs(tw - t).max() < 1e-4          # the planted motion, f32 F apart
    chk = ref["checks"][ref["winner"]]
    assert (chk["points"][chk["counted"]][:, 2] > 0).all()
    if kind == "wide":
        assert 14 < chk["parallax"] < 16


@pytest.mark.parametrize("kind,seed", ir.CASES)
def test_preconditions(kind, seed):
    c = ir.case(kind, seed)
    ref, ref32 = ir.case_reference(kind, seed), ir.case_reference(kind, seed, True)
    assert abs(c["RH"] - 0.40) >= 0.07                                         # the choice of the model is not in question
    assert c["model"] == (0 if kind == "planar" else 1)
    assert ref["ok"] == ref32["ok"] == ir.EXPECT_OK[(kind, seed)]
    n_in = int(c["H" if c["model"] == 0 else "F"]["inliers"].sum())
    goods = sorted(k["nGood"] for k in ref["checks"])
    worst = max(int(k["borderline"].sum()) for k in ref["checks"])
    print("%s seed %d: RH %.3f, N %d, singular values %s, nGood %s, most borderline matches under a candidate %d"
          % (kind, seed, c["RH"], n_in, np.round(ref["w"], 4).tolist(), [k["nGood"] for k in ref["checks"]], worst))
    assert worst <= ir.MAX_BORDERLINE_SHARE * n_in
    if ref["ok"]:
        assert goods[-1] - goods[-2] >= ir.MIN_WINNER_MARGIN
    # the float32 run of the reference decides every flag as the float64 run does
    perm, _, _ = ir.compare_candidates(ref, [k[0] for k in ref32["cands"]], [k[1] for k in ref32["cands"]])
    for i, j in enumerate(perm):
        np.testing.assert_array_equal(ref32["checks"][i]["counted"], ref["checks"][j]["counted"])
        np.testing.assert_array_equal(ref32["checks"][i]["good"], ref["checks"][j]["good"])


def test_spread_sizes_the_parallax_bar():
    spread = ir.parallax_spread()
    cand = 0.0
    for kind, seed in ir.CASES:
        ref, ref32 = ir.case_reference(kind, seed), ir.case_reference(kind, seed, True)
        _, worst, bound = ir.compare_candidates(ref, [k[0] for k in ref32["cands"]], [k[1] for k in ref32["cands"]])
        cand = max(cand, worst / bound)
    text = ("float64 / numpy-float32 spread of the reference over %d cases\n"
            "parallax: largest |p32 - p64| = %.3e degrees; bar = 2 x %.1e = %.2e\n"
            "candidates: largest max(|R32 - R64|, |t32 - t64|) = %.3f of its bound\n"
            % (len(ir.CASES), spread, ir.MEASURED_PARALLAX_SPREAD, ir.PARALLAX_BAR, cand))
    print(text)
    try:
        with open(os.path.join(ROOT, "profiles", "reconstruct_bars.txt"), "w") as f:
            f.write(text)
    except OSError:
        pass                                                                    # a read-only checkout still runs the test
    assert spread <= ir.MEASURED_PARALLAX_SPREAD
    assert spread >= 0.5 * ir.MEASURED_PARALLAX_SPREAD                          # the pasted figure is the measured one
    assert cand <= 1.0


def test_quirks_of_the_selection_rules():
    f, h = ir.pick_f, ir.pick_h
    par = [np.float32(5)] * 8
    # F: nMinGood = MAX(0.9 N, minTriangulated)
    assert f([100, 0, 0, 0], par, 200, 50, 1.0) == -1                          # 100 < 0.9 * 200
    assert f([180, 0, 0, 0], par, 200, 50, 1.0) == 0
    assert f([40, 0, 0, 0], par, 40, 50, 1.0) == -1                            # 40 >= 36 but < minTriangulated
    # H: minGood = MIN(0.9 N, minTriangulated)
    assert h([100, 0, 0, 0, 0, 0, 0, 0], par, 200, 50, 1.0) == 0               # 100 >= min(180, 50)
    assert h([40, 0, 0, 0, 0, 0, 0, 0], par, 40, 50, 1.0) == 0                 # 40 >= min(36, 50)
    assert h([35, 0, 0, 0, 0, 0, 0, 0], par, 40, 50, 1.0) == -1
    # F: parallax > minParallax; H: parallax >= minParallax
    one = [np.float32(1)] * 8
    assert f([180, 0, 0, 0], one, 200, 50, 1.0) == -1
    assert h([180, 0, 0, 0, 0, 0, 0, 0], one, 200, 50, 1.0) == 0
    # F: nsimilar counts nGood > 0.7 maxGood, the maximum itself included
    assert f([180, 127, 0, 0], par, 200, 50, 1.0) == -1                        # 127 > 126
    assert f([180, 126, 0, 0], par, 200, 50, 1.0) == -1                        # 0.7 * 180 = 125.99999999999999 in double
    assert f([180, 125, 0, 0], par, 200, 50, 1.0) == 0
    # F: the else-if chain looks at the FIRST candidate that reaches maxGood only (a tie also has nsimilar = 2)
    assert f([0, 0, 0, 190], [np.float32(0)] * 3 + [np.float32(5)], 200, 50, 1.0) == 3
    # F with nothing counted anywhere: 0 < 0 and 0 > 0 are false, so the chain reaches candidate 1 and its parallax decides
    assert f([0, 0, 0, 0], par, 0, 0, 1.0) == 0
    assert f([0, 0, 0, 0], [np.float32(0)] * 4, 0, 0, 1.0) == -1               # CheckRT's parallax for nGood = 0
    # H: the first strict maximum; nothing counted leaves bestParallax at -1
    assert h([0, 90, 90, 0, 0, 0, 0, 0], par, 100, 50, 1.0) == 1
    assert h([0] * 8, par, 0, 0, 1.0) == -1
    assert h([0] * 8, par, 0, 0, -1.0) == 0                                    # -1 >= -1 and 0 >= 0: the reference says yes


def test_early_return_on_the_identity():
    """H = I: d1 / d2 = 1 < 1.00001"""
    c = ir.case("planar", 1)
    ref = ir.reconstruct(0, np.eye(3, dtype=np.float32), c["matches"], c["H"]["inliers"])
    assert ref["early"] and ref["ok"] == 0 and not ref["cands"]
