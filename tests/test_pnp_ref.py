"""CPU: tests/pnp_ref.py, the float64 restatement of PnPsolver, against its own invariants: the stages agree with each
other, an exact scene gives back its pose, the literal qr_solve solves least squares, SetRansacParameters' adjustment,
the record rule; and the measurement that sizes bar 3 (profiles/pnp_bars.txt)."""
import os

import numpy as np
import pytest

from tests import pnp_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_scene(seed, n):
    """a scene whose 2-D points are the exact projections (no truncation, no outliers)"""
    sc = pr.scene("base", seed, n)
    cam = sc["p3d"].astype(np.float64) @ sc["R"].T + sc["t"]
    K = sc["K"].astype(np.float64)
    us = np.stack([K[2] + K[0] * cam[:, 0] / cam[:, 2], K[3] + K[1] * cam[:, 1] / cam[:, 2]], 1)
    return sc, sc["p3d"].astype(np.float64)[None], us[None]


@pytest.mark.parametrize("n", [6, 30, 96])
def test_exact_projections_give_back_the_pose(n):
    sc, pw, us = exact_scene(4, n)
    out = pr.epnp(pw, us, sc["K"])
    dr, dt = pr.pose_distance(out["pose"][0], sc["R"], sc["t"])
    print("n %d: |R - truth| %.2e, |t - truth| %.2e, rep %s" % (n, dr, dt, out["rep"][0]))
    assert dr < 1e-7 and dt < 1e-6
    assert out["rep"][0].min() < 1e-6
    assert out["lam"][0, 11] <= 1e-9 * out["lam"][0, 0]          # one null vector: the solution


def test_stages_agree():
    sc = pr.scene("base", 1)
    pw, us = pr.gather(sc, pr.draw_sets(1, pr.N_SCENE, 20))
    cws, lam = pr.control_points(pw)
    a = pr.barycentric(cws, pw)
    assert np.abs(a.sum(-1) - 1).max() < 1e-12
    assert np.abs(np.einsum("hnj,hjk->hnk", a, cws) - pw).max() < 1e-9     # the control points reproduce the points
    assert (np.diff(lam, axis=1) <= 0).all()
    m = pr.fill_m(a, us, sc["K"])
    lam12, ut = pr.basis_eigh(np.einsum("hri,hrj->hij", m, m))
    assert np.abs(ut @ ut.transpose(0, 2, 1) - np.eye(12)).max() < 1e-13
    assert np.abs(np.einsum("hri,hki->hrk", m, ut[:, 8:])).max() < 1e-6 * np.sqrt(lam12[:, 0]).max()   # M's null space
    rho = pr.compute_rho(cws)
    assert np.allclose(rho[:, :3], (lam / 4) , rtol=1e-9)                   # |c_i - c_0|^2 = dc_i / n


def test_qr_solve_is_least_squares_and_skips_a_singular_step():
    rng = np.random.default_rng(3)
    A, b = rng.normal(size=(50, 6, 4)), rng.normal(size=(50, 6))
    x = pr.qr_solve(A, b)
    want = np.stack([np.linalg.lstsq(A[i], b[i], rcond=None)[0] for i in range(50)])
    assert np.abs(x - want).max() < 1e-11
    A[7] = 0
    assert (pr.qr_solve(A, b)[7] == 0).all()
    assert np.abs(pr.lstsq_cut(A[:5], b[:5]) - want[:5]).max() < 1e-12
    rank1 = np.outer(np.arange(1.0, 4), np.arange(2.0, 5))
    assert np.abs(pr.pinv_cut(rank1[None])[0] - np.linalg.pinv(rank1)).max() < 1e-14


def test_set_ransac_parameters():
    assert pr.set_ransac_parameters(96, 0.99, 10, 300, 4, 0.5) == (48, 35)
    assert pr.set_ransac_parameters(4, 0.99, 4, 300, 4, 0.5) == (4, 1)
    assert pr.set_ransac_parameters(15, 0.99, 10, 300, 4, 0.5) == (10, 14)


def test_record_rule():
    assert pr.records_of([3, 10, 10, 12, 11, 40], 10) == [1, 3, 5]
    assert pr.records_of([9, 9], 10) == []


@pytest.mark.parametrize("kind,seed", pr.CASES)
def test_scenes_behave_as_described(kind, seed):
    sc = pr.scene(kind, seed)
    sets = pr.draw_sets(seed, pr.N_SCENE, pr.N_ITERATIONS)
    pw, us = pr.gather(sc, sets)
    out = pr.epnp(pw, us, sc["K"])
    e2 = pr.error2(out["pose"], sc["p3d"], sc["p2d"], sc["K"])
    counts = (e2 < float(pr.TH2)).sum(1)
    rec = pr.records_of(counts, 48)
    print("%s seed %d: best count %d, records at %s" % (kind, seed, counts.max(), rec))
    assert (p2d_is_integer := (sc["p2d"] == np.floor(sc["p2d"])).all())
    if kind == "few":
        assert not rec
    if kind == "base":
        assert rec and counts.max() >= 55


def test_spread_sizes_the_pose_bar():
    worst, judged, left, median = pr.measure_pose_spread()
    text = ("change of epnp_from's (R, t) under a 16 eps elementwise perturbation of cws and ut_tail, over %d hypotheses "
            "of %d scenes (%d ill-conditioned left out)\nlargest %.3e, median %.3e; bar 3 = 2 x %.1e = %.2e\n"
            % (judged, len(pr.CASES), left, worst, median, pr.MEASURED_POSE_SPREAD, pr.POSE_BAR))
    print(text)
    try:
        with open(os.path.join(ROOT, "profiles", "pnp_bars.txt"), "w") as f:
            f.write(text)
    except OSError:
        pass                                                                    # a read-only checkout still runs the test
    assert left <= pr.MAX_LEFT_OUT * (judged + left)
    assert worst <= pr.MEASURED_POSE_SPREAD
    assert worst >= 0.5 * pr.MEASURED_POSE_SPREAD                               # the pasted figure is the measured one
