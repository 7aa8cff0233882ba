"""CPU: the float64 reference of tests/pose_ref.py on its own -- it recovers every scene (the flags are the scene's
outliers), its stages agree with each other, the conditions of bar 2 hold on it, and the two measured bars
(STEP_BAR, POSE_BAR) are measured here on the reference, printed, written to profiles/pose_opt_bars.txt and held
against the constants pasted into pose_ref.py."""
import os

import numpy as np
import pytest

from tests import pose_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind,seed", pr.CASES)
def test_the_reference_recovers_the_scene(kind, seed):
    sc = pr.scene(kind, seed)
    truth = np.concatenate([sc["R"], sc["t"][:, None]], 1).reshape(12)
    assert 0.01 < np.abs(sc["Tcw0"] - truth).max() <= 0.1 + 0.05 * (1 + np.abs(sc["t"]).max())
    ref = pr.reference(sc)
    assert ref["rounds_run"] == 4 and ref["n_edges"] == pr.N_SCENE
    assert (ref["outliers"] == sc["outlier"]).all()
    assert ref["n_good"] == int((~sc["outlier"]).sum())
    assert np.abs(ref["pose_f64"] - truth).max() < 0.02
    # rounds 1..3 leave out what the round before flagged
    for rnd in range(1, 4):
        assert (ref["rounds"][rnd]["active"] == ~ref["rounds"][rnd - 1]["flags"]).all()


def test_stages_agree():
    sc = pr.scene("base", 1)
    est = pr.estimate_of(sc["Tcw0"])
    assert abs(est[0] @ est[0] - 1) < 4 * pr.EPS and est[0][3] >= 0
    assert np.abs(pr.matrix_of(est) - sc["Tcw0"].astype(np.float64)).max() < 1e-6     # an f32 rotation is orthogonal to 1e-7
    h21, b, c, mag = pr.system(est, sc["p3d"], sc["p2d"], sc["K"], True)
    assert abs(c - pr.cost(est, sc["p3d"], sc["p2d"], sc["K"], True)) <= 8 * pr.EPS * c and (mag[:21] * (1 + 1e-12) >= np.abs(h21)).all()
    # b is minus half the gradient of the cost along exp(dx) T: central differences
    for k in range(6):
        dx = np.zeros(6)
        dx[k] = 1e-6
        up, down = (pr.cost(pr.moved(est, s * dx), sc["p3d"], sc["p2d"], sc["K"], True) for s in (1, -1))
        assert abs((up - down) / 2e-6 + 2 * b[k]) <= 1e-5 * max(1.0, abs(2 * b[k])), k
    dx = pr.solve_step(h21, b, 3.0)
    assert np.abs((pr.full(h21) + 3.0 * np.eye(6)) @ dx - b).max() <= 1e-9 * np.abs(b).max()
    assert pr.solve_step(-h21, b, 0.0) is None and pr.solve_step(h21 * np.nan, b, 1.0) is None
    # exp: a rotation, the small-angle branch, and V from the series
    R, t = pr.se3_exp(np.array([0.3, -0.2, 0.1, 1.0, 2.0, 3.0]))
    assert np.abs(R @ R.T - np.eye(3)).max() < 8 * pr.EPS and abs(np.linalg.det(R) - 1) < 8 * pr.EPS
    w = np.array([0.3, -0.2, 0.1])
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    V, term = np.eye(3), np.eye(3)
    for k in range(1, 30):
        term = term @ O / (k + 1)
        V = V + term
    assert np.abs(V @ np.array([1.0, 2.0, 3.0]) - t).max() < 1e-14
    R, t = pr.se3_exp(np.array([3e-6, 0, 0, 1.0, 0, 0]))
    assert R[1, 1] == 1 - 9e-12 and t[0] == 1.0                                       # I + Omega + Omega^2, V = R
    # Huber: continuous at delta^2, linear beyond
    rho, wgt = pr.robustify(np.array([1.0, 5.991, 5.992, 100.0]), True)
    assert rho[0] == 1 and wgt[0] == 1 and abs(rho[2] - 5.992) < 1e-6 and abs(rho[3] - (20 * pr.DELTA - 5.991)) < 1e-12
    assert pr.robustify(np.array([100.0]), False)[0][0] == 100.0


def test_early_outs_and_the_ten_edge_break():
    for n, rounds in ((0, 0), (2, 0), (3, 1), (9, 1), (10, 4)):
        sc = pr.scene("base", 2, n)
        sc["outlier"][:] = False
        ref = pr.pose_optimization(sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"])
        assert ref["rounds_run"] == rounds and ref["n_edges"] == n
        if rounds == 0:
            assert ref["n_good"] == 0 and ref["pose_f64"].tobytes() == sc["Tcw0"].astype(np.float64).tobytes()
    sc = pr.scene("base", 1)
    mask = np.arange(pr.N_SCENE) % 3 != 0
    ref = pr.pose_optimization(sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"], mask)
    assert ref["n_edges"] == mask.sum() and not ref["outliers"][~mask].any()
    assert (ref["outliers"][mask] == sc["outlier"][mask]).all()
    none = pr.pose_optimization(sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"], np.zeros(pr.N_SCENE, bool))
    assert none["n_good"] == 0 and none["rounds_run"] == 0


def test_the_measured_bars_and_the_conditions_of_bar_2():
    step, per_scene = pr.measure_step_spread()
    pose = pr.measure_pose_spread()
    clear, run = sum(c for c, _, _ in per_scene), sum(r for _, r, _ in per_scene)
    lines = ["STEP spread %r over %d clear iterations of %d run (per scene clear/run: %s)"
             % (float(step), clear, run, " ".join("%d/%d" % (c, r) for c, r, _ in per_scene)),
             "POSE spread %r over %d permutations per scene, %d scenes" % (float(pose), pr.PERMUTATIONS, len(pr.CASES))]
    print("\n".join(lines))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "pose_opt_bars.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    assert 0 < step <= pr.MEASURED_STEP_SPREAD and 0 < pose <= pr.MEASURED_POSE_SPREAD
    for (kind, seed), (c, r, first) in zip(pr.CASES, per_scene):
        assert first and 3 * c > r, (kind, seed, c, r)
    # the band of bar 3 is empty on the reference's round poses
    for kind, seed in pr.CASES:
        sc = pr.scene(kind, seed)
        for rd in pr.reference(sc)["rounds"]:
            chi2 = pr.chi2_of(rd["pose"], sc["p3d"], sc["p2d"], sc["K"])
            assert np.abs(chi2 / np.float64(pr.CHI2) - 1).min() > 1e-4
