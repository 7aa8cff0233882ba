"""GPU: k_pose_optimize (csrc/pose_kernels.hip) through msf_pose_optimize / msf_pose_optimize_device --
Optimizer::PoseOptimization's four Levenberg-Marquardt rounds and chi2 flags -- against the float64 reference of
tests/pose_ref.py, bar by bar (the sums from the device's own entry estimates, every iteration replayed from the
device's own H, b and lambda, the flags from the device's own round poses, the final pose against the reference); the
sizes of the early-outs, of the 10-edge break and of the lanes' strides; a mask; the batch against its list-by-list
replay and the host-pointer entry, bit for bit; strided entry poses and masks taken from a PnP result."""
import numpy as np
import pytest

from tests import pnp_ref
from tests import pose_ref as pr

pytestmark = pytest.mark.gpu

SIZES = [0, 2, 3, 9, 10, 63, 64, 65, 128, 129, 257, 1025, 4097, 8192]    # the last three: 17, 65 and 128 strides of a lane
SENTINEL = {"uint8": 0xAB, "int32": -77, "float32": -77.0, "float64": -77.0}


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.7, 640, 480)
    yield m
    m.close()


@pytest.mark.parametrize("kind,seed", pr.CASES)
def test_scenes_meet_the_float64_bars(fm, kind, seed):
    sc = pr.scene(kind, seed)
    got = fm.pose_optimize(sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"])
    clear, run = pr.check_result(got, sc, "device %s seed %d" % (kind, seed), scene_conditions=True)
    print("%s seed %d: %d clear iterations of %d" % (kind, seed, clear, run))
    assert (got["outliers"].astype(bool) == sc["outlier"]).all()


@pytest.mark.parametrize("n", SIZES)
def test_sizes(fm, n):
    sc = pr.scene("base", 2, n)
    got = fm.pose_optimize(sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"])
    pr.check_result(got, sc, "device n %d" % n)
    assert got["rounds_run"] == (0 if n < 3 else 1 if n < 10 else 4)


def test_mask_with_every_third_entry_out(fm):
    sc = pr.scene("wide", 2)
    mask = (np.arange(pr.N_SCENE) % 3 != 0).astype(np.uint8)
    got = fm.pose_optimize(sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"], mask=mask)
    pr.check_result(got, sc, "device masked", mask=mask)
    assert got["n_edges"] == 64 and not got["outliers"][mask == 0].any()
    none = fm.pose_optimize(sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"], mask=np.zeros(pr.N_SCENE, np.uint8))
    assert none["n_good"] == 0 and none["rounds_run"] == 0 and none["Tcw"].tobytes() == sc["Tcw0"].tobytes()


def _batch(n_lists):
    """lists of differing lengths, entry poses and masks; among twenty: one without a valid result, a 2-point list and
    a clipped one"""
    sizes = [96, 17, 64][:n_lists] if n_lists <= 3 else [(96, 17, 64, 9, 257, 33)[i % 6] for i in range(n_lists)]
    cap = 96 if n_lists <= 3 else 130
    scenes = [pr.scene(("base", "wide", "shallow")[i % 3], 1 + i % 3, n) for i, n in enumerate(sizes)]
    d_n = list(sizes)                                 # 257 > cap: the clipped list
    if n_lists == 20:
        d_n[7], d_n[9] = -1, 2
    masks = [(np.arange(cap) % 4 != 1).astype(np.uint8) if i % 5 == 2 else np.ones(cap, np.uint8) for i in range(n_lists)]
    return scenes, d_n, cap, masks


def _run_batch(fm, scenes, d_n, cap, masks, order):
    """the lists `order` of the batch in one device call, every output pre-filled with a sentinel -> numpy dict"""
    import torch
    from mono_slam_framework_amd import _lib
    L = len(order)
    p3 = np.full((L, cap, 3), 7.5, np.float32)
    p2 = np.full((L, cap, 2), 7.5, np.float32)
    t0 = np.zeros((L, 12), np.float32)
    mk = np.zeros((L, cap), np.uint8)
    for row, i in enumerate(order):
        k = min(len(scenes[i]["p3d"]), cap)
        p3[row, :k], p2[row, :k] = scenes[i]["p3d"][:k], scenes[i]["p2d"][:k]
        t0[row], mk[row] = scenes[i]["Tcw0"], masks[i]
    out = {name: torch.from_numpy(np.full(shape, SENTINEL[dt], dt)).cuda() for name, (shape, dt) in _lib.pose_shapes(L, cap).items()}
    got = fm.pose_optimize_device(torch.from_numpy(p3).cuda(), torch.from_numpy(p2).cuda(),
                                  torch.tensor([d_n[i] for i in order], dtype=torch.int32, device="cuda"), scenes[0]["K"],
                                  torch.from_numpy(t0).cuda(), d_mask=torch.from_numpy(mk).cuda(), out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("n_lists", [1, 3, 20])
def test_batch_equals_its_replay(fm, n_lists):
    from mono_slam_framework_amd import _lib
    scenes, d_n, cap, masks = _batch(n_lists)
    order = list(range(n_lists))
    got = _run_batch(fm, scenes, d_n, cap, masks, order)
    names = [a[0] for a in _lib.POSE_ARRAYS]
    per = {a[0]: a[2] for a in _lib.POSE_ARRAYS}
    sentinel = lambda name: np.array(SENTINEL[str(got[name].dtype)], got[name].dtype)
    for i in order:
        if d_n[i] < 0:                                # no valid result: n_good alone is written
            assert got["n_good"][i] == -1
            for k in names[1:]:
                assert (got[k][i] == sentinel(k)).all(), (i, k)
            continue
        n = min(d_n[i], cap)
        edge = masks[i][:n].astype(bool)
        # bytes beyond the list and outside the mask: untouched
        assert (got["outliers"][i, n:] == 0xAB).all() and (got["outliers"][i, :n][~edge] == 0xAB).all(), i
        assert (got["outliers"][i, :n][edge] <= 1).all(), i
        rounds = int(got["rounds_run"][i])
        assert rounds == (0 if edge.sum() < 3 else 1 if edge.sum() < 10 else 4), i
        ran = got["it_trials"][i] != 0
        assert (got["round_pose_f64"][i, rounds:] == -77.0).all(), i
        for k in names:
            if per[k] == "it" and k != "it_trials":
                assert (got[k][i][~ran] == -77.0).all(), (i, k)
        # the host entry on the same list: bit for bit where the device call writes
        sc = scenes[i]
        host = fm.pose_optimize(sc["p3d"][:n], sc["p2d"][:n], sc["K"], sc["Tcw0"], mask=masks[i][:n])
        assert not host["outliers"][~edge].any()
        for k in names:
            mine, theirs = got[k][i], np.asarray(host[k], got[k].dtype)
            if k == "outliers":
                mine, theirs = mine[:n][edge], theirs[edge]
            elif k == "round_pose_f64":
                mine, theirs = mine[:rounds], theirs[:rounds]
            elif per[k] == "it" and k != "it_trials":
                mine, theirs = mine[ran], theirs[ran]
            assert np.ascontiguousarray(mine).tobytes() == np.ascontiguousarray(theirs).tobytes(), (i, k)
    # the bars on two lists of the batch, from what the batch returned
    for i in ([0] if n_lists == 1 else [0, 2]):
        n = min(d_n[i], cap)
        one = {k: got[k][i] for k in names}
        for k in ("n_good", "n_edges", "rounds_run"):
            one[k] = int(one[k])
        one["outliers"] = np.where(masks[i][:n] != 0, one["outliers"][:n], 0).astype(np.uint8)
        sc = {k: (v[:n] if k in ("p3d", "p2d", "outlier") else v) for k, v in scenes[i].items()}
        pr.check_result(one, sc, "device batch of %d, list %d" % (n_lists, i), mask=masks[i][:n])
    if n_lists == 1:
        return
    # any order, and every list alone gives what it gave in the batch
    order2 = list(np.random.default_rng(n_lists).permutation(n_lists))
    again = _run_batch(fm, scenes, d_n, cap, masks, order2)
    for row, i in enumerate(order2):
        for k in names:
            assert got[k][i].tobytes() == again[k][row].tobytes(), (i, k)
    for i in order2:
        alone = _run_batch(fm, scenes, d_n, cap, masks, [i])
        for k in names:
            assert got[k][i].tobytes() == alone[k][0].tobytes(), (i, k)


def test_strided_entry_poses_and_masks_from_a_pnp_result(fm):
    """Tcw_refined / inliers_refined of pnp_ransac_device, pointed at with their strides, against the same data as copies"""
    import torch
    from mono_slam_framework_amd import _lib
    L, cap, its, max_records = 3, 100, 35, 4
    scenes = [pr.scene("base", 1 + i) for i in range(L)]
    p3 = np.zeros((L, cap, 3), np.float32)
    p2 = np.zeros((L, cap, 2), np.float32)
    for i, sc in enumerate(scenes):
        p3[i, :pr.N_SCENE], p2[i, :pr.N_SCENE] = sc["p3d"], sc["p2d"]
    d_p3, d_p2 = torch.from_numpy(p3).cuda(), torch.from_numpy(p2).cuda()
    d_n = torch.full((L,), pr.N_SCENE, dtype=torch.int32, device="cuda")
    m, _ = pnp_ref.set_ransac_parameters(pr.N_SCENE)
    pnp = fm.pnp_ransac_device(d_p3, d_p2, d_n, scenes[0]["K"], m, its, max_records=max_records, seed=3)
    torch.cuda.synchronize()
    assert (pnp["n_records"] >= 1).all()
    rec = 1 if bool((pnp["n_records"] >= 2).all()) else 0
    tcw_view, mask_view = pnp["Tcw_refined"][:, rec], pnp["inliers_refined"][:, rec]
    assert not tcw_view.is_contiguous() and not mask_view.is_contiguous()
    strided = fm.pose_optimize_device(d_p3, d_p2, d_n, scenes[0]["K"], tcw_view, d_mask=mask_view,
                                      Tcw0_stride=max_records * 12, mask_stride=max_records * cap)
    copies = fm.pose_optimize_device(d_p3, d_p2, d_n, scenes[0]["K"], tcw_view.contiguous(), d_mask=mask_view.contiguous())
    torch.cuda.synchronize()
    for k in strided:
        assert strided[k].cpu().numpy().tobytes() == copies[k].cpu().numpy().tobytes(), k
    # and they are what the host entry gives on the copies
    for i, sc in enumerate(scenes):
        mask = mask_view[i, :pr.N_SCENE].cpu().numpy()
        host = fm.pose_optimize(sc["p3d"], sc["p2d"], sc["K"], tcw_view[i].cpu().numpy(), mask=mask)
        assert host["Tcw"].tobytes() == strided["Tcw"][i].cpu().numpy().tobytes()
        assert host["n_good"] == int(strided["n_good"][i]) and host["n_edges"] == int(mask.astype(bool).sum())
        assert host["n_good"] >= 55                   # PnP's refined pose and inliers lead to the scene's pose
        assert _lib.POSE_ARRAYS[0][0] == "n_good"


def test_argument_checks(fm):
    from mono_slam_framework_amd.matcher import MsfError
    sc = pr.scene("base", 1, 16)
    with pytest.raises(MsfError) as e:
        fm.pose_optimize(sc["p3d"], sc["p2d"], sc["K"], sc["Tcw0"], chi2=float("nan"))
    assert e.value.code == -1 and "chi2" in fm.last_error()
    import torch
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises((MsfError, AssertionError)):
        fm.pose_optimize_device(z(1, 4, 3), z(1, 4, 2), d_n, sc["K"], z(12), Tcw0_stride=-12)
