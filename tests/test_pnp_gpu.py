"""GPU: k_pnp_hypotheses and k_pnp_records (csrc/pnp_kernels.hip) through msf_pnp_ransac / msf_pnp_ransac_device --
PnPsolver's RANSAC iterations and Refine -- against the float64 reference of tests/pnp_ref.py, bar by bar (control
points, basis, everything downstream of the device's own basis, counts and flags from the device's own poses, records
by integer logic, the refined pose against the truth); the sizes at which the lanes' strides can go wrong; the batch
against its list-by-list replay, bit for bit."""
import numpy as np
import pytest

from tests import pnp_ref as pr

pytestmark = pytest.mark.gpu

SIZES = [4, 5, 15, 16, 17, 63, 64, 65, 96, 257]
ITERATIONS = [1, 5, 35, 64, 65, 300]
PER_LIST = ("n_records", "counts", "iteration", "n_inliers", "refined_ok", "n_refined", "Tcw_best", "Tcw_refined",
            "inliers_best", "inliers_refined", "sets", "pose_f64", "cws", "ut_tail", "betas", "rep_errors", "pca",
            "rec_pose_f64", "rec_cws", "rec_ut_tail", "rec_betas", "rec_rep_errors", "rec_pca")


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.7, 640, 480)
    yield m
    m.close()


@pytest.mark.parametrize("kind,seed", pr.CASES)
def test_scenes_meet_the_float64_bars(fm, kind, seed):
    sc = pr.scene(kind, seed)
    sets = pr.draw_sets(seed, pr.N_SCENE, pr.N_ITERATIONS)
    m, its = pr.set_ransac_parameters(pr.N_SCENE)
    got = fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], m, its, sets=sets)
    ok = pr.check_result(got, sc, sets, m, 8, "device %s seed %d" % (kind, seed))
    if kind == "few":
        assert ok is None
    if kind == "base":                                # a record whose Refine succeeds, so bar 6 was evaluated
        assert ok is not None and got["n_refined"][ok] >= 60


@pytest.mark.parametrize("n", SIZES)
def test_sizes(fm, n):
    sc = pr.scene("base", 2, n)
    m, _ = pr.set_ransac_parameters(n, min_inliers=4)
    sets = pr.draw_sets(n, n, 12)
    got = fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], m, 12, sets=sets)
    pr.check_result(got, sc, sets, m, 8, "device n %d" % n)


@pytest.mark.parametrize("its", ITERATIONS)
def test_iteration_counts_with_sets_drawn_on_the_device(fm, its):
    sc = pr.scene("base", 3, 63)
    m, _ = pr.set_ransac_parameters(63)
    got = fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], m, its, seed=its, max_records=16)
    sets = got["sets"]
    assert sets.shape == (its, 4) and sets.min() >= 0 and sets.max() < 63
    assert all(len(set(s)) == 4 for s in sets.tolist())
    if its >= 35:
        assert len({tuple(s) for s in sets.tolist()}) > its // 2
    pr.check_result(got, sc, sets, m, 16, "device %d iterations" % its)
    # the device-drawn sets replayed through the host-sets form: bit-identical
    again = fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], m, its, sets=sets, max_records=16)
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k


def _batch(n_lists):
    """lists of differing lengths; among twenty: one without a valid result, a 3-point list and a clipped one"""
    sizes = [96, 17, 64][:n_lists] if n_lists <= 3 else [(96, 17, 64, 5, 257, 33)[i % 6] for i in range(n_lists)]
    cap = 96 if n_lists <= 3 else 130
    scenes = [pr.scene(("base", "wide", "shallow")[i % 3], 1 + i % 3, n) for i, n in enumerate(sizes)]
    d_n = list(sizes)                                 # 257 > cap: the clipped list
    if n_lists == 20:
        d_n[7], d_n[9] = -1, 3
    return scenes, d_n, cap


def _run_batch(fm, scenes, d_n, cap, order, its, seed, d_sets=None, max_records=4):
    """the lists `order` of the batch in one device call, every output pre-filled with a sentinel -> numpy dict"""
    import torch
    from mono_slam_framework_amd import _lib
    L = len(order)
    p3 = np.full((L, cap, 3), 7.5, np.float32)
    p2 = np.full((L, cap, 2), 7.5, np.float32)
    for row, i in enumerate(order):
        k = min(len(scenes[i]["p3d"]), cap)
        p3[row, :k], p2[row, :k] = scenes[i]["p3d"][:k], scenes[i]["p2d"][:k]
    out = {}
    for name, (shape, dt) in _lib.pnp_shapes(L, its, max_records, cap).items():
        out[name] = torch.from_numpy(np.full(shape, 0xAB if dt == "uint8" else -77, dt)).cuda()
    if d_sets is not None:
        d_sets = torch.from_numpy(np.ascontiguousarray(d_sets)).cuda()
    got = fm.pnp_ransac_device(torch.from_numpy(p3).cuda(), torch.from_numpy(p2).cuda(),
                               torch.tensor([d_n[i] for i in order], dtype=torch.int32, device="cuda"), scenes[0]["K"], 8,
                               its, max_records=max_records, seed=seed, d_sets=d_sets, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


@pytest.mark.parametrize("n_lists", [1, 3, 20])
def test_batch_equals_its_replay(fm, n_lists):
    from mono_slam_framework_amd import _lib
    scenes, d_n, cap = _batch(n_lists)
    its, max_records = 35, 4
    order = list(range(n_lists))
    got = _run_batch(fm, scenes, d_n, cap, order, its, 5)
    shapes = _lib.pnp_shapes(n_lists, its, max_records, cap)
    sentinel = lambda name: np.array(0xAB if shapes[name][1] == "uint8" else -77, shapes[name][1])
    for i in order:
        n = min(d_n[i], cap)
        if n < 4:                                     # no valid result: n_records alone is written
            assert got["n_records"][i] == -1
            for k in PER_LIST[1:]:
                assert (got[k][i] == sentinel(k)).all(), (i, k)
            continue
        kept = min(int(got["n_records"][i]), max_records)
        assert got["n_records"][i] >= 0
        for name, _, per, _ in _lib.PNP_ARRAYS:       # bytes beyond a list and beyond its records: untouched
            if per == "rec":
                assert (got[name][i, kept:] == sentinel(name)).all(), (i, name)
        assert (got["inliers_best"][i, :kept, n:] == 0xAB).all() and (got["inliers_refined"][i, :kept, n:] == 0xAB).all()
        assert (got["inliers_best"][i, :kept, :n] <= 1).all() and (got["inliers_refined"][i, :kept, :n] <= 1).all()
        # the host entry on the same list with the returned sets: bit for bit
        sc = scenes[i]
        host = fm.pnp_ransac(sc["p3d"][:n], sc["p2d"][:n], sc["K"], 8, its, sets=got["sets"][i], max_records=max_records)
        assert host["n_records"] == got["n_records"][i]
        for name, _, per, _ in _lib.PNP_ARRAYS[1:]:
            mine = got[name][i, :kept] if per == "rec" else got[name][i]
            if name.startswith("inliers"):
                mine = mine[:, :n]
            assert np.ascontiguousarray(mine).tobytes() == np.ascontiguousarray(host[name]).tobytes(), (i, name)
    # the bars on one list of the batch, from what the batch returned
    one = {k: got[k][0] for k in PER_LIST}
    kept = min(int(one["n_records"]), max_records)
    for name, _, per, _ in _lib.PNP_ARRAYS:
        if per == "rec":
            one[name] = one[name][:kept]
    n0 = min(d_n[0], cap)
    one["inliers_best"], one["inliers_refined"] = one["inliers_best"][:, :n0], one["inliers_refined"][:, :n0]
    one["n_records"], one["capacity"] = int(one["n_records"]), int(one["n_records"]) > max_records
    sc0 = {k: (v[:n0] if k in ("p3d", "p2d") else v) for k, v in scenes[0].items()}
    pr.check_result(one, sc0, one["sets"], 8, max_records, "device batch of %d, list 0" % n_lists)
    if n_lists == 1:
        return
    # any order, with the sets the first call drew (the draw is keyed by a list's place in its call)
    order2 = order[::-1]
    again = _run_batch(fm, scenes, d_n, cap, order2, its, 5, d_sets=got["sets"][order2])
    for row, i in enumerate(order2):
        for k in PER_LIST:
            if k == "sets":
                continue                              # given, not written
            assert got[k][i].tobytes() == again[k][row].tobytes(), (i, k)
    # and a list alone gives what it gave in the batch
    i = n_lists - 1
    alone = _run_batch(fm, scenes, d_n, cap, [i], its, 5, d_sets=got["sets"][[i]])
    for k in PER_LIST:
        if k != "sets":
            assert got[k][i].tobytes() == alone[k][0].tobytes(), k


def test_max_records_one_on_a_list_with_more(fm):
    from mono_slam_framework_amd import _lib
    sc = pr.scene("wide", 1)
    sets = pr.draw_sets(1, pr.N_SCENE, pr.N_ITERATIONS)
    full = fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], 48, 35, sets=sets)
    assert full["n_records"] >= 2 and not full["capacity"]
    one = fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], 48, 35, sets=sets, max_records=1)
    assert one["capacity"] and one["n_records"] == full["n_records"]
    assert "max_records" in fm.last_error()
    for name, _, per, _ in _lib.PNP_ARRAYS:
        if per == "rec":
            assert np.asarray(one[name]).tobytes() == np.asarray(full[name][:1]).tobytes(), name


def test_argument_checks_and_short_lists(fm):
    from mono_slam_framework_amd.matcher import MsfError
    sc = pr.scene("base", 1, 3)
    assert fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], 4, 5)["n_records"] == -1
    assert fm.pnp_ransac(np.zeros((0, 3)), np.zeros((0, 2)), sc["K"], 4, 5)["n_records"] == -1
    sc = pr.scene("base", 1, 16)
    for bad in (dict(min_inliers=0), dict(n_iterations=0), dict(max_records=0),
                dict(th2=float("nan"))):
        kw = dict(min_inliers=4, n_iterations=5)
        kw.update(bad)
        with pytest.raises((MsfError, MemoryError, ValueError)) as e:
            fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], **kw)
        assert not isinstance(e.value, MsfError) or e.value.code == -1
    # a given set that points outside the list: a NaN pose and no inliers, nothing read out of bounds
    sets = np.array([[0, 1, 2, 3], [0, 1, 2, 16], [-1, 1, 2, 3]], np.int32)
    got = fm.pnp_ransac(sc["p3d"], sc["p2d"], sc["K"], 4, 3, sets=sets)
    assert np.isnan(got["pose_f64"][1:]).all() and (got["counts"][1:] == 0).all() and np.isfinite(got["pose_f64"][0]).all()
