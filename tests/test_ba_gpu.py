"""GPU: k_bundle_adjust (csrc/ba_kernels.hip) through msf_bundle_adjust / msf_bundle_adjust_device --
Optimizer::LocalBundleAdjustment's two Schur-complement Levenberg-Marquardt rounds and vToErase flags, and
BundleAdjustment's one round -- against the float64 reference of tests/ba_ref.py, bar by bar and against the device's
own diagnostics (the sums from its own entry estimates, every iteration replayed from its own entry estimate and
lambda, the flags from its own round and final estimates, the final estimates against the reference's run where the
reference's own permutations agree); the sizes of the issue; batches with an invalid descriptor, a malformed problem,
an empty one and one above max_free_cams, bit-identical to their replay alone, shuffled, and to the host-pointer entry;
untouched bytes beyond every extent; the stop word.

Figures on an MI355X (printed with -s; steps and finals as fractions of the bars of profiles/ba_bars.txt): 115 of 149
iterations clear (20 / 20 on the initial map, 15 / 15 at 64 + 2 cameras, 9 to 12 of 12 or 15 elsewhere), the worst kept
estimate of a clear iteration 0.125 of its scene's bar, the final estimates 0.35 (initial map) and 3e-8 (64 + 2 cameras)
of theirs; the other eight scenes are held to bars 1-3 only (ba_ref.CHAOTIC)."""
import numpy as np
import pytest

from tests import ba_ref as br

pytestmark = pytest.mark.gpu

SENTINEL = {"uint8": 0xAB, "int32": -77, "float32": -77.0, "float64": -77.0}


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.7, 640, 480)
    yield m
    m.close()


def _host_call(fm, sc, schedule=br.LOCAL_BA, **kw):
    return fm.bundle_adjust(sc["cam_Tcw"], sc["cam_fixed"], sc["points"], sc["edge_cam"], sc["edge_point"], sc["edge_obs"],
                            sc["K"], schedule=schedule, **kw)


@pytest.mark.parametrize("name", list(br.SCENES))
def test_scenes_meet_the_float64_bars(fm, name):
    got = _host_call(fm, br.scene(name), br.schedule_of(name))
    clear, run, step, final = br.check_result(got, name, "device " + name)
    print("%s: %d clear iterations of %d, worst step %.3g and final %.3g of their bars" % (name, clear, run, step, final))


def _empty():
    z = lambda *s, dt=np.float32: np.zeros(s, dt)
    return dict(cam_Tcw=z(0, 12), cam_fixed=z(0, dt=np.uint8), points=z(0, 3), edge_cam=z(0, dt=np.int32),
                edge_point=z(0, dt=np.int32), edge_obs=z(0, 2), K=br.K)


def _batch(n):
    """-> [(scene, kind)]: kind "ok", "invalid" (n_cams = -1), "malformed" (an edge index out of range), "empty" (no
    cameras, points or edges) or "many" (more free cameras than the call's max_free_cams = 8)"""
    if n == 1:
        return [(br.scene("p65"), "ok")]
    if n == 3:
        return [(br.scene("e257"), "ok"), (br.scene("p63"), "malformed"), (br.scene("local"), "ok")]
    return [(br.scene("p64"), "ok"), (br.scene("p63"), "invalid"), (br.scene("local"), "ok"), (_empty(), "empty"),
            (br.scene("wide"), "many"), (br.scene("e255"), "ok"), (br.scene("p65"), "malformed"), (br.scene("e256"), "ok")]


def _run_batch(fm, problems, order, d_stop=None, pad=3, rows=None):
    """the problems `order` in one device call, every output pre-filled with a sentinel and `pad` spare rows at the end
    of every array; rows: a permutation of the descriptors, the arrays staying where they are -> (numpy dict,
    descriptors in the order passed)"""
    import torch
    from mono_slam_framework_amd import _lib
    desc, tcw, fixed, pts, ec, ep, obs = [], [], [], [], [], [], []
    c0 = p0 = e0 = 0
    for i in order:
        sc, kind = problems[i]
        nc, npt, ne = len(sc["cam_Tcw"]), len(sc["points"]), len(sc["edge_cam"])
        desc.append((-1 if kind == "invalid" else nc, npt, ne, c0, p0, e0))
        cam = sc["edge_cam"].copy()
        if kind == "malformed":
            cam[ne // 2] = nc + 1000000
        tcw.append(sc["cam_Tcw"].reshape(-1, 12)), fixed.append(sc["cam_fixed"]), pts.append(sc["points"].reshape(-1, 3))
        ec.append(cam), ep.append(sc["edge_point"]), obs.append(sc["edge_obs"].reshape(-1, 2))
        c0, p0, e0 = c0 + nc, p0 + npt, e0 + ne
    cat = lambda xs, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(xs), dt)).cuda()
    if rows is not None:                                  # the descriptors in another order than the arrays
        desc = [desc[r] for r in rows]
    shapes = _lib.ba_shapes(len(order) + pad, c0 + pad, p0 + pad, e0 + pad)
    out = {name: torch.from_numpy(np.full(shape, SENTINEL[dt], dt)).cuda() for name, (shape, dt) in shapes.items()}
    got = fm.bundle_adjust_device(torch.tensor(desc, dtype=torch.int32, device="cuda"), cat(tcw, np.float32),
                                  cat(fixed, np.uint8), cat(pts, np.float32), cat(ec, np.int32), cat(ep, np.int32),
                                  cat(obs, np.float32), br.K, max_free_cams=8, d_stop=d_stop, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}, desc


def _slice(got, desc, row):
    """problem `row` of a batch result as the dict the host call returns, plus the raw pieces for byte comparisons"""
    from mono_slam_framework_amd import _lib
    nc, npt, ne, c0, p0, e0 = desc[row]
    nc = max(nc, 0)
    one = {}
    for name, _, per, _ in _lib.BA_ARRAYS:
        a = got[name]
        if per in ("problem", "round", "it"):
            one[name] = a[row]
        elif per == "cam":
            one[name] = a[c0:c0 + nc]
        elif per == "point":
            one[name] = a[p0:p0 + npt]
        elif per == "edge":
            one[name] = a[e0:e0 + ne]
        elif per == "it_cam":
            one[name] = a[64 * c0:64 * (c0 + nc)].reshape((64, nc) + a.shape[1:])
        else:
            one[name] = a[64 * p0:64 * (p0 + npt)].reshape((64, npt) + a.shape[1:])
    one["status"] = int(one["status"])
    return one


def _written(one, name, per):
    """the part of array `name` that the device call writes for a problem that ran"""
    a = one[name]
    rounds = one["status"]
    ran = one["it_trials"] != 0
    if name == "round_flags":
        return a[:, :rounds]
    if per in ("it", "it_cam", "it_point") and name != "it_trials":
        return a[ran]
    return a


@pytest.mark.parametrize("n", [1, 3, 8])
def test_batch_equals_its_replay(fm, n):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import MsfError
    problems = _batch(n)
    order = list(range(n))
    got, desc = _run_batch(fm, problems, order)
    pers = {a[0]: a[2] for a in _lib.BA_ARRAYS}
    total = {"cam": sum(len(sc["cam_Tcw"]) for sc, _ in problems), "point": sum(d[1] for d in desc),
             "edge": sum(d[2] for d in desc)}             # the invalid problem's rows are there, its n_cams says -1
    # bytes beyond every output extent are untouched
    for name, per in pers.items():
        a, fill = got[name], SENTINEL[str(got[name].dtype)]
        end = {"problem": n, "round": n, "it": n, "cam": total["cam"], "point": total["point"], "edge": total["edge"],
               "it_cam": 64 * total["cam"], "it_point": 64 * total["point"]}[per]
        assert (a[end:] == fill).all(), name
    for i in order:
        sc, kind = problems[i]
        one = _slice(got, desc, i)
        if kind in ("invalid", "malformed", "many"):      # status alone is written
            assert one["status"] == -1, (i, kind)
            if kind == "invalid":
                continue
            for name in pers:
                if name != "status":
                    assert (one[name] == SENTINEL[str(got[name].dtype)]).all(), (i, kind, name)
            if kind == "malformed":                       # the host entry refuses it
                bad = dict(sc, edge_cam=sc["edge_cam"].copy())
                bad["edge_cam"][len(bad["edge_cam"]) // 2] += 1000000
                with pytest.raises(MsfError) as e:
                    _host_call(fm, bad)
                assert e.value.code == _lib.MSF_ERR_INVALID_ARG
            continue
        assert one["status"] == 2, (i, kind)
        # what is not written keeps the sentinel
        ran = one["it_trials"] != 0
        for name, per in pers.items():
            if per in ("it", "it_cam", "it_point") and name != "it_trials":
                assert (one[name][~ran] == -77.0).all(), (i, name)
        # the host entry on the same problem: bit for bit where the device call writes
        host = _host_call(fm, sc)
        assert host["status"] == one["status"]
        for name, per in pers.items():
            if name == "status":
                continue
            mine, theirs = _written(one, name, per), _written(host, name, per)
            assert np.ascontiguousarray(mine).tobytes() == np.ascontiguousarray(np.asarray(theirs, got[name].dtype)).tobytes(), (i, name)
    # the bars on the problems of the batch that ran, from what the batch returned
    names = {id(br.scene(k)): k for k in br.SCENES}
    for i in order:
        sc, kind = problems[i]
        if kind == "ok":
            one = _slice(got, desc, i)
            one["round_iterations"] = one["round_iterations"]
            br.check_result(one, names[id(sc)], "device batch of %d, problem %d" % (n, i))
    if n == 1:
        return
    # any order, and every problem alone gives what it gave in the batch
    order2 = [int(k) for k in np.random.default_rng(n).permutation(n)]
    again, desc2 = _run_batch(fm, problems, order2)
    for row, i in enumerate(order2):
        a, b = _slice(got, desc, i), _slice(again, desc2, row)
        for name in pers:
            assert np.ascontiguousarray(a[name]).tobytes() == np.ascontiguousarray(b[name]).tobytes(), (i, name)
    for i in order2:
        alone, desc1 = _run_batch(fm, problems, [i])
        a, b = _slice(got, desc, i), _slice(alone, desc1, 0)
        for name in pers:
            assert np.ascontiguousarray(a[name]).tobytes() == np.ascontiguousarray(b[name]).tobytes(), (i, name)


@pytest.mark.parametrize("n", [3, 8])
def test_descriptors_in_another_order_than_the_arrays(fm, n):
    """msf_ba.h asks only that the ranges do not overlap: with the arrays in place and the descriptors reversed or
    shuffled -- cam0 and point0 no longer rising with the problem index -- every problem gives, bit for bit, what it gives
    in array order and alone"""
    from mono_slam_framework_amd import _lib
    problems = _batch(n)
    order = list(range(n))
    got, desc = _run_batch(fm, problems, order)
    names = [a[0] for a in _lib.BA_ARRAYS]
    for rows in (order[::-1], [int(k) for k in np.random.default_rng(10 + n).permutation(n)]):
        again, desc2 = _run_batch(fm, problems, order, rows=rows)
        assert [d[3] for d in desc2] != sorted(d[3] for d in desc2) or rows == order
        for row, i in enumerate(rows):
            assert desc2[row] == desc[i]
            a, b = _slice(got, desc, i), _slice(again, desc2, row)
            for name in names:
                assert np.ascontiguousarray(a[name]).tobytes() == np.ascontiguousarray(b[name]).tobytes(), (rows, i, name)
    for i in order:
        if problems[i][1] != "ok":
            continue
        alone, desc1 = _run_batch(fm, problems, [i])
        a, b = _slice(again, desc2, rows.index(i)), _slice(alone, desc1, 0)
        for name in names:
            assert np.ascontiguousarray(a[name]).tobytes() == np.ascontiguousarray(b[name]).tobytes(), (i, name)


def test_stop_word_preset(fm):
    import torch
    sc = br.scene("p64")
    ref = br.run(sc, br.LOCAL_BA, stop=True)
    got = _host_call(fm, sc, stop=1)
    assert got["status"] == 0 and (got["it_trials"] == 0).all() and (got["round_iterations"] == 0).all()
    assert got["cam_Tcw"].tobytes() == sc["cam_Tcw"].tobytes() and got["points"].tobytes() == sc["points"].tobytes()
    assert (got["outliers"] == ref["outliers"]).all()
    dev, desc = _run_batch(fm, [(sc, "ok")], [0], d_stop=torch.ones(1, dtype=torch.int32, device="cuda"))
    one = _slice(dev, desc, 0)
    assert one["status"] == 0 and one["cam_Tcw"].tobytes() == sc["cam_Tcw"].tobytes()
    assert one["points"].tobytes() == sc["points"].tobytes() and (one["outliers"] == ref["outliers"]).all()
    assert (one["round_flags"] == 0xAB).all()
    assert _host_call(fm, sc, stop=0)["status"] == 2


def test_one_round_of_bundle_adjustment_without_a_kernel(fm):
    sc = br.scene("p65")
    schedule = (1, (8, 0), (0, 0))
    got = _host_call(fm, sc, schedule)
    br.check_result(got, None, "device BundleAdjustment", sc=sc, schedule=schedule, final=False)


def test_capacity_and_argument_checks(fm):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import MsfError
    sc = br.make_scene(65, 1, 40, None, 1)
    with pytest.raises(MsfError) as e:
        _host_call(fm, sc)
    assert e.value.code == _lib.MSF_ERR_CAPACITY
    sc = br.scene("p63")
    for kw in (dict(chi2=float("nan")), dict(huber_delta2=0.0), dict(schedule=(3, (5, 5), (1, 0))),
               dict(schedule=(2, (33, 5), (1, 0))), dict(schedule=(2, (5, 5), (2, 0)))):
        with pytest.raises(MsfError) as e:
            _host_call(fm, sc, **kw)
        assert e.value.code == _lib.MSF_ERR_INVALID_ARG, kw
    unsorted = dict(sc, edge_point=sc["edge_point"][::-1].copy())
    with pytest.raises(MsfError) as e:
        _host_call(fm, unsorted)
    assert e.value.code == _lib.MSF_ERR_INVALID_ARG and "sorted" in fm.last_error()
