"""GPU: the global bundle adjustment (csrc/gba_kernels.hip) through msf_global_bundle_adjust /
msf_global_bundle_adjust_device.  The oracle is the host build of csrc/ba_solve.h (tests/ba_host.py, pinned to the
float64 reference by tests/test_ba_solve_host.py): every array of msf_ba_result, the f64 diagnostics included, must be
its bytes -- above the old cap of 64 free cameras, at the tile edges of the device Cholesky, through rejected trials and
a NaN observation, on degenerate problems -- and, wherever msf_bundle_adjust takes the problem, its bytes too.  Then the
refusals (status -1 and nothing else written), the stop word, the two entry points against each other and a regrown
workspace.

The host build is a bit-exact oracle because the one transcendental step of the arithmetic, sin / cos of a pose update,
is pose::sin_cos -- plain multiplies and adds -- in every build of ba_solve.h; with libm's sin / cos the device and the
host differed in the last bit of a kept camera estimate wherever the steps were larger (a schedule without a Huber
kernel over the scenes' gross outliers), while the points of the same trial agreed."""
import numpy as np
import pytest

from tests import ba_host, ba_ref as br, gba_host, gba_scenes as gs

pytestmark = pytest.mark.gpu

SENTINEL = {"uint8": 0xAB, "int32": -77, "float32": -77.0, "float64": -77.0}


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.7, 640, 480)
    yield m
    m.close()


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    return ba_host.build(tmp_path_factory.mktemp("gba_oracle"))


def _call(fm, sc, schedule, **kw):
    return fm.global_bundle_adjust(sc["cam_Tcw"], sc["cam_fixed"], sc["points"], sc["edge_cam"], sc["edge_point"],
                                   sc["edge_obs"], sc["K"], schedule=schedule, **kw)


def _oracle(L, sc, schedule, **kw):
    return ba_host.run(L, sc, schedule, max_free=max(gs.n_free(sc), 1), **kw)


def _device(fm, sc, schedule, pad=0, sentinel=False, d_stop=None, max_free_cams=None, edge_cam=None):
    """the device entry on the scene -> (numpy dict as the shapes of one problem say, rows per unit)"""
    import torch
    from mono_slam_framework_amd import _lib
    nc, npt, ne = len(sc["cam_Tcw"]), len(sc["points"]), len(sc["edge_cam"])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    out = None
    if sentinel:
        shapes = _lib.ba_shapes(1 + pad, nc + pad, npt + pad, ne + pad)
        out = {name: torch.from_numpy(np.full(shape, SENTINEL[dt], dt)).cuda() for name, (shape, dt) in shapes.items()}
    kw = {} if max_free_cams is None else dict(max_free_cams=max_free_cams)
    got = fm.global_bundle_adjust_device(t(sc["cam_Tcw"].reshape(-1, 12), np.float32), t(sc["cam_fixed"], np.uint8),
                                         t(sc["points"].reshape(-1, 3), np.float32),
                                         t(sc["edge_cam"] if edge_cam is None else edge_cam, np.int32),
                                         t(sc["edge_point"], np.int32), t(sc["edge_obs"].reshape(-1, 2), np.float32), sc["K"],
                                         schedule=schedule, d_stop=d_stop, out=out, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def _one(raw, nc, npt, ne):
    """problem 0 of a device result with spare rows as the dict the host entry returns"""
    from mono_slam_framework_amd import _lib
    one = {}
    for name, _, per, _ in _lib.BA_ARRAYS:
        a = raw[name]
        if per in ("problem", "round", "it"):
            one[name] = a[0]
        elif per == "cam":
            one[name] = a[:nc]
        elif per == "point":
            one[name] = a[:npt]
        elif per == "edge":
            one[name] = a[:ne]
        elif per == "it_cam":
            one[name] = a[:64 * nc].reshape((64, nc) + a.shape[1:])
        else:
            one[name] = a[:64 * npt].reshape((64, npt) + a.shape[1:])
    one["status"] = int(one["status"])
    return one


@pytest.mark.parametrize("name", ["s65", "g80", "s130"])
def test_more_than_64_free_cameras_equal_the_host_build(fm, L, name):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import MsfError
    sc, schedule = gs.scene(name)
    assert gs.n_free(sc) > 64
    want = _oracle(L, sc, schedule)
    got = _call(fm, sc, schedule)
    assert want["status"] == schedule[0] and got["status"] == want["status"]
    assert gba_host.same(want, got) == []
    if name == "s65":
        with pytest.raises(MsfError) as e:
            fm.bundle_adjust(sc["cam_Tcw"], sc["cam_fixed"], sc["points"], sc["edge_cam"], sc["edge_point"], sc["edge_obs"],
                             sc["K"], schedule=schedule)
        assert e.value.code == _lib.MSF_ERR_CAPACITY


# What of an iteration's record does not pass through sin / cos: everything but the kept camera estimates and what is
# computed from them.  Held on its own, so that a difference in pose::sin_cos and one in the solve tell themselves apart.
LIBM_FREE = ("it_cam_in", "it_point_in", "it_Hcc", "it_bc", "it_Hpp", "it_bp", "it_cost_in", "it_lambda_in", "it_point_out")


@pytest.mark.parametrize("name", ["g80", "s130", "rejected"])
def test_first_iteration_above_the_old_cap_is_the_host_builds(fm, L, name):
    """The system, the Schur complement, the tiled Cholesky of up to 780 x 780, the back substitution and the point
    steps of iteration 0 -- every trial of it -- apart from sin / cos: bit for bit the host build's."""
    sc, schedule = gs.scene(name)
    want, got = _oracle(L, sc, schedule), _call(fm, sc, schedule)
    assert got["it_trials"].tobytes() == want["it_trials"].tobytes() and got["status"] == want["status"]
    for k in LIBM_FREE:
        assert gba_host._bits(got[k][0]) == gba_host._bits(want[k][0]), k
    assert np.abs(got["it_point_out"][0] - got["it_point_in"][0]).max() > 0


def test_tile_edges_equal_msf_bundle_adjust(fm):
    """the scenes of test_tile_edges have at most 33 free cameras: the one-workgroup kernel takes them, and the two
    device paths run the same code"""
    for n in gs.tile_edge_sizes(64):
        sc, schedule = gs.scene("t%d" % n)
        want = fm.bundle_adjust(sc["cam_Tcw"], sc["cam_fixed"], sc["points"], sc["edge_cam"], sc["edge_point"], sc["edge_obs"],
                                sc["K"], schedule=schedule)
        assert gba_host.same(want, _call(fm, sc, schedule)) == [], n
    schedule = gs.GLOBAL_BA
    sc60 = gs.far_off(br.make_scene(60, 2, 300, None, 1), 1)
    want = fm.bundle_adjust(sc60["cam_Tcw"], sc60["cam_fixed"], sc60["points"], sc60["edge_cam"], sc60["edge_point"],
                            sc60["edge_obs"], sc60["K"], schedule=schedule)
    assert want["it_trials"].max() >= 2 and gba_host.same(want, _call(fm, sc60, schedule)) == []


@pytest.mark.parametrize("name", list(br.SCENES))
def test_small_problems_equal_msf_bundle_adjust(fm, name):
    sc, schedule = br.scene(name), br.schedule_of(name)
    want = fm.bundle_adjust(sc["cam_Tcw"], sc["cam_fixed"], sc["points"], sc["edge_cam"], sc["edge_point"], sc["edge_obs"],
                            sc["K"], schedule=schedule)
    assert gba_host.same(want, _call(fm, sc, schedule)) == []


def test_tile_edges(fm, L):
    from mono_slam_framework_amd import _lib
    T = _lib.load().msf_global_ba_tile_rows()
    sizes = gs.tile_edge_sizes(T)
    assert all(6 * a <= k * T < 6 * b for k, (a, b) in zip((1, 2, 3), zip(sizes[::2], sizes[1::2])))
    for n in sizes:
        sc, schedule = gs.scene("t%d" % n)
        assert gs.n_free(sc) == n and len(sc["points"]) == 4 * n and int(sc["cam_fixed"].sum()) == 2
        assert gba_host.same(_oracle(L, sc, schedule), _call(fm, sc, schedule)) == [], n


def test_float64_bars_above_the_old_cap(fm):
    sc, schedule = gs.scene("g80_clean")
    assert gs.G80_STEP_SPREAD is not None and 2 * gs.G80_STEP_SPREAD <= br.STEP_BAR
    br.STEP_BARS["g80"] = 2 * gs.G80_STEP_SPREAD
    try:
        clear, run, step, final = br.check_result(_call(fm, sc, schedule), "g80", "device g80_clean", sc=sc, schedule=schedule, final=False)
    finally:
        del br.STEP_BARS["g80"]
    print("g80: %d clear iterations of %d, worst step %.3g of its bar" % (clear, run, step))


@pytest.mark.parametrize("name", ["rejected", "nan"])
def test_rejected_trials_equal_the_host_build(fm, L, name):
    sc, schedule = gs.scene(name)
    want, got = _oracle(L, sc, schedule), _call(fm, sc, schedule)
    trials = want["it_trials"][want["it_trials"] > 0].tolist()
    if name == "rejected":
        assert trials == gs.REJECTED_TRIALS and max(trials) >= 2
    else:
        assert trials == [10] and want["round_iterations"].tolist() == [1, 0]   # every trial rejected, the run ends
        assert want["cam_pose_f64"].tobytes() == got["cam_pose_f64"].tobytes()
    assert gba_host.same(want, got) == []
    assert got["it_lambda_in"].tobytes() == want["it_lambda_in"].tobytes()
    assert got["it_lambda_out"].tobytes() == want["it_lambda_out"].tobytes()


def test_degenerate_problems(fm, L):
    sc, schedule = gs.scene("lonely")
    free = np.flatnonzero(sc["cam_fixed"] == 0)
    assert not (sc["edge_cam"] == free[0]).any() and sc["cam_fixed"][sc["edge_cam"][sc["edge_point"] == 0]].all()
    want, got = _oracle(L, sc, schedule), _call(fm, sc, schedule)
    assert gba_host.same(want, got) == [] and got["status"] == 2
    last = 32 + int(got["round_iterations"][1]) - 1
    assert got["it_cam_out"][last][free[0]].tobytes() == got["it_cam_in"][0][free[0]].tobytes()
    # the camera without an edge does not move; the point seen by fixed cameras alone is still a free point: it moves
    # under its own 3 x 3 block, as in the host build (compared above)
    assert got["it_point_out"][last][0].tobytes() != got["it_point_in"][0][0].tobytes()
    z = lambda *s, dt=np.float32: np.zeros(s, dt)
    empty = dict(cam_Tcw=z(0, 12), cam_fixed=z(0, dt=np.uint8), points=z(0, 3), edge_cam=z(0, dt=np.int32),
                 edge_point=z(0, dt=np.int32), edge_obs=z(0, 2), K=br.K)
    for schedule in (br.LOCAL_BA, gs.GLOBAL_BA):
        want, got = _oracle(L, empty, schedule), _call(fm, empty, schedule)
        assert gba_host.same(want, got) == [] and got["status"] == schedule[0]
        assert _one(_device(fm, empty, schedule), 0, 0, 0)["status"] == schedule[0]


def test_refusals_write_the_status_alone_and_spare_rows_stay(fm, L):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import MsfError
    sc, schedule = gs.scene("t11")
    nc, npt, ne = len(sc["cam_Tcw"]), len(sc["points"]), len(sc["edge_cam"])
    pers = {a[0]: a[2] for a in _lib.BA_ARRAYS}
    end = {"problem": 1, "round": 1, "it": 1, "cam": nc, "point": npt, "edge": ne, "it_cam": 64 * nc, "it_point": 64 * npt}
    bad_cam = sc["edge_cam"].copy()
    bad_cam[ne // 2] = nc + 1000000
    decreasing = dict(sc, edge_point=sc["edge_point"].copy())
    decreasing["edge_point"][[5, 6]] = decreasing["edge_point"][[6, 5]] if decreasing["edge_point"][5] != decreasing["edge_point"][6] else (3, 1)
    assert (np.diff(decreasing["edge_point"]) < 0).any()
    for what in ("index", "order", "capacity"):
        if what == "capacity":
            with pytest.raises(MsfError) as e:
                _device(fm, sc, schedule, pad=3, sentinel=True, max_free_cams=10)
            assert e.value.code == _lib.MSF_ERR_CAPACITY
            continue
        raw = _device(fm, sc if what == "index" else decreasing, schedule, pad=3, sentinel=True,
                      edge_cam=bad_cam if what == "index" else None)
        assert raw["status"][0] == -1 and (raw["status"][1:] == -77).all(), what
        for name in pers:
            if name != "status":
                assert (raw[name] == SENTINEL[str(raw[name].dtype)]).all(), (what, name)
    # the refused capacity call wrote the status alone: seen through a call that keeps its tensors
    import torch
    shapes = _lib.ba_shapes(1, nc, npt, ne)
    out = {name: torch.from_numpy(np.full(shape, SENTINEL[dt], dt)).cuda() for name, (shape, dt) in shapes.items()}
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    with pytest.raises(MsfError):
        fm.global_bundle_adjust_device(t(sc["cam_Tcw"].reshape(-1, 12), np.float32), t(sc["cam_fixed"], np.uint8),
                                       t(sc["points"], np.float32), t(sc["edge_cam"], np.int32), t(sc["edge_point"], np.int32),
                                       t(sc["edge_obs"], np.float32), sc["K"], schedule=schedule, max_free_cams=10, out=out)
    torch.cuda.synchronize()
    assert int(out["status"].cpu()[0]) == -1
    for name in pers:
        if name != "status":
            assert (out[name].cpu().numpy() == SENTINEL[str(shapes[name][1])]).all(), name
    # the host entry refuses the malformed ones by code
    for bad in (dict(sc, edge_cam=bad_cam), decreasing):
        with pytest.raises(MsfError) as e:
            _call(fm, bad, schedule)
        assert e.value.code == _lib.MSF_ERR_INVALID_ARG
    # a problem that runs: what lies beyond every extent keeps the sentinel, what is written is the host build's
    raw = _device(fm, sc, schedule, pad=3, sentinel=True)
    for name, per in pers.items():
        assert (raw[name][end[per]:] == SENTINEL[str(raw[name].dtype)]).all(), name
    one, want = _one(raw, nc, npt, ne), _oracle(L, sc, schedule)
    ran = want["it_trials"] != 0
    for name, per in pers.items():
        if per in ("it", "it_cam", "it_point") and name != "it_trials":
            assert np.ascontiguousarray(one[name][ran]).tobytes() == np.ascontiguousarray(want[name][ran]).tobytes(), name
            assert (one[name][~ran] == -77.0).all(), name
        elif name == "round_flags":
            assert one[name][:, :1].tobytes() == want[name][:, :1].tobytes() and (one[name][:, 1] == 0xAB).all()
        elif name != "status":
            assert np.ascontiguousarray(one[name]).tobytes() == np.ascontiguousarray(want[name]).tobytes(), name
    assert one["status"] == want["status"] == 1


def test_stop_word(fm, L):
    import torch
    sc, _ = gs.scene("s65")
    nc = len(sc["cam_Tcw"])
    # set before the call: status 0, the estimates as they came, the flags of the entry estimates
    want = _oracle(L, sc, br.LOCAL_BA, stop=1)
    for got in (_call(fm, sc, br.LOCAL_BA, stop=1),
                _one(_device(fm, sc, br.LOCAL_BA, d_stop=torch.ones(1, dtype=torch.int32, device="cuda")), nc, len(sc["points"]),
                     len(sc["edge_cam"]))):
        assert got["status"] == 0 and (got["it_trials"] == 0).all() and (got["round_iterations"] == 0).all()
        assert got["cam_Tcw"].tobytes() == sc["cam_Tcw"].reshape(nc, 12).tobytes() and got["points"].tobytes() == sc["points"].tobytes()
        assert got["outliers"].tobytes() == want["outliers"].tobytes()
    assert _call(fm, sc, br.LOCAL_BA, stop=np.zeros(1, np.int32))["status"] == 2
    # Set on the device between round 0 and round 1.  The call blocks, so nothing outside it can write the word at that
    # moment; the word is therefore one the call itself sets when round 0 ends -- round_iterations[0], 0 until then and
    # 5 after it -- and the first call, {1, {5, 0}, {1, 0}}, says what round 0 keeps.  Round 1 is skipped: one round in
    # the status, no iteration of round 1, the estimates of round 0, and the flags of :530-540 at those estimates.
    from mono_slam_framework_amd import _lib
    first = _call(fm, sc, (1, (5, 0), (1, 0)))
    npt, ne = len(sc["points"]), len(sc["edge_cam"])
    out = {name: torch.zeros(shape, dtype=getattr(torch, dt), device="cuda") for name, (shape, dt) in _lib.ba_shapes(1, nc, npt, ne).items()}
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    fm.global_bundle_adjust_device(t(sc["cam_Tcw"].reshape(-1, 12), np.float32), t(sc["cam_fixed"], np.uint8),
                                   t(sc["points"], np.float32), t(sc["edge_cam"], np.int32), t(sc["edge_point"], np.int32),
                                   t(sc["edge_obs"], np.float32), sc["K"], schedule=br.LOCAL_BA,
                                   d_stop=out["round_iterations"][0, :1], out=out)
    torch.cuda.synchronize()
    got = _one({k: v.cpu().numpy() for k, v in out.items()}, nc, npt, ne)
    assert got["status"] == 1 and got["round_iterations"].tolist() == [5, 0] and (got["it_trials"][32:] == 0).all()
    for name in ("cam_Tcw", "points", "cam_pose_f64", "points_f64", "outliers", "it_trials", "it_cost_out", "it_cam_out"):
        assert np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(first[name]).tobytes(), name
    assert got["round_flags"][:, 0].tobytes() == first["round_flags"][:, 0].tobytes() == got["outliers"].tobytes()
    assert (got["round_flags"][:, 1] == 0).all()


def test_entry_points_agree_and_a_regrown_workspace_changes_nothing(fm):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher
    sc, schedule = gs.scene("t22")
    nc, npt, ne = len(sc["cam_Tcw"]), len(sc["points"]), len(sc["edge_cam"])
    names = [a[0] for a in _lib.BA_ARRAYS]
    fresh = FeatureMatcher(0.7, 640, 480)                 # a handle whose workspace has not grown yet
    try:
        a = _call(fresh, sc, schedule)
        dev = _one(_device(fresh, sc, schedule), nc, npt, ne)
        assert gba_host.same(a, dev, names) == []
        big, big_schedule = gs.scene("larger")
        assert _call(fresh, big, big_schedule)["status"] == 1   # 90 free cameras: the workspace is regrown
        b = _call(fresh, sc, schedule)
        assert gba_host.same(a, b, names) == []
        assert gba_host.same(a, _call(fm, sc, schedule), names) == []
    finally:
        fresh.close()


def test_device_entry_whose_second_carve_regrows_the_block_equals_the_host_build(L):
    """The device entry carves the workspace for 0 free cameras, checks, and carves again for the counted ones; a first
    large problem on a handle makes the second carve allocate a new block, so the record the trials read is not the one
    the checking launch cleared.  Before it a small call whose every trial fails leaves a trial number in the old
    record.  All 21 arrays are the host build's."""
    from mono_slam_framework_amd.matcher import FeatureMatcher
    fresh = FeatureMatcher(0.7, 640, 480)
    try:
        sc, schedule = gs.scene("nan")
        nc, npt, ne = len(sc["cam_Tcw"]), len(sc["points"]), len(sc["edge_cam"])
        assert gba_host.same(_oracle(L, sc, schedule), _one(_device(fresh, sc, schedule), nc, npt, ne)) == []
        for name in ("larger", "s130"):                   # 2.3 MB, then 4.9 MB of S: each grows the block again
            sc, schedule = gs.scene(name)
            nc, npt, ne = len(sc["cam_Tcw"]), len(sc["points"]), len(sc["edge_cam"])
            got = _one(_device(fresh, sc, schedule), nc, npt, ne)
            assert got["status"] == 1 and gba_host.same(_oracle(L, sc, schedule), got) == [], name
    finally:
        fresh.close()
