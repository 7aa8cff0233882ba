"""GPU: msf_frustum / msf_frustum_device (steps 1-2 of include/msf_tracking.h: owner, Frame::isInFrustum, n_to_match).
status, owner_kf, n_to_match and the diagnostics equal the host build of csrc/tracking_solve.h bit for bit (square root
and division are correctly rounded on both sides, contraction is off), equal the float64 reference outside the threshold
bands, the device entry equals the host entry, a malformed device call writes only status_word, and the bytes beyond
every array stay untouched.  The last tests repeat this past one chunk of 256 in every dimension of the checking kernel,
of k_frustum and of k_gate (tracking_ref.CHUNK_CASES)."""
import numpy as np
import pytest

from tests import tracking_host as th
from tests import tracking_ref as tr

pytestmark = pytest.mark.gpu

NAMES = ("n_to_match", "status", "visible", "owner_kf", "u", "v", "dist", "view_cos")
GUARD = 64


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.8, tr.W, tr.H, max_batch_pairs=8)
    yield m
    m.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return th.build(tmp_path_factory.mktemp("tracking_host"))


def guarded_out(n_points, n_kf):
    """-> (out dict of views for frustum_device, the full tensors): every array with GUARD elements of 0x5A behind it"""
    import torch
    from mono_slam_framework_amd import _lib
    full, out = {}, {}
    for k, (shape, dt) in _lib.tracking_shapes(_lib.FRUSTUM_ARRAYS, n_points, n_kf, 1, 0).items():
        t = torch.full((shape[0] + GUARD,), 0x5A, dtype=torch.uint8, device="cuda").repeat_interleave(np.dtype(dt).itemsize)
        full[k] = t.view(getattr(torch, dt))
        out[k] = full[k][:shape[0]]
    return out, full


def untouched(full, n):
    raw = full.view(__import__("torch").uint8).cpu().numpy()
    return (raw[n * (len(raw) // (n + GUARD)):] == 0x5A).all()


def run_all(fm, host, lmap, prm, label):
    want = th.frustum(host, lmap, prm)
    assert want["status_word"] == 0
    got_host = fm.frustum(lmap, tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), float(prm["cos_limit"]))
    n_points, n_kf = len(lmap["points"]), max(len(lmap["kf_start"]) - 1, 0)
    out, full = guarded_out(n_points, n_kf)
    dmap = fm.local_map_to_device(lmap)
    fm.frustum_device(dmap, tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), float(prm["cos_limit"]), out=out)
    assert got_host["status_word"] == 0 and int(out["status_word"].cpu()[0]) == 0
    for k in NAMES:
        dev = out[k].cpu().numpy()
        assert dev.tobytes() == want[k].tobytes(), (label, "device vs host build", k)
        assert got_host[k].tobytes() == want[k].tobytes(), (label, "host entry vs host build", k)
        assert untouched(full[k], len(want[k])), (label, "bytes beyond", k)
    diag = np.stack([want[k] for k in ("u", "v", "dist", "view_cos")], 1)
    return tr.check_against_f64(lmap["points"], prm, want["status"], diag, want["status"] >= 7, label)


@pytest.mark.parametrize("n_points,n_kf", [(1, 1), (63, 3), (64, 8), (65, 3), (257, 8), (900, 8), (900, 1), (65, 0)])
def test_device_equals_host_build_and_float64(fm, host, n_points, n_kf):
    lmap, prm, _, _ = tr.scene(n_points + n_kf, n_points=n_points, n_kf=n_kf, per_kf=min(200, 12 + n_points // 4),
                               n_cur=min(150, n_points // 4), list_len=30, empty_kf=1 if n_kf >= 3 else None)
    worst, in_band = run_all(fm, host, lmap, prm, "%d points, %d key frames" % (n_points, n_kf))
    print("device %d points %d key frames: worst fraction of a bar %.3f, %.2f %% in a band" % (n_points, n_kf, worst, 100 * in_band))
    ref = tr.order_independent(lmap, prm, [np.zeros((0, 4), np.int32)] * n_kf, np.zeros(n_kf, np.int32), 1, 1 << 20)
    got = fm.frustum(lmap, tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), float(prm["cos_limit"]))
    for k in ("status", "visible", "owner_kf", "n_to_match"):
        assert np.array_equal(got[k], ref[k]), k


def test_no_points_and_key_frames_without_entries(fm, host):
    prm = tr.camera(0)
    for start in ([], [0], [0, 0, 0, 0]):
        lmap = fm.make_local_map(np.zeros(0, tr.MAP_POINT), start, [], [])
        run_all(fm, host, lmap, prm, "no points, kf_start %s" % start)
    lmap = fm.make_local_map(tr.scene(5, n_points=7, n_kf=0, n_cur=0)[0]["points"], [0, 0, 0], [], [])
    run_all(fm, host, lmap, prm, "points without entries")
    assert (fm.frustum(lmap, tr.view_of(prm), prm["Ow"], tr.bounds_of(prm))["status"] == 9).all()


def test_exact_thresholds(fm, host):
    """fx = 512, z = 4: u = 512 * x * 0.25 + 320 is exact, so x = -2.5 / +2.5 land on min_x = 0 / max_x = 640"""
    prm = tr.camera(0)
    prm.update(Rcw=np.eye(3, dtype=np.float32).reshape(9), tcw=np.zeros(3, np.float32), Ow=np.zeros(3, np.float32),
               fx=np.float32(512), fy=np.float32(512))
    below = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))
    rows = [((1, 1, 0.0), (0, 0, 1), 10, 6),            # PcZ = +0: invz = inf
            ((1, 1, -0.0), (0, 0, 1), 10, 6),           # -0 in the data; the sum from 0.0f makes PcZ +0 (tracking_solve.h)
            ((0, 0, 0.0), (0, 0, 1), 10, 6),            # 0 * inf
            ((-2.5, 0, 4), (0, 0, 1), 10, 0),           # u == min_x: inclusive
            ((2.5, 0, 4), (0, 0, 1), 10, 0),            # u == max_x: inclusive
            ((below(-2.5), 0, 4), (0, 0, 1), 10, 2), ((2.50001, 0, 4), (0, 0, 1), 10, 2),   # one ulp above 2.5 is a tie that rounds to 640
            ((0, -1.875, 4), (0, 0, 1), 10, 0), ((0, 1.875, 4), (0, 0, 1), 10, 0),      # v == min_y, max_y
            ((0, below(-1.875), 4), (0, 0, 1), 10, 3), ((0, 1.87501, 4), (0, 0, 1), 10, 3),
            ((0, 0, 4), (0, 0, 1), 4, 0),               # dist == max_distance
            ((0, 0, 4), (0, 0, 1), below(4), 4),
            ((0, 0, 4), (0, 0, 0.5), 10, 0),            # viewCos == 0.5 exactly
            ((0, 0, 4), (0, 0, below(0.5)), 10, 5),
            ((np.nan, 0, 4), (0, 0, 1), 10, 6), ((0, 0, np.nan), (0, 0, 1), 10, 6), ((np.inf, 0, 4), (0, 0, 1), 10, 6),
            ((0, 0, np.inf), (0, 0, 1), 10, 6), ((0, 0, -np.inf), (0, 0, 1), 10, 1), ((0, 0, 4), (0, 0, np.nan), 10, 6),
            ((0, 0, -4), (0, 0, 1), 10, 1)]
    pts = np.zeros(len(rows), tr.MAP_POINT)
    for p, (pos, nrm, md, _) in zip(pts, rows):
        p["pos"], p["normal"], p["max_distance"] = pos, nrm, md
    n = len(rows)
    lmap = fm.make_local_map(pts, [0, n], np.arange(n) * 7, np.arange(n))
    run_all(fm, host, lmap, prm, "exact thresholds")
    got = fm.frustum(lmap, tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), 0.5)
    assert list(got["status"]) == [r[3] for r in rows]
    assert got["n_to_match"][0] == sum(r[3] == 0 for r in rows)
    assert got["u"][3] == 0 and got["u"][4] == 640 and got["v"][7] == 0 and got["v"][8] == 480
    assert got["dist"][11] == 4 and got["view_cos"][13] == 0.5
    assert np.array_equal(got["status"], tr.frustum_f32(pts, prm)[0])


def test_a_malformed_device_call_writes_only_status_word(fm):
    lmap, prm, _, _ = tr.scene(4, n_points=70, n_kf=3, per_kf=20, n_cur=8, list_len=10)
    faults = [("kf_point", 5, 70), ("kf_point", 0, -1), ("kf_key", 3, tr.W * tr.H), ("kf_key", 1, int(lmap["kf_key"][0])),
              ("kf_start", 1, 10 ** 6), ("kf_start", 3, 1), ("kf_start", 0, 1), ("cur_key", 2, -5), ("cur_point", 1, 70),
              ("flags", 9, 4)]
    for key, at, value in faults:
        bad = {k: v.copy() for k, v in lmap.items()}
        if key == "flags":
            bad["points"]["flags"][at] = value
        else:
            bad[key][at] = value
        out, full = guarded_out(70, 3)
        fm.frustum_device(fm.local_map_to_device(bad), tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), 0.5, out=out)
        assert int(out["status_word"].cpu()[0]) == -1, (key, at)
        for k in NAMES:
            assert untouched(full[k], 0), (key, at, k)
    # and the same handle goes on working
    out, _ = guarded_out(70, 3)
    fm.frustum_device(fm.local_map_to_device(lmap), tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), 0.5, out=out)
    assert int(out["status_word"].cpu()[0]) == 0


# ---- past one chunk of 256 (tracking_ref.CHUNK_CASES; test_tracking_ref.py asserts what each case reaches) ---------------

DISTINCT_MAPS = [k for k in tr.CHUNK_CASES if "-cap" not in k]      # the clipped cases share the long-runs map


def device_bytes(fm, lmap, prm):
    out, full = guarded_out(len(lmap["points"]), max(len(lmap["kf_start"]) - 1, 0))
    fm.frustum_device(fm.local_map_to_device(lmap), tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), float(prm["cos_limit"]), out=out)
    return {k: full[k].cpu().numpy().tobytes() for k in NAMES + ("status_word",)}


@pytest.mark.parametrize("name", DISTINCT_MAPS)
def test_runs_key_frames_and_the_frames_map_past_one_chunk(fm, host, name):
    """k_track_check's e += 256 loop and its second and third block ranges past one workgroup, the owner word met
    from several chunks and key frames, kf_of_entry over a long kf_start with repeated values, 64 distinct key frames
    in one wave of k_frustum, k_gate's i += 256"""
    lmap, prm, _, _, _ = tr.chunk_case(name)
    worst, in_band = run_all(fm, host, lmap, prm, name)
    print("device %s: worst fraction of a bar %.3f, %.2f %% in a band" % (name, worst, 100 * in_band))
    ref = tr.chunk_reference(name)
    got = fm.frustum(lmap, tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), float(prm["cos_limit"]))
    for k in ("status", "visible", "owner_kf", "n_to_match"):
        assert np.array_equal(got[k], ref[k]), k
    if name in ("long", "ladder-320-empty"):      # the call is bit-identical to a second call, guard bytes included
        first, again = device_bytes(fm, lmap, prm), device_bytes(fm, lmap, prm)
        for k in first:
            assert first[k] == again[k], k


def test_a_map_malformed_past_the_first_chunk_writes_only_status_word(fm):
    lmap, prm, _, _, _ = tr.chunk_case("long")
    n_points, n_kf = len(lmap["points"]), len(lmap["kf_start"]) - 1
    for key, at, value in tr.late_faults(lmap):
        out, full = guarded_out(n_points, n_kf)
        fm.frustum_device(fm.local_map_to_device(tr.with_fault(lmap, key, at, value)), tr.view_of(prm), prm["Ow"],
                          tr.bounds_of(prm), 0.5, out=out)
        assert int(out["status_word"].cpu()[0]) == -1, (key, at)
        for k in NAMES:
            assert untouched(full[k], 0), (key, at, k)


def test_host_entry_refusals(fm):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import MsfError
    lmap, prm, _, _ = tr.scene(4, n_points=70, n_kf=3, per_kf=20, n_cur=8, list_len=10)
    args = (tr.view_of(prm), prm["Ow"])
    for key, at, value, text in [("kf_point", 5, 70, "kf_point is out of range"), ("kf_key", 3, tr.W * tr.H, "outside the image"),
                                 ("kf_key", 1, int(lmap["kf_key"][0]), "strictly increasing"), ("kf_start", 3, 1, "kf_start"),
                                 ("cur_key", 2, -5, "cur_key"), ("cur_point", 1, 70, "cur_point")]:
        bad = {k: v.copy() for k, v in lmap.items()}
        bad[key][at] = value
        with pytest.raises(MsfError) as e:
            fm.frustum(bad, *args, tr.bounds_of(prm))
        assert e.value.code == _lib.MSF_ERR_INVALID_ARG and "msf_frustum: " in str(e.value) and text in str(e.value), str(e.value)
    bad = {k: v.copy() for k, v in lmap.items()}
    bad["points"]["flags"][3] = 8
    with pytest.raises(MsfError) as e:
        fm.frustum(bad, *args, tr.bounds_of(prm))
    assert "flag bits" in str(e.value)
    with pytest.raises(MsfError) as e:
        fm.frustum(lmap, *args, (0.0, float("nan"), 0.0, 480.0))
    assert "NaN" in str(e.value)
    with pytest.raises(MsfError) as e:
        fm.frustum(lmap, *args, tr.bounds_of(prm), viewing_cos_limit=float("nan"))
    assert "NaN" in str(e.value)
