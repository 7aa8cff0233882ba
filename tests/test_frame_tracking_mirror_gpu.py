"""GPU: csrc/hip_tracking.h (msf::FrameTracker, msf::TrackFrame), built with plain g++ against libmsf.so, gives for a
frame, its predecessor and its local key frames what the Python wrapper gives: FrameTracker::Track() the records, the
kept map, the removed records and the pose of track_frame, and TrackFrame() -- the tracked-frame branch of
Tracking::Track in two calls -- the final pose and flags of the two calls made by hand (track_frame, MSF_POINT_SEEN on
kept and removed, the frame's view from the new pose, search_local_points, pose_optimize), bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import tracking_ref as tr
from tests.test_create_map_points_gpu import H, SHIFTS, W
from tests.test_track_frame_gpu import frame_map_from_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
CAP = 2048
N_KF = 3


def _build(tmp_path):
    from mono_slam_framework_amd import build
    lib = build.lib_path()
    exe = str(tmp_path / "test_frame_tracking_mirror")
    pkg = os.path.join(ROOT, "mono_slam_framework_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(pkg, "csrc"), "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_frame_tracking_mirror.cpp"), lib,
                           "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-L" + os.path.join(rocm, "lib"),
                           "-lamdhip64", "-o", exe])
    return exe


def camera_centre(Tcw):
    """mOw = -mRcw' mtcw with f32 products summed left to right, as msf::TrackFrame computes it"""
    R, t = Tcw.reshape(3, 4)[:, :3], Tcw.reshape(3, 4)[:, 3]
    Ow = np.zeros(3, np.float32)
    for c in range(3):
        s = np.float32(0)
        for r in range(3):
            s = np.float32(s + np.float32(R[r, c] * t[r]))
        Ow[c] = -s
    return Ow


def scene(fm, lists, prm):
    """-> (fmap over one point table, local map on the same table): key frame 0 is the train frame with its own map,
    the others hold a point under the train end of every second match, where the frame sees its query end"""
    rng = np.random.default_rng(2)
    fmap = frame_map_from_list(lists[0], prm)
    R, t = prm["Rcw"].reshape(3, 3).astype(np.float64), prm["tcw"].astype(np.float64)
    extra, kf_start, kf_key, kf_point = [], [0, len(fmap["ref_key"])], list(fmap["ref_key"]), list(fmap["ref_point"])
    base = len(fmap["points"])
    for l in lists[1:]:
        seen_at = {}
        for (x1, y1, x2, y2) in l[1::2]:
            seen_at.setdefault(int(y2) * W + int(x2), (int(x1), int(y1)))
        for k in sorted(seen_at):
            z = rng.uniform(2, 8)
            px, py = seen_at[k]
            pc = np.array([(px - 320) / 500 * z, (py - 240) / 500 * z, z])
            kf_key.append(k)
            kf_point.append(base + len(extra))
            extra.append((R.T @ (pc - t)).astype(np.float32))
        kf_start.append(len(kf_key))
    pts = np.zeros(base + len(extra), tr.MAP_POINT)
    pts["pos"][:base] = fmap["points"]["pos"]
    pts["pos"][base:] = np.array(extra, np.float32).reshape(-1, 3)
    po = pts["pos"].astype(np.float64) - prm["Ow"].astype(np.float64)
    pts["normal"] = (po / np.linalg.norm(po, axis=1, keepdims=True)).astype(np.float32)
    pts["max_distance"] = 100.0
    observed = np.ones(len(pts), np.uint8)
    observed[:base] = fmap["observed"]
    fmap = dict(fmap, points=pts, observed=observed)
    lmap = fm.make_local_map(pts, kf_start, kf_key, kf_point)
    return fmap, lmap


def test_mirror_equals_the_wrapper_and_the_two_calls_by_hand(tmp_path):
    from mono_slam_framework_amd import _lib, synth
    from mono_slam_framework_amd.matcher import FeatureMatcher
    exe = _build(tmp_path)
    frames = [synth.synth_pair(3, W, H, shift=(0, 0))[0]] + [synth.synth_pair(3, W, H, shift=s)[1] for s in SHIFTS[:N_KF]]
    slots = list(range(1, len(frames)))
    prm = tr.camera(1)
    Tcw0 = np.concatenate([prm["Rcw"].reshape(3, 3), prm["tcw"].reshape(3, 1)], 1).astype(np.float32).reshape(12)
    K = (float(prm["fx"]), float(prm["fy"]), float(prm["cx"]), float(prm["cy"]))
    fm = FeatureMatcher(0.8, W, H, max_batch_pairs=8)
    try:
        for i, f in enumerate(frames):
            fm.store_frame(i, f)
        _, _, lists0 = fm.match_one_to_many(0, slots, cap=CAP)
        fmap, lmap = scene(fm, lists0, prm)
        exp = fm.track_frame(0, 1, fmap, K, Tcw0, cap=CAP, want_list=False)
        assert exp["track_status"] == 0 and exp["n_removed"] > 0
        # the second call by hand
        pts = lmap["points"].copy()
        pts["flags"][exp["kept_point"]] |= tr.SEEN
        pts["flags"][exp["removed"]["point"]] |= tr.SEEN
        hand = dict(lmap, points=pts, cur_key=exp["kept_key"], cur_point=exp["kept_point"])
        T = exp["Tcw"].reshape(3, 4)
        view = (T[:, :3], T[:, 3], *K)
        search = fm.search_local_points(0, slots, hand, view, camera_centre(exp["Tcw"]), tr.bounds_of(prm), 0.5, cap=CAP)
        pose = fm.pose_optimize(search["corr_p3d"], search["corr_p2d"], K, exp["Tcw"], diagnostics=False)
        params = fm._frustum_params(tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), 0.5)
    finally:
        fm.close()
    f_frames, f_map, f_out = str(tmp_path / "frames.bin"), str(tmp_path / "map.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(np.stack(frames)).tofile(f_frames)
    with open(f_map, "wb") as fo:
        fo.write(np.array([len(fmap["points"]), len(fmap["ref_key"]), len(fmap["cur_key"]), N_KF, len(lmap["kf_key"]), 1], np.int32).tobytes())
        for a in (fmap["points"], fmap["observed"], fmap["ref_key"], fmap["ref_point"], fmap["cur_key"], fmap["cur_point"],
                  lmap["kf_start"], lmap["kf_key"], lmap["kf_point"]):
            fo.write(np.ascontiguousarray(a).tobytes())
        fo.write(bytes(params))
        fo.write(np.concatenate([Tcw0, [0, 0, 0, 1]]).astype(np.float32).tobytes())
    r = subprocess.run([exe, f_frames, f_map, f_out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(f_out, "rb").read()
    (status, num, n_good, n_seen, n_map, n_kept, n_removed, final_good, n_corr, n_claims) = np.frombuffer(raw, np.int32, 10)
    at = [40]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype, count, at[0])
        at[0] += a.nbytes
        return a
    recs, kept_key, kept_point = take(_lib.FRAME_POINT_DTYPE, n_map), take(np.int32, n_kept), take(np.int32, n_kept)
    removed, Tcw, claims = take(_lib.REMOVED_POINT_DTYPE, n_removed), take(np.float32, 16), take(_lib.LOCAL_CLAIM_DTYPE, n_claims)
    Tfinal, flags = take(np.float32, 16), take(np.uint8, max(n_corr, 0))
    assert at[0] == len(raw)
    print(r.stdout.strip(), "| wrapper: n_map %d, kept %d, n_good %d; then %d claims, n_good %d" % (
        exp["n_map"], exp["n_kept"], exp["n_good"], search["n_claims"], pose["n_good"]))
    # Track() against the wrapper
    assert (status, num, n_good, n_seen) == (exp["track_status"], exp["num_matches"], exp["n_good"], exp["n_matches_map"])
    assert recs.tobytes() == exp["map"].tobytes() and removed.tobytes() == exp["removed"].tobytes()
    assert np.array_equal(kept_key, exp["kept_key"]) and np.array_equal(kept_point, exp["kept_point"])
    assert Tcw[:12].tobytes() == exp["Tcw"].tobytes() and list(Tcw[12:]) == [0, 0, 0, 1]
    # TrackFrame() against the two calls made by hand
    assert n_claims == search["n_claims"] and claims.tobytes() == search["claims"].tobytes() and n_corr == search["n_corr"]
    assert final_good == pose["n_good"] and Tfinal[:12].tobytes() == pose["Tcw"].tobytes()
    assert np.array_equal(flags, pose["outliers"])
    assert n_claims >= 10 and pose["n_good"] >= 20
