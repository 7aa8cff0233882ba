"""GPU: csrc/hip_tracking.h (msf::LocalPointSearch, msf::TrackLocalMap), built with plain g++ against libmsf.so, gives
for a frame and its local key frames what search_local_points gives through the Python wrapper -- the same claim records
in the same order, the same counts, and from Frustum() on the staged map the same statuses -- and through TrackLocalMap
the pose and the flags msf_pose_optimize gives on the host-gathered correspondences, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import tracking_ref as tr
from tests.test_create_map_points_gpu import H, SHIFTS, W
from tests.test_search_local_points_gpu import CAP, GATED, local_map_from_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _build(tmp_path):
    from mono_slam_framework_amd import build
    lib = build.lib_path()
    exe = str(tmp_path / "test_tracking_mirror")
    pkg = os.path.join(ROOT, "mono_slam_framework_amd")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(pkg, "csrc"), "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_tracking_mirror.cpp"), lib,
                           "-Wl,-rpath," + pkg, "-Wl,-rpath," + os.path.join(rocm, "lib"), "-L" + os.path.join(rocm, "lib"),
                           "-lamdhip64", "-o", exe])
    return exe


def test_mirror_equals_search_local_points_and_pose_optimize(tmp_path):
    from mono_slam_framework_amd import _lib, synth
    from mono_slam_framework_amd.matcher import FeatureMatcher
    exe = _build(tmp_path)
    frames = [synth.synth_pair(3, W, H, shift=(0, 0))[0]] + [synth.synth_pair(3, W, H, shift=s)[1] for s in SHIFTS]
    slots = list(range(1, len(frames)))
    fm = FeatureMatcher(0.8, W, H, max_batch_pairs=8)
    try:
        for i, f in enumerate(frames):
            fm.store_frame(i, f)
        _, _, lists0 = fm.match_one_to_many(0, slots, cap=CAP)
        prm = tr.camera(1)
        lmap = local_map_from_lists(lists0, prm)
        args = (tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), 0.5)
        exp = fm.search_local_points(0, slots, lmap, *args, cap=CAP)
        Tcw0 = np.concatenate([prm["Rcw"].reshape(3, 3), prm["tcw"].reshape(3, 1)], 1).astype(np.float32).reshape(12)
        K = (float(prm["fx"]), float(prm["fy"]), float(prm["cx"]), float(prm["cy"]))
        pose = fm.pose_optimize(exp["corr_p3d"], exp["corr_p2d"], K, Tcw0, diagnostics=False)
        params = fm._frustum_params(*args)
    finally:
        fm.close()
    f_frames, f_map, f_out = str(tmp_path / "frames.bin"), str(tmp_path / "map.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(np.stack(frames)).tofile(f_frames)
    n_points, n_kf = len(lmap["points"]), len(slots)
    with open(f_map, "wb") as fo:
        fo.write(np.array([n_points, n_kf, len(lmap["kf_key"]), len(lmap["cur_key"])], np.int32).tobytes())
        for k in ("points", "kf_start", "kf_key", "kf_point", "cur_key", "cur_point"):
            fo.write(np.ascontiguousarray(lmap[k]).tobytes())
        fo.write(bytes(params))
        fo.write(np.concatenate([Tcw0, [0, 0, 0, 1]]).astype(np.float32).tobytes())
    r = subprocess.run([exe, f_frames, f_map, f_out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(f_out, "rb").read()
    n_claims, n_corr, n_good, np_, nk_ = np.frombuffer(raw, np.int32, 5)
    at = [20]

    def take(dtype, count):
        a = np.frombuffer(raw, dtype, count, at[0])
        at[0] += a.nbytes
        return a
    claims = take(_lib.LOCAL_CLAIM_DTYPE, n_claims)
    num, ntm, f_ntm = take(np.int32, n_kf), take(np.int32, n_kf), take(np.int32, n_kf)
    f_status, f_visible, f_owner = take(np.uint8, n_points), take(np.uint8, n_points), take(np.int32, n_points)
    Tcw, flags = take(np.float32, 16), take(np.uint8, n_corr)
    assert at[0] == len(raw) and (np_, nk_) == (n_points, n_kf)
    print(r.stdout.strip(), "| wrapper: %d claims, %d correspondences, n_good %d" % (exp["n_claims"], exp["n_corr"], pose["n_good"]))
    assert n_claims == exp["n_claims"] >= 20 and n_corr == exp["n_corr"]
    assert claims.tobytes() == exp["claims"].tobytes()                      # the same records in the same order
    assert np.array_equal(num, exp["num_matches"]) and num[GATED] == -1
    fr = exp["frustum"]
    assert np.array_equal(ntm, fr["n_to_match"]) and np.array_equal(f_ntm, fr["n_to_match"]) and ntm[GATED] == 0
    assert np.array_equal(f_status, fr["status"]) and np.array_equal(f_visible, fr["visible"]) and np.array_equal(f_owner, fr["owner_kf"])
    # the pose through TrackLocalMap equals msf_pose_optimize on the host-gathered correspondences
    assert n_good == pose["n_good"] >= 20 and pose["rounds_run"] == 4 and 0 < flags.sum() < n_corr
    assert Tcw[:12].tobytes() == pose["Tcw"].tobytes() and list(Tcw[12:]) == [0, 0, 0, 1]
    assert np.array_equal(flags, pose["outliers"])
