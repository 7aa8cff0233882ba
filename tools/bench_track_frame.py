#!/usr/bin/env python3
"""Measurement for the body of TrackWithMotionModel / TrackReferenceKeyFrame on the device: one 1280 x 720 frame against
its predecessor, with about 1 000 map points in the train frame.  msfx_track_frame (plain, and with keep_on_device)
beside the sequence it replaces, in the same run: msf_match_one_to_many for the slot with the list copied back, the
gather of the 3-D points on the host (numpy: a sorted-key lookup per match, the last match of a pixel wins, key order),
and the msf_pose_optimize host entry on the gathered list.  Calls alternate, after a warm-up; each is timed with a pair
of device events around the (synchronous) call sequence and with the host clock; the medians are reported.  Reads
nothing outside the repository.  Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_frame.json"))
    a = ap.parse_args()
    import torch
    from mono_slam_framework_amd import _lib, results, synth
    from mono_slam_framework_amd.matcher import FeatureMatcher
    assert torch.cuda.is_available(), "this measurement needs the GPU: a CPU run says nothing about it"
    W, H, cap = a.width, a.height, a.cap
    fm = FeatureMatcher(0.8, W, H, max_batch_pairs=2)
    rng = np.random.RandomState(7)
    f = 900.0
    cur, prev = synth.synth_pair(11, W, H, shift=(14, -9))
    fm.store_frame(0, cur)
    fm.store_frame(1, prev)
    num0, _, lists0 = fm.match_one_to_many(0, [1], cap=cap)
    lst = lists0[0]
    # the train frame's map: a point under the train end of every match, where the identity camera sees the query end,
    # filled up to --points with other pixels; the frame's own map is empty (TrackWithMotionModel after Clear())
    seen_at = {}
    for (x1, y1, x2, y2) in lst:
        seen_at.setdefault(int(y2) * W + int(x2), (int(x1), int(y1)))
    while len(seen_at) < a.points:
        k = int(rng.randint(W * H))
        seen_at.setdefault(k, (k % W, k // W))
    ref_key = np.array(sorted(seen_at)[:max(a.points, 1)], np.int32)
    points = np.zeros(len(ref_key), _lib.MAP_POINT_DTYPE)
    for p, k in enumerate(ref_key):
        z = rng.uniform(2, 8)
        px, py = seen_at[int(k)]
        points["pos"][p] = ((px - W / 2) / f * z, (py - H / 2) / f * z, z)
    ref_point = np.arange(len(ref_key), dtype=np.int32)
    fmap = fm.make_frame_map(points, ref_key, ref_point)
    K = (f, f, W / 2, H / 2)
    Tcw0 = np.concatenate([np.eye(3), [[0.02], [-0.01], [0.03]]], 1).astype(np.float32).reshape(12)
    m = fm._frame_map(fmap)
    prm = fm._track_params(K, Tcw0, 5.991, 15, 10)
    corr_cap = cap
    d = results.alloc(_lib.track_shapes(cap, 0, corr_cap), leave_out=("carry_status", "cur_status", "corr_p3d", "corr_p2d", "corr_point"))
    res = results.fill(_lib.TrackResult(), d)
    keep = _lib.DeviceTrack(struct_size=C.sizeof(_lib.DeviceTrack))
    num = np.zeros(1, np.int32)
    slot = np.array([1], np.int32)
    out_list = np.zeros(cap, _lib.MATCH_DTYPE)
    L, h = fm._L, fm._h

    def track():
        fm._check(L.msfx_track_frame(h, 0, 1, C.byref(m), C.byref(prm), 0, num.ctypes.data, None, cap, C.byref(res), None, None))

    def track_keep():
        fm._check(L.msfx_track_frame(h, 0, 1, C.byref(m), C.byref(prm), _lib.MSFX_TRACK_KEEP_ON_DEVICE, num.ctypes.data, None,
                                     cap, C.byref(res), None, C.byref(keep)))

    last = {}

    def replaced():
        fm._check(L.msf_match_one_to_many(h, 0, 1, slot.ctypes.data, num.ctypes.data, None, out_list.ctypes.data, cap))
        n = int(num[0])
        ml = out_list[:n].view(np.int32).reshape(-1, 4)
        inside = (ml[:, 0] >= 0) & (ml[:, 0] < W) & (ml[:, 1] >= 0) & (ml[:, 1] < H) & (ml[:, 2] >= 0) & (ml[:, 2] < W) & \
                 (ml[:, 3] >= 0) & (ml[:, 3] < H)
        k1 = ml[:, 1] * W + ml[:, 0]
        k2 = ml[:, 3] * W + ml[:, 2]
        at = np.minimum(np.searchsorted(ref_key, k2), len(ref_key) - 1)
        hit = inside & (ref_key[at] == k2)
        # SetMapPoint in list order: the last match of a pixel stays; the map iterates in key order
        keys, first_from_the_end = np.unique(k1[hit][::-1], return_index=True)
        pts = ref_point[at[hit][::-1][first_from_the_end]]
        p3d = points["pos"][pts]
        p2d = np.stack([keys % W, keys // W], 1).astype(np.float32)
        last["pose"] = fm.pose_optimize(p3d, p2d, K, Tcw0, diagnostics=False)
        last["n"] = len(keys)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    fns = {"track": track, "track_keep": track_keep, "replaced": replaced}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    # the two paths compute the same thing
    assert int(d["n_map"][0]) == last["n"] and d["Tcw"][0].tobytes() == last["pose"]["Tcw"].tobytes(), "the two sequences disagree"
    t = {k: [] for k in fns}
    for _ in range(a.calls):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    med = {k: np.median(np.array(v), axis=0) for k, v in t.items()}
    ms = lambda k: {"events_median": round(float(med[k][0]), 4), "host_clock_median": round(float(med[k][1]), 4)}
    result = {
        "workload": "ORB %dx%d: one frame vs its predecessor, %d map points in the train frame, list of up to %d matches" % (W, H, len(ref_key), cap),
        "calls": a.calls, "warmup": a.warmup, "matches": int(num0[0]), "n_map": int(d["n_map"][0]), "n_kept": int(d["n_kept"][0]),
        "n_good": int(d["n_good"][0]), "track_status": int(d["track_status"][0]),
        "track_frame_ms": ms("track"), "track_frame_keep_on_device_ms": ms("track_keep"),
        "match_gather_pose_ms": ms("replaced"),
        "copy_back": "track_frame: counts, records, pose, kept map, removed; replaced sequence: count, list, pose result without diagnostics",
        "replaced_sequence": "msf_match_one_to_many (list copied back) + numpy gather + msf_pose_optimize; the outlier cut on the host is not in it",
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")
    fm.close()


if __name__ == "__main__":
    main()
