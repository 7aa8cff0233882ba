#!/usr/bin/env python3
"""Measurement for Tracking::SearchLocalPoints on the device: one 1280 x 720 frame against 20 resident key frames with
about 1 000 map points each.  msf_search_local_points (records only, and with keep_on_device) beside
msf_match_one_to_many on the same slots in the same run; the difference is what the frustum test, the gate and the
claims add.  Beside them the single-thread host build of steps 1-5 (csrc/tracking_solve.h) on the same lists.  Calls
alternate, after a warm-up; each is timed with a pair of device events around the (synchronous) call and with the host
clock; the medians are reported.  Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=20)
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_local_points.json"))
    a = ap.parse_args()
    import torch
    from mono_slam_framework_amd import _lib, synth
    from mono_slam_framework_amd.matcher import FeatureMatcher
    from tests import tracking_host as th
    assert torch.cuda.is_available(), "this measurement needs the GPU: a CPU run says nothing about it"
    W, H, N, cap = a.width, a.height, a.keyframes, a.cap
    fm = FeatureMatcher(0.8, W, H, max_batch_pairs=N)
    rng = np.random.RandomState(7)
    f = 900.0
    fm.store_frame(0, synth.synth_pair(11, W, H, shift=(0, 0))[0])
    for i in range(N):
        fm.store_frame(1 + i, synth.synth_pair(11, W, H, shift=(int(rng.randint(-30, 31)), int(rng.randint(-30, 31))))[1])
    slots = np.arange(1, N + 1, dtype=np.int32)
    num0, _, lists0 = fm.match_one_to_many(0, slots, cap=cap)
    # the local map: per key frame a point under the train end of its matches, filled up to --points with other pixels;
    # identity camera, every point in front of it and seen head-on; the frame holds a point under every fifth query end
    pts, kf_start, kf_key, kf_point, cur = [], [0], [], [], {}
    for i, l in enumerate(lists0):
        keys = set(int(y2) * W + int(x2) for (_, _, x2, y2) in l)
        while len(keys) < a.points:
            keys.add(int(rng.randint(W * H)))
        for k in sorted(keys)[:max(a.points, 1)]:
            z = rng.uniform(2, 8)
            pos = np.array([(k % W - W / 2) / f * z, (k // W - H / 2) / f * z, z], np.float32)
            kf_key.append(k)
            kf_point.append(len(pts))
            pts.append((pos, pos / np.linalg.norm(pos), 100.0, 0))
        kf_start.append(len(kf_key))
        for (x1, y1, _, _) in l[::5]:
            cur.setdefault(int(y1) * W + int(x1), len(pts) - 1)
    points = np.array(pts, _lib.MAP_POINT_DTYPE)
    cur_key = sorted(cur)
    points["flags"][[cur[k] for k in cur_key]] |= _lib.MSF_POINT_SEEN
    lmap = fm.make_local_map(points, kf_start, kf_key, kf_point, cur_key, [cur[k] for k in cur_key])
    view = (np.eye(3), np.zeros(3), f, f, W / 2, H / 2)
    prm = fm._frustum_params(view, np.zeros(3), (0.0, float(W), 0.0, float(H)), 0.5)
    m, n_points, n_kf = fm._local_map(lmap)
    num = np.zeros(N, np.int32)
    word, ntm, ncl, nclk = np.zeros(2, np.int32), np.zeros(N, np.int32), np.zeros(1, np.int32), np.zeros(N, np.int32)
    visible = np.zeros(n_points, np.uint8)
    records = np.zeros(N * cap, _lib.LOCAL_CLAIM_DTYPE)
    fr = _lib.FrustumResult(struct_size=C.sizeof(_lib.FrustumResult), status_word=word.ctypes.data, n_to_match=ntm.ctypes.data,
                            visible=visible.ctypes.data)
    cl = _lib.ClaimResult(struct_size=C.sizeof(_lib.ClaimResult), status_word=word.ctypes.data + 4, n_claims=ncl.ctypes.data,
                          n_claimed=nclk.ctypes.data, claims=records.ctypes.data)
    keep = _lib.DeviceCorr(struct_size=C.sizeof(_lib.DeviceCorr))
    L, h = fm._L, fm._h

    def search():
        fm._check(L.msf_search_local_points(h, 0, slots.ctypes.data, C.byref(m), C.byref(prm), 0, num.ctypes.data, None, cap,
                                            C.byref(fr), C.byref(cl), None))

    def search_keep():
        fm._check(L.msf_search_local_points(h, 0, slots.ctypes.data, C.byref(m), C.byref(prm), _lib.MSF_SEARCH_KEEP_ON_DEVICE,
                                            num.ctypes.data, None, cap, C.byref(fr), C.byref(cl), C.byref(keep)))

    def match_only():
        fm._check(L.msf_match_one_to_many(h, 0, N, slots.ctypes.data, num.ctypes.data, None, None, 0))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    fns = {"search": search, "search_keep": search_keep, "match": match_only}
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    t = {k: [] for k in fns}
    for _ in range(a.calls):
        for k, fn in fns.items():
            t[k].append(timed(fn))
    med = {k: np.median(np.array(v), axis=0) for k, v in t.items()}
    # the host build of steps 1-5 on the same lists, one thread
    with tempfile.TemporaryDirectory() as tmp:
        host = th.build(tmp)
        prm_ref = dict(Rcw=np.eye(3, dtype=np.float32).reshape(9), tcw=np.zeros(3, np.float32), fx=f, fy=f, cx=W / 2, cy=H / 2,
                       Ow=np.zeros(3, np.float32), min_x=0.0, max_x=float(W), min_y=0.0, max_y=float(H), cos_limit=0.5)
        padded = th.pad_lists(lists0, cap)
        matched = (ntm > 0).astype(np.uint8)
        host_ms = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            hf = th.frustum(host, lmap, prm_ref, W, H)
            hc = th.claims(host, lmap, padded, num0, matched, len(cur_key) + N * cap, W, H)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(hf["n_to_match"], ntm) and hc["n_claims"] == int(ncl[0])
    ms = lambda k: {"events_median": round(float(med[k][0]), 4), "host_clock_median": round(float(med[k][1]), 4)}
    result = {
        "workload": "ORB %dx%d: one frame vs %d resident key frames of %d map points, lists of up to %d matches" % (W, H, N, a.points, cap),
        "calls": a.calls, "warmup": a.warmup, "points": int(n_points), "entries": int(len(kf_key)), "n_cur": len(cur_key),
        "mean_matches_per_key_frame": round(float(np.clip(num0, 0, None).mean()), 1), "claims_per_call": int(ncl[0]),
        "search_local_points_ms": ms("search"), "search_local_points_keep_on_device_ms": ms("search_keep"),
        "match_one_to_many_ms": ms("match"),
        "added_ms": round(float(med["search"][0] - med["match"][0]), 4),
        "added_keep_on_device_ms": round(float(med["search_keep"][0] - med["match"][0]), 4),
        "host_build_steps_1_to_5_ms": round(float(np.median(host_ms)), 4),
        "copy_back": "search: counts, n_to_match, visible, claim records; match: counts only",
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
