#!/usr/bin/env python3
"""Measurement for LocalMapping::CreateNewMapPoints on the device: one 1280 x 720 query key frame against 20 resident
neighbours, msf_create_map_points (match + triangulate + copy-back of counts, lists and packed new points) beside
msf_match_one_to_many for the same slots (match + copy-back of counts and lists).  The difference is what the new step
costs: one kernel behind the matcher's and the copy-back of the packed records.  Calls alternate, after a warm-up; each
is timed with a pair of device events around the (synchronous) call and with the host clock; the medians are reported.
Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "create_map_points.json"))
    a = ap.parse_args()
    import torch
    from mono_slam_framework_amd import _lib, synth
    from mono_slam_framework_amd.matcher import FeatureMatcher
    assert torch.cuda.is_available(), "this measurement needs the GPU: a CPU run says nothing about it"
    W, H, N, cap = a.width, a.height, a.neighbours, a.cap
    fm = FeatureMatcher(0.8, W, H, max_batch_pairs=N)
    rng = np.random.RandomState(7)
    f, depth = 900.0, 5.0
    shifts = [(int(rng.randint(-30, 31)), int(rng.randint(-30, 31))) for _ in range(N)]
    fm.store_frame(0, synth.synth_pair(11, W, H, shift=(0, 0))[0])
    views = []
    for i, (dx, dy) in enumerate(shifts):
        fm.store_frame(1 + i, synth.synth_pair(11, W, H, shift=(dx, dy))[1])
        views.append((np.eye(3), np.array([-dx, -dy, 0.0]) * depth / f, f, f, W / 2, H / 2))
    qv = fm.make_views([(np.eye(3), np.zeros(3), f, f, W / 2, H / 2)])
    nv = fm.make_views(views)
    slots = np.arange(1, N + 1, dtype=np.int32)
    num = np.zeros(N, np.int32)
    lists = np.zeros((N, cap), _lib.MATCH_DTYPE)
    n_new = np.zeros(N, np.int32)
    packed = np.zeros((N, cap), _lib.NEW_POINT_DTYPE)
    prm = _lib.NewPointsParams(struct_size=C.sizeof(_lib.NewPointsParams), max_cos_parallax=1.1, chi2=5.991)
    res = _lib.NewPointsResult(struct_size=C.sizeof(_lib.NewPointsResult), n_new=n_new.ctypes.data, packed=packed.ctypes.data)
    L, h = fm._L, fm._h

    def create():
        fm._check(L.msf_create_map_points(h, 0, qv.ctypes.data, N, slots.ctypes.data, nv.ctypes.data, C.byref(prm),
                                          num.ctypes.data, lists.ctypes.data, cap, C.byref(res)))

    def match_only():
        fm._check(L.msf_match_one_to_many(h, 0, N, slots.ctypes.data, num.ctypes.data, None, lists.ctypes.data, cap))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        create()
        match_only()
    t = {"create": [], "match": []}
    for _ in range(a.calls):
        t["create"].append(timed(create))
        t["match"].append(timed(match_only))
    med = {k: np.median(np.array(v), axis=0) for k, v in t.items()}
    spread = {k: np.percentile(np.array(v)[:, 0], [10, 90]) for k, v in t.items()}
    result = {
        "workload": "ORB %dx%d: one query key frame vs %d resident neighbours, lists of up to %d matches" % (W, H, N, cap),
        "calls": a.calls, "warmup": a.warmup,
        "mean_matches_per_neighbour": round(float(np.clip(num, 0, None).mean()), 1),
        "new_points_per_call": int(np.clip(n_new, 0, None).sum()),
        "create_map_points_ms": {"events_median": round(float(med["create"][0]), 4), "host_clock_median": round(float(med["create"][1]), 4),
                                 "events_p10_p90": [round(float(x), 4) for x in spread["create"]]},
        "match_one_to_many_ms": {"events_median": round(float(med["match"][0]), 4), "host_clock_median": round(float(med["match"][1]), 4),
                                 "events_p10_p90": [round(float(x), 4) for x in spread["match"]]},
        "added_ms": round(float(med["create"][0] - med["match"][0]), 4),
        "copy_back": "both: counts + lists (one copy per neighbour); create_map_points adds n_new and one copy of packed records per neighbour",
    }
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
