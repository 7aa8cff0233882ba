#!/usr/bin/env python3
"""Measurement for bundle adjustment on the device (include/msf_ba.h): one LocalBundleAdjustment problem of 20 free and
10 fixed key frames, 1500 points and about 4 observations each; one BundleAdjustment(20) of the two-key-frame initial
map with 300 points; and a batch of 8 of the first, each as one msf_bundle_adjust_device call on device-resident
arrays without diagnostics.  Each call is timed with a pair of device events on the handle's work (the call is
synchronous on the handle's stream); the medians of --calls calls are reported.  Beside them: the single-thread host
build of csrc/ba_solve.h (tests/cpp/ba_solve_host.cpp, g++ -O2) on the same problems -- the same arithmetic on one CPU
thread, NOT the reference's g2o (there is no g2o here).  Prints one JSON line and writes it to --out."""
import argparse
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
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_ba.json"))
    a = ap.parse_args()
    import torch
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher
    from tests import ba_host
    from tests import ba_ref as br
    assert torch.cuda.is_available(), "this measurement needs the GPU: a CPU run says nothing about it"
    fm = FeatureMatcher(0.8, 640, 480)
    host = ba_host.build(tempfile.mkdtemp(prefix="ba_host_"))
    result = {"calls": a.calls, "warmup": a.warmup}
    local = [br.make_scene(20, 10, 1500, None, 1 + i) for i in range(8)]
    initial = br.make_scene(2, 0, 300, None, 1)
    for name, scenes, schedule in (("local_20+10x1500", local[:1], br.LOCAL_BA), ("initial_2+0x300", [initial], br.INITIAL_BA),
                                   ("batch_8x_local_20+10x1500", local, br.LOCAL_BA)):
        desc, c0, p0, e0 = [], 0, 0, 0
        for s in scenes:
            nc, npt, ne = len(s["cam_Tcw"]), len(s["points"]), len(s["edge_cam"])
            desc.append((nc, npt, ne, c0, p0, e0))
            c0, p0, e0 = c0 + nc, p0 + npt, e0 + ne
        cat = lambda key, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate([s[key] for s in scenes]), dt)).cuda()
        args = (torch.tensor(desc, dtype=torch.int32, device="cuda"), cat("cam_Tcw", np.float32), cat("cam_fixed", np.uint8),
                cat("points", np.float32), cat("edge_cam", np.int32), cat("edge_point", np.int32), cat("edge_obs", np.float32),
                br.K)
        max_free = max(int((s["cam_fixed"] == 0).sum()) for s in scenes)
        slim = fm.bundle_adjust_device(*args, schedule=schedule, max_free_cams=max_free, diagnostics=False)
        trials = torch.zeros((len(scenes), _lib.BA_SLOTS), dtype=torch.int32, device="cuda")
        fm.bundle_adjust_device(*args, schedule=schedule, max_free_cams=max_free, out=dict(slim, it_trials=trials))
        ms = []
        for i in range(a.warmup + a.calls):
            e0_, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0_.record()
            fm.bundle_adjust_device(*args, schedule=schedule, max_free_cams=max_free, out=slim)
            e1_.record()
            e1_.synchronize()
            if i >= a.warmup:
                ms.append(e0_.elapsed_time(e1_))
        t0 = time.perf_counter()
        flagged = [int(ba_host.run(host, s, schedule, max_free=max_free, diagnostics=False)["outliers"].sum()) for s in scenes]
        host_ms = (time.perf_counter() - t0) * 1e3
        out = slim["outliers"].cpu().numpy()
        mine = [int(out[d[5]:d[5] + d[2]].sum()) for d in desc]
        trials = trials.cpu().numpy()
        result[name] = {"problems": len(scenes), "free_fixed_points_edges": [max_free, desc[0][0] - max_free, desc[0][1], desc[0][2]],
                        "status": slim["status"].cpu().numpy().tolist(), "flagged_device_host": [sum(mine), sum(flagged)],
                        "iterations": int((trials != 0).sum()), "trials": int(trials.sum()),
                        "device_ms": {"events_median": round(float(np.median(ms)), 4),
                                      "events_p10_p90": [round(float(x), 4) for x in np.percentile(ms, [10, 90])]},
                        "host_build_one_thread_ms": round(host_ms, 3)}
    result["note"] = ("device: one launch on device-resident arrays, one workgroup per problem, no diagnostics; host: the same "
                      "arithmetic (csrc/ba_solve.h, g++ -O2) on one thread including the ctypes call, not the reference's g2o, "
                      "which was not measured")
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
