#!/usr/bin/env python3
"""Measurement for PoseOptimization on the device (include/msf_pose.h): the relocalization workload -- 20 candidate
lists of 96 correspondences -- as one msf_pose_optimize_device call on device-resident lists, and one list of 500 (a
tracked frame).  Each call is timed with a pair of device events on the handle's work (the call is synchronous on the
handle's stream); the medians of --calls calls are reported.  Beside them: the single-thread host build of
csrc/pose_solve.h (tests/cpp/pose_solve_host.cpp, g++ -O2) on the same lists -- the same arithmetic on one CPU thread,
NOT the reference's g2o (there is no g2o here).  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_optimize.json"))
    a = ap.parse_args()
    import torch
    from mono_slam_framework_amd.matcher import FeatureMatcher
    from tests import pose_host
    from tests import pose_ref as pr
    assert torch.cuda.is_available(), "this measurement needs the GPU: a CPU run says nothing about it"
    fm = FeatureMatcher(0.8, 640, 480)
    host = pose_host.build(tempfile.mkdtemp(prefix="pose_host_"))
    result = {"calls": a.calls, "warmup": a.warmup}
    for name, n_lists, n in (("relocalization_20x96", 20, 96), ("one_list_500", 1, 500)):
        scenes = [pr.scene(("base", "wide", "shallow")[i % 3], 1 + i % 3, n) for i in range(n_lists)]
        K = scenes[0]["K"]
        d_p3 = torch.from_numpy(np.stack([s["p3d"] for s in scenes])).cuda()
        d_p2 = torch.from_numpy(np.stack([s["p2d"] for s in scenes])).cuda()
        d_t0 = torch.from_numpy(np.stack([s["Tcw0"] for s in scenes])).cuda()
        d_n = torch.full((n_lists,), n, dtype=torch.int32, device="cuda")
        full = fm.pose_optimize_device(d_p3, d_p2, d_n, K, d_t0)
        slim = fm.pose_optimize_device(d_p3, d_p2, d_n, K, d_t0, diagnostics=False)

        def call():
            fm.pose_optimize_device(d_p3, d_p2, d_n, K, d_t0, out=slim)

        ms = []
        for i in range(a.warmup + a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        good = [pose_host.run(host, s["p3d"], s["p2d"], K, s["Tcw0"])["n_good"] for s in scenes]
        host_ms = (time.perf_counter() - t0) * 1e3
        n_good = slim["n_good"].cpu().numpy()
        assert n_good.tolist() == good, "the host build and the device disagree on n_good"
        trials = full["it_trials"].cpu().numpy()
        result[name] = {"lists": n_lists, "correspondences": n, "n_good": int(n_good.sum()),
                        "iterations": int((trials != 0).sum()), "trials": int(trials.sum()),
                        "device_ms": {"events_median": round(float(np.median(ms)), 4),
                                      "events_p10_p90": [round(float(x), 4) for x in np.percentile(ms, [10, 90])]},
                        "host_build_one_thread_ms": round(host_ms, 3)}
    result["note"] = ("device: one launch on device-resident lists, no diagnostics; host: the same arithmetic "
                      "(csrc/pose_solve.h, g++ -O2) on one thread including the ctypes call and its diagnostics, not the "
                      "reference's g2o, which was not measured")
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
