#!/usr/bin/env python3
"""Measurement for PnPsolver on the device (include/msf_pnp.h): the relocalization workload -- 20 candidate lists of 96
correspondences, 35 RANSAC iterations each (what SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) works out to) -- as one
msf_pnp_ransac_device call on device-resident lists, and one list of 96 with 300 iterations.  Each call is timed with a
pair of device events on the handle's work (the call is synchronous on the handle's stream); the medians are reported.
Beside them: the single-thread host build of csrc/pnp_solve.h (tests/cpp/pnp_solve_host.cpp, g++ -O2) on the same
lists and the sets the device drew -- the same arithmetic on one CPU thread, NOT the reference's PnPsolver (no OpenCV
here).  Prints one JSON line and writes it to --out."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_ransac.json"))
    a = ap.parse_args()
    import torch
    from mono_slam_framework_amd.matcher import FeatureMatcher
    from tests import pnp_host
    from tests import pnp_ref as pr
    assert torch.cuda.is_available(), "this measurement needs the GPU: a CPU run says nothing about it"
    fm = FeatureMatcher(0.8, 640, 480)
    host = pnp_host.build(tempfile.mkdtemp(prefix="pnp_host_"))
    floor, its = pr.set_ransac_parameters(96)
    result = {"calls": a.calls, "warmup": a.warmup, "min_inliers": floor}
    for name, n_lists, n_it in (("relocalization_20x96x35", 20, its), ("one_list_96x300", 1, 300)):
        scenes = [pr.scene(("base", "wide", "shallow")[i % 3], 1 + i % 3) for i in range(n_lists)]
        K = scenes[0]["K"]
        d_p3 = torch.from_numpy(np.stack([s["p3d"] for s in scenes])).cuda()
        d_p2 = torch.from_numpy(np.stack([s["p2d"] for s in scenes])).cuda()
        d_n = torch.full((n_lists,), 96, dtype=torch.int32, device="cuda")
        out = fm.pnp_ransac_device(d_p3, d_p2, d_n, K, floor, n_it, seed=1, max_records=8)
        sets = out["sets"].cpu().numpy()
        slim = {k: v for k, v in out.items() if not k.startswith("rec_") and k not in ("cws", "ut_tail", "betas", "rep_errors", "sets")}
        d_sets = out["sets"]

        def call():
            fm.pnp_ransac_device(d_p3, d_p2, d_n, K, floor, n_it, max_records=8, d_sets=d_sets, out=slim)

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
        records = 0
        for i, s in enumerate(scenes):
            records += pnp_host.run(host, s["p3d"], s["p2d"], K, floor, n_it, sets=sets[i])["n_records"]
        host_ms = (time.perf_counter() - t0) * 1e3
        n_rec = out["n_records"].cpu().numpy()
        assert int(n_rec.sum()) == records, "the host build and the device disagree on the records"
        result[name] = {"lists": n_lists, "correspondences": 96, "iterations": n_it, "hypotheses": n_lists * n_it,
                        "records": int(n_rec.sum()),
                        "device_ms": {"events_median": round(float(np.median(ms)), 4),
                                      "events_p10_p90": [round(float(x), 4) for x in np.percentile(ms, [10, 90])]},
                        "host_build_one_thread_ms": round(host_ms, 3)}
    result["note"] = ("device: two launches on device-resident lists, given sets, no diagnostics; host: the same arithmetic "
                      "(csrc/pnp_solve.h, g++ -O2) on one thread including the ctypes call, not the reference's PnPsolver")
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
