#!/usr/bin/env python3
"""Times msf_reconstruct and msf_reconstruct_device on one GPU and writes profiles/reconstruct.txt (or --out FILE).

  single   one msf_reconstruct call: 300 matches, host pointers in and out; wall time of 50 calls after 5 warm-up calls
  batch    one msf_reconstruct_device call on 1024 lists x 300 matches (cap 512) fed by msf_find_models_device;
           HIP events around 10 calls on one stream after 2 warm-up calls
  trace    the batch under `rocprofv3 --kernel-trace --stats`: the time per kernel

Every step is a fresh child process under its own time limit; the first step that fails ends the run (nothing more is
started on the GPU after a fault).  Matches: the scenes of tests/ransac_ref.py, as in profiles/ransac_find_models.txt.

usage: tools/bench_reconstruct.py [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = [[500, 0, 320], [0, 500, 240], [0, 0, 1]]
KERNELS = ("k_motion_candidates", "k_check_rt", "k_pick_motion", "k_winner_points")
LIMITS = {"single": 120, "batch": 180, "trace": 300}


def _batch(n_lists, cap=512):
    import numpy as np
    import torch
    from tests import ransac_ref as rr
    lists = np.zeros((n_lists, cap, 4), np.int32)
    scenes = {}
    for i in range(n_lists):
        key = (rr.SCENES[i % 2], 1 + i % 7)
        if key not in scenes:
            scenes[key] = rr.scene(*key)[0]
        lists[i, :rr.N_MATCHES] = scenes[key]
    return torch.from_numpy(lists).cuda(), torch.full((n_lists,), rr.N_MATCHES, dtype=torch.int32, device="cuda")


def step_single():
    import numpy as np
    from mono_slam_framework_amd.matcher import FeatureMatcher
    from tests import ransac_ref as rr
    fm = FeatureMatcher(0.7, rr.W, rr.H)
    m, _ = rr.scene("planar", 1)
    found = fm.find_models(m, rr.draw_sets(len(m), 200, 1), 1.0)["H"]
    args = (0, found["m21"][found["best"]], m, found["best_inliers"], np.array(K, np.float32))
    for _ in range(5):
        res = fm.reconstruct(*args)
    ms = []
    for _ in range(50):
        t0 = time.perf_counter()
        fm.reconstruct(*args)
        ms.append((time.perf_counter() - t0) * 1e3)
    fm.close()
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), ok=res["ok"], n_good=int(res["cand_good"].max()))


def step_batch(calls=10, warmup=2):
    import numpy as np
    import torch
    from mono_slam_framework_amd.matcher import FeatureMatcher
    from tests import ransac_ref as rr
    fm = FeatureMatcher(0.7, rr.W, rr.H)
    d_m, d_n = _batch(1024)
    found = fm.find_models_device(d_m, d_n, n_hyp=200, seed=1)
    stream = torch.cuda.current_stream().cuda_stream
    Kf = np.array(K, np.float32)
    ms = []
    for i in range(warmup + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        res = fm.reconstruct_device(d_m, d_n, found, Kf, stream=stream)
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    out = dict(median_ms=statistics.median(ms), min_ms=min(ms), ok=int(res["ok"].sum().item()),
               homography=int((res["model"] == 0).sum().item()))
    fm.close()
    return out


def step_trace():
    """the kernels' average time per launch, in microseconds, from rocprofv3's kernel statistics"""
    if not shutil.which("rocprofv3"):
        return dict(skipped="rocprofv3 is not installed")
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable,
               os.path.abspath(__file__), "--step", "batch"]
        subprocess.run(cmd, check=True, timeout=LIMITS["batch"] + 60, stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return dict(skipped="rocprofv3 wrote no kernel statistics")
        out = {}
        for r in csv.DictReader(open(files[0])):
            for k in KERNELS:
                if k in r["Name"]:
                    out[k] = dict(avg_us=float(r["AverageNs"]) / 1e3, calls=int(r["Calls"]))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(LIMITS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reconstruct.txt"))
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps({"single": step_single, "batch": step_batch, "trace": step_trace}[a.step]()))
        return 0
    got = {}
    for step in ("single", "batch", "trace"):
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--step", step],
                           capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write("step %s failed (exit %d); nothing more is started\n%s\n" % (step, r.returncode, r.stderr[-2000:]))
            return 1
        got[step] = json.loads(line[-1][7:])
    s, b, t = got["single"], got["batch"], got["trace"]
    text = ["msf_reconstruct / msf_reconstruct_device on one MI355X (gfx950), ORB handle, matches of tests/ransac_ref.py scenes,",
            "K = 500 / 500 / 320 / 240, sigma 1, minTriangulated 50, minParallax 1.  Median (min).", "",
            "  reconstruct          300 matches, the kept H21 of 200 hypotheses, host pointers in and out (50 calls, wall)   "
            "%.3f ms (%.3f)   ok %d, nGood %d" % (s["median_ms"], s["min_ms"], s["ok"], s["n_good"]),
            "  reconstruct_device   1024 lists x 300 matches (cap 512) after find_models_device (10 calls, HIP events)        "
            "%.3f ms (%.3f)   %d lists ok, %d from H" % (b["median_ms"], b["min_ms"], b["ok"], b["homography"]), ""]
    if "skipped" in t:
        text.append("per kernel: not measured (%s)" % t["skipped"])
    else:
        text.append("rocprofv3 --kernel-trace --stats of the batch, average per launch in microseconds:")
        text += ["  %-22s %9.1f   (%d launches)" % (k, t[k]["avg_us"], t[k]["calls"]) for k in KERNELS if k in t]
    open(a.out, "w").write("\n".join(text) + "\n")
    print("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
