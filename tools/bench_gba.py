#!/usr/bin/env python3
"""Measurement for the global bundle adjustment on the device (include/msf_global_ba.h): scenes of
tests/ba_ref.make_scene on device-resident arrays without diagnostics, each as one msf_global_bundle_adjust_device call
-- (200 + 1) x 1600 with the reference's schedule {1, {10, 0}, {0, 0}}, (64 + 2) x 160 and the (20 + 10) x 1500 problem
of tools/bench_ba.py with LocalBundleAdjustment's.  The call returns when the problem is finished (the host decides
every trial), so it is timed on the host's clock around the call; the medians of --calls calls are reported, with the
launches and host waits the call made (derived from its iterations and trials by the schedule of gba_kernels.hip).
Beside each, in the same run: the single-thread host build of csrc/ba_solve.h (g++ -O2; the same arithmetic on one CPU
thread, NOT the reference's g2o: there is no g2o here; the median of --host-calls runs), and where msf_bundle_adjust
takes the problem, that call on the same host clock.  The launch and wait counts come from counts() below, which
restates the Driver of gba_kernels.hip: the library exports no counter, and a change to the Driver has to be made here
too.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def counts(n_free, tile, rounds, iterations, trials, round1_ran):
    """launches and host waits of one call without diagnostics: the Driver of gba_kernels.hip"""
    n = 6 * n_free
    panels = (n + tile - 1) // tile
    row_tiles = n // tile + 1
    solve = 2 + sum(1 + (1 if row_tiles - j > 1 else 0) for j in range(panels)) if n_free else 0   # schur, back, the tiles
    per_trial = 1 + solve + 3                             # invert; step, trial cost, reduce
    launches = 1 + 2 + rounds + (2 if round1_ran else 0) + 3 * iterations + per_trial * trials + rounds + 1
    waits = 1 + (1 if round1_ran else 0) + iterations + trials + 1
    return launches, waits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_ba.json"))
    a = ap.parse_args()
    import torch
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher
    from tests import ba_host
    from tests import ba_ref as br
    assert torch.cuda.is_available(), "this measurement needs the GPU: a CPU run says nothing about it"
    fm = FeatureMatcher(0.8, 640, 480)
    host = ba_host.build(tempfile.mkdtemp(prefix="ba_host_"))
    tile = _lib.load().msf_global_ba_tile_rows()
    result = {"calls": a.calls, "warmup": a.warmup, "tile_rows": tile}
    GLOBAL = (1, (10, 0), (0, 0))
    for name, s, schedule in (("global_200+1x1600", br.make_scene(200, 1, 1600, None, 1), GLOBAL),
                              ("local_64+2x160", br.make_scene(64, 2, 160, None, 10), br.LOCAL_BA),
                              ("local_20+10x1500", br.make_scene(20, 10, 1500, None, 1), br.LOCAL_BA)):
        nc, npt, ne = len(s["cam_Tcw"]), len(s["points"]), len(s["edge_cam"])
        n_free = int((s["cam_fixed"] == 0).sum())
        t = lambda key, dt: torch.from_numpy(np.ascontiguousarray(s[key], dt)).cuda()
        args = (t("cam_Tcw", np.float32), t("cam_fixed", np.uint8), t("points", np.float32), t("edge_cam", np.int32),
                t("edge_point", np.int32), t("edge_obs", np.float32), br.K)
        slim = fm.global_bundle_adjust_device(*args, schedule=schedule, max_free_cams=n_free, diagnostics=False)
        trials = torch.zeros((1, _lib.BA_SLOTS), dtype=torch.int32, device="cuda")
        fm.global_bundle_adjust_device(*args, schedule=schedule, max_free_cams=n_free, out=dict(slim, it_trials=trials))
        trials = trials.cpu().numpy()[0]
        ms = []
        for i in range(a.warmup + a.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fm.global_bundle_adjust_device(*args, schedule=schedule, max_free_cams=n_free, out=slim)
            if i >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        host_ms = []
        for _ in range(a.host_calls):
            t0 = time.perf_counter()
            want = ba_host.run(host, s, schedule, max_free=n_free, diagnostics=False)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        host_ms = float(np.median(host_ms))
        status = int(slim["status"].cpu()[0])
        launches, waits = counts(n_free, tile, status, int((trials != 0).sum()), int(trials.sum()), bool((trials[32:] != 0).any()))
        row = {"free_fixed_points_edges": [n_free, nc - n_free, npt, ne], "status": status,
               "flagged_device_host": [int(slim["outliers"].sum()), int(want["outliers"].sum())],
               "iterations": int((trials != 0).sum()), "trials": int(trials.sum()), "launches": launches, "host_waits": waits,
               "device_ms": {"wall_median": round(float(np.median(ms)), 4),
                             "wall_p10_p90": [round(float(x), 4) for x in np.percentile(ms, [10, 90])]},
               "host_build_one_thread_ms": round(host_ms, 3)}
        if n_free <= 64:
            desc = torch.tensor([(nc, npt, ne, 0, 0, 0)], dtype=torch.int32, device="cuda")
            one = fm.bundle_adjust_device(desc, *args, schedule=schedule, max_free_cams=n_free, diagnostics=False)
            ev = []
            for i in range(a.warmup + a.calls):                # the same clock as above: the host's, around call and wait
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fm.bundle_adjust_device(desc, *args, schedule=schedule, max_free_cams=n_free, out=one)
                torch.cuda.synchronize()
                if i >= a.warmup:
                    ev.append((time.perf_counter() - t0) * 1e3)
            row["msf_bundle_adjust_device_ms"] = {"wall_median": round(float(np.median(ev)), 4)}
            row["same_bytes_as_msf_bundle_adjust"] = all(one[k].cpu().numpy().tobytes() == slim[k].cpu().numpy().tobytes() for k in one)
        result[name] = row
    result["note"] = ("device: one blocking call on device-resident arrays, host-driven Levenberg-Marquardt, no diagnostics, "
                      "host clock around the call; host: the same arithmetic (csrc/ba_solve.h, g++ -O2) on one thread "
                      "including the ctypes call, not the reference's g2o, which was not measured")
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
