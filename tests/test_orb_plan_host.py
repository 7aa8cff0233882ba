"""CPU: csrc/orb_plan.h -- the host arithmetic behind OrbPipeline::init: level sizes, quotas, list capacities, the tile
and strip grids, the resize tables and the checks that decide which kernels a handle launches -- in a stand-alone
executable (tests/cpp/orb_plan_main.cpp), never inside python.  tests/golden/orb_plan_digests.txt holds the plans of a
fixed request list as the code inside init produced them before the header existed; the sweep goes over every supported
width and height, where no GPU test can go; the cross-checks hold the plan to oracle/orb.py and tests/orb_capacity.py."""
import os
import re
import subprocess

import pytest

from oracle import orb as oracle_orb
from tests import orb_capacity as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "cpp", "orb_plan_main.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "orb_plan_digests.txt")
SANITIZED = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + flags + ["-I", CSRC, MAIN, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "orb_plan", SANITIZED)


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def _plans(lines):
    """the printed lines as one dict per request: line name -> {key: value string}"""
    plans = []
    for ln in lines:
        name, _, rest = ln.partition(" ")
        if name == "req":
            plans.append({})
        plans[-1][name] = rest if name == "error" else dict(kv.split("=") for kv in rest.split())
    return plans


def _ints(s):
    return [int(v) for v in s.split(",")]


def test_header_needs_no_hip():
    """the header alone, with nothing but the compiler's own include path"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", CSRC, "-x", "c++", "-"],
                   input='#include "orb_plan.h"\n', text=True, check=True)


@pytest.mark.parametrize("size,levels", [((192, 144), 5), ((333, 257), 8), ((76, 64), 1), ((100, 92), 3)])
def test_tail_list_check_in_a_sanitized_executable(sanitized, size, levels):
    """check_tail_lists, the host check in front of msf_debug_orb_tail, at the sizes tests/test_orb_tail_gpu.py uses: the
    rectangle's corners pass, one step outside is refused on every level, lists are read to their end and no further"""
    out = _run([sanitized, "tail_lists", str(size[0]), str(size[1])])
    assert out == ["tail_lists %d x %d: levels_with_rectangle=%d failures=0" % (size[0], size[1], levels)]


def test_golden_plans_in_a_sanitized_executable(sanitized):
    """every scalar of OrbGeometry, every member of each OrbLevelInfo, the primary lists, resize_shared, umax, the
    Harris units, length and FNV-1a 64 of the tables and of the disc: as recorded from the code init held before"""
    got = _run([sanitized, "golden"])
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    plans = _plans(want)
    errors = [p["error"] for p in plans if "error" in p]
    assert errors == ["ORB candidate arrays exceed 2^32 entries: reduce max_batch_pairs",
                      "arg: ORB image size must be in [64, 8192] x [64, 8192]",
                      "arg: ORB image size must be in [64, 8192] x [64, 8192]", "arg: ORB max_slots < 2"]
    # the anchors of the recorded file itself
    p = next(p for p in plans if p["req"]["w"] == "1280" and p["req"]["max_slots"] == "2048")
    assert (p["tab"]["len"], p["geom"]["total_strips"], p["geom"]["total_tiles"]) == ("19668", "69", "626")
    p = next(p for p in plans if p["req"]["w"] == "8192" and p["req"]["h"] == "8192")
    assert [p["lv%d" % l]["wk_fused"] for l in range(1, 8)] == ["0", "0", "0", "0", "1", "1", "1"]
    assert {p["geom"]["pool_entries"] for p in plans if "geom" in p and p["req"]["stream_min"] == "1"} == {"16"}


def test_supported_range_sweep(tmp_path_factory):
    """every width 64..8192 at height 64 and every height 64..8192 at width 64, both level-size modes, max_slots 2 and
    256: resize_shared on all levels, wk_fused on all levels exactly up to width 4160, and the invariants the kernels
    rely on re-derived from the tables (taps inside the strip's window, xstrip, yemit, table and list offsets)"""
    exe = _build(tmp_path_factory, "orb_plan_sweep", ["-O2"])   # the sanitized build takes minutes over 65 032 plans
    parts = 8
    procs = [subprocess.Popen([exe, "sweep", str(k), str(parts)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k in range(parts)]
    plans = unfused = 0
    first = []
    for p in procs:
        out, err = p.communicate()
        assert p.returncode == 0, err
        m = re.match(r"plans=(\d+) unfused=(\d+) first_unfused=(\d+) failures=0$", out.strip())
        plans += int(m.group(1))
        unfused += int(m.group(2))
        first.append(int(m.group(3)))
    assert plans == 2 * 8129 * 2 * 2
    assert unfused == 4032 and min(first) == 4161


# image sizes: those of the recorded plans, those of tests/test_orb_capacity.py (SIZES and the level sizes its literal
# numbers are for, as far as they are image sizes: 100 x 60 is below the smallest)
CROSS_SIZES = [(640, 480), (1280, 720), (1920, 1080), (64, 64), (69, 64), (333, 251), (4096, 2160), (8192, 8192), (8192, 64),
               (64, 8192), (1067, 600), (357, 201), (889, 500), (444, 333), (429, 241)]


def test_plan_agrees_with_the_oracle_and_the_capacity_helper(sanitized):
    reqs = [(w, h, 2, m) for (w, h) in CROSS_SIZES for m in (0, 1)]
    plans = _plans(_run([sanitized, "plans"] + [str(v) for r in reqs for v in r]))
    assert len(plans) == len(reqs)
    assert oc.KP_CAP == int(re.search(r"constexpr int kKpCap = (\d+);", open(os.path.join(CSRC, "orb_plan.h")).read()).group(1))
    for (w, h, _, m), p in zip(reqs, plans):
        o = oracle_orb.OrbOracle(w, h, level_size_mul_inv=m)
        assert _ints(p["flags"]["umax"]) == o.umax(), (w, h, m)
        caps = _ints(p["prim"]["cap"])
        for l in range(8):
            lv = p["lv%d" % l]
            lw, lh = int(lv["w"]), int(lv["h"])
            assert (lw, lh) == o.level_size(l), (w, h, m, l)
            assert int(lv["quota"]) == o.level_quota(l), (w, h, m, l)
            assert float.fromhex(lv["scale"]) == o.level_scale(l), (w, h, m, l)
            assert int(lv["cand_cap"]) == oc.full_list(lw, lh), (w, h, m, l)
            assert caps[l] == oc.primary_list(lw, lh), (w, h, m, l)
            assert min(oc.S1_CAP, int(lv["cand_cap"])) == oc.stage1_cap(lw, lh), (w, h, m, l)
            assert int(lv["s1_off"]) == l * oc.S1_CAP, (w, h, m, l)
