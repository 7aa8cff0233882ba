"""CPU: csrc/orb_plan.h, walk_unit / walk_grid -- which unit a workgroup of the walker launch (k_walk) is.  The kernel's
bounded waits rest on one property of that order: whatever a unit waits for has a LOWER workgroup index.  A stand-alone
executable (tests/cpp/walk_units_main.cpp, built with the address and undefined-behaviour sanitizers, never inside
python) decodes every workgroup of every launch form the pipeline uses -- one launch over all levels without finish
units and with them in either placement, and one launch per level -- and checks that the grid maps onto every unit
exactly once, that every dependency (threshold <- strips of the level above, strip <- threshold, non-quarter <- quarter,
finish <- all strips of its level) points downwards, and that surplus indices decode to "none"."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "cpp", "walk_units_main.cpp")
SANITIZED = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

FRAMES = [9, 16, 18, 294, 2048]
SIZES = [(1280, 720), (640, 480), (333, 251), (72, 100)]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk_units") / "walk_units")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + SANITIZED + ["-I", CSRC, MAIN, "-o", exe])
    return exe


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("n", FRAMES)
def test_every_unit_once_and_every_dependency_at_a_lower_index(sanitized, size, n):
    # max_slots as a handle for n / 2 pairs has them (4 slots per pair): short strips below 256 slots, tall ones above
    r = subprocess.run([sanitized, str(size[0]), str(size[1]), str(2 * n), str(n)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr
    m = re.match(r"walk_units %d x %d n=%d: strips=(\d+) workgroups=(\d+) none=(\d+) failures=0$" % (size[0], size[1], n),
                 r.stdout.strip())
    assert m, r.stdout
    strips, workgroups, none = (int(v) for v in m.groups())
    # four forms of the whole pyramid (three launches over all levels, and the eight per-level launches together):
    # 8 threshold units + the strips each, 8 finish units more in two of them
    frames_padded = 8 * ((n + 7) // 8)
    assert workgroups == frames_padded * (4 * (8 + strips) + 2 * 8)
    assert none == (frames_padded - n) * (4 * (8 + strips) + 2 * 8)
    assert (none == 0) == (n % 8 == 0)
