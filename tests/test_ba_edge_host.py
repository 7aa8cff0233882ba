"""CPU: csrc/ba_solve.h on problems at the edge of its domain, in a stand-alone sanitized executable
(tests/cpp/ba_edge_main.cpp), never inside python: 0 edges, 0 free cameras, a point with one edge, a camera with none,
no fixed camera, every edge flagged after round 0, points at Z <= 0, NaN input, 64 and 65 free cameras, a stop word set
from the start, an edge index out of range, edge_point decreasing.  The scratch is exactly what ba::layout() asks for."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")


def test_edge_problems_in_a_sanitized_executable(tmp_path):
    exe = str(tmp_path / "ba_edge")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "ba_edge_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("\n") >= 14 and "BAD" not in r.stdout
