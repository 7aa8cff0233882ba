"""CPU: tests/cpp/gba_edge_main.cpp, a program of its own under AddressSanitizer and UBSan -- gba::layout for 0 / 1 / 65 /
1024 free cameras (pieces aligned, disjoint, sized by the counts) and the tile schedule of the Cholesky for every n in
0 .. 4 T + 7 (every entry of the lower triangle and of the extra row exactly once per step, nothing outside)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")


def test_layout_and_tile_schedule_under_sanitizers(tmp_path):
    exe = str(tmp_path / "gba_edge")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "gba_edge_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "gba edge checks passed" in r.stdout, r.stdout
