"""CPU: csrc/carve.h -- the carver behind every geometry workspace of abi_*.cpp -- in a stand-alone sanitized
executable (tests/cpp/carve_main.cpp), never inside python.  The measuring pass sizes a malloc block of exactly the bytes
it reports and the placing pass writes every piece of it in full: a piece that the first pass did not count is an
overrun that AddressSanitizer reports here, where on the device it would be a write past the workspace."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")


def test_carver_in_a_sanitized_executable(tmp_path):
    """sizes 0 / 1 / 255 / 256 / 257, a given pointer, a false condition, double and a 16-byte struct: both passes end at
    the same offset, pieces start on the 256-byte grid, in order and disjoint; what takes no room takes none"""
    exe = str(tmp_path / "carve")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "carve_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
