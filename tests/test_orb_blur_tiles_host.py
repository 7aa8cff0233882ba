"""CPU: csrc/orb_blur_tiles.h -- the LDS image of k_describe's patch and its row blur as nine 16 x 16 x 64 integer matrix
products -- in a stand-alone executable (tests/cpp/orb_blur_tiles_main.cpp) built with the address and undefined-behaviour
sanitizers and run directly, never inside python.  The executable runs the header's integer model of the tiling (operand
and result lane maps, the u16 packing, every LDS index) on arrays of exactly the kernel's sizes: constant, 0 | 255 by
column and by row, and random patches, for both tap sets, every hb[c][r] against the direct 7-tap sum; nothing outside
the two arrays is indexed and no row >= 46 or column >= 40 is stored.  The kernel takes its constants, offsets and B
operand from the same header; tests/test_orb_describe_gpu.py holds what the hardware then computes to the reference."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "cpp", "orb_blur_tiles_main.cpp")
SANITIZED = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("orb_blur_tiles") / "orb_blur_tiles")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + SANITIZED + ["-I", CSRC, MAIN, "-o", exe])
    return exe


def test_header_needs_no_hip():
    """the header alone, with nothing but the compiler's own include path"""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", CSRC, "-x", "c++", "-"],
                   input='#include "orb_blur_tiles.h"\n', text=True, check=True)


def test_tiling_model_in_a_sanitized_executable(sanitized):
    r = subprocess.run([sanitized], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["orb_blur_tiles: patches=60 failures=0"]


def test_kernel_takes_its_layout_from_the_header():
    """the constants the model is run with are the ones the kernel is compiled with"""
    src = open(os.path.join(CSRC, "orb_kernels.hip")).read()
    for name in ("blur_tiles::kRawBytes", "blur_tiles::kHbEntries", "blur_tiles::kHbPitch", "blur_tiles::b_dword(SUM256, nt, lane, d)",
                 "blur_tiles::a_byte_offset(0, lane)", "blur_tiles::hb_store_byte_offset(0, 0, lane)",
                 "blur_tiles::samp_byte_offset(0, 0)", "blur_tiles::acc_init(SUM256)", "blur_tiles::fetch_lane(lane)"):
        assert name in src, name
