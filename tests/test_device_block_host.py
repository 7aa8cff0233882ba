"""CPU: csrc/hip_device_block.h -- how the C++ mirrors stage the batch of a `_device` call -- in a stand-alone sanitized
executable (tests/cpp/device_block_main.cpp), never inside python, against a host stand-in for the HIP runtime API
(tests/cpp/hip_host) whose device memory is malloc memory of exactly the size asked for: a piece that the measuring
pass did not count, or a copy that runs past a block, is an overrun that AddressSanitizer reports here, where on the
device it would be a write past the allocation; a block that a failure path forgets is a leak."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")


def test_device_block_in_a_sanitized_executable(tmp_path):
    """pieces of 0 / 1 / 255 / 256 / 257 bytes, double, int32 and a 16-byte struct: the same member at the same offset on
    both sides, on the 256-byte grid, the total what msf::Carver measures; upload moves the inputs and nothing else,
    download the rest and nothing else; hipMalloc, hipMemset and either copy failing in turn return false and leave no
    block behind; placing twice frees the first block"""
    exe = str(tmp_path / "device_block")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hip_host"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "device_block_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
