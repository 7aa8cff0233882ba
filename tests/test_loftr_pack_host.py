"""CPU: csrc/loftr_pack.h -- the host arithmetic that turns the LoFTR weights into the operand layouts of the MFMA
kernels -- in a stand-alone sanitized executable (tests/cpp/loftr_pack_main.cpp), never inside python.  It packs the
shipped weights into every buffer LoftrPipeline::init uploads and prints a digest of each; tests/golden/
loftr_pack_digests.txt holds the digests of the same 126 buffers as the packing loops inside init produced them before
the header existed, so a layout that moves by one element fails here, with no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
WEIGHTS = os.path.join(ROOT, "mono_slam_framework_amd", "weights", "loftr_teacher.bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "loftr_pack_digests.txt")


def test_packed_buffers_in_a_sanitized_executable(tmp_path):
    """21 d_w, 5 d_w2, 20 d_wx, 48 encoder matrices, 32 split twins: bytes and FNV-1a 64 as recorded; split() on every
    weight and on 0, -0, the smallest normal, an all-ones mantissa and ties; non-zero counts of every fragment buffer;
    the format each of the 21 convolutions selects"""
    exe = str(tmp_path / "loftr_pack")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "loftr_pack_main.cpp"),
                           os.path.join(CSRC, "weights_io.cpp"), "-o", exe])
    r = subprocess.run([exe, WEIGHTS], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    print(r.stderr)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(want) == 21 + 5 + 20 + 48 + 32
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
