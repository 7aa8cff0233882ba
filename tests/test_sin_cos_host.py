"""CPU: pose::sin_cos (csrc/pose_solve.h), the sin / cos of the bundle adjustments' pose update in plain multiplies
and adds, against the host's libm -- tests/cpp/sin_cos_main.cpp, a program of its own under ASan and UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")


def test_sin_cos_stays_within_one_ulp_of_libm(tmp_path):
    exe = str(tmp_path / "sin_cos")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "sin_cos_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "sin_cos checks passed" in r.stdout, r.stdout
