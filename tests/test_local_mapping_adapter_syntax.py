"""CPU: csrc/hip_local_mapping.h -- msf::NewMapPoints, the header-only C++ mirror of LocalMapping::CreateNewMapPoints
above msf_create_map_points -- compiles as C++14 with no OpenCV type, alone and next to hip_initializer.h: the include
path holds only the project's headers, the OpenCV stand-ins of tests/cpp/stubs (which it must not need) and the HIP
runtime API (for hip_initializer.h; hip_local_mapping.h itself needs none)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")


@pytest.mark.skipif(not os.path.exists(os.path.join(ROCM_INCLUDE, "hip", "hip_runtime_api.h")),
                    reason="needs the HIP runtime API header")
def test_local_mapping_adapter_compiles_next_to_the_initializer():
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror",
           "-I", os.path.join(ROOT, "tests", "cpp", "stubs"), "-I", os.path.join(ROOT, "include"),
           "-I", CSRC, "-isystem", ROCM_INCLUDE,
           os.path.join(ROOT, "tests", "cpp", "test_local_mapping_adapter_syntax.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_local_mapping_adapter_needs_neither_opencv_nor_hip(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "hip_local_mapping.h"\n'
                   "bool f(msf_handle* h, const msf_view& v, const std::vector<msf::Neighbour>& n, std::vector<msf::NewMapPoint>& o)"
                   " { return msf::NewMapPoints(h, 0, v, n, 1.1, o); }\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-I", CSRC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = open(os.path.join(CSRC, "hip_local_mapping.h")).read()
    assert "#include <opencv" not in text and "cv::Mat " not in text and "#include <hip" not in text
