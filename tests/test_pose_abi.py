"""CPU: include/msf_pose.h -- plain C, every symbol it declares is exported by libmsf.so and listed in
_lib.POSE_SYMBOLS, none of them belongs to the four earlier headers (whose lists and versions stay what they are), and
the two structs have the layout the ctypes view relies on."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
EARLIER = ("msf_abi.h", "msf_initializer.h", "msf_local_mapping.h", "msf_pnp.h")


def _declared(header):
    hdr = open(os.path.join(INCLUDE, header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(msf_[a-z_0-9]+)\s*\(", hdr)))


def test_header_symbols_are_exported_and_new():
    from mono_slam_framework_amd import _lib
    L = _lib.load()
    names = _declared("msf_pose.h")
    assert names == sorted(_lib.POSE_SYMBOLS) and len(names) == 3
    earlier = _lib.ABI_SYMBOLS + _lib.INITIALIZER_SYMBOLS + _lib.LOCAL_MAPPING_SYMBOLS + _lib.PNP_SYMBOLS
    for n in names:
        assert hasattr(L, n), n
        assert n not in earlier
        for h in EARLIER:
            assert n not in _declared(h)
    assert L.msf_pose_version() == 1
    assert L.msf_abi_version() == 4 and L.msf_initializer_version() == 1 and L.msf_local_mapping_version() == 1
    assert L.msf_pnp_version() == 1
    assert len(_lib.ABI_SYMBOLS) == 45 and len(_lib.INITIALIZER_SYMBOLS) == 3 and len(_lib.LOCAL_MAPPING_SYMBOLS) == 4
    assert len(_lib.PNP_SYMBOLS) == 3 and _declared("msf_pnp.h") == sorted(_lib.PNP_SYMBOLS)


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "msf_pose.h"\n'
                   "int main(void){ msf_pose_params p; msf_pose_result r; p.struct_size = sizeof p; "
                   "r.struct_size = sizeof r; return (int)(p.struct_size + r.struct_size) + MSF_POSE_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_struct_layouts_match_ctypes(tmp_path):
    from mono_slam_framework_amd import _lib
    fields = [name for name, _, _, _ in _lib.POSE_ARRAYS]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msf_pose.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu", sizeof(msf_pose_params), sizeof(msf_pose_result), '
                   "offsetof(msf_pose_params, fx), offsetof(msf_pose_params, chi2));\n"
                   + "".join('printf(" %%zu", offsetof(msf_pose_result, %s));\n' % f for f in fields)
                   + "return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, str(src), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    P, R = _lib.PoseParams, _lib.PoseResult
    assert sizes == [C.sizeof(P), C.sizeof(R), P.fx.offset, P.chi2.offset] + [getattr(R, f).offset for f in fields]
    assert C.sizeof(P) == 28 and C.sizeof(R) == 8 + 8 * len(fields) and len(fields) == 17


def test_shapes():
    from mono_slam_framework_amd import _lib
    s = _lib.pose_shapes(3, 50)
    assert s["n_good"] == ((3,), "int32") and s["outliers"] == ((3, 50), "uint8") and s["Tcw"] == ((3, 12), "float32")
    assert s["round_pose_f64"] == ((3, 4, 12), "float64") and s["it_H"] == ((3, 4, 10, 21), "float64")
    assert s["it_pose_out"] == ((3, 4, 10, 7), "float64") and s["it_trials"] == ((3, 4, 10), "int32")


def test_the_kernel_file_is_built_and_its_header_is_a_dependency():
    from mono_slam_framework_amd import build
    assert "pose_kernels.hip" in build.HIP_SOURCES
    assert os.path.join(INCLUDE, "msf_pose.h") in build._deps()


def test_the_mirror_compiles_with_plain_gxx():
    """csrc/hip_optimizer.h and its test program: syntax only, no GPU (the behaviour is in test_pose_mirror_gpu.py)"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE,
                           "-I", os.path.join(ROOT, "mono_slam_framework_amd", "csrc"), "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pose_mirror.cpp")])
