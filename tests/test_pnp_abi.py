"""CPU: include/msf_pnp.h -- plain C, every symbol it declares is exported by libmsf.so and listed in _lib.PNP_SYMBOLS,
none of them belongs to the three earlier headers (whose lists and versions stay what they are), and the two structs
have the layout the ctypes view relies on."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
EARLIER = ("msf_abi.h", "msf_initializer.h", "msf_local_mapping.h")


def _declared(header):
    hdr = open(os.path.join(INCLUDE, header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(msf_[a-z_0-9]+)\s*\(", hdr)))


def test_header_symbols_are_exported_and_new():
    from mono_slam_framework_amd import _lib
    L = _lib.load()
    names = _declared("msf_pnp.h")
    assert names == sorted(_lib.PNP_SYMBOLS) and len(names) == 3
    for n in names:
        assert hasattr(L, n), n
        assert n not in _lib.ABI_SYMBOLS + _lib.INITIALIZER_SYMBOLS + _lib.LOCAL_MAPPING_SYMBOLS
        for h in EARLIER:
            assert n not in _declared(h)
    assert L.msf_pnp_version() == 1
    assert L.msf_abi_version() == 4 and L.msf_initializer_version() == 1 and L.msf_local_mapping_version() == 1
    assert len(_lib.ABI_SYMBOLS) == 45 and len(_lib.INITIALIZER_SYMBOLS) == 3 and len(_lib.LOCAL_MAPPING_SYMBOLS) == 4


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "msf_pnp.h"\n'
                   "int main(void){ msf_pnp_params p; msf_pnp_result r; p.struct_size = sizeof p; "
                   "r.struct_size = sizeof r; return (int)(p.struct_size + r.struct_size) + MSF_PNP_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_struct_layouts_match_ctypes(tmp_path):
    from mono_slam_framework_amd import _lib
    fields = [name for name, _, _, _ in _lib.PNP_ARRAYS]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msf_pnp.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu", sizeof(msf_pnp_params), sizeof(msf_pnp_result), '
                   "offsetof(msf_pnp_params, th2), offsetof(msf_pnp_params, max_records), offsetof(msf_pnp_params, seed));\n"
                   + "".join('printf(" %%zu", offsetof(msf_pnp_result, %s));\n' % f for f in fields)
                   + "return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, str(src), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    P, R = _lib.PnpParams, _lib.PnpResult
    assert sizes == [C.sizeof(P), C.sizeof(R), P.th2.offset, P.max_records.offset, P.seed.offset] + \
        [getattr(R, f).offset for f in fields]
    assert C.sizeof(P) == 48 and C.sizeof(R) == 8 + 8 * len(fields)


def test_the_kernel_file_is_built_and_its_header_is_a_dependency():
    from mono_slam_framework_amd import build
    assert "pnp_kernels.hip" in build.HIP_SOURCES
    assert os.path.join(INCLUDE, "msf_pnp.h") in build._deps()


def test_the_mirror_compiles_with_plain_gxx():
    """csrc/hip_pnp_solver.h and its test program: syntax only, no GPU (the behaviour is in test_pnp_mirror_gpu.py)"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE,
                           "-I", os.path.join(ROOT, "mono_slam_framework_amd", "csrc"), "-isystem", os.path.join(rocm, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_pnp_mirror.cpp")])
