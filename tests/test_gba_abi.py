"""CPU: include/msf_global_ba.h -- plain C, every symbol it declares is exported by libmsf.so and listed in
_lib.GLOBAL_BA_SYMBOLS, none of them belongs to the six earlier headers (whose lists and versions stay what they are),
the tile edge the library reports is the constant of gba_solve.h, and a null handle is refused without a GPU."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
EARLIER = ("msf_abi.h", "msf_initializer.h", "msf_local_mapping.h", "msf_pnp.h", "msf_pose.h", "msf_ba.h")


def _declared(header):
    hdr = open(os.path.join(INCLUDE, header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(msf_[a-z_0-9]+)\s*\(", hdr)))


def test_header_symbols_are_exported_and_new():
    from mono_slam_framework_amd import _lib
    L = _lib.load()
    names = _declared("msf_global_ba.h")
    assert names == sorted(_lib.GLOBAL_BA_SYMBOLS) and len(names) == 4
    earlier = (_lib.ABI_SYMBOLS + _lib.INITIALIZER_SYMBOLS + _lib.LOCAL_MAPPING_SYMBOLS + _lib.PNP_SYMBOLS
               + _lib.POSE_SYMBOLS + _lib.BA_SYMBOLS)
    for n in names:
        assert hasattr(L, n), n
        assert n not in earlier
        for h in EARLIER:
            assert n not in _declared(h)
    assert L.msf_global_ba_version() == 1
    # the six earlier versions and symbol counts are unchanged
    assert L.msf_abi_version() == 4 and L.msf_initializer_version() == 1 and L.msf_local_mapping_version() == 1
    assert L.msf_pnp_version() == 1 and L.msf_pose_version() == 1 and L.msf_ba_version() == 1
    assert len(_lib.ABI_SYMBOLS) == 45 and len(_lib.INITIALIZER_SYMBOLS) == 3 and len(_lib.LOCAL_MAPPING_SYMBOLS) == 4
    assert len(_lib.PNP_SYMBOLS) == 3 and len(_lib.POSE_SYMBOLS) == 3 and len(_lib.BA_SYMBOLS) == 3
    assert _declared("msf_ba.h") == sorted(_lib.BA_SYMBOLS)


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "msf_global_ba.h"\n'
                   "int main(void){ msf_ba_params p; msf_ba_result r; p.struct_size = sizeof p; r.struct_size = sizeof r; "
                   "return (int)(p.struct_size + r.struct_size) + MSF_GLOBAL_BA_VERSION + MSF_GBA_MAX_FREE_CAMS + MSF_BA_SLOTS; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_tile_rows_is_the_constant_of_gba_solve_h():
    from mono_slam_framework_amd import _lib
    L = _lib.load()
    src = open(os.path.join(CSRC, "gba_solve.h")).read()
    tile = int(re.search(r"constexpr int kTile = (\d+);", src).group(1))
    cap = int(re.search(r"constexpr int kMaxFreeCams = (\d+);", src).group(1))
    assert L.msf_global_ba_tile_rows() == tile and tile > 0
    hdr = open(os.path.join(INCLUDE, "msf_global_ba.h")).read()
    assert int(re.search(r"#define MSF_GBA_MAX_FREE_CAMS (\d+)", hdr).group(1)) == cap == _lib.GBA_MAX_FREE_CAMS == 1024


def test_the_kernel_file_is_built_and_its_headers_are_dependencies():
    from mono_slam_framework_amd import build
    assert "gba_kernels.hip" in build.HIP_SOURCES
    deps = build._deps()
    assert os.path.join(INCLUDE, "msf_global_ba.h") in deps
    for f in ("gba_solve.h", "gba_pipeline.h", "gba_kernels.hip"):
        assert os.path.join(CSRC, f) in deps
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "_lib.GLOBAL_BA_SYMBOLS" in entry


def test_a_null_handle_is_refused():
    from mono_slam_framework_amd import _lib
    L = _lib.load()
    prm, res = _lib.BaParams(), _lib.BaResult()
    assert L.msf_global_bundle_adjust(None, 0, None, None, 0, None, 0, None, None, None, None, C.byref(prm),
                                      C.byref(res)) == _lib.MSF_ERR_INVALID_ARG
    assert L.msf_global_bundle_adjust_device(None, 0, None, None, 0, None, 0, None, None, None, 1, None, C.byref(prm),
                                             C.byref(res), None) == _lib.MSF_ERR_INVALID_ARG


def test_the_mirror_compiles_with_plain_gxx():
    """csrc/hip_bundle_adjustment.h with GlobalBundleAdjustment and both test programs: syntax only, no GPU"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for prog in ("test_ba_mirror.cpp", "test_gba_mirror.cpp"):
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, "-I", CSRC,
                               "-isystem", os.path.join(rocm, "include"), os.path.join(ROOT, "tests", "cpp", prog)])
