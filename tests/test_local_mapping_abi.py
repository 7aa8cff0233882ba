"""CPU: include/msf_local_mapping.h -- plain C, every symbol it declares is exported by libmsf.so and listed in
_lib.LOCAL_MAPPING_SYMBOLS, none of them belongs to msf_abi.h or msf_initializer.h (whose lists and versions stay what
they are), and the two record types have the sizes the device code relies on."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def _declared(header):
    hdr = open(os.path.join(INCLUDE, header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(msf_[a-z_0-9]+)\s*\(", hdr)))


def test_header_symbols_are_exported_and_new():
    from mono_slam_framework_amd import _lib
    L = _lib.load()
    names = _declared("msf_local_mapping.h")
    assert names == sorted(_lib.LOCAL_MAPPING_SYMBOLS) and len(names) == 4
    for n in names:
        assert hasattr(L, n), n
        assert n not in _lib.ABI_SYMBOLS and n not in _lib.INITIALIZER_SYMBOLS
        assert n not in _declared("msf_abi.h") and n not in _declared("msf_initializer.h")
    assert L.msf_local_mapping_version() == 1
    assert L.msf_abi_version() == 4 and L.msf_initializer_version() == 1


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "msf_local_mapping.h"\n'
                   "typedef char view_is_64[sizeof(msf_view) == 64 ? 1 : -1];\n"
                   "typedef char point_is_16[sizeof(msf_new_point) == 16 ? 1 : -1];\n"
                   "int main(void){ msf_new_points_params p; msf_new_points_result r; p.struct_size = sizeof p; "
                   "r.struct_size = sizeof r; return (int)(p.struct_size + r.struct_size) + MSF_LOCAL_MAPPING_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_struct_layouts_match_ctypes(tmp_path):
    from mono_slam_framework_amd import _lib
    assert C.sizeof(_lib.View) == 64 and _lib.VIEW_DTYPE.itemsize == 64
    assert _lib.NEW_POINT_DTYPE.itemsize == 16
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "msf_local_mapping.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu\\n", sizeof(msf_view), sizeof(msf_new_point), '
                   "sizeof(msf_new_points_params), sizeof(msf_new_points_result)); return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, str(src), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [64, 16, C.sizeof(_lib.NewPointsParams), C.sizeof(_lib.NewPointsResult)]
