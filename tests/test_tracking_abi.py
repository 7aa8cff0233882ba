"""CPU: include/msf_tracking.h -- plain C99, the names it declares are the names libmsf.so exports for it and the names
in _lib.TRACKING_SYMBOLS, none of them belongs to an earlier header (whose lists keep their lengths and whose versions
stay what they are), and the ctypes structs have the C sizes."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
EARLIER = {"ABI_SYMBOLS": 45, "INITIALIZER_SYMBOLS": 3, "LOCAL_MAPPING_SYMBOLS": 4, "PNP_SYMBOLS": 3, "POSE_SYMBOLS": 3,
           "BA_SYMBOLS": 3, "GLOBAL_BA_SYMBOLS": 4}


def _declared(header):
    hdr = open(os.path.join(INCLUDE, header)).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(msf_[a-z_0-9]+)\s*\(", hdr)))


def test_declared_exported_and_listed_names_agree():
    from mono_slam_framework_amd import _lib, build
    L = _lib.load()
    names = _declared("msf_tracking.h")
    assert names == sorted(_lib.TRACKING_SYMBOLS) and len(names) == 5
    nm = subprocess.check_output(["nm", "-D", "--defined-only", build.lib_path()], text=True)
    exported = set(re.findall(r" T (msf_\w+)", nm))
    earlier = set()
    for name, length in EARLIER.items():
        assert len(getattr(_lib, name)) == length, name
        earlier |= set(getattr(_lib, name))
    assert set(names) <= exported and not set(names) & earlier
    assert exported - earlier == set(names)           # nothing exported for this header that it does not declare
    for n in names:
        assert hasattr(L, n), n
    assert L.msf_tracking_version() == 1
    assert (L.msf_abi_version(), L.msf_initializer_version(), L.msf_local_mapping_version(), L.msf_pnp_version(),
            L.msf_pose_version(), L.msf_ba_version(), L.msf_global_ba_version()) == (4, 1, 1, 1, 1, 1, 1)


def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "msf_tracking.h"\n'
                   "typedef char point_is_32[sizeof(msf_map_point) == 32 ? 1 : -1];\n"
                   "typedef char claim_is_16[sizeof(msf_local_claim) == 16 ? 1 : -1];\n"
                   "int main(void){ msf_local_map m; msf_frustum_params p; msf_frustum_result r; msf_claim_result c; "
                   "msf_device_corr k; m.struct_size = sizeof m; p.struct_size = sizeof p; r.struct_size = sizeof r; "
                   "c.struct_size = sizeof c; k.struct_size = sizeof k; return (int)(m.struct_size + p.struct_size + "
                   "r.struct_size + c.struct_size + k.struct_size) + MSF_TRACKING_VERSION + (int)MSF_POINT_SEEN; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_struct_layouts_match_ctypes(tmp_path):
    from mono_slam_framework_amd import _lib
    assert _lib.MAP_POINT_DTYPE.itemsize == 32 and _lib.LOCAL_CLAIM_DTYPE.itemsize == 16
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msf_tracking.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(msf_map_point), sizeof(msf_local_claim), '
                   "sizeof(msf_local_map), sizeof(msf_frustum_params), sizeof(msf_frustum_result), sizeof(msf_claim_result), "
                   "sizeof(msf_device_corr), offsetof(msf_frustum_params, Ow), offsetof(msf_local_map, points)); return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", INCLUDE, str(src), "-o", exe])
    sizes = [int(x) for x in subprocess.check_output([exe]).split()]
    assert sizes == [32, 16, C.sizeof(_lib.LocalMap), C.sizeof(_lib.FrustumParams), C.sizeof(_lib.FrustumResult),
                     C.sizeof(_lib.ClaimResult), C.sizeof(_lib.DeviceCorr), _lib.FrustumParams.Ow.offset,
                     _lib.LocalMap.points.offset]
    assert [a[0] for a in _lib.FRUSTUM_ARRAYS] == [f[0] for f in _lib.FrustumResult._fields_[2:]]
    assert [a[0] for a in _lib.CLAIM_ARRAYS] == [f[0] for f in _lib.ClaimResult._fields_[2:]]
