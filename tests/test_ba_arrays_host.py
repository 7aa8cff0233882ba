"""CPU: csrc/ba_arrays.h -- the table behind the carve and the copy-back of msf_ba_result -- in a stand-alone sanitized
executable (tests/cpp/ba_arrays_main.cpp), never inside python, and the same table against its Python side
(_lib.BA_ARRAYS, ba_shapes and the ctypes struct)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mono_slam_framework_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
UNITS = ["problem", "cam", "point", "edge", "round", "it", "it_cam", "it_point"]   # the C++ unit counts, in their order


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ba_arrays") / "ba_arrays")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "ba_arrays_main.cpp"), "-o", path])
    return path


def test_carve_and_copy_back_in_a_sanitized_executable(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout


def test_the_table_agrees_with_the_python_side(exe):
    rows = [line.split() for line in subprocess.check_output([exe, "--print"], text=True).splitlines()]
    assert [r[1] for r in rows] == [a[0] for a in _lib.BA_ARRAYS] == [f[0] for f in _lib.BaResult._fields_[2:]]
    nc, npt, ne = 7, 11, 23
    shapes = _lib.ba_shapes(1, nc, npt, ne)
    count = {"problem": 1, "cam": nc, "point": npt, "edge": ne, "round": 2, "it": 64, "it_cam": 64 * nc, "it_point": 64 * npt}
    for (_, name, offset, elem, unit, tail, per_cap, required), (_, dt, per, shape_tail) in zip(rows, _lib.BA_ARRAYS):
        assert int(offset) == getattr(_lib.BaResult, name).offset, name
        assert int(elem) == np.dtype(dt).itemsize and UNITS[int(unit)] == per and int(per_cap) == 0, name
        assert int(tail) == int(np.prod(shape_tail, dtype=np.int64)), name
        shape, sdt = shapes[name]
        assert sdt == dt and count[per] * int(tail) == int(np.prod(shape)), name
        assert bool(int(required)) == (name == "status"), name
    assert C.sizeof(_lib.BaResult) == 8 + 8 * len(rows)
