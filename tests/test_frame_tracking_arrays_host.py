"""CPU: csrc/frame_tracking_arrays.h -- the table behind the carve and the copy-back of msfx_track_result -- in a
stand-alone sanitized executable (tests/cpp/frame_tracking_arrays_main.cpp), never inside python, and the same table
against its Python side (_lib.TRACK_ARRAYS, track_shapes and the ctypes struct)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mono_slam_framework_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")
UNITS = ["call", "match", "cur", "corr"]      # the C++ unit counts, in their order


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("frame_tracking_arrays") / "frame_tracking_arrays")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "frame_tracking_arrays_main.cpp"), "-o", path])
    return path


def test_carve_and_copy_back_in_a_sanitized_executable(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout


def test_the_table_agrees_with_the_python_side(exe):
    rows = [line.split() for line in subprocess.check_output([exe, "--print"], text=True).splitlines()]
    table, struct = _lib.TRACK_ARRAYS, _lib.TrackResult
    assert [r[1] for r in rows] == [a[0] for a in table] == [f[0] for f in struct._fields_[2:]]
    cap, n_cur, corr = 7, 5, 23
    shapes = _lib.track_shapes(cap, n_cur, corr)
    count = {"call": 1, "match": cap, "cur": n_cur, "corr": corr}
    for (_, name, offset, elem, unit, tail, per_cap, required), (_, dt, per, shape_tail) in zip(rows, table):
        assert int(offset) == getattr(struct, name).offset, name
        assert int(elem) == np.dtype(dt).itemsize and UNITS[int(unit)] == per, name
        assert int(per_cap) == 0 and int(required) == 1, name
        assert int(tail) == int(np.prod(shape_tail, dtype=np.int64)), name
        shape, sdt = shapes[name]
        assert sdt == dt and count[per] * int(tail) == int(np.prod(shape)), name
    assert C.sizeof(struct) == 8 + 8 * len(rows) and len(rows) == 16
    assert _lib.CARRY_NAMES == tuple(a[0] for a in table[:8]) and _lib.CARRY_NAMES[-1] == "corr_point"
