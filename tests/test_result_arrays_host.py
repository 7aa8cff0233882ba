"""CPU: csrc/result_arrays.h -- the tables behind the carve and the copy-back of the four geometry result structs -- in a
stand-alone sanitized executable (tests/cpp/result_arrays_main.cpp), never inside python, and the same tables against
their Python side (_lib.PNP_ARRAYS, POSE_ARRAYS, MOTION_ARRAYS, NEW_POINTS_ARRAYS and the ctypes structs).  A wrong
count in a carve is a kernel writing past its piece of the workspace and a wrong count in a copy-back a write past the
caller's array: here AddressSanitizer reports either."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mono_slam_framework_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mono_slam_framework_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("result_arrays") / "result_arrays")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "cpp", "result_arrays_main.cpp"), "-o", path])
    return path


def test_carve_and_copy_back_in_a_sanitized_executable(exe):
    """every table over lists {1, 3}, cap {1, 5}, the smallest unit counts and the wanted sets none / all / alone /
    alternating: pieces on the 256-byte grid, disjoint, of the documented size, none for what nobody needs; the
    copy-back moves the asked extent and nothing else, full rows as one copy"""
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout


# table -> (ctypes struct, Python table, unit names in the order of the C++ unit counts, shapes for a call)
LISTS, ITS, RECS, CAP = 3, 5, 2, 7
PER_LIST = {"list": 1, "hyp": ITS, "rec": RECS, "round": 4, "it": 40}


def _list_shapes(arrays):
    return {name: ((LISTS,) + tuple(CAP if t == "cap" else t for t in tail), dt) for name, dt, _, tail in arrays}


TABLES = {"pnp": (_lib.PnpResult, _lib.PNP_ARRAYS, ["list", "hyp", "rec"], _lib.pnp_shapes(LISTS, ITS, RECS, CAP)),
          "pose": (_lib.PoseResult, _lib.POSE_ARRAYS, ["list", "round", "it"], _lib.pose_shapes(LISTS, CAP)),
          "motion": (_lib.MotionResult, _lib.MOTION_ARRAYS, ["list"], _list_shapes(_lib.MOTION_ARRAYS)),
          "new_points": (_lib.NewPointsResult, _lib.NEW_POINTS_ARRAYS, ["list"], _list_shapes(_lib.NEW_POINTS_ARRAYS))}
REQUIRED = {"pnp": {"n_records", "counts", "pose_f64"}, "pose": {"n_good"}, "new_points": {"n_new"},
            "motion": {"ok", "model", "n_cand", "cand_R", "cand_t", "cand_good", "cand_parallax", "winner"}}


def test_tables_agree_with_the_python_side(exe):
    """names, order and offsets against the ctypes structs; element size, unit and trailing shape against the Python
    tables; the byte size of every array against np.prod(shape) * itemsize; the required sets against the pipeline
    headers"""
    rows = {}
    for line in subprocess.check_output([exe, "--print"], text=True).splitlines():
        table, name, offset, elem, unit, tail, per_cap, required = line.split()
        rows.setdefault(table, []).append((name, int(offset), int(elem), int(unit), int(tail), int(per_cap), int(required)))
    assert set(rows) == set(TABLES)
    for table, (struct, arrays, unit_names, shapes) in TABLES.items():
        fields = struct._fields_[2:]
        assert [r[0] for r in rows[table]] == [f[0] for f in fields] == [a[0] for a in arrays], table
        assert C.sizeof(struct) == 8 + 8 * len(arrays), table
        for (name, offset, elem, unit, tail, per_cap, required), (_, dt, per, shape_tail) in zip(rows[table], arrays):
            what = "%s.%s" % (table, name)
            assert offset == getattr(struct, name).offset, what
            assert elem == np.dtype(dt).itemsize, what
            assert unit_names[unit] == per, what
            assert per_cap == (1 if "cap" in shape_tail else 0), what
            assert shape_tail[:1] == ("cap",) or "cap" not in shape_tail, what   # a per-cap row runs along the list first
            assert tail == int(np.prod([t for t in shape_tail if t != "cap"], dtype=np.int64)), what
            shape, sdt = shapes[name]
            assert sdt == dt, what
            assert LISTS * PER_LIST[per] * tail * (CAP if per_cap else 1) * elem == int(np.prod(shape)) * np.dtype(dt).itemsize, what
            assert bool(required) == (name in REQUIRED[table]), what
