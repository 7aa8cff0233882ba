"""CPU: the host build of csrc/frame_tracking_solve.h (the code the kernels run), chained with the host build of
csrc/pose_solve.h, equals tests/frame_tracking_ref.py exactly in every integer output; and its edge cases run in a
stand-alone sanitized executable."""
import os
import subprocess

import numpy as np
import pytest

from tests import frame_tracking_host as fh
from tests import frame_tracking_ref as fr
from tests import pose_host
from tests.test_frame_tracking_ref import dressed, large_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return fh.build(tmp_path_factory.mktemp("frame_tracking_host"))


@pytest.fixture(scope="module")
def pose(tmp_path_factory):
    return pose_host.build(tmp_path_factory.mktemp("pose_host"))


def large_case(case):
    return fr.boundary_case() if case == "boundary" else large_scene()


@pytest.mark.parametrize("seed", (0, 1, 2, "boundary", "large"))
def test_carry_equals_the_reference(host, seed):
    """seeds: 150 entries and a list of 160; boundary and large: more than 4096 words, runs over the chunk edges"""
    fmap, matches = fr.scene(seed) if isinstance(seed, int) else large_case(seed)
    n_cur, k = len(fmap["cur_key"]), len(matches)
    for n, cap, corr_cap, min_matches in ((k, k, n_cur + k, 0), (k + 140, k - 40, n_cur + k - 40, 0), (0, k, n_cur, 0),
                                          (14, k, n_cur, 15), (k, k, n_cur + k - 1, 0), (-1, k, n_cur + k, 0),
                                          (1, k, n_cur + k, 0)):
        got = fh.carry(host, fmap, fh.pad_list(matches, cap), n, corr_cap, min_matches)
        fh.check_carry(got, fr.carry(fmap, matches, n, cap, corr_cap, min_matches), (seed, n, cap, corr_cap))
    for what, bad in fr.malformed(fmap):
        fh.check_carry(fh.carry(host, bad, fh.pad_list(matches, k), k, n_cur + k), dict(status=-1), what)


def test_tied_case(host):
    fmap, matches = fr.tied_case()
    n = len(matches)
    fh.check_carry(fh.carry(host, fmap, fh.pad_list(matches, n + 3), n, n + 3), fr.carry(fmap, matches, n, n + 3, n + 3), "tied")


@pytest.mark.parametrize("kind,seed,observed,n_given,n_scene", [
    pytest.param("base", 1, True, None, 96, id="base-1-True-None"), pytest.param("few", 2, True, None, 96, id="few-2-True-None"),
    pytest.param("base", 1, False, None, 96, id="base-1-False-None"), pytest.param("wide", 3, True, 14, 96, id="wide-3-True-14"),
    pytest.param("base", 2, True, 9, 96, id="base-2-True-9"), pytest.param("wide", 3, True, None, 1500, id="wide-3-True-None-1500")])
def test_chain_with_the_pose_host_build(host, pose, kind, seed, observed, n_given, n_scene):
    """carry -> pose_solve.h -> cut, all three as host builds: every integer output equals the reference run on the same
    outlier bytes, and the list the optimiser was given is the reference's.  The scene of 1500: six chunks of the cut,
    each with kept and removed records."""
    fmap, matches, sc = dressed(kind, seed, observed, n=n_scene)
    cap = len(matches)
    n = cap if n_given is None else n_given
    min_matches = 15 if n_given != 9 else 0
    got = fh.carry(host, fmap, fh.pad_list(matches, cap), n, cap, min_matches)
    ref_carry = fr.carry(fmap, matches, n, cap, cap, min_matches)
    fh.check_carry(got, ref_carry, kind)
    n_map = ref_carry["n_map"]
    if got["status"] == 0:
        p = pose_host.run(pose, got["corr_p3d"][:n_map], got["corr_p2d"][:n_map], sc["K"], sc["Tcw0"])
        outliers = p["outliers"]
    else:
        outliers = np.zeros(max(n_map, 1), np.uint8)
    cut = fh.cut(host, fmap, got, np.concatenate([outliers, np.zeros(1, np.uint8)]), 10)
    ref = fr.order_independent(fmap, matches, n, cap, cap, min_matches, 10, lambda keys, points: (outliers[:len(keys)], {}))
    fh.check_cut(dict(cut, map=got["map"]), ref, kind)
    print("%s %d: n_map %d, kept %d, removed %d, n_matches_map %d, track_status %d" % (
        kind, seed, n_map, ref["n_kept"], ref["n_removed"], ref["n_matches_map"], ref["track_status"]))
    want = {(True, None): 0, (False, None): 2, (True, 14): 1, (True, 9): 2}[(observed, n_given)]
    assert ref["track_status"] == want
    if want == 0:
        assert ref["n_removed"] > 0 and ref["n_kept"] >= 10
    if n_scene == 1500:
        chunks = fr.cut_chunks(outliers[:n_map])
        print("n_good %d, (kept, removed) per chunk of 256: %s" % (p["n_good"], chunks))
        assert n_map == 1497 and len(chunks) == 6 and min(min(c) for c in chunks) >= 1


def test_edge_inputs_in_a_sanitized_executable(tmp_path):
    """an empty list, n_map of 0 / 2 / 3 / 9 / 10, the capacity edge at 8191 / 8192 / 8193 candidates, every malformed
    map, in buffers of exactly the promised sizes"""
    exe = str(tmp_path / "frame_tracking_edge")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", fh.CSRC,
                           os.path.join(ROOT, "tests", "cpp", "frame_tracking_edge_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
