"""CPU: csrc/tracking_solve.h -- the arithmetic and index rules of tracking_kernels.hip -- compiled for the host
(g++ -ffp-contract=off, tests/cpp/tracking_host.cpp): step 2 against the float64 reference of tests/tracking_ref.py
within the bars written out there and bit for bit against its numpy float32 restatement, steps 1, 4 and 5 exactly
against the order-independent statement.  The device build runs the same expressions in the same order; what only the
GPU can show is in test_frustum_gpu.py and test_claim_points_gpu.py.  The empty, one-element and malformed inputs run in
a stand-alone sanitized executable, never inside python.  The scenes past one chunk of 256 (tracking_ref.CHUNK_CASES) and
the maps that are malformed only there are held to the same references."""
import os
import subprocess

import numpy as np
import pytest

from tests import tracking_host as th
from tests import tracking_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return th.build(tmp_path_factory.mktemp("tracking_host"))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_build_meets_the_float64_bars(host, seed):
    lmap, prm, lists, n_out = tr.scene(seed)
    ref = tr.order_independent(lmap, prm, lists, n_out, 256, 1 << 20)
    got = th.frustum(host, lmap, prm)
    assert got["status_word"] == 0
    diag = np.stack([got[k] for k in ("u", "v", "dist", "view_cos")], 1)
    for k in ("status", "visible", "owner_kf", "n_to_match"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(diag.view(np.uint32), ref["diag"].view(np.uint32))     # the numpy f32 restatement, bit for bit
    worst, in_band = tr.check_against_f64(lmap["points"], prm, got["status"], diag, got["status"] >= 7, "host seed %d" % seed)
    print("host seed %d: worst fraction of a bar %.3f, %.2f %% of the points in a band" % (seed, worst, 100 * in_band))


@pytest.mark.parametrize("seed,cap", [(1, 128), (2, 256), (3, 64)])
def test_host_claims_equal_the_reference(host, seed, cap):
    lmap, prm, lists, n_out = tr.scene(seed)
    n_cur = len(lmap["cur_key"])
    ref = tr.order_independent(lmap, prm, lists, n_out, cap, n_cur + 8 * cap)
    got = th.claims(host, lmap, th.pad_lists(lists, cap), n_out, ref["matched"], n_cur + 8 * cap)
    th.check_claims(got, ref, n_out, cap, "host seed %d" % seed)
    short = th.claims(host, lmap, th.pad_lists(lists, cap), n_out, ref["matched"], n_cur + ref["n_claims"] - 1)
    assert short["n_corr"][0] == -1 and not short["corr_point"].any()
    assert np.array_equal(short["claims"], got["claims"])


def test_tied_cases(host):
    lmap, prm, lists, n_out = tr.tied_case()
    for matched in (None, np.ones(5, np.uint8)):
        ref = tr.order_independent(lmap, prm, lists, n_out, 16, 100, matched=matched)
        got = th.claims(host, lmap, th.pad_lists(lists, 16), n_out, ref["matched"], 100)
        th.check_claims(got, ref, n_out, 16, "host tied")
    f = th.frustum(host, lmap, prm)
    assert list(f["n_to_match"]) == [3, 0, 4, 0, 0] and list(f["owner_kf"][:10]) == [0, 0, 0, 0, 2, 2, 2, 2, 1, 1]


def test_malformed_maps_are_refused(host):
    lmap, prm, lists, n_out = tr.scene(1, n_points=40, n_kf=3, per_kf=10, n_cur=6, list_len=10)
    for key, at, value in [("kf_point", 3, 40), ("kf_point", 0, -1), ("kf_key", 2, tr.W * tr.H), ("kf_start", 1, 1000),
                           ("kf_start", 3, 5), ("cur_key", 1, -1), ("cur_point", 0, 40)]:
        bad = {k: v.copy() for k, v in lmap.items()}
        bad[key][at] = value
        assert th.frustum(host, bad, prm)["status_word"] == -1, (key, at)
    bad = {k: v.copy() for k, v in lmap.items()}
    bad["kf_key"][1] = bad["kf_key"][0]            # not strictly increasing
    assert th.frustum(host, bad, prm)["status_word"] == -1
    bad = {k: v.copy() for k, v in lmap.items()}
    bad["points"]["flags"][5] = 4
    assert th.frustum(host, bad, prm)["status_word"] == -1
    nan = dict(prm, max_x=np.float32(np.nan))
    assert th.frustum(host, lmap, nan)["status_word"] == -1


@pytest.mark.parametrize("name", list(tr.CHUNK_CASES))
def test_host_build_equals_the_reference_past_one_chunk(host, name):
    """runs, key frames, the frame's map and lists past 256 (tracking_ref.CHUNK_CASES): steps 1-2 and, once with the
    gate of step 3 and once with every key frame matched, steps 4-5"""
    lmap, prm, lists, n_out, cap = tr.chunk_case(name)
    ref = tr.chunk_reference(name)
    got = th.frustum(host, lmap, prm)
    assert got["status_word"] == 0
    diag = np.stack([got[k] for k in ("u", "v", "dist", "view_cos")], 1)
    for k in ("status", "visible", "owner_kf", "n_to_match"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(diag.view(np.uint32), ref["diag"].view(np.uint32))
    tr.check_against_f64(lmap["points"], prm, got["status"], diag, got["status"] >= 7, "host " + name)
    padded = th.pad_lists(lists, cap)
    for forced in (False, True):
        ref = tr.chunk_reference(name, forced)
        claimed = th.claims(host, lmap, padded, n_out, ref["matched"], tr.corr_room(lmap, lists, cap))
        th.check_claims(claimed, ref, n_out, cap, "host %s forced %d" % (name, forced))


def test_late_malformed_maps_are_refused(host):
    """the faults that only a later chunk or workgroup of the checking kernel meets"""
    lmap, prm, _, _, _ = tr.chunk_case("long")
    assert th.frustum(host, lmap, prm)["status_word"] == 0
    for key, at, value in tr.late_faults(lmap):
        assert th.frustum(host, tr.with_fault(lmap, key, at, value), prm)["status_word"] == -1, (key, at)


def test_edge_inputs_in_a_sanitized_executable(tmp_path):
    """the family's layout and the five steps on the empty, one-element and malformed inputs of the refusal list"""
    exe = str(tmp_path / "tracking_edge")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-I", th.CSRC,
                           os.path.join(ROOT, "tests", "cpp", "tracking_edge_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
