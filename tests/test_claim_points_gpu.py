"""GPU: msf_claim_points_device (steps 4-5 of include/msf_tracking.h) on injected lists -- extracted frames never give the
tied and edge cases.  The records, statuses, n_claimed and corr_* are exactly those of tests/tracking_ref.py's
order-independent statement (which test_tracking_ref.py proves equal to the literal sequential loop) and of the host
build of csrc/tracking_solve.h.  The last tests repeat this with lists, runs, key frames and the frame's own map past one
chunk of 256 (tracking_ref.CHUNK_CASES)."""
import numpy as np
import pytest

from tests import tracking_host as th
from tests import tracking_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.8, tr.W, tr.H, max_batch_pairs=8)
    yield m
    m.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return th.build(tmp_path_factory.mktemp("tracking_host"))


def run_device(fm, lmap, lists, n_out, matched, cap, corr_cap):
    """-> dict of numpy arrays; claims beyond n_claims and claim_status beyond the lists keep their fill (-9, 255)"""
    import torch
    from mono_slam_framework_amd import _lib
    n_kf = len(lists)
    z = lambda shape, dt, fill: torch.full(shape, fill, dtype=getattr(torch, dt), device="cuda")
    out = {}
    for k, (shape, dt) in _lib.tracking_shapes(_lib.CLAIM_ARRAYS, len(lmap["points"]), n_kf, cap, corr_cap).items():
        out[k] = z((n_kf * cap, 4), "int32", -9) if k == "claims" else z(shape, dt, 255 if k == "claim_status" else 0)
    d_m = torch.from_numpy(th.pad_lists(lists, cap)).cuda()
    d_n = torch.from_numpy(np.ascontiguousarray(n_out, np.int32)).cuda()
    d_g = torch.from_numpy(np.ascontiguousarray(matched, np.uint8)).cuda()
    fm.claim_points_device(fm.local_map_to_device(lmap), d_m, d_n, d_g, corr_cap, out=out)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got["n_claims"] = int(got["n_claims"][0])
    return got


def check(fm, host, lmap, prm, lists, n_out, cap, corr_cap, matched=None, label="", ref=None):
    """ref: order_independent() of these very arguments where the caller has it already"""
    if ref is None:
        ref = tr.order_independent(lmap, prm, lists, n_out, cap, corr_cap, matched=matched)
    got = run_device(fm, lmap, lists, n_out, ref["matched"], cap, corr_cap)
    assert int(got["status_word"][0]) == 0
    th.check_claims(got, ref, n_out, cap, label)
    assert (got["claims"][ref["n_claims"]:] == -9).all(), "records beyond n_claims are untouched"
    hb = th.claims(host, lmap, th.pad_lists(lists, cap), n_out, ref["matched"], corr_cap)
    th.check_claims(hb, ref, n_out, cap, label + " (host build)")
    return ref, got


def test_list_lengths_and_a_clipped_list(fm, host):
    """lists of 0, 1, 63, 64, 65, 256, 257 matches and one with n_out > cap (clipped at 280)"""
    lmap, prm, lists, _ = tr.scene(11, list_len=330)
    lens = [0, 1, 63, 64, 65, 256, 257, 300]
    assert all(len(l) >= 300 for l in lists)
    n_out = np.array(lens, np.int32)
    n_cur = len(lmap["cur_key"])
    ref, got = check(fm, host, lmap, prm, lists, n_out, 280, n_cur + 8 * 280, matched=np.ones(8, np.uint8), label="lengths")
    assert (ref["claim_status"][7, :280] != 255).all() and list((ref["claim_status"] != 255).sum(1)) == lens[:7] + [280]
    assert all(np.bincount(ref["claim_status"][ref["claim_status"] != 255], minlength=5) >= 5)
    # the call is bit-identical to a second call
    again = run_device(fm, lmap, lists, n_out, np.ones(8, np.uint8), 280, n_cur + 8 * 280)
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k
    # corr_cap one short: n_corr = -1, nothing of corr_* written, the claims intact
    short = run_device(fm, lmap, lists, n_out, np.ones(8, np.uint8), 280, n_cur + ref["n_claims"] - 1)
    assert short["n_corr"][0] == -1 and not short["corr_point"].any() and not short["corr_p3d"].any()
    assert np.array_equal(short["claims"], got["claims"]) and np.array_equal(short["claim_status"], got["claim_status"])
    exact = run_device(fm, lmap, lists, n_out, np.ones(8, np.uint8), 280, n_cur + ref["n_claims"])
    assert exact["n_corr"][0] == n_cur + ref["n_claims"]


@pytest.mark.parametrize("seed,cap", [(1, 128), (2, 256), (3, 64)])
def test_scenes_with_the_gate_of_step_three(fm, host, seed, cap):
    lmap, prm, lists, n_out = tr.scene(seed)
    check(fm, host, lmap, prm, lists, n_out, cap, len(lmap["cur_key"]) + 8 * cap, label="scene %d" % seed)


def test_tied_and_edge_cases(fm, host):
    """the same k1 in three key frames and three times inside one list, the corners, end points at -1 and at W, k1
    occupied, k2 without an entry, an unmatched key frame in the middle, an invalid list"""
    lmap, prm, lists, n_out = tr.tied_case()
    ref, _ = check(fm, host, lmap, prm, lists, n_out, 16, 100, label="tied, gated")
    assert list(ref["claim_status"][0, :13]) == [0, 4, 4, 0, 0, 1, 1, 1, 1, 2, 3, 3, 3]
    forced, _ = check(fm, host, lmap, prm, lists, n_out, 16, 100, matched=np.ones(5, np.uint8), label="tied, every key frame")
    assert list(forced["n_claimed"]) == [3, 1, 1, 2, 0]


def test_unrelated_rows_of_the_point_table_do_not_matter(fm, host):
    lmap, prm, lists, n_out = tr.scene(2)
    cap, corr_cap = 256, len(lmap["cur_key"]) + 8 * 256
    ref, got = check(fm, host, lmap, prm, lists, n_out, cap, corr_cap)
    unrelated = np.setdiff1d(np.arange(len(lmap["points"])), np.concatenate([lmap["kf_point"], lmap["cur_point"]]))
    assert len(unrelated) >= 20
    other = dict(lmap, points=lmap["points"].copy())
    other["points"][unrelated] = lmap["points"][np.random.default_rng(0).permutation(unrelated)]
    again = run_device(fm, other, lists, n_out, ref["matched"], cap, corr_cap)
    for k in got:
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k


def test_a_malformed_map_writes_only_status_word_and_zero_key_frames_are_no_error(fm):
    lmap, prm, lists, n_out = tr.scene(3, n_points=60, n_kf=3, per_kf=20, n_cur=8, list_len=30)
    bad = dict(lmap, kf_point=lmap["kf_point"].copy())
    bad["kf_point"][7] = 60
    got = run_device(fm, bad, lists, n_out, np.ones(3, np.uint8), 32, 200)
    assert int(got["status_word"][0]) == -1 and got["n_claims"] == 0 and not got["n_claimed"].any()
    assert (got["claims"] == -9).all() and (got["claim_status"] == 255).all() and not got["corr_point"].any()
    none = fm.make_local_map(lmap["points"], [], [], [], lmap["cur_key"], lmap["cur_point"])
    got = run_device(fm, none, [], np.zeros(0, np.int32), np.zeros(0, np.uint8), 32, 200)
    assert int(got["status_word"][0]) == 0 and got["n_claims"] == 0 and got["n_corr"][0] == 8
    assert np.array_equal(got["corr_point"][:8], lmap["cur_point"])


# ---- past one chunk of 256 (tracking_ref.CHUNK_CASES; test_tracking_ref.py asserts what each case reaches) ---------------

@pytest.mark.parametrize("name", list(tr.CHUNK_CASES))
def test_lists_runs_and_key_frames_past_one_chunk(fm, host, name):
    """k_claim_mark at blockIdx.x >= 2, k_claim_pack's running offset over three and more chunks with winners and
    losers of one pixel in different chunks and key frames, k_claim_finish's k += 256 sums and its row n_kf at
    blockIdx.x > 0 -- once behind the gate of step 3, once with every key frame matched"""
    lmap, prm, lists, n_out, cap = tr.chunk_case(name)
    corr_cap = tr.corr_room(lmap, lists, cap)
    for forced in (False, True):
        ref = tr.chunk_reference(name, forced)
        _, got = check(fm, host, lmap, prm, lists, n_out, cap, corr_cap, label="%s forced %d" % (name, forced), ref=ref)
        k = ref["n_corr"]
        assert k == len(lmap["cur_key"]) + ref["n_claims"]
        assert not got["corr_point"][k:].any() and not got["corr_p2d"][k:].any() and not got["corr_p3d"][k:].any()
        if forced and name in ("long", "ladder-320-empty"):      # the call is bit-identical to a second call
            again = run_device(fm, lmap, lists, n_out, ref["matched"], cap, corr_cap)
            for key in got:
                assert np.asarray(got[key]).tobytes() == np.asarray(again[key]).tobytes(), key


def test_a_map_malformed_past_the_first_chunk_writes_only_status_word(fm):
    lmap, prm, lists, n_out, cap = tr.chunk_case("long")
    for key, at, value in tr.late_faults(lmap):
        got = run_device(fm, tr.with_fault(lmap, key, at, value), lists, n_out, np.ones(4, np.uint8), cap,
                         tr.corr_room(lmap, lists, cap))
        assert int(got["status_word"][0]) == -1 and got["n_claims"] == 0 and not got["n_claimed"].any(), (key, at)
        assert (got["claims"] == -9).all() and (got["claim_status"] == 255).all(), (key, at)
        assert not got["corr_point"].any() and not got["corr_p3d"].any() and not got["corr_p2d"].any(), (key, at)
        assert int(got["n_corr"][0]) == 0, (key, at)
