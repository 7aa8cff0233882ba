"""GPU: msfx_carry_points_device on injected lists -- k_carry alone.  For list lengths on both sides of a wave and of the
workgroup's chunk, a clipped list, the tied case and an empty frame map: the records, both status arrays, n_map and the
correspondences are exactly those of tests/frame_tracking_ref.py and of the host build of csrc/frame_tracking_solve.h,
and every byte beyond n_map (and beyond the list) is untouched.  A corr_cap one short answers -2, each malformed map -1,
an invalid list -3, all without writing anything else.  A second call is bit-identical.

Past one chunk of step 3 (more words than the workgroup has threads): totals on both sides of 1024, 2048, 4096 and at 8191
and 8192, the two one-sided splits of 8192, 8193, a clipped list of 6000 and fr.boundary_case() -- runs of equal keys over
the chunk edges, a last word that is no padding, the 64 KiB LDS block above 4096 words.  That the inputs reach these is
asserted from fr.sorted_words first."""
import numpy as np
import pytest

from tests import frame_tracking_host as fh
from tests import frame_tracking_ref as fr

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.8, fr.W, fr.H, max_batch_pairs=2)
    yield m
    m.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return fh.build(tmp_path_factory.mktemp("frame_tracking_host"))


def filled(fm, cap, n_cur, corr_cap):
    """the carry's output tensors filled with 255 (bytes) / -7: what stays is what was not written"""
    import torch
    from mono_slam_framework_amd import _lib, results
    shapes = _lib.track_shapes(cap, n_cur, corr_cap)
    d = results.alloc(shapes, "cuda", leave_out=set(shapes) - set(_lib.CARRY_NAMES))
    for k, v in d.items():
        v.fill_(255 if v.dtype == torch.uint8 else -7)
    return d


def device_carry(fm, d_fmap, matches, n, cap, n_cur, corr_cap):
    import torch
    d = filled(fm, cap, n_cur, corr_cap)
    d_m = torch.from_numpy(fh.pad_list(matches, cap)).cuda()
    d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
    fm.carry_points_device(d_fmap, d_m, d_n, corr_cap, out=d)
    torch.cuda.synchronize()
    return d


def scene_330(seed):
    """the reference scene with a list of 330 matches, so that every length of LENGTHS is a prefix of it"""
    return fr.scene(seed, n_matches=330)


@pytest.mark.parametrize("n", LENGTHS)
def test_list_lengths(fm, host, n):
    fmap, matches = scene_330(n)
    d_fmap = fm.frame_map_to_device(fmap)
    cap, n_cur = 330, len(fmap["cur_key"])
    corr_cap = n_cur + n                                  # exactly enough
    got = device_carry(fm, d_fmap, matches, n, cap, n_cur, corr_cap)
    ref = fr.carry(fmap, matches, n, cap, corr_cap)
    assert ref["status"] == 0
    fh.check_carry(got, ref, "device n=%d" % n)
    fh.check_carry(fh.carry(host, fmap, fh.pad_list(matches, cap), n, corr_cap), ref, "host n=%d" % n)
    again = device_carry(fm, d_fmap, matches, n, cap, n_cur, corr_cap)
    for k in got:
        assert got[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), k      # bit-identical replay


def test_clipped_list_tied_case_and_empty_frame_map(fm, host):
    fmap, matches = scene_330(9)
    n_cur = len(fmap["cur_key"])
    ref = fr.carry(fmap, matches, 300, 280, n_cur + 280)        # n_out 300, cap 280: the first 280
    assert ref["status"] == 0 and (ref["carry_status"] != 255).sum() == 280
    fh.check_carry(device_carry(fm, fm.frame_map_to_device(fmap), matches, 300, 280, n_cur, n_cur + 280), ref, "clipped")
    tied, tm = fr.tied_case()
    n = len(tm)
    ref = fr.carry(tied, tm, n, n + 5, 3 + n)
    fh.check_carry(device_carry(fm, fm.frame_map_to_device(tied), tm, n, n + 5, 3, 3 + n), ref, "tied")
    fh.check_carry(fh.carry(host, tied, fh.pad_list(tm, n + 5), n, 3 + n), ref, "tied, host")
    assert list(ref["carry_status"][:n]) == [4, 4, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 3, 3, 3, 3, 3]
    empty = dict(fmap, cur_key=np.zeros(0, np.int32), cur_point=np.zeros(0, np.int32))     # after Clear()
    ref = fr.carry(empty, matches, 257, 330, 257)
    assert ref["status"] == 0 and 0 < ref["n_map"] < 257
    fh.check_carry(device_carry(fm, fm.frame_map_to_device(empty), matches, 257, 330, 0, 257), ref, "n_cur = 0")


# ---- past one chunk of step 3: more words than the workgroup has threads, up to the 8192 of the interface ----------------

# (n_cur, n): totals on both sides of 1024, 2048, 4096 (above it the sort takes the 64 KiB block) and at 8192, then the
# two splits of 8192 words with one side empty
EDGE_PAIRS = [(150, 873), (150, 874), (150, 875), (500, 1548), (500, 1549), (500, 3596), (500, 3597), (3000, 5191),
              (3000, 5192), (0, 8192), (8192, 0)]
SEED = 7
_SCENES = {}


def large_scene(n_cur, n):
    """fr.scene over 3000 points and 6000 entries of the train frame, computed once per size"""
    if (n_cur, n) not in _SCENES:
        _SCENES[n_cur, n] = fr.scene(SEED, n_points=3000, n_ref=6000, n_cur=n_cur, n_matches=n)
    return _SCENES[n_cur, n]


def carry_three_ways(fm, host, fmap, matches, n, cap, corr_cap, label, replay=True):
    """the device and the host build against the reference, every byte; one replay of the device -> (device, reference)"""
    n_cur = len(fmap["cur_key"])
    d_fmap = fm.frame_map_to_device(fmap)
    ref = fr.carry(fmap, matches, n, cap, corr_cap)
    got = device_carry(fm, d_fmap, matches, n, cap, n_cur, corr_cap)
    fh.check_carry(got, ref, "device " + label)
    fh.check_carry(fh.carry(host, fmap, fh.pad_list(matches, cap), n, corr_cap), ref, "host " + label)
    if replay:
        again = device_carry(fm, d_fmap, matches, n, cap, n_cur, corr_cap)
        for k in got:
            assert got[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), (label, k)
    return got, ref


@pytest.mark.parametrize("n_cur,n", EDGE_PAIRS)
def test_totals_at_the_size_edges(fm, host, n_cur, n):
    """corr_cap = n_cur + n exactly.  What a size reaches is proven from fr.sorted_words before the device is asked."""
    fmap, matches = large_scene(n_cur, n)
    assert (len(fmap["cur_key"]), len(matches)) == (n_cur, n)
    total, cap = n_cur + n, max(n, 1)
    words = fr.sorted_words(fmap, matches, n, cap)
    p2 = 1 << max(total - 1, 0).bit_length()
    across = [e for e in range(1024, total, 1024) if fr.runs_across(words, e)]
    print("(%d, %d): total %d, %d valid words, p2 %d, %d chunks of step 3, runs across %s" % (
        n_cur, n, total, len(words), p2, -(-total // 1024), across))
    if n_cur == 150:                                     # from index 1023 on padding alone: at 1025 a second chunk runs
        assert len(words) <= 1023 <= total               # over nothing, and offset must not move
    if (n_cur, n) in ((3000, 5192), (0, 8192)):
        assert across and total == p2 == 8192
    if (n_cur, n) == (8192, 0):
        assert len(words) == total == p2 == 8192         # no padding: the word at 8191 wins through i + 1 >= n
    got, ref = carry_three_ways(fm, host, fmap, matches, n, cap, total, "(%d, %d)" % (n_cur, n))
    assert ref["status"] == 0 and ref["n_map"] == len(set(k for k, _ in words))
    if (n_cur, n) == (8192, 0):
        assert ref["n_map"] == 8192 and not got["cur_status"].cpu().numpy().any()
    if n_cur == 0:
        assert got["cur_status"].numel() == 0


def test_one_over_8192_answers_no_room(fm, host):
    fmap, matches = large_scene(3000, 5193)
    _, ref = carry_three_ways(fm, host, fmap, matches, 5193, 5193, 8193, "8193 words", replay=False)
    assert ref["status"] == -2
    fmap, matches = large_scene(3000, 5192)
    _, ref = carry_three_ways(fm, host, fmap, matches, 5192, 5192, 8191, "corr_cap 8191", replay=False)
    assert ref["status"] == -2


def test_boundary_case(fm, host):
    """runs of equal keys over the chunk edges at 1024 and 3072, a run of one at 2047, on the 64 KiB block"""
    fmap, matches = fr.boundary_case()
    runs = fr.boundary_runs(fmap, matches)               # the inputs reach the edges: proven before the device is asked
    n_cur, n = len(fmap["cur_key"]), len(matches)
    got, ref = carry_three_ways(fm, host, fmap, matches, n, n, n_cur + n, "boundary")
    carry_status, cur_status = got["carry_status"].cpu().numpy(), got["cur_status"].cpu().numpy()
    entry, *three = runs[1022]
    assert cur_status[entry] == 1 and [carry_status[r - n_cur] for r in sorted(three)] == [4, 4, 0]
    assert carry_status[runs[2047][0] - n_cur] == 0
    entry, match = runs[3071]
    assert cur_status[entry] == 1 and carry_status[match - n_cur] == 0
    # the records at and behind each edge: a record's place is the number of distinct keys in front of it
    words = fr.sorted_words(fmap, matches, n, n)
    keys = sorted(set(k for k, _ in words))
    rec = got["map"].cpu().numpy()
    for first, ranks in runs.items():
        at = keys.index(words[first][0])
        assert tuple(rec[at][[0, 2]]) == (keys[at], max(ranks) - n_cur), first
        assert rec[at + 1][0] == keys[at + 1] == words[first + len(ranks)][0], first


def test_clipped_long_list(fm, host):
    fmap, matches = large_scene(3000, 6000)
    got, ref = carry_three_ways(fm, host, fmap, matches, 6000, 5000, 8000, "n_out 6000, cap 5000")     # the first 5000
    assert ref["status"] == 0 and tuple(got["carry_status"].shape) == (5000,)
    assert not (got["carry_status"].cpu().numpy() == 255).any()
    assert np.array_equal(ref["map"], fr.carry(fmap, matches[:5000], 5000, 5000, 8000)["map"])


def test_refusals_write_nothing(fm):
    fmap, matches = scene_330(3)
    d_fmap = fm.frame_map_to_device(fmap)
    n_cur = len(fmap["cur_key"])
    for n, corr_cap, want in ((160, n_cur + 159, -2), (-1, n_cur + 330, -3), (160, n_cur + 160, 0)):
        ref = fr.carry(fmap, matches, n, 330, corr_cap)
        assert ref["status"] == want
        fh.check_carry(device_carry(fm, d_fmap, matches, n, 330, n_cur, corr_cap), ref, "corr_cap %d" % corr_cap)
    bad = fr.malformed(fmap)
    assert len(bad) == 12
    for what, m in bad:
        fh.check_carry(device_carry(fm, fm.frame_map_to_device(m), matches, 160, 330, n_cur, n_cur + 330), dict(status=-1), what)


def test_host_refusals(fm):
    import torch
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import MsfError
    fmap, matches = scene_330(3)
    d_fmap = fm.frame_map_to_device(fmap)
    d_m = torch.from_numpy(fh.pad_list(matches, 330)).cuda()
    d_n = torch.tensor([10], dtype=torch.int32, device="cuda")
    with pytest.raises(MsfError) as e:
        fm.carry_points_device(d_fmap, d_m, d_n, -1, out=filled(fm, 330, len(fmap["cur_key"]), 16))
    assert e.value.code == _lib.MSF_ERR_INVALID_ARG and "msfx_carry_points_device: " in str(e.value) and "corr_cap < 0" in str(e.value)
