"""GPU: msfx_carry_points_device on injected lists -- k_carry alone.  For list lengths on both sides of a wave and of the
workgroup's chunk, a clipped list, the tied case and an empty frame map: the records, both status arrays, n_map and the
correspondences are exactly those of tests/frame_tracking_ref.py and of the host build of csrc/frame_tracking_solve.h,
and every byte beyond n_map (and beyond the list) is untouched.  A corr_cap one short answers -2, each malformed map -1,
an invalid list -3, all without writing anything else.  A second call is bit-identical."""
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
