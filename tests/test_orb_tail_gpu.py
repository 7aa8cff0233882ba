"""GPU: everything OrbPipeline launches behind FAST -- k_thr_harris (both forms), k_harris_flat, k_select and the three
instantiations of k_describe -- on candidate lists the test supplies (msf_debug_orb_tail), against the numpy
restatement in tests/orb_tail_ref.py.  The entry runs the launches an extraction runs (one helper serves both), so what
is pinned here is the product's path, at inputs a whole-image run never produces: the corners of every level's
rectangle, orientations on the axes, exact blur ties, key point counts around k_describe's stride -- with one patch
for all and with a different patch for each --, lists around every threshold and capacity of the two selection kernels.

Every comparison is array equality: stage 1 sorted by (y, x) with score and response bits, the key points in order with
the bits of x, y, response and angle, the descriptors.  The slots next to the call's are pre-set to a sentinel and must
still hold it.  Where a capacity is exceeded the kept subset depends on the order of atomics: the flag (a match call
answers n_out = -1) and the neighbours are all that is asserted.

That the inputs reach what they are made for, and that the reference equals the C oracle, is asserted on the CPU in
tests/test_orb_tail_ref.py."""
import functools

import numpy as np
import pytest

from tests import orb_tail_ref as R

pytestmark = pytest.mark.gpu

FORMS = (0, 1)                                   # dense form of k_thr_harris | streaming form + k_harris_flat
SENT = 0xA5


def _flags(mode):
    from mono_slam_framework_amd import _lib
    return _lib.MSF_FLAG_NO_FRAME_CACHE | {"even257": 0, "up257": _lib.MSF_FLAG_BLUR_TIE_HALF_UP,
                                           "up256": _lib.MSF_FLAG_BLUR_SUM256}[mode]


def _handle(w, h, mode="even257", pairs=5):
    from mono_slam_framework_amd.matcher import FeatureMatcher
    return FeatureMatcher(0.8, w, h, max_batch_pairs=pairs, flags=_flags(mode))


@functools.lru_cache(maxsize=None)
def _levels_of(key):
    return R.Levels.from_oracle(_IMAGES[key])


_IMAGES = {}


def _levels(img):
    key = (img.shape, img.tobytes())
    _IMAGES[key] = img
    return _levels_of(key)


def _device(imgs):
    """frames on the device with a row pitch 16 above the padded width, so that level 0's pitch is not its width"""
    import torch
    h, w = imgs[0].shape
    d = torch.full((len(imgs), h, ((w + 15) & ~15) + 16), 0x5A, dtype=torch.uint8, device="cuda")
    for i, im in enumerate(imgs):
        d[i, :, :w] = torch.from_numpy(np.ascontiguousarray(im)).cuda()
    return d


def _sentinel():
    kp = np.frombuffer(bytes([SENT]) * (R.KP_CAP * 32), R.KP_DTYPE).copy()
    return kp, np.full((R.KP_CAP, 32), SENT, np.uint8)


def _guard(fm, slot0, n):
    kp, desc = _sentinel()
    for s in (slot0 - 1, slot0 + n):
        if 0 <= s < 2 * fm.max_batch_pairs:
            fm.set_features(s, kp, desc)


def _guard_intact(fm, slot0, n, label):
    kp, desc = _sentinel()
    for s in (slot0 - 1, slot0 + n):
        if 0 <= s < 2 * fm.max_batch_pairs:
            assert fm.keypoints(s, cache=True).tobytes() == kp.tobytes(), "%s: key points of slot %d touched" % (label, s)
            assert (fm.descriptors(s, cache=True) == SENT).all(), "%s: descriptors of slot %d touched" % (label, s)


def _refused(fm, slots):
    """n_out of matching each slot with itself: -1 marks a slot whose extraction exceeded a capacity"""
    import torch
    s = torch.tensor(list(slots), dtype=torch.int32, device="cuda")
    out = torch.zeros((len(slots), 8, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(len(slots), dtype=torch.int32, device="cuda")
    fm.match_slots_device(s, s, out, cnt)
    return (cnt.cpu().numpy() == -1).tolist()


def _by_yx(a):
    return a[np.lexsort((a["lx"], a["ly"]))]


def _run(fm, imgs, lists, mode="even257", slot0=1, forms=FORMS, caps=None, label=""):
    """one call per form; every frame that stays inside the capacities against the reference, the others by their flag"""
    d = _device(imgs)
    n = len(imgs)
    refs = [R.tail(_levels(im), ls, mode, caps) for im, ls in zip(imgs, lists)]
    for form in forms:
        where = "%s form %d" % (label, form)
        _guard(fm, slot0, n)
        fm.orb_tail(d, lists, first_slot=slot0, form=form)
        assert _refused(fm, range(slot0, slot0 + n)) == [r.overflow for r in refs], where
        for f, ref in enumerate(refs):
            if ref.overflow:
                continue
            slot = slot0 + f
            for l in range(8):
                got = _by_yx(fm.stage1(slot, l, cache=True))
                assert len(got) == len(ref.stage1[l]), "%s frame %d level %d: stage 1 %d, reference %d" % (
                    where, f, l, len(got), len(ref.stage1[l]))
                assert got.tobytes() == ref.stage1[l].tobytes(), "%s frame %d level %d: stage 1" % (where, f, l)
            kp, desc = fm.keypoints(slot, cache=True), fm.descriptors(slot, cache=True)
            assert len(kp) == len(ref.kp), "%s frame %d: %d key points, reference %d" % (where, f, len(kp), len(ref.kp))
            for name in R.KP_DTYPE.names:
                np.testing.assert_array_equal(kp[name].view(np.int32), ref.kp[name].view(np.int32),
                                              err_msg="%s frame %d: %s" % (where, f, name))
            np.testing.assert_array_equal(desc, ref.desc, err_msg="%s frame %d: descriptors" % (where, f))
        _guard_intact(fm, slot0, n, where)
    return refs


# ------------------------------------------------------------------------------------------------------------ positions
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("size", ((R.W, R.H), (R.BIG_W, R.BIG_H)) + R.SMALL_SIZES)
def test_rectangle_corners_on_every_level(size, mode):
    """the four corners of every level's rectangle and four consecutive lx at both horizontal extremes, on noise: the
    aligned fetches of harris_at and k_describe at their outermost positions and with every byte offset"""
    w, h = size
    img = R.noise_image(w, h)
    lv = _levels(img)
    fm = _handle(w, h, mode)
    sizes = fm.level_sizes()
    assert [tuple(s[:2]) for s in sizes.tolist()] == [im.shape[::-1] for im in lv.images]
    assert sizes[:, 3].tolist() == lv.quotas
    lists = R.corner_lists(lv)
    refs = _run(fm, [img], [lists], mode, label="%dx%d %s" % (w, h, mode))
    assert len(refs[0].kp) == sum(len(c) for c in lists) > 0
    # the lists are where an extraction keeps them, and the pyramid is the reference's
    for l in range(8):
        got = fm.fast_candidates(1, l, cache=True)
        np.testing.assert_array_equal(got, lists[l].astype(np.int32).reshape(-1, 3))
        if l:
            np.testing.assert_array_equal(fm.level_pixels(1, l, cache=True), lv.images[l])
    fm.close()


# ------------------------------------------------------------------------------------------------------------ patches
@pytest.mark.parametrize("mode", R.MODES)
def test_patches(mode):
    """one call of five frames: orientations on the axes, the diagonals and at (0, 0); a constant frame; 253..255 (the
    clamp behind the 257-sum blur); exact column-pass ties of both kernels; Sobel sums above 2^24"""
    cases = [R.case_axis(), R.case_constant(), R.case_clamp(), R.case_tie(), R.case_blocks()]
    fm = _handle(R.W, R.H, mode)
    refs = _run(fm, [c[0] for c in cases], [c[1] for c in cases], mode, label="patches " + mode)
    assert [len(r.kp) for r in refs[:4]] == [9, 60, 100, 100] and len(refs[4].kp) >= 109
    assert (refs[1].desc == 0).all() and (refs[1].kp["angle"] == 0).all()
    fm.close()


# ------------------------------------------------------------------------------------------------------------ counts
def test_tied_key_point_counts_one_frame():
    """k tied key points of a period-2 frame, k around the 512 key points one pass of k_describe's 128 workgroups holds"""
    fm = _handle(R.W, R.H)
    for k in R.TIED_COUNTS:
        img, lists = R.case_tied(k)
        ref = _run(fm, [img], [lists], label="tied %d" % k)[0]
        assert len(ref.kp) == k
    fm.close()


def test_tied_key_point_counts_eight_frames():
    """one call of eight frames (the lists then live in the primary regions, k_describe runs 8 workgroups per frame)"""
    fm = _handle(R.W, R.H)
    cases = [R.case_tied(k) for k in R.BATCH_COUNTS]
    refs = _run(fm, [c[0] for c in cases], [c[1] for c in cases], label="tied batch")
    assert [len(r.kp) for r in refs] == list(R.BATCH_COUNTS)
    fm.close()


def test_distinct_patch_counts_one_frame():
    """the same counts with equal responses but 2048 different patches (tied key points of a period-2 frame all see one
    patch, so a prefetched patch that lands on the wrong key point would not show there)"""
    fm = _handle(R.LATTICE_W, R.LATTICE_H)
    for k in R.TIED_COUNTS:
        img, lists = R.case_lattice(k)
        ref = _run(fm, [img], [lists], label="lattice %d" % k)[0]
        assert len(ref.kp) == k
    fm.close()


def test_distinct_patch_counts_eight_frames():
    fm = _handle(R.LATTICE_W, R.LATTICE_H)
    cases = [R.case_lattice(k) for k in R.BATCH_COUNTS]
    refs = _run(fm, [c[0] for c in cases], [c[1] for c in cases], label="lattice batch")
    assert [len(r.kp) for r in refs] == list(R.BATCH_COUNTS)
    fm.close()


def test_one_key_point_too_many():
    """2049 tied key points: the slot is refused by a match call and its neighbours' rows are untouched"""
    fm = _handle(R.W, R.H)
    img, lists = R.case_tied(2049)
    ref = _run(fm, [img], [lists], label="tied 2049")[0]
    assert ref.overflow
    fm.close()


# ------------------------------------------------------------------------------------------------------------ selection
def test_lists_around_both_cuts():
    """per level n = N, N + 1, 2 N, 2 N + 1 with random scores; a level with N candidates beside empty levels; scores
    and responses tied exactly at both cuts -- six frames in one call"""
    img = R.noise_image(R.W, R.H)
    lv = _levels(img)
    frames = R.selection_lists(lv, np.random.default_rng(31))
    alone = [R._empty(), R._empty(), R.random_list(lv.rect(2), lv.quotas[2], np.random.default_rng(32))]
    tie_img, tie_lists = R.case_cut_ties()
    fm = _handle(R.W, R.H)
    refs = _run(fm, [img] * 5 + [tie_img], frames + [alone, tie_lists], label="cuts")
    assert len(refs[4].kp) == lv.quotas[2] and len(refs[5].kp) == lv.quotas[0] + 1
    fm.close()


def test_long_lists():
    """equal scores, so that stage 1 keeps the whole list: 4096 and 4097 responses (the staged and the unstaged counting
    loop of k_select), 8192 (kS1Cap exactly) and 8193 (flagged)"""
    fm = _handle(R.BIG_W, R.BIG_H)
    cases = [R.case_equal_scores(n) for n in (4096, 4097, 8192, 8193)]
    refs = _run(fm, [c[0] for c in cases], [c[1] for c in cases], label="long")
    assert [r.overflow for r in refs] == [False, False, False, True]
    assert [r.n_s1[0] for r in refs] == [4096, 4097, 8192, 8193]
    fm.close()


def test_capacities():
    """a count above the list's capacity (clamped and flagged by k_thr_harris), and two levels of 1100 tied key points
    each (k_select truncates at 2048 and flags)"""
    fm = _handle(R.W, R.H)
    cap = 4096
    img = R.noise_image(R.W, R.H)
    over = [R.random_list(R._rect(R.W, R.H), cap + 16, np.random.default_rng(61), scores=33)]
    full = [R.random_list(R._rect(R.W, R.H), cap, np.random.default_rng(62), scores=33)]
    refs = _run(fm, [img, img], [over, full], caps=[cap] * 8, label="capacity")
    assert [r.overflow for r in refs] == [True, False] and refs[1].n_s1[0] == cap
    s_img, s_lists = R.case_sum_overflow()
    refs = _run(fm, [s_img], [s_lists], label="sum")
    assert refs[0].overflow and max(r for r in refs[0].n_s1) == 1100
    fm.close()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_slot_alone():
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import MsfError
    w, h = R.SMALL_SIZES[1]
    img = R.noise_image(w, h)
    lv = _levels(img)
    fm = _handle(w, h)
    d = _device([img])
    good = R.corner_lists(lv)
    fm.orb_tail(d, [good], first_slot=2)
    before = fm.keypoints(2, cache=True).tobytes(), fm.descriptors(2, cache=True).tobytes()
    assert len(before[0]) > 0
    x0, x1, y0, y1 = lv.rect(1)
    assert lv.rect(3) is None

    def at(l, x, y, s=50):
        return [R._empty()] * l + [np.array([[x, y, s]], np.int64)]

    bad = {"x = 30": at(1, x0 - 1, y0), "x = w - 31": at(1, x1 + 1, y0), "y = 30": at(1, x0, y0 - 1),
           "y = h - 31": at(1, x0, y1 + 1), "negative x": at(0, -40, 40), "level without a rectangle": at(3, 31, 31),
           "score 256": at(0, 40, 40, 256), "score -1": at(0, 40, 40, -1),
           "count above capacity + 16": [np.tile(np.array([[40, 40, 50]], np.int64), (4096 + 17, 1))]}
    for what, lists in bad.items():
        with pytest.raises(MsfError) as e:
            fm.orb_tail(d, [lists], first_slot=2)
        assert e.value.code == _lib.MSF_ERR_INVALID_ARG, what
        assert "msf_debug_orb_tail" in str(e.value), what
    counts = np.zeros((1, 8), np.int32)

    def raw(h=fm._h, n=1, frames=d.data_ptr(), row=d.stride(1), slot=2, count0=0, form=0):
        counts[0, 0] = count0
        return fm._L.msf_debug_orb_tail(h, n, frames, d.stride(0), row, slot, counts.ctypes.data, None, form)

    assert raw() == _lib.MSF_OK                                  # an empty frame: the slot now holds no key point
    fm.orb_tail(d, [good], first_slot=2)
    for what, kw in (("negative count", {"count0": -1}), ("form 2", {"form": 2}), ("no frames", {"n": 0}),
                     ("slot range", {"slot": 2 * fm.max_batch_pairs}), ("null frames", {"frames": None}),
                     ("row stride below the width", {"row": 64}), ("misaligned row stride", {"row": d.stride(1) + 4}),
                     ("null handle", {"h": None})):
        assert raw(**kw) == _lib.MSF_ERR_INVALID_ARG, what
    assert (fm.keypoints(2, cache=True).tobytes(), fm.descriptors(2, cache=True).tobytes()) == before
    assert _refused(fm, [2]) == [False]
    fm.orb_tail(d, [good], first_slot=2, form=1)                # and the handle still works
    assert (fm.keypoints(2, cache=True).tobytes(), fm.descriptors(2, cache=True).tobytes()) == before
    fm.close()
