"""GPU: k_describe's patch fetch at the byte address and its row blur on the matrix pipe (csrc/orb_blur_tiles.h), through
FeatureMatcher.orb_tail against tests/orb_tail_ref.py, in all three blur modes, at 76 x 64, 100 x 92 and 192 x 144 with a
level-0 pitch that is not the width.  What tests/test_orb_tail_gpu.py does not reach:

(a) 0 | 255 and 255 | 0 step images, vertical and horizontal, with a key point at every offset of the patch across the
    edge the level's rectangle admits (all 45 at 192 x 144) and every lx mod 4: an operand byte that meets the wrong tap,
    a row or column of a result tile stored in the wrong place, or a sign slip at p - 128 moves the blurred edge;
(b) 0 / 255 stripes of period 1 and 2 by column and by row: neighbouring bytes and rows exchanged;
(c) lx = 31 .. 34 and w - 35 .. w - 32 on every level: the unaligned fetch at both ends of a row;
(d) 0, 1, 31, 32, 33 and 65 key points per frame in calls of one and of eight frames: counts around the kernel's stride.

Every comparison is array equality of the angle bits and the descriptors (and of everything else the tail writes); the
slots next to the call's keep their sentinel -- both by tests.test_orb_tail_gpu._run."""
import numpy as np
import pytest

from tests import orb_tail_ref as R
from tests import test_orb_tail_gpu as T

pytestmark = pytest.mark.gpu

SIZES = ((76, 64), (100, 92), (192, 144))
HALF = 22                                            # the patch reaches 22 rows and 24 | 23 columns from the key point


def _step(w, h, axis, first):
    """0 | 255 (first = 0) or 255 | 0 across the middle of level 0's rectangle -> (image, edge coordinate)"""
    x0, x1, y0, y1 = R._rect(w, h)
    e = (x0 + x1 + 1) // 2 if axis == "x" else (y0 + y1 + 1) // 2
    img = np.full((h, w), first, np.uint8)
    if axis == "x":
        img[:, e:] = 255 - first
    else:
        img[e:, :] = 255 - first
    return img, e


def _across(w, h, axis, e):
    """one key point per offset -22 .. 22 from the edge that the rectangle admits; the other coordinate walks through
    the rectangle, so that every lx mod 4 occurs on both kinds of edge"""
    x0, x1, y0, y1 = R._rect(w, h)
    rows = []
    for i, d in enumerate(range(-HALF, HALF + 1)):
        if axis == "x":
            x, y = e + d, y0 + (7 * i) % (y1 - y0 + 1)
        else:
            x, y = x0 + (5 * i) % (x1 - x0 + 1), e + d
        if x0 <= x <= x1 and y0 <= y <= y1:
            rows.append((x, y, 20 + i))
    return np.array(rows, np.int64)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("size", SIZES)
def test_step_edges_at_every_offset(size, mode):
    w, h = size
    imgs, lists = [], []
    for axis in ("x", "y"):
        for first in (0, 255):
            img, e = _step(w, h, axis, first)
            rows = _across(w, h, axis, e)
            if size == SIZES[-1]:
                assert len(rows) == 2 * HALF + 1
            imgs.append(img)
            lists.append([rows])
    assert all({int(x) & 3 for ls in lists[k:k + 2] for x in ls[0][:, 0]} == {0, 1, 2, 3} for k in (0, 2) if size != SIZES[0])
    assert {int(x) & 3 for ls in lists for x in ls[0][:, 0]} == {0, 1, 2, 3}
    fm = T._handle(w, h, mode)
    refs = T._run(fm, imgs, lists, mode, label="steps %dx%d %s" % (w, h, mode))
    assert [len(r.kp) for r in refs] == [len(ls[0]) for ls in lists]
    # the edge is seen: descriptors differ along the sweep, and the two polarities are not the same frame
    assert len({d.tobytes() for d in refs[0].desc}) > 1 and refs[0].desc.tobytes() != refs[1].desc.tobytes()
    fm.close()


def _stripes(w, h, axis, period):
    v = ((np.arange(w if axis == "x" else h) // period) & 1).astype(np.uint8) * 255
    return np.repeat(v[None, :], h, axis=0) if axis == "x" else np.repeat(v[:, None], w, axis=1)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("size", SIZES)
def test_stripes_of_period_one_and_two(size, mode):
    w, h = size
    imgs = [_stripes(w, h, axis, period) for axis in ("x", "y") for period in (1, 2)]
    rect = R._rect(w, h)
    room = (rect[1] - rect[0] + 1) * (rect[3] - rect[2] + 1)
    lists = [[R.random_list(rect, min(48, room), np.random.default_rng(70 + i))] for i in range(len(imgs))]
    fm = T._handle(w, h, mode)
    refs = T._run(fm, imgs, lists, mode, label="stripes %dx%d %s" % (w, h, mode))
    assert [len(r.kp) for r in refs] == [len(ls[0]) for ls in lists]
    fm.close()


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("size", SIZES)
def test_both_row_ends_on_every_level(size, mode):
    w, h = size
    img = R.noise_image(w, h, seed=8)
    lv = T._levels(img)
    lists = R.corner_lists(lv)
    for l in range(8):
        if lv.rect(l):
            x0, x1 = lv.rect(l)[:2]
            assert lv.images[l].shape[1] == x1 + 32 and x0 == 31
            assert set(range(31, 35)) | set(range(x1 - 3, x1 + 1)) <= {int(x) for x in lists[l][:, 0]}
    fm = T._handle(w, h, mode)
    refs = T._run(fm, [img], [lists], mode, label="row ends %dx%d %s" % (w, h, mode))
    assert len(refs[0].kp) == sum(len(c) for c in lists) > 0
    fm.close()


def test_a_call_of_260_frames():
    """from 256 frames on k_describe runs eight workgroups per frame and hands the frames of a group of eight to the
    workgroups by their position in the grid (a frame per XCD); the last four frames of 260 are no full group.  Four
    different frames in turn, so a workgroup that took another frame's key points or pyramid shows"""
    w, h = SIZES[1]
    rect = R._rect(w, h)
    kinds = [(R.noise_image(w, h, seed=20 + i), [R.random_list(rect, n, np.random.default_rng(30 + i), scores=40)])
             for i, n in enumerate((33, 0, 65, 7))]
    n = 260
    fm = T._handle(w, h, pairs=n // 2 + 1)
    refs = T._run(fm, [kinds[i % 4][0] for i in range(n)], [kinds[(i // 2) % 4][1] for i in range(n)], forms=(1,), label="260 frames")
    assert [len(r.kp) for r in refs[:8]] == [33, 33, 0, 0, 65, 65, 7, 7]
    fm.close()


COUNTS = (0, 1, 31, 32, 33, 65)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("size", SIZES)
def test_counts_around_the_stride(size, mode):
    """every count in a call of its own, then eight frames with these counts in one call; each frame its own noise, so a
    patch that lands on the wrong key point shows.  76 x 64 has 28 positions: its counts stop there"""
    w, h = size
    rect = R._rect(w, h)
    room = (rect[1] - rect[0] + 1) * (rect[3] - rect[2] + 1)
    counts = sorted({min(c, room) for c in COUNTS})
    assert size == SIZES[0] or counts == list(COUNTS)
    frames = []
    for i, n in enumerate(counts + [counts[-1], counts[1]]):
        frames.append((R.noise_image(w, h, seed=90 + i), [R.random_list(rect, n, np.random.default_rng(50 + i), scores=40)]))
    fm = T._handle(w, h, mode)
    for (img, lists), n in zip(frames, counts):
        ref = T._run(fm, [img], [lists], mode, forms=(1,), label="count %d %dx%d %s" % (n, w, h, mode))[0]
        assert len(ref.kp) == n
    batch = (frames * 2)[:8]
    refs = T._run(fm, [f[0] for f in batch], [f[1] for f in batch], mode, forms=(1,), label="count batch %dx%d %s" % (w, h, mode))
    assert [len(r.kp) for r in refs] == [len(f[1][0]) for f in batch]
    fm.close()
