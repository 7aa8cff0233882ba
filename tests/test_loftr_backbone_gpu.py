"""GPU: the LoFTR ResNet backbone alone (msf_debug_loftr_backbone) against the float64 reference
oracle/loftr_backbone.py, on every path run_backbone can take (PATHS: the switches and the kernels each pins).

Frames (tests/loftr_frames.py, all 640 x 480): a synth textured frame, KAT ii img0, uniform noise, the 1-px checkerboard,
all white, a grid of 3-px white lines on every 128th column and 64th row (the strip, tile and band edges of every
backbone kernel) with a white two-pixel rim, and four 8 x 8 white corner blocks.

The check that can fail: every entry of all four layer activations and of the tokens, of every image of an extract-form
call (7 frames) and of a match-form call (3 A + 3 B frames, grid and noise among the B frames), within BAR = 1e-3 of
its scale -- the RMS over the channels of that pixel or token, at least 1: the suite's end-to-end bar in the form
tests/test_loftr_transformer_gpu.py uses.  tests/test_loftr_backbone_ref.py shows that each reference mutant (strip
seams, missing last rows, a wrong residual, shortcut phase, input scale, image index, ignored stride, lost split terms)
moves some entry past that bar.

Measured on an MI355X, largest error over scale (bar 1e-3) per layer and frame family, over both forms; the largest
|error| of a row in brackets.  banded_tail2 equals banded and f32_unfused equals f32 in every digit.

  strip          synth    kat_ii   noise    checker  white    grid     corners
    layer1       6.2e-05  7.5e-05  7.1e-05  3.5e-05  2.7e-05  3.5e-05  2.2e-05   (2.9e-04)
    layer2       1.0e-04  1.1e-04  7.0e-05  8.6e-05  7.7e-05  4.5e-05  4.6e-05   (1.8e-04)
    layer3       6.7e-05  6.7e-05  3.5e-05  7.0e-05  6.2e-05  3.7e-05  4.1e-05   (1.9e-04)
    layer4       2.6e-05  1.9e-05  2.8e-05  4.9e-05  5.2e-05  2.6e-05  3.3e-05   (6.9e-05)
    tokens       7.6e-05  7.5e-05  4.9e-05  1.4e-04  1.3e-04  6.4e-05  8.4e-05   (1.8e-04)
  banded
    layer1       5.0e-05  4.5e-05  5.2e-05  2.2e-05  1.8e-05  2.2e-05  1.9e-05   (1.7e-04)
    layer2       4.1e-05  5.4e-05  2.2e-05  2.8e-05  5.3e-05  2.8e-05  2.7e-05   (9.7e-05)
    layer3       3.3e-05  2.7e-05  2.1e-05  4.5e-05  4.8e-05  2.2e-05  2.3e-05   (1.1e-04)
    layer4       1.6e-05  1.6e-05  2.0e-05  2.5e-05  3.8e-05  1.9e-05  2.5e-05   (4.9e-05)
    tokens       5.4e-05  5.3e-05  3.6e-05  5.8e-05  1.0e-04  4.9e-05  6.9e-05   (1.2e-04)
  f32
    layer1       2.6e-06  2.4e-06  2.5e-06  8.8e-07  5.5e-07  1.1e-06  8.7e-07   (9.1e-06)
    layer2       3.1e-06  3.6e-06  1.9e-06  1.9e-06  2.0e-06  1.6e-06  2.1e-06   (5.1e-06)
    layer3       2.0e-06  2.5e-06  2.4e-06  1.7e-06  2.3e-06  1.9e-06  2.3e-06   (8.6e-06)
    layer4       1.6e-06  1.8e-06  1.8e-06  2.0e-06  3.0e-06  1.3e-06  1.7e-06   (3.8e-06)
    tokens       4.0e-06  5.0e-06  3.2e-06  3.8e-06  6.7e-06  4.1e-06  4.4e-06   (8.1e-06)
  strip_unfused  (layers 1 and 2 are f32's: k_conv)
    layer3       2.1e-05  2.8e-05  1.9e-05  1.8e-05  1.5e-05  1.8e-05  1.8e-05   (6.9e-05)
    layer4       1.5e-05  1.7e-05  1.7e-05  2.0e-05  1.8e-05  1.5e-05  2.2e-05   (3.1e-05)
    tokens       5.3e-05  3.6e-05  3.3e-05  5.6e-05  7.7e-05  5.3e-05  7.9e-05   (8.7e-05)

Every split path is at least 7 times inside the bar on every family, noise, checkerboard, white and grid included, so no
family is dropped or dimmed on any layer.

What these tests found: asked for the streaming kernels, MSF_LOFTR_UNFUSED=1 without MSF_LOFTR_F32 gave layer 3 values
of 1e36 (k_strip32x read f32 NCHW as split pixels), and MSF_LOFTR_DOWN=0 gave layer 2 errors of 2.4 .. 8.2 over scale
(k_conv read k_strip8x's split pixels as f32).  run_backbone now runs the streaming kernels all or none (the
strip_unfused path above), and MSF_LOFTR_DOWN is gone."""
import numpy as np
import pytest

from tests import loftr_frames as FR

pytestmark = pytest.mark.gpu

BAR = 1e-3
# name -> (MSF_FLAG_LOFTR_F32, switches read at msf_create): the kernels it pins
PATHS = {
    "strip": (False, {"MSF_LOFTR_STRIP_MIN": "1"}),          # the six streaming kernels, k_convx2<32>, k_convx, k_out_tokens
    "banded": (False, {}),                                   # k_conv stem / down16, k_block8x, k_block16x, k_convx2<16>, k_convx
    "banded_tail2": (False, {"MSF_LOFTR_OUT_FUSED": "0"}),   # k_conv<32, 32, 1, 1> + k_tokens across the nA / nB split
    "f32": (True, {}),                                       # k_conv, k_block8, k_block16
    "f32_unfused": (True, {"MSF_LOFTR_UNFUSED": "1"}),       # k_conv for every convolution
    "strip_unfused": (False, {"MSF_LOFTR_STRIP_MIN": "1", "MSF_LOFTR_UNFUSED": "1"}),   # strips asked for, blocks unfused
}
LAYERS = ("layer1", "layer2", "layer3", "layer4", "tokens")
MATCH_A, MATCH_B = [0, 1, 6], [5, 2, 3]      # synth, kat_ii, corners + grid, noise, checker


def _handle(monkeypatch, pairs, path):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    f32, env = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = _lib.MSF_FLAG_KEEP_DEBUG | _lib.MSF_FLAG_NO_FRAME_CACHE | (_lib.MSF_FLAG_LOFTR_F32 if f32 else 0)
    dm = DNNFeatureMatcher(threshold=0.15, max_batch_pairs=pairs, flags=f)
    for k in env:
        monkeypatch.delenv(k)
    return dm


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _run(dm, d_a, d_b, act_image=0, layers=(), **kw):
    """one call of the entry -> (tokens of the pass [nA + nB][1200][32], {layer: activation of act_image})"""
    import torch
    n = kw.get("n", d_a.shape[0])
    ta = torch.full((n, 1200, 32), float("nan"), dtype=torch.float32, device="cuda")
    tb = torch.full((n, 1200, 32), float("nan"), dtype=torch.float32, device="cuda") if d_b is not None else None
    dm.backbone_device(d_a, d_b, ta, tb, act_image=act_image, **kw)
    tok = ta.cpu().numpy() if tb is None else np.concatenate([ta.cpu().numpy(), tb.cpu().numpy()])
    return tok, {l: dm.backbone_activation(l) for l in layers}


def _worst(err, rel):
    i = np.unravel_index(int(np.argmax(rel)), rel.shape)
    return float(rel[i]), float(err[i]), tuple(int(k) for k in i)


@pytest.mark.parametrize("path", list(PATHS))
def test_layers_and_tokens_match_the_float64_reference(monkeypatch, path):
    """every image of both forms, selected with act_image: four layers and the tokens, entry by entry"""
    fr, ref = FR.frames(), FR.reference()
    dm = _handle(monkeypatch, 7, path)
    d_all = _dev(fr)
    forms = [("extract", d_all, None, list(range(7))),
             ("match", _dev(fr[MATCH_A]), _dev(fr[MATCH_B]), MATCH_A + MATCH_B)]
    stats, failures = {}, []
    for form, d_a, d_b, ids in forms:
        for k, i in enumerate(ids):
            tok, act = _run(dm, d_a, d_b, act_image=k, layers=range(4))
            fam = FR.NAMES[i]
            for l in range(5):
                got = act[l] if l < 4 else tok[k]
                want = ref["act"][l][i] if l < 4 else ref["tok"][i]
                tag = "%s %s image %d (%s) %s" % (path, form, k, fam, LAYERS[l])
                assert got.shape == want.shape and np.isfinite(got).all(), tag
                err, rel = FR.errors(got, want, 0 if l < 4 else 1)
                w = _worst(err, rel)
                st = stats.setdefault((LAYERS[l], fam), [0.0, 0.0])
                st[0], st[1] = max(st[0], float(err.max())), max(st[1], w[0])
                if w[0] > BAR:
                    failures.append((tag, "err/scale %.3g, |err| %.3g at %s (c, y, x | token, c), %d entries past the bar"
                                     % (w[0], w[1], w[2], int((rel > BAR).sum()))))
            if form == "match" or k == 0:
                # the tokens of every image of the pass, whichever image's activations were kept
                for kk, ii in enumerate(ids):
                    _, rel = FR.errors(tok[kk], ref["tok"][ii], 1)
                    if rel.max() > BAR:
                        failures.append(("%s %s act_image %d: tokens of image %d" % (path, form, k, kk), float(rel.max())))
    print("\n[%s] largest |err| / largest err over scale (bar %g), per layer and frame family:" % (path, BAR))
    print("  %-7s %s" % ("", " ".join("%19s" % n for n in FR.NAMES)))
    for L in LAYERS:
        print("  %-7s %s" % (L, " ".join("%9.2e /%8.2e" % tuple(stats[(L, n)]) for n in FR.NAMES)))
    assert not failures, failures[:12]


@pytest.mark.parametrize("path", ["strip", "banded", "f32"])
def test_an_image_does_not_depend_on_its_batch(monkeypatch, path):
    """tokens and the layer-4 activation of every image of n = 1, 3 and 7, extract and match forms, forward and reversed
    order: bit-identical to the same image alone"""
    fr = FR.frames()
    dm = _handle(monkeypatch, 7, path)
    alone = []
    for i in range(7):
        tok, act = _run(dm, _dev(fr[[i]]), None, 0, layers=(3,))
        alone.append((tok[0], act[3]))
    for n in (1, 3, 7):
        fwd, rev = list(range(7))[:n], list(range(7))[::-1][:n]
        for a, b in ((fwd, None), (rev, None), (fwd, rev)):
            ids = a + (b or [])
            d_a, d_b = _dev(fr[a]), (None if b is None else _dev(fr[b]))
            for k, i in enumerate(ids):
                tok, act = _run(dm, d_a, d_b, k, layers=(3,))
                assert np.array_equal(act[3], alone[i][1]), (path, n, a, b, k)
                for kk, ii in enumerate(ids):
                    assert np.array_equal(tok[kk], alone[ii][0]), (path, n, a, b, k, kk)


@pytest.mark.parametrize("path", ["strip", "banded"])
def test_strides_and_padding_bytes_are_ignored(monkeypatch, path):
    """row_stride 704 and a frame_stride of one row more than 480 rows, the padding 255 on one run and 0 on the other:
    tokens bit-identical to those of dense frames, in both forms"""
    fr = FR.frames()
    dm = _handle(monkeypatch, 7, path)
    dense, _ = _run(dm, _dev(fr), None)
    dense_m, _ = _run(dm, _dev(fr[MATCH_A]), _dev(fr[MATCH_B]))
    rs, fs = 704, 704 * 481
    for fill in (255, 0):
        tok, _ = _run(dm, _dev(FR.padded(fr, rs, 1, fill)), None, n=7, row_stride=rs, frame_stride=fs)
        assert np.array_equal(tok, dense), (path, fill)
        tok, _ = _run(dm, _dev(FR.padded(fr[MATCH_A], rs, 1, fill)), _dev(FR.padded(fr[MATCH_B], rs, 1, fill)), n=3,
                      row_stride=rs, frame_stride=fs)
        assert np.array_equal(tok, dense_m), (path, fill)


def test_the_64_image_rule(monkeypatch):
    """a default handle: a pass of 64 images takes the streaming kernels (tokens bit-identical to the `strip` handle's for
    every image, 0, 37 and 63 among them), one of 63 the banded ones (bit-identical to the `banded` handle's); the same
    at 32 + 32 and 31 + 31 in the match form.  The two sets of kernels differ in bits, so the rule is visible."""
    fr = FR.frames()
    seven = {p: _run(_handle(monkeypatch, 7, p), _dev(fr), None)[0] for p in ("strip", "banded")}
    assert not np.array_equal(seven["strip"], seven["banded"])
    dm = _handle(monkeypatch, 64, "banded")              # no switches: the default rule
    ids = [i % 7 for i in range(64)]
    d = _dev(fr[ids])
    for n, path in ((64, "strip"), (63, "banded")):
        tok, _ = _run(dm, d[:n], None)
        for k in range(n):
            assert np.array_equal(tok[k], seven[path][ids[k]]), (n, path, k)
    for n, path in ((32, "strip"), (31, "banded")):
        tok, _ = _run(dm, d[:n], d[32:32 + n])
        for k in range(2 * n):
            assert np.array_equal(tok[k], seven[path][ids[k] if k < n else ids[32 + k - n]]), (n, path, k)


def test_entry_is_bit_identical_to_match(monkeypatch):
    """after MatchFrames and after an 8-pair match_batch, backbone_tokens() (pair 0 of the match call) equals the entry's
    tokens for pair 0 of the same frames, on split and f32 handles; the activations kept are those of image 0 either way"""
    fr = FR.frames()
    A = [fr[i % 7] for i in range(8)]
    Bf = [fr[(i + 3) % 7] for i in range(8)]
    for path in ("banded", "f32"):
        for n in (1, 8):
            dm = _handle(monkeypatch, n, path)
            if n == 1:
                dm.MatchFrames(A[0], Bf[0], cap=8192)
            else:
                dm.match_batch(A, Bf, cap=8192)
            want = dm.backbone_tokens().copy()
            want_act = [dm.backbone_activation(l).copy() for l in range(4)]
            tok, act = _run(dm, _dev(np.stack(A[:n])), _dev(np.stack(Bf[:n])), 0, layers=range(4))
            assert np.array_equal(tok[0], want[0]) and np.array_equal(tok[n], want[1]), (path, n)
            for l in range(4):
                assert np.array_equal(act[l], want_act[l]), (path, n, l)


def test_entry_rejects_bad_arguments(monkeypatch):
    import torch
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher, FeatureMatcher
    INV = _lib.MSF_ERR_INVALID_ARG
    dm = _handle(monkeypatch, 2, "banded")
    L, h = dm._L, dm._h
    d = torch.zeros((3, 480, 640), dtype=torch.uint8, device="cuda")
    t = torch.zeros((3, 1200, 32), dtype=torch.float32, device="cuda")
    p, q, fs = d.data_ptr(), t.data_ptr(), 640 * 480
    err = lambda: L.msf_last_error(h).decode()                                                   # noqa: E731
    for n, act in ((-1, 0), (3, 0), (1, -1), (1, 2), (2, 4)):      # n < 0, n above the chunk, act_image out of range
        assert L.msf_debug_loftr_backbone(h, n, p, p, fs, 640, act, q, q, None) == INV, (n, act)
        assert err() == "msf_debug_loftr_backbone: bad argument"
    assert L.msf_debug_loftr_backbone(h, 1, p, None, fs, 640, 1, q, None, None) == INV          # extract form: one image
    assert L.msf_debug_loftr_backbone(h, 1, None, p, fs, 640, 0, q, q, None) == INV
    assert L.msf_debug_loftr_backbone(h, 1, p, p, fs, 640, 0, q, None, None) == INV             # B frames without tokens
    for args in ((p + 4, p, fs, 640, 0, q, q), (p, p + 8, fs, 640, 0, q, q), (p, p, fs, 640, 0, q + 4, q),
                 (p, p, fs, 640, 0, q, q + 8), (p, p, fs + 8, 648, 0, q, q), (p, p, fs + 8, 640, 0, q, q)):
        assert L.msf_debug_loftr_backbone(h, 1, *args, None) == INV, args
        assert err() == "msf_debug_loftr_backbone: misaligned pointer"
    assert L.msf_debug_loftr_backbone(h, 1, p, p, fs, 624, 0, q, q, None) == INV
    assert err() == "row_stride < image_width"
    assert L.msf_debug_loftr_backbone(h, 1, p, p, fs - 16, 640, 0, q, q, None) == INV
    assert err() == "frame_stride < row_stride * image_height (frames would overlap)"
    assert L.msf_debug_loftr_backbone(h, 0, p, p, fs, 640, 0, q, q, None) == _lib.MSF_OK
    assert L.msf_debug_loftr_backbone(h, 2, p, p, fs, 640, 3, q, q, None) == _lib.MSF_OK         # and the call after
    orb = FeatureMatcher()
    assert L.msf_debug_loftr_backbone(orb._h, 1, p, p, fs, 640, 0, q, q, None) == INV
    assert L.msf_last_error(orb._h).decode() == "msf_debug_loftr_backbone: not a LoFTR handle"
    # tokens need no MSF_FLAG_KEEP_DEBUG, and the entry is not a match call: the stage-timing ring stays empty
    prof = DNNFeatureMatcher(threshold=0.15, max_batch_pairs=2, flags=_lib.MSF_FLAG_PROFILE | _lib.MSF_FLAG_NO_FRAME_CACHE)
    tok, _ = _run(prof, d[:2], d[:2])
    assert np.isfinite(tok).all() and prof.stage_times() == {}
    with pytest.raises(Exception):
        prof.backbone_activation(0)
