"""GPU: the LoFTR coarse transformer alone (msf_debug_loftr_transformer) against the float64 reference
oracle/loftr_transformer.py, on every encoder path: split-bf16 with paired launches (the default), split-bf16 with one
launch per block (MSF_LOFTR_ATTN_PAIR=0), and exact f32 (MSF_FLAG_LOFTR_F32).

Ranges: each single block 0..7 on the f32-rounded reference state before it (errors do not compound), the paired
ranges (0, 2) and (4, 2), and the whole range [0, 8).  Token families (tests/loftr_tokens.py): KAT tokens, a scale sweep
1/64 .. 64, tokens that drive q and k to -4, -12 and -20 at the block under test, zero tokens, one large-norm token at
index 0 or 1199, and self pairs.

The check that can fail: every entry of every family, the negative ones included, within BAR = 1e-3 of its token's
scale (RMS, at least 1) -- the suite's end-to-end bar.  tests/test_loftr_transformer_ref.py shows that each reference
mutant moves some family past that bar.  Each entry is also held to the reference's derived bound, but that bound is a
worst case through six weight products and two LayerNorms: on the KAT tokens it reaches ~0.26 (f32) and ~17 (split) per
block, and in the eps-dominated negative families it is not finite, so it is reported (largest error-to-bound ratio and
the count of undetermined entries), not relied on.  Each path prints its measured error per family."""
import numpy as np
import pytest

from oracle import loftr_transformer as T
from tests import loftr_tokens as TK

pytestmark = pytest.mark.gpu

BAR = 1e-3
PATHS = {"split": (0, {}), "split_unpaired": (0, {"MSF_LOFTR_ATTN_PAIR": "0"}), "f32": ("f32", {})}


def _handle(monkeypatch, pairs, path):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    flags, env = PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = _lib.MSF_FLAG_KEEP_DEBUG | _lib.MSF_FLAG_NO_FRAME_CACHE | (_lib.MSF_FLAG_LOFTR_F32 if flags == "f32" else 0)
    dm = DNNFeatureMatcher(threshold=0.15, max_batch_pairs=pairs, flags=f)
    for k in env:
        monkeypatch.delenv(k)
    return dm


def _run(dm, A0, A1, first, n):
    import torch
    d0 = torch.from_numpy(np.ascontiguousarray(np.stack(A0), np.float32)).cuda()
    d1 = torch.from_numpy(np.ascontiguousarray(np.stack(A1), np.float32)).cuda()
    o0 = torch.full_like(d0, float("nan"))
    o1 = torch.full_like(d1, float("nan"))
    dm.transformer_device(d0, d1, o0, o1, first, n)
    return o0.cpu().numpy(), o1.cpu().numpy()


class _Case:
    """one pair on one range: f32 inputs, the reference outputs and their bounds"""
    def __init__(self, fam, name, first, n, in0, in1):
        self.fam, self.name, self.first, self.n, self.in0, self.in1 = fam, name, first, n, in0, in1
        self.out0, self.out1, self.E0, self.E1 = T.run(in0, in1, first, n)


_CASES = None


def _cases():
    """{(first, n): [_Case]}, computed once per module"""
    global _CASES
    if _CASES is None:
        _CASES = {r: [] for r in TK.RANGES}
        for c in TK.cases():
            _CASES[(c[2], c[3])].append(_Case(*c))
    return _CASES


def _check(case, g0, g1, unit, stats):
    """every updated entry within BAR of its scale and within the derived bound; the sequence no block of the range
    updates is copied through bit for bit"""
    updated = {bi % 2 for bi in range(case.first, case.first + case.n)}
    for side, got, ref, E, inp in ((0, g0, case.out0, case.E0[unit], case.in0), (1, g1, case.out1, case.E1[unit], case.in1)):
        tag = "%s/%s [%d, %d) side %d" % (case.fam, case.name, case.first, case.first + case.n, side)
        assert np.isfinite(got).all(), tag
        if side not in updated:
            assert np.array_equal(got, inp), tag
            continue
        err = np.abs(got.astype(np.float64) - ref)
        rel = err / TK.scale_of(ref)
        assert rel.max() <= BAR, (tag, float(rel.max()), float(err.max()))
        bad = err > E
        assert not bad.any(), (tag, int(bad.sum()), float(err[bad].max()), float(E[bad].min()))
        st = stats.setdefault(case.fam, {"err": 0.0, "rel": 0.0, "ratio": 0.0, "undetermined": 0, "entries": 0})
        st["err"] = max(st["err"], float(err.max()))
        st["rel"] = max(st["rel"], float(rel.max()))
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.isfinite(E) & (E > 0), err / E, 0.0)
        st["ratio"] = max(st["ratio"], float(ratio.max()))
        st["undetermined"] += int(T.undetermined(ref, E).sum())
        st["entries"] += err.size


@pytest.mark.parametrize("path", list(PATHS))
def test_blocks_match_the_float64_reference(monkeypatch, path):
    cases = _cases()
    unit = "f32" if path == "f32" else "split"
    dm = _handle(monkeypatch, 24, path)
    stats = {}
    for (first, n), cs in cases.items():
        assert len(cs) <= 24
        g0, g1 = _run(dm, [c.in0 for c in cs], [c.in1 for c in cs], first, n)
        for k, c in enumerate(cs):
            _check(c, g0[k], g1[k], unit, stats)
    print("\n[%s, %s bound] per family over all ranges:" % (path, unit))
    for fam, st in stats.items():
        print("  %-9s max |err| %.3g, max err/scale %.3g (bar %g), max err/bound %.3g, undetermined %d of %d" % (
            fam, st["err"], st["rel"], BAR, st["ratio"], st["undetermined"], st["entries"]))


def test_saturated_message_is_exactly_zero(monkeypatch):
    """-20 family at the cross blocks: K is exactly 0 for every source token, so the message is exactly 0 and the merged
    value exactly n1b whatever V is.  Observed on the GPU: scaling the source by 1.5 and 3 (k stays saturated, V
    changes) leaves the updated sequence bit-identical, on both paths."""
    W = T.weights()
    for path in ("split", "f32"):
        dm = _handle(monkeypatch, 1, path)
        for bi in (2, 3, 6, 7):
            a = list(TK.negative(bi, -20))
            me = bi % 2
            _, _, inter = T.block(a[me], a[1 - me], W[bi])
            assert np.all(inter["K"] == 0) and np.all(inter["msg"] == 0) and np.all(inter["merged"] == W[bi]["n1b"])
            base = _run(dm, [a[0]], [a[1]], bi, 1)[me][0]
            for k in (1.5, 3.0):
                b = list(a)
                b[1 - me] = (a[1 - me] * np.float32(k)).astype(np.float32)
                _, _, ib = T.block(b[me], b[1 - me], W[bi])
                assert np.all(ib["K"] == 0) and not np.allclose(b[1 - me] @ W[bi]["wv"], a[1 - me] @ W[bi]["wv"])
                got = _run(dm, [b[0]], [b[1]], bi, 1)[me][0]
                assert np.array_equal(got, base), (path, bi, k)


@pytest.mark.parametrize("path", list(PATHS))
def test_a_pair_does_not_depend_on_its_batch(monkeypatch, path):
    """n_pairs 1, 3 and 8 on handles of max_batch_pairs 8 and 24: every pair bit-identical to the same pair alone, at
    any batch position, on the whole range and on the paired range (4, 2)"""
    fams = TK.families()
    pool = [(t0, t1) for fam in ("kat", "large", "zero", "self") for _, t0, t1 in fams[fam]][:8]
    assert len(pool) == 8
    for first, n in ((0, 8), (4, 2)):
        for mb in (8, 24):
            dm = _handle(monkeypatch, mb, path)
            alone = [_run(dm, [a], [b], first, n) for a, b in pool]
            for order in ([5, 0, 2], [7, 6, 5, 4, 3, 2, 1, 0]):
                g0, g1 = _run(dm, [pool[p][0] for p in order], [pool[p][1] for p in order], first, n)
                for k, p in enumerate(order):
                    assert np.array_equal(g0[k], alone[p][0][0]), (path, first, n, mb, order, k)
                    assert np.array_equal(g1[k], alone[p][1][0]), (path, first, n, mb, order, k)


def test_paired_launch_equals_one_launch_per_block(monkeypatch):
    """the ranges that pair blocks (0, 2), (4, 2), [0, 8), and ranges that cannot pair (1, 2), (3, 3), bit for bit"""
    fams = TK.families()
    A0 = [t0 for fam in ("kat", "scale") for _, t0, _ in fams[fam]]
    A1 = [t1 for fam in ("kat", "scale") for _, _, t1 in fams[fam]]
    for first, n in ((0, 2), (4, 2), (0, 8), (1, 2), (3, 3)):
        a = _run(_handle(monkeypatch, 8, "split"), A0, A1, first, n)
        b = _run(_handle(monkeypatch, 8, "split_unpaired"), A0, A1, first, n)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (first, n)


def test_entry_is_bit_identical_to_match(monkeypatch):
    """Fidelity: the tokens match() kept (backbone_tokens), fed through transformer_device, give coarse_features() bit
    for bit -- split and f32 handles, a single pair and pair 0 of an 8-pair batch"""
    G = TK.GOLD
    frames = [(G["img0_" + k], G["img1_" + k]) for k in TK.KATS]
    for path in ("split", "f32"):
        for n in (1, 8):
            dm = _handle(monkeypatch, n, path)
            if n == 1:
                dm.MatchFrames(*frames[1], cap=8192)
            else:
                dm.match_batch([frames[p % 4][0] for p in range(1, 9)], [frames[p % 4][1] for p in range(1, 9)], cap=8192)
            tok = dm.backbone_tokens().copy()
            feat = dm.coarse_features().copy()
            g0, g1 = _run(dm, [tok[0]], [tok[1]], 0, 8)
            assert np.array_equal(g0[0], feat[0]) and np.array_equal(g1[0], feat[1]), (path, n)
            print("\n[fidelity %s n=%d] transformer_device(backbone_tokens) == coarse_features bit for bit" % (path, n))


def test_backbone_tokens_match_the_graph(monkeypatch):
    """the first direct check of the backbone against the graph: KAT ii against the ONNX tokens, the other KATs against
    the C restatement's, within the end-to-end bar"""
    G = TK.GOLD
    for path in ("split", "f32"):
        dm = _handle(monkeypatch, 1, path)
        worst = {}
        for k in TK.KATS:
            dm.MatchFrames(G["img0_" + k], G["img1_" + k], cap=8192)
            tok = dm.backbone_tokens()
            ref = TK.kat_tokens(k)
            worst[k] = max(float(np.abs(tok[0] - ref[0]).max()), float(np.abs(tok[1] - ref[1]).max()))
        print("\n[tokens %s] max |gpu - graph| %s" % (path, {k: "%.2e" % v for k, v in worst.items()}))
        assert max(worst.values()) <= BAR, (path, worst)


def test_entry_rejects_bad_arguments(monkeypatch):
    import torch
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher, MsfError
    dm = _handle(monkeypatch, 2, "split")
    f = torch.zeros((3, 1200, 32), dtype=torch.float32, device="cuda")
    with pytest.raises(MsfError) as e:                   # n_pairs > max_batch_pairs
        dm.transformer_device(f, f, f.clone(), f.clone())
    assert e.value.code == _lib.MSF_ERR_INVALID_ARG
    L, h = dm._L, dm._h
    p = f.data_ptr()
    for n, first, nb in ((-1, 0, 8), (1, -1, 2), (1, 0, 0), (1, 7, 2), (1, 8, 1), (1, 0, 9)):
        assert L.msf_debug_loftr_transformer(h, n, first, nb, p, p, p, p, None) == _lib.MSF_ERR_INVALID_ARG, (n, first, nb)
    fb = torch.zeros((2 * 1200 * 32 + 4,), dtype=torch.float32, device="cuda")
    q = fb.data_ptr() + 4
    for args in ((q, p, p, p), (p, q, p, p), (p, p, q, p), (p, p, p, q)):
        assert L.msf_debug_loftr_transformer(h, 1, 0, 8, *args, None) == _lib.MSF_ERR_INVALID_ARG   # not 16-byte aligned
    assert L.msf_debug_loftr_transformer(h, 0, 0, 8, p, p, p, p, None) == _lib.MSF_OK
    orb = FeatureMatcher()
    assert L.msf_debug_loftr_transformer(orb._h, 1, 0, 8, p, p, p, p, None) == _lib.MSF_ERR_INVALID_ARG   # not LoFTR
    # the entry is not a match call: the stage-timing ring stays empty
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    prof = DNNFeatureMatcher(threshold=0.15, max_batch_pairs=2, flags=_lib.MSF_FLAG_PROFILE | _lib.MSF_FLAG_NO_FRAME_CACHE)
    g = f[:2].contiguous()
    prof.transformer_device(g, g, g.clone(), g.clone())
    assert prof.stage_times() == {}
