"""CPU: pins the float64 transformer reference (oracle/loftr_transformer.py) that tests/test_loftr_transformer_gpu.py
holds the GPU encoder blocks to: to the ONNX graph (golden pre- and post-transformer tokens of KAT ii), to the C
restatement (oracle/loftr_oracle.c), and checks that each token family reaches its regime and that changes to the
reference that stand for kernel bugs are visible to the GPU checks."""
import numpy as np
import pytest

from oracle import loftr_transformer as T
from tests import loftr_tokens as TK

ONNX_BAR = 1e-4
BAR = 1e-3          # the GPU tests' bar for the sharp families (1e-3 of the token's scale, at least 1)


def test_reference_reproduces_the_onnx_graph():
    """golden tok*_ii -> feat*_ii: measured gap 2.0e-6, held to 1e-4"""
    G = TK.GOLD
    s0, s1, _, _ = T.run(G["tok0_ii"], G["tok1_ii"])
    gap = max(np.abs(s0 - G["feat0_ii"]).max(), np.abs(s1 - G["feat1_ii"]).max())
    print("\nONNX gap %.2e" % gap)
    assert gap <= ONNX_BAR


@pytest.mark.parametrize("name", ["i", "ii", "iii", "synth", "synth_pair"])
def test_reference_reproduces_the_c_restatement(name):
    from oracle import loftr
    if name == "synth_pair":
        from mono_slam_framework_amd import synth
        a, b = synth.synth_pair(3, 640, 480, mode=1)
    else:
        a, b = TK.GOLD["img0_" + name], TK.GOLD["img1_" + name]
    r = loftr.DNNFeatureMatcherOracle(0.15).run(a, b)
    s0, s1, _, _ = T.run(r["tok"][0], r["tok"][1])
    gap = max(np.abs(s0 - r["feat0"]).max(), np.abs(s1 - r["feat1"]).max())
    print("\n[%s] |ref - C| %.2e" % (name, gap))
    assert gap <= ONNX_BAR


def test_block_follows_the_block_table():
    """run(first, n) composes: [0, 3) then [3, 5) equals [0, 5); a range leaves the sequence it does not update alone"""
    t0, t1 = TK.kat_tokens("ii")
    a0, a1, _, _ = T.run(t0, t1, 0, 5)
    b0, b1, _, _ = T.run(t0, t1, 0, 3)
    c0, c1, _, _ = T.run(b0, b1, 3, 2)
    assert np.array_equal(a0, c0) and np.array_equal(a1, c1)
    d0, d1, _, _ = T.run(t0, t1, 0, 1)
    assert np.array_equal(d1, np.asarray(t1, np.float64)) and not np.array_equal(d0, np.asarray(t0, np.float64))


def test_kat_bounds_are_finite_per_block():
    """On the KAT tokens every single-block bound is finite; the largest per unit is printed.  The issue's target, bounds
    ten times tighter than 1e-3, is not met: the bound is a worst case through six weight products and two LayerNorms
    (about 0.26 for f32 and 17 for split per block), so the GPU tests hold every family to the 1e-3 bar instead and
    only report the bound."""
    worst = {u: 0.0 for u in T.UNITS}
    for name in TK.KATS:
        t0, t1 = TK.kat_tokens(name)
        s = [np.asarray(t0, np.float32), np.asarray(t1, np.float32)]
        for bi in range(8):
            o0, o1, E0, E1 = T.run(s[0], s[1], bi, 1)
            for u in T.UNITS:
                E = (E0, E1)[bi % 2][u]
                assert np.isfinite(E).all(), (name, bi, u)
                worst[u] = max(worst[u], float(E.max()))
            s = [o0.astype(np.float32), o1.astype(np.float32)]
    print("\nlargest single-block bound on the KAT tokens: %s" % {u: "%.3g" % v for u, v in worst.items()})


def test_families_reach_their_regimes():
    W = T.weights()
    fams = TK.families()
    # scale sweep: the x64 KV sums are 64^2 x the plain ones' (Ksum over 1200 tokens of K ~ 64 |k|)
    t0, t1 = TK.kat_tokens("ii")
    _, _, base = T.block(t0, t0, W[0])
    big = [f for f in fams["scale"] if f[0] == "x64"][0]
    _, _, inter = T.block(big[1], big[1], W[0])
    assert inter["Ksum"].max() > 30 * base["Ksum"].max()
    # zero tokens: zero variance at LayerNorm 1, whose output is its bias exactly
    z = fams["zero"][0][1]
    _, _, inter = T.block(z, z, W[0])
    assert np.all(inter["msg"] == 0) and np.all(inter["merged"] == W[0]["n1b"])
    assert np.all(inter["sigma1"] == np.sqrt(T.LN_EPS))
    # one large token: 50 x the largest other norm, its k far outside the others' range
    for name, a0, a1 in fams["large"]:
        at = 0 if name.endswith("@0") else 1199
        nrm = np.linalg.norm(a0, axis=1)
        assert nrm[at] >= 49 * np.delete(nrm, at).max(), name
        _, _, inter = T.block(a0, a0, W[0])
        assert np.abs(inter["k"][at]).max() > 10 * np.abs(np.delete(inter["k"], at, 0)).max(), name
    # self pairs
    for _, a0, a1 in fams["self"]:
        assert np.array_equal(a0, a1)
    # negative targets at the block they are built for
    for bi in range(8):
        for target in TK.TARGETS:
            a0, a1 = TK.negative(bi, target)
            me = bi % 2
            x, s = (a0, a1)[me], (a0, a1)[me if T.SELF[bi] else 1 - me]
            _, _, inter = T.block(x, s, W[bi])
            assert inter["q"].max() <= target + 1 and inter["k"].max() <= target + 1, (bi, target)
            if target == -12:          # eps-dominated normaliser: Q . Ksum no larger than a few eps
                assert inter["den"].max() < 5 * T.Z_EPS, (bi, inter["den"].max())
            if target == -20:          # saturated ELU: K and Q exactly 0 in the graph and in both kernels (bound 0)
                assert np.all(inter["K"] == 0) and np.all(inter["Q"] == 0)
                assert np.all(inter["msg"] == 0) and np.all(inter["merged"] == W[bi]["n1b"])
                for u in T.UNITS:
                    e = inter["E_" + u]
                    assert np.all(e["K"] == 0) and np.all(e["Q"] == 0) and np.all(e["msg"] == 0), (bi, u)


_CASES = None


def _mutant_cases():
    """the GPU tests' (family, range) cases with their reference outputs, computed once"""
    global _CASES
    if _CASES is None:
        _CASES = []
        for fam, name, first, n, a0, a1 in TK.cases():
            r0, r1, _, _ = T.run(a0, a1, first, n, with_bounds=False)
            _CASES.append((fam, name, first, n, a0, a1, r0, r1))
    return _CASES


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_mutants_are_caught(mutant):
    """Changes to the reference that stand for kernel bugs.  Each must move some entry of some case of
    tests/test_loftr_transformer_gpu.py past the criterion that test holds the GPU to there (BAR of the token's scale),
    so a kernel with that bug fails it.  The case that moves furthest is printed."""
    best = (0.0, None)
    for fam, name, first, n, a0, a1, r0, r1 in _mutant_cases():
        m0, m1, _, _ = T.run(a0, a1, first, n, mutant=mutant, with_bounds=False)
        rel = max(float((np.abs(m0 - r0) / TK.scale_of(r0)).max()), float((np.abs(m1 - r1) / TK.scale_of(r1)).max()))
        best = max(best, (rel, "%s/%s [%d, %d)" % (fam, name, first, first + n)), key=lambda t: t[0])
    print("\n[%s] furthest: %s, %.3g of scale (bar %g)" % (mutant, best[1], best[0], BAR))
    assert best[0] > BAR, (mutant, best)
