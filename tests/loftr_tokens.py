"""Token families for the LoFTR transformer tests (tests/test_loftr_transformer_*.py): pairs of f32 sequences
[1200][32] before an encoder block, each built to reach the regime it is named for (seeded, built at test time)."""
import os

import numpy as np

from oracle import loftr_transformer as T

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "loftr_kat.npz"))
KATS = ["i", "ii", "iii", "synth"]
SCALES = [1 / 64, 1 / 8, 8, 64]
TARGETS = [-4, -12, -20]
_TOK = {}


def kat_tokens(name):
    """pre-transformer tokens of a KAT pair: the ONNX graph's for ii (golden), the C restatement's for the others"""
    if name not in _TOK:
        if name == "ii":
            _TOK[name] = (GOLD["tok0_ii"].copy(), GOLD["tok1_ii"].copy())
        else:
            from oracle import loftr
            r = loftr.DNNFeatureMatcherOracle(0.15).run(GOLD["img0_" + name], GOLD["img1_" + name])
            _TOK[name] = (r["tok"][0].copy(), r["tok"][1].copy())
    return _TOK[name]


def _one_sided_lstsq(A, target, iters=2000):
    """x with x A <= target in every entry, by least squares onto the clipped target (alternating projections)"""
    t = np.full(A.shape[1], float(target))
    for _ in range(iters):
        x = np.linalg.lstsq(A.T, t, rcond=None)[0]
        t = np.minimum(x @ A, target)
    return x


def negative(bi, target, seed=0):
    """(in0, in1) before block bi whose q and k at block bi are all <= target (+ 1): least squares through the block's
    Wq / Wk; a self block drives both from the updated sequence, a cross block q from it and k from the source.  Each
    token is the solution times 1 .. 1.5 plus a random perturbation that moves no q or k by more than 1."""
    W = T.weights()[bi]
    rng = np.random.default_rng(seed + 100 * bi)
    me = bi % 2

    def tokens(A):
        x = _one_sided_lstsq(A, target)
        d = rng.standard_normal((T.NTOK, T.DM))
        d /= np.abs(d @ A).max(1, keepdims=True)
        return (x[None] * (1 + 0.5 * rng.random((T.NTOK, 1))) + d).astype(np.float32)

    if T.SELF[bi]:
        xs = tokens(np.concatenate([W["wq"], W["wk"]], 1))
        seq = [xs, xs.copy()]
    else:
        seq = [None, None]
        seq[me] = tokens(W["wq"])
        seq[1 - me] = tokens(W["wk"])
    return seq[0], seq[1]


def large_norm(at, k=50.0):
    """KAT ii with the token at index `at` of both sequences scaled to k x the largest token norm"""
    t0, t1 = (a.copy() for a in kat_tokens("ii"))
    for t in (t0, t1):
        t[at] *= np.float32(k * np.linalg.norm(t, axis=1).max() / np.linalg.norm(t[at]))
    return t0, t1


def families():
    """{family: [(name, t0, t1)]} of sequences before block 0 (every family but 'negative', which is per block)"""
    kat = [(n,) + kat_tokens(n) for n in KATS]
    t0, t1 = kat_tokens("ii")
    z = np.zeros((T.NTOK, T.DM), np.float32)
    return {
        "kat": kat,
        "scale": [("x%g" % k, (t0 * np.float32(k)).astype(np.float32), (t1 * np.float32(k)).astype(np.float32)) for k in SCALES],
        "zero": [("zero", z, z.copy())],
        "large": [("large@0",) + large_norm(0), ("large@1199",) + large_norm(1199)],
        "self": [("self_ii", t0, t0.copy()), ("self_i",) + (kat_tokens("i")[1], kat_tokens("i")[1].copy())],
    }


RANGES = [(bi, 1) for bi in range(8)] + [(0, 2), (4, 2), (0, 8)]


def cases():
    """[(family, name, first, n, in0, in1)]: every family on every range of RANGES, from the f32-rounded reference state
    before `first` (errors do not compound); the negative families on the ranges they are built for (not [0, 8))"""
    out = []
    for fam, pairs in families().items():
        for name, t0, t1 in pairs:
            blocks = []
            T.run(t0, t1, 0, 8, blocks=blocks, with_bounds=False)
            state = [(np.asarray(t0, np.float32), np.asarray(t1, np.float32))] + [None] * 8
            s = [np.asarray(t0, np.float64), np.asarray(t1, np.float64)]
            for bi, o, _, _ in blocks:
                s[bi % 2] = o
                state[bi + 1] = (s[0].astype(np.float32), s[1].astype(np.float32))
            for first, n in RANGES:
                out.append((fam, name, first, n) + state[first])
    for target in TARGETS:
        for first, n in RANGES:
            if n < 8:
                out.append(("negative", "%d@%d" % (target, first), first, n) + negative(first, target))
    return out


def scale_of(ref):
    """the scale an entry's error is measured against: its token's RMS, at least 1"""
    return np.maximum(1.0, np.sqrt((np.asarray(ref, np.float64) ** 2).mean(-1, keepdims=True)))
