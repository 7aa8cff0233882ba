"""CPU helpers of the ORB matcher tests (tests/test_orb_match_ref.py, tests/test_orb_match_gpu.py): a plain numpy
restatement of the reference's matching step, and generators of feature sets that put both Hamming 2-NN kernels of
csrc/orb_kernels.hip where real frames never take them.  No GPU, no library of the project.

ref_match restates featurematcher.cpp:23-42 (BFMatcher(NORM_HAMMING).knnMatch(k = 2), the ratio test, the two
cv::Point2i) on its own, independently of oracle/orb_oracle.c: distances from unpacked bits, the best train row the
LOWEST index at the minimum distance (batchDistance's strict '<' insertion), the second-best distance the minimum over
the remaining rows, the ratio test in f32 with the product rounded once.

The features are (kp, desc): kp a KP_DTYPE array of which only x and y matter to a matcher, desc uint8 [n, 32]."""
import functools

import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("angle", "<f4"),
                     ("octave", "<i4"), ("lx", "<i4"), ("ly", "<i4"), ("fast_score", "<i4")])

KP_CAP = 2048                      # key points a feature slot holds
CHUNK = 1024                       # train rows per LDS pass of both kernels (the default)
SIZES = [0, 1, 2, 63, 64, 65, 255, 257, 1023, 1025, 2048]
POOL_SEED = 20260
# One seed per size: 1000 + n, except where that draw misses a condition on the INPUTS that tests/test_orb_match_ref.py
# asserts.  The three small sets share few pool rows with each other (a pair of them needs a match and six ties), and
# row 1024 of the 1025-row set -- its only row in the second chunk -- has to be one of two equal bests and the best or
# second-best of a passing query.  The seeds were picked by those conditions on the CPU reference, before any kernel ran.
SEEDS = {n: 1000 + n for n in SIZES}
SEEDS.update({63: 1863, 64: 2764, 65: 1365, 1025: 2029})


def _bits(desc):
    return np.unpackbits(np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), axis=1)


def hamming(d1, d2):
    """int32 [n1, n2]: Hamming distances of uint8 [n, 32] descriptors, from unpacked bits (sums of 256 products of 0 / 1
    in f32 are exact)"""
    a, b = _bits(d1).astype(np.float32), _bits(d2).astype(np.float32)
    return (a @ (1.0 - b).T + (1.0 - a) @ b.T).astype(np.int32)


def ref_knn(d1, d2):
    """-> (d0, i0, dd1, i1) int32 [n1]: best distance and its LOWEST train index, second-best distance = the minimum over
    the remaining rows, and the lowest index of that; needs n2 >= 2"""
    D = hamming(d1, d2)
    rows = np.arange(len(D))
    i0 = D.argmin(axis=1)                      # numpy: the first occurrence of the minimum
    d0 = D[rows, i0]
    D[rows, i0] = 1 << 20
    i1 = D.argmin(axis=1)
    return d0.astype(np.int32), i0.astype(np.int32), D[rows, i1].astype(np.int32), i1.astype(np.int32)


def ratio_pass(d0, d1, ratio):
    """float(d0) < ratio * float(d1) as featurematcher.cpp:32 computes it: all three f32, the product rounded once"""
    return np.asarray(d0).astype(np.float32) < np.float32(ratio) * np.asarray(d1).astype(np.float32)


def ref_match(k1, d1, k2, d2, ratio, knn=None):
    """featurematcher.cpp:23-42 -> int32 [m, 4] rows (int(x1), int(y1), int(x2), int(y2)) in query order; nothing when
    n1 == 0 or n2 < 2.  knn: ref_knn(d1, d2) if the caller has it already."""
    if len(d1) == 0 or len(d2) < 2:
        return np.zeros((0, 4), np.int32)
    d0, i0, dd1, _ = ref_knn(d1, d2) if knn is None else knn
    q = np.flatnonzero(ratio_pass(d0, dd1, ratio))
    t = i0[q]
    out = np.stack([k1["x"][q], k1["y"][q], k2["x"][t], k2["y"][t]], axis=1)
    return np.trunc(out).astype(np.int32)      # static_cast<int>(pt.x)


def pool():
    """2048 seeded random descriptors every set of the grid draws from: uint8 [2048, 32]"""
    return np.random.default_rng(POOL_SEED).integers(0, 256, (2048, 32), dtype=np.uint8)


def _flip(rng, bits, row, k):
    at = rng.choice(256, k, replace=False)
    bits[row, at] ^= 1


def feature_set(n, seed, pool_desc):
    """n distinct pool rows with 0 to 29 random bits flipped each; then n // 8 random rows become exact copies of other
    rows of the set (two equal bests at different train indices) and n // 4 random rows copies with 1 to 11 bits flipped
    (a second-best close to the best).  Key points: seeded uniform f32 in [0, 640) x [0, 480); a copied row keeps its own,
    so a match shows which train row it took.  -> (kp KP_DTYPE [n], desc uint8 [n, 32])"""
    rng = np.random.default_rng(seed)
    bits = _bits(pool_desc[rng.choice(len(pool_desc), n, replace=False)])
    for r in range(n):
        _flip(rng, bits, r, int(rng.integers(0, 30)))
    for exact in (True, False):
        for _ in range(n // 8 if exact else n // 4):
            dst = int(rng.integers(0, n))
            src = int(rng.integers(0, n - 1))
            src += src >= dst
            bits[dst] = bits[src]
            if not exact:
                _flip(rng, bits, dst, int(rng.integers(1, 12)))
    kp = np.zeros(n, KP_DTYPE)
    kp["x"] = rng.random(n, dtype=np.float32) * np.float32(640)
    kp["y"] = rng.random(n, dtype=np.float32) * np.float32(480)
    return kp, np.packbits(bits, axis=1).reshape(n, 32)


@functools.lru_cache(maxsize=None)
def grid_sets():
    """the 11 sets of SIZES, set i for slot i"""
    p = pool()
    return tuple(feature_set(n, SEEDS[n], p) for n in SIZES)


@functools.lru_cache(maxsize=None)
def grid_knn(a, b):
    """ref_knn of (query set a, train set b) of the grid, computed once; None where there is nothing to match"""
    (_, d1), (_, d2) = grid_sets()[a], grid_sets()[b]
    return None if len(d1) == 0 or len(d2) < 2 else ref_knn(d1, d2)


@functools.lru_cache(maxsize=None)
def grid_ref(a, b, ratio):
    """ref_match of (query set a, train set b) of the grid; shared by the tests, never written to"""
    (k1, d1), (k2, d2) = grid_sets()[a], grid_sets()[b]
    out = ref_match(k1, d1, k2, d2, ratio, knn=grid_knn(a, b))
    out.setflags(write=False)
    return out


def quarter_of(t, n2, chunk=CHUNK):
    """(chunk, wave) that scans train row t of an n2-row set in k_match_split: the chunk's rows [tn w / 4, tn (w + 1) / 4)
    go to wave w of four"""
    c = t // chunk
    tn = min(n2 - c * chunk, chunk)
    r = t - c * chunk
    return c, next(w for w in range(4) if (tn * w) >> 2 <= r < (tn * (w + 1)) >> 2)


def pair_list():
    """all 121 ordered pairs of the 11 slots, then 39 of them again by a seeded choice: 160 pairs, int32 [160, 2]"""
    n = len(SIZES)
    every = np.array([(a, b) for a in range(n) for b in range(n)], np.int32)
    again = np.random.default_rng(160).choice(len(every), 160 - len(every), replace=False)
    return np.concatenate([every, every[again]])


def ratio_edge_pairs(ratio):
    """every (d0, d1), d0 <= d1 <= 64, on which the f32 ratio test differs from the same comparison in float64 -- with the
    ratio as written, or with the ratio rounded to f32 first.  -> list of (d0, d1, passes in f32, passes in float64,
    passes in float64 with the f32 ratio)"""
    out = []
    for d1 in range(1, 65):
        for d0 in range(0, d1 + 1):
            p32 = bool(ratio_pass(d0, d1, ratio))
            p64 = float(d0) < float(ratio) * float(d1)
            p64r = float(d0) < float(np.float32(ratio)) * float(d1)
            if p32 != p64 or p32 != p64r:
                out.append((d0, d1, p32, p64, p64r))
    return out


EDGE_TRAIN_ROWS = 1100             # crosses the 1024 chunk
EDGE_QUERY_ROWS = 140              # three 64-query blocks; planted query j is row 12 j


def edge_positions(j):
    """train rows (best, second-best) of planted pair j: even j in different 256-row quarters of the first chunk -- or,
    j = 0 and 6, in different chunks --, odd j three rows apart; j // 2 even: the second-best comes first"""
    lo = 30 + 8 * j
    hi = lo + 3 if j % 2 else (1030 if j % 3 == 0 else 600) + 8 * j
    return (hi, lo) if (j // 2) % 2 == 0 else (lo, hi)


@functools.lru_cache(maxsize=None)
def ratio_edge_set(ratio):
    """One query per pair of ratio_edge_pairs(ratio), with a train row at exactly d0 flipped bits and another at exactly
    d1 flipped bits of a disjoint bit set, among random fillers (which sit near distance 128).
    -> (kq, dq, kt, dt, planted) with planted a list of (query row, d0, d1, best train row, second-best train row)"""
    pairs = ratio_edge_pairs(ratio)
    rng = np.random.default_rng(int(round(ratio * 1000)))
    qbits = rng.integers(0, 2, (EDGE_QUERY_ROWS, 256), dtype=np.uint8)
    tbits = rng.integers(0, 2, (EDGE_TRAIN_ROWS, 256), dtype=np.uint8)
    planted = []
    for j, (d0, d1, _, _, _) in enumerate(pairs):
        q = 12 * j
        best, second = edge_positions(j)
        at = rng.permutation(256)
        tbits[best] = qbits[q]
        tbits[best, at[:d0]] ^= 1
        tbits[second] = qbits[q]
        tbits[second, at[d0:d0 + d1]] ^= 1
        planted.append((q, d0, d1, best, second))
    taken = {r for p in planted for r in p[3:]}
    dq = np.packbits(qbits, axis=1)
    for _ in range(100):
        dt = np.packbits(tbits, axis=1)
        D = hamming(dq[[p[0] for p in planted]], dt)
        close = {int(t) for j, p in enumerate(planted) for t in np.flatnonzero(D[j] <= p[2]) if int(t) not in taken}
        if not close:
            break
        for t in close:                        # a filler nearer than a planted second-best: draw it again
            tbits[t] = rng.integers(0, 2, 256, dtype=np.uint8)
    else:
        raise AssertionError("fillers keep landing inside a planted distance")
    kq, kt = np.zeros(EDGE_QUERY_ROWS, KP_DTYPE), np.zeros(EDGE_TRAIN_ROWS, KP_DTYPE)
    for k in (kq, kt):
        k["x"] = rng.random(len(k), dtype=np.float32) * np.float32(639)
        k["y"] = rng.random(len(k), dtype=np.float32) * np.float32(479)
    return kq, dq, kt, dt, planted
