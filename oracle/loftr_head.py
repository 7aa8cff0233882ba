"""Float64 restatement of the LoFTR matching head -- TEST INFRASTRUCTURE ONLY.
s = (f0 / sqrt(32)) . (f1 / sqrt(32)) / 0.1, conf = softmax_rows(s) * softmax_cols(s), matches = conf > thr in
row-major order (src/dnnfeaturematcher.cpp:44-102 after the graph).  Pinned by tests/test_loftr_head_ref.py to
tests/golden/loftr_kat.npz and to the CPU restatement of the whole graph (oracle/loftr.py).

rho(f0, f1) bounds the error of the GPU head on the same f32 features, as |ln conf_gpu - ln conf_ref| (derivation in
tests/test_loftr_head_gpu.py)."""
import numpy as np

U = 2.0 ** -24            # unit roundoff of f32
C_S = 48                  # error of one exponent argument, in units of U * G
C_SUM = 256               # relative error of one 1200-term f32 sum, in units of U
C_OPS = 8                 # the exps, divisions and product of the final confidence, in units of U
EXP_MIN = 2.0 ** -126     # below this an f32 exp result may be lost
RANGE_LO, RANGE_HI = 1e-30, 1e30   # the single-pass statistics' range check (k_sim_finish)


def logits(f0, f1):
    f0 = np.asarray(f0, np.float64)
    f1 = np.asarray(f1, np.float64)
    return (f0 @ f1.T) / 32.0 / 0.1


def g_bound(f0, f1):
    """max_i |f0_i| max_j |f1_j| / 3.2 >= every |s_ij| (Cauchy-Schwarz); the single pass's offset is 1.0001 x this."""
    n0 = np.sqrt((np.asarray(f0, np.float64) ** 2).sum(1)).max()
    n1 = np.sqrt((np.asarray(f1, np.float64) ** 2).sum(1)).max()
    return float(n0 * n1 / 3.2)


def head(f0, f1, thr):
    """float64 S, conf and the row-major (i, j) list of conf > thr for one pair of [1200][32] feature arrays"""
    s = logits(f0, f1)
    er = np.exp(s - s.max(1, keepdims=True))
    ec = np.exp(s - s.max(0, keepdims=True))
    conf = (er / er.sum(1, keepdims=True)) * (ec / ec.sum(0, keepdims=True))
    return s, conf, np.argwhere(conf > thr)


def rho(f0, f1):
    """Bound on |ln conf_gpu - ln conf_ref| for every entry whose f32 confidence is a normal number."""
    G = g_bound(f0, f1)
    r = 4 * C_S * U * G + 2 * C_SUM * U + C_OPS * U
    if 2 * 1.0001 * G > -np.log(EXP_MIN):
        # an entry of the single pass can underflow; a sum that passed the range check loses at most 1200 of them
        r += 2 * 1200 * EXP_MIN / RANGE_LO
    return float(r)


def single_pass_flagged(f0, f1, margin=2.0):
    """Whether k_sim_finish flags the pair for the running-maximum redo: some row or column sum of exp(s - G) outside
    [1e-30, 1e30].  Returns (flagged, clear): clear is False when the answer rests on a sum within a factor e^margin of
    a bound."""
    s = logits(f0, f1)
    G = 1.0001 * g_bound(f0, f1)
    with np.errstate(under="ignore"):
        e = np.exp(s - G)
    lo, hi = np.log(RANGE_LO), np.log(RANGE_HI)
    sums = np.concatenate([e.sum(1), e.sum(0)])
    with np.errstate(divide="ignore"):
        ls = np.log(sums)
    flagged = bool((ls <= lo).any() or (ls >= hi).any())
    if flagged:      # certain when some sum is well outside
        clear = bool((ls < lo - margin).any() or (ls > hi + margin).any())
    else:            # certain when every sum is well inside
        clear = bool(np.all((ls > lo + margin) & (ls < hi - margin)))
    return flagged, clear


def cells(ij):
    """(i, j) pairs -> msf_match rows (x1, y1, x2, y2): the top-left corners of the 16 x 16 cells"""
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    i, j = ij[:, 0], ij[:, 1]
    return np.stack([(i % 40) * 16, (i // 40) * 16, (j % 40) * 16, (j // 40) * 16], 1).astype(np.int32)
