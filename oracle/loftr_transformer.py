"""Float64 restatement of the LoFTR coarse transformer (8 linear-attention encoder blocks) -- TEST INFRASTRUCTURE ONLY.
Block b updates sequence b % 2 from itself (b % 4 < 2) or from the other sequence's current value, as the graph
and oracle/loftr_oracle.c block() do.  Pinned by tests/test_loftr_transformer_ref.py to tests/golden/loftr_kat.npz
and to the C restatement; tests/test_loftr_transformer_gpu.py holds the GPU blocks to it.

Everything is float64 except ELU + 1, which is the graph's f32 form f32(f32(f32(exp x) - 1) + 1) on f32(x) (a float64
ELU is not the graph: below x ~ -17.3 the graph's value is exactly 0).

Alongside each value the reference carries a bound E on |gpu - ref| for two units, "f32" (k_attn_kv / k_attn_update)
and "split" (k_attn_kv_x / k_attn_update_x).  Each operation pushes the bounds of its inputs through (first order plus
the cross terms, so the bound holds for finite perturbations) and adds its own rounding.  u = 2^-24.

* Products sum_k a_k w_k over K terms (a and w both carrying bounds: E_a |w| + |a| E_w + E_a E_w), plus rounding
  rel(K) (|a| + E_a)(|w| + E_w):
  - f32: a chain of v_mfma_f32_16x16x4f32, K roundings of partial sums: K u.
  - split: hi = bf16(v) and lo = bf16(v - hi), both round to nearest: |v - hi - lo| <= 2^-16 |v| and
    |lo| <= 2^-8 (1 + 2^-8) |v|.  Keeping hi.hi, hi.lo and lo.hi drops lo.lo and the two remainders' products:
    <= (2^-16 (1 + 2^-8)^2 + 2 2^-16 (1 + 2^-16) + 2^-32) |a w| <= C_SPLIT |a w| with C_SPLIT = 3.02 2^-16.  The three
    MFMAs accumulate 3K products into f32, each rounding at a partial sum <= (1 + 2^-7) sum |a w|: 3K (1 + 2^-7) u.
* The 1200-term sums (sums of products over tokens).  Ksum: per lane <= 40 terms, 2 lane-group and 7 wave additions:
  D_KSUM = 50 for both units (all terms >= 0, so relative to the sum).  KV: f32, per wave <= 10 tiles x 4 MFMAs x 4
  tokens = 160 roundings + 7 waves: D_KV = 168; split, <= 5 tile pairs x 3 MFMAs x 32 tokens = 480 + 7, at partial sums
  <= (1 + 2^-7) sum |K V|: D_KV = 492, plus C_SPLIT.
* V = v / 1200: f32 divides (u), split multiplies by the rounded reciprocal (2u).
* ELU + 1 of q with bound E_q (the graph rounds q to f32 first: u |q| more): Lipschitz min(1, e^(q + E)) on the
  interval; rounding, positive branch: f32(x + 1) on both sides, 2u |Q|; negative branch: exp's relative errors
  (graph ~u, kernel expf or v_exp_f32 of x log2(e): <= 3.5u), e^x (1 + 4.5u) at most, then -1 and +1: each side can
  land on either neighbour of a 2^-24-spaced grid near 1: an absolute ulp(1) = 2^-23.  Where q + E_q + u |q| <= -17.5
  both the graph and both kernels give exactly 0 (exp <= 2^-25 makes e - 1 round to -1): E_Q = 0.
* z = 1 / (Q . Ksum + eps), eps = f32(1e-6): the denominator is a sum of positive terms: its bound is
  sum E_Q Ks + Q E_Ks + E_Q E_Ks + (K + 2) u den (32 products, 8 per lane, 2 lane-group additions, + eps).  With
  r = E_den / den < 1: E_z <= z r / (1 - r) + 2u z (v_rcp_f32 or the division).  r >= 1: infinite.
* msg = (Q . KV) z 1200: product bounds as above, then 2u |msg|.
* LayerNorm y = (m - mean) / sigma w + b, sigma = sqrt(var + 1e-7): the GPU's sigma' >= sigma_lo =
  max(sqrt(eps), sigma - |E_m|_2 / sqrt(32)) (the standard deviation is 1/sqrt(32)-Lipschitz in the 2-norm), so
  |n' - n| <= (2 |E_m|_inf + |n| |E_m|_2 / sqrt(32)) / sigma_lo.  Its own rounding: the mean, 10u mean|m| (8 + 2
  additions), enters every n as 10u mean|m| / sigma_lo; sigma (variance sum, eps, sqrt or v_rsq_f32) and the
  subtraction, division or product: 16u |n|.  Then times w and plus b: |w| E_n + 2u |n w| + u |y|.  The amplification
  is |w| / sigma with eps included: at zero variance sigma = sqrt(1e-7).
* ReLU is 1-Lipschitz; the residual adds E_x and u |out|.

An entry whose bound is not finite, or exceeds its token's RMS (the value's own scale), is undetermined: the tests
count and report those entries; they are still held to their (finite) bound.
"""
import os
import struct

import numpy as np

U = 2.0 ** -24
C_SPLIT = 3.02 * 2.0 ** -16
ULP1 = 2.0 ** -23
SAT = -17.5                      # q at or below this (with its bound): ELU + 1 is exactly 0 in the graph and both kernels
Z_EPS = 9.99999997e-7
LN_EPS = 1.0000000116860974e-07
NTOK, DM = 1200, 32
UNITS = ("f32", "split")
WEIGHTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mono_slam_framework_amd", "weights",
                       "loftr_teacher.bin")
# one-block sources (bi % 4 < 2: self-attention) and the sequence each block updates (bi % 2)
SELF = [bi % 4 < 2 for bi in range(8)]

MUTANTS = ("drop_last_tile", "z_eps_1e-5", "ln_eps_1e-5", "block3_stale_f0", "neighbour_ln", "split_drop_hi_lo")


class Unit:
    def __init__(self, name):
        self.name = name
        split = name == "split"
        self.c_prod = (lambda K: C_SPLIT + 3 * K * (1 + 2.0 ** -7) * U) if split else (lambda K: K * U)
        self.d_ksum = 50 * U
        self.c_kv = C_SPLIT + 492 * (1 + 2.0 ** -7) * U if split else 168 * U
        self.c_div1200 = 2 * U if split else U


_UNITS = {n: Unit(n) for n in UNITS}


def load_weights(path=WEIGHTS):
    """{'blk%d' % b: {wq, wk, wv, wm, w0, w1, n1w, n1b, n2w, n2b}} as float64 ([in][out] matrices); the LayerNorm
    parameters of block b are those of layer b // 2"""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != b"MSFLTR01":
        raise IOError("not an MSFLTR01 blob: " + path)
    n = struct.unpack_from("<I", raw, 8)[0]
    recs, o = {}, 12
    for _ in range(n):
        name, nd, d0, d1, d2, d3, off, cnt = struct.unpack_from("<32sI4III", raw, o)
        o += 60
        recs[name.rstrip(b"\0").decode()] = ((d0, d1, d2, d3)[:nd], off, cnt)
    data = np.frombuffer(raw, np.float32, offset=o)

    def get(k):
        shape, off, cnt = recs[k]
        return data[off:off + cnt].reshape(shape).astype(np.float64)

    W = []
    for b in range(8):
        L = b // 2
        W.append({"wq": get("blk%d.wq" % b), "wk": get("blk%d.wk" % b), "wv": get("blk%d.wv" % b),
                  "wm": get("blk%d.wmerge" % b), "w0": get("blk%d.wmlp0" % b), "w1": get("blk%d.wmlp1" % b),
                  "n1w": get("ln%d.n1w" % L), "n1b": get("ln%d.n1b" % L), "n2w": get("ln%d.n2w" % L),
                  "n2b": get("ln%d.n2b" % L)})
    return W


_W = None


def weights():
    global _W
    if _W is None:
        _W = load_weights()
    return _W


def elu1_graph(x):
    """the graph's ELU + 1 in f32 arithmetic on f32(x)"""
    xf = np.asarray(x, np.float64).astype(np.float32)
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp(xf.astype(np.float64)).astype(np.float32)
    neg = ((e - np.float32(1)) + np.float32(1)).astype(np.float32)
    pos = (xf + np.float32(1)).astype(np.float32)
    return np.where(xf > 0, pos, neg).astype(np.float64)


def _bf16(v):
    """round-to-nearest-even bf16 of f32 values, as float64"""
    b = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def _split_mm_drop(a, w):
    """mutant: a split product that keeps hi.hi and lo.hi but drops hi.lo"""
    ah = _bf16(a.astype(np.float32))
    al = _bf16((a.astype(np.float32) - ah.astype(np.float32)).astype(np.float32))
    wh = _bf16(w.astype(np.float32))
    return ah @ wh + al @ wh


# ------------------------------------------------------------------ bounds
def _mm_err(a, Ea, w, Ew, c):
    """bound of a @ w where a, w carry bounds (Ew None: exact weights), c the product's relative rounding"""
    aa = np.abs(a) + Ea
    if Ew is None:
        aw = np.abs(w)
        return Ea @ aw + c * (aa @ aw)
    ww = np.abs(w) + Ew
    return Ea @ np.abs(w) + np.abs(a) @ Ew + Ea @ Ew + c * (aa @ ww)


def _elu_err(q, Eq, Q):
    Eq = Eq + U * np.abs(q)
    with np.errstate(over="ignore"):
        lip = np.minimum(1.0, np.exp(np.minimum(q + Eq, 0.0)))
    E = lip * Eq
    maybe_neg = q - Eq <= 0
    maybe_pos = q + Eq > 0
    exact_one = (q == 0) & (Eq == 0)                   # exp(0) = 1 exactly: both branches give 1
    E = E + np.where(maybe_pos, 2 * U * (np.abs(Q) + E), 0.0)
    with np.errstate(over="ignore"):
        e_hi = np.exp(np.minimum(q + Eq, 0.0))
    E = E + np.where(maybe_neg & ~exact_one, ULP1 + 4.5 * U * e_hi, 0.0)
    sat = q + Eq <= SAT
    return np.where(sat, 0.0, E)


def _ln(m, Em, w, b, eps=LN_EPS):
    """LayerNorm of rows of m (float64) and its bound"""
    mu = m.mean(1, keepdims=True)
    c = m - mu
    var = (c * c).mean(1, keepdims=True)
    sig = np.sqrt(var + eps)
    n = c / sig
    y = n * w + b
    if Em is None:
        return y, n, sig, None
    e2 = np.sqrt((Em * Em).sum(1, keepdims=True))
    einf = Em.max(1, keepdims=True)
    sig_lo = np.maximum(np.sqrt(eps), sig - e2 / np.sqrt(DM))
    En = (2 * einf + np.abs(n) * e2 / np.sqrt(DM)) / sig_lo
    En = En + 10 * U * np.abs(m).mean(1, keepdims=True) / sig_lo + 16 * U * (np.abs(n) + En)
    Ey = np.abs(w) * En + 2 * U * (np.abs(n) + En) * np.abs(w) + U * (np.abs(y) + np.abs(w) * En)
    return y, n, sig, Ey


def block(x, s, W, Ex=None, Es=None, mutant=None, with_bounds=True):
    """One encoder block: x [1200][32] updated from source s.  W: one entry of weights().  Ex / Es: {unit: bound} of the
    inputs (None: exact).  Returns (out float64, {unit: bound}, intermediates)."""
    x = np.asarray(x, np.float64)
    s = np.asarray(s, np.float64)
    mm = _split_mm_drop if mutant == "split_drop_hi_lo" else (lambda a, w: a @ w)
    q = mm(x, W["wq"])
    k = mm(s, W["wk"])
    v = mm(s, W["wv"])
    Q, K = elu1_graph(q), elu1_graph(k)
    V = v / 1200.0
    Kt, Vt = (K[:-16], V[:-16]) if mutant == "drop_last_tile" else (K, V)
    KV = Kt.T @ Vt                                    # [d][e]
    Ks = Kt.sum(0)                                    # [d]
    zeps = 1e-5 if mutant == "z_eps_1e-5" else Z_EPS
    den = Q @ Ks + zeps
    z = 1.0 / den
    t = Q @ KV
    msg = t * z[:, None] * 1200.0
    mg = mm(msg, W["wm"])
    lneps = 1e-5 if mutant == "ln_eps_1e-5" else LN_EPS
    merged, _, sig1, _ = _ln(mg, None, W["n1w"], W["n1b"], lneps)
    cat = np.concatenate([x, merged], 1)
    h = np.maximum(mm(cat, W["w0"]), 0.0)
    o = mm(h, W["w1"])
    o2, _, sig2, _ = _ln(o, None, W["n2w"], W["n2b"], lneps)
    out = x + o2
    inter = {"q": q, "k": k, "Q": Q, "K": K, "Ksum": Ks, "den": den, "msg": msg, "merged": merged, "sigma1": sig1[:, 0],
             "sigma2": sig2[:, 0]}
    bounds = {}
    old = np.seterr(invalid="ignore", over="ignore")      # an infinite bound times 0 is handled below
    for un in UNITS if with_bounds else ():
        u = _UNITS[un]
        ex = np.zeros_like(x) if Ex is None else Ex[un]
        es = np.zeros_like(s) if Es is None else Es[un]
        Eq = _mm_err(x, ex, W["wq"], None, u.c_prod(32))
        Ek = _mm_err(s, es, W["wk"], None, u.c_prod(32))
        Ev = _mm_err(s, es, W["wv"], None, u.c_prod(32))
        EQ, EK = _elu_err(q, Eq, Q), _elu_err(k, Ek, K)
        EV = Ev / 1200.0 + u.c_div1200 * (np.abs(V) + Ev / 1200.0)
        EKV = _mm_err(K.T, EK.T, V, EV, u.c_kv)
        EKs = EK.sum(0) + u.d_ksum * (Ks + EK.sum(0))
        Eden = EQ @ Ks + Q @ EKs + EQ @ EKs + (DM + 2) * U * (den + EQ @ Ks + Q @ EKs + EQ @ EKs)
        r = Eden / den
        with np.errstate(divide="ignore", invalid="ignore"):
            Ez = np.where(r < 1, z * r / (1 - r), np.inf) + 2 * U * z
        Et = _mm_err(Q, EQ, KV, EKV, u.c_prod(32))
        with np.errstate(invalid="ignore"):
            Emsg = 1200.0 * (Et * z[:, None] + np.abs(t) * Ez[:, None] + Et * Ez[:, None])
            Emsg = np.where(Et + np.abs(t) == 0, 0.0, Emsg)          # t exactly 0 on both sides: msg exactly 0
        Emsg = Emsg + 2 * U * (np.abs(msg) + Emsg)
        Emg = _mm_err(msg, Emsg, W["wm"], None, u.c_prod(32))
        _, _, _, Emerged = _ln(mg, Emg, W["n1w"], W["n1b"])
        Eh = _mm_err(cat, np.concatenate([ex, Emerged], 1), W["w0"], None, u.c_prod(64))
        Eo = _mm_err(h, Eh, W["w1"], None, u.c_prod(64))
        _, _, _, Eo2 = _ln(o, Eo, W["n2w"], W["n2b"])
        with np.errstate(invalid="ignore"):
            Eout = ex + Eo2 + U * (np.abs(out) + ex + Eo2)
        bounds[un] = np.where(np.isnan(Eout), np.inf, Eout)          # inf x 0 of an undetermined input: undetermined
        inter["E_" + un] = {"q": Eq, "k": Ek, "Q": EQ, "K": EK, "Ksum": EKs, "z": Ez, "msg": Emsg, "merged": Emerged}
    np.seterr(**old)
    return out, bounds, inter


def run(t0, t1, first=0, n=8, W=None, E0=None, E1=None, mutant=None, blocks=None, with_bounds=True):
    """Blocks [first, first + n) on the two sequences before block `first`.  Returns (s0, s1, {unit: E0}, {unit: E1});
    `blocks`, a list, receives (bi, out, bounds, intermediates) per block.  with_bounds=False: values only (bounds
    None)."""
    W = weights() if W is None else W
    seq = [np.asarray(t0, np.float64), np.asarray(t1, np.float64)]
    err = [E0, E1]
    stale0 = None
    for bi in range(first, first + n):
        me = bi % 2
        src = me if SELF[bi] else 1 - me
        Wb = W[bi]
        if mutant == "neighbour_ln":
            Wn = W[(bi + 2) % 8]
            Wb = dict(Wb, n1w=Wn["n1w"], n1b=Wn["n1b"], n2w=Wn["n2w"], n2b=Wn["n2b"])
        s, es = seq[src], err[src]
        if mutant == "block3_stale_f0" and bi == 3 and stale0 is not None:
            s, es = stale0
        if bi == 2:
            stale0 = (seq[0], err[0])
        bm = mutant if mutant in ("drop_last_tile", "z_eps_1e-5", "ln_eps_1e-5", "split_drop_hi_lo") else None
        out, bnd, inter = block(seq[me], s, Wb, err[me], es, mutant=bm, with_bounds=with_bounds)
        bnd = bnd or None
        if blocks is not None:
            blocks.append((bi, out, bnd, inter))
        seq[me], err[me] = out, bnd
    if not with_bounds:
        return seq[0], seq[1], None, None
    z = {un: np.zeros((NTOK, DM)) for un in UNITS}
    return seq[0], seq[1], err[0] if err[0] is not None else z, err[1] if err[1] is not None else z


def undetermined(value, bound):
    """entries whose bound is not finite or exceeds the RMS of their token"""
    scale = np.sqrt((np.asarray(value, np.float64) ** 2).mean(-1, keepdims=True))
    return ~np.isfinite(bound) | (bound > scale)
