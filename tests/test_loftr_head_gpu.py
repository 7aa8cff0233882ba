"""GPU: the LoFTR matching head alone (msf_debug_loftr_head) against the float64 reference oracle/loftr_head.py, on
features the test chooses, on every path the head can take.

The error band rho bounds |ln conf_gpu - ln conf_ref| for one pair; it is derived, not tuned.  u = 2^-24, and
G = max_i |f0_i| max_j |f1_j| / 3.2 bounds every |s_ij| (Cauchy-Schwarz; the single pass's offset is 1.0001 G).

1. One exponent argument, s_ij minus its offset (the pair's G, or the row / column maximum), is off by at most
   delta = 48 u G:
   - the head's inputs f / sqrt(32), one rounding of the product or quotient plus the rounding of the constant:
     2 u |s| (u G per side);
   - the split path's three bf16 planes hold the scaled features exactly; the six products dropped or kept leave
     <= 2 u sum_k |f0s_ik f1s_jk| / 0.1 <= 2 u G; the f32 accumulation inside the MFMAs, one rounding per product
     (a k-ordered fma chain; the lower-plane products are summed first at < 2^-7 of the magnitude), <= 34 u G; the
     exact-f32 path's 32-step f32 MFMA chain is the same <= 32 u G;
   - the division by the temperature, correctly rounded: u |s| <= u G;
   - the argument itself: s - m with |s - m| <= 2 G, rounded, and v_exp_f32's argument s * log2(e) (or d * c1 + c0
     with c0 = -G log2(e), c1 = 10 log2(e) rounded), <= 4 u G.
   2 + 2 + 34 + 1 + 4 = 43 u G; the constant is rounded up to 48.
2. Every soft-max value is exp(arg) / sum_k exp(arg_k): at most 2 delta in ln from the arguments; conf is a product of
   two: 4 delta = 192 u G.
3. Each 1200-term f32 sum of positive terms (the running maximum's 25 rescaled steps of three and a 16-lane tree, or
   the single pass's 25 + 4 + 2 row and 12 + 2 + 25 column additions) is good to D u with D <= 200, with the exp ulps of
   its terms: 256 u per sum, 512 u for the two.
4. The final two exps, two divisions and one product: 8 u.
5. Only where 2 G > 87 can an entry of the single pass underflow: a sum that passed the [1e-30, 1e30] check lost at most
   1200 x 2^-126, i.e. 1.4e-5 relative each, 2.9e-5 for the two.
rho = 192 u G + 520 u (+ 2.9e-5) -- for the golden features (G = 26.5 .. 27.9) rho = 3.34e-4 .. 3.50e-4, i.e.
5.0e-5 .. 5.3e-5 absolute at thr = 0.15, twenty times tighter than the 1e-3 end-to-end bar.  Entries whose confidence is
below f32's normal range are held to 1e-9 absolute instead.

Thresholds are always > 0: at thr = 0 the f32 underflow of conf (an entry that is 0 in f32 is not listed) is the
reference graph's behaviour too, and a float64 reference cannot speak to it."""
import os

import numpy as np
import pytest

from oracle import loftr_head as ref

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "loftr_kat.npz"))
KATS = ["i", "ii", "iii", "synth"]
SCALES = [0.25, 1, 1.5, 1.9, 2.0, 2.1, 3, 8, 32, 64]
CAP = 16384
SPARSE_THR = (0.15, 0.3, 0.05)
DENSE_THR = (0.0499, 1e-4)

# path -> (pair counts per call, flags beyond KEEP_DEBUG, environment read at msf_create)
PATHS = {
    "split_few": ((1, 7), 0, {}),
    "split_single": ((8, 24), 0, {}),
    "split_running_max": ((24,), 0, {"MSF_LOFTR_SIM_SINGLE": "0"}),
    "split_no_skip": ((24,), 0, {"MSF_LOFTR_SIM_SKIP": "0"}),
    "f32": ((1, 8), "f32", {}),
    "dense_head": ((1, 24), 0, {"MSF_LOFTR_DENSE_HEAD": "1"}),
}


def _feat(name, k=1.0):
    return (GOLD["feat0_" + name] * np.float32(k)).astype(np.float32), (GOLD["feat1_" + name] * np.float32(k)).astype(np.float32)


def _handle(monkeypatch, pairs, flags=0, env=None, thr=0.15):
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = _lib.MSF_FLAG_KEEP_DEBUG | _lib.MSF_FLAG_NO_FRAME_CACHE | (_lib.MSF_FLAG_LOFTR_F32 if flags == "f32" else flags)
    dm = DNNFeatureMatcher(threshold=thr, max_batch_pairs=pairs, flags=f)
    for k in env:
        monkeypatch.delenv(k)
    return dm


def _run(dm, F0, F1, cap=CAP):
    """head_device on [n][1200][32] host features -> (n_out int32 [n], lists of (i, j) index pairs)"""
    import torch
    n = len(F0)
    d0 = torch.from_numpy(np.ascontiguousarray(F0, np.float32)).cuda()
    d1 = torch.from_numpy(np.ascontiguousarray(F1, np.float32)).cuda()
    out = torch.full((n, cap, 4), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dm.head_device(d0, d1, out, cnt)
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    return cnt, [out[p, :min(max(cnt[p], 0), cap)] for p in range(n)]


def _to_ij(m):
    m = np.asarray(m).reshape(-1, 4)
    return np.stack([(m[:, 1] // 16) * 40 + m[:, 0] // 16, (m[:, 3] // 16) * 40 + m[:, 2] // 16], 1)


class _Ref:
    """float64 reference of one pair (S, conf, rho), computed once"""
    def __init__(self, f0, f1):
        self.f0, self.f1 = f0, f1
        self.s, self.conf, _ = ref.head(f0, f1, 1.0)
        self.rho = ref.rho(f0, f1)
        self.flagged, self.clear = ref.single_pass_flagged(f0, f1)

    def band(self, thr):
        return thr * np.exp(self.rho), thr * np.exp(-self.rho)


def _check(r, n_out, got, thr, cap=CAP, tag=""):
    """listed: every conf_ref > thr e^rho; not listed: every conf_ref <= thr e^-rho; row-major; n_out consistent"""
    hi, lo = r.band(thr)
    sure = np.argwhere(r.conf > hi)
    maybe = np.argwhere(r.conf > lo)
    assert n_out >= 0, tag
    assert len(sure) <= n_out <= len(maybe), (tag, n_out, len(sure), len(maybe))
    assert len(got) == min(n_out, cap), tag
    ij = _to_ij(got)
    key = ij[:, 0].astype(np.int64) * 1200 + ij[:, 1]
    assert np.all(np.diff(key) > 0), tag + ": not row-major"
    ok = np.zeros(1200 * 1200, bool)
    ok[maybe[:, 0] * 1200 + maybe[:, 1]] = True
    assert ok[key].all(), tag + ": an entry below thr e^-rho is listed"
    if n_out <= cap:
        have = np.zeros(1200 * 1200, bool)
        have[key] = True
        missing = sure[~have[sure[:, 0] * 1200 + sure[:, 1]]]
        assert len(missing) == 0, (tag, "missing", missing[:5], r.conf[missing[:5, 0], missing[:5, 1]])
    return len(maybe) - len(sure)


def _check_conf(r, conf_dbg, tag=""):
    err = np.abs(conf_dbg.astype(np.float64) - r.conf)
    bound = np.expm1(r.rho) * r.conf + 1e-9
    bad = err > bound
    assert not bad.any(), (tag, int(bad.sum()), float((err / (r.conf + 1e-30))[bad].max()))
    return float(err.max())


# ------------------------------------------------------------------ feature families (built at test time, seeded)
def _fam_scale():
    return [_feat(KATS[p % 4], SCALES[p % 10]) for p in range(24)]


def _outlier(name, seed):
    f0, f1 = _feat(name)
    f0 = f0.copy()
    t = np.random.default_rng(seed).integers(1200)
    f0[t] *= np.float32(50.0 * np.linalg.norm(f0, axis=1).max() / np.linalg.norm(f0[t]))
    return f0, f1


def _ordinary(name, seed):
    """a KAT pair with its tokens permuted on both sides: realistic logits, a different pair per seed"""
    f0, f1 = _feat(name)
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(f0[rng.permutation(1200)]), np.ascontiguousarray(f1[rng.permutation(1200)])


def _fam_mixed():
    fam = [_ordinary(KATS[p % 4], 100 + p) for p in range(24)]
    fam[0] = _feat("ii", 3)
    fam[7] = _outlier("synth", 7)
    fam[8] = _feat("i", 8)
    fam[23] = _feat("iii", 3)
    return fam


def _fam_flat():
    z = np.zeros((1200, 32), np.float32)
    one = np.full((1200, 32), 0.5, np.float32)
    v = np.random.default_rng(5).standard_normal(32).astype(np.float32)
    tok = np.tile(v, (1200, 1))
    return [(z, z), (one, one), (tok, tok), (tok, 2 * tok)]


def _fam_ties(seed=11):
    """Rows whose maximum is shared by exactly 19 (+ one near-tie 0.005 below), 20 or 21 bitwise-identical columns:
    ~20 candidates per row at thr = 0.05, close to the sparse head's capacity; every 30th row has one strong unique
    match (conf ~ 1)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((100, 32))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    a = np.sqrt(60 * 3.2)                          # s = 60 on an aligned pair, ~36 at most across directions
    f0 = np.zeros((1200, 32), np.float64)
    f1 = np.zeros((1200, 32), np.float64)
    marked = np.arange(0, 1200, 30)                # 40 rows
    for t, i in enumerate(marked):
        f0[i] = a * d[t]
        f1[1160 + t] = a * d[t]
    sizes = [20, 20, 19, 20, 21]
    j, groups = 0, []
    g = 0
    while True:
        k = sizes[g % 5]
        width = 20 if k == 19 else k
        if j + width > 1160:
            break
        f1[j:j + k] = a * d[40 + g]
        if k == 19:
            f1[j + 19] = a * d[40 + g] * (1 - 0.005 / 60)
        groups.append(40 + g)
        j += width
        g += 1
    rows = [i for i in range(1200) if i not in set(marked)]
    for q, i in enumerate(rows):
        f0[i] = a * d[groups[q % len(groups)]]
    f0, f1 = f0.astype(np.float32), f1.astype(np.float32)
    return [(f0, f1), (f1, f0)], marked


def _fam_anti_self():
    fam = []
    for name in KATS:
        f0, _ = _feat(name)
        fam.append((f0, -f0))
        fam.append((f0, f0.copy()))
    return fam


def _fam_separated():
    """random unit tokens, every row with one match of logit L on the other side and all other logits ~L cos: every row
    has nearly the same candidate limit, and its match (conf 0.9 .. 0.99) is the largest entry of its tile"""
    fam = []
    for L, seed in ((15.0, 21), (20.0, 22)):
        rng = np.random.default_rng(seed)
        u = rng.standard_normal((1200, 32))
        u *= np.sqrt(3.2 * L) / np.linalg.norm(u, axis=1, keepdims=True)
        f = u.astype(np.float32)
        fam.append((f, np.ascontiguousarray(f[rng.permutation(1200)]) if seed == 22 else f.copy()))
    return fam


FAMILIES = {"scale": _fam_scale, "separated": _fam_separated, "mixed": _fam_mixed, "flat": _fam_flat, "ties": lambda: _fam_ties()[0],
            "anti_self": _fam_anti_self}
_REFS = {}


def _refs(family):
    if family not in _REFS:
        fam = FAMILIES[family]()
        _REFS[family] = (fam, [_Ref(f0, f1) for f0, f1 in fam])
    return _REFS[family]


def _brackets(r, thr_floor):
    """up to two entries with conf_ref in (thr_floor e^2rho, e^-2rho): the threshold can sit just either side of them;
    only where the pair's whole list at those thresholds fits the output (a cut list says nothing about a late entry)"""
    lo, hi = thr_floor * np.exp(2 * r.rho), np.exp(-2 * r.rho)
    v = np.sort(r.conf, axis=None)
    fits = v[-CAP] * np.exp(3 * r.rho) if v.size > CAP else 0.0      # below this more than CAP entries can be listed
    c = np.argwhere((r.conf > max(lo, fits)) & (r.conf < hi))
    if not len(c):
        return []
    v = r.conf[c[:, 0], c[:, 1]]
    o = np.argsort(v)
    return [tuple(c[o[0]]), tuple(c[o[len(o) // 2]])] if len(o) > 1 else [tuple(c[o[0]])]


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("path", list(PATHS))
def test_head_matches_float64_reference(monkeypatch, path, family):
    counts, flags, env = PATHS[path]
    fam, refs = _refs(family)
    thrs = (0.15,) if path == "dense_head" else SPARSE_THR + DENSE_THR
    for n in counts:
        dm = _handle(monkeypatch, n, flags, env)
        # the pairs of the family in consecutive calls of n (a family shorter than n repeats)
        m = max(n, len(fam))
        order = [p % len(fam) for p in range(((m + n - 1) // n) * n)]
        flagged = [p for p in order[:n] if refs[p].flagged]
        print("\n[%s n=%d %s] rho %.2e .. %.2e; single pass would flag pairs %s of the first call%s" % (
            path, n, family, min(r.rho for r in refs), max(r.rho for r in refs), flagged,
            "" if (path == "split_single") else " (not this path)"))
        for thr in thrs:
            dm.SetThreshold(thr)
            worst, ambiguous = 0.0, 0
            for c0 in range(0, len(order), n):
                idx = order[c0:c0 + n]
                cnt, lists = _run(dm, [fam[p][0] for p in idx], [fam[p][1] for p in idx])
                for k, p in enumerate(idx):
                    ambiguous += _check(refs[p], cnt[k], lists[k], thr, tag="%s/%s n=%d thr=%g pair %d" % (path, family, n, thr, p))
                if c0 == 0:
                    worst = _check_conf(refs[idx[0]], dm.conf_matrix(), tag="%s/%s thr=%g" % (path, family, thr))
            print("  thr %-7g worst |dconf| of pair 0 %.2e, %d entries inside the band" % (thr, worst, ambiguous))
        # threshold bracketing around chosen entries of the first and the last pair of the first call
        floor = 0.05 if path != "dense_head" else 1e-6
        for p in sorted({order[0], order[n - 1]}):
            r = refs[p]
            for e in _brackets(r, floor):
                c = r.conf[e]
                for thr, listed in ((c * np.exp(-2 * r.rho), True), (c * np.exp(2 * r.rho), False)):
                    dm.SetThreshold(float(thr))
                    idx = order[:n]
                    cnt, lists = _run(dm, [fam[q][0] for q in idx], [fam[q][1] for q in idx])
                    k = idx.index(p)
                    assert cnt[k] <= CAP, (path, family, p, cnt[k])
                    _check(r, cnt[k], lists[k], float(np.float32(thr)), tag="bracket %s/%s pair %d" % (path, family, p))
                    have = set(map(tuple, _to_ij(lists[k]).tolist()))
                    assert (tuple(int(x) for x in e) in have) == listed, (path, family, p, e, c, thr)


def test_mixed_batch_flags_some_pairs_and_lists_do_not_depend_on_the_batch(monkeypatch):
    """24 pairs, those at 0, 7 (one token 50x the others' norm), 8 and 23 trip the single pass's range check, the others
    do not; each pair's list is bit-identical in a differently composed batch, and matches the reference."""
    fam, refs = _refs("mixed")
    flags = [r.flagged for r in refs]
    assert all(r.clear for r in refs)
    assert [p for p in range(24) if flags[p]] == [0, 7, 8, 23], flags
    dm = _handle(monkeypatch, 24)
    for thr in SPARSE_THR + DENSE_THR:
        dm.SetThreshold(thr)
        cnt, lists = _run(dm, [f[0] for f in fam], [f[1] for f in fam])
        other = [23, 8, 7, 0, 3, 12, 19, 1, 5]       # flagged and unflagged pairs in another batch of 9
        cnt2, lists2 = _run(dm, [fam[p][0] for p in other], [fam[p][1] for p in other])
        for k, p in enumerate(other):
            assert cnt2[k] == cnt[p]
            np.testing.assert_array_equal(lists2[k], lists[p])
        for p in range(24):
            _check(refs[p], cnt[p], lists[p], thr, tag="mixed pair %d thr %g" % (p, thr))


def test_flat_features_count_exactly_with_a_small_cap(monkeypatch):
    """all-zero features and equal tokens: conf = 1 / 1200^2 everywhere; none at thr >= 0.05, all 1 440 000 at
    thr = 6.9e-7 (dense head), n_out exact, the list its row-major first cap entries"""
    fam, refs = _refs("flat")
    for path in ("split_few", "split_single", "f32"):
        counts, flags, env = PATHS[path]
        n = counts[-1]
        dm = _handle(monkeypatch, n, flags, env)
        F0 = [fam[p % len(fam)][0] for p in range(n)]
        F1 = [fam[p % len(fam)][1] for p in range(n)]
        dm.SetThreshold(0.05)
        cnt, _ = _run(dm, F0, F1)
        assert (cnt == 0).all(), (path, cnt)
        dm.SetThreshold(6.9e-7)
        cnt, lists = _run(dm, F0, F1, cap=64)
        assert (cnt == 1200 * 1200).all(), (path, cnt)
        first = np.stack([np.zeros(64, np.int64), np.arange(64)], 1)
        for lst in lists:
            np.testing.assert_array_equal(_to_ij(lst), first)
        print("\n[%s n=%d flat] n_out %s" % (path, n, sorted(set(cnt.tolist()))))


def test_ties_at_the_candidate_capacity(monkeypatch):
    """~20 tied candidates per row fill the sparse head's candidate list close to kCandCap; the marked rows' strong
    matches and n_out must equal the reference exactly (a truncated candidate list shows up as a missing match)"""
    fam, marked = _fam_ties()
    refs = [_Ref(f0, f1) for f0, f1 in fam]
    for path in ("split_few", "split_single", "split_running_max", "split_no_skip", "f32"):
        counts, flags, env = PATHS[path]
        for n in counts:
            dm = _handle(monkeypatch, n, flags, env)
            for thr in (0.05, 0.0501):
                dm.SetThreshold(thr)
                F0 = [fam[p % 2][0] for p in range(n)]
                F1 = [fam[p % 2][1] for p in range(n)]
                cnt, lists = _run(dm, F0, F1)
                for k in range(n):
                    r = refs[k % 2]
                    exp = np.argwhere(r.conf > thr)
                    hi, lo = r.band(thr)
                    assert ((r.conf > lo) == (r.conf > hi)).all()        # no reference entry inside the band
                    assert cnt[k] == len(exp), (path, n, thr, k, cnt[k], len(exp))
                    np.testing.assert_array_equal(_to_ij(lists[k]), exp)
                if n == counts[-1]:
                    print("\n[%s n=%d ties thr=%g] n_out %s" % (path, n, thr, sorted(set(cnt.tolist()))))
    # the construction does what it says: ~20 candidates per row at 0.05, 40 strong matches in pair 0
    r = refs[0]
    sm = np.exp(r.s - r.s.max(1, keepdims=True))
    sm /= sm.sum(1, keepdims=True)
    per_row = (sm >= 0.05 * np.exp(-1e-2)).sum(1)
    assert per_row.max() <= 21 and per_row.sum() > 15000, per_row.sum()
    assert len(np.argwhere(r.conf > 0.05)) == len(marked)


def test_entry_is_bit_identical_to_match(monkeypatch):
    """Fidelity: the features match() kept, fed back through head_device, give the same list and confidence matrix bit
    for bit -- split handle at n = 1 and n = 8 (8 copies of the pair), exact-f32 handle at n = 1."""
    from mono_slam_framework_amd import synth
    a, b = synth.synth_pair(5, 640, 480, mode=1)
    frames = [(GOLD["img0_ii"], GOLD["img1_ii"]), (a, b)]
    for flags, n in ((0, 1), (0, 8), ("f32", 1)):
        dm = _handle(monkeypatch, n, flags, thr=0.1)
        for fa, fb in frames:
            if n == 1:
                ref_list = [dm.MatchFrames(fa, fb, cap=8192)]
            else:
                ref_list = dm.match_batch([fa] * n, [fb] * n, cap=8192)
            conf = dm.conf_matrix().copy()
            feat = dm.coarse_features().copy()
            import torch
            d0 = torch.from_numpy(np.repeat(feat[0][None], n, 0)).cuda()
            d1 = torch.from_numpy(np.repeat(feat[1][None], n, 0)).cuda()
            out = torch.zeros((n, 8192, 4), dtype=torch.int32, device="cuda")
            cnt = torch.zeros((n,), dtype=torch.int32, device="cuda")
            dm.head_device(d0, d1, out, cnt)
            out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
            assert len(ref_list[0]) > 10
            for k in range(n):
                assert cnt[k] == len(ref_list[k])
                np.testing.assert_array_equal(out[k, :cnt[k]], ref_list[k])
            assert np.array_equal(dm.conf_matrix().view(np.uint32), conf.view(np.uint32))
            np.testing.assert_array_equal(dm.coarse_features(), feat)
            print("\n[fidelity %s n=%d] %d matches, conf bit-identical" % (flags or "split", n, len(ref_list[0])))


def test_entry_rejects_bad_arguments(monkeypatch):
    import torch
    from mono_slam_framework_amd import _lib
    from mono_slam_framework_amd.matcher import FeatureMatcher, MsfError
    dm = _handle(monkeypatch, 2)
    f = torch.zeros((3, 1200, 32), dtype=torch.float32, device="cuda")
    out = torch.zeros((3, 16, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros((3,), dtype=torch.int32, device="cuda")
    with pytest.raises(MsfError) as e:                   # n_pairs > max_batch_pairs
        dm.head_device(f, f, out, cnt)
    assert e.value.code == _lib.MSF_ERR_INVALID_ARG
    L, h = dm._L, dm._h
    fb = torch.zeros((2 * 1200 * 32 + 4,), dtype=torch.float32, device="cuda")
    rc = L.msf_debug_loftr_head(h, 2, fb.data_ptr() + 4, fb.data_ptr() + 4, out.data_ptr(), 16, cnt.data_ptr(), None)
    assert rc == _lib.MSF_ERR_INVALID_ARG                # features not 16-byte aligned
    orb = FeatureMatcher()
    rc = L.msf_debug_loftr_head(orb._h, 1, f.data_ptr(), f.data_ptr(), out.data_ptr(), 16, cnt.data_ptr(), None)
    assert rc == _lib.MSF_ERR_INVALID_ARG                # not a LoFTR handle
    # the entry is not a match call: the stage-timing ring stays empty
    prof = _handle(monkeypatch, 2, _lib.MSF_FLAG_PROFILE)
    prof.head_device(f[:2].contiguous(), f[:2].contiguous(), out[:2].contiguous(), cnt[:2].contiguous())
    assert prof.stage_times() == {}
