"""TEST INFRASTRUCTURE ONLY -- reference side of the reconstruction tests (test_reconstruct_ref.py,
test_reconstruct_host.py, test_reconstruct_gpu.py), written from slam_pipeline/src/Initializer.cc:489-934 as a
specification: ReconstructF / ReconstructH, DecomposeE, Triangulate, CheckRT and the two selection rules, with
numpy.linalg.svd, on the f32 inputs as given.

  reconstruct(...)         the whole tail in float64 (dtype=np.float32: the same chain in numpy float32, cosParallax in f64
                           from the f32 vectors -- only to measure the f64 / f32 spread)
  pick_f / pick_h          the selection rules alone, literally
  case(kind, seed)         the nine scenes: matches, the best-of-200 model of each kind, its inliers, RH
  compare_candidates / compare_flags / triangulation_figures   the bars, as (value, bound) figures

Nothing here is code under test and nothing here is imported by the product package."""
import functools

import numpy as np

from oracle import initializer as oracle_init
from tests import ransac_ref as rr

EPS = rr.EPS
K = np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], np.float32)
SIGMA = 1.0
MIN_TRIANGULATED = 50
MIN_PARALLAX = 1.0
KINDS = ("planar", "two_view", "wide")
CASES = [(k, s) for k in KINDS for s in rr.SEEDS]
EXPECT_OK = {("planar", 1): 1, ("planar", 2): 1, ("planar", 3): 1, ("two_view", 1): 0, ("two_view", 2): 0,
             ("two_view", 3): 0, ("wide", 1): 0, ("wide", 2): 1, ("wide", 3): 1}
# nGood of the winner over the runner-up on every ok = 1 case, so that the reference's first-strict-maximum tie rule
# decides nothing.  The winners count 213 / 200 / 210 (planar) and 181 / 216 (wide), the planar runners-up 127-132:
# the margins are 81, 73, 81, 181, 216, and 68 = 200 - 132 is what those figures guarantee.  (A margin of 80 does not
# hold for planar seed 2.)  Borderline matches could move a count by 4 at the most.
MIN_WINNER_MARGIN = 68
MAX_BORDERLINE_SHARE = 0.03     # of a candidate's inliers; a condition on the inputs
WIDE_A, WIDE_T = 0.15, np.array([1.5, 0.15, 0.3])

# Parallax bar: twice the largest |parallax32 - parallax64| (degrees) between the float64 and the numpy-float32 run of
# reconstruct() over all cases and candidates with nGood > 0 in both.  test_reconstruct_ref.py recomputes the spread,
# prints it, writes it to profiles/reconstruct_bars.txt and asserts it is no larger than the figure pasted here.
# Measured 2026-10-18: 5.791e-05 degrees (planar seed 1, a runner-up candidate at 1.13 degrees; profiles/reconstruct_bars.txt).
MEASURED_PARALLAX_SPREAD = 5.8e-05
PARALLAX_BAR = 2 * MEASURED_PARALLAX_SPREAD


def wide_scene(seed, n=rr.N_MATCHES, out_frac=0.3):
    """ransac_ref.two_view_scene's recipe with a 1.5-unit baseline and 0.15 rad about y -> (matches, outlier mask)"""
    r = np.random.RandomState(seed)
    X = np.c_[r.uniform(-2, 2, n), r.uniform(-1.5, 1.5, n), r.uniform(3, 9, n)]
    K64 = K.astype(np.float64)
    a = WIDE_A
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    x1 = X @ K64.T
    x2 = (X @ R.T + WIDE_T) @ K64.T
    return rr._finish(x1[:, :2] / x1[:, 2:], x2[:, :2] / x2[:, 2:], r, out_frac)


def planted_f(kind):
    """the F21 the two-view scenes plant: K^-T [t]x R K^-1"""
    a, t = (0.08, np.array([0.5, 0.05, 0.1])) if kind == "two_view" else (WIDE_A, WIDE_T)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K.astype(np.float64))
    return (Ki.T @ tx @ R @ Ki).astype(np.float32), R, t / np.linalg.norm(t)


def scene(kind, seed, **kw):
    return wide_scene(seed, **kw) if kind == "wide" else rr.scene(kind, seed, **kw)


@functools.lru_cache(maxsize=None)
def case(kind, seed):
    """-> dict: matches int32 [300, 4], bad (planted outliers), sets, and per model name "H" / "F": m21 f32 [3, 3] (the
    best of 200 float64-solved hypotheses, scored as CheckHomography / CheckFundamental score), inliers bool [300],
    score; RH; model (the one Initialize reconstructs from)"""
    m, bad = scene(kind, seed)
    sets = rr.draw_sets(len(m), rr.N_HYP, seed)
    H21, H12, F21 = rr.solve64(m, sets)
    out = dict(matches=m, bad=bad, sets=sets)
    for name, model, a, b in (("H", 0, H21, H12), ("F", 1, F21, None)):
        best, scores, inl = oracle_init.find_best(model, a, b, m, SIGMA)
        assert best >= 0
        out[name] = dict(m21=a[best].copy(), inliers=inl, score=np.float32(scores[best]))
    out["RH"] = float(out["H"]["score"] / np.float32(out["H"]["score"] + out["F"]["score"]))
    out["model"] = 0 if out["RH"] > 0.40 else 1
    return out


# ---- the reference ----
def decompose_e(F21, Kd, dtype):
    """-> ([(R, t)] x 4 in the reference's order, singular values of E21)"""
    E = Kd.T @ F21.astype(dtype) @ Kd
    u, w, vt = np.linalg.svd(E)
    t = u[:, 2] / np.linalg.norm(u[:, 2])
    W = np.zeros((3, 3), dtype)
    W[0, 1], W[1, 0], W[2, 2] = -1, 1, 1
    R1 = u @ W @ vt
    if np.linalg.det(R1) < 0:
        R1 = -R1
    R2 = u @ W.T @ vt
    if np.linalg.det(R2) < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)], w


def decompose_h(H21, Kd, dtype):
    """-> ([(R, t, n)] x 8 or None for the early return, singular values of A)"""
    A = np.linalg.inv(Kd) @ H21.astype(dtype) @ Kd
    U, w, Vt = np.linalg.svd(A)
    V = Vt.T
    s = dtype(np.linalg.det(U) * np.linalg.det(Vt))
    d1, d2, d3 = w
    with np.errstate(all="ignore"):
        if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
            return None, w
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
    out = []
    for i in range(4):
        Rp = np.eye(3, dtype=dtype)
        Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[i], st[i], ct
        tp = np.array([x1[i], 0, -x3[i]], dtype) * (d1 - d3)
        out.append((Rp, tp, i))
    for i in range(4):
        Rp = np.eye(3, dtype=dtype)
        Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[i], -1, sp[i], -cp
        tp = np.array([x1[i], 0, x3[i]], dtype) * (d1 + d3)
        out.append((Rp, tp, i))
    cands = []
    for Rp, tp, i in out:
        R = s * U @ Rp @ Vt
        t = U @ tp
        n = V @ np.array([x1[i], 0, x3[i]], dtype)
        if n[2] < 0:
            n = -n
        cands.append((R, t / np.linalg.norm(t), n))
    return cands, w


def triangulation_matrices(matches, Kd, R, t, dtype):
    """the 4 x 4 matrix of Triangulate for every match -> [n, 4, 4]"""
    m = np.asarray(matches).reshape(-1, 4).astype(dtype)
    P1 = np.zeros((3, 4), dtype)
    P1[:, :3] = Kd
    P2 = Kd @ np.c_[R, t].astype(dtype)
    return np.stack([m[:, 0:1] * P1[2] - P1[0], m[:, 1:2] * P1[2] - P1[1],
                     m[:, 2:3] * P2[2] - P2[0], m[:, 3:4] * P2[2] - P2[1]], 1)


def check_rt(R, t, matches, inliers, Kd, th2, dtype):
    """CheckRT -> dict: nGood, parallax (degrees, f32), counted / good / borderline bool [n], points [n, 3], cos [n]"""
    R, t = R.astype(dtype), t.astype(dtype)
    m = np.asarray(matches).reshape(-1, 4).astype(dtype)
    inl = np.asarray(inliers, bool)
    n = len(m)
    fx, fy, cx, cy = Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2]
    th2 = dtype(th2)
    O2 = -R.T @ t
    with np.errstate(all="ignore"):
        A = triangulation_matrices(matches, Kd, R, t, dtype)
        ok_rows = np.isfinite(A).all((1, 2))
        vt = np.full((n, 4), np.nan, dtype)
        if ok_rows.any():
            vt[ok_rows] = np.linalg.svd(A[ok_rows])[2][:, 3]
        p = (vt[:, :3] / vt[:, 3:]).astype(dtype)
        finite = np.isfinite(p).all(1)
        p64 = p.astype(np.float64)
        n2 = (p - O2).astype(np.float64)
        dist1, dist2 = np.linalg.norm(p64, axis=1), np.linalg.norm(n2, axis=1)
        cos = (p64 * n2).sum(1) / (dist1 * dist2)
        p2 = (p @ R.T + t).astype(dtype)
        z1, z2 = p[:, 2], p2[:, 2]
        inv1, inv2 = dtype(1) / z1, dtype(1) / z2
        e1 = (fx * p[:, 0] * inv1 + cx - m[:, 0]) ** 2 + (fy * p[:, 1] * inv1 + cy - m[:, 1]) ** 2
        e2 = (fx * p2[:, 0] * inv2 + cx - m[:, 2]) ** 2 + (fy * p2[:, 1] * inv2 + cy - m[:, 3]) ** 2
        low = cos < 0.99998
        near_cos = np.abs(cos - 0.99998) <= 1e-6
        alive = inl & finite
        border = np.zeros(n, bool)
        # the stages in the reference's order; a match a stage rejects decisively is not borderline at a later one
        for z, norm in ((z1, dist1), (z2, np.linalg.norm(p2.astype(np.float64), axis=1))):
            border |= alive & ((np.abs(z) <= 1e-3 * norm) | (near_cos & (z <= 0)))
            alive = alive & ~((z <= 0) & low)
        for e in (e1, e2):
            border |= alive & (np.abs(e - th2) <= 0.01 * th2)
            alive = alive & ~(e > th2)
        border |= alive & near_cos
    counted = alive
    good = counted & low
    nGood = int(counted.sum())
    if nGood > 0:
        srt = np.sort(cos[counted])
        parallax = np.float32(np.arccos(srt[min(50, nGood - 1)]) * 180 / np.pi)
    else:
        parallax = np.float32(0)
    pts = np.where(counted[:, None], p, 0).astype(np.float32)
    return dict(nGood=nGood, parallax=parallax, counted=counted, good=good, borderline=border, points=pts, cos=cos)


def pick_f(nGood, parallax, N, min_triangulated, min_parallax):
    """ReconstructF :524-582 -> candidate index or -1"""
    maxGood = max(nGood)
    nMinGood = max(int(0.9 * N), min_triangulated)
    nsimilar = sum(1 for g in nGood if g > 0.7 * maxGood)
    if maxGood < nMinGood or nsimilar > 1:
        return -1
    for k in range(4):
        if maxGood == nGood[k]:
            return k if parallax[k] > min_parallax else -1
    return -1


def pick_h(nGood, parallax, N, min_triangulated, min_parallax):
    """ReconstructH :700-741 -> candidate index or -1"""
    bestGood, bestIdx, bestParallax = 0, 0, np.float32(-1)
    for k in range(8):
        if nGood[k] > bestGood:
            bestGood, bestIdx, bestParallax = nGood[k], k, parallax[k]
    minGood = min(int(0.9 * N), min_triangulated)
    return bestIdx if bestParallax >= min_parallax and bestGood >= minGood else -1


def reconstruct(model, m21, matches, inliers, Kf=K, sigma=SIGMA, min_triangulated=MIN_TRIANGULATED,
                min_parallax=MIN_PARALLAX, dtype=np.float64):
    """ReconstructH (model 0) / ReconstructF (model 1) -> dict: ok, winner, N, w (singular values), early (H's early
    return), cands [(R, t)], checks [check_rt dict per candidate]"""
    Kd = np.asarray(Kf, np.float32).astype(dtype)
    m21 = np.asarray(m21, np.float32).reshape(3, 3)
    inliers = np.asarray(inliers, bool)
    N = int(inliers.sum())
    if model == 1:
        cands, w = decompose_e(m21, Kd, dtype)
    else:
        cands, w = decompose_h(m21, Kd, dtype)
    out = dict(model=model, N=N, w=np.asarray(w, np.float64), early=cands is None, cands=[], checks=[], winner=-1, ok=0)
    if cands is None:
        return out
    th2 = 4.0 * sigma * sigma
    out["cands"] = [(c[0], c[1]) for c in cands]
    out["checks"] = [check_rt(c[0], c[1], matches, inliers, Kd, th2, dtype) for c in cands]
    nGood = [c["nGood"] for c in out["checks"]]
    par = [c["parallax"] for c in out["checks"]]
    pick = pick_f if model == 1 else pick_h
    out["winner"] = pick(nGood, par, N, min_triangulated, np.float32(min_parallax))
    out["ok"] = int(out["winner"] >= 0)
    return out


@functools.lru_cache(maxsize=None)
def case_reference(kind, seed, f32=False):
    """reconstruct() of the model Initialize picks for the case; computed once and shared: do not modify"""
    c = case(kind, seed)
    name = "H" if c["model"] == 0 else "F"
    return reconstruct(c["model"], c[name]["m21"], c["matches"], c[name]["inliers"],
                       dtype=np.float32 if f32 else np.float64)


# ---- the bars, as figures ----
def candidate_bound(model, w):
    """16 eps s1 / min(d1 - d2, d2 - d3) for H, 16 eps s1 / (s2 - s3) for E"""
    w = np.asarray(w, np.float64)
    gap = min(w[0] - w[1], w[1] - w[2]) if model == 0 else w[1] - w[2]
    return 16 * EPS * w[0] / gap


def compare_candidates(ref, cand_R, cand_t):
    """Matches every candidate (R [k, 3, 3], t [k, 3]) to its nearest reference candidate.
    -> (perm: perm[i] = reference index of candidate i, worst max(|R - R64|, |t - t64|), bound); asserts a bijection"""
    cand_R = np.asarray(cand_R, np.float64).reshape(-1, 3, 3)
    cand_t = np.asarray(cand_t, np.float64).reshape(-1, 3)
    assert len(cand_R) == len(ref["cands"]), (len(cand_R), len(ref["cands"]))
    perm, worst = [], 0.0
    for R, t in zip(cand_R, cand_t):
        d = [max(np.abs(R - Rr).max(), np.abs(t - tr).max()) for Rr, tr in ref["cands"]]
        perm.append(int(np.argmin(d)))
        worst = max(worst, float(min(d)))
    assert sorted(perm) == list(range(len(perm))), perm
    return perm, worst, candidate_bound(ref["model"], ref["w"])


def compare_flags(ref_check, inliers, counted, good, n_good):
    """non-borderline inlier matches agree exactly; nGood differs by at most the number of borderline matches; the cap
    on the borderline share is a condition on the inputs -> number of borderline matches"""
    inl = np.asarray(inliers, bool)
    b = ref_check["borderline"]
    assert b.sum() <= MAX_BORDERLINE_SHARE * max(int(inl.sum()), 1), (int(b.sum()), int(inl.sum()))
    keep = ~b
    np.testing.assert_array_equal(np.asarray(counted, bool)[keep], ref_check["counted"][keep])
    np.testing.assert_array_equal(np.asarray(good, bool)[keep], ref_check["good"][keep])
    assert abs(int(n_good) - ref_check["nGood"]) <= int(b.sum())
    return int(b.sum())


def triangulation_figures(matches, Kf, R, t, hom, rows):
    """The step alone: the float64 null vector of the 4 x 4 matrices built from the given (device) R, t against hom
    [n, 4] on `rows`.  -> (err / bound per informative row, number of uninformative rows)"""
    Kd = np.asarray(Kf, np.float32).astype(np.float64)
    A = triangulation_matrices(matches, Kd, np.asarray(R, np.float32).reshape(3, 3).astype(np.float64),
                               np.asarray(t, np.float32).astype(np.float64), np.float64)[rows]
    hom = np.asarray(hom, np.float64).reshape(-1, 4)[rows]
    hom = hom / np.linalg.norm(hom, axis=1, keepdims=True)
    _, s, vt = np.linalg.svd(A)
    v = vt[:, 3]
    err = np.minimum(np.linalg.norm(hom - v, axis=1), np.linalg.norm(hom + v, axis=1))
    bound = 16 * EPS * s[:, 0] / (s[:, 2] - s[:, 3])
    informative = bound <= rr.UNINFORMATIVE
    return err[informative] / bound[informative], int((~informative).sum())


def parallax_spread():
    """largest |parallax32 - parallax64| over all cases and candidates counted in both runs, candidates paired by (R, t)"""
    worst = 0.0
    for kind, seed in CASES:
        r64, r32 = case_reference(kind, seed), case_reference(kind, seed, True)
        if not r64["cands"]:
            continue
        perm, _, _ = compare_candidates(r64, [c[0] for c in r32["cands"]], [c[1] for c in r32["cands"]])
        for i, j in enumerate(perm):
            a, b = r32["checks"][i], r64["checks"][j]
            if a["nGood"] > 0 and b["nGood"] > 0:
                worst = max(worst, abs(float(a["parallax"]) - float(b["parallax"])))
    return worst


def check_result(ref, got, matches, inliers, Kf=K, label="", selection=True):
    """Every bar on one result (host build or device) against `ref` = reconstruct(...) in float64; prints each figure
    before it asserts.  got: ok, winner, n_cand, cand_R [k, 3, 3], cand_t [k, 3], cand_good [k], cand_parallax [k], and
    optionally w [3] (singular values), flags [k, n] (bit 0 counted, bit 1 vbGood), hom [k, n, 4] (null vectors before the
    division), points [n, 3] + triangulated [n] (the winner's vP3D / vbTriangulated).  -> perm (reference index of each
    candidate).  selection=False: candidates, counts, flags and parallax only -- for inputs made to exercise a count,
    where two candidates tie and the reference's first-come tie rule says nothing across candidate orders."""
    inl = np.asarray(inliers, bool)
    k = len(ref["cands"])
    assert int(got["n_cand"]) == k, (label, got["n_cand"], k)
    if got.get("w") is not None and np.isfinite(ref["w"]).all():
        dw = np.abs(np.asarray(got["w"], np.float64) - ref["w"]).max()
        print("%s: singular values off by %.3e (bound %.3e)" % (label, dw, 16 * EPS * ref["w"][0]))
        assert dw <= 16 * EPS * ref["w"][0]
    if k == 0:
        assert int(got["ok"]) == 0 and int(got["winner"]) == -1
        return []
    perm, worst, bound = compare_candidates(ref, np.asarray(got["cand_R"])[:k], np.asarray(got["cand_t"])[:k])
    print("%s: candidates off by %.3e (bound %.3e)" % (label, worst, bound))
    assert worst <= bound
    # the reference's tie rules (first strict maximum, first equal) cannot be compared across candidate orders: the
    # inputs must leave a strict winner by more than the borderline matches could move
    goods = sorted(c["nGood"] for c in ref["checks"])
    most_borderline = max(int(c["borderline"].sum()) for c in ref["checks"])
    assert not selection or goods[-1] == 0 or goods[-1] - goods[-2] > 2 * most_borderline, (label, goods, most_borderline)
    tri_worst, uninformative, n_rows = 0.0, 0, 0
    for i, j in enumerate(perm):
        chk = ref["checks"][j]
        nb = int(chk["borderline"].sum())
        assert nb <= MAX_BORDERLINE_SHARE * max(int(inl.sum()), 1)
        good_i, par_i = int(got["cand_good"][i]), float(got["cand_parallax"][i])
        print("%s: candidate %d (reference %d): nGood %d (%d, %d borderline), parallax %.6f (%.6f, bar %.2e)"
              % (label, i, j, good_i, chk["nGood"], nb, par_i, float(chk["parallax"]), PARALLAX_BAR))
        assert abs(good_i - chk["nGood"]) <= nb
        if good_i == chk["nGood"]:      # the same multiset size: the same rank is selected
            assert abs(par_i - float(chk["parallax"])) <= PARALLAX_BAR
        if got.get("flags") is not None:
            f = np.asarray(got["flags"])[i]
            compare_flags(chk, inl, (f & 1) != 0, (f & 2) != 0, good_i)
        if got.get("hom") is not None and inl.any():
            rows = np.flatnonzero(inl)
            ratio, unin = triangulation_figures(matches, Kf, np.asarray(got["cand_R"])[i], np.asarray(got["cand_t"])[i],
                                                np.asarray(got["hom"])[i], rows)
            tri_worst = max(tri_worst, float(ratio.max()) if len(ratio) else 0.0)
            uninformative += unin
            n_rows += len(rows)
    if n_rows:
        print("%s: triangulation worst err / bound %.3f; uninformative bounds %d of %d" % (label, tri_worst, uninformative, n_rows))
        assert uninformative <= rr.MAX_UNINFORMATIVE_SHARE * n_rows
        assert tri_worst <= 1.0
    if not selection:
        return perm
    # selection: ok and the winner's identity by its (R, t)
    assert int(got["ok"]) == ref["ok"], (label, got["ok"], ref["ok"])
    if ref["ok"]:
        assert perm[int(got["winner"])] == ref["winner"]
    else:
        assert int(got["winner"]) == -1
    if got.get("points") is not None:
        pts, tri = np.asarray(got["points"]), np.asarray(got["triangulated"], bool)
        if ref["ok"]:
            wi = int(got["winner"])
            chk = ref["checks"][ref["winner"]]
            compare_flags(chk, inl, (pts != 0).any(1), tri, int(got["cand_good"][wi]))
            rows = np.flatnonzero((pts != 0).any(1))
            hom = np.c_[pts, np.ones(len(pts))]
            ratio, unin = triangulation_figures(matches, Kf, np.asarray(got["cand_R"])[wi], np.asarray(got["cand_t"])[wi],
                                                hom, rows)
            print("%s: winner's points: worst err / bound %.3f; uninformative %d of %d" % (label, ratio.max(), unin, len(rows)))
            assert unin <= rr.MAX_UNINFORMATIVE_SHARE * len(rows) and ratio.max() <= 1.0
        else:
            assert not pts.any() and not tri.any()
    return perm
