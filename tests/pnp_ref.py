"""float64 numpy restatement of PnPsolver (slam_pipeline/src/PnPsolver.cc), stage by stage, each stage callable alone
and batched over a leading axis H of hypotheses; the scenes and the checks (bars 1..6 of test_pnp_gpu.py) that the
host build of csrc/pnp_solve.h and the device are both held to.

The upstream half ends at the basis: control_points, barycentric, fill_m, and basis_eigh (numpy.linalg.eigh of M'M).
The downstream half is epnp_from(cws, ut_tail, pw, us, K): it takes control points and basis as given, because a
minimum set leaves a 4-dimensional null space whose basis belongs to whoever computed it (see csrc/pnp_solve.h).

The restatement keeps the defined divergences of pnp_solve.h: rep_errors[n] instead of rep_errors[N], a singular
qr_solve step adds zero, singular values at or below 2 eps sum(w) are dropped by the pseudo-inverse / least squares."""
import numpy as np

EPS = 2.0 ** -52
TH2 = np.float32(5.991)
N_SCENE = 96
N_ITERATIONS = 35
KINDS = ("base", "wide", "shallow", "few")
CASES = [(kind, seed) for kind in KINDS for seed in (1, 2, 3)]
PERTURB = 16 * EPS
ILL_CONDITIONED = 1e-6          # a hypothesis whose reference moves by more under PERTURB is left out of bar 3
MAX_LEFT_OUT = 0.01
BAND = 1e-9                     # |error2 - th2| <= BAND th2: the flag may go either way (bar 4)
MAX_IN_BAND = 1e-4

# Bar 3: twice the worst change of epnp_from's own (R, t) when cws and ut_tail are perturbed elementwise by 16 eps
# relative, over all hypotheses of CASES that are not ill-conditioned.  tests/test_pnp_ref.py measures it, prints it,
# writes it to profiles/pnp_bars.txt and asserts that it is no larger than the figure pasted here.
# Measured 2026-10-19, pasted unrounded: 8.221e-10 over 420 hypotheses, none left out, median 2.4e-13 (base seed 1 ... few seed 3).
MEASURED_POSE_SPREAD = 8.220808478398567e-10
POSE_BAR = 2 * MEASURED_POSE_SPREAD


# ---------------------------------------------------------------- scenes
def rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-angle, angle)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * k + (1 - np.cos(a)) * k @ k


def scene(kind, seed, n=N_SCENE):
    """-> dict: K (fx, fy, cx, cy) f32, p3d f32 [n, 3], p2d f32 [n, 2], R, t (the truth), outlier bool [n].
    A camera at a random pose, depths in [2, 8] (wide: [1, 30]; shallow: 5 % spread around 5), 2-D points truncated to
    integers as keyPoints1 are, 30 % replaced by random pixels (few: 55 %)."""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + seed + 17 * n)
    K = np.array([520.0, 515.0, 318.5, 242.25], np.float32)
    R, t = rotation(rng, 0.6), rng.uniform(-1.5, 1.5, 3)
    lo, hi = {"base": (2, 8), "wide": (1, 30), "shallow": (4.875, 5.125), "few": (2, 8)}[kind]
    uv = np.stack([rng.uniform(20, 620, n), rng.uniform(20, 460, n)], 1)
    depth = rng.uniform(lo, hi, n)
    xc = np.stack([(uv[:, 0] - K[2]) / K[0] * depth, (uv[:, 1] - K[3]) / K[1] * depth, depth], 1)
    p3d = ((xc - t) @ R).astype(np.float32)                      # R' (xc - t)
    cam = p3d.astype(np.float64) @ R.T + t
    p2d = np.floor(np.stack([K[2] + K[0] * cam[:, 0] / cam[:, 2], K[3] + K[1] * cam[:, 1] / cam[:, 2]], 1))
    outlier = rng.uniform(size=n) < (0.55 if kind == "few" else 0.30)
    p2d[outlier] = np.floor(np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1))[outlier]
    return dict(K=K, p3d=p3d, p2d=p2d.astype(np.float32), R=R, t=t, outlier=outlier)


def draw_sets(seed, n, n_iterations):
    """minimum sets without replacement from numpy's generator (the device's own draw is replayed from what it returns)"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.choice(n, 4, replace=False) for _ in range(n_iterations)]).astype(np.int32)


def set_ransac_parameters(n, probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5):
    """SetRansacParameters (:130-165) -> (mRansacMinInliers, mRansacMaxIts)"""
    epsilon = np.float32(epsilon)
    m = max(int(np.float32(n) * epsilon), min_inliers, min_set)
    if epsilon < np.float32(m) / np.float32(n):
        epsilon = np.float32(m) / np.float32(n)
    if m == n:
        its = 1
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.ceil(np.log(1 - probability) / np.log(1 - float(epsilon) ** 3))
        its = int(q) if np.isfinite(q) else -2 ** 31             # n below the floor: epsilon > 1, a NaN cast as x86 casts it
    return m, max(1, min(its, max_iterations))


# ---------------------------------------------------------------- small linear algebra
def _svd(a):
    """numpy's SVD over a batch; a matrix with a non-finite entry gives NaN factors instead of an exception"""
    bad = ~np.isfinite(a).all(axis=(-2, -1))
    u, w, vt = np.linalg.svd(np.where(bad[..., None, None], 0.0, a), full_matrices=False)
    for x in (u, w, vt):
        x[bad] = np.nan
    return u, w, vt


def _inverse_w(w):
    cut = 2 * EPS * w.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w > cut, 1.0 / w, np.where(np.isnan(w), np.nan, 0.0))


def pinv_cut(a):
    u, w, vt = _svd(a)
    return np.einsum("...ji,...j,...kj->...ik", vt, _inverse_w(w), u)


def lstsq_cut(a, b):
    u, w, vt = _svd(a)
    return np.einsum("...ji,...j,...kj,...k->...i", vt, _inverse_w(w), u, b)


# ---------------------------------------------------------------- upstream of the basis
def control_points(pw):
    """choose_control_points (:362-392): pw [H, n, 3] -> cws [H, 4, 3], the eigenvalues dc [H, 3] (descending)"""
    n = pw.shape[1]
    c0 = pw.sum(1) / n
    d = pw - c0[:, None]
    lam, vec = np.linalg.eigh(np.einsum("hni,hnj->hij", d, d))
    lam, vec = lam[:, ::-1], vec[:, :, ::-1]
    k = np.sqrt(np.maximum(lam, 0) / n)
    return np.concatenate([c0[:, None], c0[:, None] + k[:, :, None] * vec.transpose(0, 2, 1)], 1), lam


def pca_axes(pw):
    """eigh's unit axes of the points, rows by descending eigenvalue -> [H, 3, 3]"""
    d = pw - (pw.sum(1) / pw.shape[1])[:, None]
    return np.linalg.eigh(np.einsum("hni,hnj->hij", d, d))[1][:, :, ::-1].transpose(0, 2, 1)


def inverse3_extended(a):
    """the inverse of [H, 3, 3] by cofactors in extended precision, rounded once"""
    a = a.astype(np.longdouble)
    c = np.stack([np.cross(a[:, :, 1], a[:, :, 2]), np.cross(a[:, :, 2], a[:, :, 0]), np.cross(a[:, :, 0], a[:, :, 1])], 1)
    det = (a[:, :, 0] * c[:, 0]).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (c / det[:, None, None]).astype(np.float64)


def control_inverse(cws):
    """cvInvert(CC, CV_SVD).  Where no singular value is cut the pseudo-inverse is the inverse, and it is taken by
    cofactors in extended precision: LAPACK's SVD leaves eps cond(CC) in the alphas, which would use up bars that are
    sized by eps lambda_1 alone."""
    cc = (cws[:, 1:] - cws[:, :1]).transpose(0, 2, 1)            # cc[i][j - 1] = cws[j][i] - cws[0][i]
    _, w, _ = _svd(cc)
    with np.errstate(invalid="ignore"):
        full = (w > 2 * EPS * w.sum(-1, keepdims=True)).all(-1)
    return np.where(full[:, None, None], inverse3_extended(cc), pinv_cut(cc))


def barycentric(cws, pw):
    """compute_barycentric_coordinates (:394-414) -> alphas [H, n, 4]"""
    ci = control_inverse(cws)
    d = pw - cws[:, :1]
    # in the order the reference writes it: a nearly coplanar set makes these three products cancel
    a = ci[:, None, :, 0] * d[..., 0:1] + ci[:, None, :, 1] * d[..., 1:2] + ci[:, None, :, 2] * d[..., 2:3]
    return np.concatenate([(1.0 - a[..., 0] - a[..., 1] - a[..., 2])[..., None], a], -1)


def fill_m(alphas, us, K):
    """fill_M (:416-430) -> M [H, 2 n, 12]"""
    fu, fv, uc, vc = [float(x) for x in K]
    H, n, _ = alphas.shape
    m = np.zeros((H, n, 2, 4, 3))
    m[:, :, 0, :, 0] = alphas * fu
    m[:, :, 0, :, 2] = alphas * (uc - us[:, :, 0])[..., None]
    m[:, :, 1, :, 1] = alphas * fv
    m[:, :, 1, :, 2] = alphas * (vc - us[:, :, 1])[..., None]
    return m.reshape(H, 2 * n, 12)


def mtm_of(cws, pw, us, K):
    """M'M (cvMulTransposed): the products and the sum over the 2 n rows in extended precision, rounded once, so that the
    reference's own summation error (it grows with n) does not use up the bars that are sized by eps lambda_1"""
    m = fill_m(barycentric(cws, pw), us, K).astype(np.longdouble)
    return np.einsum("hri,hrj->hij", m, m).astype(np.float64)


def basis_eigh(mtm):
    """-> eigenvalues descending [H, 12], Ut [H, 12, 12] with rows in that order (row 11: the smallest)"""
    bad = ~np.isfinite(mtm).all(axis=(-2, -1))
    lam, vec = np.linalg.eigh(np.where(bad[:, None, None], 0.0, mtm))
    lam, ut = lam[:, ::-1].copy(), vec[:, :, ::-1].transpose(0, 2, 1).copy()
    lam[bad], ut[bad] = np.nan, np.nan
    return lam, ut


# ---------------------------------------------------------------- downstream of the basis
def compute_l(ut_tail):
    v = ut_tail[:, ::-1].reshape(-1, 4, 4, 3)                    # v[i] = row 11 - i; [H, i, control point, xyz]
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    dv = np.stack([v[:, :, a] - v[:, :, b] for a, b in pairs], 2)   # [H, 4, 6, 3]
    dot = lambda i, j: (dv[:, i] * dv[:, j]).sum(-1)             # [H, 6]
    return np.stack([dot(0, 0), 2 * dot(0, 1), dot(1, 1), 2 * dot(0, 2), 2 * dot(1, 2), dot(2, 2), 2 * dot(0, 3),
                     2 * dot(1, 3), 2 * dot(2, 3), dot(3, 3)], -1)   # [H, 6, 10]


def compute_rho(cws):
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    return np.stack([((cws[:, a] - cws[:, b]) ** 2).sum(-1) for a, b in pairs], -1)


def find_betas(which, l, rho):
    with np.errstate(invalid="ignore", divide="ignore"):
        if which == 0:
            b = lstsq_cut(l[:, :, [0, 1, 3, 6]], rho)
            neg = b[:, 0] < 0
            b0 = np.sqrt(np.where(neg, -b[:, 0], b[:, 0]))
            sign = np.where(neg, -1.0, 1.0)
            return np.stack([b0, sign * b[:, 1] / b0, sign * b[:, 2] / b0, sign * b[:, 3] / b0], -1)
        b = lstsq_cut(l[:, :, :3 if which == 1 else 5], rho)
        neg = b[:, 0] < 0
        b0 = np.sqrt(np.where(neg, -b[:, 0], b[:, 0]))
        b1 = np.where(neg, np.where(b[:, 2] < 0, np.sqrt(np.abs(b[:, 2])), 0.0), np.where(b[:, 2] > 0, np.sqrt(np.abs(b[:, 2])), 0.0))
        b0 = np.where(b[:, 1] < 0, -b0, b0)
        b2 = np.zeros_like(b0) if which == 1 else b[:, 3] / b0
        return np.stack([b0, b1, b2, np.zeros_like(b0)], -1)


def qr_solve(A, b):
    """qr_solve (:812-901) of [H, 6, 4] systems, literally: the pivot scan stops one row short of the end; a singular
    matrix gives x = 0"""
    A, b = A.copy(), b.copy()
    H, nr, nc = A.shape
    A1, A2 = np.zeros((H, nc)), np.zeros((H, nc))
    singular = np.zeros(H, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(nc):
            eta = np.abs(A[:, k, k])
            for i in range(k + 1, nr):
                elt = np.abs(A[:, i - 1, k])
                eta = np.where(eta < elt, elt, eta)
            singular |= eta == 0
            inv_eta = 1.0 / eta
            total = np.zeros(H)
            for i in range(k, nr):
                A[:, i, k] *= inv_eta
                total = total + A[:, i, k] * A[:, i, k]
            sigma = np.sqrt(total)
            sigma = np.where(A[:, k, k] < 0, -sigma, sigma)
            A[:, k, k] += sigma
            A1[:, k] = sigma * A[:, k, k]
            A2[:, k] = -eta * sigma
            for j in range(k + 1, nc):
                total = np.zeros(H)
                for i in range(k, nr):
                    total = total + A[:, i, k] * A[:, i, j]
                tau = total / A1[:, k]
                for i in range(k, nr):
                    A[:, i, j] -= tau * A[:, i, k]
        for j in range(nc):
            tau = np.zeros(H)
            for i in range(j, nr):
                tau = tau + A[:, i, j] * b[:, i]
            tau = tau / A1[:, j]
            for i in range(j, nr):
                b[:, i] -= tau * A[:, i, j]
        x = np.zeros((H, nc))
        x[:, nc - 1] = b[:, nc - 1] / A2[:, nc - 1]
        for i in range(nc - 2, -1, -1):
            total = np.zeros(H)
            for j in range(i + 1, nc):
                total = total + A[:, i, j] * x[:, j]
            x[:, i] = (b[:, i] - total) / A2[:, i]
    x[singular] = 0.0
    return x


def gauss_newton(l, rho, betas):
    betas = betas.copy()
    idx = [(0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2), (0, 3), (1, 3), (2, 3), (3, 3)]
    for _ in range(5):
        A = np.zeros(l.shape[:2] + (4,))
        val = np.zeros(l.shape[:2])
        for c, (i, j) in enumerate(idx):
            val = val + l[:, :, c] * (betas[:, i] * betas[:, j])[:, None]
            if i == j:
                A[:, :, i] += 2 * l[:, :, c] * betas[:, i, None]
            else:
                A[:, :, i] += l[:, :, c] * betas[:, j, None]
                A[:, :, j] += l[:, :, c] * betas[:, i, None]
        betas = betas + qr_solve(A, rho - val)
    return betas


def project(pose, pw, K):
    """-> ue, ve [H, n] of pose [H, 3, 4] on pw [H, n, 3]"""
    fu, fv, uc, vc = [float(x) for x in K]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        cam = np.einsum("hij,hnj->hni", pose[:, :, :3], pw) + pose[:, None, :, 3]
        inv = 1.0 / cam[..., 2]
        return uc + fu * cam[..., 0] * inv, vc + fv * cam[..., 1] * inv


def compute_r_and_t(cws, alphas, ut_tail, betas, pw, us, K):
    """compute_R_and_t (:614-624) -> pose [H, 3, 4], the reprojection error [H]"""
    ccs = np.einsum("hi,hik->hk", betas, ut_tail[:, ::-1]).reshape(-1, 4, 3)
    pcs = np.einsum("hnj,hjk->hnk", alphas, ccs)
    pcs = np.where((pcs[:, 0, 2] < 0)[:, None, None], -pcs, pcs)
    n = pw.shape[1]
    pc0, pw0 = pcs.sum(1) / n, pw.sum(1) / n
    abt = np.einsum("hnj,hnk->hjk", pcs - pc0[:, None], pw - pw0[:, None])
    u, w, vt = _svd(abt)
    R = u @ vt
    with np.errstate(invalid="ignore"):
        neg = np.linalg.det(np.nan_to_num(R)) < 0
    R[neg, 2] = -R[neg, 2]
    t = pc0 - np.einsum("hij,hj->hi", R, pw0)
    pose = np.concatenate([R, t[..., None]], -1)
    ue, ve = project(pose, pw, K)
    with np.errstate(invalid="ignore"):
        rep = np.sqrt((us[..., 0] - ue) ** 2 + (us[..., 1] - ve) ** 2).sum(1) / n
    return pose, rep


def epnp_from(cws, ut_tail, pw, us, K):
    """compute_pose behind cvSVD (:471-499), given control points [H, 4, 3] and rows 8..11 of Ut [H, 4, 12];
    pw [H, n, 3], us [H, n, 2] float64.  -> dict: pose [H, 3, 4], betas [H, 3, 4], rep [H, 3], chosen [H]"""
    alphas = barycentric(cws, pw)
    l, rho = compute_l(ut_tail), compute_rho(cws)
    poses, reps, betas = [], [], []
    for which in range(3):
        b = gauss_newton(l, rho, find_betas(which, l, rho))
        pose, rep = compute_r_and_t(cws, alphas, ut_tail, b, pw, us, K)
        poses.append(pose), reps.append(rep), betas.append(b)
    rep = np.stack(reps, -1)
    with np.errstate(invalid="ignore"):
        chosen = np.where(rep[:, 1] < rep[:, 0], 1, 0)
        chosen = np.where(rep[:, 2] < np.take_along_axis(rep, chosen[:, None], 1)[:, 0], 2, chosen)
    pose = np.stack(poses, 1)[np.arange(len(chosen)), chosen]
    return dict(pose=pose, betas=np.stack(betas, 1), rep=rep, chosen=chosen, poses=np.stack(poses, 1))


def epnp(pw, us, K):
    """the whole compute_pose with eigh's basis -> epnp_from's dict plus cws, ut_tail, lam"""
    cws, _ = control_points(pw)
    lam, ut = basis_eigh(mtm_of(cws, pw, us, K))
    out = epnp_from(cws, ut[:, 8:], pw, us, K)
    out.update(cws=cws, ut_tail=ut[:, 8:], lam=lam)
    return out


def error2(pose, p3d, p2d, K):
    """CheckInliers' error2 (:302-331) of every pose [H, 3, 4] on every point -> [H, N]"""
    H = len(pose)
    pw = np.broadcast_to(p3d.astype(np.float64), (H,) + p3d.shape)
    ue, ve = project(pose, pw, K)
    with np.errstate(invalid="ignore"):
        return (p2d[None, :, 0].astype(np.float64) - ue) ** 2 + (p2d[None, :, 1].astype(np.float64) - ve) ** 2


def records_of(counts, min_inliers):
    """the iterations whose count is at least min_inliers and strictly above every earlier count"""
    best, out = 0, []
    for it, c in enumerate(counts):
        if c >= min_inliers and c > best:
            best = int(c)
            out.append(it)
    return out


def pose_distance(pose, R, t):
    return float(np.abs(pose[:, :3] - R).max()), float(np.abs(pose[:, 3] - t).max())


def perturbed(x, rng):
    return x * (1.0 + PERTURB * rng.choice([-1.0, 1.0], size=x.shape))


def sensitivity(cws, ut_tail, pw, us, K, base=None, seed=5):
    """the change of epnp_from's (R, t), max over the 12 entries, under the elementwise perturbation -> [H]"""
    rng = np.random.default_rng(seed)
    base = base if base is not None else epnp_from(cws, ut_tail, pw, us, K)
    moved = epnp_from(perturbed(cws, rng), perturbed(ut_tail, rng), pw, us, K)
    with np.errstate(invalid="ignore"):
        d = np.abs(moved["pose"] - base["pose"]).reshape(len(cws), 12).max(1)
    return np.where(np.isfinite(d), d, np.inf)


# ---------------------------------------------------------------- the checks both builds are held to
def gather(sc, sets):
    return sc["p3d"][sets].astype(np.float64), sc["p2d"][sets].astype(np.float64)


def check_control_points(pw, cws, pca, label):
    """bar 1: c0, the unit axes `pca` [H, 3, 3] as returned (before they are folded into c0 + k axis) and the lengths
    -> the worst figure / bar of each"""
    H, n, _ = pw.shape
    ref, lam = control_points(pw)
    axes = pca_axes(pw)
    worst = [0.0, 0.0, 0.0]
    for h in range(H):
        if not np.isfinite(cws[h]).all():
            assert not np.isfinite(pw[h]).all(), label
            continue
        bar0 = 4 * n * EPS * np.abs(pw[h]).max()
        worst[0] = max(worst[0], np.abs(cws[h, 0] - ref[h, 0]).max() / bar0)
        s1 = lam[h, 0]
        assert np.abs(pca[h] @ pca[h].T - np.eye(3)).max() <= 64 * EPS, label
        for i in range(3):
            got = cws[h, i + 1] - cws[h, 0]
            length2 = (got ** 2).sum() * n                       # the eigenvalue dc[i] the length was made from
            worst[2] = max(worst[2], abs(length2 - lam[h, i]) / (16 * EPS * s1))
            # the control point is c0 + k axis of the returned axis, up to the rounding of that sum and this difference
            k = np.linalg.norm(got)
            assert np.abs(got - k * pca[h, i]).max() <= 4 * EPS * np.abs(cws[h]).max(), label
            gaps = [abs(lam[h, i] - lam[h, j]) for j in range(3) if j != i]
            if min(gaps) <= 1e3 * EPS * s1:
                continue                                          # no direction to compare: a (near) repeated eigenvalue
            want = axes[h, i]
            err = min(np.abs(pca[h, i] - want).max(), np.abs(pca[h, i] + want).max())
            worst[1] = max(worst[1], err / (16 * EPS * s1 / min(gaps)))
    print("%s: control points, worst / bar: c0 %.3f, axes %.3f, lengths %.3f" % ((label,) + tuple(worst)))
    assert max(worst) <= 1.0, (label, worst)
    return worst


def check_basis(cws, ut_tail, pw, us, K, refine, label):
    """bar 2, M'M formed from the given control points -> worst figure / bar"""
    H = len(cws)
    lam, ut = basis_eigh(mtm_of(cws, pw, us, K))
    worst = [0.0, 0.0]
    for h in range(H):
        if not np.isfinite(ut_tail[h]).all():
            assert not np.isfinite(lam[h]).all() or not np.isfinite(cws[h]).all(), label
            continue
        t = ut_tail[h]
        worst[0] = max(worst[0], np.abs(t @ t.T - np.eye(4)).max() / (64 * EPS))
        if refine:
            gap = lam[h, 10] - lam[h, 11]
            err = min(np.abs(t[3] - ut[h, 11]).max(), np.abs(t[3] + ut[h, 11]).max())
        else:
            gap = lam[h, 7] - lam[h, 8]
            err = np.abs(t.T @ t - ut[h, 8:].T @ ut[h, 8:]).max()
        if gap <= 1e3 * EPS * lam[h, 0]:
            continue
        worst[1] = max(worst[1], err / (16 * EPS * lam[h, 0] / gap))
    print("%s: basis, worst / bar: orthonormal %.3f, %s %.3f" % (label, worst[0], "row 11" if refine else "projector", worst[1]))
    assert max(worst) <= 1.0, (label, worst)
    return worst


def check_downstream(got, pw, us, K, label):
    """bar 3: got = dict(pose [H, 12], cws, ut_tail, rep_errors) against epnp_from on the given basis -> worst |dpose|"""
    H = len(got["cws"])
    cws, tail = got["cws"].reshape(H, 4, 3), got["ut_tail"].reshape(H, 4, 12)
    finite = np.isfinite(cws).all((1, 2)) & np.isfinite(tail).all((1, 2))
    ref = epnp_from(cws, tail, pw, us, K)
    move = sensitivity(cws, tail, pw, us, K, ref)
    with np.errstate(invalid="ignore"):
        d = np.abs(got["pose_f64"].reshape(H, 3, 4) - ref["pose"]).reshape(H, 12).max(1)
    both_nan = ~np.isfinite(got["pose_f64"]).all(1) & ~np.isfinite(ref["pose"]).reshape(H, 12).all(1)
    rep = ref["rep"]
    with np.errstate(invalid="ignore"):
        srt = np.sort(rep, 1)
        tie = (np.abs(srt[:, 1] - srt[:, 0]) <= 1e-9 * np.abs(srt[:, 0]))
    # Two candidates whose rep_errors agree to 1e-9 may be chosen either way: there the pose is held to the nearer of the
    # tied candidates' poses; everywhere else to the chosen one's, and the choice itself is compared.
    with np.errstate(invalid="ignore"):
        tied = np.abs(rep - srt[:, :1]) <= 1e-9 * np.abs(srt[:, :1])
        each = np.abs(got["pose_f64"].reshape(H, 1, 3, 4) - ref["poses"]).reshape(H, 3, 12).max(2)
        d = np.where(tie, np.where(tied, each, np.inf).min(1), d)
    judged = finite & ~both_nan & (move <= ILL_CONDITIONED)
    left_out = int((finite & ~both_nan & (move > ILL_CONDITIONED)).sum())
    worst = float(d[judged].max()) if judged.any() else 0.0
    got_choice = np.full(H, -1)
    r = got["rep_errors"]
    with np.errstate(invalid="ignore"):
        got_choice = np.where(r[:, 1] < r[:, 0], 1, 0)
        got_choice = np.where(r[:, 2] < np.take_along_axis(r, got_choice[:, None], 1)[:, 0], 2, got_choice)
    print("%s: downstream of the basis: worst |pose - reference| %.3e (bar %.3e) over %d hypotheses, %d ill-conditioned "
          "left out, %d ties, median %.3e" % (label, worst, POSE_BAR, int(judged.sum()), left_out, int(tie.sum()),
                                              float(np.median(d[judged])) if judged.any() else 0.0))
    assert left_out <= MAX_LEFT_OUT * H + 1e-9, (label, left_out, H)
    assert (got_choice[judged & ~tie] == ref["chosen"][judged & ~tie]).all(), label
    assert worst <= POSE_BAR, (label, worst, POSE_BAR)
    return worst


def check_counts(pose_f64, counts, sc, th2, label, flags=None):
    """bar 4: counts (and flags [H, N], where given) recomputed in f64 from the given poses"""
    e2 = error2(pose_f64.reshape(-1, 3, 4), sc["p3d"], sc["p2d"], sc["K"])
    th = float(np.float32(th2))
    with np.errstate(invalid="ignore"):
        inside = e2 < th
        band = np.abs(e2 - th) <= BAND * th
    assert band.sum() <= MAX_IN_BAND * band.size, (label, int(band.sum()))
    lo, hi = (inside & ~band).sum(1), (inside | band).sum(1)
    assert ((counts >= lo) & (counts <= hi)).all(), label
    if flags is not None:
        assert (flags[~band] == inside[~band]).all(), label
        assert (flags.sum(1) == counts).all(), label
    return int(band.sum())


def measure_pose_spread():
    """-> (worst change over the judged hypotheses of CASES, how many judged, how many left out, the median)"""
    worst, judged, left, all_moves = 0.0, 0, 0, []
    for kind, seed in CASES:
        sc = scene(kind, seed)
        pw, us = gather(sc, draw_sets(seed, N_SCENE, N_ITERATIONS))
        ref = epnp(pw, us, sc["K"])
        move = sensitivity(ref["cws"], ref["ut_tail"], pw, us, sc["K"], ref)
        ok = move <= ILL_CONDITIONED
        judged, left = judged + int(ok.sum()), left + int((~ok).sum())
        all_moves += list(move[ok])
        worst = max(worst, float(move[ok].max()))
    return worst, judged, left, float(np.median(all_moves))


def check_result(got, sc, sets, min_inliers, max_records, label, th2=TH2):
    """Bars 1..6 on one list's result `got` (the dict of _Matcher.pnp_ransac or of the host build) for the scene `sc` and
    the sets that were used.  -> the first successful record or None"""
    K, p3d, p2d = sc["K"], sc["p3d"], sc["p2d"]
    n, H = len(p3d), len(sets)
    pw, us = gather(sc, sets)
    check_control_points(pw, got["cws"], got["pca"], label)
    check_basis(got["cws"], got["ut_tail"], pw, us, K, False, label)
    check_downstream(got, pw, us, K, label)
    check_counts(got["pose_f64"], got["counts"], sc, th2, label)
    # bar 5: the records, by integer logic from the counts
    want = records_of(got["counts"], min_inliers)
    assert got["n_records"] == len(want), (label, got["n_records"], want)
    assert got["capacity"] == (len(want) > max_records), label
    want = want[:max_records]
    assert list(got["iteration"]) == want, (label, got["iteration"], want)
    first_ok = None
    for r, it in enumerate(want):
        tag = "%s record %d" % (label, r)
        assert got["n_inliers"][r] == got["counts"][it], tag
        assert got["Tcw_best"][r].tobytes() == got["pose_f64"][it].astype(np.float32).tobytes(), tag
        assert got["Tcw_refined"][r].tobytes() == got["rec_pose_f64"][r].astype(np.float32).tobytes(), tag
        assert got["refined_ok"][r] == int(got["n_refined"][r] > min_inliers), tag
        check_counts(got["pose_f64"][it:it + 1], got["n_inliers"][r:r + 1], sc, th2, tag, got["inliers_best"][r:r + 1] != 0)
        check_counts(got["rec_pose_f64"][r:r + 1], got["n_refined"][r:r + 1], sc, th2, tag, got["inliers_refined"][r:r + 1] != 0)
        flags = got["inliers_best"][r] != 0
        pwr, usr = p3d[flags].astype(np.float64)[None], p2d[flags].astype(np.float64)[None]
        rec = dict(cws=got["rec_cws"][r:r + 1], ut_tail=got["rec_ut_tail"][r:r + 1], pose_f64=got["rec_pose_f64"][r:r + 1],
                   rep_errors=got["rec_rep_errors"][r:r + 1])
        if flags.sum() >= 4:
            check_control_points(pwr, rec["cws"], got["rec_pca"][r:r + 1], tag)
            check_basis(rec["cws"], rec["ut_tail"], pwr, usr, K, True, tag)
            check_downstream(rec, pwr, usr, K, tag)
        if first_ok is None and got["refined_ok"][r]:
            first_ok = r
            # bar 6: no further from the truth than the reference's refine of the same inlier set
            # The reference's own refine: eigh's control points and basis.  With noisy points the EPnP solution
            # depends on which way each PCA axis points, and that sign belongs to whoever computed it (csrc/pnp_solve.h):
            # the reference takes the signs the result has, everything else is its own.
            ref_cws, _ = control_points(pwr)
            for i in range(1, 4):
                if np.dot(ref_cws[0, i] - ref_cws[0, 0], got["rec_cws"][r, i] - got["rec_cws"][r, 0]) < 0:
                    ref_cws[0, i] = 2 * ref_cws[0, 0] - ref_cws[0, i]
            _, ref_ut = basis_eigh(mtm_of(ref_cws, pwr, usr, K))
            ref = epnp_from(ref_cws, ref_ut[:, 8:], pwr, usr, K)
            dr, dt = pose_distance(got["rec_pose_f64"][r].reshape(3, 4), sc["R"], sc["t"])
            rr, rt = pose_distance(ref["pose"][0], sc["R"], sc["t"])
            print("%s: refined pose from the truth: R %.3e t %.3e (reference %.3e, %.3e), %d inliers"
                  % (tag, dr, dt, rr, rt, got["n_refined"][r]))
            assert dr <= 1.01 * rr + 1e-9 and dt <= 1.01 * rt + 1e-9, tag
    return first_ok


class IterateReplay:
    """PnPsolver::iterate (:172-257) over the counts and records of a pnp_ransac result (`results`), mnIterations and the
    best state included; Tcw as float32 [16] (zeros for the empty Mat)"""

    def __init__(self, n, n_matches, key_point_indices, min_inliers, max_its):
        self.n, self.n_matches, self.idx = n, n_matches, np.asarray(key_point_indices)
        self.min_inliers, self.max_its = min_inliers, max_its
        self.iterations = self.best_inliers = 0
        self.best = None
        self.results = None

    def _out(self, ok, n=0, flags=None, rt=None, no_more=False):
        tcw = np.zeros(16, np.float32)
        true = []
        if ok:
            tcw[:12], tcw[15] = rt, 1.0
            true = sorted(int(self.idx[i]) for i in np.flatnonzero(flags))
        return dict(ok=int(ok), n=int(n), no_more=int(no_more), its=self.iterations, Tcw=tcw,
                    size=self.n_matches if ok else 0, true=true)

    def iterate(self, n_iterations):
        if self.n < self.min_inliers:
            return self._out(False, no_more=True)
        r, current = self.results, 0
        while self.iterations < self.max_its or current < n_iterations:
            current += 1
            self.iterations += 1
            c = r["counts"][self.iterations - 1]
            if c >= self.min_inliers:
                if c > self.best_inliers:
                    self.best_inliers = int(c)
                    self.best = list(r["iteration"]).index(self.iterations - 1)
                b = self.best
                if r["n_refined"][b] > self.min_inliers:
                    return self._out(True, r["n_refined"][b], r["inliers_refined"][b], r["Tcw_refined"][b])
        if self.iterations >= self.max_its:
            if self.best_inliers >= self.min_inliers:
                b = self.best
                return self._out(True, self.best_inliers, r["inliers_best"][b], r["Tcw_best"][b], no_more=True)
            return self._out(False, no_more=True)
        return self._out(False)
