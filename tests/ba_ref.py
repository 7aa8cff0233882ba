"""Float64 numpy restatement of csrc/ba_solve.h (Optimizer::LocalBundleAdjustment / BundleAdjustment over g2o's
BlockSolver_6_3 and Levenberg): a dense H, an explicit Schur complement, numpy's Cholesky.  SE3Quat, exp, the oplus and
the Huber kernel are those of tests/pose_ref.py.  Where a difference of two costs decides a trial the sums run in the
kernel's order -- a point's cost in edge order, the total as the pairwise tree of ba::tree -- for the reason the pose
reference gives: with another order lambda_out of an unclamped step agrees only to 1e-8.  Everything else (H, b, the
Schur complement, the solve) is plain numpy in whatever order it likes; bars 1 and 2 bound the difference.

Also the scene maker, the bars of tests/test_ba_gpu.py and tests/test_ba_solve_host.py, and the measurements behind them
(profiles/ba_bars.txt)."""
import numpy as np

from tests import pose_ref as pr

EPS = 2.0 ** -52
K = (500.0, 500.0, 320.0, 240.0)
SLOTS, MAX_IT = 64, 32
LOCAL_BA = (2, (5, 10), (1, 0))                       # :475-:527: 5 Huber iterations, 10 without a kernel
INITIAL_BA = (1, (20, 0), (1, 0))                     # Tracking.cc:319: BundleAdjustment(20 iterations), robust
CLEAR = 1e-9                                          # bar 2: |cost - cost_trial| > CLEAR cost for every trial
LAMBDA_RTOL = 1e-9
PERTURB = 16 * EPS
BAND = 1e-6                                           # bar 3: edges this near a threshold are not compared
PERMUTATIONS = 8

# name -> (free, fixed, points, edges or None for 4 per point, seed, schedule).  The seed is the first draw, counted
# from 1, for which scene_conditions() holds (tests/test_ba_ref.py asserts that it does): 1 everywhere but "full",
# whose ten edges per camera leave some poses no nearer the truth in draws 1..9.
SCENES = {
    "initial": (1, 1, 40, None, 1, INITIAL_BA),
    "local": (5, 3, 200, None, 1, LOCAL_BA),
    "wide": (12, 6, 300, None, 1, LOCAL_BA),
    "full": (64, 2, 160, None, 10, LOCAL_BA),
    "e255": (3, 2, 64, 255, 1, LOCAL_BA),
    "e256": (3, 2, 64, 256, 1, LOCAL_BA),
    "e257": (3, 2, 65, 257, 1, LOCAL_BA),
    "p63": (3, 2, 63, None, 1, LOCAL_BA),
    "p64": (3, 2, 64, None, 1, LOCAL_BA),
    "p65": (3, 2, 65, None, 1, LOCAL_BA),
}
# measured on the CPU by measure_bars() (python -m tests.ba_ref), recorded in profiles/ba_bars.txt
MEASURED_STEP_SPREAD = 1.307454712939915e-05   # set by the initial map: one fixed camera leaves the scale to lambda
MEASURED_FINAL_SPREAD = 3.4448989971735955e-06
STEP_BAR = 2 * MEASURED_STEP_SPREAD
# The same measurement scene by scene.  The issue's bar is twice the largest move over all scenes; a scene is held to
# twice its own largest move, which is never wider, so that the initial map's loose figure does not excuse the others.
MEASURED_STEP_SPREADS = {"initial": 1.31e-05, "local": 2.04e-14, "wide": 2.48e-14, "full": 8.83e-12, "e255": 2.13e-14,
                         "e256": 2.13e-14, "e257": 2.13e-14, "p63": 2.04e-14, "p64": 2.13e-14, "p65": 3e-14}
STEP_BARS = {k: min(2 * v, STEP_BAR) for k, v in MEASURED_STEP_SPREADS.items()}
FINAL_BAR = 2 * MEASURED_FINAL_SPREAD
# scenes whose permutations already change a trial count: held to bars 1-3 only
CHAOTIC = ('local', 'wide', 'e255', 'e256', 'e257', 'p63', 'p64', 'p65')


# ---------------------------------------------------------------- scenes
def _look_at(centre):
    """Tcw [3, 4] of a camera at `centre` looking at the origin, y down"""
    z = -centre / np.linalg.norm(centre)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ centre)[:, None]], 1)


def _rotation(axis_angle):
    return pr.se3_exp(np.concatenate([axis_angle, np.zeros(3)]))[0]


def make_scene(n_free, n_fixed, n_points, n_edges=None, seed=1, outliers=0.05):
    """Cameras on an arc looking at a point cloud; integer-truncated pixels; a share of gross outliers; entry poses of
    the free cameras rotated by <= 0.02 rad and shifted by <= 0.05, points moved by <= 2 %; fixed cameras at the truth.
    Edges sorted by point, about 4 per point (or exactly n_edges in all)."""
    rng = np.random.default_rng([seed, n_free, n_fixed, n_points, n_edges or 0])
    nc = n_free + n_fixed
    ang = np.linspace(-0.7, 0.7, nc) if nc > 1 else np.zeros(1)
    centres = np.stack([6 * np.sin(ang), 0.4 * np.cos(3 * ang), -6 * np.cos(ang)], 1)
    truth_T = np.stack([_look_at(c) for c in centres])
    truth_p = rng.uniform(-1.5, 1.5, (n_points, 3))
    per = min(4, nc)
    counts = np.full(n_points, per)
    if n_edges is not None:
        extra = n_edges - per * n_points
        assert abs(extra) <= n_points and per + 1 <= nc and per > 1
        counts[:abs(extra)] += 1 if extra > 0 else -1
    ec, ep = [], []
    for q in range(n_points):
        cams = np.sort(rng.choice(nc, counts[q], replace=False))
        ec += list(cams)
        ep += [q] * len(cams)
    ec, ep = np.array(ec, np.int32), np.array(ep, np.int32)
    fixed = np.zeros(nc, np.uint8)
    fixed[rng.choice(nc, n_fixed, replace=False)] = 1
    xc = np.einsum("eij,ej->ei", truth_T[ec][:, :, :3], truth_p[ep]) + truth_T[ec][:, :, 3]
    pix = np.floor(np.stack([K[0] * xc[:, 0] / xc[:, 2] + K[2], K[1] * xc[:, 1] / xc[:, 2] + K[3]], 1))
    gross = rng.random(len(ec)) < outliers
    pix[gross] = np.floor(rng.uniform([0, 0], [640, 480], (int(gross.sum()), 2)))
    T0 = truth_T.copy()
    for c in range(nc):
        if fixed[c]:
            continue
        axis = rng.normal(size=3)
        dR = _rotation(axis / np.linalg.norm(axis) * rng.uniform(0.015, 0.02))
        shift = rng.normal(size=3)
        T0[c, :, :3] = dR @ truth_T[c, :, :3]
        T0[c, :, 3] = dR @ truth_T[c, :, 3] + shift / np.linalg.norm(shift) * rng.uniform(0.04, 0.05)
    p0 = truth_p * (1 + rng.uniform(-0.02, 0.02, truth_p.shape))
    return dict(cam_Tcw=T0.reshape(nc, 12).astype(np.float32), cam_fixed=fixed, points=p0.astype(np.float32),
                edge_cam=ec, edge_point=ep, edge_obs=pix.astype(np.float32), K=K, gross=gross,
                truth_Tcw=truth_T.reshape(nc, 12), truth_points=truth_p)


_SCENES = {}


def scene(name):
    if name not in _SCENES:
        f, x, p, e, seed, _ = SCENES[name]
        _SCENES[name] = make_scene(f, x, p, e, seed)
    return _SCENES[name]


def schedule_of(name):
    return SCENES[name][5]


# ---------------------------------------------------------------- sums in the kernel's order
def tree(a, largest=False):
    """ba::tree: pairwise, the shape a function of len(a) alone"""
    a = np.array(a, np.float64)
    n, s = len(a), 1
    while s < n:
        if largest:
            a[0:n - s:2 * s] = np.maximum(a[0:n - s:2 * s], a[s:n:2 * s])
        else:
            a[0:n - s:2 * s] = a[0:n - s:2 * s] + a[s:n:2 * s]
        s *= 2
    return a[0] if n else 0.0


def by_owner(values, owner, n):
    """sum of values per owner, each owner adding in index order (np.add.at is unbuffered and sequential)"""
    out = np.zeros((n,) + values.shape[1:])
    np.add.at(out, owner, values)
    return out


# ---------------------------------------------------------------- the edges
def matrices(cams):
    """[n_cams, 7] estimates -> [n_cams, 12]"""
    return np.stack([pr.matrix_of((c[:4], c[4:])) for c in cams]) if len(cams) else np.zeros((0, 12))


def estimates_of(tcw):
    return np.stack([np.concatenate(pr.estimate_of(t)) for t in tcw]) if len(tcw) else np.zeros((0, 7))


def edge_errors(rt, p, obs):
    """rt [E, 12], p [E, 3], obs [E, 2] -> camera points, e; term by term and left to right like pose::edge_error"""
    xc = np.stack([rt[:, 4 * r] * p[:, 0] + rt[:, 4 * r + 1] * p[:, 1] + rt[:, 4 * r + 2] * p[:, 2] + rt[:, 4 * r + 3]
                   for r in range(3)], 1)
    with np.errstate(all="ignore"):
        proj = np.stack([xc[:, 0] / xc[:, 2] * K[0] + K[2], xc[:, 1] / xc[:, 2] * K[1] + K[3]], 1)
    return xc, obs - proj


def robustify(e2, huber, delta2):
    s = 5.991 / delta2
    rho, w = pr.robustify(e2 * s, huber)
    return rho / s, w


class State:
    """a problem with its estimates: cams [n_cams, 7], pts [n_points, 3]"""

    def __init__(self, sc, cams=None, pts=None, huber_delta2=5.991, chi2=5.991):
        self.sc = sc
        self.ec, self.ep = np.asarray(sc["edge_cam"], np.int64), np.asarray(sc["edge_point"], np.int64)
        self.obs = np.asarray(sc["edge_obs"], np.float32).astype(np.float64).reshape(-1, 2)
        self.nc, self.np, self.ne = len(sc["cam_Tcw"]), len(sc["points"]), len(self.ec)
        self.fixed = np.asarray(sc["cam_fixed"]).astype(bool)
        self.free_of = np.where(self.fixed, -1, np.cumsum(~self.fixed) - 1)
        self.nf = int((~self.fixed).sum())
        self.cams = estimates_of(np.asarray(sc["cam_Tcw"], np.float32).reshape(-1, 12)) if cams is None else np.array(cams)
        self.pts = np.asarray(sc["points"], np.float32).astype(np.float64).reshape(-1, 3) if pts is None else np.array(pts)
        self.delta2, self.chi2 = huber_delta2, chi2

    def errors(self, cams=None, pts=None):
        cams = self.cams if cams is None else cams
        pts = self.pts if pts is None else pts
        return edge_errors(matrices(cams)[self.ec], pts[self.ep], self.obs)

    def flags(self, cams=None, pts=None):
        """-> chi2 > threshold or depth not positive, chi2, Z"""
        xc, e = self.errors(cams, pts)
        chi2 = (e * e).sum(1)
        with np.errstate(all="ignore"):
            return (chi2 > self.chi2) | ~(xc[:, 2] > 0), chi2, xc

    def cost(self, cams, pts, active, huber):
        xc, e = self.errors(cams, pts)
        rho = robustify((e * e).sum(1), huber, self.delta2)[0]
        return tree(by_owner(rho[active], self.ep[active], self.np))

    def terms(self, active, huber):
        """per active edge: Jc [a, 2, 6], Jp [a, 2, 3], e, rho', rho, and the edges' indices"""
        idx = np.flatnonzero(active)
        rt = matrices(self.cams)[self.ec[idx]]
        xc, e = edge_errors(rt, self.pts[self.ep[idx]], self.obs[idx])
        x, y = xc[:, 0], xc[:, 1]
        with np.errstate(all="ignore"):
            invz = 1.0 / xc[:, 2]
            invz2 = invz * invz
            fu, fv = K[0], K[1]
            zero = np.zeros_like(x)
            j0 = np.stack([x * y * invz2 * fu, -(1 + x * x * invz2) * fu, y * invz * fu, -invz * fu, zero, x * invz2 * fu], 1)
            j1 = np.stack([(1 + y * y * invz2) * fv, -x * y * invz2 * fv, -x * invz * fv, zero, -invz * fv, y * invz2 * fv], 1)
            t02, t12 = -x * invz * fu, -y * invz * fv
            p0 = np.stack([-invz * (fu * rt[:, k] + t02 * rt[:, 8 + k]) for k in range(3)], 1)
            p1 = np.stack([-invz * (fv * rt[:, 4 + k] + t12 * rt[:, 8 + k]) for k in range(3)], 1)
            rho, w = robustify((e * e).sum(1), huber, self.delta2)
        return idx, np.stack([j0, j1], 1), np.stack([p0, p1], 1), e, w, rho

    def system(self, active, huber):
        """-> dict: Hcc [nc, 6, 6], bc [nc, 6] (zero for fixed), Hpp [np, 3, 3], bp [np, 3], W [(edge, 6 x 3)], cost, and
        the abs-term sums and counts bar 1 needs"""
        idx, Jc, Jp, e, w, rho = self.terms(active, huber)
        ec, ep = self.ec[idx], self.ep[idx]
        free = ~self.fixed[ec]
        tc = w[:, None, None] * np.einsum("eki,ekj->eij", Jc, Jc)
        tb = -(w[:, None] * np.einsum("eki,ek->ei", Jc, e))
        tp = w[:, None, None] * np.einsum("eki,ekj->eij", Jp, Jp)
        tq = -(w[:, None] * np.einsum("eki,ek->ei", Jp, e))
        W = w[:, None, None] * np.einsum("eki,ekj->eij", Jc, Jp)
        s = dict(idx=idx, free=free, W=W,
                 Hcc=by_owner(tc[free], ec[free], self.nc), bc=by_owner(tb[free], ec[free], self.nc),
                 Hpp=by_owner(tp, ep, self.np), bp=by_owner(tq, ep, self.np),
                 aHcc=by_owner(np.abs(tc[free]), ec[free], self.nc), abc=by_owner(np.abs(tb[free]), ec[free], self.nc),
                 aHpp=by_owner(np.abs(tp), ep, self.np), abp=by_owner(np.abs(tq), ep, self.np),
                 kc=np.bincount(ec[free], minlength=self.nc), kp=np.bincount(ep, minlength=self.np),
                 kc_all=np.bincount(ec, minlength=self.nc),
                 cost=tree(by_owner(rho, ep, self.np)), acost=np.abs(rho).sum(), k=len(idx))
        return s


def point_inverses(Hpp, lam, moves):
    """(Hpp + lambda I)^-1 per point, zero where the point does not move; ok False: a leading minor not positive"""
    A = Hpp + lam * np.eye(3)
    inv = np.zeros_like(A)
    ok = True
    with np.errstate(all="ignore"):
        m1, m2, det = A[:, 0, 0], A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] ** 2, np.linalg.det(A)
        good = (m1 > 0) & (m2 > 0) & (det > 0) & np.isfinite(det)
    if (~good & moves).any():
        return inv, False
    if moves.any():
        inv[moves] = np.linalg.inv(A[moves])
    return inv, ok


def solve_step(st, s, lam, perturb=None):
    """BlockSolver_6_3 at lambda -> dx_c [nc, 6] (zero rows for fixed), dx_p [np, 3], or None when the trial is rejected.
    perturb: an rng, to move H and b by 16 eps (the bar-2 measurement)."""
    nf, npt = st.nf, st.np
    Hcc, bc, Hpp, bp, W = s["Hcc"], s["bc"], s["Hpp"], s["bp"], s["W"]
    if perturb is not None:
        Hcc, bc, Hpp, bp, W = (x * (1 + PERTURB * perturb.uniform(-1, 1, x.shape)) for x in (Hcc, bc, Hpp, bp, W))
        Hcc, Hpp = (Hcc + np.swapaxes(Hcc, 1, 2)) / 2, (Hpp + np.swapaxes(Hpp, 1, 2)) / 2
    if not np.isfinite(lam):
        return None
    inv, ok = point_inverses(Hpp, lam, s["kp"] > 0)
    if not ok:
        return None
    free_cams = np.flatnonzero(~st.fixed)
    Wd = np.zeros((6 * nf, 3 * npt))
    ec, ep = st.ec[s["idx"]], st.ep[s["idx"]]
    for k in np.flatnonzero(s["free"]):
        f, q = st.free_of[ec[k]], ep[k]
        Wd[6 * f:6 * f + 6, 3 * q:3 * q + 3] += W[k]
    S = np.zeros((6 * nf, 6 * nf))
    bS = np.zeros(6 * nf)
    moves_c = s["kc_all"][free_cams] > 0
    for f, c in enumerate(free_cams):
        S[6 * f:6 * f + 6, 6 * f:6 * f + 6] = Hcc[c] + lam * np.eye(6) if moves_c[f] else np.eye(6)
        bS[6 * f:6 * f + 6] = bc[c] if moves_c[f] else 0.0
    WI = np.zeros_like(Wd)
    for q in range(npt):
        WI[:, 3 * q:3 * q + 3] = Wd[:, 3 * q:3 * q + 3] @ inv[q]
    S = S - WI @ Wd.T
    bS = bS - WI @ bp.reshape(-1)
    if not (np.isfinite(S).all() and np.isfinite(bS).all()):
        return None
    dxc = np.zeros((st.nc, 6))
    if nf:
        try:
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return None
        x = np.linalg.solve(L.T, np.linalg.solve(L, bS))
        dxc[free_cams] = x.reshape(nf, 6)
        dxc[free_cams[~moves_c]] = 0.0
    else:
        x = np.zeros(0)
    dxp = np.einsum("pij,pj->pi", inv, bp - (Wd.T @ x).reshape(npt, 3))
    return dxc, dxp


def iteration(st, lam, first, active, huber, perturb=None):
    """One Levenberg iteration from st's estimates -> dict(trials, accepted, lambda_in, lambda_out, cost_in, cost_out,
    trial_costs, cams, pts, system); st is left at the estimates the iteration keeps."""
    s = st.system(active, huber)
    cost = s["cost"]
    ni = 2.0
    if first:
        free_cams = ~st.fixed
        top_p = tree(np.abs(np.stack([s["Hpp"][:, k, k] for k in range(3)], 1)).max(1), True) if st.np else 0.0
        top_c = tree(np.abs(np.stack([s["Hcc"][free_cams][:, k, k] for k in range(6)], 1)).max(1), True) if st.nf else 0.0
        lam = 1e-5 * max(top_c, top_p)
    lam_in, cost_out, trials, accepted, trial_costs = lam, cost, 0, False, []
    moves_c = (~st.fixed) & (s["kc_all"] > 0)
    moves_p = s["kp"] > 0
    while trials < 10 and not accepted:
        trials += 1
        gain, trial_cost = -1.0, np.inf
        step = solve_step(st, s, lam, perturb)
        if step is not None:
            dxc, dxp = step
            cams = st.cams.copy()
            for c in np.flatnonzero(moves_c):
                cams[c] = np.concatenate(pr.moved((st.cams[c, :4], st.cams[c, 4:]), dxc[c]))
            pts = np.where(moves_p[:, None], st.pts + dxp, st.pts)
            with np.errstate(all="ignore"):
                trial_cost = st.cost(cams, pts, active, huber)
                sp = np.zeros(st.np)
                for k in range(3):
                    sp = sp + dxp[:, k] * (lam * dxp[:, k] + s["bp"][:, k])
                scv = np.zeros(st.nc)
                for k in range(6):
                    scv = scv + dxc[:, k] * (lam * dxc[:, k] + s["bc"][:, k])
                scv = np.where(moves_c, scv, 0.0)[~st.fixed]
                gain = (cost - trial_cost) / ((1e-3 + tree(scv)) + tree(sp))
            trial_costs.append(trial_cost)
        if step is not None and gain > 0 and np.isfinite(trial_cost):
            y = 2 * gain - 1
            lam *= max(1.0 / 3.0, min(2.0 / 3.0, 1.0 - y * y * y))
            st.cams, st.pts, cost_out, accepted = cams, pts, trial_cost, True
        else:
            with np.errstate(all="ignore"):
                lam *= ni
            ni *= 2.0
            if not np.isfinite(lam) or gain == 0:
                break
    return dict(trials=trials, accepted=accepted, lambda_in=lam_in, lambda_out=lam, cost_in=cost, cost_out=cost_out,
                trial_costs=trial_costs, system=s)


def run(sc, schedule, stop=False, huber_delta2=5.991, chi2=5.991):
    """The whole schedule -> the dict _Matcher.bundle_adjust returns (the per-iteration arrays as [64, ...])"""
    n_rounds, its, robust = schedule
    st = State(sc, huber_delta2=huber_delta2, chi2=chi2)
    nc, npt, ne = st.nc, st.np, st.ne
    out = dict(round_iterations=np.zeros(2, np.int32), it_trials=np.zeros(SLOTS, np.int32),
               round_flags=np.zeros((ne, 2), np.uint8), it_cam_in=np.zeros((SLOTS, nc, 7)), it_cam_out=np.zeros((SLOTS, nc, 7)),
               it_point_in=np.zeros((SLOTS, npt, 3)), it_point_out=np.zeros((SLOTS, npt, 3)), clear=np.zeros(SLOTS, bool))
    for k in ("it_lambda_in", "it_lambda_out", "it_cost_in", "it_cost_out"):
        out[k] = np.zeros(SLOTS)
    active = np.ones(ne, bool)
    chi2_0 = np.zeros(ne)
    rounds_run = 0
    for rnd in range(n_rounds):
        if stop:
            break
        if rnd == 1:
            f, chi2_0, _ = st.flags()
            active = ~f
        lam, it = 0.0, 0
        while it < its[rnd]:
            slot = rnd * MAX_IT + it
            out["it_cam_in"][slot], out["it_point_in"][slot] = st.cams, st.pts
            r = iteration(st, lam, it == 0, active, bool(robust[rnd]))
            lam = r["lambda_out"]
            out["it_cam_out"][slot], out["it_point_out"][slot] = st.cams, st.pts
            out["it_trials"][slot] = r["trials"]
            out["clear"][slot] = is_clear(r)
            for k in ("lambda_in", "lambda_out", "cost_in", "cost_out"):
                out["it_" + k][slot] = r[k]
            it += 1
            if not r["accepted"]:
                break
        rounds_run = rnd + 1
        out["round_iterations"][rnd] = it
        if rnd == 0:
            out["round_flags"][:, 0] = st.flags()[0]
    f, _, xc = st.flags()
    if rounds_run == 2:
        with np.errstate(all="ignore"):
            f = np.where(active, f, (chi2_0 > chi2) | ~(xc[:, 2] > 0))
        out["round_flags"][:, 1] = f
    out["outliers"] = f.astype(np.uint8)
    out["status"] = rounds_run
    pose = matrices(st.cams)
    tcw = np.asarray(sc["cam_Tcw"], np.float32).reshape(-1, 12)
    as_came = st.fixed | (rounds_run == 0)
    out["cam_pose_f64"] = np.where(as_came[:, None], tcw.astype(np.float64), pose)
    out["points_f64"] = st.pts
    out["cam_Tcw"], out["points"] = out["cam_pose_f64"].astype(np.float32), st.pts.astype(np.float32)
    return out


def is_clear(r):
    """every trial's cost differs from the entry cost by more than CLEAR of it"""
    return r["trials"] == len(r["trial_costs"]) and all(abs(c - r["cost_in"]) > CLEAR * abs(r["cost_in"]) for c in r["trial_costs"])


_RUNS = {}


def reference(name):
    if name not in _RUNS:
        _RUNS[name] = run(scene(name), schedule_of(name))
    return _RUNS[name]


# ---------------------------------------------------------------- recovery
def pose_distance(a, b):
    """rotation angle + translation distance between two [12] poses"""
    A, B = np.asarray(a, np.float64).reshape(3, 4), np.asarray(b, np.float64).reshape(3, 4)
    c = (np.trace(A[:, :3] @ B[:, :3].T) - 1) / 2
    return float(np.arccos(np.clip(c, -1, 1)) + np.linalg.norm(A[:, 3] - B[:, 3]))


def recovery(sc, res):
    """-> (rms of the unflagged edges before, after, poses that ended nearer the truth, free poses)"""
    keep = res["outliers"] == 0
    st0 = State(sc)
    st1 = State(sc, estimates_of(res["cam_pose_f64"].astype(np.float32)), res["points_f64"])
    e0, e1 = st0.errors()[1][keep], edge_errors(res["cam_pose_f64"][st0.ec], res["points_f64"][st0.ep], st0.obs)[1][keep]
    del st1
    rms = lambda e: float(np.sqrt((e * e).sum(1).mean()))
    free = np.flatnonzero(~st0.fixed)
    nearer = sum(pose_distance(res["cam_pose_f64"][c], sc["truth_Tcw"][c]) < pose_distance(sc["cam_Tcw"][c], sc["truth_Tcw"][c])
                 for c in free)
    return rms(e0), rms(e1), int(nearer), len(free)


def scene_conditions(sc, schedule, res):
    """What a scene must give the reference before it is used: -> list of what fails (empty: usable).  The reprojection
    RMS of the unflagged edges falls, every free pose ends nearer the truth, iteration 0 of every round and at least a
    third of all iterations are clear (bar 2 is a cap, not a measurement), and at most 1 % of the edges lie within BAND
    of a threshold (bar 3)."""
    fails = []
    before, after, nearer, free = recovery(sc, res)
    if not after < before:
        fails.append("rms %.3g -> %.3g" % (before, after))
    if nearer != free:
        fails.append("%d of %d free poses nearer the truth" % (nearer, free))
    ran = res["it_trials"] > 0
    for rnd in range(schedule[0]):
        if schedule[1][rnd] and not res["clear"][rnd * MAX_IT]:
            fails.append("iteration 0 of round %d is not clear" % rnd)
    if 3 * int(res["clear"][ran].sum()) < int(ran.sum()):
        fails.append("%d clear iterations of %d" % (int(res["clear"][ran].sum()), int(ran.sum())))
    near_threshold = 0
    for rnd in range(schedule[0]):
        _, chi2, xc = State(sc, *kept_estimates(res, sc, rnd)).flags()
        with np.errstate(all="ignore"):
            near_threshold += int(((np.abs(chi2 / 5.991 - 1) <= BAND) | (np.abs(xc[:, 2]) <= BAND * np.abs(xc).max(1))).sum())
    if near_threshold > 0.01 * len(chi2):
        fails.append("%d edges within the band of a threshold" % near_threshold)
    return fails


def first_usable_seed(name, limit=40):
    f, x, p, e, _, schedule = SCENES[name]
    for seed in range(1, limit):
        sc = make_scene(f, x, p, e, seed)
        if not scene_conditions(sc, schedule, run(sc, schedule)):
            return seed
    return None


# ---------------------------------------------------------------- the bars
def kept_estimates(got, sc, upto_round):
    """the device's own estimates at the end of round `upto_round`: it_cam_out / it_point_out of the last iteration run"""
    cams = estimates_of(np.asarray(sc["cam_Tcw"], np.float32).reshape(-1, 12))
    pts = np.asarray(sc["points"], np.float32).astype(np.float64).reshape(-1, 3)
    for rnd in range(upto_round + 1):
        n = int(got["round_iterations"][rnd])
        if n:
            cams, pts = got["it_cam_out"][rnd * MAX_IT + n - 1], got["it_point_out"][rnd * MAX_IT + n - 1]
    return cams, pts


def near(a, b, tol, what):
    with np.errstate(all="ignore"):
        bad = ~(np.abs(np.asarray(a) - np.asarray(b)) <= tol)
    assert not bad.any(), "%s: %d beyond the bar, worst %.3g of it" % (
        what, int(bad.sum()), float(np.nanmax(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(tol, 1e-300))))


def triu6(H):
    return H[..., np.triu_indices(6)[0], np.triu_indices(6)[1]]


def triu3(H):
    return H[..., np.triu_indices(3)[0], np.triu_indices(3)[1]]


def check_result(got, name, label, sc=None, schedule=None, final=True):
    """Bars 1-4 of tests/test_ba_gpu.py on the result dict of one problem.  -> (clear iterations, iterations run,
    worst step difference / STEP_BAR, worst final difference / FINAL_BAR)"""
    sc = scene(name) if sc is None else sc
    n_rounds, its, robust = schedule_of(name) if schedule is None else schedule
    st = State(sc)
    ne = st.ne
    assert got["status"] == n_rounds, label
    clear = run_its = 0
    worst_step, step_bar = 0.0, STEP_BARS.get(name, STEP_BAR)
    active = np.ones(ne, bool)
    for rnd in range(n_rounds):
        if rnd == 1:
            active = got["round_flags"][:, 0] == 0
        n_it = int(got["round_iterations"][rnd])
        assert 1 <= n_it <= its[rnd] or its[rnd] == 0, label
        for it in range(MAX_IT):
            slot = rnd * MAX_IT + it
            if it >= n_it:
                assert got["it_trials"][slot] == 0, (label, slot)
                continue
            run_its += 1
            what = "%s round %d iteration %d" % (label, rnd, it)
            huber = bool(robust[rnd])
            # bar 1: the sums from the device's own entry estimates
            s0 = State(sc, got["it_cam_in"][slot], got["it_point_in"][slot])
            s = s0.system(active, huber)
            near(got["it_Hcc"][slot], triu6(s["Hcc"]), (s["kc"][:, None] + 64) * EPS * triu6(s["aHcc"]), what + " Hcc")
            near(got["it_bc"][slot], s["bc"], (s["kc"][:, None] + 64) * EPS * s["abc"], what + " bc")
            near(got["it_Hpp"][slot], triu3(s["Hpp"]), (s["kp"][:, None] + 64) * EPS * triu3(s["aHpp"]), what + " Hpp")
            near(got["it_bp"][slot], s["bp"], (s["kp"][:, None] + 64) * EPS * s["abp"], what + " bp")
            near(got["it_cost_in"][slot], s["cost"], (s["k"] + 64) * EPS * s["acost"], what + " cost")
            # bar 2: the iteration replayed from the device's entry estimate and lambda
            lam_in = got["it_lambda_in"][slot]
            r = iteration(s0, lam_in, it == 0, active, huber)
            if it == 0:
                assert abs(r["lambda_in"] - lam_in) <= 1e-12 * lam_in, what
            if is_clear(r):
                clear += 1
                assert got["it_trials"][slot] == r["trials"], (what, got["it_trials"][slot], r["trials"])
                assert abs(got["it_lambda_out"][slot] - r["lambda_out"]) <= LAMBDA_RTOL * r["lambda_out"], what
                d = max(np.abs(got["it_cam_out"][slot] - s0.cams).max(initial=0), np.abs(got["it_point_out"][slot] - s0.pts).max(initial=0))
                worst_step = max(worst_step, d / step_bar)
                assert d <= step_bar, (what, d, step_bar)
            else:
                assert it > 0, what + ": iteration 0 of a round must be clear"
                assert got["it_cost_out"][slot] <= got["it_cost_in"][slot], what
        assert 3 * clear >= run_its or rnd + 1 < n_rounds, (label, clear, run_its)
    # bar 3: the flags from the device's own round and final estimates
    excluded = np.zeros(ne, bool)

    def sure(st_flags):
        f, chi2, xc = st_flags
        with np.errstate(all="ignore"):
            unsure = (np.abs(chi2 / 5.991 - 1) <= BAND) | (np.abs(xc[:, 2]) <= BAND * np.abs(xc).max(1))
        return f, chi2, xc, unsure
    f0, chi2_0, _, u0 = sure(State(sc, *kept_estimates(got, sc, 0)).flags())
    excluded |= u0
    f_last = f0
    if n_rounds == 2:
        assert (got["round_flags"][:, 0][~u0] == f0[~u0]).all(), label
        f1, _, xc1, u1 = sure(State(sc, *kept_estimates(got, sc, 1)).flags())
        with np.errstate(all="ignore"):
            f_last = np.where(got["round_flags"][:, 0] == 0, f1, (chi2_0 > 5.991) | ~(xc1[:, 2] > 0))
        excluded |= u1
        assert (got["round_flags"][:, 1] == got["outliers"]).all(), label
    else:
        assert (got["round_flags"][:, 0] == got["outliers"]).all(), label
    assert (got["outliers"][~excluded] == f_last[~excluded]).all(), label
    assert excluded.sum() <= 0.01 * max(ne, 1) + (ne < 100), (label, int(excluded.sum()))
    # bar 4: the f32 results are the roundings of the f64 ones; the final estimates against the reference's run
    assert got["cam_Tcw"].tobytes() == got["cam_pose_f64"].astype(np.float32).tobytes(), label
    assert got["points"].tobytes() == got["points_f64"].astype(np.float32).tobytes(), label
    fixed = st.fixed
    assert got["cam_Tcw"][fixed].tobytes() == np.asarray(sc["cam_Tcw"], np.float32).reshape(-1, 12)[fixed].tobytes(), label
    worst_final = 0.0
    if final and name is not None and name not in CHAOTIC:
        ref = reference(name)
        worst_final = max(np.abs(got["cam_pose_f64"] - ref["cam_pose_f64"]).max(initial=0),
                          np.abs(got["points_f64"] - ref["points_f64"]).max(initial=0))
        assert worst_final <= FINAL_BAR, (label, worst_final)
        worst_final /= FINAL_BAR
    return clear, run_its, worst_step, worst_final


# ---------------------------------------------------------------- the measurements behind the bars
def permuted(sc, rng):
    """the same problem with the points renumbered and the edges of every point reordered"""
    npt = len(sc["points"])
    new_of = rng.permutation(npt)                     # old point -> new index
    ep = new_of[sc["edge_point"]]
    order = np.lexsort((rng.random(len(ep)), ep))
    out = dict(sc)
    out["points"] = np.zeros_like(sc["points"])
    out["points"][new_of] = sc["points"]
    out["edge_point"], out["edge_cam"] = ep[order].astype(np.int32), sc["edge_cam"][order]
    out["edge_obs"] = sc["edge_obs"][order]
    return out, new_of


def measure_bars(names=None, log=print):
    """-> (step spread, final spread, chaotic scenes): how far the reference's own iteration moves when H, b and the
    entry estimates are perturbed by 16 eps, over the clear iterations; how far its final result moves under 8
    permutations of the point order and of the edge order within each point"""
    step = final = 0.0
    chaotic = []
    for name in names or SCENES:
        sc, schedule = scene(name), schedule_of(name)
        ref = reference(name)
        rng = np.random.default_rng(7)
        own = 0.0
        active = np.ones(len(sc["edge_cam"]), bool)
        for rnd in range(schedule[0]):
            if rnd == 1:
                active = ref["round_flags"][:, 0] == 0
            for it in range(int(ref["round_iterations"][rnd])):
                slot = rnd * MAX_IT + it
                if not ref["clear"][slot]:
                    continue
                jig = lambda x: x * (1 + PERTURB * rng.uniform(-1, 1, x.shape))
                st = State(sc, jig(ref["it_cam_in"][slot]), jig(ref["it_point_in"][slot]))
                st.cams[:, :4] /= np.linalg.norm(st.cams[:, :4], axis=1, keepdims=True)
                r = iteration(st, ref["it_lambda_in"][slot], it == 0, active, bool(schedule[2][rnd]), perturb=rng)
                if r["trials"] != ref["it_trials"][slot]:
                    continue
                d = max(np.abs(st.cams - ref["it_cam_out"][slot]).max(initial=0), np.abs(st.pts - ref["it_point_out"][slot]).max(initial=0))
                step, own = max(step, d), max(own, d)
        worst, changed = 0.0, False
        for k in range(PERMUTATIONS):
            sc2, new_of = permuted(sc, np.random.default_rng(100 + k))
            r2 = run(sc2, schedule)
            changed |= not (r2["it_trials"] == ref["it_trials"]).all()
            worst = max(worst, np.abs(r2["cam_pose_f64"] - ref["cam_pose_f64"]).max(initial=0),
                        np.abs(r2["points_f64"][new_of] - ref["points_f64"]).max(initial=0))
        log("%-8s step spread %.3g, final spread %.3g%s" % (name, own, worst, "  (trial counts change)" if changed else ""))
        if changed:
            chaotic.append(name)
        else:
            final = max(final, worst)
    return step, final, chaotic


if __name__ == "__main__":
    s, f, c = measure_bars()
    print("MEASURED_STEP_SPREAD = %r\nMEASURED_FINAL_SPREAD = %r\nCHAOTIC = %r" % (s, f, tuple(c)))
