"""TEST INFRASTRUCTURE ONLY -- reference side of the new-map-point tests (test_new_points_ref.py, test_new_points_host.py,
test_new_points_gpu.py, test_create_map_points_gpu.py), written from slam_pipeline/src/LocalMapping.cc:195-265 as a
specification: the loop body of CreateNewMapPoints, stage by stage, in numpy.

  new_points(matches, v1, v2, max_cos, chi2, dtype)   the stages; parameterised by the dtype of the SVD ONLY: the key
                           points, normalised coordinates, rays and the 4 x 4 matrix are always built in f32 in the
                           reference's order, the cosine in f64 from the f32 rays; the float64 reference is "float64 SVD
                           of the same f32 matrix" (the convention of initializer_ref.triangulation_matrices), and the
                           depth and reprojection checks are in f64 on the resulting point
  stages_from_points(...)  stages 3-7 alone, in f64, from a given null vector / point (self-consistency of a device result)
  scene(seed) / handmade() the inputs
  check_result(...)        every bar on one result (host build or device)

Borderline: a match alive at a stage and within that stage's band (those of initializer_ref.check_rt):
|cos| <= 1e-6; |cos - max_cos| <= 1e-6; |z| <= 1e-3 |p|; |e - chi2| <= 0.01 chi2.  A match that reaches the
triangulation is also borderline when its null-vector bound 16 EPS s1 / (s3 - s4) exceeds ransac_ref.UNINFORMATIVE, or
when |hom[3]| of the unit float64 null vector is within that bound of zero: the bar on the null vector then leaves the
sign of the fourth entry -- and with it `hom[3] == 0` and the side of both cameras the point lies on -- undecided.

Nothing here is code under test and nothing here is imported by the product package."""
import functools

import numpy as np

from tests import initializer_ref as ir
from tests import ransac_ref as rr

EPS = rr.EPS
CHI2 = 5.991
MAX_COS = (1.1, 0.9998)
SEEDS = (1, 2, 3)
CASES = [(s, c) for s in SEEDS for c in MAX_COS]
N_NEIGHBOURS, N_MATCHES = 8, 320
BASELINES = (0.15, 0.3, 0.6, 0.05, 0.4, 0.25, 0.1, 0.5)
AXIAL = 2                        # the neighbour whose baseline lies along the optical axis
VIEW_DTYPE = np.dtype([("Rcw", "<f4", (9,)), ("tcw", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4")])


def rodrigues(v):
    v = np.asarray(v, np.float64)
    a = np.linalg.norm(v)
    if a == 0:
        return np.eye(3)
    k = v / a
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def make_view(R, t, K=ir.K):
    """one VIEW_DTYPE record (the bytes of msf_view) from Rcw [3, 3], tcw [3] and a 3 x 3 K"""
    v = np.zeros((), VIEW_DTYPE)
    v["Rcw"] = np.asarray(R, np.float32).reshape(9)
    v["tcw"] = np.asarray(t, np.float32).reshape(3)
    v["fx"], v["fy"], v["cx"], v["cy"] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    return v


# ---- the inputs ----
@functools.lru_cache(maxsize=None)
def scene(seed):
    """-> (view1: VIEW_DTYPE record, views2: VIEW_DTYPE [8], matches int32 [8, 320, 4]); computed once: do not modify.
    The current view is a small random pose; neighbour i sits BASELINES[i] away in a random direction (AXIAL: along the
    optical axis) with a relative rotation of up to 0.12 rad.  Points: a uniformly random pixel of view 1 at depth 3-12
    (12 %: 150-3000), projected into view 2 with 0.7 px Gaussian noise; 15 % outliers with a uniformly random end point
    2; integer pixels."""
    r = np.random.RandomState(1000 + seed)
    K64 = ir.K.astype(np.float64)
    R1 = rodrigues(r.uniform(-0.05, 0.05, 3))
    t1 = r.uniform(-0.2, 0.2, 3)
    view1 = make_view(R1, t1)
    views2 = np.zeros(N_NEIGHBOURS, VIEW_DTYPE)
    matches = np.zeros((N_NEIGHBOURS, N_MATCHES, 4), np.int32)
    for i, base in enumerate(BASELINES):
        d = r.randn(3)
        if i == AXIAL:
            d = np.array([0.0, 0.0, 1.0])
        c2_in_c1 = base * d / np.linalg.norm(d)              # camera 2's centre in camera 1's frame
        axis = r.randn(3)
        R21 = rodrigues(axis / np.linalg.norm(axis) * r.uniform(0.0, 0.12))
        t21 = -R21 @ c2_in_c1
        R2, t2 = R21 @ R1, R21 @ t1 + t21
        views2[i] = make_view(R2, t2)
        n = N_MATCHES
        px = np.c_[r.uniform(0, rr.W, n), r.uniform(0, rr.H, n)]
        depth = r.uniform(3, 12, n)
        far = r.rand(n) < 0.12
        depth[far] = r.uniform(150, 3000, int(far.sum()))
        Xc1 = np.c_[(px[:, 0] - K64[0, 2]) / K64[0, 0], (px[:, 1] - K64[1, 2]) / K64[1, 1], np.ones(n)] * depth[:, None]
        Xc2 = Xc1 @ R21.T + t21
        p2 = np.c_[K64[0, 0] * Xc2[:, 0] / Xc2[:, 2] + K64[0, 2], K64[1, 1] * Xc2[:, 1] / Xc2[:, 2] + K64[1, 2]]
        p2 += r.randn(n, 2) * 0.7
        out = r.rand(n) < 0.15
        p2[out] = np.c_[r.uniform(0, rr.W, int(out.sum())), r.uniform(0, rr.H, int(out.sum()))]
        matches[i] = np.rint(np.c_[px, p2]).astype(np.int32)
    matches.setflags(write=False)
    views2.setflags(write=False)
    return view1, views2, matches


def handmade():
    """Matches made by hand so that stages 1 and 3 occur -> (view1, view2, matches int32 [3, 4]).  View 1 is the origin,
    view 2 one unit to its right with the same orientation.  Match 0: both rays along the optical axis -- parallel, so
    the point is at infinity and column 2 of the 4 x 4 matrix is exactly zero: the null vector is (0, 0, 1, 0) exactly in
    any arithmetic, hom[3] == 0, stage 3.  Match 1: end points 1000 px right and left of the principal points, rays
    more than 90 degrees apart, stage 1.  Match 2: a point at (0.5, 0, 5), accepted."""
    v1 = make_view(np.eye(3), np.zeros(3))
    v2 = make_view(np.eye(3), np.array([-1.0, 0.0, 0.0]))
    m = np.array([[320, 240, 320, 240], [1320, 240, -680, 240], [370, 240, 270, 240]], np.int32)
    return v1, v2, m


# ---- the reference ----
def _f32_front(matches, v1, v2):
    """everything in front of the SVD, in f32 in the reference's order -> (kp [n, 4] f32, cos f64 [n], A f32 [n, 4, 4])"""
    m = np.asarray(matches, np.int32).reshape(-1, 4).astype(np.float32)
    one = np.float32(1)
    xn, rays, T = [], [], []
    for v, kx, ky in ((v1, m[:, 0], m[:, 1]), (v2, m[:, 2], m[:, 3])):
        R = np.asarray(v["Rcw"], np.float32).reshape(3, 3)
        invfx, invfy = one / np.float32(v["fx"]), one / np.float32(v["fy"])
        x = np.stack([(kx - np.float32(v["cx"])) * invfx, (ky - np.float32(v["cy"])) * invfy, np.ones_like(kx)], 1)
        ray = np.stack([(R[0, r] * x[:, 0] + R[1, r] * x[:, 1]) + R[2, r] * x[:, 2] for r in range(3)], 1)   # Rcw' xn
        assert ray.dtype == np.float32
        xn.append(x)
        rays.append(ray.astype(np.float64))
        T.append(np.c_[R, np.asarray(v["tcw"], np.float32).reshape(3, 1)])
    r1, r2 = rays
    dot = (r1[:, 0] * r2[:, 0] + r1[:, 1] * r2[:, 1]) + r1[:, 2] * r2[:, 2]
    n1 = np.sqrt((r1[:, 0] * r1[:, 0] + r1[:, 1] * r1[:, 1]) + r1[:, 2] * r1[:, 2])
    n2 = np.sqrt((r2[:, 0] * r2[:, 0] + r2[:, 1] * r2[:, 1]) + r2[:, 2] * r2[:, 2])
    cos = dot / (n1 * n2)
    A = np.stack([xn[0][:, 0:1] * T[0][2] - T[0][0], xn[0][:, 1:2] * T[0][2] - T[0][1],
                  xn[1][:, 0:1] * T[1][2] - T[1][0], xn[1][:, 1:2] * T[1][2] - T[1][1]], 1)
    assert A.dtype == np.float32
    return m, cos, A


def _camera(v, p):
    """f64: Rcw p + tcw on f32 entries, summed left to right -> (x, y, z)"""
    R = np.asarray(v["Rcw"], np.float32).reshape(3, 3).astype(np.float64)
    t = np.asarray(v["tcw"], np.float32).astype(np.float64)
    return [((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r] for r in range(3)]


def stages_from_points(m, v1, v2, hom, p, chi2, alive):
    """Stages 3-7 in f64 from the null vectors hom [n, 4] and the points p [n, 3] = hom[:3] / hom[3] (f32 entries read
    as f64) for the matches `alive` at stage 3.  -> (status [n] with 0 for rows not alive or accepted, near [n]: within
    1e-9 relative of a threshold, quantities dict)"""
    n = len(m)
    p = np.asarray(p, np.float64)
    status = np.zeros(n, np.int32)
    alive = alive.copy()
    with np.errstate(all="ignore"):
        bad = (np.asarray(hom)[:, 3] == 0) | ~np.isfinite(p).all(1)
        status[alive & bad] = 3
        alive &= ~bad
        near = np.zeros(n, bool)
        q = {}
        z = {}
        for k, v in ((1, v1), (2, v2)):
            x, y, zz = _camera(v, p)
            z[k] = (x, y, zz)
            q["z%d" % k] = zz
            q["norm%d" % k] = np.sqrt(x * x + y * y + zz * zz)
            near |= alive & (np.abs(zz) <= 1e-9 * q["norm%d" % k])
            status[alive & (zz <= 0)] = 3 + k
            alive &= ~(zz <= 0)
        for k, v, kx, ky in ((1, v1, m[:, 0], m[:, 1]), (2, v2, m[:, 2], m[:, 3])):
            x, y, zz = z[k]
            invz = 1.0 / zz
            u = np.float64(v["fx"]) * x * invz + np.float64(v["cx"])
            w = np.float64(v["fy"]) * y * invz + np.float64(v["cy"])
            ex, ey = u - kx.astype(np.float64), w - ky.astype(np.float64)
            e = ex * ex + ey * ey
            q["e%d" % k] = e
            near |= alive & (np.abs(e - chi2) <= 1e-9 * chi2)
            status[alive & (e > chi2)] = 5 + k
            alive &= ~(e > chi2)
    return status, near, q


def new_points(matches, v1, v2, max_cos=1.1, chi2=CHI2, dtype=np.float64):
    """-> dict: status int32 [n], borderline bool [n], reached bool [n] (the triangulation), cos f64 [n], A f32 [n, 4, 4],
    hom [n, 4] (unit null vector, dtype), s [n, 4] singular values, bound [n] = 16 EPS s1 / (s3 - s4), uninformative
    bool [n], points [n, 3] (dtype; zero where status != 0), n_new"""
    m, cos, A = _f32_front(matches, v1, v2)
    n = len(m)
    status = np.zeros(n, np.int32)
    border = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        alive = np.ones(n, bool)
        border |= alive & (np.abs(cos) <= 1e-6)
        status[alive & ~(cos > 0)] = 1
        alive &= cos > 0
        border |= alive & (np.abs(cos - max_cos) <= 1e-6)
        status[alive & ~(cos < max_cos)] = 2
        alive &= cos < max_cos
        reached = alive.copy()
        hom = np.full((n, 4), np.nan, dtype)
        s = np.full((n, 4), np.nan, np.float64)
        ok_rows = np.isfinite(A).all((1, 2))
        if ok_rows.any():
            _, sv, vt = np.linalg.svd(A[ok_rows].astype(dtype))
            hom[ok_rows] = vt[:, 3]
            s[ok_rows] = sv
        bound = 16 * EPS * s[:, 0] / (s[:, 2] - s[:, 3])
        uninformative = reached & ~(bound <= rr.UNINFORMATIVE)
        border |= uninformative
        border |= reached & (np.abs(hom[:, 3].astype(np.float64)) <= bound)
        p = (hom[:, :3] / hom[:, 3:]).astype(dtype)
        st, _, q = stages_from_points(m, v1, v2, hom, p, chi2, alive)
        status[alive] = st[alive]
        # the bands of stages 4-7, each for the matches alive at it
        live = alive & (st != 3)
        for k in (1, 2):
            border |= live & (np.abs(q["z%d" % k]) <= 1e-3 * q["norm%d" % k])
            live = live & ~(q["z%d" % k] <= 0)
        for k in (1, 2):
            border |= live & (np.abs(q["e%d" % k] - chi2) <= 0.01 * chi2)
            live = live & ~(q["e%d" % k] > chi2)
    accepted = status == 0
    pts = np.where(accepted[:, None], p, 0)
    return dict(status=status, borderline=border, reached=reached, cos=cos, A=A, hom=hom, s=s, bound=bound,
                uninformative=uninformative, points=pts, n_new=int(accepted.sum()))


@functools.lru_cache(maxsize=None)
def scene_reference(seed, max_cos, f32=False):
    """new_points() of the 8 lists of a scene; computed once and shared: do not modify"""
    view1, views2, matches = scene(seed)
    return [new_points(matches[i], view1, views2[i], max_cos, CHI2, np.float32 if f32 else np.float64)
            for i in range(N_NEIGHBOURS)]


@functools.lru_cache(maxsize=None)
def handmade_reference():
    v1, v2, m = handmade()
    return new_points(m, v1, v2, 1.1, CHI2)


# ---- the bars ----
def check_result(ref, got, matches, v1, v2, max_cos=1.1, chi2=CHI2, label=""):
    """Every bar on one list's result against ref = new_points(...) in float64; prints each figure before it asserts.
    got: n_new, status [n], points [n, 3], hom [n, 4], cos_parallax [n], packed (records with match, x, y, z).
    -> (worst null-vector error as a share of its bar, number of borderline matches)"""
    m = np.asarray(matches, np.int32).reshape(-1, 4).astype(np.float32)
    n = len(m)
    status = np.asarray(got["status"]).astype(np.int32)
    pts = np.asarray(got["points"], np.float32).reshape(n, 3)
    hom = np.asarray(got["hom"], np.float32).reshape(n, 4)
    cos = np.asarray(got["cos_parallax"], np.float64)
    assert status.shape == (n,) and ((status >= 0) & (status <= 7)).all()
    # (a) the cosine: f64 on f32 rays
    fin = np.isfinite(ref["cos"])
    rel = np.abs(cos[fin] - ref["cos"][fin]) / np.maximum(np.abs(ref["cos"][fin]), 1e-300)
    print("%s: cos_parallax off by %.3e relative (bar 1e-12)" % (label, rel.max() if len(rel) else 0.0))
    assert (rel <= 1e-12).all() and not np.isfinite(cos[~fin]).any()
    # (b) the null vector on every informative row that reached the triangulation, and the division
    rows = ref["reached"] & ((status == 0) | (status >= 3)) & ~ref["uninformative"]
    worst = 0.0
    if rows.any():
        h = hom[rows].astype(np.float64)
        h = h / np.linalg.norm(h, axis=1, keepdims=True)
        v = ref["hom"][rows].astype(np.float64)
        err = np.minimum(np.linalg.norm(h - v, axis=1), np.linalg.norm(h + v, axis=1))
        worst = float((err / ref["bound"][rows]).max())
        print("%s: null vector worst err / bound %.3f over %d rows" % (label, worst, int(rows.sum())))
        assert worst <= 1.0
    with np.errstate(all="ignore"):
        div = hom[:, :3] / hom[:, 3:]
    acc = status == 0
    assert np.array_equal(pts[acc].view(np.uint32), div[acc].view(np.uint32)) and not pts[~acc].any()
    assert not hom[(status == 1) | (status == 2)].any()
    # (c) self-consistency: stages 3-7 in f64 from the result's own null vector and point
    alive = status >= 3
    alive |= acc
    st, near, _ = stages_from_points(m, v1, v2, hom, div, chi2, alive)
    keep = alive & ~near
    assert np.array_equal(st[keep], status[keep]), (label, np.flatnonzero(keep & (st != status))[:8])
    # (d) end to end against float64
    b = ref["borderline"]
    keep = ~b
    print("%s: n_new %d (%d), %d borderline of %d" % (label, int(got["n_new"]), ref["n_new"], int(b.sum()), n))
    assert np.array_equal(status[keep], ref["status"][keep]), (label, np.flatnonzero(keep & (status != ref["status"]))[:8])
    assert abs(int(got["n_new"]) - ref["n_new"]) <= int(b.sum())
    # (e) the packed records: the accepted matches in ascending order with the points' values
    idx = np.flatnonzero(acc)
    packed = np.asarray(got["packed"])
    assert int(got["n_new"]) == len(idx) and len(packed) >= len(idx)
    packed = packed[:len(idx)]
    assert np.array_equal(packed["match"], idx)
    for k, name in enumerate("xyz"):
        assert np.array_equal(packed[name].view(np.uint32), pts[idx, k].view(np.uint32))
    return worst, int(b.sum())
