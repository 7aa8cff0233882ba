"""Reference for include/msf_tracking.h (Tracking::SearchLocalPoints, slam_pipeline/src/Tracking.cc:594-632, with
Frame::isInFrustum, Frame.cc:48-84), written here from the reference's text:

  literal()            the sequential loop restated literally: dicts for the KeyPointMaps, mnTrackReferenceForFrame and
                       mnLastFrameSeen per point, MatchFrames only behind nToMatch > 0, SetMapPoint as it goes
  order_independent()  the statement the header gives: owner = smallest entry, gate = n_to_match > 0, the claim of a
                       pixel goes to the smallest ordinal
  frustum_f32()        step 2 in numpy float32 in the order csrc/tracking_solve.h states (one rounding per operation)
  frustum_f64()        the same expressions in float64, with the forward bound of every value and the threshold bands

tests/test_tracking_ref.py proves literal() == order_independent() on random scenes and the tied cases; the GPU tests
hold the device to order_independent() exactly and to frustum_f64() outside the bands.

Bars.  eps = 2^-24.  Every bound is (roundings + 2) * eps * sum |terms| of the stated expression, inputs exact:
  Pc_r  = ((0 + R_r0 P_0) + R_r1 P_1) + R_r2 P_2) + t_r : 3 products, 2 roundings in the sum (0 + x is exact), 1 add
          -> 8 eps (sum_k |R_rk P_k| + |t_r|)
  u     = fx * PcX * invz + cx : invz, two products, one add -> 6 eps (|fx PcX / PcZ| + |cx|), plus what Pc hands on:
          |fx / PcZ| dPcX + |fx PcX / PcZ^2| dPcZ                      (v likewise)
  dist  = (float)sqrt(sum (double)PO_k^2), PO_k = P_k - Ow_k : one rounding per PO_k, the cast -> 4 eps dist
  cos   = (float)(sum PO_k n_k / dist) : PO_k, dist, the cast -> 5 eps sum_k |PO_k n_k| / dist
A threshold band is that bound around each comparison; a point inside a band is excluded from the status comparison
with float64 (never from the bit comparison with the host build).
"""
import numpy as np

EPS = 2.0 ** -24
W, H = 640, 480
MAP_POINT = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("max_distance", "<f4"), ("flags", "<u4")])
CLAIM = np.dtype([("key", "<i4"), ("point", "<i4"), ("kf", "<i4"), ("match", "<i4")])
BAD, SEEN = 1, 2


# ---- step 2 -----------------------------------------------------------------------------------------------------------

def frustum_f32(points, prm):
    """-> (status uint8 [n] of codes 0..6, diag f32 [n, 4] = u, v, dist, viewCos; 0 behind the rejecting stage, NaN
    canonical), in numpy float32, one rounding per operation, in the order of csrc/tracking_solve.h"""
    f = np.float32
    P = points["pos"].astype(f)
    n = len(P)
    R, t = np.asarray(prm["Rcw"], f).reshape(3, 3), np.asarray(prm["tcw"], f)
    with np.errstate(all="ignore"):
        pc = []
        for r in range(3):
            s = np.zeros(n, f)
            for k in range(3):
                s = s + R[r, k] * P[:, k]
            pc.append(s + t[r])
        invz = f(1.0) / pc[2]
        u = f(prm["fx"]) * pc[0] * invz + f(prm["cx"])
        v = f(prm["fy"]) * pc[1] * invz + f(prm["cy"])
        po = P - np.asarray(prm["Ow"], f)
        po64 = po.astype(np.float64)
        dist = np.sqrt(po64[:, 0] * po64[:, 0] + po64[:, 1] * po64[:, 1] + po64[:, 2] * po64[:, 2]).astype(f)
        nn = points["normal"].astype(np.float64)
        dot = po64[:, 0] * nn[:, 0] + po64[:, 1] * nn[:, 1] + po64[:, 2] * nn[:, 2]
        cos = (dot / dist.astype(np.float64)).astype(f)
        status = np.full(n, 255, np.uint8)
        stage = np.zeros(n, np.int32)   # how many of the four diagnostics were computed

        def decide(cond, code, upto):
            m = (status == 255) & cond
            status[m] = code
            stage[m] = upto
        decide(pc[2] < 0, 1, 0)
        decide(~np.isfinite(u) | ~np.isfinite(v), 6, 2)
        decide((u < f(prm["min_x"])) | (u > f(prm["max_x"])), 2, 2)
        decide((v < f(prm["min_y"])) | (v > f(prm["max_y"])), 3, 2)
        decide(~np.isfinite(dist), 6, 3)
        decide(dist > points["max_distance"], 4, 3)
        decide(~np.isfinite(cos), 6, 4)
        decide(cos < f(prm["cos_limit"]), 5, 4)
        decide(np.ones(n, bool), 0, 4)
    diag = np.stack([u, v, dist, cos], axis=1).astype(f)
    for k in range(4):
        diag[stage <= k, k] = 0
    diag[np.isnan(diag)] = np.float32(np.nan)
    return status, diag


def frustum_f64(points, prm):
    """-> dict: status [n] (codes 0..6 in float64), value [n, 4] (u, v, dist, cos), bound [n, 4], band bool [n] (a
    comparison up to the deciding one lies within its bound of the threshold), upto [n] (diagnostics computed)"""
    d = np.float64
    P = points["pos"].astype(d)
    n = len(P)
    R, t = np.asarray(prm["Rcw"], d).reshape(3, 3), np.asarray(prm["tcw"], d)
    fx, fy, cx, cy = (d(prm[k]) for k in ("fx", "fy", "cx", "cy"))
    with np.errstate(all="ignore"):
        pc = P @ R.T + t
        dpc = 8 * EPS * (np.abs(P) @ np.abs(R).T + np.abs(t))
        z = pc[:, 2]
        u = fx * pc[:, 0] / z + cx
        v = fy * pc[:, 1] / z + cy
        du = 6 * EPS * (np.abs(fx * pc[:, 0] / z) + abs(cx)) + np.abs(fx / z) * dpc[:, 0] + np.abs(fx * pc[:, 0] / z ** 2) * dpc[:, 2]
        dv = 6 * EPS * (np.abs(fy * pc[:, 1] / z) + abs(cy)) + np.abs(fy / z) * dpc[:, 1] + np.abs(fy * pc[:, 1] / z ** 2) * dpc[:, 2]
        po = P - np.asarray(prm["Ow"], d)
        dist = np.sqrt((po * po).sum(1))
        ddist = 4 * EPS * dist
        nn = points["normal"].astype(d)
        cos = (po * nn).sum(1) / dist
        dcos = 5 * EPS * np.abs(po * nn).sum(1) / dist
    status = np.full(n, 255, np.uint8)
    upto = np.zeros(n, np.int32)
    band = np.zeros(n, bool)

    def near(x, thr, dx):
        with np.errstate(all="ignore"):
            return (status == 255) & (np.abs(x - thr) <= dx)   # a NaN value is decided by isfinite, exactly on both sides

    def decide(cond, code, k):
        m = (status == 255) & cond
        status[m] = code
        upto[m] = k
    band |= near(z, 0.0, dpc[:, 2])
    decide(z < 0, 1, 0)
    decide(~np.isfinite(u) | ~np.isfinite(v), 6, 2)
    band |= near(u, d(prm["min_x"]), du) | near(u, d(prm["max_x"]), du)
    decide((u < prm["min_x"]) | (u > prm["max_x"]), 2, 2)
    band |= near(v, d(prm["min_y"]), dv) | near(v, d(prm["max_y"]), dv)
    decide((v < prm["min_y"]) | (v > prm["max_y"]), 3, 2)
    decide(~np.isfinite(dist), 6, 3)
    band |= near(dist, points["max_distance"].astype(d), ddist)
    decide(dist > points["max_distance"], 4, 3)
    decide(~np.isfinite(cos), 6, 4)
    band |= near(cos, d(prm["cos_limit"]), dcos)
    decide(cos < prm["cos_limit"], 5, 4)
    decide(np.ones(n, bool), 0, 4)
    return dict(status=status, value=np.stack([u, v, dist, cos], 1), bound=np.stack([du, dv, ddist, dcos], 1), band=band,
                upto=upto)


def check_against_f64(points, prm, status, diag, flagged, label=""):
    """Holds a build's step 2 (status [n] with the codes 7..9 already applied where `flagged`, diag [n, 4]) to the
    float64 recomputation: the diagnostics within their bounds, the status equal outside the bands.  -> (worst fraction
    of a bar, fraction of points inside a band)"""
    ref = frustum_f64(points, prm)
    free = ~flagged
    worst = 0.0
    for k in range(4):
        m = free & (ref["upto"] > k) & np.isfinite(ref["value"][:, k]) & ~ref["band"]
        m &= np.asarray(status) == ref["status"]     # the same stages were computed
        if not m.any():
            continue
        err = np.abs(diag[m, k].astype(np.float64) - ref["value"][m, k])
        frac = err / ref["bound"][m, k]
        assert (frac <= 1.0).all(), "%s diagnostic %d: worst err / bound %.3f" % (label, k, frac.max())
        worst = max(worst, float(frac.max()))
    m = free & ~ref["band"]
    assert np.array_equal(np.asarray(status)[m], ref["status"][m]), "%s status differs from float64 outside the bands" % label
    return worst, float((free & ref["band"]).mean()) if len(points) else 0.0


# ---- the two statements of the loop -----------------------------------------------------------------------------------

def pixel_key(x, y):
    return int(y) * W + int(x) if 0 <= x < W and 0 <= y < H else None


def list_of(lists, n_out, cap, i):
    return lists[i][:max(min(int(n_out[i]), cap), 0)]


def order_independent(lmap, prm, lists, n_out, cap, corr_cap, matched=None):
    """The header's statement.  lists [n_kf] of int [k, 4], n_out [n_kf] (may exceed cap or be -1).  matched None: the
    gate of step 3, else the bytes to use.  -> dict of every output of the five steps"""
    pts = lmap["points"]
    n_points, n_kf = len(pts), max(len(lmap["kf_start"]) - 1, 0)
    start, kkey, kpoint = lmap["kf_start"], lmap["kf_key"], lmap["kf_point"]
    owner = np.full(n_points, -1, np.int64)
    for e in range(len(kpoint) - 1, -1, -1):
        owner[kpoint[e]] = e
    owner_kf = np.full(n_points, -1, np.int32)
    for p in range(n_points):
        if owner[p] >= 0:
            owner_kf[p] = np.searchsorted(start, owner[p], side="right") - 1
    st32, diag = frustum_f32(pts, prm)
    status = st32.copy()
    status[(pts["flags"] & SEEN) != 0] = 8
    status[(pts["flags"] & BAD) != 0] = 7
    status[owner_kf < 0] = 9
    diag[status >= 7] = 0
    n_to_match = np.zeros(n_kf, np.int32)
    for p in range(n_points):
        if status[p] == 0:
            n_to_match[owner_kf[p]] += 1
    if matched is None:
        matched = (n_to_match > 0).astype(np.uint8)
    occupied = set(int(k) for k in lmap["cur_key"])
    cand, best = {}, {}
    claim_status = np.full((n_kf, cap), 255, np.uint8)
    for i in range(n_kf):
        if not matched[i]:
            continue
        at = {int(kkey[e]): int(kpoint[e]) for e in range(start[i], start[i + 1])}
        for j, (x1, y1, x2, y2) in enumerate(list_of(lists, n_out, cap, i)):
            k1, k2 = pixel_key(x1, y1), pixel_key(x2, y2)
            if k1 is None:
                claim_status[i, j] = 1
            elif k1 in occupied:
                claim_status[i, j] = 2
            elif k2 is None or k2 not in at:
                claim_status[i, j] = 3
            else:
                cand[(i, j)] = (k1, at[k2])
                best[k1] = min(best.get(k1, (i, j)), (i, j))
    claims, n_claimed = [], np.zeros(n_kf, np.int32)
    for (i, j) in sorted(cand):
        k1, p = cand[(i, j)]
        won = best[k1] == (i, j)
        claim_status[i, j] = 0 if won else 4
        if won:
            claims.append((k1, p, i, j))
            n_claimed[i] += 1
    claims = np.array(claims, np.int32).reshape(-1, 4)
    corr = [(int(k), int(p)) for k, p in zip(lmap["cur_key"], lmap["cur_point"])] + [(int(c[0]), int(c[1])) for c in claims]
    fits = len(corr) <= corr_cap
    out = dict(owner_kf=owner_kf, status=status, visible=(status == 0).astype(np.uint8), n_to_match=n_to_match, diag=diag,
               matched=np.asarray(matched, np.uint8), claim_status=claim_status, claims=claims, n_claimed=n_claimed,
               n_claims=len(claims), n_corr=len(corr) if fits else -1)
    if fits:
        out["corr_point"] = np.array([p for _, p in corr], np.int32)
        out["corr_p2d"] = np.array([(k % W, k // W) for k, _ in corr], np.float32).reshape(-1, 2)
        out["corr_p3d"] = np.array([pts["pos"][p] for _, p in corr], np.float32).reshape(-1, 3)
    return out


def literal(lmap, prm, lists, n_out, cap, frame_id=7):
    """Tracking.cc:594-632 restated line by line.  The first loop of :576-592 has run: the frame's map is cur_key ->
    cur_point and the points it holds carry mnLastFrameSeen == frame_id (the SEEN flag).  -> dict: visible (the points
    that got IncreaseVisible here), n_to_match per key frame, matched, the SetMapPoint calls in order, the final map"""
    pts = lmap["points"]
    in_frustum = frustum_f32(pts, prm)[0] == 0                       # Frame::isInFrustum per point, NaN rejected (code 6)
    mnTrackReferenceForFrame = {}
    mnLastFrameSeen = {p: frame_id for p in range(len(pts)) if pts["flags"][p] & SEEN}
    cur_map = {int(k): int(p) for k, p in zip(lmap["cur_key"], lmap["cur_point"])}
    visible, n_to_match, matched, calls = [], [], [], []
    start = lmap["kf_start"]
    for i in range(max(len(start) - 1, 0)):
        vpMPs = {int(lmap["kf_key"][e]): int(lmap["kf_point"][e]) for e in range(start[i], start[i + 1])}
        nToMatch = 0
        for key in sorted(vpMPs):                                    # the map iterates in key order
            pMP = vpMPs[key]
            if mnTrackReferenceForFrame.get(pMP) == frame_id:
                continue
            if not (pts["flags"][pMP] & BAD):
                mnTrackReferenceForFrame[pMP] = frame_id
                if mnLastFrameSeen.get(pMP) != frame_id:
                    if in_frustum[pMP]:
                        visible.append(pMP)
                        nToMatch += 1
        n_to_match.append(nToMatch)
        matched.append(int(nToMatch > 0))
        if nToMatch > 0:
            for j, (x1, y1, x2, y2) in enumerate(list_of(lists, n_out, cap, i)):   # MatchFrames(current, KF)
                k1, k2 = pixel_key(x1, y1), pixel_key(x2, y2)
                pMP1 = cur_map.get(k1) if k1 is not None else None    # GetMapPoint ignores a point outside the image
                pMP2 = vpMPs.get(k2) if k2 is not None else None
                if pMP1 is None and pMP2 is not None:
                    if k1 is not None:                                # so does SetMapPoint
                        cur_map[k1] = pMP2
                        calls.append((k1, pMP2, i, j))
    return dict(visible=sorted(visible), n_to_match=np.array(n_to_match, np.int32), matched=np.array(matched, np.uint8),
                calls=np.array(calls, np.int32).reshape(-1, 4), cur_map=cur_map)


# ---- scenes -------------------------------------------------------------------------------------------------------------

def camera(seed=0):
    """-> prm dict: a camera near the origin looking down +z, 640 x 480, Ow = -Rcw' tcw in f32"""
    rng = np.random.default_rng(1000 + seed)
    a = rng.normal(0, 0.03, 3)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.linalg.qr(np.eye(3) + K)[0]
    R *= np.sign(np.diag(R))
    R = R.astype(np.float32)
    t = rng.normal(0, 0.1, 3).astype(np.float32)
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(np.float32)
    return dict(Rcw=R.reshape(9), tcw=t, fx=np.float32(500), fy=np.float32(500), cx=np.float32(320), cy=np.float32(240),
                Ow=Ow, min_x=np.float32(0), max_x=np.float32(W), min_y=np.float32(0), max_y=np.float32(H),
                cos_limit=np.float32(0.5))


def view_of(prm):
    return (prm["Rcw"].reshape(3, 3), prm["tcw"], float(prm["fx"]), float(prm["fy"]), float(prm["cx"]), float(prm["cy"]))


def bounds_of(prm):
    return (float(prm["min_x"]), float(prm["max_x"]), float(prm["min_y"]), float(prm["max_y"]))


def scene(seed, n_points=900, n_kf=8, per_kf=200, n_cur=150, list_len=160, empty_kf=None, kf_sizes=None):
    """A local map and match lists that reach every frustum code and every claim status: the camera looks at a slab of
    depths 2..8; of the points some lie behind the camera, outside each image edge, beyond max_distance, are seen at
    more than 60 degrees, are bad, seen, not finite or referred to by no entry.  kf_sizes [n_kf]: the exact entry count
    of every key frame in place of per_kf +- 10 (no draw is made for a size then; without it every draw is what it was,
    which test_tracking_ref.py pins).
    -> (lmap dict as matcher.make_local_map gives it, prm, lists [n_kf] int32 [k, 4], n_out int32 [n_kf])"""
    assert kf_sizes is None or len(kf_sizes) == n_kf
    rng = np.random.default_rng(seed)
    prm = camera(seed)
    R, t = prm["Rcw"].reshape(3, 3).astype(np.float64), prm["tcw"].astype(np.float64)
    pts = np.zeros(n_points, MAP_POINT)
    kind = rng.choice(12, n_points, p=[0.52, 0.06, 0.03, 0.03, 0.03, 0.03, 0.06, 0.06, 0.05, 0.05, 0.02, 0.06])
    for p in range(n_points):
        z = rng.uniform(2, 8)
        px, py = rng.uniform(20, W - 20), rng.uniform(20, H - 20)
        k = kind[p]
        if k == 1: z = -z
        if k == 2: px = rng.uniform(-200, -5)
        if k == 3: px = rng.uniform(W + 5, W + 200)
        if k == 4: py = rng.uniform(-200, -5)
        if k == 5: py = rng.uniform(H + 5, H + 200)
        pc = np.array([(px - 320) / 500 * z, (py - 240) / 500 * z, z])
        pos = (R.T @ (pc - t)).astype(np.float32)
        po = pos.astype(np.float64) - prm["Ow"].astype(np.float64)
        dist = np.linalg.norm(po)
        nrm = po / dist + rng.normal(0, 0.1, 3)
        nrm /= np.linalg.norm(nrm)
        if k == 7:    # seen at more than 60 degrees
            side = np.cross(po, rng.normal(0, 1, 3))
            side /= np.linalg.norm(side)
            ang = rng.uniform(np.radians(65), np.radians(120))
            nrm = np.cos(ang) * po / dist + np.sin(ang) * side
        pts["pos"][p] = pos
        pts["normal"][p] = nrm
        pts["max_distance"][p] = dist * (rng.uniform(0.3, 0.9) if k == 6 else rng.uniform(1.2, 3.0))
        if k == 8: pts["flags"][p] = BAD
        if k == 10: pts["pos"][p, rng.integers(3)] = np.nan if rng.random() < 0.7 else np.inf
    referred = np.flatnonzero(kind != 11)
    # the frame's own map: the seen points, each under a pixel of its own
    seen = np.flatnonzero(kind == 9)
    pts["flags"][seen] |= SEEN
    more = rng.choice(referred, max(n_cur - len(seen), 0)) if len(referred) else np.zeros(0, np.int64)
    cur_point = np.concatenate([seen, more]).astype(np.int32)[:n_cur]
    cur_key = np.sort(rng.choice(W * H, len(cur_point), replace=False)).astype(np.int32)
    kf_start, kf_key, kf_point = [0], [], []
    for i in range(n_kf):
        if kf_sizes is not None:
            m = int(kf_sizes[i]) if len(referred) else 0
        else:
            m = 0 if i == empty_kf or not len(referred) else per_kf + int(rng.integers(-10, 10))
        kf_key.append(np.sort(rng.choice(W * H, m, replace=False)))
        kp = rng.choice(referred, m) if m else np.zeros(0, np.int64)
        if m > 4:
            kp[1] = kp[0]       # a point twice inside one key frame, under two keys
        kf_point.append(kp)
        kf_start.append(kf_start[-1] + m)
    lmap = dict(points=pts, kf_start=np.array(kf_start if n_kf else [], np.int32),
                kf_key=np.concatenate(kf_key + [np.zeros(0, np.int64)]).astype(np.int32),
                kf_point=np.concatenate(kf_point + [np.zeros(0, np.int64)]).astype(np.int32), cur_key=cur_key, cur_point=cur_point)
    lists, used = [], []
    for i in range(n_kf):
        keys = lmap["kf_key"][kf_start[i]:kf_start[i + 1]]
        rows = []
        for j in range(list_len + int(rng.integers(-20, 20))):
            c = rng.choice(5, p=[0.55, 0.08, 0.1, 0.12, 0.15])
            k1 = int(rng.integers(W * H))
            k2 = int(rng.choice(keys)) if len(keys) else int(rng.integers(W * H))
            x1, y1, x2, y2 = k1 % W, k1 // W, k2 % W, k2 // W
            if c == 1: x1, y1 = [(-1, y1), (W, y1), (x1, -1), (x1, H)][int(rng.integers(4))]
            if c == 2 and len(cur_key):
                kk = int(rng.choice(cur_key)); x1, y1 = kk % W, kk // W
            if c == 3:
                if rng.random() < 0.3: x2 = W + 3
                else:
                    kk = int(rng.integers(W * H)); x2, y2 = kk % W, kk // W
            if c == 4 and used:
                kk = used[int(rng.integers(len(used)))]; x1, y1 = kk % W, kk // W
            rows.append((x1, y1, x2, y2))
            if 0 <= x1 < W and 0 <= y1 < H:
                used.append(y1 * W + x1)
        lists.append(np.array(rows, np.int32).reshape(-1, 4))
    n_out = np.array([len(l) for l in lists], np.int32)
    return lmap, prm, lists, n_out


def tied_case():
    """The LoFTR cell-centre case and the edges: the same k1 in three key frames and three times inside one list, k1 at
    (0, 0) and (W - 1, H - 1), end points at -1 and at W, k1 occupied, k2 without an entry, an unmatched key frame in
    the middle and an invalid list.  -> (lmap, prm, lists, n_out)"""
    prm = camera(0)
    R, t = prm["Rcw"].reshape(3, 3).astype(np.float64), prm["tcw"].astype(np.float64)
    pts = np.zeros(12, MAP_POINT)
    for p in range(12):
        pc = np.array([0.1 * (p % 4) - 0.15, 0.1 * (p // 4) - 0.1, 4.0 if p < 8 else -4.0])   # points 8..11 behind the camera
        pos = (R.T @ (pc - t)).astype(np.float32)
        po = pos.astype(np.float64) - prm["Ow"].astype(np.float64)
        pts["pos"][p], pts["normal"][p], pts["max_distance"][p] = pos, po / np.linalg.norm(po), 100.0
    pts["flags"][3] = BAD      # claimed all the same: the reference checks nothing at pMP2
    key = lambda x, y: y * W + x
    # key frame 0: points 0..3; 1: only points behind the camera (unmatched); 2: points 4..7 and point 0 again; 3: 4, 5
    kf = [[(key(8, 8), 0), (key(24, 8), 1), (key(40, 8), 2), (key(56, 8), 3)],
          [(key(8, 8), 8), (key(24, 8), 9)],
          [(key(8, 8), 4), (key(24, 8), 5), (key(40, 8), 6), (key(56, 8), 7), (key(72, 8), 0)],
          [(key(8, 8), 4), (key(24, 8), 5)],
          [(key(8, 8), 6)]]
    start = np.cumsum([0] + [len(k) for k in kf]).astype(np.int32)
    lmap = dict(points=pts, kf_start=start, kf_key=np.array([k for f in kf for k, _ in f], np.int32),
                kf_point=np.array([p for f in kf for _, p in f], np.int32),
                cur_key=np.array([key(100, 100), key(200, 100)], np.int32), cur_point=np.array([1, 2], np.int32))
    lists = [np.array([(8, 8, 8, 8), (8, 8, 24, 8), (8, 8, 40, 8),          # the same k1 three times in one list
                       (0, 0, 56, 8), (W - 1, H - 1, 8, 8),                  # the corners; point 3 is bad and is claimed
                       (-1, 5, 8, 8), (W, 5, 8, 8), (5, -1, 8, 8), (5, H, 8, 8),
                       (100, 100, 8, 8),                                      # occupied
                       (300, 300, 9, 8), (301, 300, -1, 8), (302, 300, W, 8)], np.int32),   # no point at k2
             np.array([(50, 50, 8, 8), (8, 8, 24, 8)], np.int32),             # unmatched: takes no part
             np.array([(8, 8, 8, 8), (50, 50, 24, 8), (0, 0, 8, 8), (60, 60, 72, 8)], np.int32),
             np.array([(8, 8, 8, 8), (50, 50, 8, 8), (70, 70, 24, 8), (71, 70, 24, 8)], np.int32),
             np.array([(90, 90, 8, 8)], np.int32)]                            # invalid: n_out = -1
    n_out = np.array([len(lists[0]), 2, 4, 4, -1], np.int32)
    return lmap, prm, lists, n_out


# ---- scenes past one chunk of 256 -----------------------------------------------------------------------------------------
# tracking_kernels.hip works in chunks of 256 threads: the entries of a key frame, the key frames, the frame's own map and
# the matches of a list each have code that only runs past the first chunk.  The cases below reach it; the CPU tests
# hold literal(), order_independent() and the host build to each other on them and assert that they do reach it, the
# GPU tests hold the device to the same references.

def ladder_empty_runs(n_kf, n_empty_runs):
    """-> [(first, length)] of the ladder's stretches of empty key frames: the first at the very end, the second across
    index 256 (in the middle of a shorter ladder), the third in the first quarter"""
    assert 0 <= n_empty_runs <= 3 and (n_empty_runs == 0 or n_kf >= 32)
    runs = [(n_kf - 3, 3), (254, 5) if n_kf >= 270 else (n_kf // 2, 5), (n_kf // 4, 2)]
    return runs[:n_empty_runs]


def ladder(n_kf, rounds, n_empty_runs=0):
    """Deterministic.  Of the L non-empty key frames the q-th owns the points q, q + L, q + 2 L, ..: point p is owned by
    non-empty key frame p % L at entry p // L of its run, so with L >= 64 every aligned group of 64 points has 64
    owners.  Every point lies in front of the camera, projects inside the image, is seen head-on and has a large
    max_distance: status 0, n_to_match == rounds.  Every key frame but the first also refers, last in its run, to the
    first point of the one before it, which that one keeps.  The stretches of empty key frames (ladder_empty_runs)
    repeat values in kf_start.  The lists hold 4..6 matches: k1 shared by key frames i and i + 256 (the lower wins) and
    repeated inside the list, a free k1, one outside the image, an occupied one, a k2 without an entry.
    -> (lmap, prm, lists, n_out) as scene() gives them"""
    prm = camera(0)
    R, t = prm["Rcw"].reshape(3, 3).astype(np.float64), prm["tcw"].astype(np.float64)
    empty = np.zeros(n_kf, bool)
    for a, k in ladder_empty_runs(n_kf, n_empty_runs):
        empty[a:a + k] = True
    live = np.flatnonzero(~empty)
    L = len(live)
    n_points = L * rounds
    p = np.arange(n_points)
    z = 2.0 + p % 7
    pc = np.stack([(20 + (37 * p) % 601 - 320) / 500 * z, (20 + (53 * p) % 441 - 240) / 500 * z, z], 1)
    pts = np.zeros(n_points, MAP_POINT)
    pts["pos"] = ((pc - t) @ R).astype(np.float32)                 # R' (pc - t)
    po = pts["pos"].astype(np.float64) - prm["Ow"].astype(np.float64)
    pts["normal"] = po / np.linalg.norm(po, axis=1, keepdims=True)
    pts["max_distance"] = 100.0
    key_of = lambda q, r: 5000 * r + 7 * q                          # strictly increasing in r: 7 q < 5000
    cur_key = (300000 + 11 * np.arange(8)).astype(np.int32)
    cur_point = (np.arange(8) % n_points).astype(np.int32)
    kf_start, kf_key, kf_point, lists = [0], [], [], []
    for i in range(n_kf):
        q = int(np.searchsorted(live, i))
        if not empty[i]:
            kf_key += [key_of(q, r) for r in range(rounds)]
            kf_point += [q + r * L for r in range(rounds)]
            if q > 0:
                kf_key.append(key_of(q, rounds))
                kf_point.append(q - 1)
        kf_start.append(len(kf_key))
        shared, occupied = 100000 + i % 256, int(cur_key[i % 8])
        k2 = [key_of(q, 0), key_of(q, rounds - 1), key_of(q, 0), key_of(q, 0), key_of(q, 0) + 1, key_of(q, rounds)]
        rows = [(shared % W, shared // W), ((200000 + i) % W, (200000 + i) // W), (-1, i % H), (occupied % W, occupied // W),
                ((210000 + i) % W, (210000 + i) // W), (shared % W, shared // W)]
        rows = [(x1, y1, k % W, k // W) for (x1, y1), k in zip(rows, k2)][:4 + i % 3]
        lists.append(np.array(rows, np.int32).reshape(-1, 4))
    lmap = dict(points=pts, kf_start=np.array(kf_start, np.int32), kf_key=np.array(kf_key, np.int32),
                kf_point=np.array(kf_point, np.int32), cur_key=cur_key, cur_point=cur_point)
    return lmap, prm, lists, np.array([len(l) for l in lists], np.int32)


LONG = dict(n_points=3000, n_kf=4, per_kf=1000, n_cur=700, list_len=1100)
EDGE_SIZES = (255, 256, 257, 0, 512, 513, 1)
EDGE_N_OUT = (511, 512, 513, 256, 768, 1025, 257)      # over lists of at least 1100; key frame 3 has no entry
MANY_SIZES = tuple((7 * i) % 25 for i in range(300))   # 12 on average, none in every 25th key frame
LADDERS = ((63, 0), (64, 0), (65, 0), (255, 0), (256, 0), (257, 0), (257, 1), (320, 0), (320, 3))
LADDER_ROUNDS = 3


def _with_n_out(case, n_out):
    lmap, prm, lists, have = case
    assert all(h >= n for h, n in zip(have, n_out))
    return lmap, prm, lists, np.array(n_out, np.int32)


# name -> (builder, cap).  n_out stays above the cap where the cap clips.
CHUNK_CASES = {
    "long": (lambda: scene(21, **LONG), 1100),
    "long-cap512": (lambda: scene(21, **LONG), 512),
    "long-cap513": (lambda: scene(21, **LONG), 513),
    "few-points": (lambda: scene(22, n_points=300, n_kf=3, per_kf=600, n_cur=100, list_len=300), 320),
    "many-kf": (lambda: scene(23, n_points=2000, n_kf=300, kf_sizes=MANY_SIZES, n_cur=300, list_len=40), 64),
}
for _n_cur in (255, 256, 257):
    CHUNK_CASES["edges-cur%d" % _n_cur] = (
        lambda n_cur=_n_cur: _with_n_out(scene(24, n_points=1500, n_kf=7, kf_sizes=EDGE_SIZES, n_cur=n_cur, list_len=1130),
                                         EDGE_N_OUT), 1100)
for _n_kf, _runs in LADDERS:
    CHUNK_CASES["ladder-%d" % _n_kf + ("-empty" if _runs else "")] = (
        lambda n_kf=_n_kf, runs=_runs: ladder(n_kf, LADDER_ROUNDS, runs), 8)
SCENE_CASES = [k for k in CHUNK_CASES if not k.startswith("ladder")]
LADDER_CASES = [k for k in CHUNK_CASES if k.startswith("ladder")]

_built, _refs = {}, {}


def chunk_case(name):
    """-> (lmap, prm, lists, n_out, cap) of CHUNK_CASES[name], built once per process: the map's arrays and the lists
    are shared and read-only, n_out is the caller's own"""
    if name not in _built:
        lmap, prm, lists, n_out = CHUNK_CASES[name][0]()
        for a in list(lmap.values()) + lists + [n_out]:
            a.setflags(write=False)
        _built[name] = (lmap, prm, lists, n_out)
    lmap, prm, lists, n_out = _built[name]
    return lmap, prm, lists, n_out.copy(), CHUNK_CASES[name][1]


def corr_room(lmap, lists, cap):
    return len(lmap["cur_key"]) + len(lists) * cap


def chunk_reference(name, forced=False):
    """order_independent() of a case, computed once per process; forced: every key frame matched, else the gate of
    step 3.  corr_cap = n_cur + n_kf * cap"""
    if (name, forced) not in _refs:
        lmap, prm, lists, n_out, cap = chunk_case(name)
        matched = np.ones(len(lists), np.uint8) if forced else None
        _refs[(name, forced)] = order_independent(lmap, prm, lists, n_out, cap, corr_room(lmap, lists, cap), matched=matched)
    return _refs[(name, forced)]


def owner_entries(lmap):
    """-> (points that have an entry, the smallest entry index of each, its offset inside its key frame's run)"""
    points, first = np.unique(lmap["kf_point"], return_index=True)
    kf = np.searchsorted(lmap["kf_start"], first, side="right") - 1
    return points, first, first - lmap["kf_start"][kf]


def with_fault(lmap, key, at, value):
    """a copy of the map with one value replaced; key "flags" is points["flags"]"""
    bad = {k: v.copy() for k, v in lmap.items()}
    if key == "flags":
        bad["points"]["flags"][at] = value
    else:
        bad[key][at] = value
    return bad


def late_faults(lmap):
    """What a malformed map of the long-runs scene has wrong where only a later chunk or workgroup of k_track_check
    looks: -> [(key, at, value)], one fault per map.  a = the start of the second key frame's run."""
    a, n_points = int(lmap["kf_start"][1]), len(lmap["points"])
    faults = [("kf_key", a + 256, int(lmap["kf_key"][a + 255])),    # the comparison across the chunk edge
              ("kf_point", a + 700, n_points), ("flags", 2900, 4), ("cur_key", 256, int(lmap["cur_key"][255])),
              ("cur_point", 600, n_points)]
    assert lmap["kf_start"][2] > a + 700 and n_points > 2900 and len(lmap["cur_key"]) > 600
    return faults
