"""The body of Tracking::TrackWithMotionModel / TrackReferenceKeyFrame (slam_pipeline/src/Tracking.cc:434-485, :380-424)
twice: literal() restates the sequential code line by line -- a dict filled by SetMapPoint in list order, the early
return, the cut loop -- and order_independent() is the statement of include/msf_frame_tracking.h.
tests/test_frame_tracking_ref.py proves the two equal.  Both take the optimiser as a function of the gathered
correspondences, so that a test can put pose_ref.pose_optimization, the host build or the device's own outlier bytes
behind the carry.  The image is tracking_ref.W x H."""
import numpy as np

from tests import tracking_ref as tr

W, H = tr.W, tr.H
FRAME_POINT = np.dtype([("key", "<i4"), ("point", "<i4"), ("match", "<i4"), ("flags", "<i4")])
REMOVED = np.dtype([("key", "<i4"), ("point", "<i4")])
MAX_CANDIDATES = 8192
pixel_key = tr.pixel_key


def map_fault(fmap):
    """True for a map that the header calls malformed"""
    n_points = len(fmap["points"])
    for key, point in ((fmap["ref_key"], fmap["ref_point"]), (fmap["cur_key"], fmap["cur_point"])):
        key, point = np.asarray(key, np.int64), np.asarray(point, np.int64)
        if ((key < 0) | (key >= W * H)).any() or (np.diff(key) <= 0).any() or ((point < 0) | (point >= n_points)).any():
            return True
    return False


def is_observed(fmap, p):
    return fmap.get("observed") is None or bool(fmap["observed"][p])


def no_optimiser(keys, points):
    """-> (outliers, pose fields): nothing flagged"""
    return np.zeros(len(keys), bool), {}


def literal(fmap, matches, n, cap, min_matches, min_map_matches, optimise=no_optimiser):
    """Tracking.cc:448-484 restated.  fmap: a make_frame_map dict; matches int [k, 4]; n = the matcher's count (may
    exceed cap).  -> dict: ok (the function's return value), cur_map {key: point} as the frame holds it at return,
    calls [(key, point, match)] the SetMapPoint calls in order, erased [(key, point)] in map order, n_matches_map"""
    cur_map = {int(k): int(p) for k, p in zip(fmap["cur_key"], fmap["cur_point"])}     # mKeyPointMap of the current frame
    ref_map = {int(k): int(p) for k, p in zip(fmap["ref_key"], fmap["ref_point"])}
    lst = matches[:max(min(int(n), cap), 0)]
    calls = []
    if n < min_matches:                                          # if (matches.size() < mMinLocalMatchCount) return false
        return dict(ok=False, early=True, cur_map=cur_map, calls=calls, erased=[], n_matches_map=None)
    for i, (x1, y1, x2, y2) in enumerate(lst):
        k2 = pixel_key(x2, y2)
        pMP = ref_map.get(k2) if k2 is not None else None        # GetMapPoint ignores a point outside the image
        if pMP is not None:
            k1 = pixel_key(x1, y1)
            if k1 is not None:                                   # so does SetMapPoint
                cur_map[k1] = pMP
                calls.append((k1, pMP, i))
    keys = sorted(cur_map)                                       # the map iterates in key order
    outliers, _ = optimise(keys, [cur_map[k] for k in keys])     # Optimizer::PoseOptimization(&mCurrentFrame)
    erased, nmatchesMap = [], 0
    for k, bad in zip(keys, outliers):
        pMP = cur_map[k]
        if bad:                                                  # pointsToRemove -> SetMapPoint(index, nullptr); mnLastFrameSeen is the caller's
            del cur_map[k]
            erased.append((k, pMP))
        elif is_observed(fmap, pMP):                             # Observations() > 0
            nmatchesMap += 1
    return dict(ok=nmatchesMap >= min_map_matches, early=False, cur_map=cur_map, calls=calls, erased=erased,
                n_matches_map=nmatchesMap)


def carry(fmap, matches, n, cap, corr_cap, min_matches=0):
    """Steps 0-3 of the header.  -> dict: status (0, 1 gated, or negative: then nothing else), n_map, map FRAME_POINT
    [n_map], carry_status uint8 [cap] (255: not written), cur_status uint8 [n_cur], corr_p3d, corr_p2d, corr_point"""
    if map_fault(fmap):
        return dict(status=-1)
    if n < 0:
        return dict(status=-3)
    gated = n < min_matches
    lst = [] if gated else [tuple(int(v) for v in m) for m in matches[:min(int(n), cap)]]
    n_cur = len(fmap["cur_key"])
    if n_cur + len(lst) > min(corr_cap, MAX_CANDIDATES):
        return dict(status=-2)
    ref = {int(k): int(p) for k, p in zip(fmap["ref_key"], fmap["ref_point"])}
    carry_status = np.full(cap, 255, np.uint8)
    winner = {}                                                  # k1 -> the largest candidate j
    cand = {}
    for j, (x1, y1, x2, y2) in enumerate(lst):
        k1, k2 = pixel_key(x1, y1), pixel_key(x2, y2)
        if k1 is None:
            carry_status[j] = 1
        elif k2 is None or k2 not in ref:
            carry_status[j] = 3
        else:
            cand[j] = (k1, ref[k2])
            winner[k1] = max(winner.get(k1, j), j)
    for j, (k1, _) in cand.items():
        carry_status[j] = 0 if winner[k1] == j else 4
    cur_status = np.array([1 if int(k) in winner else 0 for k in fmap["cur_key"]], np.uint8)
    recs = [(int(k), int(p), -1, 0) for k, p, s in zip(fmap["cur_key"], fmap["cur_point"], cur_status) if not s]
    recs += [(k1, cand[j][1], j, 0) for k1, j in winner.items()]
    recs.sort()
    rec = np.array(recs, np.int32).reshape(-1, 4)
    return dict(status=1 if gated else 0, n_map=len(recs), map=rec, carry_status=carry_status, cur_status=cur_status,
                corr_point=rec[:, 1].copy(), corr_p2d=np.stack([rec[:, 0] % W, rec[:, 0] // W], 1).astype(np.float32),
                corr_p3d=np.asarray(fmap["points"]["pos"], np.float32)[rec[:, 1]].reshape(-1, 3))


def sorted_words(fmap, matches, n, cap):
    """The valid words of the carry in ascending order, as the sort leaves them: [(key, rank)] with rank = c for entry c
    of the frame and n_cur + j for candidate j of the list (a match with carry_status 0 or 4 in carry()'s own result).
    Non-candidates carry no word.  Index i of this list is index i of the sorted words."""
    n_cur = len(fmap["cur_key"])
    c = carry(fmap, matches, n, cap, MAX_CANDIDATES)
    assert c["status"] == 0, c["status"]
    words = [(int(k), i) for i, k in enumerate(fmap["cur_key"])]
    words += [(pixel_key(*matches[j][:2]), n_cur + j) for j in np.flatnonzero((c["carry_status"] == 0) | (c["carry_status"] == 4))]
    return sorted(words)


def runs_across(words, index):
    """does a run of equal keys of sorted_words() hold both index - 1 and index?"""
    return 0 < index < len(words) and words[index - 1][0] == words[index][0]


def order_independent(fmap, matches, n, cap, corr_cap, min_matches, min_map_matches, optimise=no_optimiser, Tcw0=None):
    """The header's statement, steps 0-6.  -> the dict of carry() plus track_status, n_kept, kept_key, kept_point,
    n_removed, removed int32 [n_removed, 2], n_matches_map, outliers bool [n_map], and what `optimise` returned beside
    its flags (a gated call: Tcw = Tcw0, n_good = -1)"""
    out = carry(fmap, matches, n, cap, corr_cap, min_matches)
    out["track_status"] = out["status"]
    if out["status"] < 0:
        return out
    rec = out["map"]
    if out["status"] == 1:
        outliers, pose = np.zeros(len(rec), bool), dict(Tcw=None if Tcw0 is None else np.asarray(Tcw0, np.float32).reshape(12), n_good=-1)
    else:
        outliers, pose = optimise([int(k) for k in rec[:, 0]], [int(p) for p in rec[:, 1]])
    outliers = np.asarray(outliers).astype(bool)
    rec[outliers, 3] |= 1
    kept = rec[~outliers]
    n_seen = sum(is_observed(fmap, int(p)) for p in kept[:, 1])
    out.update(pose)
    out.update(outliers=outliers, n_kept=len(kept), kept_key=kept[:, 0].copy(), kept_point=kept[:, 1].copy(),
               n_removed=int(outliers.sum()), removed=rec[outliers][:, :2].copy(), n_matches_map=n_seen)
    if out["status"] == 0:
        out["track_status"] = 0 if n_seen >= min_map_matches else 2
    return out


def cut_chunks(outliers, chunk=256):
    """-> [(kept, removed)] of every chunk of 256 records of the map, as the cut walks them"""
    out = np.asarray(outliers).astype(bool)
    return [(int((~out[i:i + chunk]).sum()), int(out[i:i + chunk].sum())) for i in range(0, len(out), chunk)]


def agree(lit, oi):
    """literal() and order_independent() on the same inputs: the frame's map at return, the SetMapPoint calls that
    survive, the erased records, the count and the verdict"""
    assert oi["track_status"] >= 0
    assert lit["early"] == (oi["track_status"] == 1)
    assert lit["ok"] == (oi["track_status"] == 0)
    assert lit["cur_map"] == {int(k): int(p) for k, p in zip(oi["kept_key"], oi["kept_point"])}
    assert lit["erased"] == [(int(k), int(p)) for k, p in oi["removed"]]
    if not lit["early"]:
        assert lit["n_matches_map"] == oi["n_matches_map"]
        last = {}
        for k1, p, j in lit["calls"]:
            last[k1] = (p, j)                                    # what the dict holds after the loop
        got = {int(r[0]): (int(r[1]), int(r[2])) for r in oi["map"] if r[2] >= 0}
        assert got == last
        assert sorted(j for _, _, j in lit["calls"]) == [j for j in range(len(oi["carry_status"])) if oi["carry_status"][j] in (0, 4)]
    assert (np.diff(oi["kept_key"]) > 0).all() and (np.diff(oi["map"][:, 0]) > 0).all()


# ---- scenes -------------------------------------------------------------------------------------------------------------

def scene(seed, n_points=400, n_ref=300, n_cur=150, n_matches=160):
    """Random inputs that reach every carry_status and cur_status value: of the matches some have k1 outside the image,
    some no entry at k2 (or k2 outside), some repeat an earlier k1, some hit an entry of the frame.
    -> (fmap dict as make_frame_map gives it, matches int32 [n_matches, 4])"""
    rng = np.random.default_rng(4000 + seed)
    pts = np.zeros(n_points, tr.MAP_POINT)
    pts["pos"] = rng.uniform(-4, 4, (n_points, 3)).astype(np.float32)
    keys = rng.choice(W * H, n_ref + n_cur, replace=False)
    ref_key, cur_key = np.sort(keys[:n_ref]).astype(np.int32), np.sort(keys[n_ref:]).astype(np.int32)
    fmap = dict(points=pts, ref_key=ref_key, ref_point=rng.integers(0, n_points, n_ref).astype(np.int32), cur_key=cur_key,
                cur_point=rng.integers(0, n_points, n_cur).astype(np.int32),
                observed=(rng.random(n_points) < 0.8).astype(np.uint8))
    rows, used = [], []
    for j in range(n_matches):
        c = rng.choice(5, p=[0.45, 0.1, 0.15, 0.15, 0.15])
        k1, k2 = int(rng.integers(W * H)), int(rng.choice(ref_key)) if n_ref else 0
        x1, y1, x2, y2 = k1 % W, k1 // W, k2 % W, k2 // W
        if c == 1: x1, y1 = [(-1, y1), (W, y1), (x1, -1), (x1, H)][int(rng.integers(4))]
        if c == 2:
            if rng.random() < 0.3: x2, y2 = [(W + 3, y2), (x2, -1)][int(rng.integers(2))]
            else:
                kk = int(rng.integers(W * H)); x2, y2 = kk % W, kk // W
        if c == 3 and used:
            kk = used[int(rng.integers(len(used)))]; x1, y1 = kk % W, kk // W
        if c == 4 and n_cur:
            kk = int(rng.choice(cur_key)); x1, y1 = kk % W, kk // W
        rows.append((x1, y1, x2, y2))
        if 0 <= x1 < W and 0 <= y1 < H:
            used.append(y1 * W + x1)
    return fmap, np.array(rows, np.int32).reshape(-1, 4)


def tied_case():
    """The same k1 three times in the list, k1 on an entry of the frame, k2 without an entry, the four image corners,
    end points at -1 and W.  -> (fmap, matches)"""
    key = lambda x, y: y * W + x
    pts = np.zeros(10, tr.MAP_POINT)
    pts["pos"] = np.arange(30, dtype=np.float32).reshape(10, 3)
    ref = sorted([(key(8, 8), 0), (key(24, 8), 1), (key(40, 8), 2), (key(56, 8), 3), (key(0, 0), 4), (key(W - 1, 0), 5),
                  (key(0, H - 1), 6), (key(W - 1, H - 1), 7)])
    cur = sorted([(key(100, 100), 8), (key(200, 100), 9), (key(0, 0), 8)])
    fmap = dict(points=pts, ref_key=np.array([k for k, _ in ref], np.int32), ref_point=np.array([p for _, p in ref], np.int32),
                cur_key=np.array([k for k, _ in cur], np.int32), cur_point=np.array([p for _, p in cur], np.int32),
                observed=None)
    matches = np.array([(8, 8, 8, 8), (8, 8, 24, 8), (300, 200, 56, 8), (8, 8, 40, 8),       # the same k1 three times: j = 3 wins
                        (100, 100, 8, 8),                                                     # k1 on an entry: replaced
                        (0, 0, W - 1, H - 1), (W - 1, 0, 0, H - 1), (0, H - 1, W - 1, 0), (W - 1, H - 1, 0, 0),   # the corners
                        (-1, 5, 8, 8), (W, 5, 8, 8), (5, -1, 8, 8), (5, H, 8, 8),             # no k1
                        (300, 300, 9, 8), (301, 300, -1, 8), (302, 300, W, 8), (303, 300, 8, H),   # no point at k2
                        (200, 100, 9, 9)], np.int32)                                          # k1 on an entry, no point at k2: stays
    return fmap, matches


BOUNDARY_RUNS = {1022: "emmm", 2047: "m", 3071: "em"}          # first sorted index -> the run there: e an entry, m a match
BOUNDARY_WORDS = 4100


def boundary_case():
    """BOUNDARY_WORDS valid words laid out by sorted index: runs of one everywhere (an entry or a match, drawn) but for
    BOUNDARY_RUNS -- four equal keys over the chunk edge at 1024, a run of one at the last index of the second chunk, a
    run of two over the edge at 3072.  More than 4096 words, so the sort runs on 8192.  7 matches without k1 and 9
    without a point at k2 are added and the list is shuffled with a fixed seed: rank order says nothing about key order.
    -> (fmap, matches)"""
    rng = np.random.default_rng(4096)
    n_points, n_ref = 300, 500
    pts = np.zeros(n_points, tr.MAP_POINT)
    pts["pos"] = rng.uniform(-4, 4, (n_points, 3)).astype(np.float32)
    layout, i = [], 0
    while i < BOUNDARY_WORDS:
        layout.append(BOUNDARY_RUNS.get(i, "e" if rng.random() < 0.4 else "m"))
        i += len(layout[-1])
    assert i == BOUNDARY_WORDS
    keys = rng.choice(W * H, len(layout) + n_ref + 9, replace=False)
    run_key = np.sort(keys[:len(layout)])
    ref_key = np.sort(keys[len(layout):len(layout) + n_ref]).astype(np.int32)
    no_entry = keys[len(layout) + n_ref:]                            # 9 pixels of the train frame without an entry
    cur_key = np.array([k for k, run in zip(run_key, layout) if "e" in run], np.int32)
    fmap = dict(points=pts, ref_key=ref_key, ref_point=rng.integers(0, n_points, n_ref).astype(np.int32), cur_key=cur_key,
                cur_point=rng.integers(0, n_points, len(cur_key)).astype(np.int32),
                observed=(rng.random(n_points) < 0.8).astype(np.uint8))
    rows = []
    for k, run in zip(run_key, layout):
        for _ in range(run.count("m")):
            k2 = int(rng.choice(ref_key))
            rows.append((int(k) % W, int(k) // W, k2 % W, k2 // W))
    k2 = int(ref_key[0])
    rows += [(x, y, k2 % W, k2 // W) for x, y in ((-1, 5), (W, 5), (5, -1), (5, H), (-7, -7), (W + 1, H + 1), (0, H))]
    rows += [(11 + i, 3, int(k) % W, int(k) // W) for i, k in enumerate(no_entry[:6])]
    rows += [(21, 3, -1, 0), (22, 3, W, 0), (23, 3, 0, H)]
    rows = np.array(rows, np.int32)
    return fmap, rows[rng.permutation(len(rows))]


def boundary_runs(fmap, matches):
    """Proves from sorted_words() alone that boundary_case() reaches what it was built for: the three runs lie where
    BOUNDARY_RUNS says, an entry first where it names one, and there are more than 4096 words.
    -> {first index: the ranks of the run's words in sorted order}"""
    n_cur, n = len(fmap["cur_key"]), len(matches)
    words = sorted_words(fmap, matches, n, n)
    assert 4096 < len(words) <= n_cur + n <= MAX_CANDIDATES                 # p2 = 8192: the 64 KiB block
    runs = {}
    for first, run in BOUNDARY_RUNS.items():
        last = first + len(run) - 1
        assert len(set(k for k, _ in words[first:last + 1])) == 1, first
        assert words[first - 1][0] < words[first][0] and words[last][0] < words[last + 1][0], first   # no longer than that
        ranks = [r for _, r in words[first:last + 1]]
        assert [("e" if r < n_cur else "m") for r in ranks] == list(run), first
        runs[first] = ranks
    return runs


def malformed(fmap):
    """-> [(what, fmap)]: every way the header calls a map malformed"""
    out = []
    for name in ("ref", "cur"):
        key, point = name + "_key", name + "_point"
        def changed(k, i, v, name=name):
            a = fmap[k].copy()
            a[i] = v
            return dict(fmap, **{k: a})
        out.append((name + " key negative", changed(key, 0, -1)))
        out.append((name + " key beyond the image", changed(key, len(fmap[key]) - 1, W * H)))
        out.append((name + " keys equal", changed(key, 1, fmap[key][0])))
        out.append((name + " keys decreasing", changed(key, 2, fmap[key][1] - 1)))
        out.append((name + " point negative", changed(point, 1, -1)))
        out.append((name + " point beyond the table", changed(point, len(fmap[point]) - 1, len(fmap["points"]))))
    return out
