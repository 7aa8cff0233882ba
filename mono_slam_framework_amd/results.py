"""The layout of a result dict of the geometry calls, said once: from a table of _lib (rows (name, dtype, per, tail) in
the result struct's declaration order) to shapes, to zero arrays on the host or a device, to the struct's pointers, and
to what a host wrapper returns of a one-list call.  Pure Python over the tables it is given: no libmsf.so, and torch
only where a device is named."""
import ctypes as C

import numpy as np


def shapes(table, lead, cap=None):
    """-> {name: (shape, dtype)} in table order: lead[per] + the tail, with "cap" in a tail the lists' stride `cap`"""
    return {name: (lead[per] + tuple(cap if t == "cap" else t for t in tail), dt) for name, dt, per, tail in table}


# what a call without diagnostics -- "search": with keep_on_device -- leaves out, as a predicate over (name, per)
_LEFT_OUT = {"new_points": lambda name, per: name in ("hom", "cos_parallax"),
             "pnp": lambda name, per: name.startswith("rec_") or (per == "hyp" and name != "counts"),
             "pose": lambda name, per: per != "list",
             "ba": lambda name, per: per.startswith("it"),
             "search": lambda name, per: per == "corr"}


def left_out(family, table, whole=False):
    """-> the names of `table` that a call of `family` does not ask for; none of a call that wants the `whole` result"""
    return set() if whole else {name for name, _, per, _ in table if _LEFT_OUT[family](name, per)}


def alloc(shapes, device=None, leave_out=(), init=None, flat=()):
    """-> {name: zeros} in the order of `shapes` without `leave_out`: numpy arrays, or torch tensors on `device` (any
    device; only fill insists on CUDA).  An array with a structured dtype (NEW_POINT_DTYPE, LOCAL_CLAIM_DTYPE: records of
    4-byte fields) is that dtype on the host and int32 [..., itemsize / 4] on a device.  A name in `flat` loses its
    shape ([n_kf, cap] -> [n_kf * cap]: claims); init = {name: first value} where that is not 0 (best: -1)."""
    if device is not None:
        import torch
    out = {}
    for name, (shape, dt) in shapes.items():
        if name in leave_out:
            continue
        if name in flat:
            shape = (int(np.prod(shape)),)
        if device is None:
            out[name] = np.zeros(shape, dt)
        elif np.dtype(dt).fields:
            out[name] = torch.zeros(shape + (np.dtype(dt).itemsize // 4,), dtype=torch.int32, device=device)
        else:
            out[name] = torch.zeros(shape, dtype=getattr(torch, dt), device=device)
        if init and name in init:
            out[name][...] = init[name]
    return out


def alloc_ransac(shapes, device=None):
    """-> {"H": ..., "F": ...}: msf_ransac_result's zero arrays per model, best = -1; H has no fn and F no m12, and the
    model's own of the two comes last"""
    out = {}
    for name, own, other in (("H", "m12", "fn"), ("F", "fn", "m12")):
        out[name] = d = alloc(shapes, device, leave_out=(other,), init={"best": -1})
        d[own] = d.pop(own)
    return out


def fill(res, arrays):
    """Points the result struct `res` at `arrays` (field name -> numpy array or contiguous CUDA tensor) and sets its
    struct_size; a field without an array stays NULL.  -> res.  The struct holds addresses only: the caller keeps
    `arrays` until the call that reads `res` has returned."""
    res.struct_size = C.sizeof(type(res))
    for k, v in arrays.items():
        if isinstance(v, np.ndarray):
            setattr(res, k, v.ctypes.data)
        else:
            assert v.is_cuda and v.is_contiguous()
            setattr(res, k, v.data_ptr())
    return res


def host_view(d, i=0, ints=(), cut=None, bools=()):
    """What a host wrapper returns of list `i` of the arrays `d`: element i of the leading dimension, `ints` as int,
    cut[name] = n (or one n per dimension) rows of it, `bools` as bool.  Names that `d` lacks are passed over."""
    out = {k: v[i] for k, v in d.items()}
    for k in ints:
        out[k] = int(out[k])
    for k, n in (cut or {}).items():
        if k in out:
            out[k] = out[k][tuple(slice(0, c) for c in (n if isinstance(n, tuple) else (n,)))]
    for k in bools:
        out[k] = out[k].astype(bool)
    return out


def view_ransac(d, n):
    return host_view(d, ints=("best",), cut={"best_inliers": n}, bools=("best_inliers",))


def view_motion(d, n):
    return host_view(d, ints=("ok", "model", "n_cand", "winner"), cut={"points": n, "triangulated": n},
                     bools=("triangulated",))


def view_new_points(d, n, i=0):
    """list i of msf_new_points_result: packed cut to n_new, the per-match arrays to the list's n matches"""
    cut = {k: n for k in ("status", "points", "hom", "cos_parallax")}
    return host_view(d, i, ints=("n_new",), cut=dict(cut, packed=max(int(d["n_new"][i]), 0)))


def view_pnp(d, table, n, max_records):
    """n_records is the true number: the per-record arrays are cut to those kept, their inlier rows to [:, :n]"""
    kept = min(max(int(d["n_records"][0]), 0), max_records)
    cut = {name: (kept, n) if name.startswith("inliers_") else kept for name, _, per, _ in table if per == "rec"}
    return host_view(d, ints=("n_records",), cut=cut)


def view_pose(d, n):
    return host_view(d, ints=("n_good", "n_edges", "rounds_run"), cut={"outliers": n})


def view_frustum(d):
    """msf_frustum_result on the host: the arrays as they are, status_word as an int; -> d"""
    d["status_word"] = int(d["status_word"][0])
    return d


def view_track(d, n_list):
    """msfx_track_result on the host: the counts and the status as ints, every array cut to its count (carry_status to
    the list's n_list matches); a negative track_status leaves the counts at 0 and the arrays empty"""
    ints = ("track_status", "n_map", "n_good", "n_kept", "n_removed", "n_matches_map")
    out = host_view({k: v for k, v in d.items() if k in ints or k == "Tcw"}, ints=ints)
    ok = out["track_status"] >= 0
    n_map, n_kept, n_removed = (out[k] if ok else 0 for k in ("n_map", "n_kept", "n_removed"))
    cuts = dict(map=n_map, corr_p3d=n_map, corr_p2d=n_map, corr_point=n_map, kept_key=n_kept, kept_point=n_kept,
                removed=n_removed, carry_status=n_list if out["track_status"] in (0, 2) else 0, cur_status=None if ok else 0)
    out.update({k: d[k][:n] for k, n in cuts.items() if k in d})
    return out


def view_ba(d, table, slots, nc, npt):
    """One problem of msf_ba_result on the host: status as an int, round_iterations [2], the per-iteration arrays as
    [slots] / [slots, n_cams, ...] / [slots, n_points, ...]; everything else as it is."""
    out = dict(d)
    out["status"] = int(d["status"][0])
    out["round_iterations"] = d["round_iterations"][0]
    for name, _, per, _ in table:
        if name in d and per == "it":
            out[name] = d[name][0]
        elif name in d and per in ("it_cam", "it_point"):
            out[name] = d[name].reshape((slots, nc if per == "it_cam" else npt) + d[name].shape[1:])
    return out
