"""The geometry calls of the C ABI (include/msf_initializer.h, msf_local_mapping.h, msf_tracking.h, msf_pnp.h, msf_pose.h,
msf_ba.h, msf_global_ba.h) as methods of a matcher handle: _Geometry is mixed into matcher._Matcher and uses its _L, _h
and _check.  Every result dict comes from results.alloc over a table of _lib and goes into its struct through
results.fill; a host form returns a results.view_* of it.

What each wrapper keeps to:
  lifetime    every array whose address goes into a call is a local of the wrapper (the ascontiguousarray results, `sets`
              of pnp_ransac, the result dict) and so stays referenced until the call has returned; a struct that is
              filled in the argument list lives as long as that list
  host sizes  a host form allocates max(n, 1) rows and its view cuts them to n on return
  out=        a caller's dict is filled and returned as it is, nothing added or removed; `stream` passes through"""
import ctypes as C

import numpy as np

from . import _lib, results
from .results import alloc, fill


def _device_lists(d_matches, d_n_out):
    """The lists of a batch in device memory, as every *_device wrapper takes them -> (n_lists, cap, device)"""
    import torch
    assert d_matches.is_cuda and d_n_out.is_cuda and d_matches.is_contiguous() and d_n_out.is_contiguous()
    assert d_matches.dtype == torch.int32 and d_n_out.dtype == torch.int32
    return d_matches.shape[0], d_matches.shape[1], d_matches.device


def _device_points(d_p3d, d_p2d, d_n):
    """The 3-D / 2-D correspondences of a batch in device memory, as pnp and pose take them -> (n_lists, cap)"""
    import torch
    assert d_p3d.is_cuda and d_p2d.is_cuda and d_n.is_cuda and d_p3d.is_contiguous() and d_p2d.is_contiguous()
    assert d_p3d.dtype == torch.float32 and d_p2d.dtype == torch.float32 and d_n.dtype == torch.int32
    L, cap = d_p3d.shape[0], d_p3d.shape[1]
    assert tuple(d_p3d.shape) == (L, cap, 3) and tuple(d_p2d.shape) == (L, cap, 2) and d_n.numel() == L
    return L, cap


def _host_points(p3d, p2d):
    """-> (p3d f32 [n, 3], p2d f32 [n, 2], n), contiguous"""
    p3 = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
    p2 = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
    assert len(p2) == len(p3)
    return p3, p2, len(p3)


class _Geometry:
    def check_hypotheses(self, model, m21, m12, matches, sigma=1.0):
        """Initializer::CheckHomography (model 0: m21 = H21, m12 = H12) / CheckFundamental (model 1: m21 = F21) for
        all RANSAC hypotheses [n_hyp, 3, 3] on the match list [n, 4] (Initializer.cc:152-245, 322-487).
        -> (best index or -1, scores f32 [n_hyp], vbMatchesInliers of the best [n])"""
        m21 = np.ascontiguousarray(m21, np.float32).reshape(-1, 9)
        m12 = None if m12 is None else np.ascontiguousarray(m12, np.float32).reshape(-1, 9)
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 4)
        scores = np.zeros(len(m21), np.float32)
        inl = np.zeros(max(len(m), 1), np.uint8)
        best = C.c_int32(-1)
        self._check(self._L.msf_check_hypotheses(self._h, model, len(m21), m21.ctypes.data,
                                                 None if m12 is None else m12.ctypes.data, len(m), m.ctypes.data,
                                                 float(sigma), scores.ctypes.data, C.byref(best), inl.ctypes.data))
        return best.value, scores, inl[:len(m)].astype(bool)

    def find_models(self, matches, sets, sigma=1.0):
        """Initializer::FindHomography + FindFundamental (Initializer.cc:152-245) with the hypotheses made on the device:
        matches int32 [n, 4], sets int32 [n_hyp, 8] (mvSets).  -> {"H": ..., "F": ...}, each a dict with m21 [n_hyp, 3, 3],
        null_vec [n_hyp, 3, 3], scores [n_hyp], best (index or -1), best_inliers bool [n], T1, T2 [3, 3], and m12 (H) or
        fn (F) [n_hyp, 3, 3]; scores / best / best_inliers are those of check_hypotheses on m21 / m12."""
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 4)
        sets = np.ascontiguousarray(sets, np.int32).reshape(-1, 8)
        n, n_hyp = len(m), len(sets)
        out = results.alloc_ransac(_lib.ransac_shapes(1, n_hyp, max(n, 1)))
        h, f = fill(_lib.RansacResult(), out["H"]), fill(_lib.RansacResult(), out["F"])
        self._check(self._L.msf_find_models(self._h, n, m.ctypes.data, n_hyp, sets.ctypes.data, float(sigma),
                                            C.byref(h), C.byref(f)))
        return {name: results.view_ransac(d, n) for name, d in out.items()}

    def find_models_device(self, d_matches, d_n_out, n_hyp=200, seed=0, sigma=1.0, stream=None):
        """The same for the lists of a batch in device memory: d_matches int32 CUDA tensor [n_lists, cap, 4] and d_n_out
        int32 [n_lists], as match_batch_device leaves them; the sets are drawn on the device from `seed`.
        -> {"sets": int32 [n_lists, n_hyp, 8], "H": ..., "F": ...} of CUDA tensors with a leading n_lists dimension
        (keys as find_models; best int32 [n_lists], best_inliers uint8 [n_lists, cap]).  Lists shorter than 8 or longer
        than 8192 get best = -1.  Asynchronous on `stream` (None = handle stream + sync)."""
        L, cap, dev = _device_lists(d_matches, d_n_out)
        out = alloc({"sets": ((L, n_hyp, 8), "int32")}, dev)
        out.update(results.alloc_ransac(_lib.ransac_shapes(L, n_hyp, cap), dev))
        batch = fill(_lib.RansacBatch(), {"sets": out["sets"]})
        fill(batch.homography, out["H"])
        fill(batch.fundamental, out["F"])
        self._check(self._L.msf_find_models_device(self._h, L, d_matches.data_ptr(), cap, d_n_out.data_ptr(), n_hyp,
                                                   int(seed), float(sigma), C.byref(batch), stream))
        return out

    @staticmethod
    def _motion_params(K, sigma, min_triangulated, min_parallax):
        prm = _lib.MotionParams(struct_size=C.sizeof(_lib.MotionParams), sigma=float(sigma),
                                min_triangulated=int(min_triangulated), min_parallax=float(min_parallax))
        prm.K[:] = [float(v) for v in np.asarray(K, np.float32).reshape(9)]
        return prm

    def reconstruct(self, model, m21, matches, inliers, K, sigma=1.0, min_triangulated=50, min_parallax=1.0):
        """Initializer::ReconstructH (model 0) / ReconstructF (model 1) (Initializer.cc:489-934) of one list: m21 [3, 3]
        the H21 / F21, matches int32 [n, 4], inliers bool [n] (vbMatchesInliers), K [3, 3].  -> dict: ok, model (-1: no
        list to reconstruct from), R21 [3, 3], t21 [3], points f32 [n, 3] (vP3D), triangulated bool [n], and the
        diagnostics n_cand, cand_R [8, 3, 3], cand_t [8, 3], cand_good [8], cand_parallax [8], winner."""
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 4)
        n = len(m)
        inl = np.ascontiguousarray(np.asarray(inliers).reshape(-1), np.uint8)
        if len(inl) != n:
            raise ValueError("one inlier flag per match")
        m21 = np.ascontiguousarray(m21, np.float32).reshape(9)
        d = alloc(_lib.list_shapes(_lib.MOTION_ARRAYS, 1, max(n, 1)))
        prm = self._motion_params(K, sigma, min_triangulated, min_parallax)
        self._check(self._L.msf_reconstruct(self._h, int(model), m21.ctypes.data, n, m.ctypes.data, inl.ctypes.data,
                                            C.byref(prm), C.byref(fill(_lib.MotionResult(), d))))
        return results.view_motion(d, n)

    def reconstruct_device(self, d_matches, d_n_out, found, K, sigma=1.0, min_triangulated=50, min_parallax=1.0,
                           stream=None):
        """The tail of Initializer::Initialize for the lists of a batch in device memory: `found` is what
        find_models_device returned for the same d_matches / d_n_out; H or F is chosen per list by RH.
        -> dict of CUDA tensors with a leading n_lists dimension (keys as reconstruct; points [n_lists, cap, 3],
        triangulated uint8 [n_lists, cap]).  Asynchronous on `stream` (None = handle stream + sync)."""
        L, cap, dev = _device_lists(d_matches, d_n_out)
        n_hyp = found["H"]["scores"].shape[1]
        batch = fill(_lib.RansacBatch(), {"sets": found["sets"]})
        for name, r in (("H", batch.homography), ("F", batch.fundamental)):
            given = {k: found[name][k] for k in ("m21", "scores", "best", "best_inliers")}
            assert all(t.shape[0] == L for t in given.values())
            fill(r, given)
        d = alloc(_lib.list_shapes(_lib.MOTION_ARRAYS, L, cap), dev)
        prm = self._motion_params(K, sigma, min_triangulated, min_parallax)
        self._check(self._L.msf_reconstruct_device(self._h, L, d_matches.data_ptr(), cap, d_n_out.data_ptr(), n_hyp,
                                                   C.byref(batch), C.byref(prm), C.byref(fill(_lib.MotionResult(), d)), stream))
        return d

    @staticmethod
    def make_views(views):
        """views: a VIEW_DTYPE array or record, or an iterable of (Rcw [3, 3], tcw [3], fx, fy, cx, cy) -> VIEW_DTYPE [n]"""
        if getattr(views, "dtype", None) == _lib.VIEW_DTYPE:
            return np.ascontiguousarray(np.asarray(views).reshape(-1))
        views = list(views)
        out = np.zeros(len(views), _lib.VIEW_DTYPE)
        for o, (R, t, fx, fy, cx, cy) in zip(out, views):
            o["Rcw"] = np.asarray(R, np.float32).reshape(9)
            o["tcw"] = np.asarray(t, np.float32).reshape(3)
            o["fx"], o["fy"], o["cx"], o["cy"] = fx, fy, cx, cy
        return out

    @staticmethod
    def _new_points_params(max_cos_parallax, chi2):
        return _lib.NewPointsParams(struct_size=C.sizeof(_lib.NewPointsParams), max_cos_parallax=float(max_cos_parallax),
                                    chi2=float(chi2))

    def new_points(self, matches, view1, view2, max_cos_parallax=1.1, chi2=5.991):
        """The loop body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:195-265) on one list: matches int32 [n, 4],
        view1 / view2 one view each (see make_views).  -> dict: n_new, packed NEW_POINT_DTYPE [n_new] (match index and
        x3D, in match order), status uint8 [n] (0 or the rejecting stage 1..7), points f32 [n, 3] (zero where rejected),
        and the diagnostics hom f32 [n, 4], cos_parallax f64 [n]."""
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 4)
        n = len(m)
        v1, v2 = self.make_views(view1), self.make_views(view2)
        d = alloc(_lib.list_shapes(_lib.NEW_POINTS_ARRAYS, 1, max(n, 1)))
        prm = self._new_points_params(max_cos_parallax, chi2)
        self._check(self._L.msf_new_points(self._h, n, m.ctypes.data, v1.ctypes.data, v2.ctypes.data, C.byref(prm),
                                           C.byref(fill(_lib.NewPointsResult(), d))))
        return results.view_new_points(d, n)

    def new_points_device(self, d_matches, d_n_out, d_view1, d_view2, max_cos_parallax=1.1, chi2=5.991, out=None,
                          stream=None):
        """The same for the lists of a batch in device memory (d_matches int32 [L, cap, 4], d_n_out int32 [L]) with the
        views as CUDA uint8 tensors [L, 64] (torch.from_numpy(make_views(...).view(np.uint8)).cuda()).  -> dict of CUDA
        tensors with a leading L: n_new int32, packed int32 [L, cap, 4] (match index, then the bits of x, y, z), status
        uint8 [L, cap], points [L, cap, 3], hom [L, cap, 4], cos_parallax f64 [L, cap].  `out`: tensors to write into
        instead of fresh zeros.  Asynchronous on `stream` (None = handle stream + sync)."""
        import torch
        L, cap, dev = _device_lists(d_matches, d_n_out)
        for v in (d_view1, d_view2):
            assert v.is_cuda and v.is_contiguous() and v.dtype == torch.uint8 and v.numel() == 64 * L
        d = alloc(_lib.list_shapes(_lib.NEW_POINTS_ARRAYS, L, cap), dev) if out is None else out
        prm = self._new_points_params(max_cos_parallax, chi2)
        self._check(self._L.msf_new_points_device(self._h, L, d_matches.data_ptr(), cap, d_n_out.data_ptr(), d_view1.data_ptr(),
                                                  d_view2.data_ptr(), C.byref(prm), C.byref(fill(_lib.NewPointsResult(), d)), stream))
        return d

    def create_map_points(self, query_slot, query_view, slots, views, cap=4096, max_cos_parallax=1.1, chi2=5.991,
                          diagnostics=False):
        """LocalMapping::CreateNewMapPoints' loop (LocalMapping.cc:161-282) in one call: the stored frame query_slot is
        matched against the stored frames `slots` and every match is triangulated from query_view and views[i].  The
        baseline / median-depth gate stays with the caller: leave the neighbours it drops out of `slots`.
        -> (num_matches [n], lists [n] of int32 [k, 4], new: list of dicts as new_points returns them; hom and
        cos_parallax only with diagnostics=True)"""
        slots = np.ascontiguousarray(np.asarray(slots, np.int32).reshape(-1))
        n = slots.size
        one = getattr(query_view, "dtype", None) == _lib.VIEW_DTYPE
        qv, nv = self.make_views(query_view if one else [query_view]), self.make_views(views)
        if len(qv) != 1 or len(nv) != n:
            raise ValueError("one query view and one view per slot")
        num = np.zeros(n, np.int32)
        lists = np.zeros((n, cap), _lib.MATCH_DTYPE)
        d = alloc(_lib.list_shapes(_lib.NEW_POINTS_ARRAYS, max(n, 1), cap),
                  leave_out=results.left_out("new_points", _lib.NEW_POINTS_ARRAYS, diagnostics))
        prm = self._new_points_params(max_cos_parallax, chi2)
        self._check(self._L.msf_create_map_points(self._h, query_slot, qv.ctypes.data, n, slots.ctypes.data,
                                                  nv.ctypes.data, C.byref(prm), num.ctypes.data, lists.ctypes.data, cap,
                                                  C.byref(fill(_lib.NewPointsResult(), d))))
        out_lists, new = [], []
        for i in range(n):
            k = min(max(int(num[i]), 0), cap)
            out_lists.append(lists[i, :k].view(np.int32).reshape(-1, 4).copy())
            new.append({key: v.copy() if isinstance(v, np.ndarray) else v
                        for key, v in results.view_new_points(d, k, i).items()})
        return num, out_lists, new

    # --- Tracking::SearchLocalPoints (include/msf_tracking.h) --------------------------------------
    _MAP_KEYS = ("points", "kf_start", "kf_key", "kf_point", "cur_key", "cur_point")

    @staticmethod
    def make_local_map(points, kf_start, kf_key, kf_point, cur_key=(), cur_point=()):
        """-> the local map of one call as a dict of contiguous numpy arrays: points MAP_POINT_DTYPE [n_points],
        kf_start int32 [n_kf + 1] (empty: no key frame), kf_key / kf_point int32 [n_entries], cur_key / cur_point
        int32 [n_cur]"""
        i32 = lambda a: np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))
        return dict(points=np.ascontiguousarray(np.asarray(points, _lib.MAP_POINT_DTYPE).reshape(-1)),
                    kf_start=i32(kf_start), kf_key=i32(kf_key), kf_point=i32(kf_point), cur_key=i32(cur_key),
                    cur_point=i32(cur_point))

    @classmethod
    def local_map_to_device(cls, lmap, device="cuda"):
        """a make_local_map dict -> the same with CUDA tensors (points as uint8 [n_points, 32])"""
        import torch
        out = {}
        for k in cls._MAP_KEYS:
            a = lmap[k].view(np.uint8).reshape(-1, 32) if k == "points" else lmap[k]
            out[k] = torch.from_numpy(a.copy()).to(device)
        return out

    @classmethod
    def _local_map(cls, lmap):
        """-> (msf_local_map over the dict's numpy arrays or CUDA tensors, n_points, n_kf)"""
        ptr = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
        count = lambda a: a.size if isinstance(a, np.ndarray) else a.numel()
        pts = lmap["points"]
        n_points = pts.size if isinstance(pts, np.ndarray) else pts.numel() // 32
        n_kf = max(count(lmap["kf_start"]) - 1, 0)
        n_entries, n_cur = count(lmap["kf_key"]), count(lmap["cur_key"])
        assert count(lmap["kf_point"]) == n_entries and count(lmap["cur_point"]) == n_cur
        m = _lib.LocalMap(struct_size=C.sizeof(_lib.LocalMap), n_points=n_points, n_kf=n_kf, n_entries=n_entries,
                          n_cur=n_cur, **{k: ptr(lmap[k]) for k in cls._MAP_KEYS})
        return m, n_points, n_kf

    @classmethod
    def _frustum_params(cls, view, Ow, bounds, viewing_cos_limit):
        v = cls.make_views(view if getattr(view, "dtype", None) == _lib.VIEW_DTYPE else [view])
        prm = _lib.FrustumParams(struct_size=C.sizeof(_lib.FrustumParams), viewing_cos_limit=viewing_cos_limit)
        C.memmove(C.byref(prm.view), v.ctypes.data, 64)
        prm.Ow[:] = [float(x) for x in np.asarray(Ow, np.float32).reshape(3)]
        prm.min_x, prm.max_x, prm.min_y, prm.max_y = [float(b) for b in bounds]
        return prm

    @staticmethod
    def _tracking_arrays(table, n_points, n_kf, cap=1, corr_cap=0, device=None, leave_out=()):
        """claims is one flat list of the call: [n_kf * cap] records (int32 [n_kf * cap, 4] on the device)"""
        return alloc(_lib.tracking_shapes(table, n_points, n_kf, cap, corr_cap), device, leave_out, flat=("claims",))

    def frustum(self, lmap, view, Ow, bounds, viewing_cos_limit=0.5):
        """Steps 1-2 of Tracking::SearchLocalPoints on a make_local_map dict: per point the owner key frame and
        Frame::isInFrustum (Frame.cc:48-84) from the current frame's `view`, camera centre Ow and bounds = (mnMinX,
        mnMaxX, mnMinY, mnMaxY).  -> dict of msf_frustum_result's arrays (status_word as an int)."""
        m, n_points, n_kf = self._local_map(lmap)
        d = self._tracking_arrays(_lib.FRUSTUM_ARRAYS, n_points, n_kf)
        prm = self._frustum_params(view, Ow, bounds, viewing_cos_limit)
        self._check(self._L.msf_frustum(self._h, C.byref(m), C.byref(prm), C.byref(fill(_lib.FrustumResult(), d))))
        return results.view_frustum(d)

    def frustum_device(self, d_lmap, view, Ow, bounds, viewing_cos_limit=0.5, out=None, stream=None):
        """The same on a local_map_to_device dict.  -> dict of CUDA tensors named and shaped as msf_frustum_result says;
        `out`: tensors to write into instead of fresh zeros.  Asynchronous on `stream` (None = handle stream + sync)."""
        m, n_points, n_kf = self._local_map(d_lmap)
        d = out if out is not None else self._tracking_arrays(_lib.FRUSTUM_ARRAYS, n_points, n_kf, device=d_lmap["points"].device)
        prm = self._frustum_params(view, Ow, bounds, viewing_cos_limit)
        self._check(self._L.msf_frustum_device(self._h, C.byref(m), C.byref(prm), C.byref(fill(_lib.FrustumResult(), d)), stream))
        return d

    def claim_points_device(self, d_lmap, d_matches, d_n_out, d_matched, corr_cap, out=None, stream=None):
        """Steps 4-5 on lists in device memory: d_matches int32 [n_kf, cap, 4], d_n_out int32 [n_kf], d_matched uint8
        [n_kf] (the gate).  -> dict of CUDA tensors named as msf_claim_result says: claims int32 [n_kf * cap, 4] (key,
        point, kf, match; the first n_claims), claim_status uint8 [n_kf, cap], corr_* [corr_cap, ...].  `out`: tensors
        to write into instead of fresh zeros."""
        import torch
        m, n_points, n_kf = self._local_map(d_lmap)
        cap = d_matches.shape[1]
        assert d_matches.is_cuda and d_matches.is_contiguous() and d_matches.dtype == torch.int32
        assert tuple(d_matches.shape) == (n_kf, cap, 4) and d_n_out.numel() == n_kf and d_matched.numel() == n_kf
        assert d_n_out.dtype == torch.int32 and d_matched.dtype == torch.uint8
        dev = d_lmap["points"].device
        d = out if out is not None else self._tracking_arrays(_lib.CLAIM_ARRAYS, n_points, n_kf, cap, corr_cap, dev)
        self._check(self._L.msf_claim_points_device(self._h, C.byref(m), d_matches.data_ptr(), cap, d_n_out.data_ptr(),
                                                    d_matched.data_ptr(), corr_cap, C.byref(fill(_lib.ClaimResult(), d)), stream))
        return d

    def search_local_points(self, query_slot, slots, lmap, view, Ow, bounds, viewing_cos_limit=0.5, cap=4096,
                            keep_on_device=False, want_lists=True):
        """Tracking::SearchLocalPoints' loop (Tracking.cc:594-632) in one call: the stored frame query_slot against the
        stored frames `slots`, one per key frame of the make_local_map dict `lmap`.  -> dict: num_matches [n_kf]
        (-1 for a key frame the gate left out), lists (or None), frustum (as frustum() returns it), n_claims,
        n_claimed [n_kf], claims LOCAL_CLAIM_DTYPE [n_claims], claim_status [n_kf, cap], and the correspondences
        n_corr, corr_p3d, corr_p2d, corr_point -- or with keep_on_device `keep`: (d_corr_p3d, d_corr_p2d, d_corr_point,
        d_n_corr, corr_cap) as device addresses inside the handle's workspace, valid until the next call of this
        family."""
        slots = np.ascontiguousarray(np.asarray(slots, np.int32).reshape(-1))
        m, n_points, n_kf = self._local_map(lmap)
        if slots.size != n_kf:
            raise ValueError("one slot per key frame")
        corr_cap = m.n_cur + n_kf * cap
        num = np.zeros(n_kf, np.int32)
        lists = np.zeros((n_kf, cap), _lib.MATCH_DTYPE) if want_lists else None
        fd = self._tracking_arrays(_lib.FRUSTUM_ARRAYS, n_points, n_kf)
        cd = self._tracking_arrays(_lib.CLAIM_ARRAYS, n_points, n_kf, cap, corr_cap,
                                   leave_out=results.left_out("search", _lib.CLAIM_ARRAYS, not keep_on_device))
        fres, cres = fill(_lib.FrustumResult(), fd), fill(_lib.ClaimResult(), cd)
        keep = _lib.DeviceCorr(struct_size=C.sizeof(_lib.DeviceCorr))
        prm = self._frustum_params(view, Ow, bounds, viewing_cos_limit)
        self._check(self._L.msf_search_local_points(
            self._h, query_slot, slots.ctypes.data, C.byref(m), C.byref(prm),
            _lib.MSF_SEARCH_KEEP_ON_DEVICE if keep_on_device else 0, num.ctypes.data,
            lists.ctypes.data if want_lists else None, cap, C.byref(fres), C.byref(cres),
            C.byref(keep) if keep_on_device else None))
        n_claims, n_corr = int(cd["n_claims"][0]), int(cd["n_corr"][0])
        out = dict(num_matches=num, lists=None, frustum=results.view_frustum(fd), n_claims=n_claims,
                   n_claimed=cd["n_claimed"], claims=cd["claims"][:n_claims], claim_status=cd["claim_status"], n_corr=n_corr)
        if want_lists:
            out["lists"] = [lists[i, :min(max(int(num[i]), 0), cap)].view(np.int32).reshape(-1, 4).copy() for i in range(n_kf)]
        if keep_on_device:
            out["keep"] = (keep.d_corr_p3d, keep.d_corr_p2d, keep.d_corr_point, keep.d_n_corr, keep.corr_cap)
        else:
            k = max(n_corr, 0)
            out.update(corr_p3d=cd["corr_p3d"][:k], corr_p2d=cd["corr_p2d"][:k], corr_point=cd["corr_point"][:k])
        return out

    _FRAME_MAP_KEYS = ("points", "ref_key", "ref_point", "cur_key", "cur_point")

    @staticmethod
    def make_frame_map(points, ref_key, ref_point, cur_key=(), cur_point=(), observed=None):
        """-> the inputs of one frame-tracking call (msfx_frame_map) as a dict of contiguous numpy arrays: points
        MAP_POINT_DTYPE [n_points], ref_key / ref_point int32 [n_ref] (the train frame's mKeyPointMap), cur_key /
        cur_point int32 [n_cur] (the current frame's own map at entry), observed uint8 [n_points] or None"""
        i32 = lambda a: np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))
        pts = np.ascontiguousarray(np.asarray(points, _lib.MAP_POINT_DTYPE).reshape(-1))
        obs = None if observed is None else np.ascontiguousarray(np.asarray(observed, np.uint8).reshape(pts.size))
        return dict(points=pts, ref_key=i32(ref_key), ref_point=i32(ref_point), cur_key=i32(cur_key),
                    cur_point=i32(cur_point), observed=obs)

    @classmethod
    def frame_map_to_device(cls, fmap, device="cuda"):
        """a make_frame_map dict -> the same with CUDA tensors (points as uint8 [n_points, 32])"""
        import torch
        out = {"observed": None if fmap["observed"] is None else torch.from_numpy(fmap["observed"].copy()).to(device)}
        for k in cls._FRAME_MAP_KEYS:
            a = fmap[k].view(np.uint8).reshape(-1, 32) if k == "points" else fmap[k]
            out[k] = torch.from_numpy(a.copy()).to(device)
        return out

    @classmethod
    def _frame_map(cls, fmap):
        """-> msfx_frame_map over the dict's numpy arrays or CUDA tensors"""
        ptr = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()
        count = lambda a: a.size if isinstance(a, np.ndarray) else a.numel()
        pts = fmap["points"]
        n_points = pts.size if isinstance(pts, np.ndarray) else pts.numel() // 32
        n_ref, n_cur = count(fmap["ref_key"]), count(fmap["cur_key"])
        assert count(fmap["ref_point"]) == n_ref and count(fmap["cur_point"]) == n_cur
        obs = fmap.get("observed")
        assert obs is None or count(obs) == n_points
        return _lib.FrameMap(struct_size=C.sizeof(_lib.FrameMap), n_points=n_points, n_ref=n_ref, n_cur=n_cur,
                             observed=None if obs is None else ptr(obs), **{k: ptr(fmap[k]) for k in cls._FRAME_MAP_KEYS})

    @classmethod
    def _track_params(cls, K, Tcw0, chi2, min_matches, min_map_matches):
        prm = _lib.TrackParams(struct_size=C.sizeof(_lib.TrackParams), pose=cls._pose_params(K, chi2),
                               min_matches=min_matches, min_map_matches=min_map_matches)
        prm.Tcw0[:] = [float(v) for v in np.asarray(Tcw0, np.float32).reshape(12)]
        return prm

    @staticmethod
    def _device_list(d_matches, d_n_out):
        """One list in device memory: d_matches int32 [cap, 4], d_n_out int32 [1] -> cap"""
        import torch
        assert d_matches.is_cuda and d_n_out.is_cuda and d_matches.is_contiguous() and d_n_out.numel() == 1
        assert d_matches.dtype == torch.int32 and d_n_out.dtype == torch.int32 and d_matches.shape[1:] == (4,)
        return d_matches.shape[0]

    def carry_points_device(self, d_fmap, d_matches, d_n_out, corr_cap, out=None, stream=None):
        """The carry of TrackWithMotionModel / TrackReferenceKeyFrame (Tracking.cc:448-459) on one list in device memory:
        d_fmap a frame_map_to_device dict, d_matches int32 [cap, 4], d_n_out int32 [1].  -> dict of CUDA tensors named as
        msfx_track_result says, up to corr_point: track_status [1] (0, -1 malformed map, -2 no room, -3 no list), n_map
        [1], map int32 [corr_cap, 4] (key, point, match, flags; ascending key), carry_status uint8 [cap], cur_status
        uint8 [n_cur], corr_* [corr_cap, ...].  `out`: tensors to write into instead of fresh zeros."""
        cap = self._device_list(d_matches, d_n_out)
        m = self._frame_map(d_fmap)
        d = out
        if d is None:
            shapes = _lib.track_shapes(cap, m.n_cur, corr_cap)
            d = alloc(shapes, d_matches.device, leave_out=set(shapes) - set(_lib.CARRY_NAMES))
        self._check(self._L.msfx_carry_points_device(self._h, C.byref(m), d_matches.data_ptr(), cap, d_n_out.data_ptr(),
                                                     corr_cap, C.byref(fill(_lib.TrackResult(), d)), stream))
        return d

    def track_list_device(self, d_fmap, d_matches, d_n_out, corr_cap, K, Tcw0, chi2=5.991, min_matches=15,
                          min_map_matches=10, out=None, pose_out=None, diagnostics=False, stream=None):
        """The body of TrackWithMotionModel / TrackReferenceKeyFrame behind the match (Tracking.cc:448-484) on one list
        in device memory: carry, PoseOptimization from Tcw0, cut.  -> (dict of CUDA tensors named and shaped as
        msfx_track_result says, dict of msf_pose_result's tensors for the one list with cap = corr_cap).  track_status
        [1]: 0 tracked, 1 fewer than min_matches matches, 2 fewer than min_map_matches kept observed points, negative
        as carry_points_device.  Three launches, asynchronous on `stream` (None = handle stream + sync)."""
        cap = self._device_list(d_matches, d_n_out)
        m = self._frame_map(d_fmap)
        dev = d_matches.device
        d = out if out is not None else alloc(_lib.track_shapes(cap, m.n_cur, corr_cap), dev)
        pd = pose_out if pose_out is not None else self._pose_arrays(1, max(corr_cap, 1), diagnostics, dev)
        prm = self._track_params(K, Tcw0, chi2, min_matches, min_map_matches)
        self._check(self._L.msfx_track_list_device(self._h, C.byref(m), d_matches.data_ptr(), cap, d_n_out.data_ptr(),
                                                   corr_cap, C.byref(prm), C.byref(fill(_lib.TrackResult(), d)),
                                                   C.byref(fill(_lib.PoseResult(), pd)), stream))
        return d, pd

    def track_frame(self, query_slot, train_slot, fmap, K, Tcw0, chi2=5.991, min_matches=15, min_map_matches=10,
                    cap=4096, keep_on_device=False, want_list=True, diagnostics=False):
        """TrackWithMotionModel / TrackReferenceKeyFrame in one call: the stored frame query_slot against the stored
        frame train_slot, fmap a make_frame_map dict.  -> dict: num_matches, list int32 [n, 4] (or None), capacity (True:
        the list overflowed, as match_one_to_many reports it), track_status, n_map, map FRAME_POINT_DTYPE [n_map],
        carry_status, cur_status, corr_p3d / corr_p2d / corr_point [n_map], Tcw [12], n_good, n_kept, kept_key / kept_point
        [n_kept] (the cur_key / cur_point of the local map that goes on to search_local_points), n_removed, removed
        REMOVED_POINT_DTYPE [n_removed], n_matches_map, pose (as pose_optimize returns it) -- and with keep_on_device
        `keep`: the device addresses of msfx_device_track by name, valid until the next call of this family."""
        m = self._frame_map(fmap)
        corr_cap = m.n_cur + cap
        num = np.zeros(1, np.int32)
        lst = np.zeros(cap, _lib.MATCH_DTYPE) if want_list else None
        d = alloc(_lib.track_shapes(cap, m.n_cur, corr_cap))
        pd = self._pose_arrays(1, corr_cap, diagnostics)
        keep = _lib.DeviceTrack(struct_size=C.sizeof(_lib.DeviceTrack))
        prm = self._track_params(K, Tcw0, chi2, min_matches, min_map_matches)
        rc = self._L.msfx_track_frame(self._h, query_slot, train_slot, C.byref(m), C.byref(prm),
                                      _lib.MSFX_TRACK_KEEP_ON_DEVICE if keep_on_device else 0, num.ctypes.data,
                                      lst.ctypes.data if want_list else None, cap, C.byref(fill(_lib.TrackResult(), d)),
                                      C.byref(fill(_lib.PoseResult(), pd)), C.byref(keep) if keep_on_device else None)
        if rc != _lib.MSF_ERR_CAPACITY:
            self._check(rc)
        n = min(max(int(num[0]), 0), cap)
        out = results.view_track(d, n)
        out.update(num_matches=int(num[0]), capacity=rc == _lib.MSF_ERR_CAPACITY, list=None,
                   pose=results.view_pose(pd, max(out["n_map"], 0) if out["track_status"] in (0, 2) else 0))
        if want_list:
            out["list"] = lst[:n].view(np.int32).reshape(-1, 4).copy()
        if keep_on_device:
            out["keep"] = {name: getattr(keep, name) for name, _ in _lib.DeviceTrack._fields_[1:]}
        return out

    @staticmethod
    def _pnp_params(K, th2, min_inliers, n_iterations, max_records, seed):
        fx, fy, cx, cy = K
        return _lib.PnpParams(struct_size=C.sizeof(_lib.PnpParams), fx=fx, fy=fy, cx=cx, cy=cy, th2=th2,
                              min_inliers=min_inliers, n_iterations=n_iterations, max_records=max_records, seed=seed)

    def pnp_ransac(self, p3d, p2d, K, min_inliers, n_iterations, th2=5.991, max_records=8, seed=0, sets=None):
        """PnPsolver's RANSAC iterations [0, n_iterations) and Refine on one list (PnPsolver.cc:172-331): p3d f32 [n, 3]
        (mvP3Dw), p2d f32 [n, 2] (mvP2D), K = (fx, fy, cx, cy), min_inliers = mRansacMinInliers after
        SetRansacParameters' adjustment, sets int32 [n_iterations, 4] or None to draw them from `seed`.
        -> dict: n_records (the true number; -1: fewer than 4 correspondences), capacity (True: more records than
        max_records, the first max_records are complete), counts [n_iterations], the per-record arrays cut to the
        records kept (iteration, n_inliers, refined_ok, n_refined, Tcw_best [., 12], Tcw_refined, inliers_best [., n],
        inliers_refined, rec_*), and the per-hypothesis diagnostics sets, pose_f64, cws, ut_tail, betas, rep_errors, pca."""
        p3, p2, n = _host_points(p3d, p2d)
        d = alloc(_lib.pnp_shapes(1, n_iterations, max_records, max(n, 1)))
        s = None
        if sets is not None:   # the call reads `s`; the result gets a copy, as if the sets had been drawn
            s = np.ascontiguousarray(sets, np.int32).reshape(n_iterations, 4)
            d["sets"][0] = s
        prm = self._pnp_params(K, th2, min_inliers, n_iterations, max_records, seed)
        rc = self._L.msf_pnp_ransac(self._h, n, p3.ctypes.data, p2.ctypes.data, C.byref(prm),
                                    s.ctypes.data if s is not None else None, C.byref(fill(_lib.PnpResult(), d)))
        if rc != _lib.MSF_ERR_CAPACITY:   # more records than max_records is a result, not a failure
            self._check(rc)
        v = results.view_pnp(d, _lib.PNP_ARRAYS, n, max_records)
        return dict(n_records=v.pop("n_records"), capacity=rc == _lib.MSF_ERR_CAPACITY, **v)

    def pnp_ransac_device(self, d_p3d, d_p2d, d_n, K, min_inliers, n_iterations, th2=5.991, max_records=8, seed=0,
                          d_sets=None, out=None, diagnostics=True, stream=None):
        """The same for a batch in device memory: d_p3d f32 [L, cap, 3], d_p2d f32 [L, cap, 2], d_n int32 [L] (negative:
        no valid list), d_sets int32 [L, n_iterations, 4] or None.  -> dict of CUDA tensors with a leading L, named and
        shaped as msf_pnp_result says (per-record arrays [L, max_records, ...], inlier rows [.., cap]); without
        `diagnostics` only n_records, counts and the per-record results.  `out`: tensors to write into instead of fresh
        zeros.  Two launches, asynchronous on `stream` (None = handle stream + sync)."""
        import torch
        L, cap = _device_points(d_p3d, d_p2d, d_n)
        d = out
        if d is None:
            d = alloc(_lib.pnp_shapes(L, n_iterations, max_records, cap), d_p3d.device,
                      results.left_out("pnp", _lib.PNP_ARRAYS, diagnostics))
        if d_sets is not None:
            assert d_sets.is_cuda and d_sets.is_contiguous() and d_sets.dtype == torch.int32
            assert d_sets.numel() == L * n_iterations * 4
        prm = self._pnp_params(K, th2, min_inliers, n_iterations, max_records, seed)
        self._check(self._L.msf_pnp_ransac_device(self._h, L, d_p3d.data_ptr(), d_p2d.data_ptr(), cap, d_n.data_ptr(),
                                                  C.byref(prm), d_sets.data_ptr() if d_sets is not None else None,
                                                  C.byref(fill(_lib.PnpResult(), d)), stream))
        return d

    @staticmethod
    def _pose_params(K, chi2):
        fx, fy, cx, cy = K
        return _lib.PoseParams(struct_size=C.sizeof(_lib.PoseParams), fx=fx, fy=fy, cx=cx, cy=cy, chi2=chi2)

    @staticmethod
    def _pose_arrays(lists, cap, diagnostics, device=None):
        return alloc(_lib.pose_shapes(lists, cap), device, results.left_out("pose", _lib.POSE_ARRAYS, diagnostics))

    def pose_optimize(self, p3d, p2d, K, Tcw0, mask=None, chi2=5.991, diagnostics=True):
        """Optimizer::PoseOptimization on one list (Optimizer.cc:217-334): p3d f32 [n, 3] (GetWorldPos()), p2d f32 [n, 2]
        (the key points' pixels), K = (fx, fy, cx, cy), Tcw0 f32 [12] or [3, 4] (rows 0..2 of mTcw), mask uint8 [n] or
        None (non-zero: the correspondence is an edge).  -> dict: n_good, n_edges, rounds_run (ints), Tcw f32 [12],
        pose_f64 [12], outliers uint8 [n] (0 outside the mask), and with `diagnostics` the per-round arrays [4, ...]
        and per-iteration arrays [4, 10, ...] of msf_pose_result."""
        p3, p2, n = _host_points(p3d, p2d)
        t0 = np.ascontiguousarray(Tcw0, np.float32).reshape(12)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(n)
        d = self._pose_arrays(1, max(n, 1), diagnostics)
        prm = self._pose_params(K, chi2)
        self._check(self._L.msf_pose_optimize(self._h, n, p3.ctypes.data, p2.ctypes.data, t0.ctypes.data,
                                              m.ctypes.data if m is not None else None, C.byref(prm),
                                              C.byref(fill(_lib.PoseResult(), d))))
        return results.view_pose(d, n)

    def pose_optimize_device(self, d_p3d, d_p2d, d_n, K, d_Tcw0, d_mask=None, chi2=5.991, Tcw0_stride=12,
                             mask_stride=None, out=None, diagnostics=True, stream=None):
        """The same for a batch in device memory: d_p3d f32 [L, cap, 3], d_p2d f32 [L, cap, 2], d_n int32 [L] (negative:
        no valid list), d_Tcw0 f32 with list l's 12 floats at element l * Tcw0_stride, d_mask uint8 with list l's bytes
        at l * mask_stride (default cap) or None: a view into Tcw_refined / inliers_refined of pnp_ransac_device's result
        can be passed with its strides.  -> dict of CUDA tensors with a leading L, named and shaped as msf_pose_result
        says; without `diagnostics` only the per-list arrays.  `out`: tensors to write into instead of fresh zeros.
        One launch, asynchronous on `stream` (None = handle stream + sync)."""
        import torch
        L, cap = _device_points(d_p3d, d_p2d, d_n)
        # the strided inputs must lie inside their storage: list L - 1 ends at (L - 1) * stride + its length
        assert d_Tcw0.is_cuda and d_Tcw0.dtype == torch.float32 and Tcw0_stride >= 0
        assert L == 0 or d_Tcw0.untyped_storage().nbytes() // 4 - d_Tcw0.storage_offset() >= (L - 1) * Tcw0_stride + 12
        if d_mask is not None:   # mask_stride defaults to cap only with a mask; without one the call gets 0
            mask_stride = cap if mask_stride is None else mask_stride
            assert d_mask.is_cuda and d_mask.dtype == torch.uint8 and mask_stride >= 0
            assert L == 0 or d_mask.untyped_storage().nbytes() - d_mask.storage_offset() >= (L - 1) * mask_stride + cap
        d = self._pose_arrays(L, cap, diagnostics, d_p3d.device) if out is None else out
        prm = self._pose_params(K, chi2)
        self._check(self._L.msf_pose_optimize_device(self._h, L, d_p3d.data_ptr(), d_p2d.data_ptr(), cap, d_n.data_ptr(),
                                                     d_Tcw0.data_ptr(), Tcw0_stride,
                                                     d_mask.data_ptr() if d_mask is not None else None,
                                                     mask_stride or 0, C.byref(prm), C.byref(fill(_lib.PoseResult(), d)), stream))
        return d

    @staticmethod
    def _ba_params(K, schedule, huber_delta2, chi2):
        fx, fy, cx, cy = K
        n_rounds, its, robust = schedule
        p = _lib.BaParams(struct_size=C.sizeof(_lib.BaParams), fx=fx, fy=fy, cx=cx, cy=cy, n_rounds=n_rounds,
                          huber_delta2=huber_delta2, chi2=chi2)
        p.iterations[0], p.iterations[1] = its
        p.robust[0], p.robust[1] = robust
        return p

    @staticmethod
    def _ba_arrays(problems, cams, points, edges, diagnostics, device=None):
        return alloc(_lib.ba_shapes(problems, cams, points, edges), device, results.left_out("ba", _lib.BA_ARRAYS, diagnostics))

    def _ba_host(self, symbol, st, cam_Tcw, cam_fixed, points, edge_cam, edge_point, edge_obs, K, schedule, huber_delta2,
                 chi2, diagnostics):
        """bundle_adjust / global_bundle_adjust through `symbol` of the library; st: None or the int32 array of one
        element whose address is the call's stop flag"""
        given = ((cam_Tcw, np.float32, 12), (cam_fixed, np.uint8, 1), (points, np.float32, 3), (edge_cam, np.int32, 1),
                 (edge_point, np.int32, 1), (edge_obs, np.float32, 2))
        tcw, fixed, pts, ec, ep, obs = [np.ascontiguousarray(a, dt).reshape((-1, w) if w > 1 else -1) for a, dt, w in given]
        nc, npt, ne = len(tcw), len(pts), len(ec)
        assert len(fixed) == nc and len(ep) == ne and len(obs) == ne
        d = self._ba_arrays(1, nc, npt, ne, diagnostics)
        prm = self._ba_params(K, schedule, huber_delta2, chi2)
        self._check(symbol(self._h, nc, tcw.ctypes.data, fixed.ctypes.data, npt, pts.ctypes.data, ne, ec.ctypes.data,
                           ep.ctypes.data, obs.ctypes.data, st.ctypes.data if st is not None else None, C.byref(prm),
                           C.byref(fill(_lib.BaResult(), d))))
        return results.view_ba(d, _lib.BA_ARRAYS, _lib.BA_SLOTS, nc, npt)

    def _ba_device(self, call, problems, d_problems, d_cam_Tcw, d_cam_fixed, d_points, d_edge_cam, d_edge_point, d_edge_obs,
                   K, schedule, d_stop, huber_delta2, chi2, out, diagnostics):
        """bundle_adjust_device / global_bundle_adjust_device: the checks of the inputs, the result arrays, then
        call(cams, points, edges, stop address or None, params, result) -> status"""
        import torch
        given = ((d_cam_Tcw, torch.float32), (d_cam_fixed, torch.uint8), (d_points, torch.float32),
                 (d_edge_cam, torch.int32), (d_edge_point, torch.int32), (d_edge_obs, torch.float32))
        for t, dt in given + (((d_problems, torch.int32),) if d_problems is not None else ()):
            assert t.is_cuda and t.is_contiguous() and t.dtype == dt
        cams, points, edges = d_cam_fixed.numel(), d_points.numel() // 3, d_edge_cam.numel()
        assert d_cam_Tcw.numel() == cams * 12 and d_edge_point.numel() == edges and d_edge_obs.numel() == edges * 2
        if d_stop is not None:
            assert d_stop.is_cuda and d_stop.dtype == torch.int32 and d_stop.numel() == 1
        d = self._ba_arrays(problems, cams, points, edges, diagnostics, d_points.device) if out is None else out
        prm = self._ba_params(K, schedule, huber_delta2, chi2)
        self._check(call(cams, points, edges, d_stop.data_ptr() if d_stop is not None else None, C.byref(prm),
                         C.byref(fill(_lib.BaResult(), d))))
        return d

    def bundle_adjust(self, cam_Tcw, cam_fixed, points, edge_cam, edge_point, edge_obs, K, schedule=(2, (5, 10), (1, 0)),
                      stop=None, huber_delta2=5.991, chi2=5.991, diagnostics=True):
        """Optimizer::LocalBundleAdjustment (Optimizer.cc:336-574; the default schedule) or BundleAdjustment (:71-215;
        schedule = (1, (nIterations, 0), (bRobust, 0))) on one problem: cam_Tcw f32 [n_cams, 12] (rows 0..2 of Tcw),
        cam_fixed uint8 [n_cams], points f32 [n_points, 3], edge_cam / edge_point int32 [n_edges] sorted by point,
        edge_obs f32 [n_edges, 2], K = (fx, fy, cx, cy), schedule = (n_rounds, (iterations, iterations), (robust,
        robust)), stop None or an int (pbStopFlag as the call starts).  -> dict: status (the rounds run), cam_Tcw f32
        [n_cams, 12], points f32 [n_points, 3], outliers uint8 [n_edges], cam_pose_f64, points_f64, round_flags
        [n_edges, 2], round_iterations [2] and with `diagnostics` the per-iteration arrays of msf_ba_result as [64] /
        [64, n_cams, ...] / [64, n_points, ...].  More than 64 free cameras: MsfError with code MSF_ERR_CAPACITY."""
        return self._ba_host(self._L.msf_bundle_adjust, None if stop is None else np.array([stop], np.int32), cam_Tcw,
                             cam_fixed, points, edge_cam, edge_point, edge_obs, K, schedule, huber_delta2, chi2, diagnostics)

    def bundle_adjust_device(self, d_problems, d_cam_Tcw, d_cam_fixed, d_points, d_edge_cam, d_edge_point, d_edge_obs, K,
                             schedule=(2, (5, 10), (1, 0)), max_free_cams=64, d_stop=None, huber_delta2=5.991, chi2=5.991,
                             out=None, diagnostics=True, stream=None):
        """The same for a batch in device memory: d_problems int32 [P, 6] (n_cams, n_points, n_edges, cam0, point0,
        edge0; n_cams < 0: no valid problem), the camera, point and edge arrays concatenated (edge indices local to
        their problem), d_stop None or an int32 tensor of one element.  -> dict of CUDA tensors named and shaped as
        _lib.ba_shapes(P, cams, points, edges) says; without `diagnostics` no per-iteration arrays.  `out`: tensors to
        write into instead of fresh zeros.  One launch, asynchronous on `stream` (None = handle stream + sync)."""
        P = d_problems.numel() // 6
        call = lambda cams, points, edges, stop, prm, res: self._L.msf_bundle_adjust_device(
            self._h, P, d_problems.data_ptr(), d_cam_Tcw.data_ptr(), d_cam_fixed.data_ptr(), d_points.data_ptr(),
            d_edge_cam.data_ptr(), d_edge_point.data_ptr(), d_edge_obs.data_ptr(), cams, points, edges, max_free_cams, stop,
            prm, res, stream)
        return self._ba_device(call, P, d_problems, d_cam_Tcw, d_cam_fixed, d_points, d_edge_cam, d_edge_point, d_edge_obs,
                               K, schedule, d_stop, huber_delta2, chi2, out, diagnostics)

    def global_bundle_adjust(self, cam_Tcw, cam_fixed, points, edge_cam, edge_point, edge_obs, K, schedule=(1, (10, 0), (0, 0)),
                             stop=None, huber_delta2=5.991, chi2=5.991, diagnostics=True):
        """Optimizer::GlobalBundleAdjustemnt (Optimizer.cc:62-69; the default schedule is the reference's call) on one
        problem of up to 1024 free cameras, spread over the whole device: arguments and the returned dict as
        bundle_adjust, bit for bit the same result wherever bundle_adjust takes the problem.  stop: None, an int, or an
        int32 numpy array of one element that another thread may set while the call runs.  More than 1024 free cameras:
        MsfError with code MSF_ERR_CAPACITY."""
        if isinstance(stop, np.ndarray):   # the caller's own buffer, never a copy: another thread writes it meanwhile
            assert stop.dtype == np.int32 and stop.size == 1
            st = stop
        else:
            st = None if stop is None else np.array([stop], np.int32)
        return self._ba_host(self._L.msf_global_bundle_adjust, st, cam_Tcw, cam_fixed, points, edge_cam, edge_point, edge_obs,
                             K, schedule, huber_delta2, chi2, diagnostics)

    def global_bundle_adjust_device(self, d_cam_Tcw, d_cam_fixed, d_points, d_edge_cam, d_edge_point, d_edge_obs, K,
                                    schedule=(1, (10, 0), (0, 0)), max_free_cams=_lib.GBA_MAX_FREE_CAMS, d_stop=None,
                                    huber_delta2=5.991, chi2=5.991, out=None, diagnostics=True, stream=None):
        """The same with the problem in device memory (tensors as one problem of bundle_adjust_device, d_stop None or
        an int32 tensor of one element).  -> dict of CUDA tensors named and shaped as _lib.ba_shapes(1, cams, points,
        edges) says; without `diagnostics` no per-iteration arrays.  `out`: tensors to write into instead of fresh
        zeros.  Enqueued on `stream`, but the host decides every trial: the call returns when the problem is finished."""
        call = lambda cams, points, edges, stop, prm, res: self._L.msf_global_bundle_adjust_device(
            self._h, cams, d_cam_Tcw.data_ptr(), d_cam_fixed.data_ptr(), points, d_points.data_ptr(), edges,
            d_edge_cam.data_ptr(), d_edge_point.data_ptr(), d_edge_obs.data_ptr(), max_free_cams, stop, prm, res, stream)
        return self._ba_device(call, 1, None, d_cam_Tcw, d_cam_fixed, d_points, d_edge_cam, d_edge_point, d_edge_obs, K,
                               schedule, d_stop, huber_delta2, chi2, out, diagnostics)
