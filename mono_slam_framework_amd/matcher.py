"""Host-side mirror of the reference's matcher classes over the C ABI (include/msf_abi.h).

  FeatureMatcher     <- ::FeatureMatcher     (src/featurematcher.h:7-22,   src/featurematcher.cpp:3-47)
  DNNFeatureMatcher  <- ::DNNFeatureMatcher  (src/dnnfeaturematcher.h:9-36, src/dnnfeaturematcher.cpp:11-103)

Same names and argument meaning (threshold, SetThreshold, MatchFrames(frame1, frame2)); a frame is the
8-bit single-channel image the reference reads from FrameBase::imGray (slam_pipeline/include/FrameBase.h:45).
MatchFrames returns an int32 [m, 4] array: columns 0:2 are MatchFramesResult::keyPoints1, 2:4 keyPoints2
(slam_pipeline/include/FeatureMatcher.h:15-19).  The C++ twin for linking into slam_pipeline is
csrc/hip_feature_matcher.h.  All compute happens in libmsf.so on the GPU; there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib


class MsfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("msf error %d: %s" % (code, msg))
        self.code = code


def _fill(res, arrays):
    """Points the result struct `res` at `arrays` (field name -> numpy array or contiguous CUDA tensor) and sets its
    struct_size.  -> res"""
    res.struct_size = C.sizeof(type(res))
    for k, v in arrays.items():
        if isinstance(v, np.ndarray):
            setattr(res, k, v.ctypes.data)
        else:
            assert v.is_cuda and v.is_contiguous()
            setattr(res, k, v.data_ptr())
    return res


def _device_lists(d_matches, d_n_out):
    """The lists of a batch in device memory, as every *_device wrapper takes them -> (n_lists, cap, device)"""
    import torch
    assert d_matches.is_cuda and d_n_out.is_cuda and d_matches.is_contiguous() and d_n_out.is_contiguous()
    assert d_matches.dtype == torch.int32 and d_n_out.dtype == torch.int32
    return d_matches.shape[0], d_matches.shape[1], d_matches.device


def _zeros_on(dev):
    """-> z(shape, dtype="float32"): a tensor of zeros on `dev`"""
    import torch
    return lambda shape, dtype="float32": torch.zeros(shape, dtype=getattr(torch, dtype), device=dev)


class _Matcher:
    _kind = None

    def __init__(self, threshold, image_width, image_height, device=0, max_batch_pairs=1, flags=0,
                 weights_path=None):
        self._L = _lib.load()
        self._h = C.c_void_p()
        cfg = _lib.Config()
        self._L.msf_default_config(C.byref(cfg), self._kind)
        cfg.threshold = threshold
        cfg.device = device
        cfg.image_width = image_width
        cfg.image_height = image_height
        cfg.max_batch_pairs = max_batch_pairs
        cfg.flags = flags
        self._wpath = weights_path.encode() if weights_path else None
        cfg.weights_path = self._wpath
        rc = self._L.msf_create(C.byref(cfg), C.byref(self._h))
        if rc != _lib.MSF_OK:
            msg = self._L.msf_last_error(None).decode()
            self._h = C.c_void_p()
            raise MsfError(rc, msg)
        self.width, self.height = image_width, image_height
        self.max_batch_pairs = max_batch_pairs
        self.device = device
        self.threshold = threshold

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._L.msf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != _lib.MSF_OK:
            raise MsfError(rc, self._L.msf_last_error(self._h).decode())

    # --- reference API -------------------------------------------------------------------------
    def SetThreshold(self, value):
        self._check(self._L.msf_set_threshold(self._h, float(value)))
        self.threshold = float(value)

    @staticmethod
    def _image(arr):
        if arr.dtype != np.uint8 or arr.ndim != 2 or arr.strides[1] != 1:
            raise ValueError("frames must be 2-D uint8 with unit column stride (CV_8UC1)")
        return _lib.Image(arr.ctypes.data, arr.shape[1], arr.shape[0], arr.strides[0])

    def MatchFrames(self, frame1, frame2, cap=4096):
        a, b = self._image(frame1), self._image(frame2)
        out = np.zeros((cap,), _lib.MATCH_DTYPE)
        n = C.c_int32(0)
        self._check(self._L.msf_match_pair(self._h, C.byref(a), C.byref(b), out.ctypes.data, cap, C.byref(n)))
        m = min(n.value, cap)
        return out[:m].view(np.int32).reshape(m, 4).copy()

    def frame_cache_stats(self):
        """(hits, misses, capacity) of the transparent per-frame cache behind MatchFrames (a miss = one extraction)."""
        hits, miss, cap = C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        self._check(self._L.msf_frame_cache_stats(self._h, C.byref(hits), C.byref(miss), C.byref(cap)))
        return hits.value, miss.value, cap.value

    # --- batched forms -------------------------------------------------------------------------
    def match_batch(self, frames1, frames2, cap=4096):
        n = len(frames1)
        A = (_lib.Image * n)(*[self._image(f) for f in frames1])
        B = (_lib.Image * n)(*[self._image(f) for f in frames2])
        out = np.zeros((n, cap), _lib.MATCH_DTYPE)
        cnt = np.zeros((n,), np.int32)
        self._check(self._L.msf_match_batch(self._h, n, A, B, out.ctypes.data, cap, cnt.ctypes.data))
        return [out[i, :min(cnt[i], cap)].view(np.int32).reshape(-1, 4).copy() for i in range(n)]

    def match_batch_raw(self, frames1, frames2, cap=4096):
        """match_batch that tolerates MSF_ERR_CAPACITY: returns (n_out int32 [n] with -1 for a pair without a valid result,
        lists).  Any other error raises."""
        n = len(frames1)
        A = (_lib.Image * n)(*[self._image(f) for f in frames1])
        B = (_lib.Image * n)(*[self._image(f) for f in frames2])
        out = np.zeros((n, cap), _lib.MATCH_DTYPE)
        cnt = np.zeros((n,), np.int32)
        rc = self._L.msf_match_batch(self._h, n, A, B, out.ctypes.data, cap, cnt.ctypes.data)
        if rc not in (_lib.MSF_OK, _lib.MSF_ERR_CAPACITY):
            self._check(rc)
        return cnt, [out[i, :min(max(cnt[i], 0), cap)].view(np.int32).reshape(-1, 4).copy() for i in range(n)]

    def match_batch_device(self, d_a, d_b, d_out, d_n_out, stream=None):
        """d_a/d_b: torch uint8 CUDA tensors [n, H, W(pitch)] resident in HBM; d_out int32 [n, cap, 4];
        d_n_out int32 [n].  Asynchronous on `stream` (an int hipStream_t; None = handle stream + sync)."""
        n = d_a.shape[0]
        assert d_a.is_cuda and d_b.is_cuda and d_out.is_cuda and d_n_out.is_cuda
        assert d_a.stride(2) == 1 and d_b.stride() == d_a.stride()
        cap = d_out.shape[1]
        self._check(self._L.msf_match_batch_device(
            self._h, n, d_a.data_ptr(), d_b.data_ptr(), d_a.stride(0), d_a.stride(1),
            d_out.data_ptr(), cap, d_n_out.data_ptr(), stream))

    def extract_device(self, d_frames, first_slot=0, stream=None):
        """Per-frame part once (ORB features / LoFTR backbone tokens) into slots first_slot.. of the handle."""
        self._check(self._L.msf_extract_device(self._h, d_frames.shape[0], d_frames.data_ptr(), d_frames.stride(0),
                                               d_frames.stride(1), first_slot, stream))

    def match_slots_device(self, d_slot_a, d_slot_b, d_out, d_n_out, stream=None):
        """Pairs of slots (int32 CUDA tensors) -> match lists, as match_batch_device."""
        self._check(self._L.msf_match_slots_device(self._h, d_slot_a.shape[0], d_slot_a.data_ptr(),
                                                   d_slot_b.data_ptr(), d_out.data_ptr(), d_out.shape[1],
                                                   d_n_out.data_ptr(), stream))

    def pack_matches_device(self, d_out, d_n_out, d_packed, d_offsets, stream=None):
        """[n, cap, 4] + counts -> contiguous [total, 4] prefix of d_packed, offsets int32 [n + 1]."""
        self._check(self._L.msf_pack_matches_device(self._h, d_out.shape[0], d_out.data_ptr(), d_out.shape[1],
                                                    d_n_out.data_ptr(), d_packed.data_ptr(), d_offsets.data_ptr(),
                                                    stream))

    def set_mappoints(self, map_slot, keys):
        """KeyPointMap occupancy of one frame: `keys` = pixel keys y*cols + x that hold a map point."""
        keys = np.ascontiguousarray(np.asarray(keys, np.int32).reshape(-1))
        self._check(self._L.msf_set_mappoints(self._h, map_slot, keys.ctypes.data, keys.size))

    def count_mappoint_matches_device(self, d_out, d_n_out, d_map_a, d_map_b, d_num_mp, stream=None):
        """d_num_mp[i] = matches of pair i with a map point at both endpoints (KeyFrameDatabase.cc:37-44)."""
        self._check(self._L.msf_count_mappoint_matches_device(
            self._h, d_out.shape[0], d_out.data_ptr(), d_out.shape[1], d_n_out.data_ptr(), d_map_a.data_ptr(),
            d_map_b.data_ptr(), d_num_mp.data_ptr(), stream))

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
        out, res = {}, []
        for name in ("H", "F"):
            d = dict(m21=np.zeros((n_hyp, 3, 3), np.float32), null_vec=np.zeros((n_hyp, 3, 3), np.float32),
                     scores=np.zeros(n_hyp, np.float32), best=np.full(1, -1, np.int32),
                     best_inliers=np.zeros(max(n, 1), np.uint8), T1=np.zeros((3, 3), np.float32),
                     T2=np.zeros((3, 3), np.float32))
            d["m12" if name == "H" else "fn"] = np.zeros((n_hyp, 3, 3), np.float32)
            out[name] = d
            res.append(_fill(_lib.RansacResult(), d))
        self._check(self._L.msf_find_models(self._h, n, m.ctypes.data, n_hyp, sets.ctypes.data, float(sigma),
                                            C.byref(res[0]), C.byref(res[1])))
        for d in out.values():
            d["best"] = int(d["best"][0])
            d["best_inliers"] = d["best_inliers"][:n].astype(bool)
        return out

    def find_models_device(self, d_matches, d_n_out, n_hyp=200, seed=0, sigma=1.0, stream=None):
        """The same for the lists of a batch in device memory: d_matches int32 CUDA tensor [n_lists, cap, 4] and d_n_out
        int32 [n_lists], as match_batch_device leaves them; the sets are drawn on the device from `seed`.
        -> {"sets": int32 [n_lists, n_hyp, 8], "H": ..., "F": ...} of CUDA tensors with a leading n_lists dimension
        (keys as find_models; best int32 [n_lists], best_inliers uint8 [n_lists, cap]).  Lists shorter than 8 or longer
        than 8192 get best = -1.  Asynchronous on `stream` (None = handle stream + sync)."""
        import torch
        L, cap, dev = _device_lists(d_matches, d_n_out)
        z = _zeros_on(dev)
        out = {"sets": z((L, n_hyp, 8), "int32")}
        batch = _fill(_lib.RansacBatch(), {"sets": out["sets"]})
        for name, r in (("H", batch.homography), ("F", batch.fundamental)):
            d = dict(m21=z((L, n_hyp, 3, 3)), null_vec=z((L, n_hyp, 3, 3)), scores=z((L, n_hyp)),
                     best=torch.full((L,), -1, dtype=torch.int32, device=dev), best_inliers=z((L, cap), "uint8"),
                     T1=z((L, 3, 3)), T2=z((L, 3, 3)))
            d["m12" if name == "H" else "fn"] = z((L, n_hyp, 3, 3))
            _fill(r, d)
            out[name] = d
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
        d = dict(ok=np.zeros(1, np.int32), model=np.zeros(1, np.int32), R21=np.zeros((3, 3), np.float32),
                 t21=np.zeros(3, np.float32), points=np.zeros((max(n, 1), 3), np.float32),
                 triangulated=np.zeros(max(n, 1), np.uint8), n_cand=np.zeros(1, np.int32),
                 cand_R=np.zeros((8, 3, 3), np.float32), cand_t=np.zeros((8, 3), np.float32),
                 cand_good=np.zeros(8, np.int32), cand_parallax=np.zeros(8, np.float32), winner=np.zeros(1, np.int32))
        res = _fill(_lib.MotionResult(), d)
        prm = self._motion_params(K, sigma, min_triangulated, min_parallax)
        self._check(self._L.msf_reconstruct(self._h, int(model), m21.ctypes.data, n, m.ctypes.data, inl.ctypes.data,
                                            C.byref(prm), C.byref(res)))
        for k in ("ok", "model", "n_cand", "winner"):
            d[k] = int(d[k][0])
        d["points"] = d["points"][:n]
        d["triangulated"] = d["triangulated"][:n].astype(bool)
        return d

    def reconstruct_device(self, d_matches, d_n_out, found, K, sigma=1.0, min_triangulated=50, min_parallax=1.0,
                           stream=None):
        """The tail of Initializer::Initialize for the lists of a batch in device memory: `found` is what
        find_models_device returned for the same d_matches / d_n_out; H or F is chosen per list by RH.
        -> dict of CUDA tensors with a leading n_lists dimension (keys as reconstruct; points [n_lists, cap, 3],
        triangulated uint8 [n_lists, cap]).  Asynchronous on `stream` (None = handle stream + sync)."""
        L, cap, dev = _device_lists(d_matches, d_n_out)
        n_hyp = found["H"]["scores"].shape[1]
        batch = _fill(_lib.RansacBatch(), {"sets": found["sets"]})
        for name, r in (("H", batch.homography), ("F", batch.fundamental)):
            given = {k: found[name][k] for k in ("m21", "scores", "best", "best_inliers")}
            assert all(t.shape[0] == L for t in given.values())
            _fill(r, given)
        z, i32 = _zeros_on(dev), "int32"
        d = dict(ok=z((L,), i32), model=z((L,), i32), R21=z((L, 3, 3)), t21=z((L, 3)), points=z((L, cap, 3)),
                 triangulated=z((L, cap), "uint8"), n_cand=z((L,), i32), cand_R=z((L, 8, 3, 3)), cand_t=z((L, 8, 3)),
                 cand_good=z((L, 8), i32), cand_parallax=z((L, 8)), winner=z((L,), i32))
        res = _fill(_lib.MotionResult(), d)
        prm = self._motion_params(K, sigma, min_triangulated, min_parallax)
        self._check(self._L.msf_reconstruct_device(self._h, L, d_matches.data_ptr(), cap, d_n_out.data_ptr(), n_hyp,
                                                   C.byref(batch), C.byref(prm), C.byref(res), stream))
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

    @staticmethod
    def _new_points_arrays(lists, cap):
        return dict(n_new=np.zeros(lists, np.int32), packed=np.zeros((lists, cap), _lib.NEW_POINT_DTYPE),
                    status=np.zeros((lists, cap), np.uint8), points=np.zeros((lists, cap, 3), np.float32),
                    hom=np.zeros((lists, cap, 4), np.float32), cos_parallax=np.zeros((lists, cap), np.float64))

    def new_points(self, matches, view1, view2, max_cos_parallax=1.1, chi2=5.991):
        """The loop body of LocalMapping::CreateNewMapPoints (LocalMapping.cc:195-265) on one list: matches int32 [n, 4],
        view1 / view2 one view each (see make_views).  -> dict: n_new, packed NEW_POINT_DTYPE [n_new] (match index and
        x3D, in match order), status uint8 [n] (0 or the rejecting stage 1..7), points f32 [n, 3] (zero where rejected),
        and the diagnostics hom f32 [n, 4], cos_parallax f64 [n]."""
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 4)
        n = len(m)
        v1, v2 = self.make_views(view1), self.make_views(view2)
        d = self._new_points_arrays(1, max(n, 1))
        res = _fill(_lib.NewPointsResult(), d)
        prm = self._new_points_params(max_cos_parallax, chi2)
        self._check(self._L.msf_new_points(self._h, n, m.ctypes.data, v1.ctypes.data, v2.ctypes.data, C.byref(prm),
                                           C.byref(res)))
        n_new = int(d["n_new"][0])
        return dict(n_new=n_new, packed=d["packed"][0, :max(n_new, 0)], status=d["status"][0, :n], points=d["points"][0, :n],
                    hom=d["hom"][0, :n], cos_parallax=d["cos_parallax"][0, :n])

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
        d = out
        if d is None:
            z = _zeros_on(dev)
            d = dict(n_new=z((L,), "int32"), packed=z((L, cap, 4), "int32"), status=z((L, cap), "uint8"),
                     points=z((L, cap, 3)), hom=z((L, cap, 4)), cos_parallax=z((L, cap), "float64"))
        res = _fill(_lib.NewPointsResult(), d)
        prm = self._new_points_params(max_cos_parallax, chi2)
        self._check(self._L.msf_new_points_device(self._h, L, d_matches.data_ptr(), cap, d_n_out.data_ptr(),
                                                  d_view1.data_ptr(), d_view2.data_ptr(), C.byref(prm), C.byref(res), stream))
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
        d = self._new_points_arrays(max(n, 1), cap)
        if not diagnostics:
            del d["hom"], d["cos_parallax"]
        res = _fill(_lib.NewPointsResult(), d)
        prm = self._new_points_params(max_cos_parallax, chi2)
        self._check(self._L.msf_create_map_points(self._h, query_slot, qv.ctypes.data, n, slots.ctypes.data,
                                                  nv.ctypes.data, C.byref(prm), num.ctypes.data, lists.ctypes.data, cap,
                                                  C.byref(res)))
        out_lists, new = [], []
        for i in range(n):
            k = min(max(int(num[i]), 0), cap)
            out_lists.append(lists[i, :k].view(np.int32).reshape(-1, 4).copy())
            n_new = int(d["n_new"][i])
            e = dict(n_new=n_new, packed=d["packed"][i, :max(n_new, 0)].copy(), status=d["status"][i, :k].copy(),
                     points=d["points"][i, :k].copy())
            if diagnostics:
                e.update(hom=d["hom"][i, :k].copy(), cos_parallax=d["cos_parallax"][i, :k].copy())
            new.append(e)
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

    @staticmethod
    def local_map_to_device(lmap, device="cuda"):
        """a make_local_map dict -> the same with CUDA tensors (points as uint8 [n_points, 32])"""
        import torch
        out = {}
        for k in _Matcher._MAP_KEYS:
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

    def frustum(self, lmap, view, Ow, bounds, viewing_cos_limit=0.5):
        """Steps 1-2 of Tracking::SearchLocalPoints on a make_local_map dict: per point the owner key frame and
        Frame::isInFrustum (Frame.cc:48-84) from the current frame's `view`, camera centre Ow and bounds = (mnMinX,
        mnMaxX, mnMinY, mnMaxY).  -> dict of msf_frustum_result's arrays (status_word as an int)."""
        m, n_points, n_kf = self._local_map(lmap)
        d = {k: np.zeros(shape, dt) for k, (shape, dt) in _lib.tracking_shapes(_lib.FRUSTUM_ARRAYS, n_points, n_kf, 1, 0).items()}
        res = _fill(_lib.FrustumResult(), d)
        prm = self._frustum_params(view, Ow, bounds, viewing_cos_limit)
        self._check(self._L.msf_frustum(self._h, C.byref(m), C.byref(prm), C.byref(res)))
        d["status_word"] = int(d["status_word"][0])
        return d

    def frustum_device(self, d_lmap, view, Ow, bounds, viewing_cos_limit=0.5, out=None, stream=None):
        """The same on a local_map_to_device dict.  -> dict of CUDA tensors named and shaped as msf_frustum_result says;
        `out`: tensors to write into instead of fresh zeros.  Asynchronous on `stream` (None = handle stream + sync)."""
        m, n_points, n_kf = self._local_map(d_lmap)
        d = out
        if d is None:
            z = _zeros_on(d_lmap["points"].device)
            d = {k: z(shape, dt) for k, (shape, dt) in _lib.tracking_shapes(_lib.FRUSTUM_ARRAYS, n_points, n_kf, 1, 0).items()}
        res = _fill(_lib.FrustumResult(), d)
        prm = self._frustum_params(view, Ow, bounds, viewing_cos_limit)
        self._check(self._L.msf_frustum_device(self._h, C.byref(m), C.byref(prm), C.byref(res), stream))
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
        d = out
        if d is None:
            z = _zeros_on(d_lmap["points"].device)
            d = {}
            for k, (shape, dt) in _lib.tracking_shapes(_lib.CLAIM_ARRAYS, n_points, n_kf, cap, corr_cap).items():
                d[k] = z((n_kf * cap, 4), "int32") if k == "claims" else z(shape, dt)
        res = _fill(_lib.ClaimResult(), d)
        self._check(self._L.msf_claim_points_device(self._h, C.byref(m), d_matches.data_ptr(), cap, d_n_out.data_ptr(),
                                                    d_matched.data_ptr(), corr_cap, C.byref(res), stream))
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
        fd = {k: np.zeros(shape, dt) for k, (shape, dt) in _lib.tracking_shapes(_lib.FRUSTUM_ARRAYS, n_points, n_kf, 1, 0).items()}
        cd = {k: np.zeros(shape, dt) for k, (shape, dt) in _lib.tracking_shapes(_lib.CLAIM_ARRAYS, n_points, n_kf, cap, corr_cap).items()}
        cd["claims"] = np.zeros(n_kf * cap, _lib.LOCAL_CLAIM_DTYPE)
        if keep_on_device:
            for k in ("corr_p3d", "corr_p2d", "corr_point"):
                del cd[k]
        fres, cres = _fill(_lib.FrustumResult(), fd), _fill(_lib.ClaimResult(), cd)
        prm = self._frustum_params(view, Ow, bounds, viewing_cos_limit)
        keep = _lib.DeviceCorr(struct_size=C.sizeof(_lib.DeviceCorr))
        self._check(self._L.msf_search_local_points(
            self._h, query_slot, slots.ctypes.data, C.byref(m), C.byref(prm),
            _lib.MSF_SEARCH_KEEP_ON_DEVICE if keep_on_device else 0, num.ctypes.data,
            lists.ctypes.data if want_lists else None, cap, C.byref(fres), C.byref(cres),
            C.byref(keep) if keep_on_device else None))
        fd["status_word"] = int(fd["status_word"][0])
        n_claims, n_corr = int(cd["n_claims"][0]), int(cd["n_corr"][0])
        out = dict(num_matches=num, lists=None, frustum=fd, n_claims=n_claims, n_claimed=cd["n_claimed"],
                   claims=cd["claims"][:n_claims], claim_status=cd["claim_status"], n_corr=n_corr)
        if want_lists:
            out["lists"] = [lists[i, :min(max(int(num[i]), 0), cap)].view(np.int32).reshape(-1, 4).copy() for i in range(n_kf)]
        if keep_on_device:
            out["keep"] = (keep.d_corr_p3d, keep.d_corr_p2d, keep.d_corr_point, keep.d_n_corr, keep.corr_cap)
        else:
            k = max(n_corr, 0)
            out.update(corr_p3d=cd["corr_p3d"][:k], corr_p2d=cd["corr_p2d"][:k], corr_point=cd["corr_point"][:k])
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
        p3 = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
        p2 = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
        n = len(p3)
        assert len(p2) == n
        shapes = _lib.pnp_shapes(1, n_iterations, max_records, max(n, 1))
        d = {k: np.zeros(shape, dt) for k, (shape, dt) in shapes.items()}
        s = None
        if sets is not None:
            s = np.ascontiguousarray(sets, np.int32).reshape(n_iterations, 4)
            d["sets"][0] = s
        res = _fill(_lib.PnpResult(), d)
        prm = self._pnp_params(K, th2, min_inliers, n_iterations, max_records, seed)
        rc = self._L.msf_pnp_ransac(self._h, n, p3.ctypes.data, p2.ctypes.data, C.byref(prm),
                                    s.ctypes.data if s is not None else None, C.byref(res))
        if rc != _lib.MSF_ERR_CAPACITY:
            self._check(rc)
        records = int(d["n_records"][0])
        kept = min(max(records, 0), max_records)
        out = dict(n_records=records, capacity=rc == _lib.MSF_ERR_CAPACITY)
        for name, _, per, _ in _lib.PNP_ARRAYS[1:]:
            out[name] = d[name][0, :kept] if per == "rec" else d[name][0]
        out["inliers_best"], out["inliers_refined"] = out["inliers_best"][:, :n], out["inliers_refined"][:, :n]
        return out

    def pnp_ransac_device(self, d_p3d, d_p2d, d_n, K, min_inliers, n_iterations, th2=5.991, max_records=8, seed=0,
                          d_sets=None, out=None, diagnostics=True, stream=None):
        """The same for a batch in device memory: d_p3d f32 [L, cap, 3], d_p2d f32 [L, cap, 2], d_n int32 [L] (negative:
        no valid list), d_sets int32 [L, n_iterations, 4] or None.  -> dict of CUDA tensors with a leading L, named and
        shaped as msf_pnp_result says (per-record arrays [L, max_records, ...], inlier rows [.., cap]); without
        `diagnostics` only n_records, counts and the per-record results.  `out`: tensors to write into instead of fresh
        zeros.  Two launches, asynchronous on `stream` (None = handle stream + sync)."""
        import torch
        assert d_p3d.is_cuda and d_p2d.is_cuda and d_n.is_cuda and d_p3d.is_contiguous() and d_p2d.is_contiguous()
        assert d_p3d.dtype == torch.float32 and d_p2d.dtype == torch.float32 and d_n.dtype == torch.int32
        L, cap = d_p3d.shape[0], d_p3d.shape[1]
        assert tuple(d_p3d.shape) == (L, cap, 3) and tuple(d_p2d.shape) == (L, cap, 2) and d_n.numel() == L
        d = out
        if d is None:
            z = _zeros_on(d_p3d.device)
            d = {k: z(shape, dt) for k, (shape, dt) in _lib.pnp_shapes(L, n_iterations, max_records, cap).items()}
            if not diagnostics:
                for name, _, per, _ in _lib.PNP_ARRAYS:
                    if name.startswith("rec_") or (per == "hyp" and name != "counts"):
                        del d[name]
        if d_sets is not None:
            assert d_sets.is_cuda and d_sets.is_contiguous() and d_sets.dtype == torch.int32
            assert d_sets.numel() == L * n_iterations * 4
        res = _fill(_lib.PnpResult(), d)
        prm = self._pnp_params(K, th2, min_inliers, n_iterations, max_records, seed)
        self._check(self._L.msf_pnp_ransac_device(self._h, L, d_p3d.data_ptr(), d_p2d.data_ptr(), cap, d_n.data_ptr(),
                                                  C.byref(prm), d_sets.data_ptr() if d_sets is not None else None,
                                                  C.byref(res), stream))
        return d

    @staticmethod
    def _pose_params(K, chi2):
        fx, fy, cx, cy = K
        return _lib.PoseParams(struct_size=C.sizeof(_lib.PoseParams), fx=fx, fy=fy, cx=cx, cy=cy, chi2=chi2)

    def pose_optimize(self, p3d, p2d, K, Tcw0, mask=None, chi2=5.991, diagnostics=True):
        """Optimizer::PoseOptimization on one list (Optimizer.cc:217-334): p3d f32 [n, 3] (GetWorldPos()), p2d f32 [n, 2]
        (the key points' pixels), K = (fx, fy, cx, cy), Tcw0 f32 [12] or [3, 4] (rows 0..2 of mTcw), mask uint8 [n] or
        None (non-zero: the correspondence is an edge).  -> dict: n_good, n_edges, rounds_run (ints), Tcw f32 [12],
        pose_f64 [12], outliers uint8 [n] (0 outside the mask), and with `diagnostics` the per-round arrays [4, ...]
        and per-iteration arrays [4, 10, ...] of msf_pose_result."""
        p3 = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
        p2 = np.ascontiguousarray(p2d, np.float32).reshape(-1, 2)
        t0 = np.ascontiguousarray(Tcw0, np.float32).reshape(12)
        n = len(p3)
        assert len(p2) == n
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8).reshape(n)
        d = {k: np.zeros(shape, dt) for k, (shape, dt) in _lib.pose_shapes(1, max(n, 1)).items()}
        if not diagnostics:
            for name, _, per, _ in _lib.POSE_ARRAYS:
                if per != "list":
                    del d[name]
        res = _fill(_lib.PoseResult(), d)
        prm = self._pose_params(K, chi2)
        self._check(self._L.msf_pose_optimize(self._h, n, p3.ctypes.data, p2.ctypes.data, t0.ctypes.data,
                                              m.ctypes.data if m is not None else None, C.byref(prm), C.byref(res)))
        out = {k: v[0] for k, v in d.items()}
        for k in ("n_good", "n_edges", "rounds_run"):
            out[k] = int(out[k])
        out["outliers"] = out["outliers"][:n]
        return out

    def pose_optimize_device(self, d_p3d, d_p2d, d_n, K, d_Tcw0, d_mask=None, chi2=5.991, Tcw0_stride=12,
                             mask_stride=None, out=None, diagnostics=True, stream=None):
        """The same for a batch in device memory: d_p3d f32 [L, cap, 3], d_p2d f32 [L, cap, 2], d_n int32 [L] (negative:
        no valid list), d_Tcw0 f32 with list l's 12 floats at element l * Tcw0_stride, d_mask uint8 with list l's bytes
        at l * mask_stride (default cap) or None: a view into Tcw_refined / inliers_refined of pnp_ransac_device's result
        can be passed with its strides.  -> dict of CUDA tensors with a leading L, named and shaped as msf_pose_result
        says; without `diagnostics` only the per-list arrays.  `out`: tensors to write into instead of fresh zeros.
        One launch, asynchronous on `stream` (None = handle stream + sync)."""
        import torch
        assert d_p3d.is_cuda and d_p2d.is_cuda and d_n.is_cuda and d_p3d.is_contiguous() and d_p2d.is_contiguous()
        assert d_p3d.dtype == torch.float32 and d_p2d.dtype == torch.float32 and d_n.dtype == torch.int32
        L, cap = d_p3d.shape[0], d_p3d.shape[1]
        assert tuple(d_p3d.shape) == (L, cap, 3) and tuple(d_p2d.shape) == (L, cap, 2) and d_n.numel() == L
        assert d_Tcw0.is_cuda and d_Tcw0.dtype == torch.float32 and Tcw0_stride >= 0
        assert L == 0 or d_Tcw0.untyped_storage().nbytes() // 4 - d_Tcw0.storage_offset() >= (L - 1) * Tcw0_stride + 12
        if d_mask is not None:
            mask_stride = cap if mask_stride is None else mask_stride
            assert d_mask.is_cuda and d_mask.dtype == torch.uint8 and mask_stride >= 0
            assert L == 0 or d_mask.untyped_storage().nbytes() - d_mask.storage_offset() >= (L - 1) * mask_stride + cap
        d = out
        if d is None:
            z = _zeros_on(d_p3d.device)
            d = {k: z(shape, dt) for k, (shape, dt) in _lib.pose_shapes(L, cap).items()}
            if not diagnostics:
                for name, _, per, _ in _lib.POSE_ARRAYS:
                    if per != "list":
                        del d[name]
        res = _fill(_lib.PoseResult(), d)
        prm = self._pose_params(K, chi2)
        self._check(self._L.msf_pose_optimize_device(self._h, L, d_p3d.data_ptr(), d_p2d.data_ptr(), cap, d_n.data_ptr(),
                                                     d_Tcw0.data_ptr(), Tcw0_stride,
                                                     d_mask.data_ptr() if d_mask is not None else None,
                                                     mask_stride or 0, C.byref(prm), C.byref(res), stream))
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
        tcw = np.ascontiguousarray(cam_Tcw, np.float32).reshape(-1, 12)
        fixed = np.ascontiguousarray(cam_fixed, np.uint8).reshape(-1)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        ec = np.ascontiguousarray(edge_cam, np.int32).reshape(-1)
        ep = np.ascontiguousarray(edge_point, np.int32).reshape(-1)
        obs = np.ascontiguousarray(edge_obs, np.float32).reshape(-1, 2)
        nc, npt, ne = len(tcw), len(pts), len(ec)
        assert len(fixed) == nc and len(ep) == ne and len(obs) == ne
        d = {k: np.zeros(shape, dt) for k, (shape, dt) in _lib.ba_shapes(1, nc, npt, ne).items()}
        if not diagnostics:
            for name, _, per, _ in _lib.BA_ARRAYS:
                if per.startswith("it"):
                    del d[name]
        res = _fill(_lib.BaResult(), d)
        prm = self._ba_params(K, schedule, huber_delta2, chi2)
        st = None if stop is None else np.array([stop], np.int32)
        self._check(self._L.msf_bundle_adjust(self._h, nc, tcw.ctypes.data, fixed.ctypes.data, npt, pts.ctypes.data, ne,
                                              ec.ctypes.data, ep.ctypes.data, obs.ctypes.data,
                                              st.ctypes.data if st is not None else None, C.byref(prm), C.byref(res)))
        out = dict(d)
        out["status"] = int(d["status"][0])
        out["round_iterations"] = d["round_iterations"][0]
        for name, _, per, _ in _lib.BA_ARRAYS:
            if name not in d:
                continue
            if per == "it":
                out[name] = d[name][0]
            elif per == "it_cam":
                out[name] = d[name].reshape((_lib.BA_SLOTS, nc) + d[name].shape[1:])
            elif per == "it_point":
                out[name] = d[name].reshape((_lib.BA_SLOTS, npt) + d[name].shape[1:])
        return out

    def bundle_adjust_device(self, d_problems, d_cam_Tcw, d_cam_fixed, d_points, d_edge_cam, d_edge_point, d_edge_obs, K,
                             schedule=(2, (5, 10), (1, 0)), max_free_cams=64, d_stop=None, huber_delta2=5.991, chi2=5.991,
                             out=None, diagnostics=True, stream=None):
        """The same for a batch in device memory: d_problems int32 [P, 6] (n_cams, n_points, n_edges, cam0, point0,
        edge0; n_cams < 0: no valid problem), the camera, point and edge arrays concatenated (edge indices local to
        their problem), d_stop None or an int32 tensor of one element.  -> dict of CUDA tensors named and shaped as
        _lib.ba_shapes(P, cams, points, edges) says; without `diagnostics` no per-iteration arrays.  `out`: tensors to
        write into instead of fresh zeros.  One launch, asynchronous on `stream` (None = handle stream + sync)."""
        import torch
        for t, dt in ((d_problems, torch.int32), (d_cam_Tcw, torch.float32), (d_cam_fixed, torch.uint8), (d_points, torch.float32),
                      (d_edge_cam, torch.int32), (d_edge_point, torch.int32), (d_edge_obs, torch.float32)):
            assert t.is_cuda and t.is_contiguous() and t.dtype == dt
        P = d_problems.numel() // 6
        cams, points, edges = d_cam_fixed.numel(), d_points.numel() // 3, d_edge_cam.numel()
        assert d_cam_Tcw.numel() == cams * 12 and d_edge_point.numel() == edges and d_edge_obs.numel() == edges * 2
        if d_stop is not None:
            assert d_stop.is_cuda and d_stop.dtype == torch.int32 and d_stop.numel() == 1
        d = out
        if d is None:
            z = _zeros_on(d_points.device)
            d = {k: z(shape, dt) for k, (shape, dt) in _lib.ba_shapes(P, cams, points, edges).items()}
            if not diagnostics:
                for name, _, per, _ in _lib.BA_ARRAYS:
                    if per.startswith("it"):
                        del d[name]
        res = _fill(_lib.BaResult(), d)
        prm = self._ba_params(K, schedule, huber_delta2, chi2)
        self._check(self._L.msf_bundle_adjust_device(self._h, P, d_problems.data_ptr(), d_cam_Tcw.data_ptr(),
                                                     d_cam_fixed.data_ptr(), d_points.data_ptr(), d_edge_cam.data_ptr(),
                                                     d_edge_point.data_ptr(), d_edge_obs.data_ptr(), cams, points, edges,
                                                     max_free_cams, d_stop.data_ptr() if d_stop is not None else None,
                                                     C.byref(prm), C.byref(res), stream))
        return d

    def global_bundle_adjust(self, cam_Tcw, cam_fixed, points, edge_cam, edge_point, edge_obs, K, schedule=(1, (10, 0), (0, 0)),
                             stop=None, huber_delta2=5.991, chi2=5.991, diagnostics=True):
        """Optimizer::GlobalBundleAdjustemnt (Optimizer.cc:62-69; the default schedule is the reference's call) on one
        problem of up to 1024 free cameras, spread over the whole device: arguments and the returned dict as
        bundle_adjust, bit for bit the same result wherever bundle_adjust takes the problem.  stop: None, an int, or an
        int32 numpy array of one element that another thread may set while the call runs.  More than 1024 free cameras:
        MsfError with code MSF_ERR_CAPACITY."""
        tcw = np.ascontiguousarray(cam_Tcw, np.float32).reshape(-1, 12)
        fixed = np.ascontiguousarray(cam_fixed, np.uint8).reshape(-1)
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        ec = np.ascontiguousarray(edge_cam, np.int32).reshape(-1)
        ep = np.ascontiguousarray(edge_point, np.int32).reshape(-1)
        obs = np.ascontiguousarray(edge_obs, np.float32).reshape(-1, 2)
        nc, npt, ne = len(tcw), len(pts), len(ec)
        assert len(fixed) == nc and len(ep) == ne and len(obs) == ne
        d = {k: np.zeros(shape, dt) for k, (shape, dt) in _lib.ba_shapes(1, nc, npt, ne).items()}
        if not diagnostics:
            for name, _, per, _ in _lib.BA_ARRAYS:
                if per.startswith("it"):
                    del d[name]
        res = _fill(_lib.BaResult(), d)
        prm = self._ba_params(K, schedule, huber_delta2, chi2)
        if stop is None or isinstance(stop, np.ndarray):
            st = stop
            assert st is None or (st.dtype == np.int32 and st.size == 1)
        else:
            st = np.array([stop], np.int32)
        self._check(self._L.msf_global_bundle_adjust(self._h, nc, tcw.ctypes.data, fixed.ctypes.data, npt, pts.ctypes.data,
                                                     ne, ec.ctypes.data, ep.ctypes.data, obs.ctypes.data,
                                                     st.ctypes.data if st is not None else None, C.byref(prm), C.byref(res)))
        out = dict(d)
        out["status"] = int(d["status"][0])
        out["round_iterations"] = d["round_iterations"][0]
        for name, _, per, _ in _lib.BA_ARRAYS:
            if name not in d:
                continue
            if per == "it":
                out[name] = d[name][0]
            elif per == "it_cam":
                out[name] = d[name].reshape((_lib.BA_SLOTS, nc) + d[name].shape[1:])
            elif per == "it_point":
                out[name] = d[name].reshape((_lib.BA_SLOTS, npt) + d[name].shape[1:])
        return out

    def global_bundle_adjust_device(self, d_cam_Tcw, d_cam_fixed, d_points, d_edge_cam, d_edge_point, d_edge_obs, K,
                                    schedule=(1, (10, 0), (0, 0)), max_free_cams=_lib.GBA_MAX_FREE_CAMS, d_stop=None,
                                    huber_delta2=5.991, chi2=5.991, out=None, diagnostics=True, stream=None):
        """The same with the problem in device memory (tensors as one problem of bundle_adjust_device, d_stop None or
        an int32 tensor of one element).  -> dict of CUDA tensors named and shaped as _lib.ba_shapes(1, cams, points,
        edges) says; without `diagnostics` no per-iteration arrays.  `out`: tensors to write into instead of fresh
        zeros.  Enqueued on `stream`, but the host decides every trial: the call returns when the problem is finished."""
        import torch
        for t, dt in ((d_cam_Tcw, torch.float32), (d_cam_fixed, torch.uint8), (d_points, torch.float32),
                      (d_edge_cam, torch.int32), (d_edge_point, torch.int32), (d_edge_obs, torch.float32)):
            assert t.is_cuda and t.is_contiguous() and t.dtype == dt
        cams, points, edges = d_cam_fixed.numel(), d_points.numel() // 3, d_edge_cam.numel()
        assert d_cam_Tcw.numel() == cams * 12 and d_edge_point.numel() == edges and d_edge_obs.numel() == edges * 2
        if d_stop is not None:
            assert d_stop.is_cuda and d_stop.dtype == torch.int32 and d_stop.numel() == 1
        d = out
        if d is None:
            z = _zeros_on(d_points.device)
            d = {k: z(shape, dt) for k, (shape, dt) in _lib.ba_shapes(1, cams, points, edges).items()}
            if not diagnostics:
                for name, _, per, _ in _lib.BA_ARRAYS:
                    if per.startswith("it"):
                        del d[name]
        res = _fill(_lib.BaResult(), d)
        prm = self._ba_params(K, schedule, huber_delta2, chi2)
        self._check(self._L.msf_global_bundle_adjust_device(self._h, cams, d_cam_Tcw.data_ptr(), d_cam_fixed.data_ptr(),
                                                            points, d_points.data_ptr(), edges, d_edge_cam.data_ptr(),
                                                            d_edge_point.data_ptr(), d_edge_obs.data_ptr(), max_free_cams,
                                                            d_stop.data_ptr() if d_stop is not None else None,
                                                            C.byref(prm), C.byref(res), stream))
        return d

    def render_match_image(self, frame1, frame2, matches, has_mp1=None, has_mp2=None):
        """Tracking::CreateCurrentMatchImage (Tracking.cc:899-940) -> uint8 [H, 2W, 3]."""
        a, b = self._image(frame1), self._image(frame2)
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 4)
        f1 = None if has_mp1 is None else np.ascontiguousarray(has_mp1, np.uint8)
        f2 = None if has_mp2 is None else np.ascontiguousarray(has_mp2, np.uint8)
        out = np.zeros((self.height, 2 * self.width, 3), np.uint8)
        self._check(self._L.msf_render_match_image(self._h, C.byref(a), C.byref(b), m.ctypes.data, len(m),
                                                   None if f1 is None else f1.ctypes.data,
                                                   None if f2 is None else f2.ctypes.data, out.ctypes.data,
                                                   out.strides[0]))
        return out

    def store_frame(self, slot, frame):
        """Uploads a host frame into resident frame slot `slot` (ORB: and extracts its features once)."""
        img = self._image(frame)
        self._check(self._L.msf_store_frame(self._h, slot, C.byref(img)))

    def match_one_to_many(self, query_slot, slots, with_map_points=False, cap=0):
        """MatchFrames(frame[query_slot], frame[s]) for s in slots, one launch sequence.
        -> (num_matches[n], num_mp[n] or None, lists or None)"""
        slots = np.ascontiguousarray(np.asarray(slots, np.int32).reshape(-1))
        n = slots.size
        num = np.zeros((n,), np.int32)
        nmp = np.zeros((n,), np.int32) if with_map_points else None
        out = np.zeros((n, cap), _lib.MATCH_DTYPE) if cap else None
        self._check(self._L.msf_match_one_to_many(self._h, query_slot, n, slots.ctypes.data, num.ctypes.data,
                                                  nmp.ctypes.data if with_map_points else None,
                                                  out.ctypes.data if cap else None, cap))
        lists = None
        if cap:
            lists = [out[i, :min(max(num[i], 0), cap)].view(np.int32).reshape(-1, 4).copy() for i in range(n)]
        return num, nmp, lists

    def last_error(self):
        """msf_last_error(h): the text of the handle's last failure -- or note (a call that succeeded may leave one)"""
        return self._L.msf_last_error(self._h).decode()

    def stage_times(self):
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        n = self._L.msf_stage_times(self._h, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(n)}

    # --- introspection (parity tests) ----------------------------------------------------------
    def _debug(self, what, slot, level, dtype, cap_bytes):
        buf = np.zeros((cap_bytes,), np.uint8)
        nb = C.c_size_t(0)
        self._check(self._L.msf_debug_get(self._h, what, slot, level, buf.ctypes.data, cap_bytes, C.byref(nb)))
        if nb.value > cap_bytes:
            return self._debug(what, slot, level, dtype, nb.value)
        return buf[:nb.value].view(dtype).copy()


class FeatureMatcher(_Matcher):
    """ORB (cv::ORB::create() defaults) + BruteForce-Hamming 2-NN + ratio test, on the GPU."""
    _kind = _lib.MSF_KIND_ORB

    def __init__(self, threshold=0.8, image_width=640, image_height=480, **kw):
        super().__init__(threshold, image_width, image_height, **kw)

    def level_sizes(self):
        return self._debug(_lib.DBG_LEVEL_SIZES, 0, 0, np.int32, 8 * 4 * 4).reshape(8, 4)

    def walk_mode(self):
        """(per_level, stalls): whether this handle launches the walker level by level -- MSF_ORB_WALK_PER_LEVEL=1, or
        after a unit of a one-launch walker gave up a bounded wait (include/msf_abi.h, "Walker stall") -- and how many
        units have given up since the handle was made.  Asked of the handle, not of the environment."""
        v = self._debug(_lib.DBG_WALK_MODE, 0, 0, np.int32, 8)
        return bool(v[0]), int(v[1])

    def walk_finished(self, slot, cache=False):
        """bit mask of the levels of `slot` that were finished -- completeness check, retainBest(2N) cut, Harris responses
        -- by a finish unit inside the last extraction's walker launch (MSF_DBG_WALK_FINISHED)"""
        return int(self._debug(_lib.DBG_WALK_FINISHED, self._slot(slot, cache), 0, np.int32, 4)[0])

    def walker_launches(self, stage):
        """Launches of the dominant kernel (the streaming walker k_walk) in one extraction of a batch: ONE -- all levels,
        their thresholds and the pyramid in one launch (r03: 2 chains x 8 levels of sampler + walker launches); eight when
        the handle runs level by level (walk_mode)."""
        return 8 if (stage == "pyramid_fast" and self.walk_mode()[0]) else 1

    # Introspection of the feature slots.  `slot` counts from the scratch slots of the last MatchFrames / match_batch
    # call (frame A of pair i = i, frame B = n_pairs + i); cache=True addresses the per-frame cache slots of
    # extract_device / store_frame instead (the two ranges are disjoint: [2P, 4P) and [0, 2P), P = max_batch_pairs).
    def _slot(self, slot, cache):
        return slot if cache else 2 * self.max_batch_pairs + slot

    def level_pixels(self, slot, level, cache=False):
        w, h, pitch, _ = self.level_sizes()[level]
        return self._debug(_lib.DBG_LEVEL_PIXELS, self._slot(slot, cache), level, np.uint8,
                           int(pitch) * int(h)).reshape(h, pitch)[:, :w]

    def fast_candidates(self, slot, level, cache=False):
        return self._debug(_lib.DBG_FAST_CANDS, self._slot(slot, cache), level, np.int32, 1 << 20).reshape(-1, 3)

    def fast_tau(self, slot, cache=False):
        """int32 [8, 2]: per level the FAST score threshold the candidate list was built with, and its first estimate."""
        return self._debug(_lib.DBG_FAST_TAU, self._slot(slot, cache), 0, np.int32, 64).reshape(-1, 2)

    def stage1(self, slot, level, cache=False):
        return self._debug(_lib.DBG_STAGE1, self._slot(slot, cache), level, _lib.KP_DTYPE, 1 << 18)

    def keypoints(self, slot, cache=False):
        return self._debug(_lib.DBG_KEYPOINTS, self._slot(slot, cache), 0, _lib.KP_DTYPE, 2048 * 32)

    def descriptors(self, slot, cache=False):
        return self._debug(_lib.DBG_DESCRIPTORS, self._slot(slot, cache), 0, np.uint8, 2048 * 32).reshape(-1, 32)

    def set_features(self, slot, kp, desc):
        """Debug (msf_debug_orb_set_features): writes caller features into feature slot `slot` of [0, 2 * max_batch_pairs)
        -- the slots match_slots_device pairs and keypoints(slot, cache=True) reads.  kp: KP_DTYPE [n], or float [n, 2]
        (x, y; the other fields zero); desc: uint8 [n, 32]; n <= 2048."""
        kp = np.asarray(kp)
        if kp.dtype != _lib.KP_DTYPE:
            xy = np.asarray(kp, np.float32).reshape(-1, 2)
            kp = np.zeros(len(xy), _lib.KP_DTYPE)
            kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
        kp = np.ascontiguousarray(kp.reshape(-1))
        desc = np.ascontiguousarray(np.asarray(desc, np.uint8).reshape(-1, 32))
        if len(desc) != len(kp):
            raise ValueError("one descriptor per key point")
        self._check(self._L.msf_debug_orb_set_features(self._h, slot, len(kp), kp.ctypes.data if len(kp) else None,
                                                       desc.ctypes.data if len(kp) else None))

    def orb_tail(self, d_frames, lists, first_slot=0, form=0):
        """Debug (msf_debug_orb_tail): everything behind FAST on the caller's candidates.  d_frames: device uint8
        [n, H, pitch]; lists[f][l]: int [k, 3] rows (lx, ly, fast_score) of frame f, level l (missing levels: empty);
        form 0: the dense form of k_thr_harris, 1: the streaming form + k_harris_flat.  Results: stage1 / keypoints /
        descriptors(first_slot + f, cache=True)."""
        n = d_frames.shape[0]
        if len(lists) != n:
            raise ValueError("one list of levels per frame")
        counts = np.zeros((n, 8), np.int32)
        rows = []
        for f, levels in enumerate(lists):
            for l, c in enumerate(levels):
                c = np.asarray(c, np.int32).reshape(-1, 3)
                counts[f, l] = len(c)
                rows.append(c)
        cands = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 3), np.int32))
        self._check(self._L.msf_debug_orb_tail(self._h, n, d_frames.data_ptr(), d_frames.stride(0), d_frames.stride(1),
                                               first_slot, counts.ctypes.data, cands.ctypes.data if len(cands) else None,
                                               form))

    def match_form(self):
        """(form, chunk): the kernel of this handle's last match launch -- 0 none yet, 1 k_match_split (calls of at most
        128 pairs), 2 k_match -- and the train chunk in effect (1024, or MSF_ORB_TRAIN_CHUNK)."""
        v = self._debug(_lib.DBG_ORB_MATCH_FORM, 0, 0, np.int32, 8)
        return int(v[0]), int(v[1])


class DNNFeatureMatcher(_Matcher):
    """LoFTR_teacher (model/LoFTR_teacher.onnx restated as HIP kernels) + threshold + decode, on the GPU.
    model_file_path: the reference's .onnx file (read directly) or an MSFLTR01 blob; None = the blob shipped with the
    package."""
    _kind = _lib.MSF_KIND_LOFTR

    def __init__(self, model_file_path=None, threshold=0.15, image_width=640, image_height=480,
                 model_resolution=16, **kw):
        if model_resolution != 16:
            raise MsfError(_lib.MSF_ERR_UNSUPPORTED, "LoFTR_teacher works at 1/16 resolution only")
        super().__init__(threshold, image_width, image_height, weights_path=model_file_path, **kw)

    def conf_matrix(self, pair=0):
        return self._debug(_lib.DBG_LOFTR_CONF, pair, 0, np.float32, 1200 * 1200 * 4).reshape(1200, 1200)

    def coarse_features(self, pair=0):
        return self._debug(_lib.DBG_LOFTR_FEAT, pair, 0, np.float32, 2 * 1200 * 32 * 4).reshape(2, 1200, 32)

    def backbone_tokens(self, pair=0):
        """pair 0's tokens before the transformer (backbone + positional encoding) of the last match call: [2][1200][32]"""
        return self._debug(_lib.DBG_LOFTR_TOK, pair, 0, np.float32, 2 * 1200 * 32 * 4).reshape(2, 1200, 32)

    def transformer_device(self, d_in0, d_in1, d_out0, d_out1, first=0, n=8, stream=None):
        """Encoder blocks [first, first + n) alone (msf_debug_loftr_transformer): d_in0 / d_in1 float32 CUDA tensors
        [p, 1200, 32], the two sequences before block `first`; d_out0 / d_out1 the same shape, written with the two
        sequences after the range.  Asynchronous on `stream` (an int hipStream_t; None = handle stream + sync)."""
        import torch
        p = d_in0.shape[0]
        for t in (d_in0, d_in1, d_out0, d_out1):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (p, 1200, 32)
        self._check(self._L.msf_debug_loftr_transformer(self._h, p, first, n, d_in0.data_ptr(), d_in1.data_ptr(),
                                                        d_out0.data_ptr(), d_out1.data_ptr(), stream))

    def head_device(self, d_f0, d_f1, d_out, d_n_out, stream=None):
        """The matching head alone (msf_debug_loftr_head) on coarse features the caller supplies: d_f0 / d_f1 float32
        CUDA tensors [n, 1200, 32], post-transformer and unscaled (coarse_features() layout); d_out int32 [n, cap, 4],
        d_n_out int32 [n].  Asynchronous on `stream` (an int hipStream_t; None = handle stream + sync)."""
        import torch
        n = d_f0.shape[0]
        for t, dt in ((d_f0, torch.float32), (d_f1, torch.float32), (d_out, torch.int32), (d_n_out, torch.int32)):
            assert t.is_cuda and t.dtype == dt and t.is_contiguous()
        assert tuple(d_f0.shape) == (n, 1200, 32) and d_f1.shape == d_f0.shape
        assert d_out.dim() == 3 and d_out.shape[0] == n and d_out.shape[2] == 4 and tuple(d_n_out.shape) == (n,)
        self._check(self._L.msf_debug_loftr_head(self._h, n, d_f0.data_ptr(), d_f1.data_ptr(), d_out.data_ptr(),
                                                 d_out.shape[1], d_n_out.data_ptr(), stream))

    def backbone_device(self, d_a, d_b, d_tok_a, d_tok_b, act_image=0, frame_stride=None, row_stride=None, n=None,
                        stream=None):
        """The ResNet backbone alone (msf_debug_loftr_backbone), one backbone pass: d_a uint8 CUDA frames, n of them;
        d_b the same or None (the extract form; d_tok_b may then be None too).  Dense [n, 480, 640] frames by default,
        else `n` frames `frame_stride` bytes apart with rows `row_stride` bytes apart.  d_tok_a / d_tok_b: float32
        CUDA tensors [n, 1200, 32], written with the tokens before the transformer.  With MSF_FLAG_KEEP_DEBUG
        backbone_activation() then returns image `act_image` of the pass (A frames first).  Asynchronous on `stream`
        (an int hipStream_t; None = handle stream + sync)."""
        import torch
        if n is None:
            n = d_a.shape[0]
        row_stride = self.width if row_stride is None else row_stride
        frame_stride = row_stride * self.height if frame_stride is None else frame_stride
        for t in (d_a, d_b):
            assert t is None or (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() >= n * frame_stride)
        for t in (d_tok_a,) + ((d_tok_b,) if d_b is not None else ()):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (n, 1200, 32)
        self._check(self._L.msf_debug_loftr_backbone(self._h, n, d_a.data_ptr(), None if d_b is None else d_b.data_ptr(),
                                                     frame_stride, row_stride, act_image, d_tok_a.data_ptr(),
                                                     None if d_tok_b is None or d_b is None else d_tok_b.data_ptr(), stream))

    def backbone_activation(self, stage):
        """NCHW activation of the first frame of the last call after ResNet stage `stage` + 1 (MSF_FLAG_KEEP_DEBUG)"""
        shape = [(8, 240, 320), (16, 120, 160), (32, 60, 80), (32, 30, 40)][stage]
        return self._debug(_lib.DBG_LOFTR_ACT, 0, stage, np.float32, int(np.prod(shape)) * 4).reshape(shape)


class MultiDeviceMatcher:
    """One matcher over several GPUs of one process (msf_multi_*, include/msf_abi.h): a batch is cut into contiguous
    blocks of ceil(n / G) pairs, one per device, each run by that device's own handle on its own host thread; the lists
    come back in pair order, identical to one handle's (bit for bit for ORB and for LoFTR with MSF_FLAG_LOFTR_F32; LoFTR's
    default split-bf16 kernels depend on the call size and agree to ~1e-5 in confidence: include/msf_abi.h).  `devices`
    may name a device twice (two shards share the card).
    kind: "orb" (::FeatureMatcher) or "loftr" (::DNNFeatureMatcher).  The reference has no multi-GPU form; a
    multi-process job (bench.py --gpus N) uses ordinary matchers, one per rank."""

    def __init__(self, kind, threshold, image_width, image_height, devices=(0,), max_batch_pairs=1, flags=0,
                 weights_path=None):
        self._L = _lib.load()
        self._m = C.c_void_p()
        cfg = _lib.Config()
        self._L.msf_default_config(C.byref(cfg), {"orb": _lib.MSF_KIND_ORB, "loftr": _lib.MSF_KIND_LOFTR}[kind])
        cfg.threshold = threshold
        cfg.image_width = image_width
        cfg.image_height = image_height
        cfg.max_batch_pairs = max_batch_pairs
        cfg.flags = flags
        self._wpath = weights_path.encode() if weights_path else None
        cfg.weights_path = self._wpath
        ids = (C.c_int32 * len(devices))(*devices)
        rc = self._L.msf_multi_create(C.byref(cfg), len(devices), ids, C.byref(self._m))
        if rc != _lib.MSF_OK:
            msg = self._L.msf_multi_last_error(None).decode()
            self._m = C.c_void_p()
            raise MsfError(rc, msg)
        self.devices = tuple(devices)

    def close(self):
        if getattr(self, "_m", None) and self._m.value:
            self._L.msf_multi_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != _lib.MSF_OK:
            raise MsfError(rc, self._L.msf_multi_last_error(self._m).decode())

    def SetThreshold(self, value):
        self._check(self._L.msf_multi_set_threshold(self._m, float(value)))

    def shard_range(self, n_pairs, shard):
        first, count = C.c_int32(0), C.c_int32(0)
        self._L.msf_multi_shard_range(n_pairs, len(self.devices), shard, C.byref(first), C.byref(count))
        return first.value, count.value

    def match_batch(self, frames1, frames2, cap=4096):
        n = len(frames1)
        A = (_lib.Image * max(n, 1))(*[_Matcher._image(f) for f in frames1])
        B = (_lib.Image * max(n, 1))(*[_Matcher._image(f) for f in frames2])
        out = np.zeros((max(n, 1), cap), _lib.MATCH_DTYPE)
        cnt = np.zeros((max(n, 1),), np.int32)
        self._check(self._L.msf_multi_match_batch(self._m, n, A, B, out.ctypes.data, cap, cnt.ctypes.data))
        return [out[i, :min(cnt[i], cap)].view(np.int32).reshape(-1, 4).copy() for i in range(n)]

    def match_batch_device(self, d_a, d_b, d_out, d_n_out):
        """Per shard r: d_a[r] / d_b[r] uint8 CUDA tensors [n_r, H, pitch] on that shard's device, d_out[r] int32
        [n_r, cap, 4], d_n_out[r] int32 [n_r] (lists of len(devices) tensors; n_r may be 0).  Returns when every shard
        has finished."""
        G = len(self.devices)
        assert len(d_a) == len(d_b) == len(d_out) == len(d_n_out) == G
        vp = C.c_void_p
        ref = next(t for t in d_a if t.shape[0] > 0)
        for r in range(G):
            assert d_a[r].is_cuda and d_a[r].stride()[1:] == ref.stride()[1:] and d_b[r].stride() == d_a[r].stride()
        n = (C.c_int32 * G)(*[int(t.shape[0]) for t in d_a])
        pa = (vp * G)(*[t.data_ptr() for t in d_a])
        pb = (vp * G)(*[t.data_ptr() for t in d_b])
        po = (vp * G)(*[t.data_ptr() for t in d_out])
        pn = (vp * G)(*[t.data_ptr() for t in d_n_out])
        self._check(self._L.msf_multi_match_batch_device(self._m, n, pa, pb, ref.stride(0), ref.stride(1), po,
                                                         d_out[0].shape[1], pn))
