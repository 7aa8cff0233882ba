"""GPU: the contract of the extern "C" boundary itself (csrc/msf_abi.cpp, csrc/abi_*.cpp), entry point by entry point: what a null
handle and a bad argument return and leave in msf_last_error, that a handle works after a refused call, the chunked
host batch, the count-only one-to-many call, and the grow-on-demand workspaces.  Codes and texts are the ones
include/msf_abi.h documents and the library has always produced; nothing here looks at a kernel's numbers beyond
"the same call gives the same answer".

One ORB handle and one LoFTR handle, both with max_batch_pairs = 2, frames from synth.  ORB runs at 200 x 150: of the
sizes the ORB GPU tests use, 64 x 64 is the smallest, but ORB's 31-pixel border leaves no key point there and every
list is empty (65 x 97, 69 x 91 and 127 x 64 give 0-4 matches); 200 x 150 is the smallest of them at which every pair
has a list that a prefix can be cut from.  Its width is no multiple of 16, so the staging pitch differs from the width.
The calls that need a handle nothing was stored in ("no frame was stored", "no map slot was ever set") get a fresh
ORB handle of the same size."""
import ctypes as C

import numpy as np
import pytest

from mono_slam_framework_amd import _lib, synth
from oracle import initializer as oracle_init
from tests.test_initializer_gpu import _same

pytestmark = pytest.mark.gpu

W, H, PITCH = 200, 150, 208
P = 2                                                   # max_batch_pairs of both handles
INV = _lib.MSF_ERR_INVALID_ARG
ALIGN_TEXT = "device frames must be 16-byte aligned with strides multiple of 16"


@pytest.fixture(scope="module")
def orb():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    fm = FeatureMatcher(0.7, W, H, max_batch_pairs=P)
    yield fm
    fm.close()


@pytest.fixture(scope="module")
def loftr():
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    dm = DNNFeatureMatcher(threshold=0.15, max_batch_pairs=P)
    yield dm
    dm.close()


@pytest.fixture(scope="module")
def frames():
    """five ORB pairs (A, B uint8 [5, H, W]); every pair has well over a hundred matches at ratio 0.7"""
    return synth.synth_batch(500, 5, W, H)


def _img(a):
    return _lib.Image(a.ctypes.data, a.shape[1], a.shape[0], a.strides[0])


def _err(m):
    return m._L.msf_last_error(m._h).decode()


def _device_frames(frames_a, frames_b, pitch):
    import torch
    n, h, w = frames_a.shape
    d = torch.zeros((2, n, h, pitch), dtype=torch.uint8, device="cuda")
    d[0, :, :, :w] = torch.from_numpy(frames_a).cuda()
    d[1, :, :, :w] = torch.from_numpy(frames_b).cuda()
    return d


def _ransac_result(**arrays):
    r = _lib.RansacResult(struct_size=C.sizeof(_lib.RansacResult))
    for k, v in arrays.items():
        setattr(r, k, v.ctypes.data)
    return r


def test_null_handle(orb):
    """every entry point that takes a handle: -1 (0 from msf_stage_times), and the text msf_last_error(NULL) returns --
    the creating thread's -- is not touched"""
    L = orb._L
    cfg = _lib.Config()
    L.msf_default_config(C.byref(cfg), _lib.MSF_KIND_ORB)
    cfg.struct_size = 4
    out = C.c_void_p()
    assert L.msf_create(C.byref(cfg), C.byref(out)) == INV and not out.value
    before = L.msf_last_error(None)
    assert before == b"msf_create: struct_size mismatch"
    z = None
    calls = {
        "msf_set_threshold": lambda: L.msf_set_threshold(z, 0.5),
        "msf_match_pair": lambda: L.msf_match_pair(z, None, None, z, 16, None),
        "msf_match_batch": lambda: L.msf_match_batch(z, 1, None, None, z, 16, z),
        "msf_match_batch_device": lambda: L.msf_match_batch_device(z, 1, z, z, 0, 0, z, 16, z, z),
        "msf_extract_device": lambda: L.msf_extract_device(z, 1, z, 0, 0, 0, z),
        "msf_match_slots_device": lambda: L.msf_match_slots_device(z, 1, z, z, z, 16, z, z),
        "msf_pack_matches_device": lambda: L.msf_pack_matches_device(z, 1, z, 16, z, z, z, z),
        "msf_debug_get": lambda: L.msf_debug_get(z, 0, 0, 0, z, 0, C.byref(C.c_size_t(0))),
        "msf_debug_loftr_head": lambda: L.msf_debug_loftr_head(z, 1, z, z, z, 16, z, z),
        "msf_debug_loftr_transformer": lambda: L.msf_debug_loftr_transformer(z, 1, 0, 8, z, z, z, z, z),
        "msf_debug_loftr_backbone": lambda: L.msf_debug_loftr_backbone(z, 1, z, z, 0, 0, 0, z, z, z),
        "msf_debug_orb_set_features": lambda: L.msf_debug_orb_set_features(z, 0, 0, z, z),
        "msf_debug_orb_tail": lambda: L.msf_debug_orb_tail(z, 1, z, 0, 0, 0, z, z, 0),
        "msf_set_mappoints": lambda: L.msf_set_mappoints(z, 0, z, 0),
        "msf_count_mappoint_matches_device": lambda: L.msf_count_mappoint_matches_device(z, 1, z, 16, z, z, z, z, z),
        "msf_store_frame": lambda: L.msf_store_frame(z, 0, None),
        "msf_match_one_to_many": lambda: L.msf_match_one_to_many(z, 0, 1, z, z, z, z, 0),
        "msf_check_hypotheses": lambda: L.msf_check_hypotheses(z, 0, 0, z, z, 0, z, 1.0, z, None, z),
        "msf_find_models": lambda: L.msf_find_models(z, 0, z, 0, z, 1.0, None, None),
        "msf_find_models_device": lambda: L.msf_find_models_device(z, 0, z, 16, z, 0, 0, 1.0, None, z),
        "msf_render_match_image": lambda: L.msf_render_match_image(z, None, None, z, 0, z, z, z, 0),
        "msf_frame_cache_stats": lambda: L.msf_frame_cache_stats(z, None, None, None),
    }
    takes_none = {"msf_abi_version", "msf_default_config", "msf_create", "msf_destroy", "msf_last_error",
                  "msf_weights_info", "msf_convert_weights", "msf_stage_times"}
    single = [s for s in _lib.ABI_SYMBOLS if not s.startswith(("msf_multi_", "msf_gather_"))]
    assert set(calls) | takes_none == set(single)          # a new entry point gets a line above
    for name, call in calls.items():
        assert call() == INV, name
        assert L.msf_last_error(None) == before, name
    assert L.msf_stage_times(z, (C.c_char_p * 4)(), (C.c_float * 4)(), 4) == 0
    L.msf_destroy(z)
    assert L.msf_last_error(None) == before


def test_bad_arguments_and_the_call_after(orb, loftr, frames):
    """one refused call per kind of bad argument and entry point: the code, the text (an entry's own checks name the
    entry; the checks the frame entries share do not), and then a correct call of the same entry on the same handle --
    a lock left held would hang it, an unfinished copy or a stale error would fail it"""
    import torch
    from mono_slam_framework_amd.matcher import FeatureMatcher
    L, h, lh = orb._L, orb._h, loftr._h
    A, B = frames
    a0, b0 = A[0], B[0]
    ia, ib = _img(a0), _img(b0)
    wrong = np.zeros((H, W + 8), np.uint8)
    iw = _img(wrong)
    cap = 512
    out = np.zeros((P, cap), _lib.MATCH_DTYPE)
    cnt = np.zeros(P, np.int32)
    n1 = C.c_int32(0)
    d = _device_frames(A[:P], B[:P], PITCH)
    fs = H * PITCH
    dA, dB = d[0].data_ptr(), d[1].data_ptr()
    d_out = torch.zeros((P, cap, 4), dtype=torch.int32, device="cuda")
    d_n = torch.zeros(P, dtype=torch.int32, device="cuda")
    d_packed = torch.zeros((P * cap, 4), dtype=torch.int32, device="cuda")
    d_off = torch.zeros(P + 1, dtype=torch.int32, device="cuda")
    d_s0 = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    d_s1 = torch.tensor([2, 3], dtype=torch.int32, device="cuda")
    d_mp = torch.zeros(P, dtype=torch.int32, device="cuda")
    po, pn = d_out.data_ptr(), d_n.data_ptr()
    slots = np.array([1, 2], np.int32)
    num = np.zeros(P, np.int32)
    m = np.ascontiguousarray(orb.match_batch([a0], [b0])[0][:64])
    assert len(m) == 64
    sets = np.stack([np.arange(8, dtype=np.int32) + i for i in range(4)])
    Hs = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (4, 1))
    sc = np.zeros(4, np.float32)
    best = C.c_int32(0)
    inl = np.zeros(64, np.uint8)
    res_keep = [np.zeros(4, np.float32), np.zeros(1, np.int32), np.zeros(4, np.float32), np.zeros(1, np.int32)]
    res = [_ransac_result(scores=res_keep[0], best=res_keep[1]), _ransac_result(scores=res_keep[2], best=res_keep[3])]
    short = _ransac_result(scores=res_keep[0], best=res_keep[1])
    short.struct_size = 8
    rgb = np.zeros((H, 2 * W, 3), np.uint8)
    feat = torch.zeros((2, 1, 1200, 32), dtype=torch.float32, device="cuda")
    feat_o = torch.zeros((2, 1, 1200, 32), dtype=torch.float32, device="cuda")
    lo = torch.zeros((1, 4096, 4), dtype=torch.int32, device="cuda")
    ln = torch.zeros(1, dtype=torch.int32, device="cuda")
    f0, f1, g0, g1 = feat[0].data_ptr(), feat[1].data_ptr(), feat_o[0].data_ptr(), feat_o[1].data_ptr()
    tok = torch.zeros((2, 2, 1200, 32), dtype=torch.float32, device="cuda")
    la, lb = synth.synth_pair(60, 640, 480, mode=1, shift=(32, 16))
    ld = _device_frames(np.stack([la, la]), np.stack([lb, lb]), 640)
    batch0 = _lib.RansacBatch(struct_size=0)
    fk = np.zeros(4, _lib.KP_DTYPE)
    fk["x"], fk["y"], fk["octave"] = [1.5, 2.5, 3.5, 4.5], [9, 8, 7, 6], [0, 1, 2, 3]
    fd = np.arange(4 * 32, dtype=np.uint8).reshape(4, 32)
    pk, pd = fk.ctypes.data, fd.ctypes.data
    set_features = "msf_debug_orb_set_features"
    tail = "msf_debug_orb_tail"
    tc = np.array([[1, 0, 0, 0, 0, 0, 0, 0]], np.int32)                       # one candidate on level 0
    tl, tb = np.array([[100, 100, 50]], np.int32), np.array([[30, 100, 50]], np.int32)

    def good_set_features():
        orb.set_features(2 * P - 1, fk, fd)                  # the last caller slot
        assert orb.keypoints(2 * P - 1, cache=True).tobytes() == fk.tobytes()
        np.testing.assert_array_equal(orb.descriptors(2 * P - 1, cache=True), fd)
        orb.set_features(0, fk[:0], fd[:0])                  # n = 0 with null pointers
        assert len(orb.keypoints(0, cache=True)) == 0

    def good_find_models_device(mt):
        r = mt.find_models_device(d_out, d_n, n_hyp=8, seed=1)
        torch.cuda.synchronize()
        return r

    # correct calls, per entry (the wrappers of matcher.py raise on any status but MSF_OK)
    good = {
        "msf_match_batch": lambda: orb.match_batch(list(A[:3]), list(B[:3]), cap=cap),
        "msf_match_pair": lambda: orb.MatchFrames(a0, b0),
        "msf_match_batch_device": lambda: orb._check(L.msf_match_batch_device(h, P, dA, dB, fs, PITCH, po, cap, pn, None)),
        "msf_extract_device": lambda: orb._check(L.msf_extract_device(h, P, dA, fs, PITCH, 0, None)),
        "msf_match_slots_device": lambda: (orb._check(L.msf_extract_device(h, P, dA, fs, PITCH, 0, None)),
                                           orb._check(L.msf_extract_device(h, P, dB, fs, PITCH, 2, None)),
                                           orb.match_slots_device(d_s0, d_s1, d_out, d_n)),
        "msf_pack_matches_device": lambda: orb.pack_matches_device(d_out, d_n, d_packed, d_off),
        "msf_set_mappoints": lambda: orb.set_mappoints(1, [5, 77, W * H - 1, W * H, -3]),
        "msf_count_mappoint_matches_device": lambda: (orb.set_mappoints(0, [1, 2, 3]),
                                                      orb.count_mappoint_matches_device(d_out, d_n, d_s0, d_s0, d_mp)),
        "msf_store_frame": lambda: orb.store_frame(3, b0),
        "msf_match_one_to_many": lambda: ([orb.store_frame(i, f) for i, f in enumerate((a0, b0, B[1]))],
                                          orb.match_one_to_many(0, [1, 2])),
        "msf_check_hypotheses": lambda: orb.check_hypotheses(0, Hs, Hs, m, 1.0),
        "msf_find_models": lambda: orb.find_models(m, sets, 1.0),
        "msf_find_models_device": lambda: good_find_models_device(orb),
        "msf_render_match_image": lambda: orb.render_match_image(a0, b0, m[:10]),
        "msf_debug_get": lambda: orb.level_sizes(),
        "msf_stage_times": lambda: orb.stage_times(),
        "loftr msf_match_batch_device": lambda: loftr.match_batch_device(ld[0, :1], ld[1, :1], lo, ln),
        "loftr msf_match_slots_device": lambda: (loftr.extract_device(ld[0], 0), loftr.extract_device(ld[1], 2),
                                                 loftr.match_slots_device(d_s0[:1], d_s1[:1], lo, ln)),
        "msf_debug_loftr_head": lambda: loftr.head_device(feat[0], feat[1], lo, ln),
        "msf_debug_loftr_transformer": lambda: loftr.transformer_device(feat[0], feat[1], feat_o[0], feat_o[1], 0, 2),
        "msf_debug_loftr_backbone": lambda: loftr.backbone_device(ld[0], ld[1], tok[0], tok[1], act_image=3),
        set_features: good_set_features,
        tail: lambda: (orb.orb_tail(d[0][:1], [[tl]], first_slot=1), orb.keypoints(1, cache=True)),
    }
    bad_arg = lambda e: e + ": bad argument"                                                     # noqa: E731
    # (handle, entry whose good call follows, what is wrong, call, status, text left in msf_last_error)
    cases = [
        (orb, "msf_match_batch", "cap_per_pair = 0",
         lambda: L.msf_match_batch(h, 1, C.byref(ia), C.byref(ib), out.ctypes.data, 0, cnt.ctypes.data),
         INV, bad_arg("msf_match_batch")),
        (orb, "msf_match_batch", "wrong image size",
         lambda: L.msf_match_batch(h, 1, C.byref(ia), C.byref(iw), out.ctypes.data, cap, cnt.ctypes.data),
         INV, "msf_match_batch: image size differs from the handle's, or null data"),
        (orb, "msf_match_pair", "null out", lambda: L.msf_match_pair(h, C.byref(ia), C.byref(ib), None, cap, C.byref(n1)),
         INV, bad_arg("msf_match_batch")),                 # msf_match_pair is msf_match_batch with one pair
        (orb, "msf_match_batch_device", "cap_per_pair = 0",
         lambda: L.msf_match_batch_device(h, P, dA, dB, fs, PITCH, po, 0, pn, None), INV, bad_arg("msf_match_batch_device")),
        (orb, "msf_match_batch_device", "n_pairs > max_batch_pairs",
         lambda: L.msf_match_batch_device(h, P + 1, dA, dB, fs, PITCH, po, cap, pn, None), INV, "n_pairs exceeds max_batch_pairs"),
        (orb, "msf_match_batch_device", "misaligned frames",
         lambda: L.msf_match_batch_device(h, 1, dA + 4, dB, fs, PITCH, po, cap, pn, None), INV, ALIGN_TEXT),
        (orb, "msf_match_batch_device", "row_stride < W",
         lambda: L.msf_match_batch_device(h, P, dA, dB, fs, W - 8, po, cap, pn, None), INV, "row_stride < image_width"),
        (orb, "msf_match_batch_device", "frames overlap",
         lambda: L.msf_match_batch_device(h, P, dA, dB, fs - 16, PITCH, po, cap, pn, None),
         INV, "frame_stride < row_stride * image_height (frames would overlap)"),
        (orb, "msf_extract_device", "slot range out of bounds",
         lambda: L.msf_extract_device(h, P, dA, fs, PITCH, 2 * P - 1, None),
         INV, "msf_extract_device: slot range outside [0, 2*max_batch_pairs)"),
        (orb, "msf_extract_device", "misaligned frames", lambda: L.msf_extract_device(h, P, dA, fs, PITCH + 4, 0, None),
         INV, ALIGN_TEXT),
        (orb, "msf_extract_device", "row_stride < W", lambda: L.msf_extract_device(h, P, dA, fs, W - 8, 0, None),
         INV, "msf_extract_device: strides smaller than the frame"),
        (orb, "msf_match_slots_device", "null slots",
         lambda: L.msf_match_slots_device(h, P, None, d_s1.data_ptr(), po, cap, pn, None), INV, bad_arg("msf_match_slots_device")),
        (orb, "msf_pack_matches_device", "cap_per_pair = 0",
         lambda: L.msf_pack_matches_device(h, P, po, 0, pn, d_packed.data_ptr(), d_off.data_ptr(), None),
         INV, bad_arg("msf_pack_matches_device")),
        (orb, "msf_set_mappoints", "map slot out of bounds", lambda: L.msf_set_mappoints(h, 2 * P, None, 0),
         INV, bad_arg("msf_set_mappoints")),
        (orb, "msf_count_mappoint_matches_device", "null counts",
         lambda: L.msf_count_mappoint_matches_device(h, P, po, cap, None, d_s0.data_ptr(), d_s0.data_ptr(), d_mp.data_ptr(), None),
         INV, bad_arg("msf_count_mappoint_matches_device")),
        (orb, "msf_store_frame", "slot out of bounds", lambda: L.msf_store_frame(h, 2 * P, C.byref(ia)),
         INV, "msf_store_frame: slot outside [0, 2*max_batch_pairs) or image size differs from the handle's"),
        (orb, "msf_store_frame", "wrong image size", lambda: L.msf_store_frame(h, 0, C.byref(iw)),
         INV, "msf_store_frame: slot outside [0, 2*max_batch_pairs) or image size differs from the handle's"),
        (orb, "msf_match_one_to_many", "n > max_batch_pairs",
         lambda: L.msf_match_one_to_many(h, 0, P + 1, slots.ctypes.data, num.ctypes.data, None, None, 0),
         INV, "msf_match_one_to_many: n exceeds max_batch_pairs"),
        (orb, "msf_match_one_to_many", "null slots",
         lambda: L.msf_match_one_to_many(h, 0, P, None, num.ctypes.data, None, None, 0), INV, bad_arg("msf_match_one_to_many")),
        (orb, "msf_match_one_to_many", "lists without a capacity",
         lambda: L.msf_match_one_to_many(h, 0, P, slots.ctypes.data, num.ctypes.data, None, out.ctypes.data, 0),
         INV, bad_arg("msf_match_one_to_many")),
        (orb, "msf_check_hypotheses", "model 2",
         lambda: L.msf_check_hypotheses(h, 2, 4, Hs.ctypes.data, Hs.ctypes.data, 64, m.ctypes.data, 1.0, sc.ctypes.data,
                                        C.byref(best), inl.ctypes.data),
         INV, "msf_check_hypotheses: bad argument (models 0/1, at most 8192 matches)"),
        (orb, "msf_find_models", "wrong struct_size",
         lambda: L.msf_find_models(h, 64, m.ctypes.data, 4, sets.ctypes.data, 1.0, C.byref(short), C.byref(res[1])),
         INV, "msf_find_models: bad argument (8 to 8192 matches, sets, best and scores required, "
              "struct_size = sizeof(msf_ransac_result))"),
        (orb, "msf_find_models", "set index past the list",
         lambda: L.msf_find_models(h, 8, m.ctypes.data, 4, sets.ctypes.data, 1.0, C.byref(res[0]), C.byref(res[1])),
         INV, "msf_find_models: a set holds an index outside [0, n_matches)"),
        (orb, "msf_find_models_device", "wrong struct_size",
         lambda: L.msf_find_models_device(h, P, po, cap, pn, 8, 1, 1.0, C.byref(batch0), None),
         INV, "msf_find_models_device: bad argument (at most 65535 lists, best required, "
              "struct_size = sizeof(msf_ransac_batch))"),
        (orb, "msf_render_match_image", "wrong image size",
         lambda: L.msf_render_match_image(h, C.byref(ia), C.byref(iw), m.ctypes.data, 10, None, None, rgb.ctypes.data, 6 * W),
         INV, "msf_render_match_image: bad argument or image size differs from the handle's"),
        (orb, "msf_debug_get", "null n_bytes", lambda: L.msf_debug_get(h, 0, 0, 0, None, 0, None), INV, None),
        (orb, "msf_stage_times", "cap = 0", lambda: L.msf_stage_times(h, (C.c_char_p * 4)(), (C.c_float * 4)(), 0), 0, None),
        (orb, "msf_debug_loftr_head", "ORB handle", lambda: L.msf_debug_loftr_head(h, 1, f0, f1, lo.data_ptr(), 64, ln.data_ptr(), None),
         INV, "msf_debug_loftr_head: not a LoFTR handle"),
        (orb, "msf_debug_loftr_transformer", "ORB handle", lambda: L.msf_debug_loftr_transformer(h, 1, 0, 2, f0, f1, g0, g1, None),
         INV, "msf_debug_loftr_transformer: not a LoFTR handle"),
        (orb, "msf_debug_loftr_backbone", "ORB handle",
         lambda: L.msf_debug_loftr_backbone(h, 1, dA, dB, fs, PITCH, 0, tok[0].data_ptr(), tok[1].data_ptr(), None),
         INV, "msf_debug_loftr_backbone: not a LoFTR handle"),
        (loftr, set_features, "LoFTR handle", lambda: L.msf_debug_orb_set_features(lh, 0, 4, pk, pd),
         INV, set_features + ": not an ORB handle"),
        (orb, set_features, "slot = 2 * max_batch_pairs", lambda: L.msf_debug_orb_set_features(h, 2 * P, 4, pk, pd),
         INV, set_features + ": slot outside [0, 2*max_batch_pairs)"),
        (orb, set_features, "slot = -1", lambda: L.msf_debug_orb_set_features(h, -1, 4, pk, pd),
         INV, set_features + ": slot outside [0, 2*max_batch_pairs)"),
        (orb, set_features, "n = 2049", lambda: L.msf_debug_orb_set_features(h, 0, 2049, pk, pd),
         INV, set_features + ": n outside [0, 2048]"),
        (orb, set_features, "n = -1", lambda: L.msf_debug_orb_set_features(h, 0, -1, pk, pd),
         INV, set_features + ": n outside [0, 2048]"),
        (orb, set_features, "null key points with n > 0", lambda: L.msf_debug_orb_set_features(h, 0, 4, None, pd),
         INV, set_features + ": null pointer with n > 0"),
        (orb, set_features, "null descriptors with n > 0", lambda: L.msf_debug_orb_set_features(h, 0, 4, pk, None),
         INV, set_features + ": null pointer with n > 0"),
        (loftr, tail, "LoFTR handle", lambda: L.msf_debug_orb_tail(lh, 1, dA, fs, PITCH, 0, tc.ctypes.data, tl.ctypes.data, 0),
         INV, tail + ": not an ORB handle"),
        (orb, tail, "x = 30", lambda: L.msf_debug_orb_tail(h, 1, dA, fs, PITCH, 0, tc.ctypes.data, tb.ctypes.data, 0),
         INV, tail + ": position outside [31, w - 32] x [31, h - 32] of its level"),
        (orb, tail, "form = 2", lambda: L.msf_debug_orb_tail(h, 1, dA, fs, PITCH, 0, tc.ctypes.data, tl.ctypes.data, 2),
         INV, tail + ": form is 0 (dense) or 1 (streaming)"),
        (loftr, "loftr msf_match_batch_device", "n_pairs > max_batch_pairs",
         lambda: L.msf_match_batch_device(lh, P + 1, ld[0].data_ptr(), ld[1].data_ptr(), 640 * 480, 640, lo.data_ptr(), 64,
                                          ln.data_ptr(), None), INV, "n_pairs exceeds max_batch_pairs"),
        (loftr, "loftr msf_match_slots_device", "n_pairs > max_batch_pairs",
         lambda: L.msf_match_slots_device(lh, P + 1, d_s0.data_ptr(), d_s1.data_ptr(), lo.data_ptr(), 64, ln.data_ptr(), None),
         INV, "n_pairs exceeds max_batch_pairs"),
        (loftr, "msf_debug_loftr_head", "cap_per_pair = 0",
         lambda: L.msf_debug_loftr_head(lh, 1, f0, f1, lo.data_ptr(), 0, ln.data_ptr(), None), INV, bad_arg("msf_debug_loftr_head")),
        (loftr, "msf_debug_loftr_head", "misaligned features",
         lambda: L.msf_debug_loftr_head(lh, 1, f0 + 4, f1, lo.data_ptr(), 64, ln.data_ptr(), None),
         INV, "msf_debug_loftr_head: misaligned pointer"),
        (loftr, "msf_debug_loftr_transformer", "blocks past the eighth",
         lambda: L.msf_debug_loftr_transformer(lh, 1, 7, 2, f0, f1, g0, g1, None), INV, bad_arg("msf_debug_loftr_transformer")),
        (loftr, "msf_debug_loftr_transformer", "misaligned tokens",
         lambda: L.msf_debug_loftr_transformer(lh, 1, 0, 2, f0, f1, g0 + 8, g1, None),
         INV, "msf_debug_loftr_transformer: misaligned pointer"),
        (loftr, "msf_debug_loftr_backbone", "act_image past the pass",
         lambda: L.msf_debug_loftr_backbone(lh, 2, ld[0].data_ptr(), ld[1].data_ptr(), 640 * 480, 640, 4, tok[0].data_ptr(),
                                            tok[1].data_ptr(), None), INV, bad_arg("msf_debug_loftr_backbone")),
        (loftr, "msf_debug_loftr_backbone", "n above the backbone chunk",
         lambda: L.msf_debug_loftr_backbone(lh, P + 1, ld[0].data_ptr(), None, 640 * 480, 640, 0, tok[0].data_ptr(), None, None),
         INV, bad_arg("msf_debug_loftr_backbone")),
        (loftr, "msf_debug_loftr_backbone", "misaligned frames",
         lambda: L.msf_debug_loftr_backbone(lh, 1, ld[0].data_ptr() + 4, ld[1].data_ptr(), 640 * 480, 640, 0, tok[0].data_ptr(),
                                            tok[1].data_ptr(), None), INV, "msf_debug_loftr_backbone: misaligned pointer"),
        (loftr, "msf_debug_loftr_backbone", "row_stride < W",
         lambda: L.msf_debug_loftr_backbone(lh, 1, ld[0].data_ptr(), ld[1].data_ptr(), 640 * 480, 624, 0, tok[0].data_ptr(),
                                            tok[1].data_ptr(), None), INV, "row_stride < image_width"),
    ]
    for mt, entry, what, call, status, text in cases:
        label = "%s, %s" % (entry, what)
        before = _err(mt)
        assert call() == status, label
        assert _err(mt) == (before if text is None else text), label
        # (an ORB handle has no good call of the LoFTR stage entries, a LoFTR handle none of the ORB one)
        if not entry.startswith("msf_debug_orb" if mt is loftr else "msf_debug_loftr"):
            good[entry]()
    # every entry with an argument check of its own has a refusal above whose text starts with the entry's name
    named = {e.split()[-1] for _, e, _, _, _, t in cases if t and t.startswith(e.split()[-1] + ":")}
    assert named == {e.split()[-1] for e in good} - {"msf_match_pair", "msf_debug_get", "msf_stage_times"}

    # what only a handle without stored frames / map points refuses
    fresh = FeatureMatcher(0.7, W, H, max_batch_pairs=P)
    fh = fresh._h
    for call, text in (
            (lambda: L.msf_match_one_to_many(fh, 0, P, slots.ctypes.data, num.ctypes.data, None, None, 0),
             "msf_match_one_to_many: no frame was stored"),
            (lambda: L.msf_count_mappoint_matches_device(fh, P, po, cap, pn, d_s0.data_ptr(), d_s0.data_ptr(), d_mp.data_ptr(), None),
             "msf_count_mappoint_matches_device: no map slot was ever set")):
        assert call() == INV and _err(fresh) == text
    fresh.store_frame(0, a0)
    fresh.store_frame(1, b0)
    assert L.msf_match_one_to_many(fh, 0, 1, slots.ctypes.data, num.ctypes.data, num.ctypes.data, None, 0) == INV
    assert _err(fresh) == "msf_match_one_to_many: no map slot was ever set"
    assert L.msf_match_one_to_many(fh, 2 * P, 1, slots.ctypes.data, num.ctypes.data, None, None, 0) == INV
    assert _err(fresh) == "msf_match_one_to_many: bad query slot"
    n_one, _, lists = fresh.match_one_to_many(0, [1], cap=cap)
    np.testing.assert_array_equal(lists[0], orb.match_batch([a0], [b0], cap=cap)[0])
    fresh.close()

    # msf_create, the handle-less form: the text goes to msf_last_error(NULL)
    cfg = _lib.Config()
    L.msf_default_config(C.byref(cfg), _lib.MSF_KIND_ORB)
    made = C.c_void_p()
    assert L.msf_create(None, C.byref(made)) == INV and L.msf_last_error(None) == b"msf_create: null argument"
    cfg.struct_size += 8
    assert L.msf_create(C.byref(cfg), C.byref(made)) == INV and L.msf_last_error(None) == b"msf_create: struct_size mismatch"
    assert not made.value


def test_chunked_host_batch(orb, frames):
    """five pairs through the max_batch_pairs = 2 handle (chunks of 2, 2, 1) = five single-pair calls on a handle
    without the frame cache; with a capacity below the shortest list every list is the exact prefix, the counts stay
    the full counts and the status is MSF_OK"""
    from mono_slam_framework_amd.matcher import FeatureMatcher
    A, B = frames
    single = FeatureMatcher(0.7, W, H, flags=_lib.MSF_FLAG_NO_FRAME_CACHE)
    exp = [single.MatchFrames(A[i], B[i]) for i in range(5)]
    single.close()
    assert min(len(e) for e in exp) > 100
    got = orb.match_batch(list(A), list(B))
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e)
    # the single-pair call of the cached handle (count + list in one copy) gives the same list, hit or miss
    for _ in range(2):
        np.testing.assert_array_equal(orb.MatchFrames(A[4], B[4]), exp[4])
    cap = min(len(e) for e in exp) - 1
    n = 5
    IA = (_lib.Image * n)(*[_img(f) for f in A])
    IB = (_lib.Image * n)(*[_img(f) for f in B])
    out = np.zeros((n, cap), _lib.MATCH_DTYPE)
    cnt = np.zeros(n, np.int32)
    assert orb._L.msf_match_batch(orb._h, n, IA, IB, out.ctypes.data, cap, cnt.ctypes.data) == _lib.MSF_OK
    assert cnt.tolist() == [len(e) for e in exp]
    for i in range(n):
        np.testing.assert_array_equal(out[i].view(np.int32).reshape(-1, 4), exp[i][:cap])
    # and the single-pair form with such a capacity
    one = np.zeros(cap, _lib.MATCH_DTYPE)
    c1 = C.c_int32(0)
    assert orb._L.msf_match_pair(orb._h, C.byref(IA[2]), C.byref(IB[2]), one.ctypes.data, cap, C.byref(c1)) == _lib.MSF_OK
    assert c1.value == len(exp[2])
    np.testing.assert_array_equal(one.view(np.int32).reshape(-1, 4), exp[2][:cap])


def test_one_to_many_counts_only(orb, frames):
    """out = NULL: the counts come back, the status is MSF_OK; they are the counts of the call that also asks for lists"""
    A, B = frames
    for i, f in enumerate((A[0], B[0], B[1])):
        orb.store_frame(i, f)
    num, nmp, lists = orb.match_one_to_many(0, [1, 2])
    assert nmp is None and lists is None
    num2, _, lists2 = orb.match_one_to_many(0, [1, 2], cap=4096)
    assert num.tolist() == num2.tolist() == [len(x) for x in lists2]
    assert num[0] > 100
    np.testing.assert_array_equal(lists2[0], orb.match_batch([A[0]], [B[0]])[0])
    # a capacity below the count: the prefix, MSF_OK
    num3, _, lists3 = orb.match_one_to_many(0, [1, 2], cap=7)
    assert num3.tolist() == num.tolist()
    for x, y in zip(lists3, lists2):
        np.testing.assert_array_equal(x, y[:7])


def _scene(n, seed):
    """n matches under a small translation with integer noise, a fifth of them outliers"""
    r = np.random.RandomState(seed)
    p = np.stack([r.randint(20, 600, n), r.randint(20, 440, n)], 1)
    q = p + [7, -4] + r.randint(-1, 2, (n, 2))
    bad = r.rand(n) < 0.2
    q[bad] = np.stack([r.randint(0, 640, bad.sum()), r.randint(0, 480, bad.sum())], 1)
    return np.ascontiguousarray(np.concatenate([p, q], 1), np.int32)


def _translations(n_hyp, seed):
    r = np.random.RandomState(seed)
    H21 = np.tile(np.eye(3, dtype=np.float32), (n_hyp, 1, 1))
    H21[:, 0, 2] = 7 + r.uniform(-3, 3, n_hyp)
    H21[:, 1, 2] = -4 + r.uniform(-3, 3, n_hyp)
    H12 = H21.copy()
    H12[:, :2, 2] *= -1
    return H21, H12


def test_workspaces_grow_and_keep_working(orb):
    """msf_check_hypotheses, msf_render_match_image, msf_find_models, msf_reconstruct and msf_new_points each with a
    small call, one above the floor of its grow-on-demand workspace (256 hypotheses / 2048 matches; 4096 matches; 1 MiB;
    64 KiB; 64 KiB), and the small call again: the first and the third result are identical, and the large one is right"""
    # msf_check_hypotheses: 8 / 16, 300 / 2100, 8 / 16
    small_m, big_m = _scene(16, 1), _scene(2100, 2)
    small_h, big_h = _translations(8, 3), _translations(300, 4)
    first = orb.check_hypotheses(0, small_h[0], small_h[1], small_m, 1.0)
    big = orb.check_hypotheses(0, big_h[0], big_h[1], big_m, 1.0)
    third = orb.check_hypotheses(0, small_h[0], small_h[1], small_m, 1.0)
    assert first[0] >= 0 and first[2].any() and big[0] >= 0 and big[2].sum() > 1000
    _same(first, third)
    _same(first, oracle_init.find_best(0, small_h[0], small_h[1], small_m, 1.0))
    _same(big, oracle_init.find_best(0, big_h[0], big_h[1], big_m, 1.0))

    # msf_render_match_image: 10, 5000, 10 matches
    a, b = synth.synth_pair(500, W, H)
    r = np.random.RandomState(5)
    m = np.stack([r.randint(0, W, 5000), r.randint(0, H, 5000), r.randint(0, W, 5000), r.randint(0, H, 5000)], 1).astype(np.int32)
    flags = r.rand(5000) < 0.5
    img1 = orb.render_match_image(a, b, m[:10], flags[:10], ~flags[:10])
    img2 = orb.render_match_image(a, b, m, flags, ~flags)
    img3 = orb.render_match_image(a, b, m[:10], flags[:10], ~flags[:10])
    np.testing.assert_array_equal(img1, img3)
    from oracle import overlay as oracle_overlay
    np.testing.assert_array_equal(img1, oracle_overlay.create_current_match_image(a, b, m[:10], flags[:10], ~flags[:10]))
    np.testing.assert_array_equal(img2, oracle_overlay.create_current_match_image(a, b, m, flags, ~flags))

    # msf_find_models: 256 bytes of workspace per hypothesis and more, so 6000 hypotheses pass 1 MiB
    lst = _scene(300, 6)
    r = np.random.RandomState(7)
    sets_small = np.stack([r.choice(300, 8, replace=False) for _ in range(8)]).astype(np.int32)
    sets_big = np.stack([r.choice(300, 8, replace=False) for _ in range(6000)]).astype(np.int32)
    f1 = orb.find_models(lst, sets_small, 1.0)
    f2 = orb.find_models(lst, sets_big, 1.0)
    f3 = orb.find_models(lst, sets_small, 1.0)
    for name in ("H", "F"):
        for key, v in f1[name].items():
            np.testing.assert_array_equal(np.atleast_1d(v).view(np.uint8), np.atleast_1d(f3[name][key]).view(np.uint8),
                                          err_msg="%s %s" % (name, key))
        x = f2[name]
        assert x["best"] >= 0
        _same((x["best"], x["scores"], x["best_inliers"]),
              orb.check_hypotheses(0 if name == "H" else 1, x["m21"], x["m12"] if name == "H" else None, lst, 1.0))
    assert f2["H"]["best_inliers"].sum() > 200
    # the first sets of the large call are the small call's: the same models, whatever the workspace holds
    f4 = orb.find_models(lst, np.concatenate([sets_small, sets_big[:5992]]), 1.0)
    for name in ("H", "F"):
        np.testing.assert_array_equal(f4[name]["m21"][:8].view(np.uint32), f1[name]["m21"].view(np.uint32))

    # msf_reconstruct: about 30 bytes of workspace per match with points and flags wanted, so 8192 matches pass 64 KiB
    from tests import initializer_ref as ir
    c1, c3 = ir.case("planar", 1), ir.case("planar", 3)
    reps = -(-8192 // len(c3["matches"]))                # test_reconstruct_gpu.big_list: planar 3 tiled, +-1 px jitter
    big_m = np.concatenate([c3["matches"]] * reps)[:8192].copy()
    big_m[:, 2:] += np.random.RandomState(11).randint(-1, 2, (8192, 2))
    big_inl = np.concatenate([c3["H"]["inliers"]] * reps)[:8192]
    r1 = orb.reconstruct(0, c1["H"]["m21"], c1["matches"], c1["H"]["inliers"], ir.K)
    r2 = orb.reconstruct(0, c3["H"]["m21"], big_m, big_inl, ir.K)
    r3 = orb.reconstruct(0, c1["H"]["m21"], c1["matches"], c1["H"]["inliers"], ir.K)
    assert set(r1) == set(r3) and len(r1["points"]) == 300
    for key, v in r1.items():
        np.testing.assert_array_equal(np.atleast_1d(v).view(np.uint8), np.atleast_1d(r3[key]).view(np.uint8), err_msg=key)
    ir.check_result(ir.reconstruct(0, c3["H"]["m21"], big_m, big_inl), r2, big_m, big_inl, label="8192 matches")
    assert r2["ok"] == 1 and r2["cand_good"][r2["winner"]] > 4000

    # msf_new_points: 69 bytes of workspace per match, so 4096 matches pass 64 KiB
    from tests import local_mapping_ref as lm
    view1, views2, lists = lm.scene(1)
    tile = lists[0]
    n, whole, rest = len(tile), 4096 // len(tile), 4096 % len(tile)
    assert whole >= 2 and rest > 0
    big_m = np.concatenate([tile] * (whole + 1))[:4096]
    n1 = orb.new_points(tile, view1, views2[0])
    n2 = orb.new_points(big_m, view1, views2[0])
    n3 = orb.new_points(tile, view1, views2[0])
    keys = ("status", "points", "hom", "cos_parallax", "packed")
    assert set(n1) == set(keys) | {"n_new"} and 0 < n1["n_new"] < n and len(n1["status"]) == n
    assert n1["n_new"] == n3["n_new"]
    for key in keys:
        np.testing.assert_array_equal(n1[key].view(np.uint8), n3[key].view(np.uint8), err_msg=key)
    # a match's result does not depend on its neighbours in the list: every tile repeats the small call's rows
    for t in range(whole + 1):
        k = n if t < whole else rest
        for key in keys[:4]:
            np.testing.assert_array_equal(n2[key][t * n:t * n + k].view(np.uint8), n1[key][:k].view(np.uint8),
                                          err_msg="tile %d %s" % (t, key))
    accepted = np.flatnonzero(n1["status"] == 0)
    assert n1["n_new"] == len(accepted)
    assert n2["n_new"] == whole * n1["n_new"] + int((accepted < rest).sum()) == len(n2["packed"])
    # the records: in match order, the accepted matches of every tile with the small call's points
    want = np.concatenate([n1["packed"][accepted < (n if t < whole else rest)] for t in range(whole + 1)])
    at = np.concatenate([accepted[accepted < (n if t < whole else rest)] + t * n for t in range(whole + 1)])
    np.testing.assert_array_equal(n2["packed"]["match"], at)
    for axis in "xyz":
        np.testing.assert_array_equal(n2["packed"][axis].view(np.uint32), want[axis].view(np.uint32), err_msg=axis)
