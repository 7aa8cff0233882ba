"""The contract of include/msf_initializer.h (msf_reconstruct, msf_reconstruct_device; bodies in csrc/abi_initializer.cpp), as
test_abi_contract_gpu.py keeps it for msf_abi.h: the header is plain C99, every name it declares is exported and bound,
the ctypes structs have the C sizes (CPU part, not marked gpu); a null handle, every refusal with its text, and a good
call after each refusal (GPU part).  The entry points of msf_initializer.h are listed here and in
_lib.INITIALIZER_SYMBOLS, not in _lib.ABI_SYMBOLS: msf_abi.h and MSF_ABI_VERSION stay what they are."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mono_slam_framework_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = _lib.MSF_ERR_INVALID_ARG
gpu = pytest.mark.gpu


def _declared():
    hdr = open(os.path.join(ROOT, "include", "msf_initializer.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(msf_[a-z_0-9]+)\s*\(", hdr)))


# ---- CPU ----
def test_header_is_plain_c99(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "msf_initializer.h"\n'
                   "int main(void){ msf_motion_params p; msf_motion_result r; p.struct_size = sizeof p; r.ok = 0;\n"
                   "  return msf_reconstruct(0, MSF_MODEL_HOMOGRAPHY, 0, 0, 0, 0, &p, &r) + msf_initializer_version()\n"
                   "         + msf_reconstruct_device(0, 0, 0, 1, 0, 1, 0, &p, &r, 0) + MSF_INITIALIZER_VERSION; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


def test_declared_names_are_exported_and_bound():
    L = _lib.load()
    names = _declared()
    assert names == sorted(_lib.INITIALIZER_SYMBOLS) == ["msf_initializer_version", "msf_reconstruct",
                                                         "msf_reconstruct_device"]
    for n in names:
        assert hasattr(L, n), n
    assert not set(names) & set(_lib.ABI_SYMBOLS)
    assert L.msf_initializer_version() == 1 and L.msf_abi_version() == 4


def test_struct_sizes_match_c(tmp_path):
    src = tmp_path / "s.c"
    exe = tmp_path / "s"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msf_initializer.h"\n'
                   'int main(void){ printf("%zu %zu %zu %zu %zu\\n", sizeof(msf_motion_params), sizeof(msf_motion_result),\n'
                   "  offsetof(msf_motion_params, sigma), offsetof(msf_motion_result, n_cand), offsetof(msf_motion_result, winner));"
                   " return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_lib.MotionParams), C.sizeof(_lib.MotionResult), _lib.MotionParams.sigma.offset,
                   _lib.MotionResult.n_cand.offset, _lib.MotionResult.winner.offset]
    assert C.sizeof(_lib.MotionParams) == 56 and C.sizeof(_lib.MotionResult) == 104


# ---- GPU ----
@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    from tests import ransac_ref as rr
    m = FeatureMatcher(0.7, rr.W, rr.H)
    yield m
    m.close()


@pytest.fixture(scope="module")
def case():
    from tests import initializer_ref as ir
    c = ir.case("planar", 1)
    return dict(m=np.ascontiguousarray(c["matches"], np.int32), inl=np.ascontiguousarray(c["H"]["inliers"], np.uint8),
                m21=np.ascontiguousarray(c["H"]["m21"], np.float32).reshape(9), K=ir.K)


def _err(m):
    return m._L.msf_last_error(m._h).decode()


def _params(K, sigma=1.0):
    p = _lib.MotionParams(struct_size=C.sizeof(_lib.MotionParams), sigma=sigma, min_triangulated=50, min_parallax=1.0)
    p.K[:] = [float(v) for v in np.asarray(K, np.float32).reshape(9)]
    return p


def _result(ok):
    return _lib.MotionResult(struct_size=C.sizeof(_lib.MotionResult), ok=ok.ctypes.data)


def _good_host_call(fm, case):
    got = fm.reconstruct(0, case["m21"], case["m"], case["inl"], case["K"])
    assert got["ok"] == 1 and got["model"] == 0 and got["triangulated"].sum() > 150
    return got


@gpu
def test_null_handle(fm, case):
    L = fm._L
    cfg = _lib.Config()
    L.msf_default_config(C.byref(cfg), _lib.MSF_KIND_ORB)
    cfg.struct_size = 4
    out = C.c_void_p()
    assert L.msf_create(C.byref(cfg), C.byref(out)) == INV and not out.value
    before = L.msf_last_error(None)
    ok = np.zeros(1, np.int32)
    prm, res = _params(case["K"]), _result(ok)
    assert L.msf_reconstruct(None, 0, case["m21"].ctypes.data, len(case["m"]), case["m"].ctypes.data,
                             case["inl"].ctypes.data, C.byref(prm), C.byref(res)) == INV
    assert L.msf_reconstruct_device(None, 1, None, 16, None, 1, None, C.byref(prm), C.byref(res), None) == INV
    assert L.msf_last_error(None) == before == b"msf_create: struct_size mismatch"


@gpu
def test_reconstruct_refusals(fm, case):
    L, h = fm._L, fm._h
    first = _good_host_call(fm, case)
    ok = np.zeros(1, np.int32)
    m, inl, m21, n = case["m"].ctypes.data, case["inl"].ctypes.data, case["m21"].ctypes.data, len(case["m"])
    prm, res = _params(case["K"]), _result(ok)
    short_prm, short_res = _params(case["K"]), _result(ok)
    short_prm.struct_size -= 4
    short_res.struct_size -= 8
    no_ok = _lib.MotionResult(struct_size=C.sizeof(_lib.MotionResult))
    nan_k, sing_k, inf_k = case["K"].copy(), case["K"].copy(), case["K"].copy()
    nan_k[1, 1], sing_k[0, 0], inf_k[0, 2] = np.nan, 0.0, np.inf
    big = np.zeros((8193, 4), np.int32)
    big_inl = np.ones(8193, np.uint8)
    R = C.byref
    refusals = [
        (lambda: L.msf_reconstruct(h, 0, m21, n, m, inl, R(prm), R(short_res)), "msf_reconstruct: out is NULL or out->struct_size"),
        (lambda: L.msf_reconstruct(h, 0, m21, n, m, inl, R(prm), None), "msf_reconstruct: out is NULL or out->struct_size"),
        (lambda: L.msf_reconstruct(h, 0, m21, n, m, inl, R(prm), R(no_ok)), "msf_reconstruct: a required pointer is NULL"),
        (lambda: L.msf_reconstruct(h, 0, None, n, m, inl, R(prm), R(res)), "msf_reconstruct: a required pointer is NULL"),
        (lambda: L.msf_reconstruct(h, 0, m21, n, None, inl, R(prm), R(res)), "msf_reconstruct: a required pointer is NULL"),
        (lambda: L.msf_reconstruct(h, 0, m21, n, m, None, R(prm), R(res)), "msf_reconstruct: a required pointer is NULL"),
        (lambda: L.msf_reconstruct(h, 0, m21, 8193, big.ctypes.data, big_inl.ctypes.data, R(prm), R(res)),
         "msf_reconstruct: n_matches outside [0, 8192]"),
        (lambda: L.msf_reconstruct(h, 0, m21, -1, m, inl, R(prm), R(res)), "msf_reconstruct: n_matches outside [0, 8192]"),
        (lambda: L.msf_reconstruct(h, 2, m21, n, m, inl, R(prm), R(res)), "msf_reconstruct: model is neither"),
        (lambda: L.msf_reconstruct(h, -1, m21, n, m, inl, R(prm), R(res)), "msf_reconstruct: model is neither"),
        (lambda: L.msf_reconstruct(h, 0, m21, n, m, inl, None, R(res)), "msf_reconstruct: params is NULL"),
        (lambda: L.msf_reconstruct(h, 0, m21, n, m, inl, R(short_prm), R(res)), "msf_reconstruct: params->struct_size"),
        (lambda: L.msf_reconstruct(h, 0, m21, n, m, inl, R(_params(nan_k)), R(res)), "msf_reconstruct: K, sigma and min_parallax must be finite"),
        (lambda: L.msf_reconstruct(h, 0, m21, n, m, inl, R(_params(inf_k)), R(res)), "msf_reconstruct: K, sigma and min_parallax must be finite"),
        (lambda: L.msf_reconstruct(h, 0, m21, n, m, inl, R(_params(sing_k)), R(res)), "msf_reconstruct: K is singular"),
    ]
    for call, text in refusals:
        ok[0] = 7
        assert call() == INV, text
        assert _err(fm).startswith(text), (_err(fm), text)
        assert ok[0] == 7                                         # a refused call writes nothing
        again = _good_host_call(fm, case)                         # and the handle works afterwards, with the same answer
        np.testing.assert_array_equal(again["points"].view(np.uint32), first["points"].view(np.uint32))
        assert again["winner"] == first["winner"]


@gpu
def test_reconstruct_device_refusals(fm, case):
    import torch
    L, h = fm._L, fm._h
    lists = torch.from_numpy(np.stack([case["m"], case["m"][::-1].copy()])).cuda()
    lens = torch.tensor([300, 300], dtype=torch.int32, device="cuda")
    found = fm.find_models_device(lists, lens, n_hyp=64, seed=1)
    first = {k: v.cpu().numpy() for k, v in fm.reconstruct_device(lists, lens, found, case["K"]).items()}
    assert first["ok"].tolist() == [1, 1]

    def batch(drop=None, size=None):
        b = _lib.RansacBatch(struct_size=C.sizeof(_lib.RansacBatch) if size is None else size, sets=found["sets"].data_ptr())
        for name, r in (("H", b.homography), ("F", b.fundamental)):
            r.struct_size = C.sizeof(_lib.RansacResult)
            for k in ("m21", "scores", "best", "best_inliers"):
                if (name, k) != drop:
                    setattr(r, k, found[name][k].data_ptr())
        return b

    d_ok = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    res = _lib.MotionResult(struct_size=C.sizeof(_lib.MotionResult), ok=d_ok.data_ptr())
    short_res = _lib.MotionResult(struct_size=8, ok=d_ok.data_ptr())
    no_ok = _lib.MotionResult(struct_size=C.sizeof(_lib.MotionResult))
    prm = _params(case["K"])
    sing_k = case["K"].copy()
    sing_k[1, 1] = 0
    dm, dn, R = lists.data_ptr(), lens.data_ptr(), C.byref
    whole = batch()
    name = "msf_reconstruct_device: "
    refusals = [
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, R(whole), R(prm), R(short_res), None), name + "out is NULL or out->struct_size"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, R(whole), R(prm), None, None), name + "out is NULL or out->struct_size"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, None, R(prm), R(res), None), name + "found is NULL or found->struct_size"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, R(batch(size=16)), R(prm), R(res), None), name + "found is NULL or found->struct_size"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, R(whole), R(prm), R(no_ok), None), name + "a required pointer is NULL"),
        (lambda: L.msf_reconstruct_device(h, 2, None, 300, dn, 64, R(whole), R(prm), R(res), None), name + "a required pointer is NULL"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, None, 64, R(whole), R(prm), R(res), None), name + "a required pointer is NULL"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, R(batch(("F", "best_inliers"))), R(prm), R(res), None), name + "a required pointer is NULL"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, R(batch(("H", "scores"))), R(prm), R(res), None), name + "a required pointer is NULL"),
        (lambda: L.msf_reconstruct_device(h, 65536, dm, 300, dn, 64, R(whole), R(prm), R(res), None), name + "n_lists outside [0, 65535]"),
        (lambda: L.msf_reconstruct_device(h, -1, dm, 300, dn, 64, R(whole), R(prm), R(res), None), name + "n_lists outside [0, 65535]"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 0, dn, 64, R(whole), R(prm), R(res), None), name + "cap_per_pair < 1 or n_hyp outside"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 0, R(whole), R(prm), R(res), None), name + "cap_per_pair < 1 or n_hyp outside"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, R(whole), None, R(res), None), name + "params is NULL"),
        (lambda: L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, R(whole), R(_params(sing_k)), R(res), None), name + "K is singular"),
    ]
    for call, text in refusals:
        assert call() == INV, text
        assert _err(fm).startswith(text), (_err(fm), text)
        torch.cuda.synchronize()
        assert d_ok.tolist() == [7, 7]                            # a refused call writes nothing
        again = {k: v.cpu().numpy() for k, v in fm.reconstruct_device(lists, lens, found, case["K"]).items()}
        for k in first:
            np.testing.assert_array_equal(again[k], first[k], err_msg=k)
    # only ok given: everything else lives in the handle's workspace; no lists: nothing to do
    assert L.msf_reconstruct_device(h, 2, dm, 300, dn, 64, R(whole), R(prm), R(res), None) == 0
    assert d_ok.tolist() == [1, 1]
    assert L.msf_reconstruct_device(h, 0, None, 300, None, 64, R(whole), R(prm), R(res), None) == 0
