"""GPU: the contract lines of include/msf_ba.h on a live handle -- a refused call leaves its reason in msf_last_error and
writes nothing, and a good call after it succeeds; an empty batch is no error."""
import ctypes as C

import numpy as np
import pytest

from tests import ba_ref as br

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.7, 640, 480)
    yield m
    m.close()


def _call(fm, sc, prm, res):
    ptr = lambda a: a.ctypes.data
    return fm._L.msf_bundle_adjust(fm._h, len(sc["cam_Tcw"]), ptr(sc["cam_Tcw"]), ptr(sc["cam_fixed"]), len(sc["points"]),
                                   ptr(sc["points"]), len(sc["edge_cam"]), ptr(sc["edge_cam"]), ptr(sc["edge_point"]),
                                   ptr(sc["edge_obs"]), None, C.byref(prm), C.byref(res))


def test_a_refused_call_and_a_good_call(fm):
    from mono_slam_framework_amd import _lib
    sc = br.scene("p63")
    status = np.full(1, -77, np.int32)
    prm = fm._ba_params(br.K, br.LOCAL_BA, 5.991, 5.991)
    res = _lib.BaResult(struct_size=C.sizeof(_lib.BaResult), status=status.ctypes.data)
    bad = _lib.BaResult(struct_size=C.sizeof(_lib.BaResult) - 8, status=status.ctypes.data)
    assert _call(fm, sc, prm, bad) == _lib.MSF_ERR_INVALID_ARG and "struct_size" in fm.last_error()
    none = _lib.BaResult(struct_size=C.sizeof(_lib.BaResult))
    assert _call(fm, sc, prm, none) == _lib.MSF_ERR_INVALID_ARG and "status" in fm.last_error()
    rounds = fm._ba_params(br.K, (0, (5, 10), (1, 0)), 5.991, 5.991)
    assert _call(fm, sc, rounds, res) == _lib.MSF_ERR_INVALID_ARG and "n_rounds" in fm.last_error()
    assert status[0] == -77
    assert _call(fm, sc, prm, res) == _lib.MSF_OK and status[0] == 2      # status alone: every other output is skipped


def test_an_empty_batch_is_no_error(fm):
    from mono_slam_framework_amd import _lib
    prm = fm._ba_params(br.K, br.LOCAL_BA, 5.991, 5.991)
    status = np.full(1, -77, np.int32)
    res = _lib.BaResult(struct_size=C.sizeof(_lib.BaResult), status=status.ctypes.data)
    assert fm._L.msf_bundle_adjust_device(fm._h, 0, None, None, None, None, None, None, None, 0, 0, 0, 64, None,
                                          C.byref(prm), C.byref(res), None) == _lib.MSF_OK
    assert fm._L.msf_bundle_adjust_device(fm._h, 1, None, None, None, None, None, None, None, 0, 0, 0, 65, None,
                                          C.byref(prm), C.byref(res), None) == _lib.MSF_ERR_INVALID_ARG
    assert "max_free_cams" in fm.last_error() and status[0] == -77
