"""GPU: every *_device wrapper of mono_slam_framework_amd/geometry.py once with every array, once without diagnostics
where it has that switch, and once into an `out=` dict, on the smallest inputs each call accepts.  Only the layout is
asserted -- key set, order, shape, dtype and device equal what the CPU layer (results.alloc on torch's CPU device, pinned
by tests/test_binding_results.py) says, and `out=` comes back as the same object with the same keys; the values are
checked by the tests of each call."""
import numpy as np
import pytest
import torch

from mono_slam_framework_amd import _lib, results
from tests import ba_ref as br
from tests import initializer_ref as ir
from tests import local_mapping_ref as lm
from tests import pose_ref
from tests import tracking_host as th
from tests import tracking_ref as tr

pytestmark = pytest.mark.gpu
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.8, 640, 480, max_batch_pairs=8)
    yield m
    m.close()


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()


def same_layout(got, expect, label):
    """got: a wrapper's dict of CUDA tensors; expect: the CPU layer's dict for the same call"""
    assert list(got) == list(expect), label
    for k, e in expect.items():
        g = got[k]
        assert g.is_cuda and g.is_contiguous() and tuple(g.shape) == tuple(e.shape) and g.dtype == e.dtype, (label, k)


def three_ways(call, shapes, family=None, table=None, flat=(), label=""):
    """call(**kw) -> the wrapper's dict, with kw of diagnostics= and out="""
    cuda = torch.device("cuda", torch.cuda.current_device())
    switch = family is not None
    same_layout(call(diagnostics=True) if switch else call(), results.alloc(shapes, CPU, flat=flat), label + " whole")
    less = results.left_out(family, table) if switch else set()
    if switch:
        assert less
        same_layout(call(diagnostics=False), results.alloc(shapes, CPU, less, flat=flat), label + " no diagnostics")
    for leave_out in ((), less) if switch else ((),):
        out = results.alloc(shapes, cuda, leave_out, flat=flat)
        keys, tensors = list(out), list(out.values())
        got = call(out=out)
        assert got is out and list(out) == keys and all(a is b for a, b in zip(out.values(), tensors)), label + " out="
    torch.cuda.synchronize()


def test_pnp_and_pose(fm):
    L, cap, its, recs = 2, 8, 8, 2
    sc = pose_ref.scene("base", 1, cap)
    p3 = dev(np.stack([sc["p3d"], sc["p3d"]]), np.float32)
    p2 = dev(np.stack([sc["p2d"], sc["p2d"]]), np.float32)
    d_n = torch.tensor([8, -1], dtype=torch.int32, device="cuda")
    t0 = dev(np.stack([sc["Tcw0"], sc["Tcw0"]]), np.float32)
    three_ways(lambda **kw: fm.pnp_ransac_device(p3, p2, d_n, sc["K"], 4, its, max_records=recs, seed=7, **kw),
               _lib.pnp_shapes(L, its, recs, cap), "pnp", _lib.PNP_ARRAYS, label="pnp")
    three_ways(lambda **kw: fm.pose_optimize_device(p3, p2, d_n, sc["K"], t0, **kw), _lib.pose_shapes(L, cap), "pose",
               _lib.POSE_ARRAYS, label="pose")


def test_both_bundle_adjustments(fm):
    sc = br.scene("initial")   # two cameras, 40 points: the smallest of br.SCENES
    nc, npt, ne = len(sc["cam_Tcw"]), len(sc["points"]), len(sc["edge_cam"])
    t = [dev(sc["cam_Tcw"].reshape(-1, 12), np.float32), dev(sc["cam_fixed"], np.uint8), dev(sc["points"].reshape(-1, 3), np.float32),
         dev(sc["edge_cam"], np.int32), dev(sc["edge_point"], np.int32), dev(sc["edge_obs"].reshape(-1, 2), np.float32)]
    problems = torch.tensor([[nc, npt, ne, 0, 0, 0]], dtype=torch.int32, device="cuda")
    shapes = _lib.ba_shapes(1, nc, npt, ne)
    three_ways(lambda **kw: fm.bundle_adjust_device(problems, *t, br.K, schedule=br.INITIAL_BA, **kw), shapes, "ba",
               _lib.BA_ARRAYS, label="ba")
    three_ways(lambda **kw: fm.global_bundle_adjust_device(*t, br.K, schedule=br.INITIAL_BA, **kw), shapes, "ba",
               _lib.BA_ARRAYS, label="global ba")


def test_frustum_and_claims(fm):
    lmap, prm, lists, n_out = tr.tied_case()
    n_points, n_kf, cap, corr_cap = len(lmap["points"]), len(lists), 16, 100
    dmap = fm.local_map_to_device(lmap)
    three_ways(lambda **kw: fm.frustum_device(dmap, tr.view_of(prm), prm["Ow"], tr.bounds_of(prm), float(prm["cos_limit"]), **kw),
               _lib.tracking_shapes(_lib.FRUSTUM_ARRAYS, n_points, n_kf, 1, 0), label="frustum")
    d_m, d_n = dev(th.pad_lists(lists, cap), np.int32), dev(n_out, np.int32)
    d_g = torch.ones(n_kf, dtype=torch.uint8, device="cuda")
    shapes = _lib.tracking_shapes(_lib.CLAIM_ARRAYS, n_points, n_kf, cap, corr_cap)
    three_ways(lambda **kw: fm.claim_points_device(dmap, d_m, d_n, d_g, corr_cap, **kw), shapes, flat=("claims",), label="claims")
    claims = fm.claim_points_device(dmap, d_m, d_n, d_g, corr_cap)["claims"]
    assert tuple(claims.shape) == (n_kf * cap, 4) and claims.dtype == torch.int32


def test_initializer_chain_and_new_points(fm):
    L, cap, n_hyp = 2, 16, 8
    m = ir.case("planar", 3)["matches"]
    d_m, d_n = dev(np.stack([m[:cap], m[cap:2 * cap]]), np.int32), torch.full((L,), cap, dtype=torch.int32, device="cuda")
    found = fm.find_models_device(d_m, d_n, n_hyp=n_hyp, seed=5)
    expect = results.alloc({"sets": ((L, n_hyp, 8), "int32")}, CPU)
    expect.update(results.alloc_ransac(_lib.ransac_shapes(L, n_hyp, cap), CPU))
    assert list(found) == list(expect) == ["sets", "H", "F"]
    same_layout({"sets": found["sets"]}, {"sets": expect["sets"]}, "sets")
    for model in "HF":
        same_layout(found[model], expect[model], "find_models " + model)
    same_layout(fm.reconstruct_device(d_m, d_n, found, ir.K), results.alloc(_lib.list_shapes(_lib.MOTION_ARRAYS, L, cap), CPU),
                "reconstruct")
    v1, v2, _ = lm.handmade()
    views = lambda v: dev(np.concatenate([np.asarray(v, lm.VIEW_DTYPE).reshape(-1)] * L).view(np.uint8).reshape(L, 64), np.uint8)
    d_v1, d_v2 = views(v1), views(v2)
    three_ways(lambda **kw: fm.new_points_device(d_m, d_n, d_v1, d_v2, **kw), _lib.list_shapes(_lib.NEW_POINTS_ARRAYS, L, cap),
               label="new points")
    packed = fm.new_points_device(d_m, d_n, d_v1, d_v2)["packed"]
    assert tuple(packed.shape) == (L, cap, 4) and packed.dtype == torch.int32
    torch.cuda.synchronize()
