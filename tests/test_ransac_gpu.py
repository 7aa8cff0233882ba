"""GPU: Initializer::FindHomography + FindFundamental with the hypotheses made on the device (msf_find_models,
msf_find_models_device; csrc/ransac_kernels.hip) against tests/ransac_ref.py.

Scenes: a planar scene and a two-view 3-D scene, 300 integer-pixel matches at 640 x 480, 0.5 px noise, 30 % random outliers,
200 hypotheses, seeds 1-3.  Bars, eps = 2^-24:
  1 Normalize      T1, T2 bit-identical to the sequential f32 restatement
  2 null vector    min |h -+ v| <= 16 eps s1 / (s8 - s9) and |A h| <= s9 + 32 eps s1 against a float64 SVD of the A built
                   from the device's own T and points (a bound above 0.05 is uninformative: at most 2 % of a scene)
  3 rank-2 step    |Fn - P2(Fpre)|_F <= 16 eps |Fpre|_F and s3(Fn) <= 16 eps s1(Fn), P2 in float64 on the device's null_vec
  4 denormalise    |M21 - ref| <= 16 eps |T2^-1 or T2'| |Mn| |T1| and |H21 H12 - I| <= 16 eps |H21| |H12|, componentwise
  5 fusion         scores, best, best_inliers bit-identical to check_hypotheses and to the oracle on the returned matrices
  6 end to end     best score >= (1 - m) x the best score of the float64-solved hypotheses of the same sets (oracle-scored);
                   m = 7.0e-06 = twice the CPU spread 3.444e-06 between the float64 solve and a numpy float32 solve
                   (with only the DLT SVDs in f32: 6.565e-07; tests/ransac_ref.py, asserted by test_ransac_ref.py);
                   the kept inlier set holds >= 90 % of the planted inliers the reference's kept set holds
  7 batch          64 lists (lengths 0, 7, 8, 9, 255, 2049, the capacity, n_out = -1 among them): valid sets, replay through
                   find_models bit-identical, no dependence on the batch, best = -1 below 8 matches, same seed same sets,
                   lists straight from match_batch_device
  8 degenerate     all x equal, collinear points, repeated matches, n_hyp = 300, the error paths"""
import numpy as np
import pytest

from oracle import initializer as oracle_init
from tests import ransac_ref as rr
from tests.test_initializer_gpu import _same

pytestmark = pytest.mark.gpu

CASES = [(k, s) for k in rr.SCENES for s in rr.SEEDS]


@pytest.fixture(scope="module")
def fm():
    from mono_slam_framework_amd.matcher import FeatureMatcher
    m = FeatureMatcher(0.7, rr.W, rr.H)
    yield m
    m.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    """bit for bit, a NaN matching any NaN"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(a)
    np.testing.assert_array_equal(_bits(a)[ok], _bits(b)[ok])


@pytest.mark.parametrize("kind,seed", CASES)
def test_solve_against_float64(fm, kind, seed):
    """bars 1-4"""
    m, _ = rr.scene(kind, seed)
    sets = rr.draw_sets(len(m), rr.N_HYP, seed)
    got = fm.find_models(m, sets, 1.0)
    n1, T1 = rr.normalize_seq(m[:, :2])
    n2, T2 = rr.normalize_seq(m[:, 2:])
    for r in got.values():
        np.testing.assert_array_equal(_bits(r["T1"]), _bits(T1))
        np.testing.assert_array_equal(_bits(r["T2"]), _bits(T2))
    # T is bit-identical, so the restatement's points are the device's own (x - mean) * s in f32
    for model, name in ((0, "H"), (1, "F")):
        r = got[name]
        rr.check_solver_output(sets, model, n1, n2, T1, T2, r["null_vec"].reshape(-1, 9), r["m21"].reshape(-1, 9),
                               r["m12"].reshape(-1, 9) if model == 0 else None,
                               r["fn"].reshape(-1, 9) if model == 1 else None, label="gpu %s seed %d" % (kind, seed))


@pytest.mark.parametrize("kind,seed", CASES)
def test_fusion_is_bit_exact(fm, kind, seed):
    """bar 5"""
    m, _ = rr.scene(kind, seed)
    sets = rr.draw_sets(len(m), rr.N_HYP, seed)
    for sigma in (1.0, 2.5):
        got = fm.find_models(m, sets, sigma)
        h, f = got["H"], got["F"]
        mine = (h["best"], h["scores"], h["best_inliers"])
        _same(mine, fm.check_hypotheses(0, h["m21"], h["m12"], m, sigma))
        _same(mine, oracle_init.find_best(0, h["m21"], h["m12"], m, sigma))
        mine = (f["best"], f["scores"], f["best_inliers"])
        _same(mine, fm.check_hypotheses(1, f["m21"], None, m, sigma))
        _same(mine, oracle_init.find_best(1, f["m21"], None, m, sigma))
        assert h["best"] >= 0 and f["best"] >= 0


@pytest.mark.parametrize("kind,seed", CASES)
def test_end_to_end(fm, kind, seed):
    """bar 6 (figures in the module docstring)"""
    m, bad = rr.scene(kind, seed)
    sets = rr.draw_sets(len(m), rr.N_HYP, seed)
    model = rr.model_of(kind)
    got = fm.find_models(m, sets, 1.0)["H" if model == 0 else "F"]
    H21, H12, F21 = rr.solve64(m, sets)
    rb, rs, rinl = oracle_init.find_best(model, H21 if model == 0 else F21, H12 if model == 0 else None, m, 1.0)
    assert rb >= 0 and got["best"] >= 0
    mine, ref = float(got["scores"][got["best"]]), float(rs[rb])
    planted = rinl & ~bad
    kept = (got["best_inliers"] & planted).sum() / planted.sum()
    print("%s seed %d: best score %.4f (hyp %d), reference %.4f (hyp %d), relative deficit %.3e (margin %.1e); "
          "planted inliers of the reference kept: %.3f" % (kind, seed, mine, got["best"], ref, rb, (ref - mine) / ref,
                                                           rr.MARGIN, kept))
    assert mine >= (1 - rr.MARGIN) * ref
    assert kept >= 0.9


# ---- batch ----
CAP = 4096
LENGTHS = [0, 7, 8, 9, 255, 2049, CAP, -1]


def _batch_lists(n_lists=64, seed=5):
    """lists of scene matches (tiled to the length) with the lengths of LENGTHS first, then random ones"""
    r = np.random.RandomState(seed)
    lens = LENGTHS + [int(v) for v in r.randint(8, 600, n_lists - len(LENGTHS))]
    out = np.zeros((n_lists, CAP, 4), np.int32)
    for i, n in enumerate(lens):
        k = max(n, 0)
        base, _ = rr.scene(rr.SCENES[i % 2], 1 + i % 3, n=max(k, 1))
        out[i, :k] = base[:k]
        out[i, k:] = r.randint(0, 400, (CAP - k, 4))                    # beyond the list: must never be read
    return out, np.array(lens, np.int32)


def _to_host(res):
    return {k: ({kk: vv.cpu().numpy() for kk, vv in v.items()} if isinstance(v, dict) else v.cpu().numpy())
            for k, v in res.items()}


def _check_list_against_replay(fm, lst, n, batch, i, n_hyp):
    sets = batch["sets"][i]
    assert ((sets >= 0) & (sets < n)).all()
    assert all(len(set(s)) == 8 for s in sets.tolist())
    single = fm.find_models(lst[:n], sets, 1.0)
    for name in ("H", "F"):
        b, s = batch[name], single[name]
        for key in ("m21", "null_vec", "scores", "T1", "T2", "m12" if name == "H" else "fn"):
            _same_bits(b[key][i], s[key])
        assert int(b["best"][i]) == s["best"]
        np.testing.assert_array_equal(b["best_inliers"][i, :n].astype(bool), s["best_inliers"])
        assert not b["best_inliers"][i, n:].any()


def test_batch(fm):
    """bar 7"""
    import torch
    lists, lens = _batch_lists()
    d_m = torch.from_numpy(lists).cuda()
    d_n = torch.from_numpy(lens).cuda()
    n_hyp = 200
    batch = _to_host(fm.find_models_device(d_m, d_n, n_hyp=n_hyp, seed=77))
    again = _to_host(fm.find_models_device(d_m, d_n, n_hyp=n_hyp, seed=77))
    other = _to_host(fm.find_models_device(d_m, d_n, n_hyp=n_hyp, seed=78))
    np.testing.assert_array_equal(batch["sets"], again["sets"])
    assert (batch["sets"][8] != other["sets"][8]).any()
    for name in ("H", "F"):
        _same_bits(batch[name]["scores"], again[name]["scores"])
        np.testing.assert_array_equal(batch[name]["best"], again[name]["best"])
    kept = 0
    for i, n in enumerate(lens.tolist()):
        if n < 8:
            for name in ("H", "F"):
                assert batch[name]["best"][i] == -1 and not batch[name]["best_inliers"][i].any()
                assert not batch[name]["scores"][i].any()
            continue
        _check_list_against_replay(fm, lists[i], n, batch, i, n_hyp)
        kept += batch["H"]["best"][i] >= 0 or batch["F"]["best"][i] >= 0
    assert kept >= 50                                                     # the scenes have a model to find
    # a list alone equals the list in the batch (the generator is keyed by the list's index: pass the sets)
    for i in (2, 5, 6, 20):
        alone = _to_host(fm.find_models_device(d_m[:i + 1], d_n[:i + 1], n_hyp=n_hyp, seed=77))
        for name in ("H", "F"):
            for key in ("m21", "scores", "best", "best_inliers"):
                _same_bits(alone[name][key][i].astype(np.float32), batch[name][key][i].astype(np.float32))
        np.testing.assert_array_equal(alone["sets"][i], batch["sets"][i])


def test_batch_from_match_batch_device(fm):
    """the lists straight from match_batch_device on synthetic pairs"""
    import torch
    from mono_slam_framework_amd import synth
    from mono_slam_framework_amd.matcher import FeatureMatcher
    n = 4
    bm = FeatureMatcher(0.7, rr.W, rr.H, max_batch_pairs=n)
    pairs = [synth.synth_pair(300 + i, rr.W, rr.H, shift=(11 + 3 * i, -7 + 2 * i)) for i in range(n)]
    d_a = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    d_b = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    d_out = torch.zeros((n, 2048, 4), dtype=torch.int32, device="cuda")
    d_n = torch.zeros((n,), dtype=torch.int32, device="cuda")
    bm.match_batch_device(d_a, d_b, d_out, d_n)
    res = _to_host(bm.find_models_device(d_out, d_n, n_hyp=200, seed=3))
    lens, lists = d_n.cpu().numpy(), d_out.cpu().numpy()
    assert (lens > 100).all()
    for i in range(n):
        _check_list_against_replay(bm, lists[i], int(lens[i]), res, i, 200)
        h = res["H"]
        assert h["best"][i] >= 0 and h["best_inliers"][i].sum() > 0.5 * lens[i]     # a translation is a homography
    bm.close()


def test_degenerate_inputs_and_errors(fm):
    """bar 8"""
    from mono_slam_framework_amd.matcher import MsfError
    r = np.random.RandomState(4)
    m, _ = rr.scene("planar", 1)
    sets = rr.draw_sets(len(m), 200, 1)
    # all x equal in image 1: mean deviation 0, infinite scale, NaN models, NaN scores, nothing kept
    flat = m.copy()
    flat[:, 0] = 123
    got = fm.find_models(flat, sets, 1.0)
    for name in ("H", "F"):
        assert got[name]["best"] == -1 and not got[name]["best_inliers"].any()
        assert np.isnan(got[name]["scores"]).all() and not np.isfinite(got[name]["m21"]).any()
        assert np.isinf(got[name]["T1"][0, 0])
    # eight collinear points; one match repeated in a set's eight places (as repeated list entries); 300 hypotheses
    line = m.copy()
    line[:8, :2] = np.stack([np.arange(8) * 10 + 50, np.arange(8) * 20 + 40], 1)
    line[:8, 2:] = line[:8, :2] + 5
    rep = m.copy()
    rep[:8] = rep[0]
    first = np.tile(np.arange(8, dtype=np.int32), (300, 1))
    first[1:] = rr.draw_sets(len(m), 299, 2)
    for lst in (line, rep):
        got = fm.find_models(lst, first, 1.0)
        for name in ("H", "F"):
            mine = (got[name]["best"], got[name]["scores"], got[name]["best_inliers"])
            _same(mine, oracle_init.find_best(0 if name == "H" else 1, got[name]["m21"],
                                              got[name]["m12"] if name == "H" else None, lst, 1.0))
            assert got[name]["best"] >= 0                                  # the other 299 sets find the plane
    # no hypotheses: nothing kept
    got = fm.find_models(m, np.zeros((0, 8), np.int32), 1.0)
    assert got["H"]["best"] == -1 and got["F"]["best"] == -1 and not got["H"]["best_inliers"].any()
    got = fm.find_models(np.zeros((0, 4), np.int32), np.zeros((0, 8), np.int32), 1.0)
    assert got["H"]["best"] == -1
    # error paths
    with pytest.raises(MsfError):
        fm.find_models(m[:7], sets % 7, 1.0)                               # fewer than 8 matches
    with pytest.raises(MsfError):
        fm.find_models(np.zeros((8193, 4), np.int32), sets, 1.0)           # more than 8192
    bad = sets.copy()
    bad[17, 3] = len(m)
    with pytest.raises(MsfError):
        fm.find_models(m, bad, 1.0)                                        # index outside the list
    bad[17, 3] = -1
    with pytest.raises(MsfError):
        fm.find_models(m, bad, 1.0)
    import ctypes as C
    from mono_slam_framework_amd import _lib
    res = _lib.RansacResult(struct_size=C.sizeof(_lib.RansacResult))      # best missing
    mm = np.ascontiguousarray(m, np.int32)
    assert fm._L.msf_find_models(fm._h, len(mm), mm.ctypes.data, 200, sets.ctypes.data, 1.0, C.byref(res),
                                 C.byref(res)) == _lib.MSF_ERR_INVALID_ARG
    assert fm._L.msf_find_models(fm._h, len(mm), mm.ctypes.data, 200, sets.ctypes.data, 1.0, None,
                                 None) == _lib.MSF_ERR_INVALID_ARG
    batch = _lib.RansacBatch(struct_size=0)
    assert fm._L.msf_find_models_device(fm._h, 1, 1, 16, 1, 200, 0, 1.0, C.byref(batch), None) == _lib.MSF_ERR_INVALID_ARG
    # the largest list the scorer takes, and a LoFTR handle is as good as an ORB one
    big = np.concatenate([m] * 28)[:8192]
    got = fm.find_models(big, sets, 1.0)
    _same((got["H"]["best"], got["H"]["scores"], got["H"]["best_inliers"]),
          oracle_init.find_best(0, got["H"]["m21"], got["H"]["m12"], big, 1.0))


def test_loftr_handle_gives_the_same(fm):
    from mono_slam_framework_amd.matcher import DNNFeatureMatcher
    dm = DNNFeatureMatcher(threshold=0.15)
    m, _ = rr.scene("two_view", 2)
    sets = rr.draw_sets(len(m), 200, 2)
    a, b = fm.find_models(m, sets, 1.0), dm.find_models(m, sets, 1.0)
    for name in ("H", "F"):
        _same_bits(a[name]["m21"], b[name]["m21"])
        _same_bits(a[name]["scores"], b[name]["scores"])
        assert a[name]["best"] == b[name]["best"]
    dm.close()
