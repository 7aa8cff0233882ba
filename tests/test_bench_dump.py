"""bench.py --dump-outputs on host tensors: the files hold what msf_pack_matches_device hands a caller (packed records,
offsets, counts) exactly, in float32 / float64; above the size budget a seeded sample of whole pairs is written, the
same pairs on every run, and named in sample_pairs.npy."""
import numpy as np
import torch


def _step(P=12, cap=16, seed=3):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, cap + 1, size=P).astype(np.int32)
    cnt[4] = -1                                               # an overflowed pair packs no records
    offs = np.concatenate([[0], np.cumsum(np.maximum(cnt, 0))]).astype(np.int32)
    packed = rng.integers(0, 1280, size=(P * cap, 4)).astype(np.int32)
    return torch.from_numpy(packed), torch.from_numpy(offs), torch.from_numpy(cnt)


def _load(d, name):
    return np.load(str(d / (name + ".npy")))


def test_dump_holds_the_packed_lists_exactly(tmp_path):
    import bench
    packed, offs, cnt = _step()
    bench.dump_outputs(str(tmp_path), packed, offs, cnt, 12)
    m, o, c = _load(tmp_path, "matches"), _load(tmp_path, "offsets"), _load(tmp_path, "counts")
    assert m.dtype == np.float32 and o.dtype == np.float64 and c.dtype == np.float64
    np.testing.assert_array_equal(m, packed[:int(offs[-1])].numpy())
    np.testing.assert_array_equal(o, offs.numpy())
    np.testing.assert_array_equal(c, cnt.numpy())
    assert not (tmp_path / "sample_pairs.npy").exists()


def test_dump_over_budget_is_a_fixed_sample_of_whole_pairs(tmp_path, monkeypatch):
    import bench
    packed, offs, cnt = _step()
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 256)
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(str(d), packed, offs, cnt, 12)
        runs.append({n: _load(d, n) for n in ("matches", "offsets", "counts", "sample_pairs")})
    for n in runs[0]:
        np.testing.assert_array_equal(runs[0][n], runs[1][n])
    r, o = runs[0], offs.numpy()
    pairs = r["sample_pairs"].astype(np.int64)
    assert 0 < len(pairs) < 12 and np.all(np.diff(pairs) > 0)
    np.testing.assert_array_equal(r["counts"], cnt.numpy()[pairs])
    for j, i in enumerate(pairs):
        got = r["matches"][int(r["offsets"][j]):int(r["offsets"][j + 1])]
        np.testing.assert_array_equal(got, packed.numpy()[o[i]:o[i + 1]])
