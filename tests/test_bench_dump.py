"""bench.py --dump-outputs: the step's results as DIR/<name>.npy in float64.
Each check's pod list becomes its 0/1 membership vector over the n pods (n
elements whatever the list holds, an empty list included), policy_shadow's
pairs stay (count, 2), exact in float64, and an array beyond the per-array
limit is a fixed sample of its rows (the same rows from run to run, so two
builds compare output for output); --full and --dump-outputs are options of
the command."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "kubernetes-verification_amd"))

N = 3000


@pytest.fixture(scope="module")
def bench():
    import bench as b
    return b


def _results(n_pairs):
    rng = np.random.Generator(np.random.PCG64(5))
    return {"all_reachable": np.zeros(0, np.int32),
            "all_isolated": np.arange(3, N, 7, dtype=np.int32),
            "user_crosscheck": np.array([N - 1, 5], np.int32),
            "system_isolation": None,
            "policy_shadow": rng.integers(0, 2**31 - 1, (n_pairs, 2), dtype=np.int32),
            "policy_shadow_count": n_pairs}


def test_dump_is_exact_float64(bench, tmp_path):
    res = _results(1000)
    bench.dump_outputs(str(tmp_path / "d"), res, N)
    names = sorted(os.listdir(tmp_path / "d"))
    assert names == sorted(k + ".npy" for k, v in res.items() if v is not None)
    arrays = {k: np.load(tmp_path / "d" / (k + ".npy")) for k, v in res.items() if v is not None}
    assert all(a.dtype == np.float64 and a.size > 0 for a in arrays.values())
    for k in ("all_reachable", "all_isolated", "user_crosscheck"):
        a = arrays[k]
        assert a.shape == (N,) and set(np.unique(a)) <= {0.0, 1.0}
        assert np.flatnonzero(a).tolist() == sorted(res[k].tolist())
    assert arrays["policy_shadow"].shape == (1000, 2)
    assert np.array_equal(arrays["policy_shadow"], res["policy_shadow"].astype(np.float64))
    assert arrays["policy_shadow_count"].tolist() == [1000.0]


def test_dump_writes_no_empty_array(bench, tmp_path):
    res = _results(0)
    bench.dump_outputs(str(tmp_path / "d"), res, N)
    names = sorted(os.listdir(tmp_path / "d"))
    assert "policy_shadow.npy" not in names and "policy_shadow_count.npy" in names
    assert all(np.load(tmp_path / "d" / f).size > 0 for f in names)
    assert np.load(tmp_path / "d" / "policy_shadow_count.npy").tolist() == [0.0]


def test_dump_samples_large_arrays_the_same_way(bench, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 512)
    res = _results(1000)
    bench.dump_outputs(str(tmp_path / "a"), res, N)
    bench.dump_outputs(str(tmp_path / "b"), res, N)
    pa = np.load(tmp_path / "a" / "policy_shadow.npy")
    assert pa.shape == (256, 2)                      # whole rows, 512 elements
    assert np.array_equal(pa, np.load(tmp_path / "b" / "policy_shadow.npy"))
    # the sample is rows of the input, in the input's order
    full = res["policy_shadow"].astype(np.float64)
    pos = [int(np.flatnonzero((full == r).all(axis=1))[0]) for r in pa]
    assert pos == sorted(pos) and len(set(pos)) == 256
    # a changed row inside the sample shows
    res2 = dict(res, policy_shadow=res["policy_shadow"].copy())
    res2["policy_shadow"][pos[10], 1] ^= 1
    bench.dump_outputs(str(tmp_path / "c"), res2, N)
    assert not np.array_equal(pa, np.load(tmp_path / "c" / "policy_shadow.npy"))
    # the pod vectors are sampled alike (N > 512), the same pods in both runs
    ia = np.load(tmp_path / "a" / "all_isolated.npy")
    assert ia.shape == (512,) and np.array_equal(ia, np.load(tmp_path / "b" / "all_isolated.npy"))


def test_dump_stays_within_64_mb(bench):
    # the six results of a step, each at the per-array limit
    assert 6 * bench.DUMP_MAX_ELEMS * 8 <= 64 * 10**6


def test_options(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "x"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "x"
