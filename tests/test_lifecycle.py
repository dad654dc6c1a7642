"""Device memory over a context's life and over the calls whose buffers are
their own: kano_device_bytes (the bytes held by the engine's device buffers and
their number, process-wide) returns to where it was, exactly.

The other failing paths (an allocation or a launch that fails) are not
provoked here: the move-only buffer type frees on every return by
construction."""
import errno
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, P = 300, 40          # five words a row: every list and class buffer exists


def _tables(seed=11):
    from kano import model
    from kano._intern import group_ids, intern
    from kano.synth import make_cluster, objects_from_json
    cs, ps = objects_from_json(make_cluster(N, P, "sparse", seed=seed).to_json_obj(), model)
    return intern(cs, ps), group_ids(cs, "tenant")


def _held():
    from kano import _native as nat
    gc.collect()
    return nat.device_bytes()


def test_context_lifetime_returns_every_byte():
    from kano._engine import DeviceBuild
    t, gid = _tables()
    ncols = t.ncols + (len(t.expr_col) if t.expr_col is not None else 0)
    first = _held()
    for _ in range(2):
        eng = DeviceBuild(t)
        assert _held()[0] > first[0] and _held()[1] > first[1]
        eng.build("bitwise")
        eng.build("mfma")
        out = eng.verify(gid=gid, shadow=True)
        assert out["user_crosscheck"] is not None and out["pairs"] is not None
        # two policies on one extra pod column, then one of them removed
        xval = (np.arange(N, dtype=np.int32) % 3).reshape(1, N)
        off = np.array([0, 1, 2], np.int64)
        col = np.array([ncols, ncols], np.int32)
        a0 = eng.add_policies(xval, (off, col, np.array([1, 2], np.int32)),
                              (off, col, np.array([2, 0], np.int32)))
        eng.remove_policies([a0])
        eng.set_pipeline(True)   # a primed prologue and both input sets
        eng.verify(gid=gid, shadow=True)
        eng.verify(gid=gid, shadow=True)
        eng.close()
        del eng
    assert _held() == first


@pytest.fixture(scope="module")
def env():
    from kano._engine import DeviceBuild
    t, gid = _tables()
    rng = np.random.default_rng(5)
    e = dict(t=t, gid=gid)
    e["src"] = src = DeviceBuild(t)
    e["ing"] = DeviceBuild(_tables(seed=12)[0])       # a second build of as many pods
    e["dst"] = DeviceBuild.empty(N)
    e["half"] = half = DeviceBuild.empty(N)           # the first half of the policies
    nids = src.nids()
    src.subset_into(half, np.arange(nids) < nids // 2)
    e["rev"] = rev = DeviceBuild.empty(N)
    src.reverse_into(rev)
    e["pairs"] = rng.integers(0, N, size=(500, 2)).astype(np.int32)
    e["prio"] = rng.integers(0, 4, size=nids).astype(np.int32)
    e["action"] = (rng.random(nids) < 0.3).astype(np.uint8)
    e["pmask"] = rng.integers(1, 1 << 62, size=(nids, 2)).astype(np.uint64)
    W = (N + 63) // 64
    sets = rng.integers(0, 1 << 62, size=(2, 3, W)).astype(np.uint64)
    sets[..., W - 1] &= np.uint64((1 << (N % 64)) - 1)
    e["isrc"], e["idst"] = sets
    # level * 4 + action under np_level 1: allow / pass / deny above it, allow /
    # isolate at it
    codes = np.array([4, 4, 2, 1, 4, 7, 0], np.uint32)
    e["code_e"] = codes[np.arange(nids) % len(codes)]
    e["code_i"] = codes[np.arange(e["ing"].nids()) % len(codes)]
    yield e
    for k in ("src", "ing", "dst", "half", "rev"):
        e[k].close()


# the calls whose device buffers are the call's own (kano_engine.hpp), with
# rows_digest and diff_pairs
CALLS = {
    "group_counts": lambda e: e["src"].group_counts(e["gid"] % 5, e["gid"] % 7, rows=True),
    "hops": lambda e: e["src"].hops([0, 17, N - 1]),
    "hop_pairs": lambda e: e["src"].hop_pairs(e["pairs"][:64], paths=True),
    "intents": lambda e: e["src"].intents(e["isrc"], e["idst"], [1, 0, 3]),
    "intent_pairs": lambda e: e["src"].intent_pairs(e["isrc"][:1], e["idst"][:1], 1),
    "subset_into": lambda e: e["src"].subset_into(e["dst"], np.arange(e["src"].nids()) % 3 != 0),
    "pair_masks": lambda e: e["src"].pair_masks(e["pairs"], e["pmask"]),
    "verdict_into": lambda e: e["src"].verdict_into(e["dst"], e["prio"], e["action"]),
    "pair_verdicts": lambda e: e["src"].pair_verdicts(e["pairs"], e["prio"], e["action"]),
    "k8s_conn_from": lambda e: e["dst"].k8s_conn_from(e["src"], e["ing"]),
    "k8s_conn_tiers_from": lambda e: e["dst"].k8s_conn_tiers_from(
        e["src"], e["ing"], True, e["code_e"], 1, e["code_i"], 1),
    "k8s_isolated": lambda e: e["src"].k8s_isolated(),
    "k8s_pair_verdicts": lambda e: e["src"].k8s_pair_verdicts(
        e["ing"], e["pairs"], True, e["code_e"], 1, e["code_i"], 1),
    "reverse_into": lambda e: e["src"].reverse_into(e["dst"]),
    "zones": lambda e: e["src"].zones(e["rev"]),
    "rows_digest": lambda e: e["src"].rows_digest(0, N),
    "diff_pairs": lambda e: e["src"].diff_pairs(e["half"], "removed", 0, N),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_call_owns_its_temporaries(env, name):
    CALLS[name](env)              # (what a context keeps grows here, once)
    before = _held()
    CALLS[name](env)
    assert _held() == before


def test_rejected_call_holds_nothing(env):
    """kano_diff_pairs with room for fewer pairs than there are: -ENOSPC after
    the counting pass, and no buffer more than before."""
    from ctypes import byref, c_int64
    src, half = env["src"], env["half"]
    count = src.diff_count(half, "removed", 0, N)
    assert count > 1
    out = np.empty((count, 2), np.int32)
    got = c_int64(0)
    before = _held()
    rc = src.lib.kano_diff_pairs(src.ctx, half.ctx, 1, 0, N, count - 1, byref(got),
                                 out.ctypes.data)
    assert rc == -errno.ENOSPC and got.value == count
    assert _held() == before
