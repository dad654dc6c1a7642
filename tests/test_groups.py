"""group_reachability (kano_group_counts and the layers above it): the
quotient of a matrix by a source and a destination labelling of the pods,
  counts[g][h]     = #{(i, j) : M[i, j] = 1, gs[i] = g, gd[j] = h}
  row_counts[i][h] = #{j : M[i, j] = 1, gd[j] = h}
with negative ids leaving a pod out.  The expectation everywhere is `want`
below, a numpy restatement on the unpacked bits.  Exact integers throughout.
"""
import ctypes
import errno
import functools
import os
import re

import numpy as np
import pytest

from _golden import cluster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unpack(words, n):
    """(rows, W) u64 words -> (rows, n) bool; bits at positions >= n dropped."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    w = w.reshape(w.shape[0], -1)
    if w.shape[1] == 0:
        return np.zeros((w.shape[0], n), bool)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def one_hot(ids, G):
    """(len(ids), G) int64; a negative id gives a zero row."""
    ids = np.asarray(ids, dtype=np.int64)
    out = np.zeros((ids.shape[0], G), dtype=np.int64)
    keep = np.flatnonzero(ids >= 0)
    out[keep, ids[keep]] = 1
    return out


def times_one_hot(M, ids, G):
    """M @ one_hot(ids, G) in int64.  A one-hot factor makes the product a sum
    of M's columns by group: the columns sorted by group and added up run by
    run, the same int64 sums without the multiplications by zero (the literal
    product of a 100,003-column case takes seconds; the CPU tests below hold
    this form to it)."""
    ids = np.asarray(ids, dtype=np.int64)
    out = np.zeros((M.shape[0], G), dtype=np.int64)
    keep = np.flatnonzero(ids >= 0)
    if keep.size == 0 or M.shape[0] == 0:
        return out
    order = keep[np.argsort(ids[keep], kind="stable")]
    sorted_ids = ids[order]
    starts = np.flatnonzero(np.r_[True, sorted_ids[1:] != sorted_ids[:-1]])
    out[:, sorted_ids[starts]] = np.add.reduceat(M[:, order].astype(np.int64), starts, axis=1)
    return out


def want(words, n, gs, gd, Gs, Gd, r0=0):
    """The definition on the unpacked words of rows r0.. : (counts int64
    (Gs, Gd), row_counts int64 (rows, Gd)).  With S and D the one-hot matrices
    of gs (the rows with gs >= 0) and gd: counts = S.T @ M @ D, row_counts =
    M @ D over every row."""
    M = unpack(words, n)
    rows = M.shape[0]
    row_counts = times_one_hot(M, gd, Gd)                       # M @ D
    src = np.asarray(gs, dtype=np.int64)[r0:r0 + rows]
    return times_one_hot(row_counts.T, src, Gs).T, row_counts   # S.T @ (M @ D)


def random_words(rng, rows, n, density):
    """Random rows; the bits past n in the last word are random too."""
    W = (n + 63) // 64
    if density >= 1.0:
        return np.full((rows, W), np.uint64(0xFFFFFFFFFFFFFFFF))
    bits = rng.random((rows, W * 64)) < density
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(rows, W)


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "kano_hip.h")) as f:
        text = f.read()
    for name in ("kano_group_counts", "kano_group_counts_time"):
        assert re.search(r"^int %s\(kano_ctx\*" % name, text, re.M), name


def test_native_binds_the_entry_points():
    from kano import _native as nat
    assert len(nat.SIGNATURES["kano_group_counts"][1]) == 7
    assert len(nat.SIGNATURES["kano_group_counts_time"][1]) == 2
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libkano_hip.so not built")
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in ("kano_group_counts", "kano_group_counts_time"):
        assert getattr(lib, name) is not None


def test_api_is_exported_and_pairs_lists_the_table():
    from kano import algorithm as alg
    for name in ("group_reachability", "group_fanout", "reach_count"):
        assert callable(getattr(alg, name)), name
    assert alg.GroupReachability._fields == ("src_keys", "dst_keys", "counts", "src_sizes",
                                             "dst_sizes")
    #        a  b  ""
    #  a     4  0  2
    #  b     1  7  0
    #  ""    0  0  0
    keys = ["a", "b", ""]
    t = alg.GroupReachability(keys, keys, np.array([[4, 0, 2], [1, 7, 0], [0, 0, 0]], np.int64),
                              np.array([2, 3, 1]), np.array([2, 3, 1]))
    assert t.pairs() == [("a", "", 2), ("b", "a", 1)]
    assert t.pairs(cross_only=False) == [("a", "a", 4), ("a", "", 2), ("b", "a", 1),
                                         ("b", "b", 7)]
    assert all(type(c) is int for _, _, c in t.pairs())
    # two labellings: equal keys on both sides are still "the same group"
    u = t._replace(dst_keys=["x", "b", "y"])
    assert u.pairs() == [("a", "x", 4), ("a", "y", 2), ("b", "x", 1)]
    assert u.pairs(cross_only=False)[-1] == ("b", "b", 7)
    empty = alg.GroupReachability([], [], np.zeros((0, 0), np.int64), np.zeros(0), np.zeros(0))
    assert empty.pairs() == [] and empty.pairs(cross_only=False) == []


def test_restatement_on_a_hand_written_case():
    #      M        gs    gd = [0, 1, 0]
    # 0: 1 1 0      0     row_counts 1 1
    # 1: 0 1 1     -1                1 1    (left out of counts)
    # 2: 1 0 1      1                2 0
    # bit 3 of row 0 is set as well: past n, in no group
    M = np.array([[0b1011], [0b110], [0b101]], np.uint64)
    gs, gd = [0, -1, 1], [0, 1, 0]
    counts, rows = want(M, 3, gs, gd, 2, 2)
    assert counts.dtype == np.int64 and counts.tolist() == [[1, 1], [2, 0]]
    assert rows.tolist() == [[1, 1], [1, 1], [2, 0]]
    # a negative destination id: column 2 is counted nowhere
    counts, rows = want(M, 3, gs, [0, 1, -1], 2, 2)
    assert counts.tolist() == [[1, 1], [1, 0]] and rows.tolist() == [[1, 1], [0, 1], [1, 0]]
    # one group a side: the set bits of the rows kept
    counts, _ = want(M, 3, [0, 0, 0], [0, 0, 0], 1, 1)
    assert counts.tolist() == [[6]]
    # rows 1.. of a shard: gs is indexed by the global row
    counts, rows = want(M[1:], 3, gs, gd, 2, 2, r0=1)
    assert counts.tolist() == [[0, 0], [2, 0]] and rows.tolist() == [[1, 1], [2, 0]]
    # and the product itself, S.T @ M @ D in int64, on the same case and a random one
    keep = [0, 2]
    assert (one_hot([0, 1], 2).T @ unpack(M, 3)[keep].astype(np.int64)
            @ one_hot(gd, 2)).tolist() == [[1, 1], [2, 0]]
    rng = np.random.default_rng(9)
    n, Gs, Gd = 70, 4, 9
    R = random_words(rng, n, n, 0.4)
    gs, gd = rng.integers(-1, Gs, n), rng.integers(-2, Gd, n)
    counts, rows = want(R, n, gs, gd, Gs, Gd)
    B = unpack(R, n).astype(np.int64)
    assert np.array_equal(rows, B @ one_hot(gd, Gd))
    assert np.array_equal(counts, one_hot(gs, Gs).T @ B @ one_hot(gd, Gd))
    assert counts.dtype == np.int64 and counts.sum() > 0


def test_group_keys_follow_user_hashmap():
    from kano import algorithm as alg
    from kano import model
    labels = [{"t": "b"}, {}, {"t": "a"}, {"t": "b"}, {"other": "x"}, {"t": ""}, {"t": "c"}]
    cs = [model.Container(f"p{i}", dict(l)) for i, l in enumerate(labels)]
    keys, gid = alg.group_keys(cs, "t")
    assert keys == list(alg.user_hashmap(cs, "t").keys()) == ["b", "", "a", "c"]
    assert gid.dtype == np.int32 and gid.tolist() == [0, 1, 2, 0, 1, 1, 3]
    assert np.array_equal(gid, alg.group_ids(cs, "t"))
    assert alg.group_keys([], "t")[0] == []


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def need_gpu():
    from kano import _native
    if not _native.gpu_available():
        pytest.fail("GPU test run without a usable HIP device / libkano_hip.so")


gpu = pytest.mark.gpu


def engine_of(words, n, rows=None):
    from kano._engine import DeviceBuild
    e = DeviceBuild.empty(n, rows=rows)
    words = np.ascontiguousarray(words, dtype=np.uint64)
    if words.size:
        e.put_rows(rows[0] if rows else 0, words)
    return e


def check_against(e, words, n, gs, gd, Gs, Gd, r0=0):
    """counts and row_counts, asked for together and counts alone."""
    wc, wr = want(words, n, gs, gd, Gs, Gd, r0)
    got = e.group_counts(gs, gd, Gs, Gd, rows=True)
    assert got["counts"].dtype == np.int64 and got["counts"].shape == (Gs, Gd)
    assert got["row_counts"].dtype == np.int32 and got["row_counts"].shape == wr.shape
    assert np.array_equal(got["counts"], wc)
    assert np.array_equal(got["row_counts"], wr)
    only = e.group_counts(gs, gd, Gs, Gd)           # row_counts NULL
    assert only["row_counts"] is None and np.array_equal(only["counts"], wc)
    return wc, wr


def labellings(n, G):
    """Consecutive columns in different groups, and block-contiguous groups."""
    j = np.arange(n, dtype=np.int64)
    return (j % G).astype(np.int32), (j * G // max(n, 1)).astype(np.int32)


@gpu
@pytest.mark.parametrize("density", [0.0, 0.02, 0.5, 1.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 1000])
def test_small_n(n, density, need_gpu):
    rng = np.random.default_rng(1000 * n + int(density * 100))
    M = random_words(rng, n, n, density)
    e = engine_of(M, n)
    Gs, Gd = min(n, 3), min(n, 5)
    gs = rng.integers(0, Gs, n).astype(np.int32)
    for gd in labellings(n, Gd):
        wc, wr = check_against(e, M, n, gs, gd, Gs, Gd)
        if density == 1.0:
            assert int(wc.sum()) == n * n and (wr.sum(axis=1) == n).all()
        if density == 0.0:
            assert not wc.any()
    e.close()


@functools.lru_cache(maxsize=None)
def grid_matrix():
    n = 200
    M = random_words(np.random.default_rng(200), n, n, 0.3)
    M.setflags(write=False)
    return n, M


@gpu
@pytest.mark.parametrize("tune", ["", "gbatch=1,ggrid=3"])
@pytest.mark.parametrize("Gs", [1, 3, 65, "n"])
def test_group_counts_of_every_width(Gs, tune, monkeypatch, need_gpu):
    """Gd below, at and past one and two batches of 64 destination groups;
    gbatch=1 (KANO_TUNE) makes every batch a pass of its own and ggrid=3 has
    three blocks stride over the items."""
    monkeypatch.setenv("KANO_TUNE", tune)
    n, M = grid_matrix()
    Gs = n if Gs == "n" else Gs
    e = engine_of(M, n)
    rng = np.random.default_rng(Gs)
    gs = (np.arange(n, dtype=np.int32) if Gs == n
          else rng.integers(0, Gs, n).astype(np.int32))      # Gs = n: a pod a group
    for Gd in (1, 63, 64, 65, 130):
        for gd in labellings(n, Gd):
            wc, _ = check_against(e, M, n, gs, gd, Gs, Gd)
            assert int(wc.sum()) == int(unpack(M, n).sum())
    e.close()


@gpu
def test_source_ids_far_apart(need_gpu):
    """5,000,000 source groups of which 200 hold a pod: past 4,194,304 groups
    the host orders the rows with a comparison sort, not a counting sort."""
    n, M = grid_matrix()
    Gs, Gd = 5_000_000, 2
    rng = np.random.default_rng(5)
    gs = rng.choice(Gs, size=n, replace=False).astype(np.int32)
    gs[:2] = (Gs - 1, 0)
    gs[7] = -1
    gd = (np.arange(n) % Gd).astype(np.int32)
    e = engine_of(M, n)
    wc, _ = check_against(e, M, n, gs, gd, Gs, Gd)
    assert np.count_nonzero(wc.any(axis=1)) > 150 and wc[Gs - 1].any()
    e.close()


@gpu
def test_negative_ids_leave_pods_out(need_gpu):
    n = 130
    rng = np.random.default_rng(130)
    M = random_words(rng, n, n, 0.4)
    e = engine_of(M, n)
    Gs, Gd = 4, 70
    gs = rng.integers(0, Gs, n).astype(np.int32)
    gd = rng.integers(0, Gd, n).astype(np.int32)
    out_s, out_d = gs.copy(), gd.copy()
    out_s[rng.random(n) < 0.4] = -1
    out_d[rng.random(n) < 0.4] = -7
    none = np.full(n, -1, np.int32)
    full, _ = check_against(e, M, n, gs, gd, Gs, Gd)
    a, _ = check_against(e, M, n, out_s, gd, Gs, Gd)
    b, _ = check_against(e, M, n, gs, out_d, Gs, Gd)
    c, _ = check_against(e, M, n, out_s, out_d, Gs, Gd)
    assert full.sum() > a.sum() > c.sum() > 0 and full.sum() > b.sum() > c.sum()
    z, zr = check_against(e, M, n, none, none, Gs, Gd)
    assert not z.any() and not zr.any()
    z, zr = check_against(e, M, n, none, gd, Gs, Gd)      # the row counts are still there
    assert not z.any() and zr.sum() == unpack(M, n).sum()
    z, _ = check_against(e, M, n, gs, none, Gs, Gd)
    assert not z.any()
    e.close()


@gpu
def test_row_shards(need_gpu):
    n, rows = 200, (37, 121)
    rng = np.random.default_rng(37)
    M = random_words(rng, n, n, 0.25)
    Gs, Gd = 6, 66
    gs = rng.integers(-1, Gs, n).astype(np.int32)
    gd = rng.integers(-1, Gd, n).astype(np.int32)
    whole = engine_of(M, n)
    wc, wr = check_against(whole, M, n, gs, gd, Gs, Gd)
    total = np.zeros_like(wc)
    parts = []
    for r0, r1 in ((0, 37), rows, (121, 200)):
        e = engine_of(M[r0:r1], n, rows=(r0, r1))
        c, r = check_against(e, M[r0:r1], n, gs, gd, Gs, Gd, r0=r0)
        total += c
        parts.append(r)
        e.close()
    assert np.array_equal(total, wc)                       # the counts add up
    assert np.array_equal(np.concatenate(parts), wr)       # the row counts concatenate
    empty = engine_of(np.zeros((0, 4), np.uint64), n, rows=(50, 50))
    got = empty.group_counts(gs, gd, Gs, Gd, rows=True)
    assert got["counts"].shape == (Gs, Gd) and not got["counts"].any()
    assert got["row_counts"].shape == (0, Gd)
    for x in (whole, empty):
        x.close()


@gpu
def test_degenerate_sizes(need_gpu):
    from kano._engine import DeviceBuild
    z = DeviceBuild.empty(0)
    e0 = np.zeros(0, np.int32)
    got = z.group_counts(e0, e0, 2, 3, rows=True)
    assert got["counts"].shape == (2, 3) and not got["counts"].any()
    assert got["row_counts"].shape == (0, 3)
    assert z.group_counts(e0, e0)["counts"].tolist() == [[0]]     # G = max + 1, at least 1
    z.close()
    e = engine_of(np.array([[0b101]], np.uint64), 1)              # n = 1, bits past n set
    assert e.group_counts([0], [0])["counts"].tolist() == [[1]]
    assert e.group_counts([2], [1], rows=True)["counts"].tolist() == [[0, 0], [0, 0], [0, 1]]
    with pytest.raises(ValueError):
        e.group_counts([0, 0], [0])
    e.close()


@gpu
@pytest.mark.parametrize("density", [0.01, 1.0])
def test_wide_rows(density, need_gpu):
    """n = 100,003 is 1,563 words: seven column chunks of 256 words, the last
    one short and ending in a word with 35 valid bits; Gd = 70 is two group
    batches; the 40 rows are five groups of eight rows of a run."""
    n, rows, Gd, Gs = 100003, (5, 45), 70, 3
    rng = np.random.default_rng(100003)
    M = random_words(rng, 40, n, density)
    gs = rng.integers(-1, Gs, n).astype(np.int32)
    e = engine_of(M, n, rows=rows)
    for gd in labellings(n, Gd):
        gd = gd.copy()
        gd[::97] = -1
        wc, wr = check_against(e, M, n, gs, gd, Gs, Gd, r0=5)
        if density == 1.0:
            assert (wr.sum(axis=1) == int((gd >= 0).sum())).all()
    e.close()


@gpu
def test_sums_are_64_bit(need_gpu):
    """66,000 pods, every bit set (the tails as well), one group a side:
    n * n = 4,356,000,000 pairs."""
    from kano._engine import DeviceBuild
    n = 66000
    W = (n + 63) // 64
    e = DeviceBuild.empty(n)
    slab = np.full((6000, W), np.uint64(0xFFFFFFFFFFFFFFFF))
    for r0 in range(0, n, 6000):
        e.put_rows(r0, slab[:min(6000, n - r0)])
    zero = np.zeros(n, np.int32)
    assert n * n > 2 ** 32
    got = e.group_counts(zero, zero, 1, 1, rows=True)
    assert got["counts"].tolist() == [[n * n]]
    assert got["row_counts"].shape == (n, 1)
    assert int(got["row_counts"].min()) == n == int(got["row_counts"].max())
    assert e.group_counts(zero, zero, 1, 1)["counts"].tolist() == [[n * n]]
    e.close()


@gpu
def test_error_codes_leave_the_context_usable(need_gpu):
    from kano import _native as nat
    n = 128
    rng = np.random.default_rng(5)
    M = random_words(rng, n, n, 0.3)
    e = engine_of(M, n)
    lib = e.lib
    Gs, Gd = 3, 5
    gs = rng.integers(0, Gs, n).astype(np.int32)
    gd = rng.integers(0, Gd, n).astype(np.int32)
    counts = np.full((Gs, Gd), -7, np.int64)
    rows = np.zeros((n, Gd), np.int32)

    def call(ctx, s, S, d, D, c, r=None):
        p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        return lib.kano_group_counts(ctx, p(s), S, p(d), D, p(c), p(r))

    EINVAL, ERANGE = -errno.EINVAL, -errno.ERANGE
    assert call(None, gs, Gs, gd, Gd, counts) == EINVAL
    assert call(e.ctx, None, Gs, gd, Gd, counts) == EINVAL
    assert call(e.ctx, gs, Gs, None, Gd, counts) == EINVAL
    assert call(e.ctx, gs, Gs, gd, Gd, None, rows) == EINVAL
    assert call(e.ctx, gs, 0, gd, Gd, counts) == EINVAL
    assert call(e.ctx, gs, Gs, gd, 0, counts) == EINVAL
    assert call(e.ctx, gs, Gs, gd, -1, counts) == EINVAL
    bad = gs.copy()
    bad[77] = Gs
    assert call(e.ctx, bad, Gs, gd, Gd, counts) == ERANGE
    bad = gd.copy()
    bad[n - 1] = Gd + 100
    assert call(e.ctx, gs, Gs, bad, Gd, counts, rows) == ERANGE
    assert call(e.ctx, gs, 1 << 14, gd, 1 << 14, counts) == -errno.ENOTSUP     # 2^28 cells
    assert (counts == -7).all()                      # no error wrote a result
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.ERANGE}\b"):
        e.group_counts(gs, bad, Gs, Gd)
    ms = ctypes.c_float(-1.0)
    assert lib.kano_group_counts_time(e.ctx, None) == EINVAL
    assert lib.kano_group_counts_time(None, ctypes.byref(ms)) == EINVAL
    check_against(e, M, n, gs, gd, Gs, Gd)           # the context still answers
    assert lib.kano_group_counts_time(e.ctx, ctypes.byref(ms)) == 0 and ms.value == 0.0
    e.close()


@gpu
def test_device_time_is_recorded_under_timing(monkeypatch, need_gpu):
    monkeypatch.setenv("KANO_TUNE", "timing=1")
    n = 300
    M = random_words(np.random.default_rng(300), n, n, 0.1)
    e = engine_of(M, n)
    assert e.group_counts_time() == 0.0
    gs, gd = labellings(n, 7)
    check_against(e, M, n, gs, gd, 7, 7)
    assert 0.0 < e.group_counts_time() < 1000.0
    e.close()


@gpu
def test_nothing_else_moves(need_gpu):
    """The call writes its own buffers only: rows, column checks, the stored
    crosscheck words and the shadow pairs are what they were."""
    import test_redundancy as tr
    from kano._engine import DeviceBuild
    from kano._intern import group_ids
    name = "s_sparse_200"
    obj = cluster(name)
    cs, _ = tr.api_objects(obj)
    e = DeviceBuild(tr.cluster_tables(name))
    n = e.n
    gid = group_ids(cs, obj["label"])
    digest = e.rows_digest(0, n).copy()
    cols = [x.copy() for x in e.col_checks()]
    cross = e.crosscheck(gid).copy()
    k = e.shadow_count()
    pairs = e.shadow_fetch(k).copy()
    G = int(gid.max()) + 1
    wc, wr = check_against(e, e.rows(0, n), n, gid, gid, G, G)
    assert wc.sum() > 0
    assert np.array_equal(e.shadow_fetch(k), pairs)          # fetched, not recomputed
    assert np.array_equal(e.rows_digest(0, n), digest)
    assert all(np.array_equal(x, y) for x, y in zip(e.col_checks(), cols))
    assert np.array_equal(e.crosscheck(gid), cross)
    assert e.shadow_count() == k and np.array_equal(e.shadow_fetch(k), pairs)
    assert e.policy_impact().tolist() == tr.record(name)["impact"]
    e.close()


@gpu
def test_between_pipelined_verify_steps(need_gpu):
    """A group_counts() between two steps of a pipelined verify loop leaves
    the next step's lists and pairs at their golden values."""
    import test_redundancy as tr
    from _golden import expected, sha
    from kano._engine import DeviceBuild
    from kano._intern import intern, group_ids
    name = "s_sparse_2000"
    obj = cluster(name)
    cs, ps = tr.api_objects(obj)
    exp = expected(name)
    gid = group_ids(cs, obj["label"])
    G = int(gid.max()) + 1
    eng = DeviceBuild(intern(cs, ps), build=False)
    eng.set_pipeline(True)

    def step():
        r = eng.verify(gid, sys_row=0, shadow=True)
        assert r["all_isolated"].tolist() == exp["all_isolated"]
        assert r["all_reachable"].tolist() == exp["all_reachable"]
        assert r["user_crosscheck"].tolist() == exp["user_crosscheck"]["result"]
        assert r["system_isolation"].tolist() == exp["system_isolation"]["result"]
        assert r["shadow_count"] == exp["policy_shadow"]["count"]
        assert sha(np.ascontiguousarray(r["pairs"])) == exp["policy_shadow"]["sha256"]

    step()
    step()
    first = eng.group_counts(gid, gid, G, G, rows=True)
    step()
    again = eng.group_counts(gid, gid, G, G, rows=True)
    step()
    n = len(cs)
    M = eng.rows(0, n)
    assert sha(M) == exp["M_sha256"]
    wc, wr = want(M, n, gid, gid, G, G)
    for got in (first, again):
        assert np.array_equal(got["counts"], wc) and np.array_equal(got["row_counts"], wr)
    eng.close()


def built(name):
    import test_redundancy as tr
    from kano.model import ReachabilityMatrix
    obj = cluster(name)
    cs, ps = tr.api_objects(obj)
    return obj, cs, ps, ReachabilityMatrix.build_matrix(cs, ps)


def matrix_words(m):
    n = m.container_size
    return m._engine.rows(0, n)


@gpu
@pytest.mark.parametrize("name", ["s_sparse_200", "s_sparse_50", "q_missing_label",
                                  "q_no_conflict", "q_shadow"])
def test_api_on_a_built_cluster(name, need_gpu):
    from kano import algorithm as alg
    obj, cs, ps, m = built(name)
    label = obj["label"]
    n = m.container_size
    M = matrix_words(m)
    bits = unpack(M, n)
    keys, gid = alg.group_keys(cs, label)
    G = len(keys)
    t = alg.group_reachability(m, cs, label)
    wc, wr = want(M, n, gid, gid, G, G)
    assert t.src_keys == keys == t.dst_keys
    assert t.counts.dtype == np.int64 and np.array_equal(t.counts, wc)
    assert int(t.counts.sum()) == int(bits.sum())
    assert np.array_equal(t.src_sizes, np.bincount(gid, minlength=G))
    assert np.array_equal(t.dst_sizes, t.src_sizes)
    assert bool(t.pairs(cross_only=True)) == bool(alg.user_crosscheck(m, cs, label))
    assert sum(c for _, _, c in t.pairs(cross_only=False)) == int(bits.sum())
    dkeys, fan = alg.group_fanout(m, cs, label)
    assert dkeys == keys and fan.dtype == np.int32 and np.array_equal(fan, wr)
    assert np.array_equal(fan.sum(axis=1), bits.sum(axis=1))
    assert np.array_equal(alg.group_fanout(m, cs, label, rows=(1, n - 1))[1], wr[1:n - 1])
    with pytest.raises(ValueError):
        alg.group_fanout(m, cs, label, rows=(0, n + 1))
    for j in (0, n // 2, n - 1):
        assert alg.reach_count(m, range(n), [j]) == int(bits[:, j].sum())
    assert alg.reach_count(m, [0, n - 1], range(n)) == int(bits[0].sum() + bits[n - 1].sum())
    assert alg.reach_count(m, [], range(n)) == 0
    with pytest.raises(ValueError, match="equal length"):
        alg.group_reachability(m, cs[:-1], label)
    with pytest.raises(ValueError, match="equal length"):
        alg.group_fanout(m, cs + cs[:1], label)
    # a second labelling on the destination side
    other = "app" if any("app" in c.labels for c in cs) else label
    dk, gd = alg.group_keys(cs, other)
    t2 = alg.group_reachability(m, cs, label, dst_label=other)
    assert (t2.src_keys, t2.dst_keys) == (keys, dk)
    assert np.array_equal(t2.counts, want(M, n, gid, gd, G, len(dk))[0])
    assert np.array_equal(t2.dst_sizes, np.bincount(gd, minlength=len(dk)))


@gpu
def test_after_an_incremental_update(need_gpu):
    import test_redundancy as tr
    from kano import algorithm as alg
    from kano.model import ReachabilityMatrix
    name = "s_sparse_200"
    obj = cluster(name)
    label = obj["label"]
    cs, ps = tr.api_objects(dict(obj, policies=obj["policies"][1:]))
    m = ReachabilityMatrix.build_matrix(cs, ps)
    before = m.snapshot()
    t0 = alg.group_reachability(before, cs, label)
    new = tr.api_objects(dict(obj, policies=obj["policies"][:1]))[1][0]
    m.add_policies([new])
    t1 = alg.group_reachability(m, cs, label)
    d = alg.matrix_diff(before, m)
    assert d.added > 0
    assert int((t1.counts - t0.counts).sum()) == d.added - d.removed
    n = m.container_size
    _, gid = alg.group_keys(cs, label)
    G = len(t1.src_keys)
    assert np.array_equal(t1.counts, want(matrix_words(m), n, gid, gid, G, G)[0])
    assert np.array_equal(alg.group_reachability(before, cs, label).counts, t0.counts)
    # the two-hop matrix: a path matrix answers the same way
    hop = alg.two_hop(m)
    assert np.array_equal(alg.group_reachability(hop, cs, label).counts,
                          want(matrix_words(hop), n, gid, gid, G, G)[0])


@gpu
def test_multibuild_equals_one_context(need_gpu):
    import test_redundancy as tr
    from kano import algorithm as alg
    from kano._engine import DeviceBuild
    from kano._intern import group_ids
    from kano.model import ReachabilityMatrix
    from kano.multi import MultiBuild
    name = "s_sparse_2000"
    obj = cluster(name)
    cs, _ = tr.api_objects(obj)
    t = tr.cluster_tables(name)
    n = t.n
    gid = group_ids(cs, obj["label"])
    gd = (np.arange(n) % 77).astype(np.int32)
    one = DeviceBuild(t)
    ref = one.group_counts(gid, gd, rows=True)
    wc, wr = want(one.rows(0, n), n, gid, gd, int(gid.max()) + 1, 77)
    assert np.array_equal(ref["counts"], wc) and np.array_equal(ref["row_counts"], wr)
    one.close()
    grp = MultiBuild(t, 2, devices=[0, 0])
    got = grp.group_counts(gid, gd, rows=True)
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], ref["counts"])
    assert got["row_counts"].dtype == np.int32
    assert np.array_equal(got["row_counts"], ref["row_counts"])
    assert grp.group_counts(gid, gd)["row_counts"] is None
    m = ReachabilityMatrix.__new__(ReachabilityMatrix)
    m.container_size, m._engine = n, grp
    table = alg.group_reachability(m, cs, obj["label"])
    assert np.array_equal(table.counts.sum(axis=1), ref["counts"].sum(axis=1))
    assert alg.reach_count(m, range(n), range(n)) == int(ref["counts"].sum())
    grp.close()
