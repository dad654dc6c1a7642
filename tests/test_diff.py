"""matrix_diff (kano_diff / kano_diff_pairs / kano_copy_matrix and the layers
above them): for two matrices A and B over the same pods and rows,
added = B & ~A and removed = A & ~B, as totals, per-row counts, per-column
flags and (i, j) pair lists.  The expectation everywhere is `want` below, a
numpy restatement on the unpacked bits.  Exact integers throughout.
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


def want(A, B, n, r0=0):
    """The definition on the unpacked words of A and B (rows r0.. of both)."""
    a, b = unpack(A, n), unpack(B, n)
    added, removed = b & ~a, a & ~b
    out = {}
    for name, m in (("added", added), ("removed", removed)):
        out[name] = int(m.sum())
        out["row_" + name] = m.sum(axis=1).astype(np.int64)
        out["col_" + name] = np.flatnonzero(m.any(axis=0)).tolist()
        out["pairs_" + name] = (np.argwhere(m) + np.array([r0, 0])).astype(np.int32)
    return out


def flags(words, n):
    return np.flatnonzero(unpack(np.asarray(words).reshape(1, -1), n)[0]).tolist()


def random_words(rng, rows, n, density):
    """Random rows; the bits past n in the last word are random too."""
    W = (n + 63) // 64
    bits = rng.random((rows, W * 64)) < density
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(rows, W)


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "kano_hip.h")) as f:
        text = f.read()
    for name in ("kano_diff", "kano_diff_pairs", "kano_copy_matrix"):
        assert re.search(r"^int %s\(kano_ctx\*" % name, text, re.M), name


def test_native_binds_the_entry_points():
    from kano import _native as nat
    for name in ("kano_diff", "kano_diff_pairs", "kano_copy_matrix"):
        assert name in nat.SIGNATURES
    assert len(nat.SIGNATURES["kano_diff"][1]) == 7
    assert len(nat.SIGNATURES["kano_diff_pairs"][1]) == 8
    assert len(nat.SIGNATURES["kano_copy_matrix"][1]) == 2
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libkano_hip.so not built")
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in ("kano_diff", "kano_diff_pairs", "kano_copy_matrix"):
        assert getattr(lib, name) is not None


def test_restatement_on_a_hand_written_case():
    #      A        B       added   removed
    # 0: 1 1 0    1 0 1    . . 1    . 1 .
    # 1: 0 0 0    0 1 0    . 1 .    . . .
    # 2: 1 0 1    1 0 1    . . .    . . .
    A = np.array([[0b011], [0b000], [0b101]], np.uint64)
    B = np.array([[0b101], [0b010], [0b101]], np.uint64)
    w = want(A, B, 3)
    assert (w["added"], w["removed"]) == (2, 1)
    assert w["row_added"].tolist() == [1, 1, 0] and w["row_removed"].tolist() == [1, 0, 0]
    assert w["col_added"] == [1, 2] and w["col_removed"] == [1]
    assert w["pairs_added"].tolist() == [[0, 2], [1, 1]]
    assert w["pairs_removed"].tolist() == [[0, 1]]
    # the same numbers in the API's result type
    from kano.algorithm import MatrixDiff
    d = MatrixDiff(*(w[k] for k in MatrixDiff._fields))
    assert (d.added, d.removed, d.equal) == (2, 1, False)
    assert MatrixDiff(*(want(A, A, 3)[k] for k in MatrixDiff._fields)).equal
    # bits past n are no part of either matrix
    A[0, 0] |= np.uint64(1 << 3)
    assert want(A, B, 3)["removed"] == 1
    assert want(A, B, 3, r0=5)["pairs_added"].tolist() == [[5, 2], [6, 1]]


def test_matrix_diff_api_is_exported():
    from kano import algorithm as alg
    d = alg.MatrixDiff(0, 0, np.zeros(2, np.int64), np.zeros(2, np.int64), [], [])
    assert d.equal and not d._replace(added=1).equal and not d._replace(removed=1).equal
    assert d._fields == ("added", "removed", "row_added", "row_removed", "col_added",
                         "col_removed")
    assert callable(alg.matrix_diff) and callable(alg.matrix_diff_pairs)


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


def check_against(a, b, A, B, n, r0=0, pairs=True):
    """Every output of a.diff(b) and both pair lists against the restatement."""
    w = want(A, B, n, r0)
    d = a.diff(b)
    assert (d["added"], d["removed"]) == (w["added"], w["removed"])
    for kind in ("added", "removed"):
        assert d["row_" + kind].dtype == np.int32
        assert np.array_equal(d["row_" + kind], w["row_" + kind]), kind
        # (all 64 W bits: nothing at or past n, whatever the caller's words held there)
        assert flags(d["col_" + kind], 64 * len(d["col_" + kind])) == w["col_" + kind], kind
        if pairs:
            got = a.diff_pairs(b, kind, r0, A.shape[0], limit=max(w[kind], 1))
            assert got.dtype == np.int32 and got.shape == (w[kind], 2)
            assert np.array_equal(got, w["pairs_" + kind]), kind
    only = a.diff(b, rows=False, cols=False)      # the totals-only kernel
    assert (only["added"], only["removed"]) == (w["added"], w["removed"])
    assert only["row_added"] is None and only["col_removed"] is None
    return w


@gpu
@pytest.mark.parametrize("density", [0.5, 0.01])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 1000, 1025])
def test_word_and_pitch_edges(n, density, need_gpu):
    rng = np.random.default_rng(1000 * n + int(density * 100))
    A, B = random_words(rng, n, n, density), random_words(rng, n, n, density)
    a, b = engine_of(A, n), engine_of(B, n)
    w = check_against(a, b, A, B, n)
    if n >= 63 and density == 0.5:
        assert w["added"] > 0 and w["removed"] > 0
    a.close()
    b.close()


@gpu
def test_tail_bits_are_not_counted(need_gpu):
    n = 70
    full = np.full((n, 2), np.uint64(0xFFFFFFFFFFFFFFFF))      # bits 70..127 set as well
    zero = np.zeros((n, 2), np.uint64)
    a, b = engine_of(full, n), engine_of(zero, n)
    for x, y, X, Y, gain, loss in ((a, b, full, zero, 0, n * n), (b, a, zero, full, n * n, 0)):
        d = x.diff(y)
        assert (d["added"], d["removed"]) == (gain, loss)
        hit, miss = ("removed", "added") if loss else ("added", "removed")
        assert d["row_" + hit].tolist() == [n] * n and d["row_" + miss].tolist() == [0] * n
        assert flags(d["col_" + hit], 128) == list(range(n))          # none at or past 70
        assert flags(d["col_" + miss], 128) == []
        pairs = x.diff_pairs(y, hit, 0, n, limit=n * n)
        assert pairs.shape == (n * n, 2) and int(pairs[:, 1].max()) == n - 1
        assert x.diff_pairs(y, miss, 0, n).shape == (0, 2)
        check_against(x, y, X, Y, n)
    a.close()
    b.close()


@gpu
def test_degenerate_cases(need_gpu):
    from kano._engine import DeviceBuild
    n = 130
    rng = np.random.default_rng(7)
    A = random_words(rng, n, n, 0.3)
    a, b = engine_of(A, n), engine_of(A, n)
    w = check_against(a, b, A, A, n)                # identical matrices
    assert (w["added"], w["removed"]) == (0, 0)
    d = a.diff(a)                                   # a context against itself
    assert (d["added"], d["removed"]) == (0, 0)
    assert not d["row_added"].any() and not d["col_removed"].any()
    assert a.diff_pairs(a, "removed", 0, n).shape == (0, 2)
    e = DeviceBuild.empty(n)                        # against an empty matrix
    bits = int(unpack(A, n).sum())
    d = a.diff(e)
    assert (d["added"], d["removed"]) == (0, bits)
    assert np.array_equal(d["row_removed"], unpack(A, n).sum(axis=1))
    d = e.diff(a)
    assert (d["added"], d["removed"]) == (bits, 0)
    for x in (a, b, e):
        x.close()
    z0, z1 = DeviceBuild.empty(0), DeviceBuild.empty(0)          # n = 0
    d = z0.diff(z1)
    assert (d["added"], d["removed"]) == (0, 0)
    assert d["row_added"].shape == (0,) and d["col_added"].shape == (0,)
    assert z0.diff_pairs(z1, "added", 0, 0).shape == (0, 2)
    z0.close()
    z1.close()


@gpu
def test_row_extremes(need_gpu):
    n = 200
    rng = np.random.default_rng(11)
    A = random_words(rng, n, n, 0.2)
    A[:, -1] &= np.uint64((1 << (n & 63)) - 1)
    B = A.copy()
    A[17] = 0                                       # full in B, empty in A: four words
    B[17] = np.uint64(0xFFFFFFFFFFFFFFFF)
    B[17, -1] = np.uint64((1 << (n & 63)) - 1)
    B[60, 0] ^= np.uint64(1)                        # bit 0 alone
    B[199, 3] ^= np.uint64(1 << (199 & 63))         # bit 199 alone
    a, b = engine_of(A, n), engine_of(B, n)
    w = check_against(a, b, A, B, n)
    assert w["added"] + w["removed"] == 202
    assert w["row_added"][17] == 200
    assert (w["row_added"] + w["row_removed"]).nonzero()[0].tolist() == [17, 60, 199]
    got = a.diff_pairs(b, "added", 0, n)
    row17 = got[got[:, 0] == 17]
    assert row17[:, 1].tolist() == list(range(200))
    a.close()
    b.close()


@gpu
@pytest.mark.parametrize("tune", ["", "dgrid=7"])
def test_many_rows_per_block_and_several_grid_passes(tune, monkeypatch, need_gpu):
    """3000 rows are 188 work items of 16 rows (one 47-word chunk); at 0.1 %
    most rows and most words hold no difference.  dgrid=7 (KANO_TUNE) caps the
    grid at 7 blocks, 27 passes each; the default grid takes every item at
    once on a whole device."""
    monkeypatch.setenv("KANO_TUNE", tune)
    n = 3000
    rng = np.random.default_rng(3000)
    A = random_words(rng, n, n, 0.001)
    B = A ^ random_words(rng, n, n, 0.001)
    a, b = engine_of(A, n), engine_of(B, n)
    w = check_against(a, b, A, B, n)
    assert w["added"] > 1000 and w["removed"] >= 1
    a.close()
    b.close()


@gpu
@pytest.mark.parametrize("tune", ["", "dgrid=2", "dgrid=5"])
def test_several_column_chunks(tune, monkeypatch, need_gpu):
    """W = 1029: more than 512 words, so three column chunks (352, 352 and 325
    words, the last with an odd end and a tail), 40 rows (3 work items a
    chunk): row counts gathered over the chunks.  With the grid capped a block
    walks from one chunk into the next and hands over its column words in
    between."""
    monkeypatch.setenv("KANO_TUNE", tune)
    n, rows = 65800, (64, 104)
    rng = np.random.default_rng(65800)
    A = random_words(rng, 40, n, 0.02)
    B = random_words(rng, 40, n, 0.02)
    a, b = engine_of(A, n, rows=rows), engine_of(B, n, rows=rows)
    check_against(a, b, A, B, n, r0=64)
    a.close()
    b.close()


@gpu
def test_pairs_by_range_and_limit(need_gpu):
    from kano import algorithm as alg
    from kano.model import ReachabilityMatrix
    n = 300
    rng = np.random.default_rng(300)
    A, B = random_words(rng, n, n, 0.05), random_words(rng, n, n, 0.05)
    a, b = engine_of(A, n), engine_of(B, n)
    w = want(A, B, n)
    for kind in ("added", "removed"):
        full = w["pairs_" + kind]
        for r0, nrows in ((0, 300), (0, 1), (299, 1), (17, 100), (5, 0)):
            sel = full[(full[:, 0] >= r0) & (full[:, 0] < r0 + nrows)]
            assert np.array_equal(a.diff_pairs(b, kind, r0, nrows), sel), (kind, r0, nrows)
            assert a.diff_count(b, kind, r0, nrows) == sel.shape[0]
    count = w["added"]
    lib = a.lib
    cnt = ctypes.c_int64(-1)
    assert lib.kano_diff_pairs(a.ctx, b.ctx, 0, 0, n, 0, ctypes.byref(cnt), None) == 0
    assert cnt.value == count                       # pairs = NULL: the count alone
    buf = np.full((count, 2), -7, np.int32)
    cnt = ctypes.c_int64(-1)
    assert lib.kano_diff_pairs(a.ctx, b.ctx, 0, 0, n, count, ctypes.byref(cnt),
                               buf.ctypes.data) == 0
    assert cnt.value == count and np.array_equal(buf, w["pairs_added"])
    buf[:] = -7
    cnt = ctypes.c_int64(-1)
    rc = lib.kano_diff_pairs(a.ctx, b.ctx, 0, 0, n, count - 1, ctypes.byref(cnt),
                             buf.ctypes.data)
    assert rc == -errno.ENOSPC and cnt.value == count
    assert (buf == -7).all()                        # no pair written
    with pytest.raises(OverflowError, match=str(count)):
        a.diff_pairs(b, "added", 0, n, limit=count - 1)

    def as_matrix(eng):
        m = ReachabilityMatrix.__new__(ReachabilityMatrix)
        m.container_size, m._engine = n, eng
        return m
    ma, mb = as_matrix(a), as_matrix(b)
    with pytest.raises(OverflowError, match=str(count)):
        alg.matrix_diff_pairs(ma, mb, limit=count - 1)
    assert np.array_equal(alg.matrix_diff_pairs(ma, mb, limit=count), w["pairs_added"])
    assert np.array_equal(alg.matrix_diff_pairs(ma, mb, kind="removed", rows=(17, 117)),
                          w["pairs_removed"][(w["pairs_removed"][:, 0] >= 17) &
                                             (w["pairs_removed"][:, 0] < 117)])
    with pytest.raises(ValueError):
        alg.matrix_diff_pairs(ma, mb, kind="changed")
    with pytest.raises(ValueError):
        alg.matrix_diff_pairs(ma, mb, rows=(0, 301))
    d = alg.matrix_diff(ma, mb)
    assert (d.added, d.removed, d.equal) == (w["added"], w["removed"], False)
    assert d.row_added.dtype == np.int64 and np.array_equal(d.row_removed, w["row_removed"])
    assert d.col_added == w["col_added"] and d.col_removed == w["col_removed"]
    other = as_matrix(engine_of(np.zeros((100, 2), np.uint64), 100))
    other.container_size = 100
    with pytest.raises(ValueError):
        alg.matrix_diff(ma, other)
    with pytest.raises(ValueError):
        alg.matrix_diff_pairs(other, mb)
    for m in (ma, mb, other):
        m._engine.close()


@gpu
def test_totals_are_64_bit(need_gpu):
    """70,000 pods of one label, one policy selecting and allowing all of
    them: B is all ones, A empty, 4.9e9 added pairs."""
    from kano import model
    from kano._engine import DeviceBuild
    from kano._intern import intern
    n = 70000
    cs = [model.Container(f"p{i}", {"app": "a"}) for i in range(n)]
    ps = [model.Policy("all", model.PolicySelect({"app": "a"}), model.PolicyAllow({"app": "a"}),
                       model.PolicyIngress, model.PolicyProtocol([]))]
    b = DeviceBuild(intern(cs, ps))
    a = DeviceBuild.empty(n)
    assert n * n > 2 ** 32
    d = a.diff(b)
    assert (d["added"], d["removed"]) == (n * n, 0)
    assert d["row_added"].min() == n == d["row_added"].max() and not d["row_removed"].any()
    assert flags(d["col_added"], len(d["col_added"]) * 64) == list(range(n))
    assert not d["col_removed"].any()
    only = a.diff(b, rows=False, cols=False)
    assert (only["added"], only["removed"]) == (n * n, 0)
    assert b.diff(a, rows=False, cols=False)["removed"] == n * n
    assert a.diff_count(b, "added", 0, n) == n * n          # counted, not fetched
    a.close()
    b.close()


@gpu
def test_error_codes_leave_both_contexts_usable(need_gpu):
    from kano import _native as nat
    from kano._engine import DeviceBuild
    rng = np.random.default_rng(5)
    n = 128
    A, B = random_words(rng, n, n, 0.3), random_words(rng, n, n, 0.3)
    a, b = engine_of(A, n), engine_of(B, n)
    small = DeviceBuild.empty(100)
    lo = DeviceBuild.empty(n, rows=(0, 64))
    hi = DeviceBuild.empty(n, rows=(64, 128))
    lib = a.lib
    tot = np.zeros(2, np.int64)
    cnt = ctypes.c_int64(-1)
    EINVAL = -errno.EINVAL
    assert lib.kano_diff(a.ctx, small.ctx, tot.ctypes.data, None, None, None, None) == EINVAL
    assert lib.kano_diff(lo.ctx, hi.ctx, tot.ctypes.data, None, None, None, None) == EINVAL
    assert lib.kano_diff(a.ctx, lo.ctx, tot.ctypes.data, None, None, None, None) == EINVAL
    assert lib.kano_diff(None, b.ctx, tot.ctypes.data, None, None, None, None) == EINVAL
    assert lib.kano_diff(a.ctx, None, tot.ctypes.data, None, None, None, None) == EINVAL
    assert lib.kano_diff_pairs(a.ctx, b.ctx, 2, 0, n, 0, ctypes.byref(cnt), None) == EINVAL
    assert cnt.value == 0                            # *count is always set
    assert lib.kano_diff_pairs(a.ctx, b.ctx, -1, 0, n, 0, ctypes.byref(cnt), None) == EINVAL
    for r0, nrows in ((0, n + 1), (-1, 2), (n, 1), (5, -1)):
        assert lib.kano_diff_pairs(a.ctx, b.ctx, 0, r0, nrows, 0, ctypes.byref(cnt),
                                   None) == EINVAL, (r0, nrows)
    assert lib.kano_diff_pairs(lo.ctx, lo.ctx, 0, 60, 8, 0, ctypes.byref(cnt), None) == EINVAL
    assert lib.kano_diff_pairs(a.ctx, b.ctx, 0, 0, n, -1, ctypes.byref(cnt), None) == EINVAL
    assert lib.kano_copy_matrix(a.ctx, a.ctx) == EINVAL
    assert lib.kano_copy_matrix(a.ctx, small.ctx) == EINVAL
    assert lib.kano_copy_matrix(lo.ctx, hi.ctx) == EINVAL
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b"):
        a.diff(small)
    # both contexts still answer
    check_against(a, b, A, B, n)
    assert lo.diff(lo)["added"] == 0 and small.diff(small)["removed"] == 0
    # and a copy makes the difference empty
    b.copy_from(a)
    check_against(a, b, A, A, n)
    assert np.array_equal(b.rows(0, n), A)
    for x in (a, b, small, lo, hi):
        x.close()


@gpu
def test_nothing_else_moves(need_gpu):
    """kano_diff and kano_diff_pairs write their own buffers only: the rows
    and the column checks of both builds are what they were."""
    import test_redundancy as tr
    from kano._engine import DeviceBuild
    from kano._intern import intern
    obj = cluster("s_sparse_200")
    a = DeviceBuild(tr.cluster_tables("s_sparse_200"))
    b = DeviceBuild(intern(*tr.api_objects(dict(obj, policies=obj["policies"][1:]))))
    n = a.n
    before = [(e.rows_digest(0, n).copy(), [x.copy() for x in e.col_checks()], e.shadow_count())
              for e in (a, b)]
    d = a.diff(b)
    assert d["added"] == 0 and d["removed"] == tr.record("s_sparse_200")["impact"][0] > 0
    assert a.diff_pairs(b, "removed", 0, n).shape[0] == d["removed"]
    assert b.diff(a)["added"] == d["removed"]
    for e, (dig, cols, shadow) in zip((a, b), before):
        assert np.array_equal(e.rows_digest(0, n), dig)
        assert all(np.array_equal(x, y) for x, y in zip(e.col_checks(), cols))
        assert e.shadow_count() == shadow
    assert a.policy_impact().tolist() == tr.record("s_sparse_200")["impact"]
    a.close()
    b.close()


@gpu
@pytest.mark.parametrize("name", ["paper_example", "q_shadow", "s_sparse_50"])
def test_removing_a_policy_removes_its_impact(name, need_gpu):
    import test_redundancy as tr
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg

    def objects():
        if name == "paper_example":
            from sample import paper_example
            return paper_example()
        return tr.api_objects(cluster(name))

    impact = tr.record(name)["impact"]
    for p in range(len(impact)):
        cs, ps = objects()
        m = ReachabilityMatrix.build_matrix(cs, ps)
        before = m.snapshot()
        held = m.row_bytes().copy()
        assert np.array_equal(before.row_bytes(), held)
        m.remove_policies([p])
        d = alg.matrix_diff(before, m)
        assert (d.removed, d.added) == (impact[p], 0), p
        assert d.equal == (impact[p] == 0)
        assert int(d.row_removed.sum()) == impact[p] and not d.row_added.any()
        assert (d.col_removed == []) == (impact[p] == 0) and d.col_added == []
        back = alg.matrix_diff(m, before)
        assert (back.added, back.removed) == (impact[p], 0)
        assert np.array_equal(back.row_added, d.row_removed)
        assert back.col_added == d.col_removed
        pairs = alg.matrix_diff_pairs(before, m, kind="removed")
        assert pairs.shape == (impact[p], 2)
        assert np.array_equal(pairs, alg.matrix_diff_pairs(m, before, kind="added"))
        # the snapshot keeps the rows it was given
        assert np.array_equal(before.row_bytes(), held)
        assert np.array_equal(before.row_bytes(), m.row_bytes()) == (impact[p] == 0)


@gpu
def test_adding_a_policy_removes_nothing(need_gpu):
    import test_redundancy as tr
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    name = "s_sparse_200"
    obj = cluster(name)
    impact = tr.record(name)["impact"]
    cs, ps = tr.api_objects(dict(obj, policies=obj["policies"][1:]))
    m = ReachabilityMatrix.build_matrix(cs, ps)
    before = m.snapshot()
    held = before.row_bytes().copy()
    new = tr.api_objects(dict(obj, policies=obj["policies"][:1]))[1][0]
    m.add_policies([new])
    d = alg.matrix_diff(before, m)
    assert d.removed == 0 and d.added == impact[0] > 0     # the pairs only policy 0 allows
    assert d.col_removed == [] and len(d.col_added) > 0
    assert np.array_equal(before.row_bytes(), held)
    bits = lambda x: int(np.unpackbits(x).sum())           # noqa: E731
    assert bits(m.row_bytes()) - bits(held) == d.added


@gpu
def test_a_matrix_against_its_two_hop(need_gpu):
    import test_redundancy as tr
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = tr.api_objects(cluster("s_sparse_200"))
    m = ReachabilityMatrix.build_matrix(cs, ps)
    t = alg.two_hop(m)
    d = alg.matrix_diff(m, t)
    bits = lambda x: int(np.unpackbits(x).sum())           # noqa: E731
    assert d.removed == 0
    assert d.added == bits(t.row_bytes()) - bits(m.row_bytes())
    assert alg.matrix_diff(t, t.snapshot()).equal


@functools.lru_cache(maxsize=None)
def shard_inputs():
    """s_sparse_2000 and the same cluster without its first policy: the two
    tables and the one-context diff, checked against the restatement."""
    import test_redundancy as tr
    from kano._engine import DeviceBuild
    from kano._intern import intern
    name = "s_sparse_2000"
    obj = cluster(name)
    ta = tr.cluster_tables(name)
    tb = intern(*tr.api_objects(dict(obj, policies=obj["policies"][1:])))
    a, b = DeviceBuild(ta), DeviceBuild(tb)
    n = ta.n
    ref = a.diff(b)
    w = want(a.rows(0, n), b.rows(0, n), n)
    assert (ref["added"], ref["removed"]) == (w["added"], w["removed"])
    assert ref["removed"] == tr.record(name)["impact"][0] > 0 and ref["added"] == 0
    assert np.array_equal(ref["row_removed"], w["row_removed"])
    assert flags(ref["col_removed"], n) == w["col_removed"]
    pairs = a.diff_pairs(b, "removed", 0, n)
    assert np.array_equal(pairs, w["pairs_removed"])
    a.close()
    b.close()
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    pairs.setflags(write=False)
    return ta, tb, ref, pairs


@gpu
@pytest.mark.parametrize("G", [2, 3])
def test_row_shards_add_up(G, need_gpu):
    from kano import algorithm as alg
    from kano._engine import DeviceBuild
    from kano.model import ReachabilityMatrix
    from kano.multi import MultiBuild
    ta, tb, ref, ref_pairs = shard_inputs()
    n = ta.n
    even = [(n * g // G, n * (g + 1) // G) for g in range(G)]
    skewed = [(g, g + 1) for g in range(G - 1)] + [(G - 1, n)]
    for bounds in (even, skewed):
        tot = np.zeros(2, np.int64)
        rows = {k: [] for k in ("row_added", "row_removed")}
        cols = {k: np.zeros_like(ref[k]) for k in ("col_added", "col_removed")}
        pairs = []
        for r0, r1 in bounds:
            a, b = DeviceBuild(ta, rows=(r0, r1)), DeviceBuild(tb, rows=(r0, r1))
            d = a.diff(b)
            tot += (d["added"], d["removed"])
            for k in rows:
                assert d[k].shape == (r1 - r0,)
                rows[k].append(d[k])
            for k in cols:
                cols[k] |= d[k]
            pairs.append(a.diff_pairs(b, "removed", r0, r1 - r0))
            a.close()
            b.close()
        assert tot.tolist() == [ref["added"], ref["removed"]]
        for k in rows:
            assert np.array_equal(np.concatenate(rows[k]), ref[k])
        for k in cols:
            assert np.array_equal(cols[k], ref[k])
        assert np.array_equal(np.concatenate(pairs), ref_pairs)
    ga, gb = MultiBuild(ta, G, devices=[0] * G), MultiBuild(tb, G, devices=[0] * G)
    d = ga.diff(gb)
    assert (d["added"], d["removed"]) == (ref["added"], ref["removed"])
    for k in ("row_added", "row_removed", "col_added", "col_removed"):
        assert np.array_equal(d[k], ref[k]), k
    assert np.array_equal(ga.diff_pairs(gb, "removed", 0, n), ref_pairs)
    assert np.array_equal(ga.diff_pairs(gb, "removed", 100, 1500),
                          ref_pairs[(ref_pairs[:, 0] >= 100) & (ref_pairs[:, 0] < 1600)])

    def as_matrix(eng):
        m = ReachabilityMatrix.__new__(ReachabilityMatrix)
        m.container_size, m._engine = n, eng
        return m
    md = alg.matrix_diff(as_matrix(ga), as_matrix(gb))
    assert (md.added, md.removed) == (ref["added"], ref["removed"])
    assert np.array_equal(md.row_removed, ref["row_removed"])
    assert md.col_removed == flags(ref["col_removed"], n) and md.col_added == []
    assert np.array_equal(alg.matrix_diff_pairs(as_matrix(ga), as_matrix(gb), kind="removed"),
                          ref_pairs)
    snap = as_matrix(ga).snapshot()
    assert alg.matrix_diff(snap, as_matrix(ga)).equal
    assert alg.matrix_diff(snap, as_matrix(gb)).removed == ref["removed"]
    snap._engine.close()
    other = MultiBuild(tb, 5 - G, devices=[0] * (5 - G))
    with pytest.raises(ValueError):
        ga.diff(other)
    with pytest.raises(ValueError):
        ga.diff_pairs(other, "removed", 0, n)
    with pytest.raises(ValueError):
        alg.matrix_diff(as_matrix(ga), as_matrix(other))
    for g in (ga, gb, other):
        g.close()
