"""hop_distance / path_witness (kano_hops, kano_hop_pairs and the layers above
them): shortest paths over the matrix read as a graph, an edge i -> j iff
M[i, j] = 1.
  dist(s, t) = the least k >= 1 such that a walk of k edges leads from s to t,
               -1 if there is none (or none within max_hops; 0 = no bound)
  witness    = [s, t_1, .., t_{d-1}, t], t_{k-1} the smallest pod of level
               k - 1 with an edge to t_k
The expectation everywhere is `levels` / `witness` below, a numpy restatement
of the level sets on the unpacked bits.  Exact integers throughout.
"""
import ctypes
import errno
import functools
import os
import re

import numpy as np
import pytest

from _golden import cluster, rows01_to_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"kano_hops": 6, "kano_hop_pairs": 7, "kano_hop_pairs_fetch": 2,
                "kano_hops_time": 2}
PAPER_ROWS = ["11010", "10010", "10010", "01000", "00100"]


def unpack(words, n):
    """(rows, W) u64 words -> (rows, n) bool; bits at positions >= n dropped."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    w = w.reshape(w.shape[0], -1)
    if w.shape[1] == 0:
        return np.zeros((w.shape[0], n), bool)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def random_words(rng, n, density, tail=False):
    """n random rows of n bits; with ``tail`` the bits past n are random too."""
    W = (n + 63) // 64
    if density >= 1.0:
        bits = np.ones((n, W * 64), bool)
    else:
        bits = rng.random((n, W * 64)) < density
    if not tail:
        bits[:, n:] = False
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(n, W)


def levels(B, s, max_hops=0):
    """The definition: L_0 = {s}, V_0 = {}, L_k = (OR of row(u), u in L_{k-1})
    minus V_{k-1}; dist = k on L_k (k >= 1), -1 elsewhere.  B: (n, n) bool."""
    n = B.shape[0]
    dist = np.full(n, -1, np.int32)
    front = np.zeros(n, bool)
    front[s] = True
    visited = np.zeros(n, bool)
    k = 0
    while front.any() and (max_hops == 0 or k < max_hops):
        k += 1
        new = B[front].any(axis=0) & ~visited
        dist[new] = k
        visited |= new
        front = new
    return dist


def witness(B, dist, s, t):
    """The canonical shortest path from s to t; dist = levels(B, s)."""
    d = int(dist[t])
    if d < 1:
        return []
    path = [int(t)]
    for k in range(d, 1, -1):
        cand = np.flatnonzero((dist == k - 1) & B[:, path[0]])
        path.insert(0, int(cand[0]))
    return [int(s)] + path


def all_levels(B, sources=None, max_hops=0):
    n = B.shape[0]
    src = range(n) if sources is None else sources
    out = [levels(B, int(s), max_hops) for s in src]
    return np.stack(out) if out else np.zeros((0, n), np.int32)


def bool_hops(B, k):
    """Pairs joined by a walk of 1..k edges (k = 0: of any length >= 1), by
    numpy boolean products."""
    R = B.copy()
    step = 1
    while k == 0 or step < k:
        Rn = R | ((R.astype(np.int64) @ B.astype(np.int64)) > 0)
        step += 1
        if (Rn == R).all():
            break
        R = Rn
    return R


def paper_bits():
    return unpack(rows01_to_words(PAPER_ROWS, 5), 5)


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "kano_hip.h")) as f:
        text = f.read()
    for name in ENTRY_POINTS:
        assert re.search(r"^int %s\(kano_ctx\*" % name, text, re.M), name


def test_native_binds_the_entry_points():
    from kano import _native as nat
    for name, arity in ENTRY_POINTS.items():
        assert len(nat.SIGNATURES[name][1]) == arity, name
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libkano_hip.so not built")
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in ENTRY_POINTS:
        assert getattr(lib, name) is not None


def test_api_is_exported_and_of_slices():
    from kano import algorithm as alg
    for name in ("hop_levels", "hop_distance", "path_witnesses", "path_witness"):
        assert callable(getattr(alg, name)), name
    assert alg.HopPaths._fields == ("dist", "offsets", "nodes")
    p = alg.HopPaths(np.array([2, -1, 1], np.int32), np.array([0, 3, 3, 5], np.int64),
                     np.array([4, 2, 0, 7, 7], np.int32))
    assert p.of(0) == [4, 2, 0] and p.of(1) == [] and p.of(2) == [7, 7] == p.of(-1)
    assert all(type(v) is int for v in p.of(0))
    for q in (3, -4):
        with pytest.raises(IndexError):
            p.of(q)
    from kano._engine import DeviceBuild
    from kano.multi import MultiBuild
    for cls in (DeviceBuild, MultiBuild):
        for name in ("hops", "hop_pairs", "hops_time"):
            assert callable(getattr(cls, name)), (cls, name)


@pytest.mark.parametrize("n,density", [(1, 1.0), (1, 0.0), (5, 0.3), (64, 0.05), (65, 0.03),
                                       (130, 0.01), (130, 1.0), (200, 0.2), (200, 0.004)])
def test_restatement_against_boolean_products(n, density):
    """(1 <= dist <= k) is the k-hop matrix for k = 1, 2, 3 and the closure
    for k = 0: the yardstick pinned without a GPU."""
    rng = np.random.default_rng(n * 1000 + int(density * 1000))
    M = random_words(rng, n, density)
    B = unpack(M, n)
    D = all_levels(B)
    assert D.dtype == np.int32 and D.shape == (n, n)
    assert ((D == -1) | (D >= 1)).all()
    for k in (1, 2, 3, 0):
        want = bool_hops(B, k)
        assert np.array_equal((D >= 1) & ((D <= k) if k else True), want), k
        if k:       # the bound cuts the same search short
            Dk = all_levels(B, max_hops=k)
            assert np.array_equal(Dk, np.where(D <= k, D, -1)), k
    so = os.path.join(ROOT, "oracle", "liboracle.so")
    if os.path.exists(so):
        from oracle import kano_oracle as orc
        for k in (2, 3, 0):
            P, _ = orc.path_c(M, n, k)
            assert np.array_equal((D >= 1) & ((D <= k) if k else True), unpack(P, n)), k
    # every witness is a shortest path of edges, rebuilt from the level sets
    for s in range(0, n, max(1, n // 7)):
        for t in range(n):
            p = witness(B, D[s], s, t)
            if D[s, t] < 1:
                assert p == []
                continue
            assert len(p) == D[s, t] + 1 and p[0] == s and p[-1] == t
            assert all(B[a, b] for a, b in zip(p, p[1:]))


def test_restatement_on_chain_and_ring():
    n = 300
    chain = np.zeros((n, n), bool)
    chain[np.arange(n - 1), np.arange(1, n)] = True
    d = levels(chain, 0)
    assert d.tolist() == [-1] + list(range(1, n))
    assert levels(chain, 0, 5).tolist() == [-1, 1, 2, 3, 4, 5] + [-1] * (n - 6)
    assert witness(chain, d, 0, n - 1) == list(range(n))
    ring = chain.copy()
    ring[n - 1, 0] = True
    d = levels(ring, 0)
    assert d[0] == n and d[1] == 1 and d[n - 1] == n - 1
    assert witness(ring, d, 0, 0) == list(range(n)) + [0]


def test_restatement_on_the_paper_example():
    B = paper_bits()
    assert levels(B, 4).tolist() == [2, 3, 1, 2, -1]
    assert levels(B, 3).tolist() == [2, 1, -1, 2, -1]
    assert levels(B, 0)[0] == 1
    assert witness(B, levels(B, 4), 4, 1) == [4, 2, 0, 1]     # 0 is chosen over 3 at level 2
    assert witness(B, levels(B, 4), 4, 4) == []


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def need_gpu():
    from kano import _native
    if not _native.gpu_available():
        pytest.fail("GPU test run without a usable HIP device / libkano_hip.so")


gpu = pytest.mark.gpu


def matrix_of(words, n):
    from kano.model import BitArray, ReachabilityMatrix
    words = np.ascontiguousarray(words, dtype=np.uint64).reshape(n, -1)
    return ReachabilityMatrix(n, [BitArray.from_words(words[i], n) for i in range(n)])


def engine_of(words, n, rows=None):
    from kano._engine import DeviceBuild
    e = DeviceBuild.empty(n, rows=rows)
    words = np.ascontiguousarray(words, dtype=np.uint64)
    if words.size:
        e.put_rows(rows[0] if rows else 0, words)
    return e


def all_pairs(n):
    i, j = np.divmod(np.arange(n * n), n)
    return np.stack([i, j], axis=1).astype(np.int32)


def check_pairs(got, B, D, pairs):
    """A HopPaths against the reference: D[s] = levels(B, s) for the sources."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    want_d = np.array([D[int(s)][int(t)] for s, t in pairs], np.int32).reshape(-1)
    assert got.dist.dtype == np.int32 and np.array_equal(got.dist, want_d)
    lens = np.where(want_d >= 1, want_d.astype(np.int64) + 1, 0)
    assert got.offsets.dtype == np.int64
    assert np.array_equal(got.offsets, np.r_[0, np.cumsum(lens)])
    assert got.nodes.dtype == np.int32 and got.nodes.shape == (int(lens.sum()),)
    want_nodes = [v for s, t in pairs for v in witness(B, D[int(s)], int(s), int(t))]
    assert np.array_equal(got.nodes, np.array(want_nodes, np.int32))


@gpu
def test_paper_example(need_gpu):
    from kano import algorithm as alg
    from kano.model import ReachabilityMatrix
    from sample import paper_example
    cs, ps = paper_example()
    m = ReachabilityMatrix.build_matrix(cs, ps)
    B = paper_bits()
    assert np.array_equal(unpack(m.engine.rows(0, 5), 5), B)
    d4 = alg.hop_levels(m, 4)
    assert d4.dtype == np.int32 and d4.shape == (5,) and d4.tolist() == [2, 3, 1, 2, -1]
    assert alg.hop_levels(m, 3).tolist() == [2, 1, -1, 2, -1]
    assert alg.hop_distance(m, [(0, 0)]).tolist() == [1]
    assert alg.path_witness(m, 4, 1) == [4, 2, 0, 1]
    assert alg.path_witness(m, 4, 4) == []
    D = all_levels(B)
    assert np.array_equal(alg.hop_levels(m, range(5)), D)
    got = alg.hop_distance(m, all_pairs(5))
    assert got.dtype == np.int32 and np.array_equal(got, D.reshape(-1))
    check_pairs(alg.path_witnesses(m, all_pairs(5)), B, D, all_pairs(5))


@gpu
@pytest.mark.parametrize("n,density", [(1, 1.0), (1, 0.0), (63, 0.03), (63, 0.3), (64, 0.03),
                                       (64, 0.3), (65, 0.03), (65, 0.3), (130, 0.03),
                                       (130, 0.3), (130, 1.0)])
def test_explicit_matrices(n, density, need_gpu):
    from kano import algorithm as alg
    rng = np.random.default_rng(n * 100 + int(density * 100))
    M = random_words(rng, n, density)
    B = unpack(M, n)
    D = all_levels(B)
    m = matrix_of(M, n)
    got = alg.hop_levels(m, range(n))
    assert got.dtype == np.int32 and got.shape == (n, n)
    assert np.array_equal(got, D)
    if n <= 65:
        check_pairs(alg.path_witnesses(m, all_pairs(n)), B, D, all_pairs(n))
        assert np.array_equal(alg.hop_distance(m, all_pairs(n)), D.reshape(-1))


@gpu
def test_tail_bits_are_no_edges(need_gpu):
    n = 70
    M = random_words(np.random.default_rng(70), n, 0.05, tail=True)
    assert (M[:, 1] >> np.uint64(6)).any()                 # bits 70..127 are set somewhere
    e = engine_of(M, n)
    B = unpack(M, n)
    D = all_levels(B)
    r = e.hops(np.arange(n))
    assert np.array_equal(r["dist"], D)
    assert r["info"]["reached"] == int((D >= 1).sum()) and r["info"]["batches"] == 2
    assert r["info"]["levels"] == int(D.max())
    pr = all_pairs(n)
    got = e.hop_pairs(pr, paths=True)
    from kano import algorithm as alg
    check_pairs(alg.HopPaths(got["dist"], got["offsets"], got["nodes"]), B, D, pr)
    e.close()


def shape_bits(kind, n=300):
    B = np.zeros((n, n), bool)
    i = np.arange(n)
    if kind in ("chain", "ring"):
        B[i[:-1], i[1:]] = True
        if kind == "ring":
            B[n - 1, 0] = True
    elif kind == "star":
        B[0, 1:] = True
    elif kind == "cliques":
        B[:n // 2, :n // 2] = True
        B[n // 2:, n // 2:] = True
    elif kind == "selfloop":
        B[7, 7] = True
    return B


def words_of(B):
    n = B.shape[0]
    pad = np.zeros((n, (n + 63) // 64 * 64), bool)
    pad[:, :n] = B
    return np.packbits(pad, axis=1, bitorder="little").view("<u8").reshape(n, -1)


@gpu
@pytest.mark.parametrize("kind", ["chain", "ring", "star", "cliques", "selfloop"])
def test_shapes_that_stress_the_level_loop(kind, need_gpu):
    from kano import algorithm as alg
    n = 300
    B = shape_bits(kind, n)
    e = engine_of(words_of(B), n)
    src = [0, 7, 150, n - 1]
    D = {s: levels(B, s) for s in src}
    r = e.hops(src)
    assert np.array_equal(r["dist"], np.stack([D[s] for s in src]))
    pairs = [(s, t) for s in src for t in (0, 1, 7, 149, 150, n - 1)]
    got = e.hop_pairs(pairs, paths=True)
    check_pairs(alg.HopPaths(got["dist"], got["offsets"], got["nodes"]), B, D, pairs)
    if kind == "chain":
        assert r["info"]["levels"] == n - 1 and r["dist"][0, n - 1] == n - 1
        cut = e.hops([0], max_hops=5)
        assert np.array_equal(cut["dist"][0], levels(B, 0, 5)) and cut["info"]["levels"] == 5
        assert cut["dist"][0].tolist() == [-1, 1, 2, 3, 4, 5] + [-1] * (n - 6)
    if kind == "ring":
        assert r["dist"][0, 0] == n and r["info"]["levels"] == n
        assert got["nodes"][got["offsets"][0]:got["offsets"][1]].tolist() == list(range(n)) + [0]
    if kind == "star":
        assert r["info"]["levels"] == 1 and r["info"]["reached"] == n - 1
        assert r["info"]["rows_ored"] == 1 + (n - 1) + 3     # the leaves' empty rows, once
    if kind == "cliques":
        assert r["dist"][0, n - 1] == -1 and r["dist"][3, 0] == -1 and r["dist"][0, 0] == 1
    if kind == "selfloop":
        assert r["dist"][1].tolist() == [-1] * 7 + [1] + [-1] * (n - 8)
        assert int((r["dist"] >= 0).sum()) == 1
    e.close()


@functools.lru_cache(maxsize=None)
def wide_case():
    """n = 5000 is 79 words a row; density 0.0005 is 2.5 edges a pod, so the
    frontiers grow over several levels to thousands of pods."""
    n = 5000
    rng = np.random.default_rng(5000)
    M = random_words(rng, n, 0.0005)
    B = unpack(M, n)
    src = rng.choice(n, size=70, replace=False)
    pairs = np.stack([rng.choice(src[:40], size=2000), rng.integers(0, n, 2000)], axis=1)
    pairs[1000:1100] = pairs[:100]                          # duplicates, unsorted
    D = {int(s): levels(B, int(s)) for s in src}
    for a in (M, B, src, pairs):
        a.setflags(write=False)
    return n, M, B, src, pairs.astype(np.int32), D


@gpu
def test_several_chunks_slices_and_batches(need_gpu):
    from kano import algorithm as alg
    n, M, B, src, pairs, D = wide_case()
    e = engine_of(M, n)
    r = e.hops(src)
    assert np.array_equal(r["dist"], np.stack([D[int(s)] for s in src]))
    assert r["info"]["batches"] == 2
    assert r["info"]["reached"] == sum(int((D[int(s)] >= 1).sum()) for s in src)
    assert max(int((d == k).sum()) for d in D.values() for k in range(1, 9)) > 64   # > 1 slice
    got = e.hop_pairs(pairs, paths=True)
    paths = alg.HopPaths(got["dist"], got["offsets"], got["nodes"])
    rows = unpack(e.rows(0, n), n)
    reachable = 0
    for q, (s, t) in enumerate(pairs.tolist()):               # structurally, from the device's rows
        p = paths.of(q)
        if paths.dist[q] < 1:
            assert p == []
            continue
        reachable += 1
        assert p[0] == s and p[-1] == t and len(p) == paths.dist[q] + 1
        assert all(rows[a, b] for a, b in zip(p, p[1:]))
    assert 100 < reachable
    check_pairs(paths, B, D, pairs)                           # and the canonical path itself
    assert np.array_equal(e.hop_pairs(pairs)["dist"], paths.dist)
    e.close()


def built(name, drop_first=False):
    import test_redundancy as tr
    from kano.model import ReachabilityMatrix
    obj = cluster(name)
    if drop_first:
        obj = dict(obj, policies=obj["policies"][1:])
    cs, ps = tr.api_objects(obj)
    return ReachabilityMatrix.build_matrix(cs, ps)


def agrees_with_the_path_relation(m):
    """For 16 sources, (1 <= hop_levels <= k) equals the rows of k_hop(m, k),
    k = 2, 3, and of transitive_closure(m), as those return them."""
    from kano import algorithm as alg
    n = m.container_size
    src = np.unique(np.linspace(0, n - 1, 16).astype(np.int64))
    D = alg.hop_levels(m, src)
    assert D.shape == (len(src), n)
    B = unpack(m.engine.rows(0, n), n)
    assert np.array_equal(D, all_levels(B, src))
    for k in (2, 3, 0):
        pm = alg.k_hop(m, k) if k else alg.transitive_closure(m)
        rows = unpack(pm.engine.rows(0, n), n)[src]
        assert np.array_equal((D >= 1) & ((D <= k) if k else True), rows), k
    return D


@gpu
@pytest.mark.parametrize("name", ["s_sparse_2000", "s_broad_300", "q_dirs"])
def test_agreement_with_the_shipped_path_relation(name, need_gpu):
    m = built(name)
    agrees_with_the_path_relation(m)
    if name == "s_sparse_2000":          # an edited matrix
        m[3, 7] = 1
        m[0, 0] = 0
        agrees_with_the_path_relation(m)


@gpu
def test_after_an_incremental_update(need_gpu):
    import test_redundancy as tr
    name = "s_sparse_2000"
    obj = cluster(name)
    m = built(name, drop_first=True)
    agrees_with_the_path_relation(m)
    new = tr.api_objects(dict(obj, policies=obj["policies"][:1]))[1][0]
    m.add_policies([new])
    agrees_with_the_path_relation(m)
    m.remove_policies([0])
    agrees_with_the_path_relation(m)


@gpu
def test_max_hops(need_gpu):
    from kano import algorithm as alg
    n = 130
    M = random_words(np.random.default_rng(131), n, 0.02)
    m = matrix_of(M, n)
    pr = all_pairs(n)
    full = alg.hop_distance(m, pr)
    assert full.max() > 2
    cut = alg.hop_distance(m, pr, max_hops=2)
    assert np.array_equal(cut, np.where(full > 2, -1, full))
    B = unpack(M, n)
    assert np.array_equal(alg.hop_levels(m, range(n), max_hops=2), all_levels(B, max_hops=2))
    s, t = pr[int(np.argmax(full))]
    assert alg.path_witness(m, s, t, max_hops=2) == []
    assert len(alg.path_witness(m, s, t)) == full.max() + 1


@gpu
def test_errors_and_degenerate_sizes(need_gpu):
    from kano import algorithm as alg
    from kano import _native as nat
    from kano._engine import DeviceBuild
    from kano.model import ReachabilityMatrix
    n = 64
    M = random_words(np.random.default_rng(64), n, 0.1)
    m = matrix_of(M, n)
    for bad in ([(0, n)], [(n, 0)], [(-1, 0)]):
        with pytest.raises(IndexError):
            alg.hop_distance(m, bad)
        with pytest.raises(IndexError):
            alg.path_witnesses(m, bad)
    with pytest.raises(IndexError):
        alg.hop_levels(m, [n])
    with pytest.raises(ValueError):
        alg.hop_distance(m, [(0, 1)], max_hops=-1)
    with pytest.raises(ValueError):
        alg.hop_levels(m, 0, max_hops=-1)
    # empty queries
    assert alg.hop_distance(m, []).shape == (0,)
    assert alg.hop_levels(m, []).shape == (0, n)
    e = alg.path_witnesses(m, np.zeros((0, 2), np.int32))
    assert e.dist.shape == (0,) and e.offsets.tolist() == [0] and e.nodes.shape == (0,)
    z = DeviceBuild.empty(0)
    assert z.hops([])["dist"].shape == (0, 0)
    assert z.hop_pairs([], paths=True)["nodes"].shape == (0,)
    z.close()
    # the ABI's own codes
    eng = m.engine
    lib = eng.lib
    src = np.array([0, n], np.int32)
    dist = np.full((2, n), -7, np.int32)
    info = np.zeros(4, np.int64)
    EINVAL, ERANGE = -errno.EINVAL, -errno.ERANGE
    assert lib.kano_hops(eng.ctx, 2, src.ctypes.data, 0, dist.ctypes.data,
                         info.ctypes.data) == ERANGE
    assert lib.kano_hops(eng.ctx, 1, src.ctypes.data, -1, dist.ctypes.data, None) == EINVAL
    assert lib.kano_hops(None, 1, src.ctypes.data, 0, dist.ctypes.data, None) == EINVAL
    pr = np.array([[0, 1], [2, -1]], np.int32)
    d2 = np.full(2, -7, np.int32)
    total = ctypes.c_int64(-1)
    assert lib.kano_hop_pairs(eng.ctx, 2, pr.ctypes.data, 0, 1, d2.ctypes.data,
                              ctypes.byref(total)) == ERANGE
    assert lib.kano_hop_pairs(eng.ctx, 1, pr.ctypes.data, -1, 0, d2.ctypes.data, None) == EINVAL
    assert lib.kano_hop_pairs(eng.ctx, 1, pr.ctypes.data, 0, 2, d2.ctypes.data, None) == EINVAL
    assert lib.kano_hop_pairs_fetch(eng.ctx, d2.ctypes.data) == EINVAL      # nothing to fetch
    assert (dist == -7).all() and (d2 == -7).all()           # no error wrote a result
    big = DeviceBuild.empty(1 << 14)                         # S * n = 2^28 + n distances
    many = np.zeros((1 << 14) + 1, np.int32)
    assert lib.kano_hops(big.ctx, many.shape[0], many.ctypes.data, 0, dist.ctypes.data,
                         None) == -errno.ENOTSUP
    big.close()
    ms = ctypes.c_float(-1.0)
    assert lib.kano_hops_time(eng.ctx, None) == EINVAL
    assert lib.kano_hops_time(eng.ctx, ctypes.byref(ms)) == 0 and ms.value == 0.0
    # a row shard: the algorithm layer and the ABI both refuse
    half = engine_of(M[:n // 2], n, rows=(0, n // 2))
    hm = ReachabilityMatrix.__new__(ReachabilityMatrix)
    hm.container_size, hm._engine = n, half
    for call in (lambda: alg.hop_levels(hm, 0), lambda: alg.hop_distance(hm, [(0, 1)]),
                 lambda: alg.path_witness(hm, 0, 1)):
        with pytest.raises(ValueError, match="only rows"):
            call()
    assert lib.kano_hops(half.ctx, 1, src.ctypes.data, 0, dist.ctypes.data, None) == EINVAL
    assert lib.kano_hop_pairs(half.ctx, 1, pr.ctypes.data, 0, 0, d2.ctypes.data, None) == EINVAL
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b.*every row"):
        half.hops([0])
    half.close()
    # the context still answers
    B = unpack(M, n)
    assert np.array_equal(alg.hop_levels(m, 5), levels(B, 5))


@gpu
def test_multibuild_delegates_or_refuses(need_gpu):
    import test_redundancy as tr
    from kano.multi import MultiBuild
    name = "s_sparse_200"
    t = tr.cluster_tables(name)
    one = MultiBuild(t, 1, devices=[0])
    n = t.n
    B = unpack(one.rows(0, n), n)
    assert np.array_equal(one.hops([0, n - 1])["dist"], all_levels(B, [0, n - 1]))
    assert np.array_equal(one.hop_pairs([(0, 1)])["dist"], [levels(B, 0)[1]])
    assert one.hops_time() == 0.0
    one.close()
    two = MultiBuild(t, 2, devices=[0, 0])
    for call in (lambda: two.hops([0]), lambda: two.hop_pairs([(0, 1)]), two.hops_time):
        with pytest.raises(ValueError, match="whole matrix on one device"):
            call()
    two.close()


@gpu
def test_matrix_untouched_and_time_recorded(monkeypatch, need_gpu):
    monkeypatch.setenv("KANO_TUNE", "timing=1")
    n = 300
    M = random_words(np.random.default_rng(300), n, 0.01, tail=True)
    e = engine_of(M, n)
    before = e.rows(0, n).copy()
    assert e.hops_time() == 0.0
    e.hops(np.arange(n))
    assert 0.0 < e.hops_time() < 10000.0
    e.hop_pairs(all_pairs(n)[::7], paths=True)
    assert 0.0 < e.hops_time() < 10000.0
    after = e.rows(0, n)
    assert before.tobytes() == after.tobytes() == M.tobytes()
    e.close()
