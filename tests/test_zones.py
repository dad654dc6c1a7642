"""reverse_matrix / reach_zones (kano_reverse, kano_zones and the layers above
them): the matrix read by columns, and the pods that can all reach each other.
  reverse      R[j, i] = M[i, j] over the bits below n, tail bits zero
  kano_zones   label[i]   = min({i} | {j : A[i, j] and B[i, j]})
               fan_out[i] = popcount(A[i]), fan_in[i] = popcount(B[i]),
               cyclic[i]  = A[i, i]
  reach_zones  kano_zones on C = the closure of M and its reverse: label is the
               smallest pod of the strongly connected component
The expectation everywhere is `zones_ref` / `reach_ref` below, a numpy
restatement on the unpacked bits, itself held to an iterative Tarjan and to
planted graphs whose zones are known by construction.  Exact integers
throughout.
"""
import ctypes
import errno
import functools
import os
import re

import numpy as np
import pytest

from _golden import cluster, rows01_to_words, row_digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"kano_reverse": 3, "kano_reverse_time": 2, "kano_zones": 7, "kano_zones_time": 2}
PAPER_ROWS = ["11010", "10010", "10010", "01000", "00100"]
PAPER = dict(label=[0, 0, 2, 0, 4], fan_out=[3, 3, 3, 3, 4], fan_in=[5, 5, 1, 5, 0],
             cyclic=[1, 1, 0, 1, 0])
PLANTED = [([1, 1, 1, 2, 3, 5, 40, 64, 65, 18], 0.3, 1, 200, 10, 7),
           ([1] * 20 + [2] * 10 + [3, 7, 64, 100, 129, 130], 0.15, 2, 473, 36, 16),
           ([1] * 300 + [2, 2, 3, 64, 65, 128, 200], 0.01, 3, 764, 307, 7)]
SHAPES = ["chain", "ring", "star", "cliques"]


def unpack(words, n):
    """(rows, W) u64 words -> (rows, n) bool; bits at positions >= n dropped."""
    w = np.ascontiguousarray(words, dtype=np.uint64)
    w = w.reshape(w.shape[0], -1)
    if w.shape[1] == 0:
        return np.zeros((w.shape[0], n), bool)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def words_of(B):
    """(rows, n) bool -> (rows, W) u64 words, tail bits zero."""
    r, n = B.shape
    pad = np.zeros((r, (n + 63) // 64 * 64), bool)
    pad[:, :n] = B
    return np.packbits(pad, axis=1, bitorder="little").view("<u8").reshape(r, -1)


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


def closure(B):
    """Pairs joined by a walk of any length >= 1, by numpy boolean products
    (squaring: the counts stay below 2^24, exact in float32)."""
    R = B.copy()
    while True:
        f = R.astype(np.float32)
        Rn = R | ((f @ f) > 0)
        if (Rn == R).all():
            return R
        R = Rn


def zones_ref(A, B):
    """The definition of kano_zones on two (n, n) bool matrices."""
    n = A.shape[0]
    both = (A & B) | np.eye(n, dtype=bool)
    return dict(label=np.argmax(both, axis=1).astype(np.int32),
                fan_out=A.sum(axis=1).astype(np.int32), fan_in=B.sum(axis=1).astype(np.int32),
                cyclic=np.diagonal(A).copy())


def reach_ref(M):
    C = closure(M)
    return zones_ref(C, C.T)


def tarjan_labels(M):
    """The smallest member of every pod's strongly connected component, by an
    iterative Tarjan in plain Python (independent of the boolean products)."""
    n = M.shape[0]
    adj = [np.flatnonzero(M[i]).tolist() for i in range(n)]
    index = [-1] * n
    low = [0] * n
    on = [False] * n
    stack, label, counter = [], [-1] * n, 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                index[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on[v] = True
            descended = False
            while k < len(adj[v]):
                w = adj[v][k]
                k += 1
                if index[w] < 0:
                    work.append((v, k))
                    work.append((w, 0))
                    descended = True
                    break
                if on[w]:
                    low[v] = min(low[v], index[w])
            if descended:
                continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                m = min(comp)
                for w in comp:
                    label[w] = m
            if work:
                p = work[-1][0]
                low[p] = min(low[p], low[v])
    return np.array(label, np.int32)


@functools.lru_cache(maxsize=None)
def planted(case):
    """Groups of the given sizes under a random permutation of the pods, a
    ring inside every group of >= 2 pods, and for groups a < b one edge from a
    random member of a to a random member of b with probability p: the zones
    are the groups.  Returns (bits, expected label, restatement)."""
    sizes, p, seed = PLANTED[case][:3]
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    perm = rng.permutation(n)
    groups, at = [], 0
    for s in sizes:
        groups.append(perm[at:at + s])
        at += s
    M = np.zeros((n, n), bool)
    want = np.zeros(n, np.int32)
    for g in groups:
        want[g] = g.min()
        if len(g) >= 2:
            M[g, np.roll(g, -1)] = True
    for a in range(len(groups)):
        for b in range(a + 1, len(groups)):
            if rng.random() < p:
                M[rng.choice(groups[a]), rng.choice(groups[b])] = True
    ref = reach_ref(M)
    for arr in (M, want, *ref.values()):
        arr.setflags(write=False)
    return M, want, ref


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
    return B


def paper_bits():
    return unpack(rows01_to_words(PAPER_ROWS, 5), 5)


def same_zones(got, ref):
    """A Zones (or DeviceBuild.zones' dict) against the restatement."""
    g = got._asdict() if hasattr(got, "_asdict") else got
    assert g["label"].dtype == np.int32 and np.array_equal(g["label"], ref["label"])
    assert g["fan_out"].dtype == np.int32 and np.array_equal(g["fan_out"], ref["fan_out"])
    assert g["fan_in"].dtype == np.int32 and np.array_equal(g["fan_in"], ref["fan_in"])
    assert g["cyclic"].dtype == bool and np.array_equal(g["cyclic"], ref["cyclic"])


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


def test_api_is_exported():
    from kano import algorithm as alg
    for name in ("reverse_matrix", "reach_zones", "zone_graph"):
        assert callable(getattr(alg, name)), name
    assert alg.Zones._fields == ("label", "fan_out", "fan_in", "cyclic")
    assert alg.ZoneGraph._fields == ("reps", "counts")
    from kano._engine import DeviceBuild
    from kano.multi import MultiBuild
    for cls in (DeviceBuild, MultiBuild):
        for name in ("reverse_into", "reverse_time", "zones", "zones_time"):
            assert callable(getattr(cls, name)), (cls, name)


def test_zones_helpers_on_a_hand_written_example():
    from kano.algorithm import Zones
    label = np.array([0, 1, 0, 3, 1, 0, 6, 1], np.int32)      # zones {0,2,5} {1,4,7} {3} {6}
    z = Zones(label, np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(8, bool))
    assert z.reps().dtype == np.int32 and z.reps().tolist() == [0, 1, 3, 6]
    assert z.sizes().tolist() == [3, 3, 1, 1]
    assert z.members(1) == [1, 4, 7] and z.members(3) == [3] and z.members(2) == []
    assert all(type(v) is int for v in z.members(0))
    assert z.nontrivial().tolist() == [0, 1] and z.nontrivial(1).tolist() == [0, 1, 3, 6]
    assert z.nontrivial(4).tolist() == []
    idx = z.index()
    assert idx.dtype == np.int32 and idx.tolist() == [0, 1, 0, 2, 1, 0, 3, 1]
    assert z.index(min_size=2).tolist() == [0, 1, 0, -1, 1, 0, -1, 1]
    assert z.index(min_size=4).tolist() == [-1] * 8


def test_restatement_on_the_paper_example():
    ref = reach_ref(paper_bits())
    for k, v in PAPER.items():
        assert ref[k].astype(np.int64).tolist() == v, k
    assert np.array_equal(tarjan_labels(paper_bits()), ref["label"])


@pytest.mark.parametrize("case", range(len(PLANTED)))
def test_restatement_recovers_the_planted_zones(case):
    sizes, _, _, n, nz, nz2 = PLANTED[case]
    M, want, ref = planted(case)
    assert M.shape == (n, n)
    assert np.array_equal(ref["label"], want)
    assert np.array_equal(tarjan_labels(M), want)
    _, cnt = np.unique(ref["label"], return_counts=True)
    assert len(cnt) == nz == len(sizes) and int((cnt >= 2).sum()) == nz2
    assert sorted(cnt.tolist()) == sorted(sizes)
    C = closure(M)
    assert np.array_equal(ref["fan_out"], C.sum(axis=1)) and np.array_equal(ref["fan_in"], C.sum(axis=0))
    assert np.array_equal(ref["cyclic"], cnt[np.searchsorted(np.unique(want), want)] >= 2)


@pytest.mark.parametrize("kind", SHAPES)
def test_restatement_on_the_shapes(kind):
    n = 300
    B = shape_bits(kind, n)
    ref = reach_ref(B)
    assert np.array_equal(tarjan_labels(B), ref["label"])
    if kind == "chain":
        assert ref["label"].tolist() == list(range(n)) and not ref["cyclic"].any()
        assert ref["fan_out"].tolist() == [n - 1 - i for i in range(n)]
    if kind == "ring":
        assert (ref["label"] == 0).all() and ref["cyclic"].all()
        assert (ref["fan_out"] == n).all() and (ref["fan_in"] == n).all()
    if kind == "cliques":
        assert ref["label"].tolist() == [0] * (n // 2) + [n // 2] * (n - n // 2)


@pytest.mark.parametrize("n,density", [(1, 1.0), (1, 0.0), (65, 0.03), (130, 0.02), (200, 0.01)])
def test_restatement_against_tarjan_on_random_graphs(n, density):
    B = unpack(random_words(np.random.default_rng(n), n, density), n)
    assert np.array_equal(tarjan_labels(B), reach_ref(B)["label"])


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


def rows_of(m):
    n = m.container_size
    return m.engine.rows(0, n)


@gpu
@pytest.mark.parametrize("n,density", [(1, 0.0), (1, 1.0), (63, 0.03), (63, 1.0), (64, 0.03),
                                       (64, 1.0), (65, 0.03), (65, 1.0), (130, 0.0), (130, 0.03),
                                       (130, 1.0), (513, 0.03), (513, 1.0), (1000, 0.0),
                                       (1000, 0.03), (1000, 1.0), (4097, 0.03)])
def test_reverse_of_explicit_matrices(n, density, need_gpu):
    from kano import algorithm as alg
    rng = np.random.default_rng(n * 100 + int(density * 100))
    M = random_words(rng, n, density)
    B = unpack(M, n)
    m = matrix_of(M, n)
    digest = m.engine.rows_digest(0, n).copy()
    r = alg.reverse_matrix(m)
    got = rows_of(r)
    assert got.shape == M.shape and got.tobytes() == words_of(B.T).tobytes()
    assert r.reverse_info["bits"] == int(B.sum())
    assert r.reverse_info["tiles"] == -(-n // 512) * -(-M.shape[1] // 8)
    assert np.array_equal(m.engine.rows_digest(0, n), digest)
    assert np.array_equal(digest, row_digest(M))
    r.engine.close()
    m.engine.close()


@gpu
@pytest.mark.parametrize("n", [70, 513])
def test_random_tail_bits_are_dropped(n, need_gpu):
    M = random_words(np.random.default_rng(n), n, 0.05, tail=True)
    W = M.shape[1]
    assert (M[:, W - 1] >> np.uint64(n - 64 * (W - 1))).any()     # bits past n are set somewhere
    B = unpack(M, n)
    src, dst, back = engine_of(M, n), engine_of(M, n), engine_of(M, n)   # (dst starts with tails)
    info = src.reverse_into(dst)
    assert info["bits"] == int(B.sum())
    assert dst.rows(0, n).tobytes() == words_of(B.T).tobytes()
    dst.reverse_into(back)
    assert back.rows(0, n).tobytes() == words_of(B).tobytes()
    assert src.rows(0, n).tobytes() == M.tobytes()
    for e in (src, dst, back):
        e.close()


def levels(B, s):
    """dist(s, v) by level sets (tests/test_hops.py `levels`, restated)."""
    n = B.shape[0]
    dist = np.full(n, -1, np.int32)
    front = np.zeros(n, bool)
    front[s] = True
    visited = np.zeros(n, bool)
    k = 0
    while front.any():
        k += 1
        new = B[front].any(axis=0) & ~visited
        dist[new] = k
        visited |= new
        front = new
    return dist


def built(name):
    import test_redundancy as tr
    from kano.model import ReachabilityMatrix
    obj = cluster(name)
    cs, ps = tr.api_objects(obj)
    return obj, cs, ps, ReachabilityMatrix.build_matrix(cs, ps)


@gpu
@pytest.mark.parametrize("name", ["paper", "s_sparse_200"])
def test_reverse_of_a_built_matrix_and_column_queries(name, need_gpu):
    from kano import algorithm as alg
    from kano._bits import words_to_bool
    from kano.model import ReachabilityMatrix
    if name == "paper":
        from sample import paper_example
        m = ReachabilityMatrix.build_matrix(*paper_example())
    else:
        m = built(name)[3]
    n = m.container_size
    B = unpack(rows_of(m), n)
    if name == "paper":
        assert np.array_equal(B, paper_bits())
    r = alg.reverse_matrix(m)
    R = rows_of(r)
    assert R.tobytes() == words_of(B.T).tobytes()
    D = alg.hop_levels(r, range(n))
    for t in range(n):
        assert np.array_equal(D[t], levels(B.T, t)), t
    for j in range(0, n, max(1, n // 40)):
        assert np.array_equal(words_to_bool(m.getcol(j).words(), n), unpack(R[j:j + 1], n)[0]), j
    assert np.array_equal(unpack(rows_of(m), n), B)
    r.engine.close()


@functools.lru_cache(maxsize=None)
def two_matrices(n):
    """Two independent random matrices with tail bits set in both, and rows
    with a chosen first common bit: only the diagonal, none, one in the last
    word, one in the first."""
    rng = np.random.default_rng(n + 17)
    A = unpack(random_words(rng, n, 0.1), n)
    B = unpack(random_words(rng, n, 0.1), n)
    W = (n + 63) // 64
    if n > 4:
        i_diag, i_none, i_last = n // 3, n // 2, n - 1
        j_last = 64 * (W - 1)                       # the first bit of the last word
        for i in (i_diag, i_none, i_last):
            B[i] &= ~A[i]
        A[i_diag, i_diag] = B[i_diag, i_diag] = True
        A[i_none, i_none] = False
        A[i_last, j_last] = B[i_last, j_last] = True
    Aw, Bw = words_of(A).copy(), words_of(B).copy()
    if n % 64:
        tail = ~np.uint64(0) << np.uint64(n % 64)
        Aw[:, W - 1] |= tail
        Bw[:, W - 1] |= tail
    ref = zones_ref(A, B)
    if n > 4:
        assert ref["label"][i_diag] == i_diag and ref["cyclic"][i_diag]
        assert ref["label"][i_none] == i_none and not ref["cyclic"][i_none]
        assert ref["label"][i_last] == j_last
    for arr in (Aw, Bw, *ref.values()):
        arr.setflags(write=False)
    return Aw, Bw, ref


@gpu
@pytest.mark.parametrize("n", [1, 65, 130, 513, 4097])
def test_zones_of_two_independent_matrices(n, need_gpu):
    Aw, Bw, ref = two_matrices(n)
    a, b = engine_of(Aw, n), engine_of(Bw, n)
    got = a.zones(b)
    same_zones(got, ref)
    assert got["zones"] == len(np.unique(ref["label"]))
    assert got["moved"] == int((ref["label"] != np.arange(n)).sum())
    quick = a.zones(b, counts=False)
    assert np.array_equal(quick["label"], ref["label"])
    assert quick["fan_out"] is None and quick["fan_in"] is None and quick["cyclic"] is None
    assert (quick["zones"], quick["moved"]) == (got["zones"], got["moved"])
    # a matrix against itself: every pod's first bit at or below its own index
    own = a.zones(a)
    A = unpack(Aw, n)
    same_zones(own, zones_ref(A, A))
    assert a.rows(0, n).tobytes() == Aw.tobytes() and b.rows(0, n).tobytes() == Bw.tobytes()
    a.close()
    b.close()


@gpu
def test_reach_zones_on_the_paper_example(need_gpu):
    from kano import algorithm as alg
    from kano.model import ReachabilityMatrix
    from sample import paper_example
    m = ReachabilityMatrix.build_matrix(*paper_example())
    z = alg.reach_zones(m)
    assert isinstance(z, alg.Zones)
    same_zones(z, reach_ref(paper_bits()))
    for k, v in PAPER.items():
        assert getattr(z, k).astype(np.int64).tolist() == v, k
    assert z.reps().tolist() == [0, 2, 4] and z.members(0) == [0, 1, 3]


@gpu
@pytest.mark.parametrize("case", range(len(PLANTED)))
def test_reach_zones_and_zone_graph_on_planted_graphs(case, need_gpu):
    from kano import algorithm as alg
    sizes, _, _, n, nz, nz2 = PLANTED[case]
    M, want, ref = planted(case)
    m = matrix_of(words_of(M), n)
    z = alg.reach_zones(m)
    assert np.array_equal(z.label, want)
    same_zones(z, ref)
    assert len(z.reps()) == nz and len(z.nontrivial()) == nz2
    assert sorted(z.sizes().tolist()) == sorted(sizes)
    c = alg.transitive_closure(m)
    same_zones(alg.reach_zones(m, closure=c), ref)
    assert np.array_equal(unpack(rows_of(c), n), closure(M))       # the caller's closure is left alone
    c.engine.close()
    # the graph between the zones, on M's own edges
    for min_size in (1, 2):
        g = alg.zone_graph(m, z, min_size=min_size)
        idx = z.index(min_size)
        Z = int(idx.max()) + 1
        assert np.array_equal(g.reps, z.nontrivial(min_size)) and len(g.reps) == Z
        assert Z == (nz if min_size == 1 else nz2)
        i, j = np.nonzero(M)
        keep = (idx[i] >= 0) & (idx[j] >= 0)
        wc = np.zeros((Z, Z), np.int64)
        np.add.at(wc, (idx[i][keep], idx[j][keep]), 1)
        assert g.counts.dtype == np.int64 and np.array_equal(g.counts, wc)
        if min_size == 1:
            off = g.counts > 0
            np.fill_diagonal(off, False)
            assert not np.diagonal(closure(off)).any()              # acyclic between zones
            assert int(g.counts.sum()) == int(M.sum())
    m.engine.close()


@gpu
@pytest.mark.parametrize("kind", SHAPES)
def test_reach_zones_on_the_shapes(kind, need_gpu):
    from kano import algorithm as alg
    n = 300
    B = shape_bits(kind, n)
    m = matrix_of(words_of(B), n)
    z = alg.reach_zones(m)
    same_zones(z, reach_ref(B))
    if kind == "chain":
        assert z.label.tolist() == list(range(n)) and not z.cyclic.any()
        assert z.fan_out.tolist() == [n - 1 - i for i in range(n)]
    if kind == "ring":
        assert (z.label == 0).all() and z.cyclic.all()
        assert (z.fan_out == n).all() and (z.fan_in == n).all()
    if kind == "star":
        assert z.label.tolist() == list(range(n)) and z.fan_in.tolist() == [0] + [1] * (n - 1)
    if kind == "cliques":
        assert z.reps().tolist() == [0, n // 2] and z.sizes().tolist() == [n // 2, n - n // 2]
    m.engine.close()


@gpu
def test_reach_zones_after_an_incremental_update(need_gpu):
    import test_redundancy as tr
    from kano import algorithm as alg
    from kano.model import ReachabilityMatrix
    name = "s_sparse_200"
    obj = cluster(name)
    cs, ps = tr.api_objects(dict(obj, policies=obj["policies"][1:]))
    m = ReachabilityMatrix.build_matrix(cs, ps)
    n = m.container_size
    same_zones(alg.reach_zones(m), reach_ref(unpack(rows_of(m), n)))
    m.add_policies([tr.api_objects(dict(obj, policies=obj["policies"][:1]))[1][0]])
    B = unpack(rows_of(m), n)
    z = alg.reach_zones(m)
    same_zones(z, reach_ref(B))
    c = alg.transitive_closure(m)
    same_zones(alg.reach_zones(m, closure=c), reach_ref(B))
    c.engine.close()
    assert np.array_equal(unpack(rows_of(m), n), B)


@gpu
def test_errors_and_degenerate_sizes(need_gpu):
    from kano import algorithm as alg
    from kano import _native as nat
    from kano._engine import DeviceBuild
    from kano.model import ReachabilityMatrix
    n = 130
    M = random_words(np.random.default_rng(130), n, 0.05)
    B = unpack(M, n)
    src, dst = engine_of(M, n), DeviceBuild.empty(n)
    half = engine_of(M[:64], n, rows=(0, 64))
    other = engine_of(random_words(np.random.default_rng(65), 65, 0.1), 65)
    lib = src.lib
    EINVAL = -errno.EINVAL
    info = np.full(2, -7, np.int64)
    label = np.full(n, -7, np.int32)

    def reverse(a, b):
        return lib.kano_reverse(a.ctx if a else None, b.ctx if b else None, info.ctypes.data)

    def zones(a, b, lab=label):
        return lib.kano_zones(a.ctx if a else None, b.ctx if b else None,
                              lab.ctypes.data if lab is not None else None, None, None, None,
                              info.ctypes.data)

    def message(e):
        return lib.kano_last_error(e.ctx).decode()

    assert reverse(None, dst) == EINVAL and reverse(src, None) == EINVAL
    assert zones(None, src) == EINVAL and zones(src, None) == EINVAL
    assert reverse(src, src) == EINVAL and "another context" in message(src)
    for a, b in ((src, half), (half, dst)):                  # a row shard on either side
        assert reverse(a, b) == EINVAL and "every row" in message(b)
        assert zones(a, b) == EINVAL and "every row" in message(a)
    assert reverse(src, other) == EINVAL and "differ in size" in message(other)
    assert zones(src, other) == EINVAL and "differ in size" in message(src)
    assert zones(src, dst, None) == EINVAL and "label is NULL" in message(src)
    assert (label == -7).all()                               # no error wrote a result
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b.*every row"):
        src.reverse_into(half)
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b.*every row"):
        half.zones(src)
    hm = ReachabilityMatrix.__new__(ReachabilityMatrix)
    hm.container_size, hm._engine = n, half
    for call in (lambda: alg.reverse_matrix(hm), lambda: alg.reach_zones(hm)):
        with pytest.raises(ValueError, match="only rows"):
            call()
    ms = ctypes.c_float(-1.0)
    for fn in (lib.kano_reverse_time, lib.kano_zones_time):
        assert fn(src.ctx, None) == EINVAL
        assert fn(src.ctx, ctypes.byref(ms)) == 0 and ms.value == 0.0
    # every context still answers
    assert src.rows(0, n).tobytes() == M.tobytes()
    assert half.rows(0, 64).tobytes() == M[:64].tobytes()
    assert not dst.rows(0, n).any()
    assert src.reverse_into(dst)["bits"] == int(B.sum())
    assert dst.rows(0, n).tobytes() == words_of(B.T).tobytes()
    same_zones(src.zones(dst), zones_ref(B, B.T))
    # n = 0 launches nothing
    z0, z1 = DeviceBuild.empty(0), DeviceBuild.empty(0)
    assert z0.reverse_into(z1) == dict(bits=0, tiles=0)
    r = z0.zones(z1)
    assert r["label"].shape == (0,) and r["zones"] == 0 and r["moved"] == 0
    em = ReachabilityMatrix.__new__(ReachabilityMatrix)
    em.container_size, em._engine = 0, z0
    assert alg.reach_zones(em).label.shape == (0,)
    for e in (src, dst, half, other, z0, z1):
        e.close()


@gpu
def test_zone_graph_refuses_too_many_zones(need_gpu):
    from kano import algorithm as alg
    from kano._engine import DeviceBuild
    from kano.model import ReachabilityMatrix
    n = 11586                                                # n * n just above 2^27
    m = ReachabilityMatrix.__new__(ReachabilityMatrix)
    m.container_size, m._engine = n, DeviceBuild.empty(n)
    z = alg.Zones(np.arange(n, dtype=np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32),
                  np.zeros(n, bool))
    with pytest.raises(ValueError, match="raise min_size"):
        alg.zone_graph(m, z)
    g = alg.zone_graph(m, z, min_size=2)
    assert g.reps.shape == (0,) and g.counts.shape == (0, 0)
    m.engine.close()


@gpu
def test_multibuild_delegates_or_refuses(need_gpu):
    import test_redundancy as tr
    from kano._engine import DeviceBuild
    from kano.multi import MultiBuild
    t = tr.cluster_tables("s_sparse_200")
    n = t.n
    one = MultiBuild(t, 1, devices=[0])
    B = unpack(one.rows(0, n), n)
    dst = DeviceBuild.empty(n)
    assert one.reverse_into(dst)["bits"] == int(B.sum())
    assert dst.rows(0, n).tobytes() == words_of(B.T).tobytes()
    same_zones(one.zones(dst), zones_ref(B, B.T))
    assert one.reverse_time() == 0.0 and one.zones_time() == 0.0
    one.close()
    two = MultiBuild(t, 2, devices=[0, 0])
    for call in (lambda: two.reverse_into(dst), lambda: two.zones(dst), two.reverse_time,
                 two.zones_time):
        with pytest.raises(ValueError, match="whole matrix on one device"):
            call()
    two.close()
    dst.close()


@gpu
def test_times_are_recorded(monkeypatch, need_gpu):
    monkeypatch.setenv("KANO_TUNE", "timing=1")
    n = 513
    M = random_words(np.random.default_rng(514), n, 0.02, tail=True)
    B = unpack(M, n)
    src, dst = engine_of(M, n), engine_of(M, n)
    assert dst.reverse_time() == 0.0 and src.zones_time() == 0.0
    src.reverse_into(dst)
    assert 0.0 < dst.reverse_time() < 10000.0 and src.reverse_time() == 0.0
    same_zones(src.zones(dst), zones_ref(B, B.T))
    assert 0.0 < src.zones_time() < 10000.0 and dst.zones_time() == 0.0
    src.close()
    dst.close()


@gpu
@pytest.mark.parametrize("tile", [1, 2])
def test_other_tile_forms_give_the_same_rows(tile, monkeypatch, need_gpu):
    monkeypatch.setenv("KANO_TUNE", f"revtile={tile}")
    n = 1100
    M = random_words(np.random.default_rng(1100 + tile), n, 0.03, tail=True)
    B = unpack(M, n)
    src, dst = engine_of(M, n), engine_of(M, n)
    info = src.reverse_into(dst)
    a, b = ((8, 8), (16, 8))[tile - 1]
    assert info == dict(bits=int(B.sum()), tiles=-(-n // (64 * a)) * -(-M.shape[1] // b))
    assert dst.rows(0, n).tobytes() == words_of(B.T).tobytes()
    src.close()
    dst.close()


@gpu
def test_between_pipelined_verify_steps(need_gpu):
    """A reverse_into() and a zones() between two steps of a pipelined verify
    loop leave the next step's lists and pairs at their golden values."""
    import test_redundancy as tr
    from _golden import expected, sha
    from kano._engine import DeviceBuild
    from kano._intern import intern, group_ids
    name = "s_sparse_2000"
    obj = cluster(name)
    cs, ps = tr.api_objects(obj)
    exp = expected(name)
    gid = group_ids(cs, obj["label"])
    eng = DeviceBuild(intern(cs, ps), build=False)
    eng.set_pipeline(True)
    n = len(cs)
    rev = DeviceBuild.empty(n)

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
    first = eng.reverse_into(rev)
    first_rows = rev.rows(0, n).copy()
    step()
    zones = eng.zones(rev)
    step()
    again = eng.reverse_into(rev)
    step()
    M = eng.rows(0, n)
    assert sha(M) == exp["M_sha256"]
    B = unpack(M, n)
    assert first == again and first["bits"] == int(B.sum())
    assert first_rows.tobytes() == rev.rows(0, n).tobytes() == words_of(B.T).tobytes()
    same_zones(zones, zones_ref(B, B.T))
    eng.close()
    rev.close()
