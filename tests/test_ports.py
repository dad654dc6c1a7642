"""port_matrix / pair_ports (kano_policy_subset, kano_pair_masks and the layers
above them): port-aware reachability.  Over the working sets of the matrix's
current policies and their port table (kano/ports.py),
  subset(S)[i, j]  = 1 iff some p in S has i in select_p and j in allow_p
  port_matrix(k)   = subset({p : masks[p] has bit k})
  pair_ports(i, j) = OR of masks[p] over the p with i in select_p, j in allow_p
The expectation everywhere is the literal numpy restatement below over
kano_py's golden sets (test_redundancy.golden_sets); the reference has no port
semantics, so the ports are given to the golden clusters' policies by
protocol_for.  Exact integers and bits throughout.
"""
import ctypes
import errno
import functools
import types

import numpy as np
import pytest

from _golden import cluster, expected, sha
import test_explain as te
import test_redundancy as tr

ALL_NAMES = tr.ALL_NAMES
BIG = [k for k in ALL_NAMES if tr.TABLE[k][0] >= 50]


# --------------------------------------------------------------------------
# the port rule and the restatement
# --------------------------------------------------------------------------
def protocol_for(p, K):
    """The protocol the tests give policy p: four of ten a PolicyProtocol, one
    the parser's list form (lower case, int port), one None and one
    PolicyProtocol([]) (both: any port); the port from s = (p*7 + p//5) % K."""
    from kano.model import PolicyProtocol
    s = (p * 7 + p // 5) % K
    if p % 10 == 9:
        return PolicyProtocol([])
    if p % 5 == 4:
        return None
    if p % 5 == 3:
        return ["tcp", 8000 + s]
    return PolicyProtocol(["TCP", str(8000 + s)])


def table_for(P, K):
    from kano.ports import port_table
    return port_table([types.SimpleNamespace(name=f"p{p}", protocol=protocol_for(p, K))
                       for p in range(P)])


def slot_ports(t):
    """The port argument of every slot of a table, ANY_OTHER's last."""
    from kano.ports import ANY_OTHER
    return list(t.keys) + [ANY_OTHER]


def dense_sets(off, flat, aw, n):
    """(sel, allow) bool (P, n) from per-pod select lists and allow words."""
    allow = tr._unpack(aw, n).astype(bool)
    sel = np.zeros((allow.shape[0], n), dtype=bool)
    off = np.asarray(off, dtype=np.int64)
    sel[np.asarray(flat, dtype=np.int64), np.repeat(np.arange(n), np.diff(off))] = True
    return sel, allow


@functools.lru_cache(maxsize=None)
def golden_dense(name):
    n, off, flat, aw = tr.golden_sets(name)
    sel, allow = dense_sets(off, flat, aw, n)
    sel.setflags(write=False)
    allow.setflags(write=False)
    return n, sel, allow


def want_subset(sel, allow, S):
    """subset(S) as a bool (n, n) array: the definition, literally (counts of
    at most P policies are exact in float32)."""
    S = np.asarray(S, dtype=bool)
    return (sel[S].T.astype(np.float32) @ allow[S].astype(np.float32)) > 0


def to_words(bits):
    n = bits.shape[1]
    W = (n + 63) // 64
    buf = np.zeros((bits.shape[0], W * 64), dtype=np.uint8)
    buf[:, :n] = bits
    return np.packbits(buf, axis=1, bitorder="little").view(np.uint64).reshape(bits.shape[0], W)


def want_slot(sel, allow, t, k):
    return want_subset(sel, allow, (t.masks[:, k >> 6] >> np.uint64(k & 63)) & np.uint64(1))


def want_masks(sel, allow, masks, pairs):
    """pair_ports' masks, literally: uint64 (Q, KW)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    hit = sel[:, pairs[:, 0]] & allow[:, pairs[:, 1]]                 # (P, Q)
    out = np.zeros((pairs.shape[0], masks.shape[1]), dtype=np.uint64)
    for w in range(masks.shape[1]):
        out[:, w] = np.bitwise_or.reduce(np.where(hit, masks[:, w:w + 1], np.uint64(0)), axis=0) \
            if hit.shape[0] else 0
    return out


def all_pairs(n):
    i, j = np.divmod(np.arange(n * n), n)
    return np.stack([i, j], axis=1).astype(np.int32)


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def _pol(protocol, name="web"):
    return types.SimpleNamespace(name=name, protocol=protocol)


def test_port_key_forms():
    from kano.model import PolicyProtocol
    from kano.ports import PortSet, port_key
    for any_port in (None, [], PolicyProtocol([]), PolicyProtocol(None)):
        assert port_key(_pol(any_port)) is None
    want = (("TCP", "80"),)
    for one in (["tcp", 80], ["TCP", "80"], ("Tcp", "80"), PolicyProtocol(["TCP", "80"]),
                PolicyProtocol(["tcp", 80]), PortSet([("tcp", 80)])):
        assert port_key(_pol(one)) == want
    assert port_key(_pol(PortSet([("tcp", 80), ("UDP", "53"), ("TCP", "80")]))) == \
        (("TCP", "80"), ("UDP", "53"))
    assert PortSet([("tcp", 80)]) == PortSet([("TCP", "80")])
    for bad in ("TCP", ["TCP"], ["TCP", "80", "x"], 80, PolicyProtocol(["TCP"]), {"TCP": 80},
                ["TCP", None], PolicyProtocol("TCP")):
        with pytest.raises(TypeError, match="web"):
            port_key(_pol(bad))
    with pytest.raises(TypeError):
        PortSet(["TCP"])


def test_port_table_order_and_masks():
    from kano.model import PolicyProtocol
    from kano.ports import ANY_OTHER, PortSet, port_table
    ps = [_pol(["udp", 53]), _pol(None), _pol(PolicyProtocol(["TCP", "80"])), _pol(["UDP", "53"]),
          _pol(PortSet([("tcp", 443), ("tcp", 80)])), _pol(PolicyProtocol([]))]
    t = port_table(ps)
    assert t.keys == [("UDP", "53"), ("TCP", "80"), ("TCP", "443")]
    assert (t.K, t.KS, t.KW) == (3, 4, 1)
    assert t.masks.dtype == np.uint64 and t.masks.shape == (6, 1)
    assert t.masks[:, 0].tolist() == [1, 15, 2, 1, 6, 15]
    assert t.any_port.dtype == bool and t.any_port.tolist() == [False, True] + [False] * 3 + [True]
    assert t.slot(("udp", 53)) == 0 and t.slot(("TCP", 22)) == 3 and t.slot(ANY_OTHER) == 3
    assert t.slots([("tcp", "443"), ANY_OTHER, ("TCP", 22)]) == [2, 3]
    # K = 0: every policy any-port
    z = port_table([_pol(None), _pol([])])
    assert z.keys == [] and (z.KS, z.KW) == (1, 1) and z.masks.tolist() == [[1], [1]]
    assert port_table([]).masks.shape == (0, 1)
    # the rule, K = 3 and K = 70: any-port rows hold all KS bits, pad bits zero
    for P, K in ((40, 3), (340, 70), (200, 70)):
        t = table_for(P, K)
        assert t.KW == (t.KS + 63) // 64 and t.K <= K
        assert (t.K, t.KW) == (3, 1) if K == 3 else (t.K > 63 and t.KW == 2)
        bits = tr._unpack(t.masks, t.KW * 64)
        assert not bits[:, t.KS:].any()
        for p in range(P):
            if p % 5 == 4:
                assert t.any_port[p] and bits[p, :t.KS].all()
            else:
                s = (p * 7 + p // 5) % K
                assert not t.any_port[p] and bits[p].sum() == 1
                assert t.keys[int(np.flatnonzero(bits[p])[0])] == ("TCP", str(8000 + s))
    # 64 slots fill one word exactly; the 65th opens a second
    assert port_table([_pol(["TCP", k]) for k in range(63)]).KW == 1
    t = port_table([_pol(["TCP", k]) for k in range(64)] + [_pol(None)])
    assert t.KW == 2 and t.masks[-1].tolist() == [2 ** 64 - 1, 1]


def test_paper_example_table():
    from kano.ports import port_table
    from sample import paper_example
    t = port_table(paper_example()[1])
    assert t.keys == [("TCP", "3306"), ("TCP", "8080")]
    assert t.masks[:, 0].tolist() == [1, 2, 1, 1] and not t.any_port.any()


@pytest.mark.parametrize("K", [3, 70])
@pytest.mark.parametrize("name", BIG)
def test_restatement_is_not_vacuous(name, K):
    """Some slot's matrix lies strictly between empty and M; the sampled pairs'
    masks are empty exactly where the explain records' cover is 0, and some
    pair is open on one slot only."""
    n, sel, allow = golden_dense(name)
    t = table_for(sel.shape[0], K)
    popm = tr.TABLE[name][5]
    assert int(want_subset(sel, allow, np.ones(sel.shape[0], bool)).sum()) == popm
    assert any(0 < int(want_slot(sel, allow, t, k).sum()) < popm for k in range(t.KS))
    pairs, cover = te.record_arrays(name)[:2]
    masks = want_masks(sel, allow, t.masks, pairs)
    assert np.array_equal(masks.any(axis=1), cover > 0)
    pops = tr._unpack(masks, t.KW * 64).sum(axis=1)
    assert (pops == 1).any() and pops.max() <= t.KS


def test_library_exports_the_entry_points():
    from kano import _native as nat
    lib = ctypes.CDLL(nat.LIB_PATH)
    for sym in ("kano_policy_subset", "kano_pair_masks", "kano_policy_subset_time",
                "kano_pair_masks_time"):
        assert sym in nat.SIGNATURES
        assert getattr(lib, sym) is not None


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def need_gpu():
    from kano import _native
    if not _native.gpu_available():
        pytest.fail("GPU test run without a usable HIP device / libkano_hip.so")


gpu = pytest.mark.gpu
MASK_FORMS = ("", "pmf=1", "pmf=2", "pmf=1,pmgrid=1", "pmf=2,pmgrid=2")


def built(name, K, drop=0):
    """(containers, policies, matrix) of a golden cluster with the rule's
    ports, without its last ``drop`` policies."""
    from kano.model import ReachabilityMatrix
    cs, ps = te.api_objects_of(name)
    if drop:
        del ps[len(ps) - drop:]
    for p, pol in enumerate(ps):
        pol.protocol = protocol_for(p, K)
    return cs, ps, ReachabilityMatrix.build_matrix(cs, ps)


def rows_of(m):
    n = m.container_size
    span = getattr(m._engine, "row_span", None) or (0, n)
    return m._engine.rows(span[0], span[1] - span[0])


def check_ports(m, sel, allow, t, pairs, slots=None, exposure=True):
    """port_matrix of the given slots (default: all), pair_ports on the pairs
    and port_exposure against the restatement."""
    from kano import algorithm as alg
    ports = slot_ports(t)
    pops = []
    assert slots is None or not exposure
    for k in (range(t.KS) if slots is None else slots):
        want = want_slot(sel, allow, t, k)
        pops.append(int(want.sum()))
        pm = alg.port_matrix(m, ports[k])
        assert pm._policies is None
        assert np.array_equal(rows_of(pm), to_words(want)), k
        pm._engine.close()
    got = alg.pair_ports(m, pairs)
    assert got.keys == t.keys and got.masks.dtype == np.uint64
    want = want_masks(sel, allow, t.masks, pairs)
    assert got.masks.shape == want.shape and np.array_equal(got.masks, want)
    if exposure:
        keys, counts = alg.port_exposure(m)
        assert keys == t.keys and counts.dtype == np.int64 and counts.tolist() == pops
    return want, pops


@gpu
def test_paper_example_by_hand(need_gpu):
    from kano.model import ReachabilityMatrix
    from kano.ports import ANY_OTHER
    from kano import algorithm as alg
    from sample import paper_example
    cs, ps = paper_example()
    m = ReachabilityMatrix.build_matrix(cs, ps)
    open_on = {(("TCP", "3306"),): set(te.PAPER) - {(4, 2)}, (("TCP", "8080"),): {(4, 2)},
               (ANY_OTHER,): set(), (("TCP", "22"),): set(),
               (("tcp", 3306), ("TCP", "8080")): set(te.PAPER)}
    for port, want in open_on.items():
        pm = alg.port_matrix(m, port[0] if len(port) == 1 else list(port))
        assert {(i, j) for i in range(5) for j in range(5) if pm[i, j]} == want
        pm._engine.close()
    pp = alg.pair_ports(m, all_pairs(5))
    assert isinstance(pp, alg.PairPorts) and pp.keys == [("TCP", "3306"), ("TCP", "8080")]
    for q, (i, j) in enumerate(all_pairs(5).tolist()):
        want = [] if (i, j) not in te.PAPER else \
            [("TCP", "8080")] if (i, j) == (4, 2) else [("TCP", "3306")]
        assert pp.of(q) == want
    assert pp.on(("TCP", "8080")).tolist() == [(i, j) == (4, 2) for i, j in all_pairs(5).tolist()]
    assert not pp.on(ANY_OTHER).any() and not pp.on(("TCP", "22")).any()
    assert alg.reachable_on(m, 4, 2, ("tcp", 8080)) is True
    assert alg.reachable_on(m, 4, 2, ("TCP", "3306")) is False
    assert alg.reachable_on(m, 2, 0, ("TCP", "3306")) is True
    keys, counts = alg.port_exposure(m)
    assert keys == pp.keys and counts.tolist() == [8, 1, 0]
    # policy B open on any port: (4, 2) is open on every slot, ANY_OTHER included
    cs, ps = paper_example()
    ps[1].protocol = None
    m2 = ReachabilityMatrix.build_matrix(cs, ps)
    pp = alg.pair_ports(m2, [(4, 2), (2, 0)])
    assert pp.keys == [("TCP", "3306")] and pp.of(0) == [("TCP", "3306"), ANY_OTHER]
    assert pp.of(1) == [("TCP", "3306")]
    for port in (("TCP", "3306"), ANY_OTHER, ("TCP", "8080")):
        assert alg.reachable_on(m2, 4, 2, port)
    any_other = alg.port_matrix(m2, ANY_OTHER)
    assert {(i, j) for i in range(5) for j in range(5) if any_other[i, j]} == {(4, 2)}


@gpu
@pytest.mark.parametrize("name", ALL_NAMES)
def test_golden_cluster(name, need_gpu):
    n, sel, allow = golden_dense(name)
    cs, ps, m = built(name, 3)
    t = table_for(len(ps), 3)
    from kano.ports import port_table
    got = port_table(ps)
    assert got.keys == t.keys and np.array_equal(got.masks, t.masks)
    before = rows_of(m)
    _, pops = check_ports(m, sel, allow, t, te.record_arrays(name)[0])
    assert max(pops) <= tr.TABLE[name][5]
    # the matrix is untouched, and the union of the slots
    assert np.array_equal(rows_of(m), before)
    assert np.array_equal(before, to_words(want_subset(sel, allow, np.ones(len(ps), bool))))


@gpu
@pytest.mark.parametrize("tune", ["pathlds=0", "pathlds=1"])
@pytest.mark.parametrize("name", ["q_types", "s_sparse_200", "s_broad_300", "q_wide_select"])
def test_both_expansions(name, tune, monkeypatch, need_gpu):
    """The class rows' expansion with its table in LDS and without, over
    clusters with few and with many members per row class (the direct and the
    staged stores)."""
    monkeypatch.setenv("KANO_TUNE", tune)
    n, sel, allow = golden_dense(name)
    cs, ps, m = built(name, 3)
    t = table_for(len(ps), 3)
    check_ports(m, sel, allow, t, te.record_arrays(name)[0][:64], exposure=False)
    U = m.engine.info()["U"]
    assert ((n + U - 1) // U >= 16) == (name in ("s_broad_300", "q_wide_select"))


@gpu
@pytest.mark.parametrize("name", ["q_wide_select", "s_sparse_2000"])
def test_two_mask_words(name, need_gpu):
    n, sel, allow = golden_dense(name)
    cs, ps, m = built(name, 70)
    t = table_for(len(ps), 70)
    assert t.K > 64 and t.KW == 2
    masks, pops = check_ports(m, sel, allow, t, te.record_arrays(name)[0],
                              slots=(5, 64, t.K), exposure=False)
    assert masks[:, 1].any() and masks[:, 0].any()
    assert 0 < pops[2] < tr.TABLE[name][5]               # (the any-port policies' pairs)


@gpu
@pytest.mark.parametrize("name", ["paper_example", "q_shadow", "q_types", "s_sparse_50",
                                  "s_sparse_200"])
def test_subset_against_the_impact_records(name, need_gpu):
    from kano import algorithm as alg
    cs, ps, m = built(name, 3)
    P, n = len(ps), len(cs)
    impact = tr.record(name)["impact"]
    for p in range(P):
        sub = alg.policy_subset_matrix(m, [k for k in range(P) if k != p])
        d = alg.matrix_diff(m, sub)
        assert (d.added, d.removed) == (0, impact[p]), p
        sub._engine.close()
    full = alg.policy_subset_matrix(m, range(P))
    assert alg.matrix_diff(m, full).equal
    assert full.subset_info["kept_build"] == P and full.subset_info["kept_added"] == 0
    none = alg.policy_subset_matrix(m, [])
    assert not rows_of(none).any() and alg.all_isolated(none) == list(range(n))
    twice = alg.policy_subset_matrix(m, [0, 1, 0, -1, 1])
    once = alg.policy_subset_matrix(m, [0, 1, P - 1])
    assert alg.matrix_diff(once, twice).equal and np.array_equal(rows_of(once), rows_of(twice))
    for k in (P, -P - 1):
        with pytest.raises(IndexError):
            alg.policy_subset_matrix(m, [0, k])


@gpu
@pytest.mark.parametrize("Q", [0, 1, 63, 64, 65, 1000])
def test_query_sizes_duplicates_and_order(Q, monkeypatch, need_gpu):
    """Q around the wave and block sizes; the pairs unsorted, with duplicates;
    both forms of the kernel, grids of one and two blocks."""
    from kano._engine import DeviceBuild
    name = "s_sparse_200"
    n, sel, allow = golden_dense(name)
    t = table_for(sel.shape[0], 3)
    rng = np.random.default_rng(11 + Q)
    pairs = rng.integers(0, n, (Q, 2)).astype(np.int32)
    if Q >= 63:
        pairs[Q // 2:Q // 2 + 20] = pairs[:20]
    want = want_masks(sel, allow, t.masks, pairs)
    for form in MASK_FORMS:
        monkeypatch.setenv("KANO_TUNE", form)
        eng = DeviceBuild(tr.cluster_tables(name))
        got = eng.pair_masks(pairs, t.masks)
        assert got.shape == (Q, 1) and np.array_equal(got, want), form
        eng.close()
    if Q >= 63:
        assert want.any() and not want.all()


@gpu
def test_list_lengths_at_the_ballot_edges(monkeypatch, need_gpu):
    """Row classes whose policy lists hold 63, 64 and 65 policies (the wave
    form's rounds of 64), built through the public API."""
    from kano.model import (Container, Policy, PolicyAllow, PolicyEgress, PolicySelect,
                            ReachabilityMatrix)
    from kano.ports import port_table
    from kano import algorithm as alg
    n, groups = 150, {"a": 63, "b": 64, "c": 65}

    def objects():
        cs = [Container(f"c{i}", {"g": "abcz"[min(i // 10, 3)], "id": str(i % 13)})
              for i in range(n)]
        ps = []
        for g, k in groups.items():
            for q in range(k):
                p = len(ps)
                ps.append(Policy(f"p{p}", PolicySelect({"g": g}), PolicyAllow({"id": str(q % 13)}),
                                 PolicyEgress, protocol_for(p, 5)))
        return cs, ps

    pairs = np.array([(i, j) for i in (0, 9, 10, 19, 20, 29, 30, 149) for j in range(n)], np.int32)
    for form in MASK_FORMS[:3]:
        monkeypatch.setenv("KANO_TUNE", form)
        cs, ps = objects()
        m = ReachabilityMatrix.build_matrix(cs, ps)
        off, flat, aw = tr.policy_sets(ps, n)
        assert sorted(set(np.diff(off).tolist())) == [0, 63, 64, 65]
        sel, allow = dense_sets(off, flat, aw, n)
        t = port_table(ps)
        check_ports(m, sel, allow, t, pairs, slots=None if form == "" else (0, t.K),
                    exposure=(form == ""))
        m._engine.close()


@gpu
@pytest.mark.parametrize("name", ["q_wide_select", "s_sparse_2000"])
@pytest.mark.parametrize("G", [2, 3])
def test_row_shards(name, G, need_gpu):
    from kano._engine import DeviceBuild
    from kano.multi import MultiBuild
    n, sel, allow = golden_dense(name)
    tb = tr.cluster_tables(name)
    t = table_for(tb.P, 3)
    pairs = te.record_arrays(name)[0]
    keep = t.carries([1])
    whole = to_words(want_slot(sel, allow, t, 1))
    masks = want_masks(sel, allow, t.masks, pairs)
    cuts = [0] + [n * g // G + 7 * g for g in range(1, G)] + [n]
    assert all(c % 64 for c in cuts[1:-1])
    parts, acc = [], np.zeros_like(masks)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        e = DeviceBuild(tb, rows=(r0, r1))
        d = DeviceBuild.empty(n, rows=(r0, r1))
        info = e.subset_into(d, keep)
        assert info["kept_build"] == int(keep.sum()) and info["kept_added"] == 0
        parts.append(d.rows(r0, r1 - r0))
        got = e.pair_masks(pairs, t.masks)
        mine = (pairs[:, 0] >= r0) & (pairs[:, 0] < r1)
        assert np.array_equal(got, np.where(mine[:, None], masks, np.uint64(0)))
        acc |= got
        e.close()
        d.close()
    assert np.array_equal(np.concatenate(parts), whole) and np.array_equal(acc, masks)
    if G == 2:
        mb = MultiBuild(tb, 2, devices=[0, 0])
        md = MultiBuild.empty(n, 2, devices=[0, 0])
        mb.subset_into(md, keep)
        assert np.array_equal(md.rows(0, n), whole)
        assert np.array_equal(mb.pair_masks(pairs, t.masks), masks)
        mb.close()
        md.close()


# ---- updated matrices ------------------------------------------------------
def _check_current(m, ps, n, pairs):
    """The three queries against the restatement over the current policies'
    working sets and their port table (current indices)."""
    from kano.ports import port_table
    off, flat, aw = tr.policy_sets(ps, n)
    sel, allow = dense_sets(off, flat, aw, n)
    t = port_table(ps)
    return t, check_ports(m, sel, allow, t, pairs)


@gpu
@pytest.mark.parametrize("name", ["paper_example", "q_shadow", "s_sparse_200"])
def test_updated_matrices(name, need_gpu):
    """Add two policies (one with a key the build does not name, one open on
    any port), remove a build policy and an added one: after every step the
    queries equal the restatement over the current working sets."""
    from kano.ports import PortSet
    from kano import algorithm as alg
    P = tr.TABLE[name][1]
    cs, ps, m = built(name, 3, drop=2)
    n, P0 = len(cs), len(ps)
    pairs = te._query(name, n)
    t0, _ = _check_current(m, ps, n, pairs)
    new = te._fresh(name, [P - 2, P - 1])
    new[0].protocol = PortSet([("udp", 53), ("TCP", "8000")])
    new[1].protocol = None
    m.add_policies(new)
    assert len(ps) == P0 + 2
    t1, _ = _check_current(m, ps, n, pairs)
    assert t1.keys == t0.keys + [("UDP", "53")] and t1.any_port[-1]
    m.remove_policies([1])
    _check_current(m, ps, n, pairs)
    m.remove_policies([len(ps) - 2])                       # the first added one
    t2, _ = _check_current(m, ps, n, pairs)
    assert ("UDP", "53") not in t2.keys and len(ps) == P0
    sub = alg.policy_subset_matrix(m, range(len(ps)))
    assert alg.matrix_diff(m, sub).equal
    assert sub.subset_info["kept_build"] == P0 - 1 and sub.subset_info["kept_added"] == 1
    for mm in (sub, m):
        mm._engine.close()


@gpu
def test_only_added_policies(need_gpu):
    """A build without policies has no classes: the added part alone answers."""
    from kano.model import ReachabilityMatrix
    from kano.ports import ANY_OTHER
    from kano import algorithm as alg
    from sample import paper_example
    cs, ps = paper_example()
    m = ReachabilityMatrix.build_matrix(cs, [])
    assert alg.pair_ports(m, [(0, 0)]).masks.tolist() == [[0]]
    assert not rows_of(alg.port_matrix(m, ANY_OTHER)).any()
    assert alg.port_exposure(m)[1].tolist() == [0]
    m.add_policies(list(ps))
    _check_current(m, m._policies, 5, all_pairs(5))
    assert alg.reachable_on(m, 4, 2, ("TCP", "8080"))
    m.remove_policies([3])
    _check_current(m, m._policies, 5, all_pairs(5))
    assert alg.pair_ports(m, [(2, 0), (0, 0)]).masks[:, 0].tolist() == [1, 0]


# ---- composition -----------------------------------------------------------
@gpu
def test_queries_on_a_port_matrix(need_gpu):
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    name = "s_sparse_200"
    n, sel, allow = golden_dense(name)
    cs, ps, m = built(name, 3)
    t = table_for(len(ps), 3)
    bits = want_slot(sel, allow, t, 0)
    assert 0 < bits.sum() < tr.TABLE[name][5]
    pm = alg.port_matrix(m, t.keys[0])
    ref = ReachabilityMatrix(n, bits.astype(int).tolist())
    intents = [(range(0, 60), range(100, 180), "deny"), (range(20, 40), [3, 5, 150], "allow"),
               ([0], range(n), "deny")]
    a, b = alg.check_intents(pm, cs, intents), alg.check_intents(ref, cs, intents)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a.reachable.sum() > 0
    src = [0, 17, 101, 199]
    assert np.array_equal(alg.hop_levels(pm, src), alg.hop_levels(ref, src))
    label = cluster(name)["label"]
    ga, gb = alg.group_reachability(pm, cs, label), alg.group_reachability(ref, cs, label)
    assert ga.src_keys == gb.src_keys and np.array_equal(ga.counts, gb.counts)
    assert int(ga.counts.sum()) == int(bits.sum())
    assert alg.all_isolated(pm) == alg.all_isolated(ref)


# ---- error codes and isolation ----------------------------------------------
@gpu
def test_errors(need_gpu):
    from kano.model import ReachabilityMatrix
    from kano._engine import DeviceBuild
    from kano import algorithm as alg
    cs, ps, m = built("q_shadow", 3)
    n, P = len(cs), len(ps)
    for other in (m.snapshot(), alg.two_hop(m), ReachabilityMatrix(n, [[0] * n] * n)):
        for call in (lambda o: alg.port_matrix(o, ("TCP", "8000")),
                     lambda o: alg.pair_ports(o, [(0, 0)]), lambda o: alg.port_exposure(o),
                     lambda o: alg.policy_subset_matrix(o, [0]),
                     lambda o: alg.reachable_on(o, 0, 0, ("TCP", "8000"))):
            with pytest.raises(ValueError, match="no policies"):
                call(other)
    for bad in ([(n, 0)], [(0, -1)], [(0, 0), (0, n)]):
        with pytest.raises(IndexError):
            alg.pair_ports(m, bad)
    with pytest.raises(IndexError):
        alg.reachable_on(m, 0, n, ("TCP", "8000"))
    with pytest.raises(IndexError):
        alg.policy_subset_matrix(m, [P])
    # the C entry points
    eng = DeviceBuild(tr.cluster_tables("q_shadow"))
    dst, small, shard = DeviceBuild.empty(n), DeviceBuild.empty(n - 1), DeviceBuild.empty(
        n, rows=(0, n - 1))
    lib = eng.lib
    keep = np.ones(P, np.uint8)
    info = np.zeros(3, np.int64)
    sub = lambda s, d, k, kp: lib.kano_policy_subset(                           # noqa: E731
        s, d, k, None if kp is None else kp.ctypes.data, info.ctypes.data)
    EINVAL, ERANGE = -errno.EINVAL, -errno.ERANGE
    assert sub(None, dst.ctx, P, keep) == EINVAL and sub(eng.ctx, None, P, keep) == EINVAL
    assert sub(eng.ctx, eng.ctx, P, keep) == EINVAL
    assert sub(eng.ctx, dst.ctx, P, None) == EINVAL
    assert sub(eng.ctx, dst.ctx, P + 1, keep) == EINVAL and sub(eng.ctx, dst.ctx, 0, keep) == EINVAL
    assert sub(eng.ctx, small.ctx, P, keep) == EINVAL and sub(eng.ctx, shard.ctx, P, keep) == EINVAL
    assert sub(dst.ctx, small.ctx, 0, keep) == EINVAL
    assert b"no policies" in lib.kano_last_error(small.ctx)
    one = np.array([[0, 0]], np.int32)
    pm = np.ones((P, 1), np.uint64)
    out = np.zeros((1, 1), np.uint64)
    pmk = lambda c, q, pr, k, kw, mk, o: lib.kano_pair_masks(                    # noqa: E731
        c, q, None if pr is None else pr.ctypes.data, k, kw,
        None if mk is None else mk.ctypes.data, None if o is None else o.ctypes.data)
    assert pmk(None, 1, one, P, 1, pm, out) == EINVAL
    assert pmk(eng.ctx, -1, one, P, 1, pm, out) == EINVAL
    assert pmk(eng.ctx, 1, None, P, 1, pm, out) == EINVAL
    assert pmk(eng.ctx, 1, one, P, 1, None, out) == EINVAL
    assert pmk(eng.ctx, 1, one, P, 1, pm, None) == EINVAL
    assert pmk(eng.ctx, 1, one, P, 0, pm, out) == EINVAL
    assert pmk(eng.ctx, 1, one, P - 1, 1, pm, out) == EINVAL
    assert pmk(dst.ctx, 1, one, 0, 1, pm, out) == EINVAL
    assert b"no policies" in lib.kano_last_error(dst.ctx)
    for bad in ((n, 0), (0, n), (-1, 0), (0, -1)):
        assert pmk(eng.ctx, 1, np.array([bad], np.int32), P, 1, pm, out) == ERANGE
    assert pmk(eng.ctx, 0, None, P, 1, pm, None) == 0               # Q = 0 is valid
    # usable afterwards
    assert pmk(eng.ctx, 1, one, P, 1, pm, out) == 0
    assert sub(eng.ctx, dst.ctx, P, keep) == 0 and info.tolist()[:2] == [P, 0] and info[2] > 0
    assert np.array_equal(dst.rows(0, n), eng.rows(0, n))
    assert out[0, 0] == int(eng.get_bit(0, 0))
    for e in (eng, dst, small, shard):
        e.close()


@gpu
def test_results_of_other_checks_are_separate(need_gpu):
    from kano._engine import DeviceBuild
    import test_conflict as tc
    name = "s_broad_300"
    exp = expected(name)["policy_shadow"]
    _, conflicts = tc.golden_want(name)
    impact, _ = tr.golden_want(name)
    pairs, cover, off, ids = te.record_arrays(name)
    n, sel, allow = golden_dense(name)
    eng = DeviceBuild(tr.cluster_tables(name))
    t = table_for(eng.info()["P"], 3)
    dst = DeviceBuild.empty(n)

    def state():
        r = eng.pair_policies(pairs, hist=True)
        return (eng.shadow(), eng.conflict(), eng.policy_impact(), r["cover"], r["offsets"],
                r["policies"], eng.rows_digest(0, n))

    def ports():
        eng.subset_into(dst, t.carries([0]))
        assert np.array_equal(dst.rows(0, n), to_words(want_slot(sel, allow, t, 0)))
        assert np.array_equal(eng.pair_masks(pairs, t.masks),
                              want_masks(sel, allow, t.masks, pairs))

    first = state()
    assert sha(first[0]) == exp["sha256"] and np.array_equal(first[1], conflicts)
    assert np.array_equal(first[2], impact) and te.same(first[3:6], (cover, off, ids))
    ports()
    assert all(np.array_equal(a, b) for a, b in zip(first, state()))
    # the stored results survive the new calls: fetched after them
    k = eng.shadow_count()
    eng.conflict()
    eng.pair_policies(pairs)
    ports()
    assert sha(eng.shadow_fetch(k)) == exp["sha256"]
    assert np.array_equal(eng.conflict_fetch(conflicts.shape[0]), conflicts)
    pol = np.zeros(ids.shape[0], np.int32)
    eng._chk(eng.lib.kano_pair_policies_fetch(eng.ctx, pol.ctypes.data), "fetch")
    assert np.array_equal(pol, ids)
    eng.close()
    dst.close()


@gpu
def test_between_pipelined_verify_steps(need_gpu):
    """The port queries between two steps of a pipelined verify loop (a
    prologue is queued behind its gate then) leave the next step's lists and
    pairs at their golden values."""
    from kano._engine import DeviceBuild
    from kano._intern import intern, group_ids
    name = "s_sparse_2000"
    obj = cluster(name)
    cs, ps = tr.api_objects(obj)
    exp = expected(name)
    pairs = te.record_arrays(name)[0]
    n, sel, allow = golden_dense(name)
    t = table_for(len(ps), 3)
    want_rows = to_words(want_slot(sel, allow, t, 2))
    want = want_masks(sel, allow, t.masks, pairs)
    gid = group_ids(cs, obj["label"])
    eng = DeviceBuild(intern(cs, ps), build=False)
    dst = DeviceBuild.empty(n)
    eng.set_pipeline(True)

    def check(r, count_only=False):
        assert r["all_isolated"].tolist() == exp["all_isolated"]
        assert r["all_reachable"].tolist() == exp["all_reachable"]
        assert r["user_crosscheck"].tolist() == exp["user_crosscheck"]["result"]
        assert r["system_isolation"].tolist() == exp["system_isolation"]["result"]
        assert r["shadow_count"] == exp["policy_shadow"]["count"]
        if not count_only:
            assert sha(np.ascontiguousarray(r["pairs"])) == exp["policy_shadow"]["sha256"]

    for k in range(6):
        count_only = k in (3, 4)
        check(eng.verify(gid, sys_row=0, shadow=True, shadow_count_only=count_only), count_only)
        if k in (1, 4):
            eng.subset_into(dst, t.carries([2]))
            assert np.array_equal(dst.rows(0, n), want_rows)
        if k in (2, 3):
            assert np.array_equal(eng.pair_masks(pairs, t.masks), want)
    assert sha(eng.rows(0, len(cs))) == exp["M_sha256"]
    eng.close()
    dst.close()
