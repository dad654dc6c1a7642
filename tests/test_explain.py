"""pair_policies (kano_pair_policies and the layers above it): which policies
make a pod pair reachable.  pols(i, j) is the ascending list of the current
policies p with i in select_p and j in allow_p, cover(i, j) its length.  The
expectation everywhere is want_pairs below, a literal numpy restatement of
the definition; the records under tests/golden/explain/ hold the definition's
results on kano_py's own sets (tests/golden/make_explain_golden.py).  Exact
integers throughout.
"""
import ctypes
import errno
import functools
import json
import os

import numpy as np
import pytest

from _golden import GOLDEN, cluster, cluster_names, expected, lists_to_csr, sha
import test_redundancy as tr

EXPLAIN = os.path.join(GOLDEN, "explain")
ALL_NAMES = sorted(tr.TABLE)

# the paper example by hand (ingress policies, so the peers
# are the selected side, quirk Q2): A Nginx -> DB, B User -> Tomcat,
# C Tomcat -> Nginx, D app Alice -> Nginx.  Pods: A0 B1 C2 D3 E4.
PAPER = {(0, 0): [3], (0, 1): [0], (0, 3): [3], (1, 0): [3], (1, 3): [3], (2, 0): [2, 3],
         (2, 3): [2, 3], (3, 1): [0], (4, 2): [1]}


def want_pairs(select_off, select_list, allow_words, nbits, pairs):
    """The definition, literally: for pair (i, j) the ids of list i, as a set
    (a repeated id counts once), ascending, whose allow row holds bit j.
    Returns (cover int32 (Q,), offsets int64 (Q + 1,), ids int32)."""
    allow = tr._unpack(allow_words, nbits)                      # (P, nbits)
    off = np.asarray(select_off, dtype=np.int64)
    sl = np.asarray(select_list, dtype=np.int64)
    lists = []
    for i, j in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        ids = sorted(set(sl[off[i]:off[i + 1]].tolist()))
        lists.append([p for p in ids if allow[p, j]])
    o, flat = lists_to_csr(lists)
    return np.array([len(l) for l in lists], dtype=np.int32), o, flat


def record(name):
    with open(os.path.join(EXPLAIN, name + ".json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def record_arrays(name):
    """(pairs (Q, 2) int32, cover, offsets, ids) of a record, read-only."""
    rec = record(name)
    n = rec["n"]
    if rec["all_pairs"]:
        i, j = np.divmod(np.arange(n * n), n)
        pairs = np.stack([i, j], axis=1).astype(np.int32)
    else:
        pairs = np.array(rec["pairs"], dtype=np.int32).reshape(-1, 2)
    cover = np.array(rec["cover"], dtype=np.int32)
    off = np.zeros(cover.shape[0] + 1, dtype=np.int64)
    np.cumsum(cover, out=off[1:])
    ids = np.array(rec["policies"], dtype=np.int32)
    for a in (pairs, cover, off, ids):
        a.setflags(write=False)
    return pairs, cover, off, ids


def same(got, want):
    """(cover, offsets, ids) triples equal."""
    return all(np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_records_cover_every_cluster():
    have = sorted(f[:-5] for f in os.listdir(EXPLAIN))
    assert set(have) >= set(cluster_names()) | {"paper_example", "paper_example_rebuilt"}


@pytest.mark.parametrize("name", ALL_NAMES)
def test_restatement_equals_golden_record(name):
    n, off, flat, aw = tr.golden_sets(name)
    rec = record(name)
    pairs, cover, roff, ids = record_arrays(name)
    assert (rec["n"], rec["P"]) == tr.TABLE[name][:2] and n == rec["n"]
    assert rec["all_pairs"] == (n <= 64)
    assert pairs.shape[0] == (n * n if n <= 64 else 2048)
    assert same(want_pairs(off, flat, aw, n, pairs), (cover, roff, ids))
    assert roff[-1] == ids.shape[0] == cover.sum()


@pytest.mark.parametrize("name", ALL_NAMES)
def test_samples_hold_every_kind_of_cover(name):
    """Where some pair is allowed by two policies (the redundancy record's
    popcount_M > sum of impacts) the sampled pairs hold covers of 0, 1, >= 2."""
    red = tr.record(name)
    cover = record_arrays(name)[1]
    if red["popcount_M"] > sum(red["impact"]):
        assert (cover >= 2).any() and (cover == 1).any()
        if not record(name)["all_pairs"]:
            assert (cover == 0).any()
    else:
        assert cover.max() <= 1


@pytest.mark.parametrize("name", [k for k in ALL_NAMES if tr.TABLE[k][0] <= 64])
def test_cover_one_pairs_are_the_impacts(name):
    """Over all pairs of a small cluster, the pairs with cover == 1 attributed
    to their one policy count impact[p] (the redundancy records), and the
    covered pairs are popcount(M)."""
    pairs, cover, off, ids = record_arrays(name)
    red = tr.record(name)
    assert record(name)["all_pairs"]
    owner = ids[off[:-1][cover == 1]]
    assert np.bincount(owner, minlength=red["P"]).tolist() == red["impact"]
    assert int((cover > 0).sum()) == red["popcount_M"]


def test_paper_example_by_hand():
    for name in ("paper_example", "paper_example_rebuilt"):
        pairs, cover, off, ids = record_arrays(name)
        got = {(int(i), int(j)): ids[off[q]:off[q + 1]].tolist()
               for q, (i, j) in enumerate(pairs.tolist()) if cover[q]}
        assert got == PAPER
    n, off, flat, aw = tr.golden_sets("paper_example")
    cover, o, ids = want_pairs(off, flat, aw, n, [(2, 0), (4, 2), (4, 4), (2, 0)])
    assert cover.tolist() == [2, 1, 0, 2] and ids.tolist() == [2, 3, 1, 2, 3]
    assert o.tolist() == [0, 2, 3, 3, 5]


def test_library_exports_the_entry_points():
    from kano import _native as nat
    lib = ctypes.CDLL(nat.LIB_PATH)
    for sym in ("kano_pair_policies", "kano_pair_policies_fetch", "kano_pair_policies_lists",
                "kano_pair_policies_time"):
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
FORMS = ("", "ppf=1", "ppf=2", "ppf=1,ppgrid=1", "ppf=2,ppgrid=2")


def _lists_all_forms(lists, nbits, aw, pairs, monkeypatch, forms=FORMS):
    """pairs_from_lists in both modes, with and without the histogram, in
    every kernel form against the restatement; returns the expectation."""
    from kano._engine import pairs_from_lists
    off, flat = lists_to_csr([list(map(int, l)) for l in lists])
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    P = aw.shape[0]
    want = want_pairs(off, flat, aw, nbits, pairs)
    cover, woff, ids = want
    assert all(np.all(np.diff(ids[woff[q]:woff[q + 1]]) > 0) for q in range(len(cover)))
    for form in forms:
        monkeypatch.setenv("KANO_TUNE", form)
        r = pairs_from_lists(len(lists), nbits, off, flat, aw, pairs, hist=True)
        assert r["cover"].dtype == np.int32 and r["offsets"].dtype == np.int64, form
        assert r["policies"].dtype == np.int32 and r["hist"].dtype == np.int64, form
        assert same((r["cover"], r["offsets"], r["policies"]), want), form
        assert r["hist"].tolist() == np.bincount(ids, minlength=P).tolist(), form
        assert r["hist"].sum() == r["cover"].sum() == r["offsets"][-1], form
        assert r["offsets"][-1] == r["policies"].shape[0], form
        for q in range(len(cover)):
            assert np.all(np.diff(r["policies"][r["offsets"][q]:r["offsets"][q + 1]]) > 0)
        c = pairs_from_lists(len(lists), nbits, off, flat, aw, pairs, lists=False, hist=True)
        assert c["offsets"] is None and c["policies"] is None, form
        assert np.array_equal(c["cover"], cover), form
        assert c["hist"].tolist() == r["hist"].tolist(), form
        n = pairs_from_lists(len(lists), nbits, off, flat, aw, pairs)
        assert n["hist"] is None and same((n["cover"], n["offsets"], n["policies"]), want), form
    return want


@gpu
@pytest.mark.parametrize("nbits", [1, 63, 64, 65, 129])
def test_word_edges(nbits, monkeypatch, need_gpu):
    last = nbits - 1
    aw = np.stack([tr._bits_row(range(nbits), nbits), tr._bits_row([last], nbits),
                   tr._bits_row([min(64, last)], nbits), tr._bits_row([0], nbits)])
    lists = [[0, 1], [2], [3, 1, 0]]
    pairs = [(c, x) for c in range(3) for x in sorted({0, last, min(63, last), min(64, last)})]
    cover, off, ids = _lists_all_forms(lists, nbits, aw, pairs, monkeypatch)
    q = pairs.index((2, last))
    assert ids[off[q]:off[q + 1]].tolist() == ([0, 1, 3] if nbits == 1 else [0, 1])


@gpu
def test_list_lengths_at_the_ballot_edges(monkeypatch, need_gpu):
    """Lists of 0, 1, 63, 64, 65 and 130 ids (the wave form's rounds of 64),
    policy ids in three 64-bit words, allow sets that overlap in part."""
    rng = np.random.default_rng(20250301)
    P, nbits = 140, 200
    aw = np.stack([tr._bits_row(rng.choice(nbits, size=rng.integers(100, 200), replace=False),
                                nbits) for _ in range(P)])
    lists = [rng.choice(P, size=k, replace=False) for k in (0, 1, 63, 64, 65, 130)]
    pairs = [(c, x) for c in range(6) for x in (0, 63, 64, 65, 127, 128, 199)]
    cover, off, ids = _lists_all_forms(lists, nbits, aw, pairs, monkeypatch)
    assert cover[:7].tolist() == [0] * 7 and cover.max() > 64
    assert ids.min() < 64 and ids.max() >= 128


@gpu
@pytest.mark.parametrize("Q", [0, 1, 63, 64, 65, 1000])
def test_query_sizes_duplicates_and_order(Q, monkeypatch, need_gpu):
    """Q around the wave and block sizes; the pairs unsorted, with duplicates;
    grids of one and two blocks, so a block makes several rounds."""
    rng = np.random.default_rng(7 + Q)
    P, nbits, L = 70, 90, 40
    aw = np.stack([tr._bits_row(rng.choice(nbits, size=rng.integers(0, 60), replace=False),
                                nbits) for _ in range(P)])
    lists = [rng.choice(P, size=rng.integers(0, 9), replace=False) for _ in range(L)]
    pairs = np.stack([rng.integers(0, L, Q), rng.integers(0, nbits, Q)], axis=1)
    if Q >= 63:
        pairs[Q // 2:Q // 2 + 20] = pairs[:20]              # duplicates, out of order
    cover, off, ids = _lists_all_forms(lists, nbits, aw, pairs, monkeypatch)
    assert cover.shape == (Q,) and off.shape == (Q + 1,)
    if Q >= 63:
        assert np.array_equal(cover[Q // 2:Q // 2 + 20], cover[:20]) and cover.max() >= 2


@gpu
def test_empty_sets_and_repeated_ids(monkeypatch, need_gpu):
    nbits = 70
    aw = np.stack([tr._bits_row(range(10), nbits), tr._bits_row(range(5, 70), nbits),
                   tr._bits_row([], nbits), tr._bits_row(range(3), nbits)])
    # policy 2 allows nothing, policy 3 is in no list, list 2 is empty; list 3
    # names policy 1 three times and is not ascending
    lists = [[0, 1, 2], [1, 2], [], [1, 0, 1, 1]]
    pairs = [(c, x) for c in range(4) for x in (0, 4, 5, 9, 10, 69)]
    cover, off, ids = _lists_all_forms(lists, nbits, aw, pairs, monkeypatch)
    assert cover.reshape(4, 6).tolist() == [[1, 1, 2, 2, 1, 1], [0, 0, 1, 1, 1, 1], [0] * 6,
                                            [1, 1, 2, 2, 1, 1]]
    q = pairs.index((3, 5))
    assert ids[off[q]:off[q + 1]].tolist() == [0, 1]
    assert 2 not in ids and 3 not in ids


def api_objects_of(name):
    if name.startswith("paper_example"):
        from sample import paper_example
        return paper_example()
    return tr.api_objects(cluster(name))


@gpu
@pytest.mark.parametrize("name", ALL_NAMES)
def test_golden_cluster_api(name, need_gpu):
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = api_objects_of(name)
    m = ReachabilityMatrix.build_matrix(cs, ps)
    if name == "paper_example_rebuilt":
        m = ReachabilityMatrix.build_matrix(cs, ps)        # quirk Q5: the sets do not change
    pairs, cover, off, ids = record_arrays(name)
    got = alg.pair_policies(m, pairs)
    assert isinstance(got, alg.PairPolicies)
    assert got.cover.dtype == np.int32 and got.offsets.dtype == np.int64
    assert same(got, (cover, off, ids))
    assert np.array_equal(alg.pair_cover(m, pairs), cover)
    assert np.array_equal(alg.pair_policies(m, [tuple(p) for p in pairs[:50].tolist()]).cover,
                          cover[:50])
    blame = alg.policy_blame(m, pairs)
    assert blame.dtype == np.int64 and blame.shape == (len(ps),)
    assert blame.tolist() == np.bincount(ids, minlength=len(ps)).tolist()
    for q in (0, len(cover) // 2, len(cover) - 1, int(np.argmax(cover))):
        want = ids[off[q]:off[q + 1]].tolist()
        assert got.of(q) == want
        assert alg.why_reachable(m, *pairs[q].tolist()) == want


@gpu
def test_paper_example_table(need_gpu):
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = api_objects_of("paper_example")
    m = ReachabilityMatrix.build_matrix(cs, ps)
    for i in range(5):
        for j in range(5):
            assert alg.why_reachable(m, i, j) == PAPER.get((i, j), [])
            assert bool(m[i, j]) == ((i, j) in PAPER)
    assert alg.pair_policies(m, []).cover.shape == (0,)
    assert alg.pair_policies(m, np.zeros((0, 2), np.int32)).offsets.tolist() == [0]
    with pytest.raises(IndexError):
        alg.why_reachable(m, 5, 0)
    with pytest.raises(IndexError):
        alg.why_reachable(m, 0, -1)
    for other in (m.snapshot(), alg.two_hop(m), ReachabilityMatrix(5, [[0] * 5] * 5)):
        with pytest.raises(ValueError, match="no policies"):
            alg.pair_policies(other, [(0, 0)])
        with pytest.raises(ValueError, match="no policies"):
            alg.policy_blame(other, [(0, 0)])


@gpu
@pytest.mark.parametrize("form", ["", "ppf=1", "ppf=2"])
@pytest.mark.parametrize("name", ["q_wide_select", "s_sparse_2000"])
def test_cover_is_the_matrix_bit(name, form, monkeypatch, need_gpu):
    from kano._engine import DeviceBuild
    monkeypatch.setenv("KANO_TUNE", form)
    pairs, cover, off, ids = record_arrays(name)
    eng = DeviceBuild(tr.cluster_tables(name))
    info = eng.info()
    assert info["UA"] > 64 and info["MAXSEL"] >= 8     # column classes span words, large S(c)
    r = eng.pair_policies(pairs, hist=True)
    assert same((r["cover"], r["offsets"], r["policies"]), (cover, off, ids))
    assert r["hist"].tolist() == np.bincount(ids, minlength=info["P"]).tolist()
    bit = np.array([eng.get_bit(i, j) for i, j in pairs.tolist()])
    assert np.array_equal(bit == 1, cover > 0) and 0 < (cover > 0).sum() < len(cover)
    eng.close()


@gpu
@pytest.mark.parametrize("name", ["q_wide_select", "s_sparse_2000"])
@pytest.mark.parametrize("G", [2, 3])
def test_row_shards_add_up(name, G, need_gpu):
    from kano._engine import DeviceBuild
    from kano.multi import MultiBuild
    pairs, cover, off, ids = record_arrays(name)
    t = tr.cluster_tables(name)
    n, P = t.n, t.P
    hist = np.bincount(ids, minlength=P)
    even = [(n * g // G, n * (g + 1) // G) for g in range(G)]
    skewed = [(g, g + 1) for g in range(G - 1)] + [(G - 1, n)]
    for bounds in (even, skewed):
        tc, th = np.zeros_like(cover), np.zeros(P, np.int64)
        for r0, r1 in bounds:
            e = DeviceBuild(t, rows=(r0, r1))
            r = e.pair_policies(pairs, hist=True)
            mine = (pairs[:, 0] >= r0) & (pairs[:, 0] < r1)
            assert np.array_equal(r["cover"], np.where(mine, cover, 0))
            assert r["offsets"][-1] == r["policies"].shape[0] == r["cover"].sum()
            for q in np.flatnonzero(mine & (cover > 0))[:64].tolist():
                assert np.array_equal(r["policies"][r["offsets"][q]:r["offsets"][q + 1]],
                                      ids[off[q]:off[q + 1]])
            tc += r["cover"]
            th += r["hist"]
            e.close()
        assert np.array_equal(tc, cover) and np.array_equal(th, hist)
    mb = MultiBuild(t, G, devices=[0] * G)
    r = mb.pair_policies(pairs, hist=True)
    assert same((r["cover"], r["offsets"], r["policies"]), (cover, off, ids))
    assert np.array_equal(r["hist"], hist) and r["hist"].dtype == np.int64
    assert np.array_equal(mb.pair_policies(pairs, lists=False)["cover"], cover)
    mb.close()


# ---- updated matrices ------------------------------------------------------
def _fresh(name, idx):
    """Fresh policy objects idx of the cluster (never built)."""
    idx = list(idx)
    times = [idx[:q].count(k) for q, k in enumerate(idx)]     # (named twice: two objects)
    copies = [api_objects_of(name)[1] for _ in range(max(times) + 1)]
    return [copies[t][k] for t, k in zip(times, idx)]


def _query(name, n):
    if n <= 64:
        i, j = np.divmod(np.arange(n * n), n)
        return np.stack([i, j], axis=1).astype(np.int32)
    return record_arrays(name)[0]


def _check_against_sets(m, ps, n, pairs):
    """pair_policies / pair_cover / policy_blame on the matrix against the
    restatement over the policies' current working sets (current indices)."""
    from kano import algorithm as alg
    off, flat, aw = tr.policy_sets(ps, n)
    want = want_pairs(off, flat, aw, n, pairs)
    got = alg.pair_policies(m, pairs)
    assert same(got, want)
    assert np.array_equal(alg.pair_cover(m, pairs), want[0])
    assert alg.policy_blame(m, pairs).tolist() == np.bincount(want[2], minlength=len(ps)).tolist()
    return want


@gpu
@pytest.mark.parametrize("form", ["", "ppf=1", "ppf=2"])
@pytest.mark.parametrize("name", ["paper_example", "q_shadow", "s_sparse_200"])
def test_updated_matrices(name, form, monkeypatch, need_gpu):
    """snapshot, add 1 policy, add 3 (one a copy of a build policy, one a copy
    of the first added one), remove a build policy, remove an added one: after
    every step the query equals the restatement over the current working sets,
    and the diffs' pairs are explained by the policies that changed."""
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    monkeypatch.setenv("KANO_TUNE", form)
    P = tr.TABLE[name][1]
    base, held = list(range(P - 2)), [P - 2, P - 1]
    cs, ps = api_objects_of(name)
    del ps[P - 2:]
    n, P0 = len(cs), len(ps)
    pairs = _query(name, n)
    m = ReachabilityMatrix.build_matrix(cs, ps)
    _check_against_sets(m, ps, n, pairs)
    snap0 = m.snapshot()
    m.add_policies(_fresh(name, held[:1]))
    assert len(ps) == P0 + 1
    _check_against_sets(m, ps, n, pairs)
    m.add_policies(_fresh(name, [held[1], 0, held[0]]))
    assert len(ps) == P0 + 4
    cover, off, ids = _check_against_sets(m, ps, n, pairs)
    if name != "paper_example":
        assert (ids >= P0).any() and (ids < P0).any()
    added = alg.matrix_diff_pairs(snap0, m, kind="added")
    assert added.shape[0] > 0
    why = alg.pair_policies(m, added)
    assert (why.cover > 0).all()
    assert all(why.of(q)[-1] >= P0 for q in range(added.shape[0]))       # (ascending: the last)
    assert alg.policy_blame(m, added)[P0:].sum() >= added.shape[0]
    assert alg.matrix_diff_pairs(snap0, m, kind="removed").shape[0] == 0
    # the before-state of the removals, as a fresh build of the same list
    cs1 = api_objects_of(name)[0]
    ps1 = _fresh(name, base + held[:1] + [held[1], 0, held[0]])
    m1 = ReachabilityMatrix.build_matrix(cs1, ps1)
    assert same(alg.pair_policies(m1, pairs), (cover, off, ids))
    snap1 = m.snapshot()
    gone = [1, P0 + 1]                       # a build policy, then an added one
    m.remove_policies(gone[:1])
    assert len(ps) == P0 + 3
    _check_against_sets(m, ps, n, pairs)
    m.remove_policies([P0])                  # (held[1]: index P0 + 1 before the first removal)
    assert len(ps) == P0 + 2 and m._eids == [0] + list(range(2, P0 + 1)) + [P0 + 2, P0 + 3]
    cover2, off2, ids2 = _check_against_sets(m, ps, n, pairs)
    assert ids2.max(initial=-1) < len(ps)
    removed = alg.matrix_diff_pairs(snap1, m, kind="removed")
    assert alg.matrix_diff_pairs(snap1, m, kind="added").shape[0] == 0
    assert (alg.pair_cover(m, removed) == 0).all()
    assert alg.pair_policies(m, removed).policies.shape == (0,)
    before = alg.pair_policies(m1, removed)
    assert (before.cover > 0).all()
    assert set(before.policies.tolist()) <= set(gone)
    if name == "s_sparse_200":
        assert removed.shape[0] > 0
    for mm in (snap0, snap1, m1, m):
        mm._engine.close()


@gpu
def test_only_added_policies(need_gpu):
    """A build without policies has no classes: the added part alone answers."""
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = api_objects_of("paper_example")
    new = list(ps)
    m = ReachabilityMatrix.build_matrix(cs, [])
    m.add_policies(new)
    for i in range(5):
        for j in range(5):
            assert alg.why_reachable(m, i, j) == PAPER.get((i, j), [])
    m.remove_policies([3])
    assert alg.why_reachable(m, 2, 0) == [2] and alg.why_reachable(m, 0, 0) == []
    assert alg.policy_blame(m, [(2, 0), (2, 0), (3, 1)]).tolist() == [1, 0, 2]


# ---- error codes and isolation ----------------------------------------------
@gpu
def test_error_codes(need_gpu):
    from kano import _native as nat
    from kano._engine import DeviceBuild, pairs_from_lists
    aw = np.zeros((3, 1), np.uint64)
    off = np.array([0, 2, 4], np.int64)
    flat = np.array([0, 1, 2, 1], np.int32)
    for bad in ([(2, 0)], [(-1, 0)], [(0, 64)], [(0, 0), (1, -1)]):
        with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.ERANGE}\b"):
            pairs_from_lists(2, 64, off, flat, aw, bad)
    for mode in (2, -1):
        with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b"):
            pairs_from_lists(2, 64, off, flat, aw, [(0, 0)], mode=mode)
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.ERANGE}\b"):
        pairs_from_lists(2, 64, off, np.array([0, 1, 2, 3], np.int32), aw, [(0, 0)])
    eng = DeviceBuild(tr.cluster_tables("q_shadow"))
    pairs, cover, roff, ids = record_arrays("q_shadow")
    pol = np.zeros(ids.shape[0] + 1, np.int32)
    one = np.array([[0, 0]], np.int32)
    tot = ctypes.c_int64(-1)
    fetch = lambda: eng.lib.kano_pair_policies_fetch(eng.ctx, pol.ctypes.data)   # noqa: E731
    call = lambda q, p, mode: eng.lib.kano_pair_policies(                        # noqa: E731
        eng.ctx, q, None if p is None else p.ctypes.data, mode, None, None, None,
        ctypes.byref(tot))
    assert fetch() == -errno.EINVAL                       # before any call
    assert call(1, one, 2) == -errno.EINVAL and call(1, one, -1) == -errno.EINVAL
    assert call(-1, one, 0) == -errno.EINVAL and call(1, None, 0) == -errno.EINVAL
    for bad in ((8, 0), (0, 8), (-1, 0), (0, -1)):
        assert call(1, np.array([bad], np.int32), 0) == -errno.ERANGE
        assert fetch() == -errno.EINVAL
    assert call(0, None, 0) == 0 and tot.value == 0 and fetch() == 0        # Q = 0 is valid
    assert call(pairs.shape[0], pairs, 1) == 0 and tot.value == ids.shape[0]
    assert fetch() == -errno.EINVAL                       # mode 1 leaves no lists
    assert call(pairs.shape[0], pairs, 0) == 0 and tot.value == ids.shape[0]
    assert fetch() == 0 and np.array_equal(pol[:-1], ids)
    eng.close()
    for other in (DeviceBuild.empty(8),):
        assert other.lib.kano_pair_policies(other.ctx, 1, one.ctypes.data, 0, None, None, None,
                                            None) == -errno.EINVAL
        assert b"no policies" in other.lib.kano_last_error(other.ctx)
        other.close()


@gpu
def test_results_of_other_checks_are_separate(need_gpu):
    from kano._engine import DeviceBuild
    import test_conflict as tc
    name = "s_broad_300"
    exp = expected(name)["policy_shadow"]
    _, conflicts = tc.golden_want(name)
    impact, _ = tr.golden_want(name)
    pairs, cover, off, ids = record_arrays(name)
    want = (cover, off, ids)

    def explain(eng):
        r = eng.pair_policies(pairs, hist=True)
        return same((r["cover"], r["offsets"], r["policies"]), want)

    eng = DeviceBuild(tr.cluster_tables(name))
    k = eng.shadow_count()
    assert k == exp["count"]
    assert np.array_equal(eng.conflict(), conflicts)
    assert np.array_equal(eng.policy_impact(), impact)
    assert explain(eng)
    assert sha(eng.shadow_fetch(k)) == exp["sha256"]
    assert np.array_equal(eng.conflict_fetch(conflicts.shape[0]), conflicts)
    assert np.array_equal(eng.pair_policies(pairs, lists=False)["cover"], cover)
    assert sha(eng.shadow_fetch(k)) == exp["sha256"]
    assert np.array_equal(eng.conflict_fetch(conflicts.shape[0]), conflicts)
    # and the other way round: the lists survive the other checks
    assert explain(eng)
    assert sha(eng.shadow()) == exp["sha256"]
    assert np.array_equal(eng.conflict(), conflicts)
    assert np.array_equal(eng.policy_essential(), impact > 0)
    pol = np.zeros(ids.shape[0], np.int32)
    eng._chk(eng.lib.kano_pair_policies_fetch(eng.ctx, pol.ctypes.data), "fetch")
    assert np.array_equal(pol, ids)
    eng.close()


@gpu
def test_between_pipelined_verify_steps(need_gpu):
    """A pair_policies() between two steps of a pipelined verify loop (a
    prologue is queued behind its gate then) leaves the next step's lists and
    pairs at their golden values, in pairs and in count-only mode."""
    from kano._engine import DeviceBuild
    from kano._intern import intern, group_ids
    name = "s_sparse_2000"
    obj = cluster(name)
    cs, ps = tr.api_objects(obj)
    exp = expected(name)
    pairs, cover, off, ids = record_arrays(name)
    gid = group_ids(cs, obj["label"])
    eng = DeviceBuild(intern(cs, ps), build=False)
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
            r = eng.pair_policies(pairs, hist=True)
            assert same((r["cover"], r["offsets"], r["policies"]), (cover, off, ids))
        if k in (2, 3):
            assert np.array_equal(eng.pair_policies(pairs, lists=False)["cover"], cover)
    assert sha(eng.rows(0, len(cs))) == exp["M_sha256"]
    eng.close()
