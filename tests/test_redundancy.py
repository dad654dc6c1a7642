"""policy_impact / policy_redundant (kano_policy_impact and the layers above
it): impact[p] is the number of pod pairs (i, j) that only policy p allows --
what removing p alone takes away -- and p is redundant when it is 0.  The
expectation everywhere is want_impact below, a brute-force numpy restatement
of the definition; the records under tests/golden/redundancy/ hold the
definition's results on kano_py's own sets
(tests/golden/make_redundancy_golden.py).  Exact integers throughout.
"""
import ctypes
import errno
import functools
import json
import os

import numpy as np
import pytest

from _golden import GOLDEN, cluster, cluster_names, expected, lists_to_csr, rows01_to_words, sha

REDUNDANCY = os.path.join(GOLDEN, "redundancy")

# name: (n, P, redundant, sum of impacts, largest impact, popcount(M))
TABLE = {
    "paper_example": (5, 4, 1, 7, 4, 9), "paper_example_rebuilt": (5, 4, 1, 7, 4, 9),
    "q_dirs": (5, 5, 4, 11, 11, 25), "q_missing_label": (5, 3, 0, 8, 4, 8),
    "q_nan_list": (3, 3, 1, 3, 2, 3), "q_no_conflict": (3, 2, 0, 2, 1, 2),
    "q_shadow": (8, 6, 5, 24, 24, 52), "q_types": (8, 5, 0, 14, 6, 14),
    "q_unknown_key": (3, 3, 1, 5, 4, 7), "s_sparse_50": (50, 10, 9, 729, 729, 1971),
    "s_sparse_200": (200, 40, 6, 6751, 552, 7586),
    "s_sparse_500": (500, 50, 0, 13214, 864, 13214),
    "s_sparse_1000": (1000, 100, 0, 29667, 984, 29667),
    "s_sparse_2000": (2000, 200, 3, 72840, 2809, 73102),
    "s_broad_300": (300, 30, 22, 24762, 5940, 61946),
    "s_broad_1000": (1000, 60, 39, 216014, 45649, 610301),
    "q_wide_select": (1200, 340, 40, 496718, 25194, 567434),
}
IMPACT = {
    "paper_example": [2, 1, 0, 4], "paper_example_rebuilt": [2, 1, 0, 4],
    "q_missing_label": [4, 2, 2], "q_nan_list": [0, 2, 1], "q_types": [6, 1, 3, 2, 2],
    "q_unknown_key": [4, 1, 0],
}
REDUNDANT = {
    "q_dirs": [0, 1, 2, 3], "q_shadow": [0, 1, 2, 3, 4],
    "s_sparse_50": [0, 1, 3, 4, 5, 6, 7, 8, 9], "s_sparse_200": [4, 7, 12, 32, 37, 39],
    "s_sparse_2000": [77, 126, 136],
}


def _unpack(words, nbits):
    w = np.ascontiguousarray(words, dtype=np.uint64)
    w = w.reshape(w.shape[0], -1)
    if w.shape[1] == 0:
        return np.zeros((w.shape[0], nbits), np.int64)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :nbits].astype(np.int64)


def want_impact(select_off, select_list, allow_words, nbits, with_popcount=False):
    """The definition, literally: cover(i, j) = #{p : i in sel_p, j in allow_p}
    with sel_p = the lists holding p (as a set: a repeated id counts once),
    impact[p] = #{(i, j) in sel_p x allow_p : cover(i, j) == 1}.  int64 (P,)."""
    allow = _unpack(allow_words, nbits)                         # (P, nbits)
    P = allow.shape[0]
    off = np.asarray(select_off, dtype=np.int64)
    sl = np.asarray(select_list, dtype=np.int64)
    sel = np.zeros((P, off.shape[0] - 1), np.int64)             # (P, lists)
    sel[sl, np.repeat(np.arange(off.shape[0] - 1), np.diff(off))] = 1
    cover = sel.T @ allow                                       # (lists, nbits)
    once = (cover == 1).astype(np.int64)
    impact = np.array([int(sel[p] @ once @ allow[p]) for p in range(P)], dtype=np.int64)
    return (impact, int((cover > 0).sum())) if with_popcount else impact


def record(name):
    with open(os.path.join(REDUNDANCY, name + ".json")) as f:
        return json.load(f)


def record_names():
    return sorted(f[:-5] for f in os.listdir(REDUNDANCY)) if os.path.isdir(REDUNDANCY) else []


ALL_NAMES = sorted(TABLE)


@functools.lru_cache(maxsize=None)
def golden_sets(name):
    """(nbits, select_off, select_list, allow words) of a cluster: kano_py's
    own fields where the expected record stores them, else the C oracle's."""
    exp = expected(name)
    if "allow" in exp:
        n = exp["n"]
        off, flat = lists_to_csr(exp["select_policies"])
        return n, off, flat, rows01_to_words(exp["allow"], n)
    from oracle import kano_oracle as orc
    obj = cluster(name)
    ref = orc.run_c(obj, label=obj.get("label", "app"))
    return ref["n"], ref["select_off"], ref["select_list"], ref["allow"]


@functools.lru_cache(maxsize=None)
def golden_want(name):
    n, off, flat, aw = golden_sets(name)
    impact, pop = want_impact(off, flat, aw, n, with_popcount=True)
    impact.setflags(write=False)
    return impact, pop


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_records_cover_every_cluster():
    assert set(record_names()) >= set(cluster_names()) | {"paper_example",
                                                          "paper_example_rebuilt"}
    assert set(TABLE) == set(cluster_names()) | {"paper_example", "paper_example_rebuilt"}


@pytest.mark.parametrize("name", ALL_NAMES)
def test_restatement_equals_golden_record(name):
    impact, pop = golden_want(name)
    rec = record(name)
    assert (rec["n"], rec["P"]) == TABLE[name][:2]
    assert impact.tolist() == rec["impact"]
    assert np.flatnonzero(impact == 0).tolist() == rec["redundant"]
    assert pop == rec["popcount_M"]


@pytest.mark.parametrize("name", ALL_NAMES)
def test_records_and_restatement_reproduce_the_table(name):
    n, P, red, total, top, pop = TABLE[name]
    for imp, popm in ((record(name)["impact"], record(name)["popcount_M"]),
                      (golden_want(name)[0].tolist(), golden_want(name)[1])):
        assert len(imp) == P
        assert sum(1 for v in imp if v == 0) == red
        assert (sum(imp), max(imp), popm) == (total, top, pop)
        if name in IMPACT:
            assert imp == IMPACT[name]
        if name in REDUNDANT:
            assert [p for p, v in enumerate(imp) if v == 0] == REDUNDANT[name]
    assert record(name)["redundant"] == [p for p, v in enumerate(record(name)["impact"]) if v == 0]


@pytest.mark.parametrize("name", ALL_NAMES)
def test_sum_of_impacts_is_at_most_popcount(name):
    rec = record(name)
    assert 0 <= sum(rec["impact"]) <= rec["popcount_M"]
    assert all(v >= 0 for v in rec["impact"])


def test_both_outcomes_occur_in_every_size_range():
    for names in (("q_shadow", "q_types"), ("s_sparse_50", "s_sparse_200"),
                  ("s_sparse_2000", "q_wide_select")):
        recs = [record(k) for k in names]
        assert any(r["redundant"] for r in recs)
        assert any(len(r["redundant"]) < r["P"] for r in recs)


def test_library_exports_the_entry_points():
    from kano import _native as nat
    assert "kano_policy_impact" in nat.SIGNATURES and "kano_policy_impact_lists" in nat.SIGNATURES
    lib = ctypes.CDLL(nat.LIB_PATH)
    assert lib.kano_policy_impact is not None
    assert lib.kano_policy_impact_lists is not None


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def need_gpu():
    from kano import _native
    if not _native.gpu_available():
        pytest.fail("GPU test run without a usable HIP device / libkano_hip.so")


gpu = pytest.mark.gpu


def api_objects(obj):
    from kano import model
    from kano.synth import objects_from_json
    return objects_from_json(obj, model)


def cluster_tables(name):
    from kano._intern import intern
    return intern(*api_objects(cluster(name)))


def policy_sets(ps, n):
    """(select_off, select_list, allow words) of the policies' working sets."""
    from kano._bits import set_bit_indices
    lists = [[] for _ in range(n)]
    W = (n + 63) // 64
    aw = np.zeros((len(ps), W), np.uint64)
    for p, pol in enumerate(ps):
        for i in set_bit_indices(pol.working_select_set.words(), n).tolist():
            lists[i].append(p)
        aw[p] = pol.working_allow_set.words()[:W]
    off, flat = lists_to_csr(lists)
    return off, flat, aw


@gpu
@pytest.mark.parametrize("name", cluster_names())
def test_golden_cluster_api(name, need_gpu):
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = api_objects(cluster(name))
    m = ReachabilityMatrix.build_matrix(cs, ps)
    assert alg._fast_path(m, ps, cs)
    rec = record(name)
    got = alg.policy_impact(m, ps, cs)
    assert got.dtype == np.int64 and got.shape == (rec["P"],)
    assert got.tolist() == rec["impact"]
    assert alg.policy_redundant(m, ps, cs) == rec["redundant"]
    n, P, red, total, top, pop = TABLE[name]
    assert (len(cs), len(ps), len(alg.policy_redundant(m, ps, cs))) == (n, P, red)
    assert (int(got.sum()), int(got.max())) == (total, top)


@gpu
def test_paper_example_and_its_rebuilt_form(need_gpu):
    """Quirk Q5: a second build on the same containers doubles their lists;
    the definition is over the sets, so the general path (kano_policy_impact_lists
    over the working sets) answers as the first build does."""
    from sample import paper_example
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = paper_example()
    m = ReachabilityMatrix.build_matrix(cs, ps)
    assert alg._fast_path(m, ps, cs)
    assert alg.policy_impact(m, ps, cs).tolist() == [2, 1, 0, 4] == record("paper_example")["impact"]
    assert alg.policy_redundant(m, ps, cs) == [2]
    m2 = ReachabilityMatrix.build_matrix(cs, ps)
    assert not alg._fast_path(m2, ps, cs)
    assert alg.policy_impact(m2, ps, cs).tolist() == [2, 1, 0, 4]
    assert alg.policy_impact(m2, ps, cs).tolist() == record("paper_example_rebuilt")["impact"]
    assert alg.policy_redundant(m2, ps, cs) == [2] == record("paper_example_rebuilt")["redundant"]


@gpu
def test_general_path_needs_working_sets(need_gpu):
    from sample import paper_example
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = paper_example()
    ReachabilityMatrix.build_matrix(cs, ps)
    m2 = ReachabilityMatrix.build_matrix(cs, ps)
    fresh = paper_example()[1][1]             # never built: its working sets are None
    assert fresh.working_select_set is None
    with pytest.raises(ValueError, match=r"\bpolicy 1\b"):
        alg.policy_impact(m2, [ps[0], fresh, ps[2], ps[3]], cs)


def _bits_row(idx, nbits):
    W = (nbits + 63) // 64
    b = np.zeros(W * 64, np.uint8)
    b[list(idx)] = 1
    return np.packbits(b, bitorder="little").view("<u8")


def _lists_both_modes(lists, nbits, aw, literal, monkeypatch):
    """impact_from_lists in both modes and both kernel forms against the
    restatement and the literal expectation."""
    from kano._engine import impact_from_lists
    off, flat = lists_to_csr([list(map(int, l)) for l in lists])
    want = want_impact(off, flat, aw, nbits)
    if literal is not None:
        assert want.tolist() == list(literal)
    for form in ("", "impf=1", "impf=2"):
        monkeypatch.setenv("KANO_TUNE", form)
        got = impact_from_lists(len(lists), nbits, off, flat, aw)
        assert got.dtype == np.int64 and got.tolist() == want.tolist(), form
        ess = impact_from_lists(len(lists), nbits, off, flat, aw, flags_only=True)
        assert ess.dtype == bool and ess.tolist() == (want > 0).tolist(), form
    return want


@gpu
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_cover_count_saturates(k, monkeypatch, need_gpu):
    """k identical policies over 3 lists x 3 pods: alone a policy owns all 9
    pairs, with any copy none.  A counter wrapping at 2 fails k = 3, one
    wrapping at 4 fails k = 5."""
    aw = np.stack([_bits_row(range(3), 3)] * k)
    literal = [9] if k == 1 else [0] * k
    _lists_both_modes([list(range(k))] * 3, 3, aw, literal, monkeypatch)


@gpu
@pytest.mark.parametrize("nbits", [63, 64, 65, 129])
def test_word_edges(nbits, monkeypatch, need_gpu):
    aw = np.stack([_bits_row(range(nbits), nbits), _bits_row([nbits - 1], nbits),
                   _bits_row([min(64, nbits - 1)], nbits)])
    _lists_both_modes([[0, 1], [2]], nbits, aw, [nbits - 1, 0, 1], monkeypatch)


@gpu
def test_empty_select_and_empty_allow(monkeypatch, need_gpu):
    nbits = 70
    aw = np.stack([_bits_row(range(10), nbits), _bits_row(range(5, 70), nbits),
                   _bits_row([], nbits), _bits_row(range(3), nbits)])
    # policy 2 allows nothing, policy 3 is in no list; list 2 is empty
    want = _lists_both_modes([[0, 1, 2], [1, 2], [], [0]], nbits, aw, None, monkeypatch)
    assert want[2] == 0 and want[3] == 0 and want[0] > 0 and want[1] > 0
    assert want.tolist() == [5 + 10, 60 + 65, 0, 0]


@gpu
def test_policy_ids_across_words(monkeypatch, need_gpu):
    """P = 130: ids in three 64-bit words; lists long enough for several
    rounds of every wave, allow sets that overlap in part."""
    rng = np.random.default_rng(20240917)
    P, nbits = 130, 200
    aw = np.stack([_bits_row(rng.choice(nbits, size=rng.integers(0, 40), replace=False), nbits)
                   for _ in range(P)])
    lists = [rng.choice(P, size=k, replace=False) for k in (130, 1, 0, 64, 65, 7, 129, 2)]
    lists += [rng.choice(P, size=rng.integers(0, 6), replace=False) for _ in range(300)]
    want = _lists_both_modes(lists, nbits, aw, None, monkeypatch)
    assert (want == 0).any() and (want > 0).any()


@gpu
def test_error_codes(need_gpu):
    from kano import _native as nat
    from kano._engine import DeviceBuild, impact_from_lists
    aw = np.zeros((3, 1), np.uint64)
    off = np.array([0, 2, 4], np.int64)
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b"):
        impact_from_lists(2, 64, off, np.array([0, 1, 2, 2], np.int32), aw)    # repeated id
    for bad in (3, -1):
        with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.ERANGE}\b"):
            impact_from_lists(2, 64, off, np.array([0, 1, 2, bad], np.int32), aw)
    for mode in (2, -1):
        with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b"):
            impact_from_lists(2, 64, off, np.array([0, 1, 2, 1], np.int32), aw, mode=mode)
    # the same id in two lists is fine; degenerate sizes: no lists, no policies
    assert impact_from_lists(2, 64, off, np.array([0, 1, 0, 1], np.int32), aw).tolist() == [0] * 3
    assert impact_from_lists(0, 0, np.zeros(1, np.int64), np.zeros(0, np.int32),
                             np.zeros((0, 0), np.uint64)).shape == (0,)
    eng = DeviceBuild(cluster_tables("q_shadow"))
    for mode in (2, -1):
        rc = eng.lib.kano_policy_impact(eng.ctx, mode, None, None, None)
        assert rc == -errno.EINVAL
    assert eng.policy_impact().tolist() == record("q_shadow")["impact"]   # still usable
    eng.close()


@gpu
@pytest.mark.parametrize("form", ["", "impf=1", "impf=2"])
@pytest.mark.parametrize("name", ["q_wide_select", "s_sparse_2000"])
def test_device_build_against_the_oracle_sets(name, form, monkeypatch, need_gpu):
    from kano._engine import DeviceBuild
    monkeypatch.setenv("KANO_TUNE", form)
    want, _ = golden_want(name)
    assert want.tolist() == record(name)["impact"]
    eng = DeviceBuild(cluster_tables(name))
    info = eng.info()
    assert info["UA"] > 64 and info["MAXSEL"] >= 8     # column classes span words, large S(c)
    assert np.array_equal(eng.policy_impact(), want)
    assert np.array_equal(eng.policy_essential(), want > 0)
    n_red = ctypes.c_int64(-1)
    ess = np.zeros(want.shape[0], np.uint8)
    eng._chk(eng.lib.kano_policy_impact(eng.ctx, 1, None, ess.ctypes.data, ctypes.byref(n_red)),
             "kano_policy_impact")
    assert n_red.value == int((want == 0).sum()) and np.array_equal(ess.astype(bool), want > 0)
    eng.close()


@gpu
@pytest.mark.parametrize("name", ["q_wide_select", "s_sparse_2000"])
@pytest.mark.parametrize("G", [2, 3])
def test_row_shards_add_up(name, G, need_gpu):
    from kano._engine import DeviceBuild
    from kano.multi import MultiBuild
    want, _ = golden_want(name)
    t = cluster_tables(name)
    n = t.n
    even = [(n * g // G, n * (g + 1) // G) for g in range(G)]
    # (and G shards whose first ones hold a single row each: an even split of
    # q_wide_select leaves every row class a member in every shard)
    skewed = [(g, g + 1) for g in range(G - 1)] + [(G - 1, n)]
    # the inputs: the row classes are the pods' distinct sets of selecting
    # policies, and some shard holds a row class without a local member
    _, off, flat, _ = golden_sets(name)
    keys = [frozenset(flat[off[i]:off[i + 1]].tolist()) for i in range(n)]
    ids = {k: c for c, k in enumerate(dict.fromkeys(keys))}
    cls = np.array([ids[k] for k in keys])
    assert any(np.setdiff1d(cls, cls[r0:r1]).size > 0 for r0, r1 in skewed)
    if name == "s_sparse_2000":
        assert any(np.setdiff1d(cls, cls[r0:r1]).size > 0 for r0, r1 in even)
    for bounds in (even, skewed):
        total = np.zeros(want.shape[0], np.int64)
        flags = np.zeros(want.shape[0], bool)
        for r0, r1 in bounds:
            e = DeviceBuild(t, rows=(r0, r1))
            part = e.policy_impact()
            assert (part >= 0).all() and (part <= want).all()
            assert np.array_equal(e.policy_essential(), part > 0)
            total += part
            flags |= e.policy_essential()
            e.close()
        assert np.array_equal(total, want)
        assert np.array_equal(flags, want > 0)
    mb = MultiBuild(t, G, devices=[0] * G)
    assert np.array_equal(mb.policy_impact(), want)
    assert mb.policy_impact().dtype == np.int64
    assert np.array_equal(mb.policy_essential(), want > 0)
    mb.close()


def _bit_difference(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


@gpu
@pytest.mark.parametrize("name", ["paper_example", "q_shadow", "s_sparse_50"])
def test_removing_one_policy_changes_impact_bits(name, need_gpu):
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg

    def objects():
        if name == "paper_example":
            from sample import paper_example
            return paper_example()
        return api_objects(cluster(name))

    impact = record(name)["impact"]
    for p in range(len(impact)):
        cs, ps = objects()
        m = ReachabilityMatrix.build_matrix(cs, ps)
        if p == 0:
            assert alg.policy_impact(m, ps, cs).tolist() == impact
        before = m.row_bytes().copy()
        m.remove_policies([p])
        after = m.row_bytes()
        assert _bit_difference(before, after) == impact[p], p
        if impact[p] == 0:
            assert np.array_equal(before, after), p


@gpu
def test_after_adding_a_duplicate_policy(need_gpu):
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    name = "s_sparse_200"
    obj = cluster(name)
    cs, ps = api_objects(obj)
    m = ReachabilityMatrix.build_matrix(cs, ps)
    base = alg.policy_impact(m, ps, cs)
    assert base.tolist() == record(name)["impact"] and base[0] > 0
    copy = api_objects(dict(obj, policies=obj["policies"][:1]))[1][0]
    m.add_policies([copy])
    assert len(ps) == len(base) + 1 and not alg._fast_path(m, ps, cs)
    off, flat, aw = policy_sets(ps, len(cs))
    want = want_impact(off, flat, aw, len(cs))
    got = alg.policy_impact(m, ps, cs)
    assert got.tolist() == want.tolist()
    assert got[0] == 0 and got[-1] == 0
    assert got[1:-1].tolist() == base[1:].tolist()        # (nobody else shared policy 0's cells)
    assert alg.policy_redundant(m, ps, cs) == np.flatnonzero(want == 0).tolist()


@gpu
def test_sums_are_64_bit(need_gpu):
    """70,000 pods of one label, one policy selecting and allowing all: one
    row class, one column class, 4.9e9 pairs -- the accumulation width."""
    from kano import model
    from kano._engine import DeviceBuild
    from kano._intern import intern
    n = 70000
    cs = [model.Container(f"p{i}", {"app": "a"}) for i in range(n)]
    ps = [model.Policy("all", model.PolicySelect({"app": "a"}), model.PolicyAllow({"app": "a"}),
                       model.PolicyIngress, model.PolicyProtocol([]))]
    eng = DeviceBuild(intern(cs, ps), build=False)
    eng.build_classes()                        # (the class tables; no 600 MB matrix)
    info = eng.info()
    assert (info["U"], info["UA"]) == (1, 1)
    assert n * n > 2 ** 32
    assert eng.policy_impact().tolist() == [n * n]
    assert eng.policy_essential().tolist() == [True]
    eng.close()


@gpu
def test_shadow_conflict_and_impact_results_are_separate(need_gpu):
    from kano._engine import DeviceBuild
    import test_conflict as tc
    name = "s_broad_300"
    exp = expected(name)["policy_shadow"]
    _, conflicts = tc.golden_want(name)
    want, _ = golden_want(name)
    eng = DeviceBuild(cluster_tables(name))
    k = eng.shadow_count()
    assert k == exp["count"]
    assert np.array_equal(eng.conflict(), conflicts)
    assert np.array_equal(eng.policy_impact(), want)
    assert sha(eng.shadow_fetch(k)) == exp["sha256"]
    assert np.array_equal(eng.conflict_fetch(conflicts.shape[0]), conflicts)
    assert np.array_equal(eng.policy_essential(), want > 0)
    assert sha(eng.shadow_fetch(k)) == exp["sha256"]
    assert np.array_equal(eng.conflict_fetch(conflicts.shape[0]), conflicts)
    # and the other way round
    assert sha(eng.shadow()) == exp["sha256"]
    assert np.array_equal(eng.policy_impact(), want)
    assert np.array_equal(eng.conflict(), conflicts)
    assert np.array_equal(eng.policy_impact(), want)
    eng.close()


@gpu
def test_impact_between_pipelined_verify_steps(need_gpu):
    """A policy_impact() between two steps of a pipelined verify loop (a
    prologue is queued behind its gate then) leaves the next step's lists and
    pairs at their golden values, in pairs and in count-only mode."""
    from kano._engine import DeviceBuild
    from kano._intern import intern, group_ids
    name = "s_sparse_2000"
    obj = cluster(name)
    cs, ps = api_objects(obj)
    exp = expected(name)
    want, _ = golden_want(name)
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
            assert np.array_equal(eng.policy_impact(), want)
        if k in (2, 3):
            assert np.array_equal(eng.policy_essential(), want > 0)
    assert sha(eng.rows(0, len(cs))) == exp["M_sha256"]
    eng.close()
