"""The working policy_conflict (kano_conflict_pairs and the layers above it):
pairs (j, k) of policies selecting a common container whose allow sets share
no container.  The expectation everywhere is want_pairs below, a brute-force
numpy restatement of the predicate; the records under tests/golden/conflict/
hold its results on kano_py's own sets (tests/golden/make_conflict_golden.py).
"""
import errno
import functools
import json
import os

import numpy as np
import pytest

from _golden import GOLDEN, cluster, cluster_names, expected, lists_to_csr, rows01_to_words, sha

CONFLICT = os.path.join(GOLDEN, "conflict")

# candidate pairs / conflict pairs, brute-forced on kano_py's golden sets
TABLE = {
    "paper_example": (4, 2), "paper_example_rebuilt": (16, 8), "q_dirs": (48, 32),
    "q_shadow": (64, 32), "q_unknown_key": (6, 0), "s_sparse_50": (436, 144),
    "s_sparse_200": (2068, 1886), "s_broad_300": (15724, 10656),
    "s_broad_1000": (85918, 69136), "s_sparse_2000": (7042, 6962),
    "q_wide_select": (1035144, 1028168),
}
FIRST = {
    "paper_example": [(0, 3), (3, 0)],
    "paper_example_rebuilt": [(0, 3), (0, 3), (3, 0), (3, 0)],
    "q_dirs": [(0, 2), (0, 3), (2, 0), (2, 3)],
    "q_shadow": [(0, 2), (1, 2), (2, 0), (2, 1)],
}


def disjoint_matrix(allow_words, nbits):
    """D[j, k] = allow_j and allow_k share no bit (P x P bool)."""
    aw = np.ascontiguousarray(allow_words, dtype=np.uint64)
    P = aw.shape[0]
    if P == 0:
        return np.zeros((0, 0), bool)
    bits = np.unpackbits(aw.view(np.uint8).reshape(P, -1), axis=1, bitorder="little")
    bits = bits[:, :nbits].astype(np.float32)     # (counts <= nbits < 2^24: exact)
    return (bits @ bits.T) == 0


def want_pairs(select_off, select_list, allow_words, nbits=None, with_candidates=False):
    """For lists i ascending, j in S(i), k in S(i), both in list order, j == k
    skipped by value: (j, k) iff allow_j & allow_k is empty.  (T, 2) int32."""
    aw = np.asarray(allow_words, dtype=np.uint64)
    aw = aw.reshape(aw.shape[0], -1)
    if nbits is None:
        nbits = aw.shape[1] * 64
    D = disjoint_matrix(aw, nbits)
    off = np.asarray(select_off, dtype=np.int64)
    sl = np.asarray(select_list, dtype=np.int64)
    out, cand = [], 0
    for i in range(off.shape[0] - 1):
        S = sl[off[i]:off[i + 1]]
        if S.size < 2:
            continue
        jj, kk = np.repeat(S, S.size), np.tile(S, S.size)
        ne = jj != kk
        cand += int(ne.sum())
        keep = ne & D[jj, kk]
        out.append(np.stack([jj[keep], kk[keep]], axis=1))
    pairs = (np.concatenate(out) if out else np.zeros((0, 2))).astype(np.int32).reshape(-1, 2)
    return (cand, pairs) if with_candidates else pairs


def record(name):
    with open(os.path.join(CONFLICT, name + ".json")) as f:
        return json.load(f)


def record_names():
    return sorted(f[:-5] for f in os.listdir(CONFLICT))


def matches(pairs, rec):
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    return (pairs.shape[0] == rec["count"] and sha(pairs) == rec["sha256"] and
            pairs[:64].tolist() == rec["head"])


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
    cand, pairs = want_pairs(off, flat, aw, n, with_candidates=True)
    pairs.setflags(write=False)
    return cand, pairs


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_records_cover_every_cluster():
    assert set(record_names()) >= set(cluster_names()) | {"paper_example",
                                                          "paper_example_rebuilt"}


@pytest.mark.parametrize("name", record_names())
def test_restatement_equals_golden_record(name):
    cand, pairs = golden_want(name)
    rec = record(name)
    assert cand == rec["candidate_pairs"]
    assert matches(pairs, rec)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_restatement_reproduces_the_table(name):
    cand, pairs = golden_want(name)
    assert (cand, pairs.shape[0]) == TABLE[name]
    if name in FIRST:
        assert [tuple(p) for p in pairs[:len(FIRST[name])].tolist()] == FIRST[name]


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


@gpu
def test_paper_example_drop_in(need_gpu):
    from sample import paper_example
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = paper_example()
    m = ReachabilityMatrix.build_matrix(cs, ps)
    assert alg.policy_conflicts(m, ps, cs) == [(0, 3), (3, 0)]
    assert alg.policy_conflict_count(m, ps, cs) == 2
    assert matches(alg.policy_conflict_pairs(m, ps, cs), record("paper_example"))
    assert alg.policy_conflict_summary(m, ps, cs) == [(0, 3, 1)]
    with pytest.raises(AttributeError, match="'int' object has no attribute 'working_allow_set'"):
        alg.policy_conflict(m, ps, cs)


@gpu
def test_accumulated_lists_take_the_general_path(need_gpu):
    """Quirk Q5: a second build on the same containers doubles their lists;
    the pairs then come from kano_conflict_lists, duplicates included."""
    from sample import paper_example
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = paper_example()
    ReachabilityMatrix.build_matrix(cs, ps)
    m2 = ReachabilityMatrix.build_matrix(cs, ps)
    assert not alg._fast_path(m2, ps, cs)
    got = alg.policy_conflicts(m2, ps, cs)
    assert len(got) == 8
    assert got[:4] == [(0, 3), (0, 3), (3, 0), (3, 0)]
    assert matches(np.array(got, np.int32), record("paper_example_rebuilt"))
    assert alg.policy_conflict_count(m2, ps, cs) == 8
    # (the summary counts containers, not list entries)
    assert alg.policy_conflict_summary(m2, ps, cs) == [(0, 3, 1)]


@gpu
@pytest.mark.parametrize("name", cluster_names())
def test_golden_cluster_api(name, need_gpu):
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = api_objects(cluster(name))
    m = ReachabilityMatrix.build_matrix(cs, ps)
    rec = record(name)
    got = alg.policy_conflicts(m, ps, cs)
    assert matches(np.array(got, np.int32).reshape(-1, 2), rec)
    assert alg.policy_conflict_count(m, ps, cs) == rec["count"]
    if expected(name)["policy_conflict"].get("raises"):
        with pytest.raises(AttributeError):
            alg.policy_conflict(m, ps, cs)
    else:
        assert alg.policy_conflict(m, ps, cs) == []


def _rows(rng, P, nbits, k):
    """P allow rows of k random bits each over nbits, as (P, W) words."""
    W = (nbits + 63) // 64
    bits = np.zeros((P, W * 64), np.uint8)
    for p in range(P):
        bits[p, rng.choice(nbits, size=k, replace=False)] = 1
    return np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(P, W)


def _bits_row(idx, nbits):
    W = (nbits + 63) // 64
    b = np.zeros(W * 64, np.uint8)
    b[list(idx)] = 1
    return np.packbits(b, bitorder="little").view("<u8")


@functools.lru_cache(maxsize=None)
def crafted_cases():
    """(label, n_lists, nbits, soff, slist, allow words, want) -- the smallest
    shapes at which each path of k_conflict_test can go wrong."""
    rng = np.random.default_rng(20240611)
    cases = []

    def add(label, lists, nbits, aw):
        off, flat = lists_to_csr([list(map(int, l)) for l in lists])
        cand, want = want_pairs(off, flat, aw, nbits, with_candidates=True)
        cases.append((label, len(lists), nbits, off, flat, aw, want, cand))

    # one list of 1,100 policies: its S(c) segment is past the LDS staging
    # (the global form), the AC rows are three words
    aw = _rows(rng, 1100, 130, 9)
    add("wide", [rng.permutation(1100)], 130, aw)
    # 600 lists of 0-3 entries: many classes in one 256-pair block, empty and
    # single-entry lists among them
    add("short", [rng.integers(0, 1100, size=rng.integers(0, 4)) for _ in range(600)], 130, aw)
    # lists of 20-60: staged blocks that span classes, several rounds a block
    add("medium", [rng.choice(1100, size=rng.integers(20, 61), replace=False)
                   for _ in range(40)], 130, aw)
    for nbits in (64, 65):
        # rows: random, empty (0, 1), the top bit alone, a complementary pair
        # with nca sum == nbits (disjoint: no pigeonhole exit), and two rows
        # with nca sum > nbits (the pigeonhole exit)
        rows = [np.zeros((nbits + 63) // 64, np.uint64)] * 2
        rows += [_bits_row([nbits - 1], nbits), _bits_row(range(33), nbits),
                 _bits_row(range(33, nbits), nbits), _bits_row(range(nbits - 36, nbits), nbits),
                 _bits_row(range(0, nbits, 2), nbits)]
        rows += list(_rows(rng, 23, nbits, 5))
        aw2 = np.stack(rows)
        P = aw2.shape[0]
        lists = [np.arange(P), np.array([5, 7, 5, 9, 7, 0, 0]), np.array([3, 4]),
                 np.array([3, 5]), np.array([2, 2]), np.array([1])]
        lists += [rng.integers(0, P, size=rng.integers(0, 9)) for _ in range(30)]
        add(f"bits{nbits}", lists, nbits, aw2)
    return cases


def test_crafted_cases_exercise_both_outcomes():
    """On the reference result: conflicts and non-conflicts each make up at
    least 20 % of the tested pairs of the wide list; the pigeonhole pair and
    the complementary pair are what they were built to be."""
    by = {c[0]: c for c in crafted_cases()}
    want, cand = by["wide"][6], by["wide"][7]
    assert cand == 1100 * 1099
    assert 0.2 * cand <= want.shape[0] <= 0.8 * cand
    for nbits in (64, 65):
        _, _, _, off, flat, aw, want, _ = by[f"bits{nbits}"]
        cnt = np.array([bin(int(w)).count("1") for w in aw.reshape(-1)]).reshape(aw.shape).sum(1)
        assert cnt[3] + cnt[4] == nbits and cnt[3] + cnt[5] > nbits
        D = disjoint_matrix(aw, nbits)
        assert D[3, 4] and not D[3, 5]
        assert D[0, 1] and D[0, 6]            # (empty rows conflict with everything)


@gpu
@pytest.mark.parametrize("shr", [1, 2, 4, 8])
def test_crafted_lists_shapes(shr, monkeypatch, need_gpu):
    from kano._engine import conflict_from_lists
    monkeypatch.setenv("KANO_TUNE", f"shr={shr}")
    for label, n_lists, nbits, off, flat, aw, want, _ in crafted_cases():
        got = conflict_from_lists(n_lists, nbits, off, flat, aw)
        assert got.shape == want.shape, label
        assert np.array_equal(got, want), label
        assert conflict_from_lists(n_lists, nbits, off, flat, aw,
                                   count_only=True) == want.shape[0], label


@gpu
@pytest.mark.parametrize("name", ["q_wide_select", "s_sparse_2000"])
def test_device_build_against_the_oracle_sets(name, need_gpu):
    from kano._engine import DeviceBuild
    _, want = golden_want(name)
    assert want.shape[0] == TABLE[name][1]
    eng = DeviceBuild(cluster_tables(name))
    got = eng.conflict()
    assert np.array_equal(got, want)
    assert eng.conflict_count() == want.shape[0]
    # class level: expanding every class's list over its members gives the same
    off, pairs, members = eng.conflict_classes()
    assert int((np.diff(off) * members).sum()) == want.shape[0]
    eng.close()


@gpu
@pytest.mark.parametrize("name", ["q_wide_select", "s_sparse_2000"])
@pytest.mark.parametrize("G", [2, 3])
def test_row_shards_concatenate(name, G, need_gpu):
    from kano._engine import DeviceBuild
    from kano.multi import MultiBuild
    _, want = golden_want(name)
    t = cluster_tables(name)
    n = t.n
    bounds = [(n * g // G, n * (g + 1) // G) for g in range(G)]
    parts, total = [], 0
    for r0, r1 in bounds:
        e = DeviceBuild(t, rows=(r0, r1))
        parts.append(e.conflict())
        total += e.conflict_count()
        e.close()
    assert np.array_equal(np.concatenate(parts), want)
    assert total == want.shape[0]
    mb = MultiBuild(t, G, devices=[0] * G)
    assert np.array_equal(mb.conflict(), want)
    assert mb.conflict_count() == want.shape[0]
    mb.close()


@gpu
def test_shadow_and_conflict_results_are_separate(need_gpu):
    from kano._engine import DeviceBuild
    name = "s_broad_300"
    exp = expected(name)["policy_shadow"]
    _, want = golden_want(name)
    eng = DeviceBuild(cluster_tables(name))
    k = eng.shadow_count()
    assert k == exp["count"]
    got = eng.conflict()
    assert np.array_equal(got, want)
    assert sha(eng.shadow_fetch(k)) == exp["sha256"]
    # and the other way round
    assert sha(eng.shadow()) == exp["sha256"]
    assert np.array_equal(eng.conflict_fetch(want.shape[0]), want)
    eng.close()


@gpu
def test_conflict_between_pipelined_verify_steps(need_gpu):
    """A conflict() between two steps of a pipelined verify loop (a prologue
    is queued behind its gate then) leaves the next step's lists and pairs at
    their golden values, in pairs and in count-only mode."""
    from kano._engine import DeviceBuild
    from kano._intern import intern, group_ids
    name = "s_sparse_2000"
    obj = cluster(name)
    cs, ps = api_objects(obj)
    exp = expected(name)
    _, want = golden_want(name)
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
        if k == 1:
            assert np.array_equal(eng.conflict(), want)
        if k in (2, 3):
            assert eng.conflict_count() == want.shape[0]
        if k == 4:
            assert np.array_equal(eng.conflict(), want)
    assert sha(eng.rows(0, len(cs))) == exp["M_sha256"]
    eng.close()


@gpu
@pytest.mark.parametrize("name", ["s_broad_300", "q_shadow"])
def test_summary_equals_aggregated_pairs(name, need_gpu):
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    cs, ps = api_objects(cluster(name))
    m = ReachabilityMatrix.build_matrix(cs, ps)
    pairs = alg.policy_conflict_pairs(m, ps, cs)
    up = pairs[pairs[:, 0] < pairs[:, 1]]
    uniq, cnt = np.unique(up, axis=0, return_counts=True)
    want = [(int(j), int(k), int(c)) for (j, k), c in zip(uniq.tolist(), cnt.tolist())]
    assert want, "the cluster has conflicts"
    assert alg.policy_conflict_summary(m, ps, cs) == want


@gpu
def test_error_codes(need_gpu):
    from kano import _native as nat
    from kano._engine import DeviceBuild, conflict_from_lists
    eng = DeviceBuild(cluster_tables("q_shadow"))
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b"):
        eng.conflict_fetch(1)                 # before any kano_conflict_pairs
    n = eng.conflict_count()
    assert n == record("q_shadow")["count"]
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b"):
        eng.conflict_fetch(n)                 # after a count-only run
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b"):
        eng._conflict_run(2)                  # unknown mode
    assert matches(eng.conflict(), record("q_shadow"))     # the context is still usable
    eng.build()                               # a new build drops the old pairs
    with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.EINVAL}\b"):
        eng.conflict_fetch(n)
    eng.close()
    off = np.array([0, 2], np.int64)
    aw = np.zeros((3, 1), np.uint64)
    for bad in (3, -1):
        with pytest.raises(nat.KanoNativeError, match=rf"rc=-{errno.ERANGE}\b"):
            conflict_from_lists(1, 64, off, np.array([0, bad], np.int32), aw)
    # degenerate sizes: no lists, no policies
    assert conflict_from_lists(0, 0, np.zeros(1, np.int64), np.zeros(0, np.int32),
                               np.zeros((0, 0), np.uint64)).shape == (0, 2)
