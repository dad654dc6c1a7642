"""verdict_matrix / pair_verdicts (kano_verdict_matrix, kano_pair_verdicts and
the layers above them): deny rules and tiers.  Over the working sets of the
matrix's current policies every policy p carries an action and an integer
priority (a smaller number is evaluated first); p matches (i, j) iff i in
select_p and j in allow_p, t*(i, j) is the smallest priority over the matching
policies and
  verdict(i, j) = none   nothing matches
                  deny   some deny policy of priority t* matches
                  allow  otherwise
  decider(i, j) = the smallest index among the matching policies of priority
                  t* with the winning action
The expectation everywhere is the literal numpy restatement below over
kano_py's golden sets (test_ports.golden_dense); the reference has no deny
rules, so the actions and priorities are given to the golden clusters'
policies by the rule of tier_rule.  Exact bits and integers throughout.
"""
import ctypes
import errno
import functools
import re
import types

import numpy as np
import pytest

from _golden import cluster, expected, sha
import test_explain as te
import test_ports as tp
import test_redundancy as tr

ALL_NAMES = tr.ALL_NAMES
LEVELS = (1, 3, 70)
NON_VACUOUS = ("q_wide_select", "s_broad_1000", "s_broad_300", "s_sparse_200", "s_sparse_50")


# --------------------------------------------------------------------------
# the tier rule and the restatement
# --------------------------------------------------------------------------
def priority_table(L):
    """Level -> priority, never the identity: the int32 extremes for L = 3, a
    shuffled, gapped, partly negative table for L = 70."""
    if L == 1:
        return (5,)
    if L == 3:
        return (-2147483648, 0, 2147483647)
    return tuple(((l * 37) % L - 30) * 1000 + 7 * (l % 3) for l in range(L))


def tier_rule(P, L):
    """(deny bool (P,), priority int64 (P,)): deny[p] = (p % 3 == 1), level
    (p*5 + p//7) % L mapped through priority_table."""
    p = np.arange(P)
    table = np.array(priority_table(L), dtype=np.int64)
    return p % 3 == 1, table[(p * 5 + p // 7) % L]


def want_verdict(sel, allow, deny, prio):
    """(allowed, denied) as bool (n, n) arrays: the levels in ascending
    priority, literally."""
    n = sel.shape[1]
    verdict = np.zeros((n, n), dtype=bool)
    decided = np.zeros((n, n), dtype=bool)
    denied = np.zeros((n, n), dtype=bool)
    for t in sorted(set(prio.tolist())):
        a = tp.want_subset(sel, allow, (prio == t) & ~deny)
        d = tp.want_subset(sel, allow, (prio == t) & deny)
        new = (a | d) & ~decided
        verdict |= new & a & ~d
        denied |= new & d
        decided |= a | d
    return verdict, denied


@functools.lru_cache(maxsize=None)
def golden_verdict(name, L):
    n, sel, allow = tp.golden_dense(name)
    deny, prio = tier_rule(sel.shape[0], L)
    v, d = want_verdict(sel, allow, deny, prio)
    v.setflags(write=False)
    d.setflags(write=False)
    return v, d


def want_pairs(sel, allow, deny, prio, pairs):
    """pair_verdicts, literally: (verdict uint8, priority int32, policy int32)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Q, P = pairs.shape[0], sel.shape[0]
    verdict = np.zeros(Q, np.uint8)
    priority = np.zeros(Q, np.int32)
    policy = np.full(Q, -1, np.int32)
    if P == 0 or Q == 0:
        return verdict, priority, policy
    hit = sel[:, pairs[:, 0]] & allow[:, pairs[:, 1]]                  # (P, Q)
    big = np.int64(2) ** 40
    best = np.where(hit, prio[:, None], big).min(axis=0)
    top = hit & (prio[:, None] == best[None, :])
    dn = (top & deny[:, None]).any(axis=0)
    win = top & (deny[:, None] == dn[None, :])
    some = hit.any(axis=0)
    verdict[:] = np.where(some, np.where(dn, 2, 1), 0)
    priority[:] = np.where(some, best, 0)
    policy[:] = np.where(some, win.argmax(axis=0), -1)
    return verdict, priority, policy


def deny_class_bounds(sel, deny, r0, r1):
    """Bounds on the row classes of rows [r0, r1) that hold a deny policy: pods
    of one class share their policy list, so at least the distinct lists with
    a deny policy and at most the rows with one."""
    cols = sel[:, r0:r1][:, sel[deny][:, r0:r1].any(axis=0)]
    return np.unique(cols, axis=1).shape[1], cols.shape[1]


def sample_pairs(name, n):
    """All pairs for n <= 300, 1000 seeded pairs beyond."""
    if n <= 300:
        return tp.all_pairs(n)
    return np.random.default_rng(len(name) + n).integers(0, n, (1000, 2)).astype(np.int32)


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------
def test_priority_tables_are_no_identity():
    for L in (3, 70):
        t = priority_table(L)
        assert len(set(t)) == L and list(t) != list(range(L))
    t = priority_table(70)
    assert list(t) != sorted(t) and min(t) < 0 < max(t)
    assert min(np.diff(sorted(t))) > 1
    assert np.iinfo(np.int32).min in priority_table(3) and np.iinfo(np.int32).max in priority_table(3)


@pytest.mark.parametrize("name", NON_VACUOUS)
def test_restatement_is_not_vacuous(name):
    """With the rule at L = 3 some pairs are tied at t* between an allow and a
    deny, some verdicts differ from 'any deny wins' and some from 'any allow
    wins'; L = 1 is deny-wins."""
    n, sel, allow = tp.golden_dense(name)
    P = sel.shape[0]
    deny, prio = tier_rule(P, 3)
    v, d = golden_verdict(name, 3)
    any_allow = tp.want_subset(sel, allow, ~deny)
    any_deny = tp.want_subset(sel, allow, deny)
    assert np.array_equal(v | d, any_allow | any_deny) and not (v & d).any()
    tied = np.zeros((n, n), dtype=bool)
    decided = np.zeros((n, n), dtype=bool)
    for t in sorted(set(prio.tolist())):
        a = tp.want_subset(sel, allow, (prio == t) & ~deny)
        dd = tp.want_subset(sel, allow, (prio == t) & deny)
        tied |= a & dd & ~decided
        decided |= a | dd
    counts = (int(tied.sum()), int((v != (any_allow & ~any_deny)).sum()),
              int((v != any_allow).sum()))
    print(name, counts)
    assert all(c > 0 for c in counts)
    known = {"q_wide_select": (10988, 7811, 21644), "s_sparse_50": (115, 184, 115)}
    if name in known:
        assert counts == known[name]
    v1, _ = golden_verdict(name, 1)
    assert np.array_equal(v1, any_allow & ~any_deny)
    # the pairs' restatement agrees with the matrix's
    pairs = sample_pairs(name, n)
    verdict, priority, policy = want_pairs(sel, allow, deny, prio, pairs)
    assert np.array_equal(verdict == 1, v[pairs[:, 0], pairs[:, 1]])
    assert np.array_equal(verdict == 2, d[pairs[:, 0], pairs[:, 1]])
    hit = policy >= 0
    assert np.array_equal(hit, verdict > 0)
    assert np.array_equal(prio[policy[hit]], priority[hit])
    assert np.array_equal(deny[policy[hit]], verdict[hit] == 2)


def test_ties_survive_seventy_levels():
    n, sel, allow = tp.golden_dense("q_wide_select")
    deny, prio = tier_rule(sel.shape[0], 70)
    assert len(set(prio.tolist())) == 70
    tied, decided = 0, np.zeros((n, n), dtype=bool)
    for t in sorted(set(prio.tolist())):
        a = tp.want_subset(sel, allow, (prio == t) & ~deny)
        d = tp.want_subset(sel, allow, (prio == t) & deny)
        tied += int((a & d & ~decided).sum())
        decided |= a | d
    assert tied == 10


def _pol(**kw):
    return types.SimpleNamespace(name="web", **kw)


def test_tiering_forms_and_errors():
    from kano.verdicts import ALLOW, DENY, Tiering, resolve, tiering
    t = tiering([_pol(), _pol(action="DENY", priority=-5), _pol(action="Allow"),
                 _pol(action=DENY, priority=np.int64(2 ** 31 - 1)),
                 _pol(action=ALLOW, priority=-2 ** 31), _pol(action=np.uint8(1))])
    assert t.actions.dtype == np.uint8 and t.actions.tolist() == [0, 1, 0, 1, 0, 1]
    assert t.priorities.dtype == np.int32
    assert t.priorities.tolist() == [0, -5, 0, 2 ** 31 - 1, -2 ** 31, 0]
    assert len(t) == 6 and len(tiering([])) == 0
    e = Tiering(["deny", "ALLOW", 1], (3, 2, 1))
    assert e.actions.tolist() == [1, 0, 1] and e.priorities.tolist() == [3, 2, 1]
    for bad in ("pass", "", None, 2, -1, True, 1.0, b"deny"):
        with pytest.raises(ValueError, match="web"):
            tiering([_pol(action=bad)])
        with pytest.raises(ValueError):
            Tiering([bad], [0])
    for bad in (True, False, 1.5, "1", None, 2 ** 31, -2 ** 31 - 1, np.bool_(True)):
        with pytest.raises(ValueError, match="web"):
            tiering([_pol(priority=bad)])
        with pytest.raises(ValueError):
            Tiering(["allow"], [bad])
    with pytest.raises(ValueError):
        Tiering(["allow"], [1, 2])
    ps = [_pol(action="deny"), _pol(priority=4)]
    assert resolve(ps, None).actions.tolist() == [1, 0]
    assert resolve(ps, (["allow", "deny"], [1, 2])).priorities.tolist() == [1, 2]
    assert resolve(ps, e if len(e) == 2 else Tiering([0, 1], [0, 0])).actions.tolist() == [0, 1]
    for bad in (e, (["allow"], [0]), 5, (["allow", "deny"],)):
        with pytest.raises(ValueError):
            resolve(ps, bad)


def test_the_policy_dataclass_is_unchanged():
    import dataclasses
    from kano.model import Policy
    assert [f.name for f in dataclasses.fields(Policy)][:5] == \
        ["name", "selector", "allow", "direction", "protocol"]
    assert not {"action", "priority"} & {f.name for f in dataclasses.fields(Policy)}


def test_library_exports_the_entry_points():
    from kano import _native as nat
    lib = ctypes.CDLL(nat.LIB_PATH)
    for sym in ("kano_verdict_matrix", "kano_pair_verdicts", "kano_verdict_matrix_time",
                "kano_pair_verdicts_time"):
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
PAIR_FORMS = ("", "pvf=1", "pvf=2", "pvf=1,pvgrid=1", "pvf=2,pvgrid=2")
rows_of = tp.rows_of
to_words = tp.to_words


def carry(ps, deny, prio):
    """The tiers as plain attributes of the policy objects."""
    for p, pol in enumerate(ps):
        pol.action = "deny" if deny[p] else "allow"
        pol.priority = int(prio[p])


def built(name, L, drop=0):
    """(containers, policies, matrix) of a golden cluster whose policies carry
    the rule's tiers, without its last ``drop`` policies."""
    from kano.model import ReachabilityMatrix
    cs, ps = te.api_objects_of(name)
    if drop:
        del ps[len(ps) - drop:]
    carry(ps, *tier_rule(len(ps), L))
    return cs, ps, ReachabilityMatrix.build_matrix(cs, ps)


def check_verdicts(m, sel, allow, deny, prio, pairs, tiers=None, want=None, counts=True):
    """verdict_matrix, verdict_counts and pair_verdicts of the matrix against
    the restatement over (sel, allow, deny, prio)."""
    from kano import algorithm as alg
    v, d = want if want is not None else want_verdict(sel, allow, deny, prio)
    vm = alg.verdict_matrix(m, tiers)
    assert vm._policies is None
    assert np.array_equal(rows_of(vm), to_words(v))
    assert vm.verdict_info["allow_policies"] == int((~deny).sum())
    assert vm.verdict_info["deny_policies"] == int(deny.sum())
    assert vm.verdict_info["levels"] == len(set(prio.tolist()))
    vm._engine.close()
    if counts:
        n = sel.shape[1]
        assert alg.verdict_counts(m, tiers) == dict(
            allowed=int(v.sum()), denied=int(d.sum()), unmatched=n * n - int(v.sum() + d.sum()))
    got = alg.pair_verdicts(m, pairs, tiers)
    wv, wp, wi = want_pairs(sel, allow, deny, prio, pairs)
    assert got.verdict.dtype == np.uint8 and np.array_equal(got.verdict, wv)
    assert got.priority.dtype == np.int32 and np.array_equal(got.priority, wp)
    assert got.policy.dtype == np.int32 and np.array_equal(got.policy, wi)
    assert np.array_equal(got.allowed(), wv == 1) and np.array_equal(got.denied(), wv == 2)
    return v, d, (wv, wp, wi)


def check_why_blocked(m, sel, allow, deny, prio, pairs, verdict, tiers=None, limit=8):
    """why_blocked on up to ``limit`` pairs of every verdict against the dense
    sets (the deny policies of priority t* matching the pair, literally) and
    against a host filter of pair_policies."""
    from kano import algorithm as alg
    for kind in (0, 1, 2):
        for q in np.flatnonzero(verdict == kind)[:limit].tolist():
            i, j = map(int, pairs[q])
            match = sel[:, i] & allow[:, j]
            top = match & (prio == prio[match].min()) if match.any() else match
            dense = np.flatnonzero(top & deny).tolist()
            hit = alg.why_reachable(m, i, j)
            best = min((int(prio[p]) for p in hit), default=None)
            want = [p for p in hit if int(prio[p]) == best and deny[p]]
            assert want == dense and (len(want) > 0) == (kind == 2)
            assert alg.why_blocked(m, i, j, tiers) == dense
            name = ("none", "allow", "deny")[kind]
            assert alg.pair_verdict(m, i, j, tiers)[0] == name


@gpu
def test_paper_example_by_hand(need_gpu):
    """Policy C (2) and policy D (3) both match (2, 0).  C as a deny at a later
    priority than D leaves the pair allowed; at an earlier one it blocks it."""
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    from sample import paper_example
    assert te.PAPER[(2, 0)] == [2, 3]
    only_c = {pr for pr, ids in te.PAPER.items() if ids == [2]}
    cs, ps = paper_example()
    m = ReachabilityMatrix.build_matrix(cs, ps)
    every = set(te.PAPER)
    bits = lambda vm: {(i, j) for i in range(5) for j in range(5) if vm[i, j]}   # noqa: E731
    assert bits(alg.verdict_matrix(m)) == every                   # no attributes: all allow
    ps[2].action, ps[2].priority = "deny", 7                      # later than D's 0
    both = {pr for pr, ids in te.PAPER.items() if 2 in ids and len(ids) > 1}
    assert (2, 0) in both
    assert bits(alg.verdict_matrix(m)) == every - only_c
    assert alg.pair_verdict(m, 2, 0) == ("allow", 0, 3)
    assert alg.why_blocked(m, 2, 0) == []
    ps[2].priority = -7                                           # earlier than D's
    assert bits(alg.verdict_matrix(m)) == every - only_c - both
    assert alg.pair_verdict(m, 2, 0) == ("deny", -7, 2)
    assert alg.why_blocked(m, 2, 0) == [2]
    ps[2].priority = 0                                            # the same: deny wins
    assert alg.pair_verdict(m, 2, 0) == ("deny", 0, 2)
    assert alg.pair_verdict(m, 4, 4) == ("none", None, None)
    pv = alg.pair_verdicts(m, tp.all_pairs(5))
    assert isinstance(pv, alg.PairVerdicts)
    for q, (i, j) in enumerate(tp.all_pairs(5).tolist()):
        ids = te.PAPER.get((i, j), [])
        want = ("none", None, None) if not ids else \
            ("deny", 0, 2) if 2 in ids else ("allow", 0, ids[0])
        assert pv.of(q) == want
    c = alg.verdict_counts(m)
    assert c == dict(allowed=len(every - only_c - both), denied=len(only_c | both),
                     unmatched=25 - len(every))
    # explicit sequences instead of the attributes
    t = alg.Tiering(["allow", "allow", "DENY", "allow"], [0, 0, 9, 0])
    assert alg.pair_verdict(m, 2, 0, t) == ("allow", 0, 3)
    assert alg.pair_verdict(m, 2, 0, (["allow"] * 4, [1, 2, 3, 4])) == ("allow", 3, 2)
    # the built matrix is untouched
    assert bits(m) == every


@gpu
@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("name", ALL_NAMES)
def test_golden_cluster(name, L, need_gpu):
    from kano import algorithm as alg
    n, sel, allow = tp.golden_dense(name)
    cs, ps, m = built(name, L)
    P = len(ps)
    deny, prio = tier_rule(P, L)
    before = rows_of(m)
    pairs = sample_pairs(name, n)
    v, d, (wv, _, _) = check_verdicts(m, sel, allow, deny, prio, pairs,
                                      want=golden_verdict(name, L))
    check_why_blocked(m, sel, allow, deny, prio, pairs, wv, limit=3)
    # all-allow with any priorities: the built matrix and the subset of all
    flat = alg.Tiering(["allow"] * P, prio.tolist())
    va = alg.verdict_matrix(m, flat)
    full = alg.policy_subset_matrix(m, range(P))
    assert np.array_equal(rows_of(va), before) and np.array_equal(rows_of(full), before)
    assert va.verdict_info["deny_policies"] == 0 and va.verdict_info["deny_classes"] == 0
    if L == 1:
        sa = alg.policy_subset_matrix(m, np.flatnonzero(~deny))
        sd = alg.policy_subset_matrix(m, np.flatnonzero(deny))
        assert np.array_equal(rows_of(sa) & ~rows_of(sd), to_words(v))
        sa._engine.close()
        sd._engine.close()
    # the matrix is untouched
    assert np.array_equal(rows_of(m), before)
    for mm in (va, full, m):
        mm._engine.close()


@gpu
@pytest.mark.parametrize("tune", ["pathlds=0,pvf=1", "pathlds=1,pvf=2", "pathlds=0,pvf=2,pvgrid=2",
                                  "pathlds=1,pvf=1,pvgrid=1"])
@pytest.mark.parametrize("name", ["q_types", "s_sparse_200", "s_broad_300", "q_wide_select"])
def test_both_expansions_and_pair_forms(name, tune, monkeypatch, need_gpu):
    """The class rows' expansion with its table in LDS and without, both forms
    of the pair kernel, over clusters with few and with many members per row
    class; q_wide_select has a row class of 321 policies (a list longer than
    the block) and more than 64 column classes (two words a class row)."""
    monkeypatch.setenv("KANO_TUNE", tune)
    n, sel, allow = tp.golden_dense(name)
    for L in (3, 70):
        cs, ps, m = built(name, L)
        deny, prio = tier_rule(len(ps), L)
        check_verdicts(m, sel, allow, deny, prio, sample_pairs(name, n),
                       want=golden_verdict(name, L), counts=False)
        info = m.engine.info()
        if name == "q_wide_select":
            assert info["UA"] > 64 and info["MAXSEL"] > 256
        m._engine.close()


@gpu
@pytest.mark.parametrize("Q", [0, 1, 63, 64, 65, 1000])
def test_query_sizes_duplicates_and_order(Q, monkeypatch, need_gpu):
    """Q around the wave and block sizes; the pairs unsorted, with duplicates;
    both forms of the kernel, grids of one and two blocks."""
    from kano._engine import DeviceBuild
    name = "s_sparse_200"
    n, sel, allow = tp.golden_dense(name)
    deny, prio = tier_rule(sel.shape[0], 3)
    rng = np.random.default_rng(23 + Q)
    pairs = rng.integers(0, n, (Q, 2)).astype(np.int32)
    if Q >= 63:
        pairs[Q // 2:Q // 2 + 20] = pairs[:20]
    wv, wp, wi = want_pairs(sel, allow, deny, prio, pairs)
    for form in PAIR_FORMS:
        monkeypatch.setenv("KANO_TUNE", form)
        eng = DeviceBuild(tr.cluster_tables(name))
        r = eng.pair_verdicts(pairs, prio, deny)
        assert r["verdict"].shape == (Q,), form
        assert np.array_equal(r["verdict"], wv) and np.array_equal(r["priority"], wp), form
        assert np.array_equal(r["policy"], wi), form
        assert r["counts"].tolist() == np.bincount(wv, minlength=3).tolist(), form
        eng.close()
    if Q >= 1000:
        assert set(wv.tolist()) == {0, 1, 2}


@gpu
@pytest.mark.parametrize("name", ["q_wide_select", "s_sparse_2000"])
@pytest.mark.parametrize("G", [2, 3])
def test_row_shards(name, G, need_gpu):
    from kano._engine import DeviceBuild
    from kano.multi import MultiBuild
    n, sel, allow = tp.golden_dense(name)
    tb = tr.cluster_tables(name)
    deny, prio = tier_rule(tb.P, 3)
    v, d = golden_verdict(name, 3)
    whole = to_words(v)
    pairs = te.record_arrays(name)[0]
    wv, wp, wi = want_pairs(sel, allow, deny, prio, pairs)
    cuts = [0] + [n * g // G + 7 * g for g in range(1, G)] + [n]
    assert all(c % 64 for c in cuts[1:-1])
    parts, acc_v, acc_i, counts = [], np.zeros_like(wv), np.full_like(wi, -1), np.zeros(3, np.int64)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        e = DeviceBuild(tb, rows=(r0, r1))
        dst = DeviceBuild.empty(n, rows=(r0, r1))
        info = e.verdict_into(dst, prio, deny)
        assert info["deny_policies"] == int(deny.sum()) and info["levels"] == 3
        lo, hi = deny_class_bounds(sel, deny, r0, r1)
        assert lo <= info["deny_classes"] <= hi
        parts.append(dst.rows(r0, r1 - r0))
        r = e.pair_verdicts(pairs, prio, deny)
        mine = (pairs[:, 0] >= r0) & (pairs[:, 0] < r1)
        assert np.array_equal(r["verdict"], np.where(mine, wv, 0))
        assert np.array_equal(r["policy"], np.where(mine, wi, -1))
        assert np.array_equal(r["priority"], np.where(mine, wp, 0))
        assert r["counts"].tolist() == np.bincount(wv[mine], minlength=3).tolist()
        acc_v = np.maximum(acc_v, r["verdict"])
        acc_i = np.maximum(acc_i, r["policy"])
        counts += r["counts"]
        e.close()
        dst.close()
    assert np.array_equal(np.concatenate(parts), whole)
    assert np.array_equal(acc_v, wv) and np.array_equal(acc_i, wi)
    assert counts.tolist() == np.bincount(wv, minlength=3).tolist()
    if G == 2:
        mb = MultiBuild(tb, 2, devices=[0, 0])
        md = MultiBuild.empty(n, 2, devices=[0, 0])
        info = mb.verdict_into(md, prio, deny)
        assert np.array_equal(md.rows(0, n), whole)
        # deny_classes: the members' sum, each member over the rows it holds
        bounds = [deny_class_bounds(sel, deny, a, b) for a, b in mb.bounds]
        assert sum(lo for lo, _ in bounds) <= info["deny_classes"] <= sum(hi for _, hi in bounds)
        assert info["deny_classes"] >= deny_class_bounds(sel, deny, 0, n)[0]
        r = mb.pair_verdicts(pairs, prio, deny)
        assert np.array_equal(r["verdict"], wv) and np.array_equal(r["policy"], wi)
        assert np.array_equal(r["priority"], wp)
        assert r["counts"].tolist() == np.bincount(wv, minlength=3).tolist()
        mb.close()
        md.close()


# ---- updated matrices ------------------------------------------------------
def _check_current(m, ps, n, pairs, fresh_of=None):
    """The queries against the restatement over the current policies' working
    sets and the tiers they carry (current indices); with ``fresh_of`` also
    against verdict_matrix on a fresh build of that list."""
    from kano.model import ReachabilityMatrix
    from kano.verdicts import tiering
    from kano import algorithm as alg
    off, flat, aw = tr.policy_sets(ps, n)
    sel, allow = tp.dense_sets(off, flat, aw, n)
    t = tiering(ps)
    deny, prio = t.actions.astype(bool), t.priorities.astype(np.int64)
    v, d, (wv, _, _) = check_verdicts(m, sel, allow, deny, prio, pairs)
    check_why_blocked(m, sel, allow, deny, prio, pairs, wv, limit=2)
    if fresh_of is not None:
        cs1, ps1 = fresh_of
        carry(ps1, deny, prio)
        m1 = ReachabilityMatrix.build_matrix(cs1, ps1)
        v1 = alg.verdict_matrix(m1)
        assert np.array_equal(rows_of(v1), to_words(v))
        for mm in (v1, m1):
            mm._engine.close()
    return v, d


@gpu
@pytest.mark.parametrize("name", ["paper_example", "q_shadow", "s_sparse_200"])
def test_updated_matrices(name, need_gpu):
    """Add two policies (a deny at the earliest level, an allow at a level of
    its own), remove a build policy and an added one: after every step the
    queries equal the restatement over the current list and verdict_matrix on
    a fresh build of that list."""
    P = tr.TABLE[name][1]
    cs, ps, m = built(name, 3, drop=2)
    n, P0 = len(cs), len(ps)
    pairs = te._query(name, n)
    base = list(range(P0))
    _check_current(m, ps, n, pairs)
    new = te._fresh(name, [P - 2, P - 1])
    new[0].action, new[0].priority = "deny", -2147483648
    new[1].action, new[1].priority = "allow", 12
    m.add_policies(new)
    assert len(ps) == P0 + 2
    v1, d1 = _check_current(m, ps, n, pairs,
                            fresh_of=(te.api_objects_of(name)[0],
                                      te._fresh(name, base + [P - 2, P - 1])))
    m.remove_policies([1])
    _check_current(m, ps, n, pairs,
                   fresh_of=(te.api_objects_of(name)[0],
                             te._fresh(name, [0] + base[2:] + [P - 2, P - 1])))
    m.remove_policies([len(ps) - 2])                       # the first added one: the deny
    assert len(ps) == P0
    _check_current(m, ps, n, pairs,
                   fresh_of=(te.api_objects_of(name)[0], te._fresh(name, [0] + base[2:] + [P - 1])))
    if name == "s_sparse_200":
        assert d1.any() and v1.any()
    m._engine.close()


@gpu
def test_only_added_policies(need_gpu):
    """A build without policies has no classes: the rows' kernel alone writes
    the matrix, the added part alone answers the pairs."""
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    from sample import paper_example
    cs, ps = paper_example()
    m = ReachabilityMatrix.build_matrix(cs, [])
    assert not rows_of(alg.verdict_matrix(m)).any()
    assert alg.pair_verdicts(m, [(0, 0)]).of(0) == ("none", None, None)
    assert alg.verdict_counts(m) == dict(allowed=0, denied=0, unmatched=25)
    ps[2].action, ps[2].priority = "deny", -3
    ps[3].priority = 4
    m.add_policies(list(ps))
    _check_current(m, m._policies, 5, tp.all_pairs(5))
    assert alg.pair_verdict(m, 2, 0) == ("deny", -3, 2)
    m.remove_policies([2])
    _check_current(m, m._policies, 5, tp.all_pairs(5))
    assert alg.pair_verdict(m, 2, 0) == ("allow", 4, 2)


# ---- composition -----------------------------------------------------------
@gpu
def test_queries_on_a_verdict_matrix(need_gpu):
    from kano.model import ReachabilityMatrix
    from kano import algorithm as alg
    name = "s_sparse_200"
    n, sel, allow = tp.golden_dense(name)
    cs, ps, m = built(name, 3)
    v, d = golden_verdict(name, 3)
    assert 0 < v.sum() < tr.TABLE[name][5] and d.any()
    vm = alg.verdict_matrix(m)
    ref = ReachabilityMatrix(n, v.astype(int).tolist())
    assert alg.all_isolated(vm) == alg.all_isolated(ref) == np.flatnonzero(~v.any(axis=0)).tolist()
    intents = [(range(0, 60), range(100, 180), "deny"), (range(20, 40), [3, 5, 150], "allow"),
               ([0], range(n), "deny")]
    a, b = alg.check_intents(vm, cs, intents), alg.check_intents(ref, cs, intents)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a.reachable.sum() > 0
    diff = alg.matrix_diff(m, vm)
    counts = alg.verdict_counts(m)
    assert (diff.added, diff.removed) == (0, counts["denied"]) and counts["denied"] == int(d.sum())


# ---- error codes and isolation ----------------------------------------------
@gpu
def test_errors(need_gpu):
    from kano.model import ReachabilityMatrix
    from kano._engine import DeviceBuild
    from kano import algorithm as alg
    cs, ps, m = built("q_shadow", 3)
    n, P = len(cs), len(ps)
    for other in (m.snapshot(), alg.two_hop(m), ReachabilityMatrix(n, [[0] * n] * n)):
        for call in (lambda o: alg.verdict_matrix(o), lambda o: alg.pair_verdicts(o, [(0, 0)]),
                     lambda o: alg.pair_verdict(o, 0, 0), lambda o: alg.why_blocked(o, 0, 0),
                     lambda o: alg.verdict_counts(o)):
            with pytest.raises(ValueError, match="no policies"):
                call(other)
    for bad in ([(n, 0)], [(0, -1)], [(0, 0), (0, n)]):
        with pytest.raises(IndexError):
            alg.pair_verdicts(m, bad)
    with pytest.raises(IndexError):
        alg.pair_verdict(m, 0, n)
    # wrong-length sequences, a bad action, a bool priority
    for bad in ((["allow"] * (P + 1), [0] * (P + 1)), (["allow"] * (P - 1), [0] * (P - 1)),
                (["allow"] * P, [0] * (P - 1)), (["pass"] + ["allow"] * (P - 1), [0] * P),
                (["allow"] * P, [True] + [0] * (P - 1))):
        for call in (lambda t: alg.verdict_matrix(m, t), lambda t: alg.pair_verdicts(m, [(0, 0)], t),
                     lambda t: alg.why_blocked(m, 0, 0, t), lambda t: alg.verdict_counts(m, t)):
            with pytest.raises(ValueError):
                call(bad)
    ps[0].action = "reject"
    with pytest.raises(ValueError, match=re.escape(ps[0].name)):
        alg.verdict_matrix(m)
    ps[0].action, ps[1].priority = "allow", False
    with pytest.raises(ValueError, match=re.escape(ps[1].name)):
        alg.pair_verdicts(m, [(0, 0)])
    # the C entry points
    eng = DeviceBuild(tr.cluster_tables("q_shadow"))
    dst, small, shard = DeviceBuild.empty(n), DeviceBuild.empty(n - 1), DeviceBuild.empty(
        n, rows=(0, n - 1))
    lib = eng.lib
    prio = np.arange(P, dtype=np.int32)
    act = (np.arange(P) % 3 == 1).astype(np.uint8)
    act2 = act.copy()
    act2[P - 1] = 2
    info = np.zeros(4, np.int64)
    ptr = lambda a: None if a is None else a.ctypes.data                      # noqa: E731
    vmx = lambda s, d, k, pr, ac: lib.kano_verdict_matrix(                      # noqa: E731
        s, d, k, ptr(pr), ptr(ac), info.ctypes.data)
    EINVAL, ERANGE = -errno.EINVAL, -errno.ERANGE
    assert vmx(None, dst.ctx, P, prio, act) == EINVAL and vmx(eng.ctx, None, P, prio, act) == EINVAL
    assert vmx(eng.ctx, eng.ctx, P, prio, act) == EINVAL
    assert vmx(eng.ctx, dst.ctx, P, None, act) == EINVAL
    assert vmx(eng.ctx, dst.ctx, P, prio, None) == EINVAL
    assert vmx(eng.ctx, dst.ctx, P + 1, prio, act) == EINVAL
    assert vmx(eng.ctx, dst.ctx, 0, prio, act) == EINVAL
    assert vmx(eng.ctx, dst.ctx, P, prio, act2) == EINVAL
    assert b"action" in lib.kano_last_error(dst.ctx)
    # the destination of a failed call is untouched and still answers
    assert not dst.rows(0, n).any() and dst.get_bit(0, 0) == 0
    assert vmx(eng.ctx, small.ctx, P, prio, act) == EINVAL
    assert vmx(eng.ctx, shard.ctx, P, prio, act) == EINVAL
    assert vmx(dst.ctx, small.ctx, 0, prio, act) == EINVAL
    assert b"no policies" in lib.kano_last_error(small.ctx)
    one = np.array([[0, 0]], np.int32)
    out = np.zeros(1, np.uint8)
    dp, di = np.zeros(1, np.int32), np.zeros(1, np.int32)
    cnt = np.zeros(3, np.int64)
    pvs = lambda c, q, prs, k, pr, ac, o, full=True: lib.kano_pair_verdicts(    # noqa: E731
        c, q, ptr(prs), k, ptr(pr), ptr(ac), ptr(o), ptr(dp) if full else None,
        ptr(di) if full else None, ptr(cnt) if full else None)
    assert pvs(None, 1, one, P, prio, act, out) == EINVAL
    assert pvs(eng.ctx, -1, one, P, prio, act, out) == EINVAL
    assert pvs(eng.ctx, 1, None, P, prio, act, out) == EINVAL
    assert pvs(eng.ctx, 1, one, P, None, act, out) == EINVAL
    assert pvs(eng.ctx, 1, one, P, prio, None, out) == EINVAL
    assert pvs(eng.ctx, 1, one, P, prio, act, None) == EINVAL
    assert pvs(eng.ctx, 1, one, P - 1, prio, act, out) == EINVAL
    assert pvs(eng.ctx, 1, one, P, prio, act2, out) == EINVAL
    assert pvs(dst.ctx, 1, one, 0, prio, act, out) == EINVAL
    assert b"no policies" in lib.kano_last_error(dst.ctx)
    for bad in ((n, 0), (0, n), (-1, 0), (0, -1)):
        assert pvs(eng.ctx, 1, np.array([bad], np.int32), P, prio, act, out) == ERANGE
    # a context holding policy lists (kano_shadow_lists), as source, as
    # destination and for the pairs
    lst = DeviceBuild(None)
    loff, lflat = np.array([0, 1, 2], np.int64), np.array([0, 1], np.int32)
    law, lcnt = np.full((2, 1), 3, np.uint64), ctypes.c_int64()
    assert lib.kano_shadow_lists(lst.ctx, 2, 64, 2, ptr(loff), ptr(lflat), ptr(law),
                                 ctypes.byref(lcnt)) == 0
    assert vmx(lst.ctx, dst.ctx, 2, prio, act) == EINVAL
    assert b"policy lists" in lib.kano_last_error(dst.ctx)
    assert vmx(eng.ctx, lst.ctx, P, prio, act) == EINVAL
    assert b"policy lists" in lib.kano_last_error(lst.ctx)
    assert pvs(lst.ctx, 1, one, 2, prio, act, out) == EINVAL
    assert b"policy lists" in lib.kano_last_error(lst.ctx)
    assert not dst.rows(0, n).any()
    lst.close()
    assert pvs(eng.ctx, 0, None, P, prio, act, None) == 0              # Q = 0 is valid
    assert cnt.tolist() == [0, 0, 0]
    # usable afterwards, the optional outputs left out
    assert pvs(eng.ctx, 1, one, P, prio, act, out, full=False) == 0
    assert pvs(eng.ctx, 1, one, P, prio, act, out) == 0 and int(cnt.sum()) == 1
    n_, sel, allow = tp.golden_dense("q_shadow")
    wv, wp, wi = want_pairs(sel, allow, act.astype(bool), prio.astype(np.int64), one)
    assert (out[0], dp[0], di[0]) == (wv[0], wp[0], wi[0])
    assert vmx(eng.ctx, dst.ctx, P, prio, act) == 0
    assert info.tolist()[:3] == [int((act == 0).sum()), int(act.sum()), P]
    v, _ = want_verdict(sel, allow, act.astype(bool), prio.astype(np.int64))
    assert np.array_equal(dst.rows(0, n), to_words(v))
    # the destination reads as an edited matrix: column checks over its rows,
    # single bits read and written, no policies of its own
    from kano._bits import words_to_bool
    col_and, col_or = dst.col_checks()
    assert np.array_equal(words_to_bool(col_or, n), v.any(axis=0))
    assert np.array_equal(words_to_bool(col_and, n), v.all(axis=0))
    i0, j0 = map(int, np.argwhere(v)[0])
    assert dst.get_bit(i0, j0) == 1
    dst.set_bit(i0, j0, 0)
    assert dst.get_bit(i0, j0) == 0
    assert pvs(dst.ctx, 1, one, 0, prio, act, out) == EINVAL
    assert b"no policies" in lib.kano_last_error(dst.ctx)
    assert lib.kano_verdict_matrix(eng.ctx, dst.ctx, P, ptr(prio), ptr(act), None) == 0
    assert np.array_equal(dst.rows(0, n), to_words(v))
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
    n, sel, allow = tp.golden_dense(name)
    eng = DeviceBuild(tr.cluster_tables(name))
    deny, prio = tier_rule(eng.info()["P"], 3)
    want_rows = to_words(golden_verdict(name, 3)[0])
    want = want_pairs(sel, allow, deny, prio, pairs)
    dst = DeviceBuild.empty(n)

    def state():
        r = eng.pair_policies(pairs, hist=True)
        return (eng.shadow(), eng.conflict(), eng.policy_impact(), r["cover"], r["offsets"],
                r["policies"], eng.rows_digest(0, n))

    def verdicts():
        eng.verdict_into(dst, prio, deny)
        assert np.array_equal(dst.rows(0, n), want_rows)
        r = eng.pair_verdicts(pairs, prio, deny)
        assert all(np.array_equal(r[k], w) for k, w in zip(("verdict", "priority", "policy"), want))

    first = state()
    assert sha(first[0]) == exp["sha256"] and np.array_equal(first[1], conflicts)
    assert np.array_equal(first[2], impact) and te.same(first[3:6], (cover, off, ids))
    verdicts()
    assert all(np.array_equal(a, b) for a, b in zip(first, state()))
    # the stored results survive the new calls: fetched after them
    k = eng.shadow_count()
    eng.conflict()
    eng.pair_policies(pairs)
    verdicts()
    assert sha(eng.shadow_fetch(k)) == exp["sha256"]
    assert np.array_equal(eng.conflict_fetch(conflicts.shape[0]), conflicts)
    pol = np.zeros(ids.shape[0], np.int32)
    eng._chk(eng.lib.kano_pair_policies_fetch(eng.ctx, pol.ctypes.data), "fetch")
    assert np.array_equal(pol, ids)
    eng.close()
    dst.close()


@gpu
def test_between_pipelined_verify_steps(need_gpu):
    """The verdict queries between two steps of a pipelined verify loop (a
    prologue is queued behind its gate then) leave the next step's lists and
    pairs at their golden values."""
    from kano._engine import DeviceBuild
    from kano._intern import intern, group_ids
    name = "s_sparse_2000"
    obj = cluster(name)
    cs, ps = tr.api_objects(obj)
    exp = expected(name)
    pairs = te.record_arrays(name)[0]
    n, sel, allow = tp.golden_dense(name)
    deny, prio = tier_rule(len(ps), 3)
    want_rows = to_words(golden_verdict(name, 3)[0])
    want = want_pairs(sel, allow, deny, prio, pairs)
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
            eng.verdict_into(dst, prio, deny)
            assert np.array_equal(dst.rows(0, n), want_rows)
        if k in (2, 3):
            r = eng.pair_verdicts(pairs, prio, deny)
            assert all(np.array_equal(r[key], w)
                       for key, w in zip(("verdict", "priority", "policy"), want))
    assert sha(eng.rows(0, len(cs))) == exp["M_sha256"]
    eng.close()
    dst.close()
