"""The pair walk's edges (csrc/kano_pairwalk.hpp) on one small cluster, for the
three families that fold it: pair_policies (test_explain), pair_ports
(test_ports) and pair_verdicts / verdict_matrix (test_verdicts).  Each family
is checked against its own file's numpy restatement, and every restatement
first, on the CPU, against an answer written down from the construction.

150 pods: pods 10 g .. 10 g + 9 carry group "abcde"[g], the rest "z"; every
pod the id (index % 13).  Build policy q of a group selects the group and
allows the pods with id == q % 13, so the row classes' lists hold 63, 64, 65,
1 and 300 policies (300: past the wave form's register sums) and "z" none.
Added policy t selects group "abcdez"[t % 6] (rows with an empty list too)
and allows id t % 13.  A = 0, 1, 65 added policies (none, one, more than a
round of 64), one of them and / or a build policy removed.  The ports rule
gives 131 slots: three mask words, the odd tail of the kernels' two-word
chunks.  Exact integers and bits throughout.
"""
import types

import numpy as np
import pytest

from _golden import lists_to_csr
import test_explain as te
import test_ports as tp
import test_redundancy as tr
import test_verdicts as tv

N = 150
LISTS = (("a", 63), ("b", 64), ("c", 65), ("d", 1), ("e", 300))
P0 = sum(k for _, k in LISTS)
ADDED = (0, 1, 65)
PAIRS = np.array([(i, j) for i in (0, 10, 20, 30, 40, 49, 50, 149) for j in range(N)], np.int32)
K = 130      # the port rule's K: 130 keys and ANY_OTHER


def group(i):
    return "abcdez"[min(i // 10, 5)]


def spec(A):
    """(group selected, id allowed) of the build policies and the A added ones."""
    return [(g, q % 13) for g, k in LISTS for q in range(k)] + \
        [("abcdez"[t % 6], t % 13) for t in range(A)]


def rules_of(A):
    """((group selected, id allowed, index at creation) of the policies left,
    the removals as current indices in order)."""
    rules = [(g, d, p) for p, (g, d) in enumerate(spec(A))]
    gone = {0: [5], 1: [P0], 65: [5, P0 - 1 + 7]}[A]     # build / added / both
    for k in gone:
        del rules[k]
    return rules, gone


def dense(rules):
    """(sel, allow) bool (P, n), from the construction."""
    grp = np.array([group(i) for i in range(N)])
    ids = np.arange(N) % 13
    return (np.array([grp == g for g, _, _ in rules]), np.array([ids == d for _, d, _ in rules]))


def matches(rules):
    """{(group of i, id of j): current indices of the matching policies, ascending}."""
    out = {}
    for p, (g, d, _) in enumerate(rules):
        out.setdefault((g, d), []).append(p)
    return out


def of_pair(rules):
    """The matching policies of every pair of PAIRS, from the construction."""
    match = matches(rules)
    return [match.get((group(i), j % 13), []) for i, j in PAIRS.tolist()]


def matrix(A, dress=lambda ps: None):
    """(matrix, its current policy list, rules): built from the build policies,
    the A others added, the removals applied; dress(all policies, by index at
    creation) gives them a family's attributes first."""
    from kano.model import (Container, Policy, PolicyAllow, PolicyEgress, PolicySelect,
                            ReachabilityMatrix)
    rules, gone = rules_of(A)
    cs = [Container(f"c{i}", {"g": group(i), "id": str(i % 13)}) for i in range(N)]
    ps = [Policy(f"p{p}", PolicySelect({"g": g}), PolicyAllow({"id": str(d)}), PolicyEgress, None)
          for p, (g, d) in enumerate(spec(A))]
    dress(ps)
    m = ReachabilityMatrix.build_matrix(cs, ps[:P0])
    if A:
        m.add_policies(ps[P0:])
    for k in gone:
        m.remove_policies([k])
    assert [pol.name for pol in m._policies] == [f"p{p}" for _, _, p in rules]
    sel, allow = tp.dense_sets(*tr.policy_sets(m._policies, N), N)
    assert all(np.array_equal(a, b) for a, b in zip((sel, allow), dense(rules)))
    return m, m._policies, rules, sel, allow


# ---- pair_policies ----------------------------------------------------------
def want_policies(rules):
    """(cover, offsets, ids) on PAIRS, from the construction."""
    ids = of_pair(rules)
    cover = np.array([len(x) for x in ids], np.int32)
    return cover, np.concatenate([[0], np.cumsum(cover)]).astype(np.int64), \
        np.array([p for x in ids for p in x], np.int32)


# ---- pair_ports -------------------------------------------------------------
def dress_ports(ps):
    for p, pol in enumerate(ps):
        pol.protocol = tp.protocol_for(p, K)


def table_of(rules):
    from kano.ports import port_table
    return port_table([types.SimpleNamespace(name=f"p{p}", protocol=tp.protocol_for(p, K))
                       for _, _, p in rules])


def want_masks(rules, t):
    out = np.zeros((PAIRS.shape[0], t.masks.shape[1]), np.uint64)
    for q, ps in enumerate(of_pair(rules)):
        for p in ps:
            out[q] |= t.masks[p]
    return out


# ---- pair_verdicts ----------------------------------------------------------
def tiers_of(A, rules):
    """(deny, prio) of the policies left: test_verdicts' rule at L = 3 by index
    at creation."""
    deny, prio = tv.tier_rule(P0 + A, 3)
    idx = [p for _, _, p in rules]
    return deny[idx], prio[idx]


def dress_tiers(ps):
    tv.carry(ps, *tv.tier_rule(len(ps), 3))


def want_verdicts(rules, deny, prio):
    out = []
    for ps in of_pair(rules):
        if not ps:
            out.append((0, 0, -1))
            continue
        best = min(int(prio[p]) for p in ps)
        top = [p for p in ps if prio[p] == best]
        dn = any(deny[p] for p in top)
        out.append((2 if dn else 1, best, min(p for p in top if deny[p] == dn)))
    v, t, p = zip(*out)
    return np.array(v, np.uint8), np.array(t, np.int32), np.array(p, np.int32)


def equal(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


# --------------------------------------------------------------------------
# CPU: the restatements alone give the construction's answers
# --------------------------------------------------------------------------
@pytest.mark.parametrize("A", ADDED)
def test_restatements_on_the_edge_cluster(A):
    rules, _ = rules_of(A)
    sel, allow = dense(rules)
    nb = P0 - (A != 1)                                    # build policies left
    assert sorted(set(sel[:nb].sum(axis=0).tolist())) == [0, 1, 63 - (A != 1), 64, 65, 300]
    assert len(rules) - nb == {0: 0, 1: 0, 65: 64}[A]
    # pair_policies
    off, flat = lists_to_csr([np.flatnonzero(sel[:, i]).tolist() for i in range(N)])
    aw = np.stack([tr._bits_row(np.flatnonzero(a), N) for a in allow])
    want = want_policies(rules)
    assert te.same(te.want_pairs(off, flat, aw, N, PAIRS), want)
    assert want[0].max() > 23 and (want[0] == 0).any()
    # pair_ports
    t = table_of(rules)
    assert t.KW == 3 and t.masks.shape == (len(rules), 3)
    masks = tp.want_masks(sel, allow, t.masks, PAIRS)
    assert np.array_equal(masks, want_masks(rules, t))
    assert all(masks[:, w].any() for w in range(3))
    # pair_verdicts
    deny, prio = tiers_of(A, rules)
    verdicts = want_verdicts(rules, deny, prio)
    assert equal(tv.want_pairs(sel, allow, deny, prio, PAIRS), verdicts)
    assert set(verdicts[0].tolist()) == {0, 1, 2}


# --------------------------------------------------------------------------
# GPU: both forms of every family
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def need_gpu():
    from kano import _native
    if not _native.gpu_available():
        pytest.fail("GPU test run without a usable HIP device / libkano_hip.so")


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("form", ["ppf=1", "ppf=2"])
@pytest.mark.parametrize("A", ADDED)
def test_pair_policies(A, form, monkeypatch, need_gpu):
    monkeypatch.setenv("KANO_TUNE", form)
    m, ps, rules, _, _ = matrix(A)
    assert te.same(te._check_against_sets(m, ps, N, PAIRS), want_policies(rules))
    m._engine.close()


@gpu
@pytest.mark.parametrize("form", ["pmf=1", "pmf=2"])
@pytest.mark.parametrize("A", ADDED)
def test_pair_ports(A, form, monkeypatch, need_gpu):
    from kano.ports import port_table
    monkeypatch.setenv("KANO_TUNE", form)
    m, ps, rules, sel, allow = matrix(A, dress_ports)
    t, want = port_table(ps), table_of(rules)
    assert t.keys == want.keys and np.array_equal(t.masks, want.masks)
    masks, _ = tp.check_ports(m, sel, allow, t, PAIRS, slots=(0, 64, t.K), exposure=False)
    assert np.array_equal(masks, want_masks(rules, t))
    m._engine.close()


@gpu
@pytest.mark.parametrize("form", ["pvf=1", "pvf=2"])
@pytest.mark.parametrize("A", ADDED)
def test_pair_verdicts(A, form, monkeypatch, need_gpu):
    """(With added policies their rows of the verdict matrix are resolved bit
    by bit, k_verdict_rows.)"""
    monkeypatch.setenv("KANO_TUNE", form)
    m, ps, rules, sel, allow = matrix(A, dress_tiers)
    deny, prio = tiers_of(A, rules)
    _, _, got = tv.check_verdicts(m, sel, allow, deny, prio, PAIRS)
    assert equal(got, want_verdicts(rules, deny, prio))
    m._engine.close()
