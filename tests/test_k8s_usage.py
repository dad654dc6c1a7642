"""K8sConnectivity.rule_usage: which rules of a policy set do anything at all
-- per rule the pod pairs it decides and passes down, per NetworkPolicy rule
the pairs only that rule allows -- counted over every ordered pod pair
(kano_k8s_rule_usage).

The oracle below histograms test_k8s_pairs' naming oracle (manifest dicts
only, no kano code) per (kind, policy, rule) and reads ``sole`` off the
NetworkPolicy rules' pod masks.  On the CPU it is pinned by a table for the
six-pod cluster and by removal: taking a dead or redundant rule out of the
manifests leaves every verdict as it was, taking a rule with sole > 0 out
denies exactly ``sole`` pairs."""
import copy
import errno
import functools

import numpy as np
import pytest

from test_k8s_conn import QUERIES, _case, _counts
from test_k8s_pairs import (KNOWN_VERDICTS, PORTS, TIERS, Cluster, _all_pairs, _connect,
                            _known_cluster, _long_list_cluster, _tiered)
from test_k8s_tiers import SEED_130, SEED_1030, SEED_ABI, SEEDS_60, _anp_counts, _tier_case

DIRS = ("egress", "ingress")
# n = 300, every pod its own class on both sides (5 words a row, 8 lanes a
# class, 32 classes a block): the first seed from 1 on whose cluster meets
# _tier_case's conditions (found by running it on the CPU)
SEED_300 = 1


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
class Usage:
    """The oracle's rule usage of one (cluster, port, allow_self).  Per
    direction: ``rules`` [(kind, policy, rule, action, on_port)] in evaluation
    order, ``dec`` / ``pas`` {(kind, policy, rule): pairs} (every rule has a
    key), ``sole`` {(policy, rule): pairs} for the NetworkPolicy rules,
    ``dec_peer`` / ``pas_peer`` {naming-oracle name: pairs}, ``tiers`` the
    eight (tier, verdict) counts and ``empty`` the rules no pod pair meets."""

    def __init__(self, cl, port, allow_self):
        n, o = cl.n, cl.named(port)
        dom = ~np.eye(n, dtype=bool) if allow_self else np.ones((n, n), bool)
        self.pairs = int(dom.sum())
        for key in DIRS:
            adm, net, base, iso = cl._structure[key]
            tier, deny, dec, pas = getattr(o, key)
            rules, empty = [], set()
            for tr in (adm, net, base):
                for kind, name, ri, action, ports, subj, peers in tr:
                    on = (_counts if kind == "network" else _anp_counts)(ports, port)
                    rules.append((kind, name, ri, action, bool(on)))
                    if not any(subj.any() and pm.any() for pj, pm in peers):
                        empty.add((kind, name, ri))
            nd = np.bincount(dec[dom & (dec >= 0)], minlength=len(o.names))
            npas = np.bincount(pas[dom & (pas >= 0)], minlength=len(o.names))
            d = {r[:3]: 0 for r in rules}
            p = dict(d)
            for k, name in enumerate(o.names):
                if name[:3] in d:       # (the names of both directions share one table)
                    d[name[:3]] += int(nd[k])
                    p[name[:3]] += int(npas[k])
            assert sum(d.values()) == int((dom & (dec >= 0)).sum())
            assert sum(p.values()) == int((dom & (pas >= 0)).sum())
            masks = {}
            for kind, name, ri, action, ports, sel, peers in net:
                if _counts(ports, port):
                    m = np.zeros(n, bool)
                    for pj, pm in peers:
                        m |= pm
                    masks[(name, ri)] = sel[:, None] & m[None, :]
            hits = sum(m.astype(np.int32) for m in masks.values()) if masks else np.zeros((n, n))
            sole = {(name, ri): 0 for kind, name, ri, *_ in net}
            for k, m in masks.items():
                sole[k] = int((m & (hits == 1) & (tier == 2) & dom).sum())
            tiers = [int(((tier == t) & (deny == v) & dom).sum())
                     for t in range(4) for v in (False, True)]
            setattr(self, key, dict(
                rules=rules, dec=d, pas=p, sole=sole, tiers=tiers, empty=empty,
                dec_peer={o.names[k]: int(c) for k, c in enumerate(nd) if c},
                pas_peer={o.names[k]: int(c) for k, c in enumerate(npas) if c}))

    def dead(self, key):
        u = getattr(self, key)
        return [r[:3] for r in u["rules"] if r[4] and not u["dec"][r[:3]] and not u["pas"][r[:3]]]


@functools.lru_cache(maxsize=None)
def _usage(cl, port, allow_self):
    return Usage(cl, port, allow_self)


def _without(cl, key, kind, name, ri):
    """The cluster without rule ``ri`` of the named policy in direction
    ``key``; a NetworkPolicy keeps its policyTypes."""
    from kano import k8s
    pods, pols, nss, admin, baseline = cl.objects

    def cut(spec):
        spec = copy.deepcopy(spec)
        del spec[key][ri]
        return spec

    if kind == "admin":
        admin = [k8s.AdminNetworkPolicy(a.name, cut(a.spec)) if a.name == name else a
                 for a in admin]
    elif kind == "baseline":
        baseline = k8s.BaselineAdminNetworkPolicy(baseline.name, cut(baseline.spec))
    else:
        out = []
        for p in pols:
            if p.name == name:
                spec = copy.deepcopy(p.spec)
                spec["policyTypes"] = k8s.policy_types(spec)
                del spec[key][ri]
                p = k8s.NetworkPolicy(p.name, p.namespace, spec)
            out.append(p)
        pols = out
    return Cluster(pods, pols, nss, admin, baseline)


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------
def _nonzero(d):
    return {k: v for k, v in d.items() if v}


def test_known_cluster_oracle():
    cl = _known_cluster()
    u = Usage(cl, None, False)
    assert _nonzero(u.egress["dec"]) == {
        ("admin", "X", 1): 9, ("admin", "Y", 0): 3, ("network", "B", 0): 1,
        ("network", "D", 0): 3, ("baseline", "base", 0): 6, ("baseline", "base", 1): 9}
    assert _nonzero(u.ingress["dec"]) == {
        ("admin", "X", 0): 3, ("admin", "Y", 0): 2, ("network", "A", 0): 1}
    assert _nonzero(u.egress["pas"]) == {("admin", "X", 0): 3} and not _nonzero(u.ingress["pas"])
    assert u.egress["sole"] == {("B", 0): 1, ("D", 0): 3}
    assert u.ingress["sole"] == {("A", 0): 1, ("A", 1): 0}
    assert sum(u.egress["tiers"]) == sum(u.ingress["tiers"]) == 36
    # without the six self pairs: p5 -> p5 (Y0), p0 -> p0 (D), p3 -> p3 and p4 -> p4 (b1) go
    s = Usage(cl, None, True)
    want = dict(u.egress["dec"])
    want.update({("admin", "Y", 0): 2, ("network", "D", 0): 2, ("baseline", "base", 1): 7})
    assert s.egress["dec"] == want and s.egress["sole"] == {("B", 0): 1, ("D", 0): 2}
    assert s.egress["pas"] == {**u.egress["pas"], ("admin", "X", 0): 2}   # (p2 -> p2 was passed)
    assert _nonzero(s.ingress["dec"]) == _nonzero(u.ingress["dec"])
    assert s.ingress["sole"] == u.ingress["sole"]
    assert sum(s.egress["tiers"]) == sum(s.ingress["tiers"]) == 30


@pytest.mark.parametrize("seed", SEEDS_60)
def test_removal_on_the_oracle(seed):
    """What dead, sole == 0 and sole > 0 claim, checked by taking the rule out
    of the manifests and resolving the cluster again."""
    cl = _tiered(seed)
    ports = (None, ("TCP", 80))
    use = {port: Usage(cl, port, False) for port in ports}
    for key in DIRS:
        other = DIRS[1 - DIRS.index(key)]
        rules = use[None].__dict__[key]["rules"]
        for kind, name, ri, action, _ in rules:
            dead = {port: (kind, name, ri) in use[port].dead(key) for port in ports}
            sole = {port: use[port].__dict__[key]["sole"].get((name, ri)) if kind == "network"
                    else None for port in ports}
            if not any(dead.values()) and kind != "network":
                continue
            cut = _without(cl, key, kind, name, ri)
            for port in ports:
                was, now = cl.named(port), cut.named(port)
                same = all(np.array_equal(getattr(was, d)[k], getattr(now, d)[k])
                           for d in DIRS for k in (0, 1))
                if dead[port] or sole[port] == 0:
                    assert same, (seed, key, kind, name, ri, port)
                elif sole[port]:
                    (t0, d0), (t1, d1) = getattr(was, key)[:2], getattr(now, key)[:2]
                    assert int((d1 & ~d0).sum()) == sole[port] and not (d0 & ~d1).any()
                    assert np.array_equal(t0, t1)
                    assert all(np.array_equal(getattr(was, other)[k], getattr(now, other)[k])
                               for k in (0, 1))


def test_seeds_carry_dead_sole_and_redundant_rules():
    shared = 0
    for seed in SEEDS_60:
        u = Usage(_tiered(seed), None, False)
        found = False
        for key in DIRS:
            d = getattr(u, key)
            assert len(u.dead(key)) >= 1, (seed, key)
            assert any(v > 0 for v in d["sole"].values()), (seed, key)
            found |= any(d["dec"][("network",) + k] > 0 and v == 0 for k, v in d["sole"].items())
            for (name, ri), v in d["sole"].items():
                assert v <= d["dec"][("network", name, ri)]
        shared += found
    assert shared >= 8


def test_group_builder():
    from kano import k8s
    for cl in (_known_cluster(), _tiered(SEEDS_60[0]), _long_list_cluster()):
        c = k8s.compile_conformant(*cl.objects)
        for (group, rules), origin, tiers in zip(
                k8s.rule_groups(c), (c.origin_egress, c.origin_ingress),
                (c.tiers_egress, c.tiers_ingress)):
            assert group.dtype == np.int32 and len(group) == len(origin)
            assert (np.diff(group) >= 0).all() and (np.diff(group) <= 1).all()
            assert len(group) == 0 or (group[0] == 0 and group[-1] == len(rules) - 1)
            keys = [(t[0], o[0], o[2]) for o, t in zip(origin, tiers)]
            assert len(set(keys)) == len(rules)               # one group per (kind, policy, rule)
            for g, (kind, pi, ri, action, first, cnt) in enumerate(rules):
                assert (group[first:first + cnt] == g).all() and (group == g).sum() == cnt
                assert set(keys[first:first + cnt]) == {(kind, pi, ri)}
    # entries of one rule that are not contiguous are refused
    c = k8s.compile_conformant(*_known_cluster().objects)
    c.origin_egress = c.origin_egress + [c.origin_egress[0]]
    c.tiers_egress = c.tiers_egress + [c.tiers_egress[0]]
    with pytest.raises(AssertionError):
        k8s.rule_groups(c)


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------
def _entry_name(conn, cl, key, p):
    """(kind, policy name, rule, peer, action) of entry p: the naming oracle's name."""
    pods, pols, nss, admin, baseline = cl.objects
    by_kind = {"admin": admin, "network": pols, "baseline": [baseline]}
    c = conn._compiled
    org = getattr(c, "origin_" + key)[p]
    kind, level, action = getattr(c, "tiers_" + key)[p]
    return kind, by_kind[kind][org[0]].name, org[2], org[3], action


def _check_usage(cl, conn, u):
    """Everything rule_usage returns against the oracle of conn's port."""
    want = _usage(cl, conn.port, conn.allow_self)
    n = cl.n
    dead, redundant = [], []
    for key in DIRS:
        w, got = getattr(want, key), getattr(u, key)
        P = len(getattr(conn, "origin_" + key))
        assert got.decided.dtype == np.int64 and got.decided.shape == (P,)
        assert got.passed.dtype == np.int64 and got.passed.shape == (P,)
        names = [_entry_name(conn, cl, key, p) for p in range(P)]
        assert len(set(names)) == P
        assert [w["dec_peer"].get(nm, 0) for nm in names] == got.decided.tolist(), key
        assert [w["pas_peer"].get(nm, 0) for nm in names] == got.passed.tolist(), key
        assert sum(w["dec_peer"].values()) == int(got.decided.sum())
        assert sum(w["pas_peer"].values()) == int(got.passed.sum())
        recs = u.rules(key)
        listed = {r[:3] for r in recs}
        assert len(listed) == len(recs) and got.sole.dtype == np.int64
        rules = [r for r in w["rules"] if r[:3] in listed]
        assert len(rules) == len(recs)
        for kind, name, ri, action, on in w["rules"]:
            k = (kind, name, ri)
            if k not in listed:          # no compiled entry: nothing can meet the rule
                assert k in w["empty"] and not w["dec"][k] and not w["pas"][k], k
        for r, (kind, name, ri, action, on) in zip(recs, rules):   # the same order
            sole = w["sole"][(name, ri)] if kind == "network" else None
            assert tuple(r) == (kind, name, ri, action, on, w["dec"][(kind, name, ri)],
                                w["pas"][(kind, name, ri)], sole), (key, r)
            if sole is not None:
                assert sole <= r.decided
                if sole == 0:
                    redundant.append((key, kind, name, ri))
            if on and not r.decided and not r.passed:
                dead.append((key, kind, name, ri))
        for deny_only in (True, False):
            assert u.blame(key, deny_only) == {
                r[:3]: w["dec"][r[:3]] for r in rules
                if w["dec"][r[:3]] and (r[3] == "Deny" or not deny_only)}
        for t, tn in enumerate(TIERS):
            for v, vn in enumerate(("allow", "deny")):
                assert u.counts[f"{key}_{tn}_{vn}"] == w["tiers"][2 * t + v], (key, tn, vn)
        assert sum(v for k, v in u.counts.items() if k.startswith(key)) == want.pairs
    assert want.pairs == n * n - (n if conn.allow_self else 0)
    assert len(u.counts) == 16
    assert u.dead_rules() == dead and u.redundant_rules() == redundant
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("allow_self", [True, False])
def test_known_cluster(allow_self):
    cl = _known_cluster()
    base = _connect(cl, allow_self=allow_self)
    for port in KNOWN_VERDICTS:
        conn = base.on_port(port)
        _check_usage(cl, conn, conn.rule_usage())
    u = base.rule_usage()
    if not allow_self:
        assert u.blame("egress") == {("admin", "X", 1): 9, ("baseline", "base", 1): 9}
        assert u.blame("egress", deny_only=False) == {
            ("admin", "X", 1): 9, ("admin", "Y", 0): 3, ("network", "D", 0): 3,
            ("network", "B", 0): 1, ("baseline", "base", 0): 6, ("baseline", "base", 1): 9}
        assert u.blame("ingress") == {("admin", "Y", 0): 2}
        assert [r.sole for r in u.rules("ingress") if r.kind == "network"] == [1, 0]
        assert u.redundant_rules() == [("ingress", "network", "A", 1)]
    else:
        assert u.blame("egress") == {("admin", "X", 1): 9, ("baseline", "base", 1): 7}
    with pytest.raises(ValueError):
        u.blame("sideways")
    with pytest.raises(ValueError):
        u.rules("both")


@pytest.mark.gpu
@pytest.mark.parametrize("allow_self", [True, False])
@pytest.mark.parametrize("seed", SEEDS_60)
def test_matches_oracle(seed, allow_self):
    cl = _tiered(seed)
    base = _connect(cl, allow_self=allow_self)
    pr = _all_pairs(cl.n)
    for port in PORTS:
        conn = base.on_port(port)
        u = conn.rule_usage()
        _check_usage(cl, conn, u)
        if not allow_self:
            r = conn.pair_verdicts(pr)
            for key in DIRS:
                assert u.blame(key, False) == r.blame(key, False), (port, key)
                assert u.blame(key) == r.blame(key), (port, key)
            assert {k: v for k, v in r.counts.items() if k in u.counts} == u.counts


@pytest.mark.gpu
def test_more_than_one_word():
    """n = 130, every pod its own row and column class on both sides: three AC
    words a row, four lanes a class."""
    n = 130
    cl = _tiered(SEED_130, n=n, P=20, nns=4, uid=True)
    conn = _connect(cl, allow_self=False)
    for b in (conn.egress, conn.ingress):
        info = b.engine.info()
        assert info["U"] == n and info["UA"] == n
    for port in (None, QUERIES[0]):
        c = conn.on_port(port)
        _check_usage(cl, c, c.rule_usage())


@pytest.mark.gpu
@pytest.mark.parametrize("tune", ["kugrid=1", "kugrid=2"])
def test_more_classes_than_a_block_holds(tune, monkeypatch):
    """n = 300 own classes: 5 words and 8 lanes a class, 32 classes a block
    turn -- 10 grid-stride turns under a cap of one block, 5 under two."""
    monkeypatch.setenv("KANO_TUNE", tune)
    n = 300
    cl = _tiered(SEED_300, n=n, P=24, nns=4, uid=True)
    conn = _connect(cl)
    for b in (conn.egress, conn.ingress):
        info = b.engine.info()
        assert info["U"] == n and info["UA"] == n
    _check_usage(cl, conn, conn.rule_usage())


@pytest.mark.gpu
def test_1030_pods():
    cl = _tiered(SEED_1030, n=1030, P=30, nns=4)
    conn = _connect(cl)
    _check_usage(cl, conn, conn.rule_usage())


@pytest.mark.gpu
def test_long_subject_list():
    cl = _long_list_cluster()
    n = cl.n
    conn = _connect(cl, allow_self=False)
    assert conn._compiled.np_level[0] == 150
    u = conn.rule_usage()
    _check_usage(cl, conn, u)
    by = {(r.policy, r.rule): r for r in u.rules("egress")}
    assert len(by) == 152
    # rule 0 allows pod 1 for every pod, rule 64 denies pod 2, rule 149 passes pod 3
    r0, r64, r149 = by[("long0", 0)], by[("long1", 14)], by[("long2", 49)]
    assert (r0.action, r0.decided, r0.passed) == ("Allow", n, 0)
    assert (r64.action, r64.decided, r64.passed) == ("Deny", n, 0)
    assert (r149.action, r149.decided, r149.passed) == ("Pass", 0, n)
    # pods 10..59 are named by three rules each: the first takes them all
    assert by[("long0", 1)].decided + by[("long0", 1)].passed == n
    assert ("egress", "admin", "long1", 1) in u.dead_rules()
    # the baseline's deny of pod 4 holds for the pods no NetworkPolicy isolates
    iso = sum(1 for i in range(n) if i % 3 == 0)
    assert by[("base", 0)].decided == n - iso
    assert u.counts["egress_network_deny"] > 0 and u.counts["egress_network_allow"] > 0


@pytest.mark.gpu
def test_degenerate_inputs():
    from kano import k8s
    nss = [k8s.Namespace("a", {"team": "x"})]
    everyone = {"namespaces": {}}
    app = lambda v: {"pods": {"podSelector": {"matchLabels": {"app": v}}}}   # noqa: E731
    pods = [k8s.Pod(f"p{i}", "a", {"app": "w" if i % 3 else "d"}) for i in range(70)]
    n = 70

    def check(pols, admin, baseline, **kw):
        cl = Cluster(pods, pols, nss, admin, baseline)
        conn = _connect(cl, **kw)
        u = conn.rule_usage()
        _check_usage(cl, conn, u)
        return cl, conn, u

    # no pods
    conn = _connect(Cluster([], [], nss, [], None))
    u = conn.rule_usage()
    assert set(u.counts.values()) == {0} and u.dead_rules() == [] and u.rules("egress") == []
    # an egress admin rule only: no Ingress-typed policy, the ingress side has no classes
    a_deny = k8s.AdminNetworkPolicy("x", {"priority": 3, "subject": app("d"), "egress": [
        {"action": "Deny", "to": [app("w")], "ports": [{"portNumber": {"port": 80}}]}]})
    for allow_self in (True, False):
        cl, conn, u = check([], [a_deny], None, allow_self=allow_self)
        assert conn.ingress.engine.info()["P"] == 0
        assert u.counts["ingress_default_allow"] == n * n - (n if allow_self else 0)
        assert u.ingress.decided.shape == (0,) and u.ingress.sole.shape == (0,)
        assert u.counts["egress_admin_deny"] == 24 * 46 and u.dead_rules() == []
        # ... on a port that drops the one admin rule: everything is default
        c81 = conn.on_port(("TCP", 81))
        u = c81.rule_usage()
        _check_usage(cl, c81, u)
        assert u.counts["egress_default_allow"] == n * n - (n if allow_self else 0)
        assert [r.on_port for r in u.rules("egress")] == [False] and u.dead_rules() == []
    # no policy of any kind
    cl, conn, u = check([], [], None)
    assert u.counts["egress_default_allow"] == u.counts["ingress_default_allow"] == n * n - n
    # an untiered connectivity (np_level 0): network or default
    case = _case(5)
    cl = Cluster(*case[:3])
    for allow_self in (True, False):
        base = k8s.connectivity(*case[:3], allow_self=allow_self)
        assert base._compiled.np_level == (0, 0) and not base._compiled.tiered
        for port in PORTS:
            conn = base.on_port(port)
            u = conn.rule_usage()
            _check_usage(cl, conn, u)
            assert all(v == 0 for k, v in u.counts.items() if "admin" in k or "baseline" in k)
            assert not u.egress.passed.any() and not u.ingress.passed.any()
    # a rows= object reads the same two builds
    cl = _tiered(SEEDS_60[1])
    full, part = _connect(cl).rule_usage(), _connect(cl, rows=(10, 20))
    u = part.rule_usage()
    _check_usage(cl, part, u)
    assert u.counts == full.counts and u.rules("egress") == full.rules("egress")
    assert np.array_equal(u.ingress.decided, full.ingress.decided)
    assert np.array_equal(u.egress.sole, full.egress.sole)


@pytest.mark.gpu
def test_removed_rules_change_nothing_end_to_end():
    """Three dead and three redundant rules of one seed, each taken out of the
    manifests: the rebuilt matrix is the same."""
    from kano.algorithm import matrix_diff
    cl = _tiered(SEEDS_60[2])
    conn = _connect(cl)
    u = conn.rule_usage()
    dead, red = u.dead_rules(), [r for r in u.redundant_rules() if r not in u.dead_rules()]
    assert len(dead) >= 3 and len(red) >= 3
    for key, kind, name, ri in dead[:3] + red[:3]:
        after = _connect(_without(cl, key, kind, name, ri))
        d = matrix_diff(conn.allowed, after.allowed)
        assert (d.added, d.removed) == (0, 0), (key, kind, name, ri)
    # the rules dead on every port of a list
    every = conn.dead_rules([None] + QUERIES)
    per_port = [set(conn.on_port(p).rule_usage().dead_rules()) for p in [None] + QUERIES]
    assert every == [r for r in dead if all(r in s for s in per_port)]
    assert conn.dead_rules([None]) == dead and conn.dead_rules([]) == []


def _wide_case(n, bits):
    """bits + 4 generic policies over n pods, every pod a column class of its
    own (the first ``bits`` allow sets are the bits of the pod index) and a few row
    classes (the select sets are i % 7 and i % 2 values): entry lists as the
    codes see them, with the masks to resolve them in numpy."""
    from kano.model import Container, Policy, PolicyAllow, PolicyEgress, PolicySelect
    assert n < 1 << bits
    idx = np.arange(n)
    cs = [Container(f"c{i}", dict({f"b{b}": str(i >> b & 1) for b in range(bits)},
                                  r=str(i % 7), h=str(i % 2))) for i in range(n)]
    pols, sel, alw = [], [], []

    def add(select, allow, smask, amask):
        pols.append(Policy(f"w{len(pols)}", PolicySelect(select), PolicyAllow(allow),
                           PolicyEgress, None))
        sel.append(smask)
        alw.append(amask)

    for b in range(bits):
        r = b % 7
        add({"r": str(r)} if b % 3 else {"h": "1"}, {f"b{b}": "1"},
            idx % 7 == r if b % 3 else idx % 2 == 1, (idx >> b & 1) == 1)
    # the four the test puts at np_level: two halves for r = 1; for r = 2 a
    # half and a set that overlaps it
    add({"r": "1"}, {"h": "0"}, idx % 7 == 1, idx % 2 == 0)
    add({"r": "1"}, {"h": "1"}, idx % 7 == 1, idx % 2 == 1)
    add({"r": "2"}, {"h": "0"}, idx % 7 == 2, idx % 2 == 0)
    add({"r": "2"}, {"b1": "1"}, idx % 7 == 2, (idx >> 1 & 1) == 1)
    return cs, pols, np.array(sel), np.array(alw)


def _resolve(code, group, np_level, selects, hits, weight):
    """decided, passed, sole and tiers by first match in (code, id) order,
    vectorised over any set of pairs: selects[p] / hits[p] say per pair whether
    entry p selects the subject / matches the pair, ``weight`` the pod pairs
    behind each."""
    P = len(code)
    order = sorted((int(code[p]), p) for p in range(P) if code[p] != 0xFFFFFFFF)
    cnt = lambda m: int((weight * m).sum())   # noqa: E731
    dec, pas = np.zeros(P, np.int64), np.zeros(P, np.int64)
    sole, tiers = np.zeros(int(group[-1]) + 1, np.int64), np.zeros(8, np.int64)
    open_, passed = np.ones(weight.shape, bool), np.zeros(weight.shape, bool)
    for cd, p in order:                                   # 1: the admin tier
        if cd >> 2 < np_level:
            m = hits[p] & open_
            open_ &= ~m
            if cd & 3 == 2:
                pas[p] = cnt(m)
                passed |= m
            else:
                dec[p] = cnt(m)
                tiers[2 + (cd & 3)] += cnt(m)
    rest, iso = open_ | passed, np.zeros(weight.shape, bool)
    for cd, p in order:
        if cd >> 2 == np_level:
            iso = iso | selects[p]
    net, allowed = rest & iso, np.zeros(weight.shape, bool)   # 2: the NetworkPolicy tier
    matched, owner = np.zeros(weight.shape, np.int32), np.full(weight.shape, -1, np.int64)
    allow = [p for cd, p in order if cd == np_level * 4]
    for g in sorted({int(group[p]) for p in allow}):
        gm = np.zeros(weight.shape, bool)
        for p in allow:
            if group[p] == g:
                m = hits[p] & net & ~allowed
                dec[p] = cnt(m)
                allowed |= m
                gm |= hits[p]
        matched += gm
        owner[gm] = g
    for g in {int(group[p]) for p in allow}:
        sole[g] = cnt(net & (matched == 1) & (owner == g))
    tiers[4], tiers[5] = cnt(allowed), cnt(net & ~allowed)
    b = rest & ~iso                                       # 3: the baseline
    for cd, p in order:
        if cd >> 2 > np_level:
            m = hits[p] & b
            b &= ~m
            dec[p] = cnt(m)
            tiers[6 + (cd & 3)] += cnt(m)
    tiers[0] = cnt(b)
    return dec, pas, sole, tiers


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits", [(4100, 14), (8200, 14), (16500, 15)])
def test_class_rows_wider_than_a_wave(n, bits):
    """More than 4096 (8192) column classes: 66 (130) words a class row, so a
    class takes 128 (256) lanes and its sums meet across waves through LDS;
    more than 16384: 258 words, a second round of the 256 lanes over the words.
    Straight through the C ABI on generic builds, against a numpy resolution
    of one subject pod per row class."""
    from kano._engine import DeviceBuild
    from kano._intern import intern
    cs, pols, sel, alw = _wide_case(n, bits)
    P = len(pols)
    a, b = DeviceBuild(intern(cs, pols), build=False), DeviceBuild(intern(cs, pols), build=False)
    a.build_classes()
    b.build_classes()
    assert a.info()["UA"] == n and a.info()["U"] <= 16
    np_level = 9
    # ids 0..8 admin (levels 0..8: allow, deny, pass in turn), 9..bits - 2
    # baseline (levels 10..), bits - 1 only isolates, the last four the
    # NetworkPolicy tier's allowing entries: one group of two, two groups of one
    code = np.array([q * 4 + q % 3 for q in range(9)]
                    + [(10 + q) * 4 + q % 2 for q in range(bits - 10)]
                    + [np_level * 4 + 3] + [np_level * 4] * 4, np.uint32)
    group = np.array(list(range(bits)) + [bits, bits, bits + 1, bits + 2], np.int32)
    assert len(code) == len(group) == P == bits + 4
    plain = np.array([0xFFFFFFFF] * P, np.uint32)      # the ingress side: every entry dropped
    # one subject pod per row class, weighted by the class's pods
    pattern, rows, weight = np.unique(sel, axis=1, return_index=True, return_counts=True)
    assert weight.sum() == n and len(rows) == a.info()["U"]
    sub = sel[:, rows]
    full = (sub[:, :, None], sub[:, :, None] & alw[:, None, :],
            np.broadcast_to(weight[:, None].astype(np.int64), (len(rows), n)))
    diag = (sel, sel & alw, np.ones(n, np.int64))
    for allow_self in (False, True):
        r = a.k8s_rule_usage(b, allow_self, code, np_level, plain, 0, group, None)
        dec, pas, sole, tiers = _resolve(code, group, np_level, *full)
        if allow_self:                                   # without the diagonal
            dec, pas, sole, tiers = (x - y for x, y in zip(
                (dec, pas, sole, tiers), _resolve(code, group, np_level, *diag)))
        assert np.array_equal(r["decided_e"], dec) and np.array_equal(r["passed_e"], pas)
        assert np.array_equal(r["sole_e"], sole)
        assert np.array_equal(r["tiers"][:8], tiers)
        assert r["tiers"][:8].sum() == n * n - (n if allow_self else 0)
        assert not r["decided_i"].any() and not r["sole_i"].any() and len(r["sole_i"]) == P
        assert r["tiers"][8] == n * n - (n if allow_self else 0)
        assert dec.sum() > 0 and pas.sum() > 0 and sole.sum() > 0
    a.close()
    b.close()


@pytest.mark.gpu
def test_abi_errors_leave_the_contexts_usable():
    from kano import _native as nat, k8s
    from kano._engine import DeviceBuild
    from kano._intern import intern
    cl = _tiered(SEED_ABI)
    pods, pols, nss, admin, baseline = _tier_case(SEED_ABI)[:5]
    n = len(pods)
    c = k8s.compile_conformant(pods, pols, nss, admin, baseline)
    lib = nat.load()

    def operand(entries, rows=None):
        b = DeviceBuild(intern(c.containers, entries), rows=rows, build=False)
        b.build_classes()
        return b

    eg, ing = operand(c.egress), operand(c.ingress)
    code_e, code_i = c.codes(None)
    npe, npi = c.np_level
    (group_e, rules_e), (group_i, rules_i) = k8s.rule_groups(c)
    want = Usage(cl, None, True)

    def call(e, i, ce=code_e, ci=code_i, ge=group_e, gi=group_i, ne=None, ni=None):
        ce, ci = np.ascontiguousarray(ce, np.uint32), np.ascontiguousarray(ci, np.uint32)
        ge, gi = np.ascontiguousarray(ge, np.int32), np.ascontiguousarray(gi, np.int32)
        out = [np.zeros(len(ce), np.int64), np.zeros(len(ce), np.int64),
               np.zeros(len(ce) + 1, np.int64), np.zeros(len(ci), np.int64),
               np.zeros(len(ci), np.int64), np.zeros(len(ci) + 1, np.int64),
               np.zeros(16, np.int64)]
        rc = lib.kano_k8s_rule_usage(
            e and e.ctx, i and i.ctx, 1, len(ce) if ne is None else ne, ce.ctypes.data, npe,
            ge.ctypes.data, len(ci) if ni is None else ni, ci.ctypes.data, npi, gi.ctypes.data,
            *[o.ctypes.data for o in out])
        return rc, out

    def good():
        rc, out = call(eg, ing)
        assert rc == 0
        assert out[6][:8].tolist() == want.egress["tiers"]
        assert out[6][8:].tolist() == want.ingress["tiers"]
        assert int(out[0].sum()) == sum(want.egress["dec"].values())
        assert int(out[5].sum()) == sum(want.ingress["sole"].values())

    good()
    EINVAL, ENOTSUP = -errno.EINVAL, -errno.ENOTSUP
    # groups that decrease, or start below zero
    bad = group_e.copy()
    bad[0] = bad[-1]
    assert bad[0] > bad[1]
    assert call(eg, ing, ge=bad)[0] == EINVAL
    err = lib.kano_last_error(eg.ctx)
    assert b"non-decreasing" in err and b"egress" in err and b"kano_k8s_rule_usage" in err
    assert call(eg, ing, gi=group_i[::-1].copy())[0] == EINVAL
    assert b"ingress" in lib.kano_last_error(eg.ctx)
    assert call(eg, ing, ge=group_e - 1)[0] == EINVAL
    good()
    # nids other than the sources' P, NULL contexts, codes illegal for their level
    assert call(eg, ing, ne=len(code_e) + 1)[0] == EINVAL
    assert b"nids" in lib.kano_last_error(eg.ctx)
    assert call(eg, ing, ni=len(code_i) - 1)[0] == EINVAL
    assert call(None, ing)[0] == EINVAL and call(eg, None)[0] == EINVAL
    denies = code_e.copy()
    denies[0] = npe * 4 + 1
    assert call(eg, ing, ce=denies)[0] == EINVAL and b"denies" in lib.kano_last_error(eg.ctx)
    good()
    # a source that holds a row shard
    shard = operand(c.egress, rows=(0, n // 2))
    assert call(shard, ing)[0] == ENOTSUP and b"row shard" in lib.kano_last_error(shard.ctx)
    assert call(eg, shard, ci=code_e, gi=group_e)[0] == ENOTSUP
    assert b"row shard" in lib.kano_last_error(eg.ctx)
    good()
    # NULL groups: every id its own group; NULL outputs are skipped
    r = eg.k8s_rule_usage(ing, True, code_e, npe, code_i, npi)
    assert len(r["sole_e"]) == len(code_e) and r["tiers"][:8].tolist() == want.egress["tiers"]
    per_rule = np.zeros(len(rules_e), np.int64)
    np.add.at(per_rule, group_e, r["sole_e"])
    full = eg.k8s_rule_usage(ing, True, code_e, npe, code_i, npi, group_e, group_i)
    assert (per_rule <= full["sole_e"]).all()
    assert lib.kano_k8s_rule_usage(eg.ctx, ing.ctx, 1, len(code_e), code_e.ctypes.data, npe, None,
                                   len(code_i), code_i.ctypes.data, npi, None, None, None, None,
                                   None, None, None, None) == 0
    good()
    for b in (eg, ing, shard):
        b.close()
