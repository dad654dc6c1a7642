"""kano.k8s.connectivity with AdminNetworkPolicy tiers (policy.networking.k8s.io/
v1alpha1: Allow / Deny / Pass above the NetworkPolicies, the
BaselineAdminNetworkPolicy below them), written by kano_k8s_conn_tiers.

The oracle below restates the three tiers on numpy bool arrays, straight from
the manifest dicts: it calls neither compile_conformant nor any kano selector
code, and per direction it also says which tier decided each pair.  For every
random cluster used, the oracle alone (port=None) is first checked to have, in
each direction, off-diagonal pairs decided by every tier and action, and a
tiered matrix that both adds to and removes from the NetworkPolicy-only one,
so a pass means something."""
import errno
import functools
import random

import numpy as np
import pytest

from test_k8s_conn import (QUERIES, _bits_of, _cluster, _counts, _known, _pack, _rows, _sel,
                           _unpack, KNOWN, KNOWN_ISO_E, KNOWN_ISO_I, oracle as np_oracle)

# who decided a pair (per direction)
T_ADMIN_ALLOW, T_ADMIN_DENY, T_NETWORK, T_BASE_ALLOW, T_BASE_DENY, T_DEFAULT = range(1, 7)


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------
def _anp_selects(obj, pod, nsl):
    """An AdminNetworkPolicy subject or peer on one pod."""
    if "namespaces" in obj:
        return _sel(obj["namespaces"], nsl[pod.namespace])
    if "pods" in obj:
        pd = obj["pods"]
        return (_sel(pd.get("namespaceSelector"), nsl[pod.namespace])
                and _sel(pd.get("podSelector"), pod.labels))
    return False                                          # nodes / networks / domainNames


def _anp_counts(ports, port):
    if port is None or not ports:
        return True
    proto, num = port
    for e in ports:
        if "portNumber" in e:
            pn = e["portNumber"]
            if pn.get("protocol", "TCP") == proto and pn["port"] == num:
                return True
        elif "portRange" in e:
            pr = e["portRange"]
            if pr.get("protocol", "TCP") == proto and pr["start"] <= num <= pr["end"]:
                return True
    return False                                          # namedPort: never


def _np_direction(pods, pols, nsl, port, typ, key, side):
    """(isolated[x], R[x, y]) of the NetworkPolicies of one type."""
    n = len(pods)
    iso, R = np.zeros(n, bool), np.zeros((n, n), bool)
    for pol in pols:
        spec = pol.spec or {}
        types = spec.get("policyTypes")
        if types is None:
            types = ["Ingress"] + (["Egress"] if "egress" in spec else [])
        if typ not in types:
            continue
        selected = [i for i, p in enumerate(pods)
                    if p.namespace == pol.namespace and _sel(spec.get("podSelector"), p.labels)]
        iso[selected] = True
        for rule in spec.get(key) or []:
            rule = rule or {}
            if not _counts(rule.get("ports"), port):
                continue
            peers = rule.get(side)
            matched = np.zeros(n, bool)
            if not peers:
                matched[:] = True
            for peer in peers or []:
                peer = peer or {}
                if peer.get("ipBlock") is not None:
                    continue
                nsel, psel = peer.get("namespaceSelector"), peer.get("podSelector")
                for j, q in enumerate(pods):
                    if nsel is None:
                        if q.namespace != pol.namespace:
                            continue
                    elif not _sel(nsel, nsl[q.namespace]):
                        continue
                    if psel is not None and not _sel(psel, q.labels):
                        continue
                    matched[j] = True
            R[selected] |= matched
    return iso, R


def _rule_masks(pol, key, side, pods, nsl, port):
    """Per rule of one direction: (action, subject x peer mask), None for a
    rule that does not count."""
    subj = np.array([_anp_selects(pol.spec["subject"], p, nsl) for p in pods], bool)
    out = []
    for rule in pol.spec.get(key) or []:
        if not _anp_counts(rule.get("ports"), port):
            out.append(None)
            continue
        peer = np.array([any(_anp_selects(pe, p, nsl) for pe in rule[side]) for p in pods], bool)
        out.append((rule["action"], subj[:, None] & peer[None, :]))
    return out


def tier_oracle(pods, pols, nss, admin, baseline, port=None, allow_self=True):
    """(allowed[s, d], isoE, isoI, who, passed): who["egress"][x, y] is the
    T_* code of the tier that decided the direction for subject x and peer y,
    passed[...][x, y] whether a Pass rule handed the pair down."""
    nsl = {ns.name: ns.labels for ns in nss}
    n = len(pods)
    order = sorted(range(len(admin)), key=lambda q: (admin[q].spec["priority"], q))
    val, who, passed, iso = {}, {}, {}, {}
    for typ, key, side in (("Egress", "egress", "to"), ("Ingress", "ingress", "from")):
        v, w = np.zeros((n, n), bool), np.zeros((n, n), np.int8)
        und, ps = np.ones((n, n), bool), np.zeros((n, n), bool)
        for q in order:                                   # 1: the admin tier
            for r in _rule_masks(admin[q], key, side, pods, nsl, port):
                if r is None:
                    continue
                action, m = r[0], r[1] & und
                if action == "Allow":
                    v |= m
                    w[m] = T_ADMIN_ALLOW
                elif action == "Deny":
                    w[m] = T_ADMIN_DENY
                else:
                    assert action == "Pass"
                    ps |= m
                und &= ~m
        rest = und | ps
        isod, R = _np_direction(pods, pols, nsl, port, typ, key, side)
        m = rest & isod[:, None]                          # 2: the NetworkPolicy tier
        v |= m & R
        w[m] = T_NETWORK
        b = rest & ~isod[:, None]                         # 3: the baseline tier
        if baseline is not None:
            for r in _rule_masks(baseline, key, side, pods, nsl, port):
                if r is None:
                    continue
                m = r[1] & b
                if r[0] == "Allow":
                    v |= m
                    w[m] = T_BASE_ALLOW
                else:
                    assert r[0] == "Deny"
                    w[m] = T_BASE_DENY
                b &= ~m
        v |= b
        w[b] = T_DEFAULT
        assert w.all()
        val[key], who[key], passed[key], iso[key] = v, w, ps, isod
    allowed = val["egress"] & val["ingress"].T
    if allow_self:
        allowed |= np.eye(n, dtype=bool)
    return allowed, iso["egress"], iso["ingress"], who, passed


# ---------------------------------------------------------------------------
# clusters
# ---------------------------------------------------------------------------
ANP_PORTS = [{"portNumber": {"protocol": "TCP", "port": 80}},
             {"portRange": {"protocol": "TCP", "start": 9000, "end": 9100}},
             {"portNumber": {"protocol": "UDP", "port": 53}},
             {"portNumber": {"port": 443}}]
APPS = ["web", "db", "cache", "api"]


def _tier_cluster(seed, n=60, P=16, nns=3, uid=False):
    """test_k8s_conn's cluster plus 3-6 AdminNetworkPolicies (two of equal
    priority, all three actions, both subject forms, a peer of a non-pod kind,
    a key no pod carries, rules with portNumber, portRange and one namedPort)
    and, in two thirds of the seeds, a baseline."""
    from kano import k8s
    pods, pols, nss = _cluster(seed, n, P, nns, uid)
    rnd = random.Random(seed * 7919 + 13)

    def pods_sel(apps=None):
        sel = {"podSelector": {"matchExpressions": [
            {"key": "app", "operator": "In", "values": apps or rnd.sample(APPS, rnd.randint(1, 2))}]}}
        r = rnd.random()
        if r < 0.3:
            sel["namespaceSelector"] = {"matchLabels": {"team": rnd.choice(["a", "b", "c"])}}
        elif r < 0.5:
            sel["podSelector"]["matchLabels"] = {"tier": rnd.choice(["fe", "be"])}
        return {"pods": sel}

    def ns_sel():
        r = rnd.random()
        if r < 0.5:
            return {"namespaces": {"matchLabels": {"team": rnd.choice(["a", "b", "c"])}}}
        if r < 0.8:
            return {"namespaces": {"matchExpressions": [
                {"key": "env", "operator": rnd.choice(["Exists", "DoesNotExist"])}]}}
        return {"namespaces": {"matchExpressions": [
            {"key": "team", "operator": "NotIn", "values": rnd.sample(["a", "b", "c"], 2)}]}}

    def peer():
        r = rnd.random()
        return pods_sel() if r < 0.6 else ns_sel()

    def rule(side, action=None, ports=None):
        out = {"action": action or rnd.choice(["Allow", "Deny", "Pass"]),
               side: [peer() for _ in range(rnd.randint(1, 2))]}
        if ports is None and rnd.random() < 0.35:
            ports = rnd.sample(ANP_PORTS, rnd.randint(1, 2))
        if ports:
            out["ports"] = ports
        return out

    def anp(name, priority, subject, first=None):
        spec = {"priority": priority, "subject": subject}
        for key, side in (("egress", "to"), ("ingress", "from")):
            rules = [rule(side, first)] if first else []
            rules += [rule(side) for _ in range(rnd.randint(0, 2))]
            spec[key] = rules
        return k8s.AdminNetworkPolicy(name, spec)

    # three policies led by a Pass, a Deny and an Allow rule, the first two of
    # equal priority: the position in the list breaks the tie
    admin = [anp("a-pass", 20, pods_sel(), "Pass"), anp("a-deny", 20, ns_sel(), "Deny"),
             anp("a-allow", 30, pods_sel(), "Allow")]
    for q in range(rnd.randint(0, 3)):
        admin.append(anp(f"a{q}", rnd.choice([5, 10, 30, 40]),
                         pods_sel() if rnd.random() < 0.6 else ns_sel()))
    # the forms every cluster carries: a peer of a non-pod kind beside a pod
    # peer, a key no pod carries, portNumber, portRange and a named port
    admin[0].spec["egress"][0]["to"].append({"networks": ["10.0.0.0/8"]})
    admin[1].spec["ingress"][0]["from"].append({"nodes": {"matchLabels": {"role": "edge"}}})
    admin[2].spec["egress"].append({"action": "Deny", "to": [
        {"pods": {"podSelector": {"matchLabels": {"zone": "x"}}}}, {"domainNames": ["*.example"]}]})
    admin[2].spec["ingress"].append({"action": "Deny", "from": [pods_sel()], "ports": [
        {"portNumber": {"protocol": "TCP", "port": 80}},
        {"portRange": {"protocol": "TCP", "start": 9000, "end": 9100}}]})
    admin[0].spec["ingress"].append({"action": "Allow", "from": [ns_sel()],
                                     "ports": [{"namedPort": "http"}]})
    rnd.shuffle(admin)
    baseline = None
    if seed % 3:
        spec = {"subject": pods_sel(rnd.sample(APPS, 3))}
        for key, side in (("egress", "to"), ("ingress", "from")):
            spec[key] = [rule(side, "Allow"), {"action": "Deny", side: [{"namespaces": {}}]}]
        baseline = k8s.BaselineAdminNetworkPolicy("default", spec)
    return pods, pols, nss, admin, baseline


@functools.lru_cache(maxsize=None)
def _tier_case(seed, n=60, P=16, nns=3, uid=False):
    """A cluster with its oracle results per (port, allow_self), computed once
    and never written; the conditions that make it a meaningful case are
    checked on the oracle alone (port=None)."""
    pods, pols, nss, admin, baseline = _tier_cluster(seed, n, P, nns, uid)
    full, isoE, isoI, who, passed = tier_oracle(pods, pols, nss, admin, baseline, None, True)
    off = ~np.eye(n, dtype=bool)
    for d in ("egress", "ingress"):
        w, ps = who[d], passed[d]
        kinds = {"admin Allow": w == T_ADMIN_ALLOW, "admin Deny": w == T_ADMIN_DENY,
                 "Pass then NetworkPolicy": ps & (w == T_NETWORK),
                 "Pass then baseline or default": ps & (w >= T_BASE_ALLOW),
                 "NetworkPolicy, no admin match": ~ps & (w == T_NETWORK),
                 "default allow": w == T_DEFAULT}
        if baseline is not None:
            kinds["baseline Deny"] = w == T_BASE_DENY
        for name, m in kinds.items():
            assert (m & off).any(), (seed, d, name)
    plain = np_oracle(pods, pols, nss, None, True)[0]
    assert (full & ~plain).any() and (plain & ~full).any(), seed
    assert len({a.spec["priority"] for a in admin}) < len(admin)
    for a in (full, isoE, isoI):
        a.setflags(write=False)
    return pods, pols, nss, admin, baseline, {(None, True): full}, isoE, isoI


def _tref(case, port, allow_self):
    """The oracle's matrix of one query, computed once."""
    pods, pols, nss, admin, baseline, ref = case[:6]
    if (port, allow_self) not in ref:
        a = tier_oracle(pods, pols, nss, admin, baseline, port, allow_self)[0]
        a.setflags(write=False)
        ref[(port, allow_self)] = a
    return ref[(port, allow_self)]


# seeds whose clusters meet _tier_case's conditions (found by running it)
SEEDS_60 = [5, 6, 7, 11, 14, 16, 17, 18, 24, 26, 27, 28]     # (8 of them with a baseline)
SEEDS_40 = [2, 6, 7, 16, 18, 20]
SEED_130, SEED_1030, SEED_UID, SEED_SHARDS, SEED_QUERIES, SEED_ABI = 23, 24, 31, 5, 7, 11


# ---------------------------------------------------------------------------
# the known answers: test_k8s_conn's six-pod cluster (p0 shop/web, p1 shop/api,
# p2 shop/db, p3 ops/mon, p4 ops/job, p5 ops/web; shop team=a, ops team=b; its
# NetworkPolicies isolate egress of p0 (D: anywhere on UDP 53) and p1 (B: db),
# ingress of p0 (D: nothing), p2 (A: api on TCP 5432, mon on 9000-9100) and
# p3..p5 (C: nothing)) plus two AdminNetworkPolicies and a baseline.
# ---------------------------------------------------------------------------
def _known_tiers():
    from kano import k8s
    pods, pols, nss = _known()
    team = lambda v: {"matchLabels": {"team": v}}   # noqa: E731
    app = lambda v: {"matchLabels": {"app": v}}     # noqa: E731
    admin = [
        # Y, priority 9, subject the web pods p0, p5
        k8s.AdminNetworkPolicy("Y", {
            "priority": 9, "subject": {"pods": {"namespaceSelector": {}, "podSelector": app("web")}},
            "egress": [{"action": "Allow", "to": [{"namespaces": team("b")}]}],
            "ingress": [{"action": "Deny", "from": [{"pods": {"namespaceSelector": {},
                                                              "podSelector": app("job")}}]}]}),
        # X, priority 5 (evaluated first), subject the shop pods p0, p1, p2
        k8s.AdminNetworkPolicy("X", {
            "priority": 5, "subject": {"namespaces": team("a")},
            "egress": [
                {"action": "Pass", "to": [{"pods": {"namespaceSelector": team("a"),
                                                    "podSelector": app("db")}}]},
                {"action": "Deny", "to": [{"namespaces": team("b")}],
                 "ports": [{"portNumber": {"protocol": "TCP", "port": 80}}]}],
            "ingress": [
                {"action": "Allow", "from": [{"pods": {"namespaceSelector": team("b"),
                                                       "podSelector": app("mon")}},
                                             {"networks": ["10.0.0.0/8"]}],
                 "ports": [{"portRange": {"protocol": "TCP", "start": 9000, "end": 9100}}]}]}),
    ]
    # the baseline, subject the ops pods p3, p4, p5
    baseline = k8s.BaselineAdminNetworkPolicy("base", {
        "subject": {"namespaces": team("b")},
        "egress": [
            {"action": "Allow", "to": [{"pods": {"namespaceSelector": team("a"), "podSelector": {
                "matchExpressions": [{"key": "app", "operator": "In", "values": ["api", "web"]}]}}}]},
            {"action": "Deny", "to": [{"namespaces": {}}]}]})
    return pods, pols, nss, admin, baseline


# port=None: every rule counts.  Egress levels: X0 Pass {p0,p1,p2}->p2, X1 Deny
# {p0,p1,p2}->{p3,p4,p5}, Y0 Allow {p0,p5}->{p3,p4,p5}.  Egress rows (x -> y):
#   p0 111000  y=0,1 no admin match, D allows all; y=2 passed, D; y=3..5 X1 denies
#   p1 001000  y=2 passed, B allows db; y=0,1 B isolates; y=3..5 X1 denies
#   p2 111000  not isolated, no baseline subject: default; y=3..5 X1 denies
#   p3 110000  p4 110000  baseline: Allow shop api / web, then Deny all
#   p5 110111  y=3..5 Y0 allows; the rest by the baseline
# Ingress levels: X0 Allow {p0,p1,p2}<-p3, Y0 Deny {p0,p5}<-p4.  Rows (x <- y):
#   p0 000100  y=3 X0; y=4 Y0 denies; the rest: D isolates, no rule
#   p1 111111  y=3 X0; not isolated, the baseline has no ingress rule: default
#   p2 010100  y=3 X0; A allows p1 (and p3)
#   p3 p4 p5 000000  C isolates (p5 <- p4 also denied by Y0)
# allowed[s][d] = egress[s][d] & ingress[d][s] | diagonal.  Against the
# NetworkPolicy-only rows p3 -> p0 is added (X0 admits mon where D isolates) and
# p3 -> p2 removed (the baseline denies).
# ("TCP", 80): X0's ingress Allow (9000-9100) drops, X1's Deny counts; A's two
# rules and D's egress rule drop but still isolate.  Egress: p0 000000, p1 001000,
# p2 111000, p3 p4 110000, p5 110111; ingress: p1 111111, every other row empty.
# ("TCP", 9050): X1's Deny (TCP 80) drops, X0's ingress Allow counts; of A only
# the mon rule counts, D's egress rule drops.  Egress: p0 000111 (Y0), p1 001000,
# p2 111111, p3 p4 110000, p5 110111; ingress: p0 000100, p1 111111, p2 000100.
KNOWN_TIERS = {
    (None, True): "110000 011000 011000 110100 010010 010001",
    (("TCP", 80), True): "100000 010000 011000 010100 010010 010001",
    (("TCP", 9050), True): "100000 010000 011000 110100 010010 010001",
    (None, False): "010000 001000 010000 110000 010000 010000",
}


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------
def test_known_answers_oracle():
    pods, pols, nss, admin, baseline = _known_tiers()
    for (port, allow_self), rows in KNOWN_TIERS.items():
        a, isoE, isoI = tier_oracle(pods, pols, nss, admin, baseline, port, allow_self)[:3]
        assert np.array_equal(a, _bits_of(rows)), (port, allow_self)
        assert np.array_equal(isoE, _bits_of(KNOWN_ISO_E)[0])
        assert np.array_equal(isoI, _bits_of(KNOWN_ISO_I)[0])
    # without admin and baseline the oracle is test_k8s_conn's
    for (port, allow_self), rows in KNOWN.items():
        a = tier_oracle(pods, pols, nss, [], None, port, allow_self)[0]
        assert np.array_equal(a, _bits_of(rows)), (port, allow_self)


def _compiled_tiers(pods, pols, nss, admin, baseline, port, allow_self):
    """compile_conformant's lists evaluated by the kano restatement (oracle
    ref_py: the per-entry select / allow sets) and resolved per tier in numpy
    from the entries' codes."""
    from kano import k8s
    from oracle import kano_oracle as orc
    n = len(pods)
    c = k8s.compile_conformant(pods, pols, nss, admin, baseline)
    codes = c.codes(port)
    out = []
    for k, entries in enumerate((c.egress, c.ingress)):
        code, np_level = codes[k].astype(np.int64), c.np_level[k]
        r = orc.ref_py(c.containers, entries)
        sel = np.array([[ch == "1" for ch in s] for s in r["sel"]], dtype=bool).reshape(-1, n)
        alw = np.array([[ch == "1" for ch in s] for s in r["allow"]], dtype=bool).reshape(-1, n)
        live = code != 0xFFFFFFFF

        def pairs(ids):
            m = np.zeros((n, n), bool)
            for p in ids:
                m |= sel[p][:, None] & alw[p][None, :]
            return m

        v, und, ps = np.zeros((n, n), bool), np.ones((n, n), bool), np.zeros((n, n), bool)
        for cd in sorted(set(code[live & (code >> 2 < np_level)].tolist())):
            m = pairs(np.flatnonzero(code == cd)) & und
            if cd & 3 == 0:
                v |= m
            elif cd & 3 == 2:
                ps |= m
            und &= ~m
        rest = und | ps
        at_np = np.flatnonzero(live & (code >> 2 == np_level))
        iso = sel[at_np].any(axis=0) if len(at_np) else np.zeros(n, bool)
        v |= rest & iso[:, None] & pairs(np.flatnonzero(code == np_level * 4))
        b = rest & ~iso[:, None]
        for cd in sorted(set(code[live & (code >> 2 > np_level)].tolist())):
            m = pairs(np.flatnonzero(code == cd)) & b
            if cd & 3 == 0:
                v |= m
            b &= ~m
        out.append((v | b, iso))
    (E, isoE), (In, isoI) = out
    allowed = E & In.T
    if allow_self:
        allowed |= np.eye(n, dtype=bool)
    return allowed, isoE, isoI


def test_known_answers_compiled():
    pods, pols, nss, admin, baseline = _known_tiers()
    for (port, allow_self), rows in KNOWN_TIERS.items():
        a, isoE, isoI = _compiled_tiers(pods, pols, nss, admin, baseline, port, allow_self)
        assert np.array_equal(a, _bits_of(rows)), (port, allow_self)
        assert np.array_equal(isoE, _bits_of(KNOWN_ISO_E)[0])
        assert np.array_equal(isoI, _bits_of(KNOWN_ISO_I)[0])


def test_compiled_tiers_origins_levels_and_codes():
    from kano import k8s
    pods, pols, nss, admin, baseline = _known_tiers()
    c = k8s.compile_conformant(pods, pols, nss, admin, baseline)
    assert c.tiered and c.np_level == (3, 2) and c.admin_priority_ties == 0
    # X (index 1 of admin) comes first: priority 5 before 9; the peer that
    # selects no pod (networks) has no entry
    assert c.origin_egress == [(1, "egress", 0, 0), (1, "egress", 1, 0), (0, "egress", 0, 0),
                               (1, "egress", 0, 0), (3, "egress", 0, 0),
                               (0, "egress", 0, 0), (0, "egress", 1, 0)]
    assert c.tiers_egress == [("admin", 0, "Pass"), ("admin", 1, "Deny"), ("admin", 2, "Allow"),
                              ("network", 3, "Allow"), ("network", 3, "Allow"),
                              ("baseline", 4, "Allow"), ("baseline", 5, "Deny")]
    assert c.tiers_ingress == [("admin", 0, "Allow"), ("admin", 1, "Deny"),
                               ("network", 2, "Allow"), ("network", 2, "Allow"),
                               ("network", 2, "Isolate"), ("network", 2, "Isolate")]
    dead = 0xFFFFFFFF
    ce, ci = c.codes(None)
    assert ce.dtype == np.uint32 and ce.tolist() == [2, 5, 8, 12, 12, 16, 21]
    assert ci.tolist() == [0, 5, 8, 8, 11, 11]
    ce, ci = c.codes(("TCP", 80))
    assert ce.tolist() == [2, 5, 8, 12, 15, 16, 21]      # D's UDP rule: isolates only
    assert ci.tolist() == [dead, 5, 11, 11, 11, 11]
    ce, ci = c.codes(("TCP", 9050))
    assert ce.tolist() == [2, dead, 8, 12, 15, 16, 21]
    assert ci.tolist() == [0, 5, 11, 8, 11, 11]


@pytest.mark.parametrize("seed", SEEDS_40)
def test_compilation_matches_oracle(seed):
    case = _tier_case(seed, n=40, P=14)
    pods, pols, nss, admin, baseline, _, isoE, isoI = case
    for port in [None] + QUERIES:
        a, e, i = _compiled_tiers(pods, pols, nss, admin, baseline, port, True)
        assert np.array_equal(e, isoE) and np.array_equal(i, isoI)
        assert np.array_equal(a, _tref(case, port, True)), port
    a, _, _ = _compiled_tiers(pods, pols, nss, admin, baseline, None, False)
    assert np.array_equal(a, _tref(case, None, False))


def test_compile_without_tiers_is_unchanged():
    from kano import k8s
    pods, pols, nss = _cluster(4, 40, 14)
    plain = k8s.compile_conformant(pods, pols, nss)
    for admin, baseline in ((None, None), ([], None), ((), [])):
        c = k8s.compile_conformant(pods, pols, nss, admin, baseline)
        assert not c.tiered and c.np_level == (0, 0)
        assert c.origin_egress == plain.origin_egress
        assert c.origin_ingress == plain.origin_ingress
        assert c.ports_egress == plain.ports_egress and c.ports_ingress == plain.ports_ingress
        for got, want in ((c.egress, plain.egress), (c.ingress, plain.ingress)):
            assert [(repr(p.selector.labels), repr(p.allow.labels)) for p in got] == \
                [(repr(p.selector.labels), repr(p.allow.labels)) for p in want]
        assert [repr(x.labels) for x in c.containers] == [repr(x.labels) for x in plain.containers]
        assert {t[0] for t in c.tiers_egress + c.tiers_ingress} <= {"network"}


def test_host_errors():
    from kano import k8s
    nss = [k8s.Namespace("default")]
    pods = [k8s.Pod("a", None, {"x": "1"})]
    everyone = {"namespaces": {}}

    def anp(spec, **kw):
        return k8s.AdminNetworkPolicy("bad", dict({"priority": 1, "subject": everyone}, **spec),
                                      **kw)

    def rule(**kw):
        return dict({"action": "Allow", "to": [everyone]}, **kw)

    bad_admin = [
        anp({"egress": [rule(action="Reject")]}),
        anp({"egress": [rule(action=None)]}),
        anp({"priority": 1001}), anp({"priority": -1}), anp({"priority": "3"}),
        anp({"priority": 2.5}), anp({"priority": True}), anp({"priority": None}),
        anp({"egress": [rule(to=[])]}),
        anp({"egress": [{"action": "Allow"}]}),
        anp({"ingress": [{"action": "Deny", "to": [everyone]}]}),        # ingress needs from
        anp({"subject": {}}),
        anp({"subject": {"namespaces": {}, "pods": {}}}),
        anp({"egress": [rule(to=[{}])]}),
        anp({"egress": [rule(to=[{"namespaces": {}, "pods": {"podSelector": {}}}])]}),
    ]
    for a in bad_admin:
        with pytest.raises(ValueError, match="bad"):
            k8s.compile_conformant(pods, [], nss, [a])
    with pytest.raises(ValueError, match=r"egress rule 1"):
        k8s.compile_conformant(pods, [], nss, [anp({"egress": [rule(), rule(action="Drop")]})])
    base = lambda spec: k8s.BaselineAdminNetworkPolicy(   # noqa: E731
        "bad", dict({"subject": everyone}, **spec))
    with pytest.raises(ValueError, match="bad.*egress rule 0"):
        k8s.compile_conformant(pods, [], nss, [], base({"egress": [rule(action="Pass")]}))
    with pytest.raises(ValueError, match="bad"):
        k8s.compile_conformant(pods, [], nss, None, base({"subject": {"pods": {}, "namespaces": {}}}))
    ok = base({"egress": [rule(action="Deny")]})
    with pytest.raises(ValueError):
        k8s.compile_conformant(pods, [], nss, [], [ok, ok])
    c = k8s.compile_conformant(pods, [], nss, [], [ok])
    assert c.tiered and c.tiers_egress == [("baseline", 1, "Deny")]
    # a matchExpressions operator is checked in an admin selector too
    with pytest.raises(ValueError):
        k8s.compile_conformant(pods, [], nss, [anp({"subject": {"namespaces": {
            "matchExpressions": [{"key": "x", "operator": "Gt"}]}}})])
    with pytest.raises(ValueError):
        k8s.from_dict("ClusterNetworkPolicy", {})


def test_load_cluster(tmp_path):
    from kano import k8s
    (tmp_path / "a.yaml").write_text("""
apiVersion: v1
kind: Namespace
metadata: {name: shop, labels: {team: a}}
---
apiVersion: v1
kind: Pod
metadata: {name: web, namespace: shop, labels: {app: web}}
---
apiVersion: v1
kind: Pod
metadata: {name: db, namespace: shop, labels: {app: db}}
---
apiVersion: networking.k8s.io/v1
kind: NetworkPolicy
metadata: {name: deny, namespace: shop}
spec: {podSelector: {}, policyTypes: [Ingress]}
---
apiVersion: policy.networking.k8s.io/v1alpha1
kind: AdminNetworkPolicy
metadata: {name: second}
spec:
  priority: 7
  subject: {namespaces: {}}
  ingress:
  - action: Deny
    from: [{namespaces: {}}]
""")
    (tmp_path / "b.yml").write_text("""
apiVersion: v1
kind: List
items:
- apiVersion: policy.networking.k8s.io/v1alpha1
  kind: AdminNetworkPolicy
  metadata: {name: first}
  spec:
    priority: 3
    subject: {pods: {podSelector: {matchLabels: {app: db}}}}
    ingress:
    - action: Allow
      from: [{pods: {podSelector: {matchLabels: {app: web}}}}]
      ports: [{portNumber: {protocol: TCP, port: 5432}}]
- apiVersion: policy.networking.k8s.io/v1alpha1
  kind: BaselineAdminNetworkPolicy
  metadata: {name: default}
  spec:
    subject: {namespaces: {}}
    egress:
    - action: Deny
      to: [{namespaces: {}}]
""")
    cl = k8s.load_cluster([tmp_path])
    assert cl._fields == ("pods", "policies", "namespaces", "admin", "baseline")
    assert [p.name for p in cl.pods] == ["web", "db"]
    assert [(a.name, a.spec["priority"]) for a in cl.admin] == [("second", 7), ("first", 3)]
    assert isinstance(cl.admin[0], k8s.AdminNetworkPolicy)
    assert isinstance(cl.baseline, k8s.BaselineAdminNetworkPolicy)
    assert cl.baseline.name == "default" and cl.baseline.spec["egress"][0]["action"] == "Deny"
    # load_manifests: the same three results, the new kinds ignored
    pods, pols, nss = k8s.load_manifests([tmp_path])
    assert [p.name for p in pods] == ["web", "db"] and [p.name for p in pols] == ["deny"]
    assert {ns.name: ns.labels for ns in nss} == {ns.name: ns.labels for ns in cl.namespaces} \
        == {"shop": {"team": "a", "kubernetes.io/metadata.name": "shop"}}
    assert k8s.load_cluster(str(tmp_path / "a.yaml")).baseline is None
    # web -> db on 5432: the admin Allow beats the NetworkPolicy, but the
    # baseline denies web's egress; on other ports "second" denies ingress
    a = tier_oracle(*cl, port=("TCP", 5432), allow_self=False)[0]
    c = _compiled_tiers(*cl, ("TCP", 5432), False)[0]
    assert np.array_equal(a, c) and not a.any()
    a = tier_oracle(cl.pods, cl.policies, cl.namespaces, cl.admin, None, ("TCP", 5432), False)[0]
    c = _compiled_tiers(cl.pods, cl.policies, cl.namespaces, cl.admin, None, ("TCP", 5432), False)[0]
    assert np.array_equal(a, c) and a.tolist() == [[False, True], [False, False]]
    (tmp_path / "c.yaml").write_text("""
kind: BaselineAdminNetworkPolicy
metadata: {name: another}
spec: {subject: {namespaces: {}}}
""")
    with pytest.raises(ValueError):
        k8s.load_cluster([tmp_path])
    assert len(k8s.load_manifests([tmp_path])[0]) == 2


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------
def _connect(case_or_cluster, **kw):
    from kano import k8s
    pods, pols, nss, admin, baseline = case_or_cluster[:5]
    return k8s.connectivity(pods, pols, nss, admin=admin, baseline=baseline, **kw)


@pytest.mark.gpu
def test_known_answers_gpu():
    cl = _known_tiers()
    base = {True: _connect(cl), False: _connect(cl, allow_self=False)}
    for (port, allow_self), rows in KNOWN_TIERS.items():
        want = _bits_of(rows)
        direct = _connect(cl, port=port, allow_self=allow_self)
        again = base[allow_self].on_port(port)
        for r in (direct, again):
            assert np.array_equal(_rows(r.allowed), want), (port, allow_self)
            assert np.array_equal(r.egress_isolated, _bits_of(KNOWN_ISO_E)[0])
            assert np.array_equal(r.ingress_isolated, _bits_of(KNOWN_ISO_I)[0])
            assert r.info["egress_isolated"] == 2 and r.info["ingress_isolated"] == 5
        # the same two resident builds, nothing uploaded again
        assert again.egress is base[allow_self].egress
        assert again.ingress is base[allow_self].ingress
    r = base[True]
    assert r.info["egress_entries"] == 7 and r.info["ingress_entries"] == 6
    assert r.info["kept_egress_entries"] == 7 and r.info["kept_ingress_entries"] == 6
    assert r.info["admin_entries"] == 5 and r.info["baseline_entries"] == 2
    assert r.info["admin_levels"] == 5 and r.info["admin_priority_ties"] == 0
    p = r.on_port(("TCP", 9050))
    assert p.info["kept_egress_entries"] == 6 and p.info["kept_ingress_entries"] == 6
    assert p.info["port"] == ("TCP", 9050) and p.port == ("TCP", 9050)
    assert r.on_port(("TCP", 80)).info["kept_ingress_entries"] == 5


def _check(case, port, allow_self, r):
    assert np.array_equal(_rows(r.allowed), _tref(case, port, allow_self)), (port, allow_self)
    assert np.array_equal(r.egress_isolated, case[6])
    assert np.array_equal(r.ingress_isolated, case[7])
    assert r.info["egress_isolated"] == int(case[6].sum())
    assert r.info["ingress_isolated"] == int(case[7].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("allow_self", [True, False])
@pytest.mark.parametrize("seed", SEEDS_60)
def test_matches_oracle(seed, allow_self):
    case = _tier_case(seed)
    for form in ("auto", "direct", "stream"):
        r = _connect(case, allow_self=allow_self, form=form)
        assert r.info["admin_priority_ties"] >= 1
        _check(case, None, allow_self, r)
        for port in (QUERIES[seed % 3], QUERIES[(seed + 1) % 3]):
            _check(case, port, allow_self, r.on_port(port))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["direct", "stream", "auto"])
@pytest.mark.parametrize("seed,n,P", [(SEED_130, 130, 20), (SEED_1030, 1030, 30)])
def test_matches_oracle_more_blocks(seed, n, P, form):
    """n = 130: three words a row; n = 1030 crosses the 1024-destination
    block and the 64-row block, in both forms of the write.  Pad bits and pad
    words read as zero."""
    case = _tier_case(seed, n=n, P=P, nns=4)
    r = _connect(case, form=form)
    _check(case, None, True, r)
    for port in QUERIES[:2]:
        _check(case, port, True, r.on_port(port))
    words = r.allowed.engine.rows(0, n)
    assert words.shape == (n, (n + 63) // 64)
    assert np.array_equal(words, _pack(_tref(case, None, True)))
    assert not (words[:, -1] >> np.uint64(n & 63)).any()


@pytest.mark.gpu
def test_every_pod_its_own_class():
    """The uid cluster: every pod is its own row and column class on both
    sides, so a class row has ldC = 35 words (not a power of two: the group's
    upper lanes idle) and the class count is no multiple of the classes a
    block holds.  The direct form once, the streamed form once."""
    n = 2200
    case = _tier_case(SEED_UID, n=n, P=24, nns=3, uid=True)
    r = _connect(case, form="direct")
    ie, ii = r.egress.engine.info(), r.ingress.engine.info()
    assert (ie["UA"] + 63) // 64 == 35 and (ii["UA"] + 63) // 64 == 35
    assert ie["U"] == n and ii["U"] == n
    _check(case, None, True, r)
    _check(case, QUERIES[0], True, _connect(case, port=QUERIES[0], form="stream"))


def _long_list_cluster():
    """70 pods, each with its own "id"; four AdminNetworkPolicies of 80 egress
    rules with two single-pod peers each, all with the subject "every pod": one
    subject class with 640 admin entries over 320 levels (plus the
    NetworkPolicy and baseline entries).  Ids 1..6 are kept out of the random
    rules and used by the constructs: an Allow after a Deny on overlapping
    peers, a Pass followed (levels later) by a Deny on the same peer, and a pod
    only the last level names."""
    from kano import k8s
    rnd = random.Random(99)
    n = 70
    nss = [k8s.Namespace("a", {"team": "x"})]
    pods = [k8s.Pod(f"p{i}", "a", {"id": i, "app": "w" if i % 3 else "d"}) for i in range(n)]
    one = lambda i: {"pods": {"podSelector": {"matchLabels": {"id": i}}}}   # noqa: E731
    free = list(range(7, n))

    def rules(k):
        return [{"action": rnd.choice(["Allow", "Deny", "Pass"]),
                 "to": [one(i) for i in rnd.sample(free, 2)]} for _ in range(k)]

    admin = []
    for q in range(4):
        admin.append(k8s.AdminNetworkPolicy(f"long{q}", {
            "priority": 10 * q, "subject": {"namespaces": {}}, "egress": rules(80)}))
    first, last = admin[0].spec["egress"], admin[3].spec["egress"]
    first[3] = {"action": "Deny", "to": [one(1), one(2)]}
    first[40] = {"action": "Allow", "to": [one(2), one(3)]}     # p2 stays denied, p3 allowed
    first[5] = {"action": "Pass", "to": [one(4), one(5)]}
    last[70] = {"action": "Deny", "to": [one(5), one(1)]}       # after the Pass: no effect
    last[79] = {"action": "Allow", "to": [one(4), one(6)]}
    # the d pods' egress is isolated: a passed pair goes to this policy
    pols = [k8s.NetworkPolicy("np", "a", {
        "podSelector": {"matchLabels": {"app": "d"}}, "policyTypes": ["Egress"],
        "egress": [{"to": [{"podSelector": {"matchLabels": {"app": "w"}}}]}]})]
    baseline = k8s.BaselineAdminNetworkPolicy("base", {
        "subject": {"namespaces": {}},
        "egress": [{"action": "Deny", "to": [{"pods": {"podSelector": {"matchLabels": {"app": "d"}}}}]}]})
    return pods, pols, nss, admin, baseline


@pytest.mark.gpu
def test_long_list_of_many_levels():
    cl = _long_list_cluster()
    pods, pols, nss, admin, baseline = cl
    n = len(pods)
    want, isoE, isoI, who, passed = tier_oracle(*cl, None, False)
    eg = who["egress"]
    # the constructs decide as derived: the early Deny holds against the later
    # Allow on p2, the Allow reaches p3; p4 and p5 are passed on, whatever the
    # Deny and the Allow 300 levels later say
    assert (eg[:, 1] == T_ADMIN_DENY).all() and (eg[:, 2] == T_ADMIN_DENY).all()
    assert (eg[:, 3] == T_ADMIN_ALLOW).all()
    assert passed["egress"][:, 4].all() and passed["egress"][:, 5].all()
    d = np.array([p.labels["app"] == "d" for p in pods])
    for y in (4, 5):      # (w pods) to the NetworkPolicy for the isolated d pods, else default
        assert (eg[d, y] == T_NETWORK).all() and (eg[~d, y] == T_DEFAULT).all()
    # the last of the 320 levels matters: only it names p6
    assert (eg[:, 6] == T_ADMIN_ALLOW).all()
    assert {T_ADMIN_ALLOW, T_ADMIN_DENY, T_NETWORK, T_DEFAULT, T_BASE_DENY} \
        <= set(eg.reshape(-1).tolist())
    for form in ("direct", "stream"):
        r = _connect(cl, allow_self=False, form=form)
        assert np.array_equal(_rows(r.allowed), want), form
        assert np.array_equal(r.egress_isolated, isoE) and not r.ingress_isolated.any()
    c = r._compiled
    assert c.np_level[0] == 320 and r.info["admin_entries"] == 640
    # one row class holds every admin entry: several LDS rounds of 256 in the
    # ordered copy; and the classes are no multiple of a block's
    off, _ = r.egress.engine.select_csr()
    assert int(np.diff(off).max()) >= 600
    info = r.egress.engine.info()
    ldC = (info["UA"] + 63) // 64
    wl = 1
    while wl < 256 and wl < ldC:
        wl *= 2
    assert info["U"] % (256 // wl) != 0
    # a port no rule names changes nothing here (no rule carries ports)
    assert np.array_equal(_rows(r.on_port(("TCP", 1)).allowed), want)


@pytest.mark.gpu
def test_degenerate_inputs():
    from kano import k8s
    nss = [k8s.Namespace("a", {"team": "x"})]
    everyone = {"namespaces": {}}
    app = lambda v: {"pods": {"podSelector": {"matchLabels": {"app": v}}}}   # noqa: E731
    deny_all = k8s.BaselineAdminNetworkPolicy("deny", {
        "subject": everyone, "egress": [{"action": "Deny", "to": [everyone]}],
        "ingress": [{"action": "Deny", "from": [everyone]}]})

    def check(pods, pols, admin, baseline, want=None, ports=(None,), forms=("auto",)):
        for port in ports:
            for allow_self in (True, False):
                a, isoE, isoI = tier_oracle(pods, pols, nss, admin, baseline, port, allow_self)[:3]
                for form in forms:
                    r = k8s.connectivity(pods, pols, nss, port=port, allow_self=allow_self,
                                         form=form, admin=admin, baseline=baseline)
                    assert np.array_equal(_rows(r.allowed), a), (port, allow_self, form)
                    assert np.array_equal(r.egress_isolated, isoE)
                    assert np.array_equal(r.ingress_isolated, isoI)
                if want is not None:
                    assert np.array_equal(a, want(allow_self)), (port, allow_self)

    n_deny = k8s.NetworkPolicy("deny", "a", {"podSelector": {},
                                             "policyTypes": ["Ingress", "Egress"]})
    for n in (0, 1):
        pods = [k8s.Pod(f"p{i}", "a", {"app": "w"}) for i in range(n)]
        check(pods, [], [], deny_all, lambda s, n=n: np.eye(n, dtype=bool) & s)
        check(pods, [n_deny], [k8s.AdminNetworkPolicy("x", {
            "priority": 0, "subject": everyone,
            "egress": [{"action": "Allow", "to": [everyone]}],
            "ingress": [{"action": "Allow", "from": [everyone]}]})], None,
            lambda s, n=n: np.ones((n, n), bool))
    pods = [k8s.Pod(f"p{i}", "a", {"app": "w" if i % 3 else "d"}) for i in range(70)]
    n = len(pods)
    d = np.array([p.labels["app"] == "d" for p in pods])
    both = ("direct", "stream")
    # a baseline only: deny-all gives the diagonal, and nothing without allow_self
    check(pods, [], [], deny_all, lambda s: np.eye(n, dtype=bool) & s, forms=both)
    # ANPs only, and only egress rules: the ingress side has no entry at all
    a_deny = k8s.AdminNetworkPolicy("x", {"priority": 3, "subject": app("d"), "egress": [
        {"action": "Deny", "to": [app("w")], "ports": [{"portNumber": {"port": 80}}]}]})
    check(pods, [], [a_deny], None,
          lambda s: ~(d[:, None] & ~d[None, :]) | (np.eye(n, dtype=bool) & s),
          ports=(None, ("TCP", 80)), forms=both)
    # ... and on a port that drops every admin entry: the plain reading (all ones)
    check(pods, [], [a_deny], None, lambda s: np.ones((n, n), bool), ports=(("TCP", 81),),
          forms=both)
    # only ingress rules: the egress side has no entry
    check(pods, [], [k8s.AdminNetworkPolicy("x", {"priority": 3, "subject": app("d"), "ingress": [
        {"action": "Deny", "from": [app("w")]}]})], None,
        lambda s: ~(~d[:, None] & d[None, :]) | (np.eye(n, dtype=bool) & s), forms=both)
    # a Pass with neither a NetworkPolicy nor a baseline behind it: allowed
    a_pass = k8s.AdminNetworkPolicy("p", {"priority": 1, "subject": everyone, "egress": [
        {"action": "Pass", "to": [app("w")]}, {"action": "Deny", "to": [everyone]}]})
    check(pods, [], [a_pass], None,
          lambda s: np.broadcast_to(~d[None, :], (n, n)) | (np.eye(n, dtype=bool) & s), forms=both)
    # a port query that drops every admin entry equals the plain reading
    np_in = k8s.NetworkPolicy("i", "a", {
        "podSelector": {"matchLabels": {"app": "d"}}, "policyTypes": ["Ingress"],
        "ingress": [{"from": [{"podSelector": {"matchLabels": {"app": "d"}}}],
                     "ports": [{"port": 80}]}]})
    for port in (("TCP", 81), ("TCP", 80)):
        plain = np_oracle(pods, [np_in], nss, port, True)[0]
        if port == ("TCP", 81):    # ... which drops the policy's only rule: still isolated
            assert np.array_equal(plain, ~np.broadcast_to(d[None, :], (n, n)) | np.eye(n, dtype=bool))
        r = k8s.connectivity(pods, [np_in], nss, port=port, admin=[a_deny])
        want = plain if port == ("TCP", 81) else plain & ~(d[:, None] & ~d[None, :])
        assert np.array_equal(_rows(r.allowed), want)
        assert np.array_equal(r.ingress_isolated, d) and not r.egress_isolated.any()
        assert r.info["ingress_isolated"] == int(d.sum())
        assert r.info["kept_egress_entries"] == (0 if port == ("TCP", 81) else 1)


@pytest.mark.gpu
def test_without_tiers_is_the_plain_call():
    from kano import k8s
    case = _tier_case(SEEDS_60[2])
    pods, pols, nss = case[:3]
    n = len(pods)
    for port in (None, QUERIES[0]):
        plain = k8s.connectivity(pods, pols, nss, port=port)
        for kw in ({"admin": [], "baseline": None}, {"admin": None}, {"baseline": []}):
            r = k8s.connectivity(pods, pols, nss, port=port, **kw)
            assert np.array_equal(r.allowed.engine.rows(0, n), plain.allowed.engine.rows(0, n))
            assert r.info == plain.info and "admin_entries" not in r.info
            assert np.array_equal(r.egress_isolated, plain.egress_isolated)
            assert r.explain(3, 9) == plain.explain(3, 9)
            assert "tier" not in r.explain(3, 9)["egress"]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["direct", "stream"])
@pytest.mark.parametrize("cuts", [[0, 30, 60], [0, 1, 59, 60], [0, 20, 20, 45, 60]])
def test_row_shards(cuts, form):
    case = _tier_case(SEED_SHARDS)
    for port, allow_self in ((None, True), (QUERIES[0], False)):
        parts = []
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            r = _connect(case, port=port, allow_self=allow_self, rows=(r0, r1), form=form)
            parts.append(_rows(r.allowed, r0, r1))
            assert np.array_equal(r.egress_isolated, case[6])
            assert np.array_equal(r.ingress_isolated, case[7])
        assert np.array_equal(np.concatenate(parts, axis=0), _tref(case, port, allow_self))


def _loaded(bits):
    """A rows-only matrix holding the oracle's bits."""
    from kano import k8s
    from kano._engine import DeviceBuild
    n = bits.shape[0]
    e = DeviceBuild.empty(n)
    e.put_rows(0, _pack(bits))
    return k8s._wrap(e, n)


@pytest.mark.gpu
def test_allowed_feeds_the_queries():
    from kano import algorithm as alg
    from kano.model import Container
    case = _tier_case(SEED_QUERIES)
    pods = case[0]
    n = len(pods)
    port = QUERIES[0]
    r = _connect(case)
    rp = r.on_port(port)
    ref, refp = _loaded(_tref(case, None, True)), _loaded(_tref(case, port, True))
    pairs = [(i, (7 * i + 3) % n) for i in range(n)]
    assert np.array_equal(alg.hop_distance(r.allowed, pairs), alg.hop_distance(ref, pairs))
    assert np.array_equal(alg.hop_distance(rp.allowed, pairs), alg.hop_distance(refp, pairs))
    cs = [Container(p.name, dict(p.labels)) for p in pods]
    intents = [({"app": "web"}, {"app": "db"}, "deny"), ({"app": "api"}, {"tier": "be"}, "allow"),
               (range(0, 20), range(20, 60), "deny")]
    got, want = alg.check_intents(rp.allowed, cs, intents), alg.check_intents(refp, cs, intents)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert not got.ok.all()


@pytest.mark.gpu
def test_explain():
    cl = _known_tiers()
    r = _connect(cl)
    X, Y, base = "X", "Y", "base"
    # mon -> web(shop): the baseline allows mon's egress, X admits mon (admin Allow)
    x = r.explain(3, 0)
    assert x["allowed"] and not x["self"] and x["blocked_by"] == []
    assert x["egress"] == {"isolated": False, "policies": [], "tier": "baseline",
                           "verdict": "allow", "decider": ("baseline", base, 0, 0, "Allow")}
    assert x["ingress"] == {"isolated": True, "policies": [], "tier": "admin",
                            "verdict": "allow", "decider": ("admin", X, 0, 0, "Allow")}
    # web(shop) -> mon: X's Deny on egress, whatever D's rule allows; C isolates
    # mon's ingress with no rule
    x = r.explain(0, 3)
    assert not x["allowed"] and x["blocked_by"] == ["egress", "ingress"]
    assert x["egress"] == {"isolated": True, "policies": [("D", 0, 0)], "tier": "admin",
                           "verdict": "deny", "decider": ("admin", X, 1, 0, "Deny")}
    assert x["ingress"] == {"isolated": True, "policies": [], "tier": "network",
                            "verdict": "deny", "decider": None}
    # api -> db: X passes it on to B; A's first rule admits it (no admin match)
    x = r.explain(1, 2)
    assert x["allowed"] and x["blocked_by"] == []
    assert x["egress"] == {"isolated": True, "policies": [("B", 0, 0)], "tier": "network",
                           "verdict": "allow", "decider": ("network", "B", 0, 0, "Allow"),
                           "passed": ("admin", X, 0, 0, "Pass")}
    assert x["ingress"] == {"isolated": True, "policies": [("A", 0, 0)], "tier": "network",
                            "verdict": "allow", "decider": ("network", "A", 0, 0, "Allow")}
    # db -> db: passed, then nothing isolates db's egress and no baseline rule: default
    x = r.explain(2, 2)
    assert x["allowed"] and x["self"] and x["blocked_by"] == ["ingress"]
    assert x["egress"] == {"isolated": False, "policies": [], "tier": "default",
                           "verdict": "allow", "decider": None,
                           "passed": ("admin", X, 0, 0, "Pass")}
    # db -> web(shop): no rule at all on egress
    assert r.explain(2, 0)["egress"] == {"isolated": False, "policies": [], "tier": "default",
                                         "verdict": "allow", "decider": None}
    # mon -> db: the baseline's Deny
    x = r.explain(3, 2)
    assert not x["allowed"] and x["blocked_by"] == ["egress"]
    assert x["egress"]["tier"] == "baseline" and x["egress"]["verdict"] == "deny"
    assert x["egress"]["decider"] == ("baseline", base, 1, 0, "Deny")
    assert x["ingress"]["decider"] == ("admin", X, 0, 0, "Allow")
    # web(ops) -> job: Y's Allow
    assert r.explain(5, 4)["egress"]["decider"] == ("admin", Y, 0, 0, "Allow")
    # job -> web(ops): Y's Deny on ingress
    assert r.explain(4, 5)["ingress"]["decider"] == ("admin", Y, 0, 0, "Deny")
    # on TCP 80 X's ingress Allow does not count: web(shop)'s ingress falls to D
    x = r.on_port(("TCP", 80)).explain(3, 0)
    assert not x["allowed"] and x["blocked_by"] == ["ingress"]
    assert x["ingress"] == {"isolated": True, "policies": [], "tier": "network",
                            "verdict": "deny", "decider": None}
    with pytest.raises(IndexError):
        r.explain(0, 6)
    # every pair of two queries: explain agrees with the matrix
    for port in (None, ("TCP", 9050)):
        rp, want = r.on_port(port), _bits_of(KNOWN_TIERS[(port, True)])
        for s in range(6):
            for d in range(6):
                x = rp.explain(s, d)
                assert x["allowed"] == bool(want[s, d]), (port, s, d)
                assert x["blocked_by"] == [k for k in ("egress", "ingress")
                                           if x[k]["verdict"] == "deny"]


@pytest.mark.gpu
def test_abi_errors_leave_the_contexts_usable():
    from kano import _native as nat, k8s
    from kano._engine import DeviceBuild
    from kano._intern import intern
    case = _tier_case(SEED_ABI)
    pods, pols, nss, admin, baseline = case[:5]
    n = len(pods)
    c = k8s.compile_conformant(pods, pols, nss, admin, baseline)
    lib = nat.load()

    def operand(entries, rows=None):
        b = DeviceBuild(intern(c.containers, entries), rows=rows, build=False)
        b.build_classes()
        return b

    eg, ing = operand(c.egress), operand(c.ingress)
    dst = DeviceBuild.empty(n)
    code_e, code_i = c.codes(None)
    npe, npi = c.np_level

    def call(e, i, d, ce=code_e, ci=code_i, ne=None, ni=None, npe=npe, npi=npi):
        ce, ci = np.ascontiguousarray(ce, np.uint32), np.ascontiguousarray(ci, np.uint32)
        return lib.kano_k8s_conn_tiers(
            e and e.ctx, i and i.ctx, d and d.ctx, 1, len(ce) if ne is None else ne,
            ce.ctypes.data, npe, len(ci) if ni is None else ni, ci.ctypes.data, npi, None, None,
            None)

    def good():
        assert call(eg, ing, dst) == 0
        assert np.array_equal(_unpack(dst.rows(0, n), n), _tref(case, None, True))

    def with_code(code, value):
        out = code.copy()
        out[0] = value
        return out

    good()
    assert npe >= 1 and npi >= 1
    bad = [(npe * 4 + 2, "passes"), ((npe + 1) * 4 + 2, "passes"), (3, "isolates"),
           ((npe + 2) * 4 + 3, "isolates"), (npe * 4 + 1, "denies")]
    for value, word in bad:
        assert call(eg, ing, dst, ce=with_code(code_e, value)) == -errno.EINVAL, value
        assert word.encode() in lib.kano_last_error(dst.ctx) and b"egress" in \
            lib.kano_last_error(dst.ctx)
        good()
    assert call(eg, ing, dst, ci=with_code(code_i, npi * 4 + 1)) == -errno.EINVAL
    assert b"ingress" in lib.kano_last_error(dst.ctx)
    # no level reaches 2^30: np_level is below it and the levels above it are
    # 30-bit fields of the code
    assert call(eg, ing, dst, npe=1 << 30) == -errno.EINVAL
    assert b"2^30" in lib.kano_last_error(dst.ctx)
    assert call(eg, ing, dst, npi=(1 << 30) + 5) == -errno.EINVAL
    good()
    assert call(eg, ing, dst, ne=len(code_e) + 1) == -errno.EINVAL
    assert call(eg, ing, dst, ni=len(code_i) - 1) == -errno.EINVAL
    assert b"nids" in lib.kano_last_error(dst.ctx)
    assert call(None, ing, dst) == -errno.EINVAL
    assert call(eg, ing, None) == -errno.EINVAL
    assert call(eg, ing, eg) == -errno.EINVAL
    assert call(eg, ing, DeviceBuild.empty(n - 1)) == -errno.EINVAL
    good()
    shard = operand(c.egress, rows=(0, n // 2))
    assert call(shard, ing, dst) == -errno.ENOTSUP
    assert b"row shard" in lib.kano_last_error(dst.ctx)
    assert call(eg, shard, dst, ci=code_e) == -errno.ENOTSUP
    good()
    # a dropped entry may carry any bits; the sources still answer, and another
    # query on the same contexts is right
    iso_e, iso_i, info = dst.k8s_conn_tiers_from(eg, ing, False, *[
        x for pair in zip(c.codes(QUERIES[1]), c.np_level) for x in pair])
    assert np.array_equal(_unpack(dst.rows(0, n), n), _tref(case, QUERIES[1], False))
    assert np.array_equal(iso_e, case[6]) and np.array_equal(iso_i, case[7])
    assert info["egress_isolated"] == int(case[6].sum())
    assert info["egress_entries"] == int((c.codes(QUERIES[1])[0] != 0xFFFFFFFF).sum())
