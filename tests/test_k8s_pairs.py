"""K8sConnectivity.pair_verdicts: which tier and which rule decide each pod
pair under k8s.connectivity, for many pairs a call (kano_k8s_pair_verdicts).

The naming oracle below restates the three tiers per pair straight from the
manifest dicts -- it calls neither compile_conformant nor any kano code -- and
names, per direction, the deciding (kind, policy, rule, peer, action) and the
Pass rule that handed the pair down.  Within a tier the decider is the first
(policy, rule, peer) in evaluation order that counts on the port and matches
the pair: what "the smallest engine id at the winning code" means in manifest
terms.  On the CPU it is pinned against test_k8s_tiers' oracle, against a
numpy resolution of compile_conformant's entries by (code, id), and against a
table for the six-pod cluster worked out by hand."""
import errno
import functools

import numpy as np
import pytest

from test_k8s_conn import (QUERIES, _bits_of, _case, _counts, _ref, _rows, _sel,
                           oracle as np_oracle)
from test_k8s_tiers import (KNOWN_TIERS, SEED_130, SEED_1030, SEED_ABI, SEEDS_40, SEEDS_60,
                            T_ADMIN_ALLOW, T_ADMIN_DENY, T_BASE_ALLOW, T_BASE_DENY, T_DEFAULT,
                            T_NETWORK, _anp_counts, _anp_selects, _known_tiers, _tier_case, _tref,
                            tier_oracle)

TIERS = ("default", "admin", "network", "baseline")
DIRECTIONS = (("Egress", "egress", "to"), ("Ingress", "ingress", "from"))
PORTS = [None] + QUERIES


# ---------------------------------------------------------------------------
# the naming oracle
# ---------------------------------------------------------------------------
def _structure(pods, pols, nss, admin, baseline):
    """The rules of each direction in evaluation order with their pod masks
    (nothing here depends on the port): per tier a list of (kind, policy name,
    rule index, action, ports, subject mask, [(peer index, peer mask)]), and
    the isolated pods."""
    nsl = {ns.name: ns.labels for ns in nss}
    n = len(pods)
    mask = lambda f: np.array([bool(f(p)) for p in pods], dtype=bool).reshape(n)   # noqa: E731

    def anp_rules(kind, pol, key, side):
        subj = mask(lambda p: _anp_selects(pol.spec["subject"], p, nsl))
        return [(kind, pol.name, ri, rule["action"], rule.get("ports"), subj,
                 [(pj, mask(lambda p, pe=pe: _anp_selects(pe, p, nsl)))
                  for pj, pe in enumerate(rule[side])])
                for ri, rule in enumerate(pol.spec.get(key) or [])]

    out = {}
    for typ, key, side in DIRECTIONS:
        adm = []
        for q in sorted(range(len(admin)), key=lambda q: (admin[q].spec["priority"], q)):
            adm += anp_rules("admin", admin[q], key, side)
        net, iso = [], np.zeros(n, bool)
        for pol in pols:
            spec = pol.spec or {}
            types = spec.get("policyTypes")
            if types is None:
                types = ["Ingress"] + (["Egress"] if "egress" in spec else [])
            if typ not in types:
                continue
            sel = mask(lambda p: p.namespace == pol.namespace
                       and _sel(spec.get("podSelector"), p.labels))
            iso |= sel
            for ri, rule in enumerate(spec.get(key) or []):
                rule = rule or {}
                peers = []
                if not rule.get(side):
                    peers.append((None, np.ones(n, bool)))
                for pj, peer in enumerate(rule.get(side) or []):
                    peer = peer or {}
                    if peer.get("ipBlock") is not None:
                        continue
                    nsel, psel = peer.get("namespaceSelector"), peer.get("podSelector")
                    peers.append((pj, mask(
                        lambda p: (p.namespace == pol.namespace if nsel is None
                                   else _sel(nsel, nsl[p.namespace]))
                        and (psel is None or _sel(psel, p.labels)))))
                net.append(("network", pol.name, ri, "Allow", rule.get("ports"), sel, peers))
        base = anp_rules("baseline", baseline, key, side) if baseline is not None else []
        out[key] = (adm, net, base, iso)
    return out


class Named:
    """The naming oracle's answer for one port: per direction tier[x, y]
    (an index into TIERS), deny[x, y], decider[x, y] and passed[x, y] (indices
    into ``names``, -1: none; x the subject, y the peer)."""

    def __init__(self, structure, n, port):
        self.n, self.names, self._index = n, [], {}
        for key, (adm, net, base, iso) in structure.items():
            tier = np.zeros((n, n), np.uint8)
            deny = np.zeros((n, n), bool)
            dec, pas = np.full((n, n), -1, np.int32), np.full((n, n), -1, np.int32)
            open_, passed = np.ones((n, n), bool), np.zeros((n, n), bool)
            for kind, name, ri, action, ports, subj, peers in adm:       # 1: the admin tier
                if not _anp_counts(ports, port):
                    continue
                for pj, pm in peers:
                    m = subj[:, None] & pm[None, :] & open_
                    k = self._id((kind, name, ri, pj, action))
                    if action == "Pass":
                        pas[m] = k
                        passed |= m
                    else:
                        tier[m], deny[m], dec[m] = 1, action == "Deny", k
                    open_ &= ~m
            rest = open_ | passed
            mi = rest & iso[:, None]                                     # 2: the NetworkPolicies
            tier[mi], deny[mi] = 2, True
            for kind, name, ri, action, ports, sel, peers in net:
                if not _counts(ports, port):
                    continue
                for pj, pm in peers:
                    m = sel[:, None] & pm[None, :] & mi & deny
                    dec[m], deny[m] = self._id((kind, name, ri, pj, action)), False
            b = rest & ~iso[:, None]                                     # 3: the baseline
            for kind, name, ri, action, ports, subj, peers in base:
                if not _anp_counts(ports, port):
                    continue
                for pj, pm in peers:
                    m = subj[:, None] & pm[None, :] & b
                    tier[m], deny[m], dec[m] = 3, action == "Deny", self._id(
                        (kind, name, ri, pj, action))
                    b &= ~m
            for a in (tier, deny, dec, pas):
                a.setflags(write=False)
            setattr(self, key, (tier, deny, dec, pas))

    def _id(self, name):
        if name not in self._index:
            self._index[name] = len(self.names)
            self.names.append(name)
        return self._index[name]

    def allowed(self, allow_self):
        a = ~self.egress[1] & ~self.ingress[1].T
        return a | np.eye(self.n, dtype=bool) if allow_self else a

    def name(self, direction, x, y, what="decider"):
        k = int(getattr(self, direction)[2 if what == "decider" else 3][x, y])
        return None if k < 0 else self.names[k]


class Cluster:
    """A cluster with its naming oracle per port, computed once."""

    def __init__(self, pods, pols, nss, admin=(), baseline=None):
        self.objects = (pods, pols, nss, list(admin), baseline)
        self.n = len(pods)
        self._structure = _structure(*self.objects)
        self._named = {}

    def named(self, port) -> Named:
        if port not in self._named:
            self._named[port] = Named(self._structure, self.n, port)
        return self._named[port]


@functools.lru_cache(maxsize=None)
def _tiered(seed, **kw):
    """(the keywords as test_k8s_tiers passes them: one cached case for both files)"""
    return Cluster(*_tier_case(seed, **kw)[:5])


@functools.lru_cache(maxsize=None)
def _known_cluster():
    return Cluster(*_known_tiers())


# ---------------------------------------------------------------------------
# the six-pod cluster by hand (test_k8s_tiers._known_tiers and the comment
# above its KNOWN_TIERS).  Per direction and port a row per subject x and a
# token per peer y:
#   .     default allow            -     the NetworkPolicy tier denies (no rule)
#   NAME  the rule that decides    P>..  passed down by Pass rule P first
# Egress rules: X0 Pass {p0,p1,p2} -> p2, X1 Deny {p0,p1,p2} -> ops (TCP 80 only),
# Y0 Allow {p0,p5} -> ops; B allows p1 -> p2, D allows p0 -> anyone (UDP 53 only);
# baseline b0 Allow ops -> p0, p1, b1 Deny ops -> anyone.  Ingress rules: X0
# Allow {p0,p1,p2} <- p3 (TCP 9000-9100 only), Y0 Deny {p0,p5} <- p4; A0 allows
# p2 <- p1 (TCP 5432 only), A1 p2 <- p3 (9000-9100 only); C isolates the ops
# pods and D isolates p0 with no ingress rule.  port=None counts every rule.
# ---------------------------------------------------------------------------
KNOWN_RULES = {
    "egress": {"X0": ("admin", "X", 0, 0, "Pass"), "X1": ("admin", "X", 1, 0, "Deny"),
               "Y0": ("admin", "Y", 0, 0, "Allow"), "B": ("network", "B", 0, 0, "Allow"),
               "D": ("network", "D", 0, 0, "Allow"), "b0": ("baseline", "base", 0, 0, "Allow"),
               "b1": ("baseline", "base", 1, 0, "Deny")},
    "ingress": {"X0": ("admin", "X", 0, 0, "Allow"), "Y0": ("admin", "Y", 0, 0, "Deny"),
                "A0": ("network", "A", 0, 0, "Allow"), "A1": ("network", "A", 1, 0, "Allow")},
}
_OPS_E = ["b0 b0 b1 b1 b1 b1", "b0 b0 b1 b1 b1 b1", "b0 b0 b1 Y0 Y0 Y0"]     # p3, p4, p5
_OPS_I = ["- - - - - -", "- - - - - -", "- - - - Y0 -"]
KNOWN_VERDICTS = {
    None: {
        "egress": ["D D X0>D X1 X1 X1", "- - X0>B X1 X1 X1", ". . X0>. X1 X1 X1"] + _OPS_E,
        "ingress": ["- - - X0 Y0 -", ". . . X0 . .", "- A0 - X0 - -"] + _OPS_I},
    ("TCP", 80): {
        "egress": ["- - X0>- X1 X1 X1", "- - X0>B X1 X1 X1", ". . X0>. X1 X1 X1"] + _OPS_E,
        "ingress": ["- - - - Y0 -", ". . . . . .", "- - - - - -"] + _OPS_I},
    ("TCP", 9050): {
        "egress": ["- - X0>- Y0 Y0 Y0", "- - X0>B - - -", ". . X0>. . . ."] + _OPS_E,
        "ingress": ["- - - X0 Y0 -", ". . . X0 . .", "- - - X0 - -"] + _OPS_I},
}


def _known_answer(port, direction, x, y):
    """(tier name, deny, decider, passed) of the hand table."""
    rules = KNOWN_RULES[direction]
    token = KNOWN_VERDICTS[port][direction][x].split()[y]
    passed = None
    if ">" in token:
        p, token = token.split(">")
        passed = rules[p]
    if token == ".":
        return "default", False, None, passed
    if token == "-":
        return "network", True, None, passed
    name = rules[token]
    return name[0], name[4] == "Deny", name, passed


def _known_allowed(port, allow_self):
    a = np.array([[not _known_answer(port, "egress", s, d)[1]
                   and not _known_answer(port, "ingress", d, s)[1] for d in range(6)]
                  for s in range(6)])
    return a | np.eye(6, dtype=bool) if allow_self else a


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------
def test_known_table_matches_the_known_matrices():
    for (port, allow_self), rows in KNOWN_TIERS.items():
        assert np.array_equal(_known_allowed(port, allow_self), _bits_of(rows)), (port, allow_self)
    for port in KNOWN_VERDICTS:        # a Pass rule never decides, a decider never passes
        for direction in ("egress", "ingress"):
            for x in range(6):
                for y in range(6):
                    tier, deny, decider, passed = _known_answer(port, direction, x, y)
                    assert decider is None or decider[4] != "Pass"
                    assert passed is None or passed[4] == "Pass"


def test_known_answers_naming_oracle():
    cl = _known_cluster()
    for port in KNOWN_VERDICTS:
        o = cl.named(port)
        for direction in ("egress", "ingress"):
            tier, deny = getattr(o, direction)[:2]
            for x in range(6):
                for y in range(6):
                    want = _known_answer(port, direction, x, y)
                    got = (TIERS[tier[x, y]], bool(deny[x, y]), o.name(direction, x, y),
                           o.name(direction, x, y, "passed"))
                    assert got == want, (port, direction, x, y)
    # the issue's examples, spelled out (port=None)
    o = cl.named(None)
    assert o.name("egress", 0, 3) == ("admin", "X", 1, 0, "Deny")
    assert o.name("egress", 1, 2, "passed") == ("admin", "X", 0, 0, "Pass")
    assert o.name("egress", 1, 2) == ("network", "B", 0, 0, "Allow")
    assert o.name("egress", 3, 2) == ("baseline", "base", 1, 0, "Deny")
    assert TIERS[o.egress[0][2, 0]] == "default" and o.name("egress", 2, 0) is None
    assert o.name("ingress", 0, 3) == ("admin", "X", 0, 0, "Allow")
    assert o.name("ingress", 0, 4) == ("admin", "Y", 0, 0, "Deny")


WHO = {(1, False): T_ADMIN_ALLOW, (1, True): T_ADMIN_DENY, (2, False): T_NETWORK,
       (2, True): T_NETWORK, (3, False): T_BASE_ALLOW, (3, True): T_BASE_DENY,
       (0, False): T_DEFAULT}


def _check_against_tier_oracle(cl, port):
    o = cl.named(port)
    want, isoE, isoI, who, passed = tier_oracle(*cl.objects, port, True)
    assert np.array_equal(o.allowed(True), want), port
    for direction in ("egress", "ingress"):
        tier, deny, dec, pas = getattr(o, direction)
        code = np.zeros(tier.shape, np.int8)
        for (t, d), w in WHO.items():
            code[(tier == t) & (deny == d)] = w
        assert code.all() and np.array_equal(code, who[direction]), (port, direction)
        assert np.array_equal(pas >= 0, passed[direction]), (port, direction)
        # a decider exists exactly where a rule decides
        assert np.array_equal(dec >= 0, (tier == 1) | (tier == 3) | ((tier == 2) & ~deny))


def test_naming_oracle_matches_tier_oracle_known():
    for port in KNOWN_VERDICTS:
        _check_against_tier_oracle(_known_cluster(), port)


@functools.lru_cache(maxsize=None)
def _compiled(cl):
    """compile_conformant's entries with their select / allow sets from the
    kano restatement (oracle ref_py), as _compiled_tiers reads them."""
    from kano import k8s
    from oracle import kano_oracle as orc
    pods, pols, nss, admin, baseline = cl.objects
    n = cl.n
    c = k8s.compile_conformant(pods, pols, nss, admin, baseline)
    sets = []
    for entries in (c.egress, c.ingress):
        r = orc.ref_py(c.containers, entries)
        sets.append(tuple(np.array([[ch == "1" for ch in s] for s in r[k]],
                                   dtype=bool).reshape(-1, n) for k in ("sel", "allow")))
    by_kind = {"admin": admin, "network": pols, "baseline": [baseline]}
    return c, sets, by_kind


def _check_against_compiled(cl, port):
    """The entries resolved by code in numpy: per pair the smallest (code, id)
    among the live matching entries below, at and above np_level."""
    c, sets, by_kind = _compiled(cl)
    n, o = cl.n, cl.named(port)
    codes = c.codes(port)
    for k, direction in enumerate(("egress", "ingress")):
        code, np_level = codes[k].astype(np.int64), c.np_level[k]
        sel, alw = sets[k]
        org = (c.origin_egress, c.origin_ingress)[k]
        tiers = (c.tiers_egress, c.tiers_ingress)[k]
        a, m, b = (np.full((n, n), -1, np.int32) for _ in range(3))
        iso = np.zeros(n, bool)
        live = [p for p in range(len(code)) if code[p] != 0xFFFFFFFF]
        for p in sorted(live, key=lambda p: (code[p], p), reverse=True):   # the smallest last
            hit = sel[p][:, None] & alw[p][None, :]
            lv = code[p] >> 2
            if lv == np_level:
                iso |= sel[p]
            if lv < np_level:
                a[hit] = p
            elif lv > np_level:
                b[hit] = p
            elif code[p] == np_level * 4:
                m[hit] = p
        act = lambda ids: np.where(ids >= 0, code[np.maximum(ids, 0)] & 3, -1)   # noqa: E731
        admin_decides = (a >= 0) & (act(a) != 2)
        network = ~admin_decides & iso[:, None]
        base = ~admin_decides & ~network & (b >= 0)
        tier = np.select([admin_decides, network, base], [1, 2, 3], 0)
        deny = np.select([admin_decides, network, base], [act(a) == 1, m < 0, act(b) == 1], False)
        dec = np.select([admin_decides, network, base], [a, m, b], -1)
        pas = np.where((a >= 0) & (act(a) == 2), a, -1)

        def named(ids):
            """the entries' names as indices into the naming oracle's"""
            to = np.array([o._index.get((tiers[p][0], by_kind[tiers[p][0]][org[p][0]].name,
                                         org[p][2], org[p][3], tiers[p][2]), -2)
                           for p in range(len(code))] + [-1], dtype=np.int32)
            return to[ids]

        ot, od, odec, opas = getattr(o, direction)
        assert np.array_equal(tier, ot), (port, direction)
        assert np.array_equal(deny, od), (port, direction)
        assert np.array_equal(named(dec), odec), (port, direction)
        assert np.array_equal(named(pas), opas), (port, direction)


def test_naming_oracle_matches_compiled_known():
    for port in KNOWN_VERDICTS:
        _check_against_compiled(_known_cluster(), port)


@pytest.mark.parametrize("seed", SEEDS_40)
def test_naming_oracle_matches_both(seed):
    cl = _tiered(seed, n=40, P=14)
    for port in (None, ("TCP", 80), ("TCP", 9050)):
        _check_against_tier_oracle(cl, port)
        _check_against_compiled(cl, port)


def _unconnected(cl):
    """A K8sConnectivity without device builds: pair_verdicts checks its pairs
    before it reaches them."""
    from kano import k8s
    pods, pols, nss, admin, baseline = cl.objects
    c = k8s.compile_conformant(pods, pols, nss, admin, baseline)
    return k8s.K8sConnectivity(None, None, None, c, {}, None, True, {}, (None, None), 0, None)


def test_host_errors():
    r = _unconnected(_known_cluster())
    for bad in ([1, 2, 3], [[1, 2, 3]], np.zeros((2, 2, 2), np.int32), [(0, 1), (2,)]):
        with pytest.raises(ValueError):
            r.pair_verdicts(bad)
    for bad in ([[0.0, 1.0]], np.zeros((3, 2), np.float32), [("a", "b")], [(True, False)]):
        with pytest.raises(TypeError):
            r.pair_verdicts(bad)
    for bad in ([(0, 6)], [(6, 0)], [(0, 1), (-1, 2)], [(0, 2 ** 31)], [(-2 ** 40, 0)],
                np.array([[0, 1], [5, 6]], np.int64)):
        with pytest.raises(IndexError):
            r.pair_verdicts(bad)


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------
def _connect(cl, **kw):
    from kano import k8s
    pods, pols, nss, admin, baseline = cl.objects
    return k8s.connectivity(pods, pols, nss, admin=admin, baseline=baseline, **kw)


def _all_pairs(n, seed=0):
    """Every (s, d), shuffled."""
    pr = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2)
    return np.random.default_rng(seed).permutation(pr).astype(np.int32)


def _want_counts(o, pr, allow_self):
    s, d = pr[:, 0], pr[:, 1]
    self_ = (s == d) & allow_self
    want = {"allowed": int((o.allowed(allow_self)[s, d]).sum()), "self": int(self_.sum())}
    for direction, (x, y) in (("egress", (s, d)), ("ingress", (d, s))):
        tier, deny = getattr(o, direction)[:2]
        for t, tn in enumerate(TIERS):
            for v, vn in ((False, "allow"), (True, "deny")):
                want[f"{direction}_{tn}_{vn}"] = int(((tier[x, y] == t) & (deny[x, y] == v)).sum())
    return want


def _check_verdicts(cl, conn, pr, r, names=60):
    """Everything pair_verdicts returns for the pairs pr against the naming
    oracle of conn's port; ``names``: how many pairs also go through name() /
    passed_name() / blocked_by() (the arrays are compared for all)."""
    o = cl.named(conn.port)
    pr = np.asarray(pr, np.int32).reshape(-1, 2)
    s, d = pr[:, 0], pr[:, 1]
    assert np.array_equal(r.pairs, pr) and len(r) == len(pr)
    assert r.allowed.dtype == bool and np.array_equal(r.allowed, o.allowed(conn.allow_self)[s, d])
    assert np.array_equal(r.self_, (s == d) & conn.allow_self)
    for direction, (x, y) in (("egress", (s, d)), ("ingress", (d, s))):
        got = getattr(r, direction)
        tier, deny, dec, pas = getattr(o, direction)
        assert np.array_equal(got.tier, tier[x, y]), direction
        assert np.array_equal(got.deny, deny[x, y]), direction
        # engine ids -> the oracle's names, compared for every pair at once
        P = len(getattr(conn, "origin_" + direction))
        to = np.array([o._index.get(got.entry(p), -2) for p in range(P)] + [-1], np.int32)
        assert got.decider.dtype == np.int32 and got.decider.min(initial=0) >= -1
        assert got.decider.max(initial=-1) < P and got.passed.max(initial=-1) < P
        assert np.array_equal(to[got.decider], dec[x, y]), direction
        assert np.array_equal(to[got.passed], pas[x, y]), direction
        for q in range(0, len(pr), max(1, len(pr) // names)):
            assert r.name(direction, q) == o.name(direction, x[q], y[q]), (direction, q)
            assert r.passed_name(direction, q) == o.name(direction, x[q], y[q], "passed")
            assert (direction in r.blocked_by(q)) == bool(deny[x[q], y[q]])
    assert r.counts == _want_counts(o, pr, conn.allow_self)
    assert sum(v for k, v in r.counts.items() if k.startswith("egress")) == len(pr)


def _check_explain(conn, pr, r, sample):
    for q in sample:
        x = conn.explain(int(pr[q, 0]), int(pr[q, 1]))
        assert x["allowed"] == bool(r.allowed[q]) and x["self"] == bool(r.self_[q])
        assert x["blocked_by"] == r.blocked_by(q)
        for direction in ("egress", "ingress"):
            got, e = getattr(r, direction), x[direction]
            if "tier" in e:
                assert e["tier"] == TIERS[got.tier[q]] == got.tier_name(q)
                assert e["verdict"] == ("deny" if got.deny[q] else "allow")
                assert e["decider"] == r.name(direction, q)
                assert e.get("passed") == r.passed_name(direction, q)
            else:                      # the untiered explain: the allowing rules, in id order
                assert TIERS[got.tier[q]] == ("network" if e["isolated"] else "default")
                assert bool(got.deny[q]) == (e["isolated"] and not e["policies"])
                name = r.name(direction, q)
                assert (name[1:4] if name else None) == (e["policies"][0] if e["policies"]
                                                         and e["isolated"] else None)


@pytest.mark.gpu
@pytest.mark.parametrize("allow_self", [True, False])
def test_known_cluster(allow_self):
    cl = _known_cluster()
    base = _connect(cl, allow_self=allow_self)
    pr = _all_pairs(6)
    for port in KNOWN_VERDICTS:
        conn = base.on_port(port)
        r = conn.pair_verdicts(pr)
        for q, (s, d) in enumerate(pr.tolist()):
            for direction, (x, y) in (("egress", (s, d)), ("ingress", (d, s))):
                got = getattr(r, direction)
                want = _known_answer(port, direction, x, y)
                assert (TIERS[got.tier[q]], bool(got.deny[q]), r.name(direction, q),
                        r.passed_name(direction, q)) == want, (port, direction, x, y)
        assert np.array_equal(r.allowed, _known_allowed(port, allow_self)[pr[:, 0], pr[:, 1]])
        _check_verdicts(cl, conn, pr, r)
    # blame: the rules that deny, and all deciding rules (port=None, egress)
    r = base.pair_verdicts(pr)
    assert r.blame("egress") == {("admin", "X", 1): 9, ("baseline", "base", 1): 9}
    assert r.blame("egress", deny_only=False) == {
        ("admin", "X", 1): 9, ("admin", "Y", 0): 3, ("network", "D", 0): 3, ("network", "B", 0): 1,
        ("baseline", "base", 0): 6, ("baseline", "base", 1): 9}
    assert r.blame("ingress") == {("admin", "Y", 0): 2}
    with pytest.raises(ValueError):
        r.blame("sideways")
    with pytest.raises(IndexError):
        r.name("egress", 36)


@pytest.mark.gpu
@pytest.mark.parametrize("allow_self", [True, False])
@pytest.mark.parametrize("seed", SEEDS_60)
def test_matches_naming_oracle(seed, allow_self):
    cl = _tiered(seed)
    case = _tier_case(seed)
    n = cl.n
    pr = _all_pairs(n, seed)
    base = _connect(cl, allow_self=allow_self)
    for k, port in enumerate(PORTS):
        conn = base.on_port(port)
        r = conn.pair_verdicts(pr)
        _check_verdicts(cl, conn, pr, r)
        # the oracle's matrix, and the bits the existing kernel wrote
        assert np.array_equal(r.allowed, _tref(case, port, allow_self)[pr[:, 0], pr[:, 1]])
        assert np.array_equal(r.allowed, _rows(conn.allowed)[pr[:, 0], pr[:, 1]])
        if k == seed % len(PORTS):
            _check_explain(conn, pr, r, range(0, len(pr), len(pr) // 20))


SHAPES = ["kpf=1,kpgrid=1", "kpf=1,kpgrid=2", "kpf=2,kpgrid=1", "kpf=2,kpgrid=2"]


@pytest.mark.gpu
@pytest.mark.parametrize("tune", SHAPES)
def test_forms_and_grid_caps(tune, monkeypatch):
    """The lane and the wave form, each forced, under grid caps of 1 and 2
    blocks: 3600 pairs take many grid-stride turns (lane: 256 or 512 pairs a
    turn) and long wave runs (900 or 450 pairs a wave)."""
    monkeypatch.setenv("KANO_TUNE", tune)
    cl = _tiered(SEEDS_60[0])
    n = cl.n
    conn = _connect(cl, allow_self=False).on_port(QUERIES[0])
    pr = _all_pairs(n, 3)
    _check_verdicts(cl, conn, pr, conn.pair_verdicts(pr))
    for Q in (1, 65):
        _check_verdicts(cl, conn, pr[:Q], conn.pair_verdicts(pr[:Q]))
    # duplicates and (s, s) pairs without allow_self: resolved like any pair
    dup = np.concatenate([pr[:7]] * 5 + [np.stack([np.arange(n)] * 2, 1).astype(np.int32)])
    r = conn.pair_verdicts(dup)
    _check_verdicts(cl, conn, dup, r)
    assert not r.self_.any()
    for k in range(1, 5):
        assert np.array_equal(r.egress.decider[:7], r.egress.decider[7 * k:7 * k + 7])


@pytest.mark.gpu
@pytest.mark.parametrize("tune", ["kpf=1", "kpf=2"])
def test_more_than_64_classes(tune, monkeypatch):
    """n = 130 with every pod its own row and column class on both sides: the
    hit reads the AC words past the first (three words a row)."""
    monkeypatch.setenv("KANO_TUNE", tune)
    n = 130
    cl = _tiered(SEED_130, n=n, P=20, nns=4, uid=True)
    conn = _connect(cl)
    for b in (conn.egress, conn.ingress):
        info = b.engine.info()
        assert info["U"] == n and info["UA"] == n
    pr = _all_pairs(n, 1)
    for port in (None, QUERIES[0]):
        c = conn.on_port(port)
        _check_verdicts(cl, c, pr, c.pair_verdicts(pr))


@pytest.mark.gpu
def test_1030_pods():
    n = 1030
    cl = _tiered(SEED_1030, n=n, P=30, nns=4)
    conn = _connect(cl)
    pr = _all_pairs(n, 2)
    r = conn.pair_verdicts(pr)
    _check_verdicts(cl, conn, pr, r)
    assert np.array_equal(r.allowed, _rows(conn.allowed)[pr[:, 0], pr[:, 1]])


def _long_list_cluster():
    """70 pods of one namespace, each with its own "id"; three
    AdminNetworkPolicies of 50 egress rules with one single-pod peer each,
    subject every pod: every pod's egress list starts with 150 admin entries
    over 150 levels, entry k at position k (a wave strides it three times).
    Rule k names pod 10 + k % 50, except rule 0 (pod 1), rule 64 (pod 2) and
    rule 149 (pod 3); the baseline's one rule (pod 4) is every list's last
    entry.  The d pods' egress is isolated by a NetworkPolicy."""
    from kano import k8s
    n = 70
    nss = [k8s.Namespace("a", {"team": "x"})]
    pods = [k8s.Pod(f"p{i}", "a", {"id": i, "app": "w" if i % 3 else "d"}) for i in range(n)]
    one = lambda i: {"pods": {"podSelector": {"matchLabels": {"id": i}}}}   # noqa: E731
    peer = {0: 1, 64: 2, 149: 3}
    action = {0: "Allow", 64: "Deny", 149: "Pass"}
    admin = []
    for q in range(3):
        rules = [{"action": action.get(k, ["Allow", "Deny", "Pass"][k % 3]),
                  "to": [one(peer.get(k, 10 + k % 50))]} for k in range(50 * q, 50 * q + 50)]
        admin.append(k8s.AdminNetworkPolicy(f"long{q}", {
            "priority": 10 * q, "subject": {"namespaces": {}}, "egress": rules}))
    pols = [k8s.NetworkPolicy("np", "a", {
        "podSelector": {"matchLabels": {"app": "d"}}, "policyTypes": ["Egress"],
        "egress": [{"to": [{"podSelector": {"matchLabels": {"app": "w"}}}]}]})]
    baseline = k8s.BaselineAdminNetworkPolicy("base", {
        "subject": {"namespaces": {}}, "egress": [{"action": "Deny", "to": [one(4)]}]})
    return Cluster(pods, pols, nss, admin, baseline)


@pytest.mark.gpu
@pytest.mark.parametrize("tune", ["kpf=1", "kpf=2,kpgrid=2"])
def test_long_subject_list(tune, monkeypatch):
    monkeypatch.setenv("KANO_TUNE", tune)
    cl = _long_list_cluster()
    n = cl.n
    o = cl.named(None)
    # the constructs decide as designed (on the oracle alone)
    assert o.name("egress", 7, 1) == ("admin", "long0", 0, 0, "Allow")
    assert o.name("egress", 7, 2) == ("admin", "long1", 14, 0, "Deny")
    assert o.name("egress", 7, 3, "passed") == ("admin", "long2", 49, 0, "Pass")
    assert TIERS[o.egress[0][7, 3]] == "default" and TIERS[o.egress[0][6, 3]] == "network"
    assert o.name("egress", 7, 4) == ("baseline", "base", 0, 0, "Deny")
    conn = _connect(cl, allow_self=False)
    assert conn._compiled.np_level[0] == 150
    pr = _all_pairs(n, 4)
    r = conn.pair_verdicts(pr)
    _check_verdicts(cl, conn, pr, r)
    # where the deciding (or passed) entries sit in the subject's list
    off, lst = conn.egress.engine.select_csr()
    cls = conn.egress.engine.classes()
    where = {(int(s), int(d)): q for q, (s, d) in enumerate(pr.tolist())}
    for x in (7, 6):                                     # a w pod, and an isolated d pod
        own = lst[off[cls[x]]:off[cls[x] + 1]].tolist()
        assert len(own) == (151 if x == 7 else 152) and own == sorted(own)
        at = lambda y, ids: own.index(int(ids[where[(x, y)]]))   # noqa: E731
        assert at(1, r.egress.decider) == 0
        assert at(2, r.egress.decider) == 64
        assert at(3, r.egress.passed) == 149
        if x == 7:
            assert at(4, r.egress.decider) == len(own) - 1
        else:                                            # isolated: the NetworkPolicy entry decides
            assert r.name("egress", where[(x, 4)]) == ("network", "np", 0, 0, "Allow")
            assert at(5, r.egress.decider) == 150


@pytest.mark.gpu
@pytest.mark.parametrize("allow_self", [True, False])
def test_untiered_connectivity(allow_self):
    """Without admin and baseline rules the tiers are network or default."""
    from kano import k8s
    seed = 5
    case = _case(seed)
    pods, pols, nss = case[:3]
    cl = Cluster(pods, pols, nss)
    n = cl.n
    base = k8s.connectivity(pods, pols, nss, allow_self=allow_self)
    pr = _all_pairs(n, 5)
    for port in PORTS:
        conn = base.on_port(port)
        r = conn.pair_verdicts(pr)
        _check_verdicts(cl, conn, pr, r)
        want, isoE, isoI = np_oracle(pods, pols, nss, port, allow_self)
        assert np.array_equal(want, _ref(case, port, allow_self))
        assert np.array_equal(r.allowed, want[pr[:, 0], pr[:, 1]])
        assert np.array_equal(r.allowed, _rows(conn.allowed)[pr[:, 0], pr[:, 1]])
        assert np.array_equal(r.egress.tier, np.where(isoE[pr[:, 0]], 2, 0))
        assert np.array_equal(r.ingress.tier, np.where(isoI[pr[:, 1]], 2, 0))
        assert (r.egress.passed == -1).all() and (r.ingress.passed == -1).all()
        assert all(v == 0 for k, v in r.counts.items() if "admin" in k or "baseline" in k)
        _check_explain(conn, pr, r, range(0, len(pr), len(pr) // 20))


@pytest.mark.gpu
def test_degenerate_inputs():
    from kano import k8s
    nss = [k8s.Namespace("a", {"team": "x"})]
    everyone = {"namespaces": {}}
    app = lambda v: {"pods": {"podSelector": {"matchLabels": {"app": v}}}}   # noqa: E731
    pods = [k8s.Pod(f"p{i}", "a", {"app": "w" if i % 3 else "d"}) for i in range(70)]
    pr = _all_pairs(70, 6)

    def check(pols, admin, baseline, **kw):
        cl = Cluster(pods, pols, nss, admin, baseline)
        conn = _connect(cl, **kw)
        r = conn.pair_verdicts(pr)
        _check_verdicts(cl, conn, pr, r)
        return conn, r

    # no NetworkPolicies: a baseline only
    deny_all = k8s.BaselineAdminNetworkPolicy("deny", {
        "subject": everyone, "egress": [{"action": "Deny", "to": [everyone]}],
        "ingress": [{"action": "Deny", "from": [everyone]}]})
    conn, r = check([], [], deny_all)
    assert r.counts["egress_baseline_deny"] == len(pr) and r.counts["allowed"] == 70
    # no admin rules in one direction, and no entry at all on the ingress side
    a_deny = k8s.AdminNetworkPolicy("x", {"priority": 3, "subject": app("d"), "egress": [
        {"action": "Deny", "to": [app("w")], "ports": [{"portNumber": {"port": 80}}]}]})
    conn, r = check([], [a_deny], None)
    assert conn.ingress.engine.info()["P"] == 0
    assert r.counts["ingress_default_allow"] == len(pr) and (r.ingress.decider == -1).all()
    assert r.counts["egress_admin_deny"] > 0
    # ... on a port that drops the one admin entry: everything is default
    r = conn.on_port(("TCP", 81)).pair_verdicts(pr)
    assert r.counts["egress_default_allow"] == len(pr) and r.allowed.all()
    # only ingress rules: the egress side has no entry
    conn, r = check([], [k8s.AdminNetworkPolicy("x", {"priority": 3, "subject": app("d"), "ingress": [
        {"action": "Deny", "from": [app("w")]}]})], None)
    assert conn.egress.engine.info()["P"] == 0 and r.counts["egress_default_allow"] == len(pr)
    # no policy of any kind
    conn, r = check([], [], None)
    assert r.allowed.all() and r.counts["egress_default_allow"] == len(pr)
    # Q = 0, in every accepted spelling
    for empty in ([], np.zeros((0, 2), np.int32), ()):
        r = conn.pair_verdicts(empty)
        assert len(r) == 0 and r.pairs.shape == (0, 2) and r.allowed.shape == (0,)
        assert set(r.counts.values()) == {0} and r.blame("egress") == {}
        assert r.egress.decider.shape == (0,)
    # no pods
    conn = _connect(Cluster([], [], nss, [], deny_all))
    assert len(conn.pair_verdicts([])) == 0
    with pytest.raises(IndexError):
        conn.pair_verdicts([(0, 0)])
    # a rows= object answers pairs outside its rows: only the builds are read
    cl = _tiered(SEEDS_60[1])
    conn = _connect(cl, rows=(10, 20))
    far = _all_pairs(cl.n, 7)
    _check_verdicts(cl, conn, far, conn.pair_verdicts(far))


@pytest.mark.gpu
def test_abi_errors_leave_the_contexts_usable():
    from kano import _native as nat, k8s
    from kano._engine import DeviceBuild
    from kano._intern import intern
    from test_k8s_conn import _unpack
    case = _tier_case(SEED_ABI)
    cl = _tiered(SEED_ABI)
    pods, pols, nss, admin, baseline = case[:5]
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
    pr = _all_pairs(n, 8)
    o = cl.named(None)

    def call(e, i, Q=len(pr), pairs=pr, ce=code_e, ci=code_i, ne=None, ni=None, npe=npe, npi=npi,
             verdict=True):
        ce, ci = np.ascontiguousarray(ce, np.uint32), np.ascontiguousarray(ci, np.uint32)
        pairs = np.ascontiguousarray(pairs, np.int32)
        out = np.zeros(max(Q, 1), np.uint8)
        rc = lib.kano_k8s_pair_verdicts(
            e and e.ctx, i and i.ctx, 1, Q, pairs.ctypes.data, len(ce) if ne is None else ne,
            ce.ctypes.data, npe, len(ci) if ni is None else ni, ci.ctypes.data, npi,
            out.ctypes.data if verdict else None, None, None, None, None, None)
        return rc, out

    def good():
        """the call answers, and kano_k8s_conn_tiers on the same sources still
        writes the same matrix"""
        rc, v = call(eg, ing)
        assert rc == 0
        assert np.array_equal((v & 1).astype(bool), o.allowed(True)[pr[:, 0], pr[:, 1]])
        dst = DeviceBuild.empty(n)
        dst.k8s_conn_tiers_from(eg, ing, True, code_e, npe, code_i, npi)
        assert np.array_equal(_unpack(dst.rows(0, n), n), _tref(case, None, True))
        dst.close()

    def with_code(code, value):
        out = code.copy()
        out[0] = value
        return out

    good()
    EINVAL, ERANGE, ENOTSUP = -errno.EINVAL, -errno.ERANGE, -errno.ENOTSUP
    # codes: illegal for their level, np_level too large, NULL
    assert npe >= 1 and npi >= 1
    for value, word in [(npe * 4 + 2, "passes"), (3, "isolates"), (npe * 4 + 1, "denies")]:
        assert call(eg, ing, ce=with_code(code_e, value))[0] == EINVAL, value
        err = lib.kano_last_error(eg.ctx)
        assert word.encode() in err and b"egress" in err and b"kano_k8s_pair_verdicts" in err
    assert call(eg, ing, ci=with_code(code_i, npi * 4 + 1))[0] == EINVAL
    assert b"ingress" in lib.kano_last_error(eg.ctx)
    assert call(eg, ing, npe=1 << 30)[0] == EINVAL and b"2^30" in lib.kano_last_error(eg.ctx)
    assert call(eg, ing, npi=(1 << 30) + 5)[0] == EINVAL
    rc = lib.kano_k8s_pair_verdicts(eg.ctx, ing.ctx, 1, 0, None, len(code_e), None, npe,
                                    len(code_i), None, npi, None, None, None, None, None, None)
    assert rc == EINVAL and b"NULL" in lib.kano_last_error(eg.ctx)
    good()
    # nids, Q, NULL arguments
    assert call(eg, ing, ne=len(code_e) + 1)[0] == EINVAL
    assert call(eg, ing, ni=len(code_i) - 1)[0] == EINVAL
    assert b"nids" in lib.kano_last_error(eg.ctx)
    assert call(eg, ing, Q=-1)[0] == EINVAL
    assert call(eg, ing, verdict=False)[0] == EINVAL
    assert call(None, ing)[0] == EINVAL and call(eg, None)[0] == EINVAL
    assert lib.kano_k8s_pair_verdicts(eg.ctx, ing.ctx, 1, 3, None, len(code_e),
                                      code_e.ctypes.data, npe, len(code_i), code_i.ctypes.data,
                                      npi, np.zeros(3, np.uint8).ctypes.data, None, None, None,
                                      None, None) == EINVAL
    small = DeviceBuild(intern(c.containers[:-1], c.ingress), build=False)
    small.build_classes()
    assert call(eg, small)[0] == EINVAL
    good()
    # a pair index outside [0, n)
    for bad in ((0, n), (n, 0), (-1, 0), (0, -1)):
        out_of_range = pr.copy()
        out_of_range[len(pr) // 2] = bad
        assert call(eg, ing, pairs=out_of_range)[0] == ERANGE, bad
        assert b"out of range" in lib.kano_last_error(eg.ctx)
    good()
    # sources that are no full, unedited class-level builds
    shard = operand(c.egress, rows=(0, n // 2))
    assert call(shard, ing)[0] == ENOTSUP and b"row shard" in lib.kano_last_error(shard.ctx)
    assert call(eg, shard, ci=code_e)[0] == ENOTSUP
    assert b"row shard" in lib.kano_last_error(eg.ctx)
    good()
    # Q = 0 with NULL pairs and verdict, and the counts of an empty call
    counts = np.full(18, 7, np.int64)
    assert lib.kano_k8s_pair_verdicts(eg.ctx, ing.ctx, 1, 0, None, len(code_e),
                                      code_e.ctypes.data, npe, len(code_i), code_i.ctypes.data,
                                      npi, None, None, None, None, None, counts.ctypes.data) == 0
    assert not counts.any()
    # a dropped entry may carry any bits; another port on the same contexts
    r = eg.k8s_pair_verdicts(ing, pr, False, *[x for pair in zip(c.codes(QUERIES[1]), c.np_level)
                                               for x in pair])
    assert np.array_equal((r["verdict"] & 1).astype(bool),
                          cl.named(QUERIES[1]).allowed(False)[pr[:, 0], pr[:, 1]])
    good()
