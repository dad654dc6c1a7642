"""kano.k8s.connectivity: the reading of NetworkPolicies a cluster enforces
(networking.k8s.io/v1), written by kano_k8s_conn from two class-level builds.

The oracle below restates the semantics on numpy bool arrays, straight from
the manifest dicts: it calls neither compile_conformant nor any kano selector
code.  For every random cluster used, the oracle alone is first checked to be
neither all ones nor the diagonal, with isolated and non-isolated pods in both
directions, so a pass means something."""
import ctypes
import errno
import functools
import random

import numpy as np
import pytest

# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------


def _sel(selector, labels):
    """matchLabels AND matchExpressions on one label dict."""
    if not selector:
        return True
    for k, v in (selector.get("matchLabels") or {}).items():
        if k not in labels or not labels[k] == v:
            return False
    for e in selector.get("matchExpressions") or []:
        k, op = e["key"], e["operator"]
        listed = k in labels and any(labels[k] == x for x in e.get("values") or [])
        if op == "In":
            ok = listed
        elif op == "NotIn":
            ok = not listed
        elif op == "Exists":
            ok = k in labels
        elif op == "DoesNotExist":
            ok = k not in labels
        else:
            raise ValueError(op)
        if not ok:
            return False
    return True


def _counts(ports, port):
    if port is None or not ports:
        return True
    proto, num = port
    for e in ports:
        if e.get("protocol", "TCP") != proto:
            continue
        p = e.get("port")
        if p is None:
            return True
        if isinstance(p, str):
            continue                                     # a named port: out of scope
        if "endPort" in e:
            if p <= num <= e["endPort"]:
                return True
        elif p == num:
            return True
    return False


def oracle(pods, pols, nss, port=None, allow_self=True):
    """(allowed[s, d], isoE, isoI) as numpy bool arrays."""
    nsl = {ns.name: ns.labels for ns in nss}
    for p in pods:
        if p.namespace not in nsl:
            raise KeyError(p.namespace)
    n = len(pods)
    iso = {"Egress": np.zeros(n, bool), "Ingress": np.zeros(n, bool)}
    R = {"Egress": np.zeros((n, n), bool), "Ingress": np.zeros((n, n), bool)}
    for pol in pols:
        spec = pol.spec or {}
        types = spec.get("policyTypes")
        if types is None:
            types = ["Ingress"] + (["Egress"] if "egress" in spec else [])
        selected = [i for i, p in enumerate(pods)
                    if p.namespace == pol.namespace and _sel(spec.get("podSelector"), p.labels)]
        for typ, key, side in (("Egress", "egress", "to"), ("Ingress", "ingress", "from")):
            if typ not in types:
                continue
            iso[typ][selected] = True
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
                R[typ][selected] |= matched
    E, In = R["Egress"], R["Ingress"]
    isoE, isoI = iso["Egress"], iso["Ingress"]
    allowed = (~isoE[:, None] | E) & (~isoI[None, :] | In.T)
    if allow_self:
        allowed |= np.eye(n, dtype=bool)
    return allowed, isoE, isoI


# ---------------------------------------------------------------------------
# clusters
# ---------------------------------------------------------------------------
NS_LABELS = [{"team": "a", "env": "prod"}, {"team": "b"}, {"env": "dev"}, {}, {"team": "a"}]
PORT_POOL = [{"protocol": "TCP", "port": 80}, {"port": 443}, {"protocol": "UDP", "port": 53},
             {"port": 9000, "endPort": 9100}, {"protocol": "TCP"},
             {"protocol": "SCTP", "port": 80, "endPort": 90}]
NAMED_PORT = {"protocol": "TCP", "port": "http"}
QUERIES = [("TCP", 80), ("UDP", 53), ("TCP", 9050)]
OPS = ["In", "NotIn", "Exists", "DoesNotExist"]


def _cluster(seed, n=60, P=16, nns=3, uid=False):
    """test_k8s.py's generator read conformantly: policyTypes in every form,
    empty rule lists, empty from / to, ipBlock and bare podSelector peers, keys
    no pod / no namespace carries under all four operators, ports with
    protocol, port and endPort, and one named port.  ``uid``: every pod has
    its own value under "uid", which a policy selector and a peer name."""
    from kano import k8s
    rnd = random.Random(seed)
    nss = [k8s.Namespace(f"ns{i}", NS_LABELS[i % len(NS_LABELS)]) for i in range(nns)]
    names = [ns.name for ns in nss]
    pods = []
    for i in range(n):
        lab = {"app": rnd.choice(["web", "db", "cache", "api"])}
        if rnd.random() < 0.6:
            lab["tier"] = rnd.choice(["fe", "be"])
        if rnd.random() < 0.2:
            lab["ver"] = rnd.choice([1, 2, "1"])
        if uid:
            lab["uid"] = i
        pods.append(k8s.Pod(f"p{i}", rnd.choice([None] + names), lab))
    nss.append(k8s.Namespace("default", {"team": "c"}))
    names.append("default")
    pod_keys = ["app", "tier", "ver", "zone"]             # zone: no pod carries it
    pod_vals = ["web", "db", "api", "fe", "be", 1, "1"]
    ns_keys = ["team", "env", "region"]                   # region: no namespace carries it
    ns_vals = ["a", "b", "c", "prod", "dev"]

    def expr(keys, vals):
        op = rnd.choice(OPS)
        e = {"key": rnd.choice(keys), "operator": op}
        if op in ("In", "NotIn"):
            e["values"] = rnd.sample(vals, 2)
        return e

    def selector(keys, vals):
        r = rnd.random()
        if r < 0.5:
            return {"matchLabels": {keys[0]: rnd.choice(vals)}}
        if r < 0.6:
            return {}
        s = {}
        if rnd.random() < 0.6:
            s["matchLabels"] = {k: rnd.choice(vals) for k in rnd.sample(keys, rnd.randint(0, 2))}
        s["matchExpressions"] = [expr(keys, vals) for _ in range(rnd.randint(1, 2))]
        return s

    def peer():
        r = rnd.random()
        if r < 0.08:
            return {"ipBlock": {"cidr": "10.0.0.0/8"}}
        if r < 0.12:
            return {}
        p = {}
        if r < 0.7:                                       # r < 0.5: a bare podSelector
            p["podSelector"] = selector(pod_keys, pod_vals)
        if r >= 0.5:
            p["namespaceSelector"] = selector(ns_keys, ns_vals)
        return p

    def rules(side):
        out = []
        for _ in range(rnd.randint(0, 2)):
            r = rnd.random()
            rule = {} if r < 0.1 else {side: [peer() for _ in range(rnd.randint(0, 2))]}
            if rnd.random() < 0.6:
                rule["ports"] = rnd.sample(PORT_POOL, rnd.randint(1, 2))
            out.append(None if r > 0.97 else rule)
        return out

    pols = []
    for q in range(P):
        spec = {}
        r = rnd.random()
        if r < 0.8:                                       # narrow: one app of the namespace
            spec["podSelector"] = {"matchLabels": {"app": rnd.choice(["web", "db", "cache", "api"])}}
        elif r < 0.9:
            spec["podSelector"] = selector(pod_keys, pod_vals)
        form = rnd.randrange(6)
        if form < 4:
            spec["policyTypes"] = [["Ingress"], ["Egress"], ["Ingress", "Egress"], []][form]
        if form != 4 or rnd.random() < 0.5:
            if rnd.random() < 0.8:
                spec["egress"] = rules("to")
            if rnd.random() < 0.8:
                spec["ingress"] = rules("from") if rnd.random() < 0.9 else None
        else:
            spec["ingress"] = rules("from")               # no egress key: Ingress only
        pols.append(k8s.NetworkPolicy(f"np{q}", rnd.choice(names + [None, "ghost"]), spec))
    # one named port, and -- uid -- the key that makes every pod a class
    pols.append(k8s.NetworkPolicy("named", names[0], {
        "podSelector": {"matchLabels": {"app": "web"}},
        "ingress": [{"from": [{"podSelector": {}}], "ports": [NAMED_PORT]}]}))
    if uid:     # (plain values: the engine classifies the pods by the key's value)
        pols.append(k8s.NetworkPolicy("uid", pods[3].namespace, {
            "podSelector": {"matchLabels": {"uid": 3}},
            "policyTypes": ["Ingress", "Egress"],
            "ingress": [{"from": [{"namespaceSelector": {},
                                   "podSelector": {"matchLabels": {"uid": n - 2}}}]}],
            "egress": [{"to": [{"namespaceSelector": {},
                                "podSelector": {"matchLabels": {"uid": n // 2}}}]}]}))
    return pods, pols, nss


@functools.lru_cache(maxsize=None)
def _case(seed, n=60, P=16, nns=3, uid=False):
    """A cluster with its oracle results per (port, allow_self), computed once
    and never written; the oracle alone is checked to be a meaningful case."""
    pods, pols, nss = _cluster(seed, n, P, nns, uid)
    full, isoE, isoI = oracle(pods, pols, nss, None, True)
    assert not full.all(), "all ones"
    assert (full & ~np.eye(n, dtype=bool)).any(), "only the diagonal"
    assert isoE.any() and not isoE.all() and isoI.any() and not isoI.all()
    for a in (full, isoE, isoI):
        a.setflags(write=False)
    return pods, pols, nss, {(None, True): full}, isoE, isoI


def _ref(case, port, allow_self):
    """The oracle's matrix of one query, computed once."""
    pods, pols, nss, ref = case[:4]
    if (port, allow_self) not in ref:
        a = oracle(pods, pols, nss, port, allow_self)[0]
        a.setflags(write=False)
        ref[(port, allow_self)] = a
    return ref[(port, allow_self)]


def _unpack(words, n):
    w = np.ascontiguousarray(words, dtype=np.uint64)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little")[:, :n].astype(bool)


def _pack(bits):
    n = bits.shape[1]
    W = (n + 63) // 64
    padded = np.zeros((bits.shape[0], W * 64), dtype=np.uint8)
    padded[:, :n] = bits
    return np.packbits(padded, axis=1, bitorder="little").view(np.uint64).reshape(-1, W)


def _rows(m, r0=0, r1=None):
    n = m.container_size
    r1 = n if r1 is None else r1
    return _unpack(m.engine.rows(r0, r1 - r0), n) if r1 > r0 else np.zeros((0, n), bool)


# ---------------------------------------------------------------------------
# the known answers: a six-pod cluster worked out from the rules, as literals
# ---------------------------------------------------------------------------
def _known():
    from kano import k8s
    nss = [k8s.Namespace("shop", {"team": "a"}), k8s.Namespace("ops", {"team": "b"})]
    pods = [k8s.Pod(f"p{i}", ns, {"app": app}) for i, (ns, app) in enumerate(
        [("shop", "web"), ("shop", "api"), ("shop", "db"), ("ops", "mon"), ("ops", "job"),
         ("ops", "web")])]
    app = lambda v: {"matchLabels": {"app": v}}   # noqa: E731
    pols = [
        k8s.NetworkPolicy("A", "shop", {
            "podSelector": app("db"), "policyTypes": ["Ingress"],
            "ingress": [
                {"from": [{"podSelector": app("api")}],
                 "ports": [{"protocol": "TCP", "port": 5432}]},
                {"from": [{"namespaceSelector": {"matchLabels": {"team": "b"}},
                           "podSelector": app("mon")}],
                 "ports": [{"port": 9000, "endPort": 9100}]}]}),
        k8s.NetworkPolicy("B", "shop", {
            "podSelector": app("api"), "policyTypes": ["Egress"],
            "egress": [{"to": [{"podSelector": app("db")}]}]}),
        k8s.NetworkPolicy("C", "ops", {"podSelector": {}, "policyTypes": ["Ingress"]}),
        k8s.NetworkPolicy("D", "shop", {
            "podSelector": app("web"),
            "egress": [{"to": [{"namespaceSelector": {}}],
                        "ports": [{"protocol": "UDP", "port": 53}]}]}),
    ]
    return pods, pols, nss


KNOWN_ISO_E, KNOWN_ISO_I = "110000", "101111"
KNOWN = {   # (port, allow_self) -> rows 0..5
    (None, True): "110000 011000 011000 011100 010010 010001",
    (("TCP", 5432), True): "100000 011000 011000 010100 010010 010001",
    (("TCP", 9050), True): "100000 010000 011000 011100 010010 010001",
    (("UDP", 53), True): "110000 010000 011000 010100 010010 010001",
    (("TCP", 80), True): "100000 010000 011000 010100 010010 010001",
    (None, False): "010000 001000 010000 011000 010000 010000",
}


def _bits_of(text):
    return np.array([[c == "1" for c in row] for row in text.split()], dtype=bool)


# ---------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------
def test_known_answers_oracle():
    pods, pols, nss = _known()
    for (port, allow_self), rows in KNOWN.items():
        a, isoE, isoI = oracle(pods, pols, nss, port, allow_self)
        assert np.array_equal(a, _bits_of(rows)), (port, allow_self)
        assert np.array_equal(isoE, _bits_of(KNOWN_ISO_E)[0])
        assert np.array_equal(isoI, _bits_of(KNOWN_ISO_I)[0])
    assert oracle(pods, [], nss)[0].all()


def _compiled_matrix(pods, pols, nss, port, allow_self):
    """compile_conformant's lists evaluated by the kano restatement (oracle
    ref_py: the per-entry select / allow sets), combined in numpy."""
    from kano import k8s
    from oracle import kano_oracle as orc
    n = len(pods)
    c = k8s.compile_conformant(pods, pols, nss)
    keep = c.keep(port)
    out = []
    for entries, kp in ((c.egress, keep[0]), (c.ingress, keep[1])):
        r = orc.ref_py(c.containers, entries)
        sel = np.array([[ch == "1" for ch in s] for s in r["sel"]], dtype=bool).reshape(-1, n)
        alw = np.array([[ch == "1" for ch in s] for s in r["allow"]], dtype=bool).reshape(-1, n)
        iso = sel.any(axis=0)
        if kp is not None:
            sel, alw = sel[kp.astype(bool)], alw[kp.astype(bool)]
        else:     # every entry: ref_py's own matrix is the same OR
            M = np.array([[ch == "1" for ch in s] for s in r["M"]], dtype=bool).reshape(n, n)
            assert np.array_equal(M, (sel.T.astype(np.int64) @ alw.astype(np.int64)) > 0)
        out.append(((sel.T.astype(np.int64) @ alw.astype(np.int64)) > 0, iso))
    (E, isoE), (In, isoI) = out
    allowed = (~isoE[:, None] | E) & (~isoI[None, :] | In.T)
    if allow_self:
        allowed |= np.eye(n, dtype=bool)
    return allowed, isoE, isoI


def test_known_answers_compiled():
    pods, pols, nss = _known()
    for (port, allow_self), rows in KNOWN.items():
        a, isoE, isoI = _compiled_matrix(pods, pols, nss, port, allow_self)
        assert np.array_equal(a, _bits_of(rows)), (port, allow_self)
        assert np.array_equal(isoE, _bits_of(KNOWN_ISO_E)[0])
        assert np.array_equal(isoI, _bits_of(KNOWN_ISO_I)[0])


@pytest.mark.parametrize("seed", range(6))
def test_compilation_matches_oracle(seed):
    case = _case(seed, n=40, P=14)
    pods, pols, nss, _, isoE, isoI = case
    for port in [None] + QUERIES:
        a, e, i = _compiled_matrix(pods, pols, nss, port, True)
        assert np.array_equal(e, isoE) and np.array_equal(i, isoI)
        assert np.array_equal(a, _ref(case, port, True)), port
    a, _, _ = _compiled_matrix(pods, pols, nss, None, False)
    assert np.array_equal(a, _ref(case, None, False))


def test_compiled_origins_and_isolation_entries():
    from kano import k8s
    from kano.model import DoesNotExist
    pods, pols, nss = _known()
    c = k8s.compile_conformant(pods, pols, nss)
    assert c.origin_egress == [(1, "egress", 0, 0), (3, "egress", 0, 0)]
    # C has no rules: one entry that isolates and allows nothing; D is Ingress
    # by default with no ingress rules: likewise
    assert c.origin_ingress == [(0, "ingress", 0, 0), (0, "ingress", 1, 0),
                                (2, "ingress", None, None), (3, "ingress", None, None)]
    assert c.ports_ingress[:2] == [pols[0].spec["ingress"][0]["ports"],
                                   pols[0].spec["ingress"][1]["ports"]]
    assert all(isinstance(v, DoesNotExist) for v in c.ingress[2].allow.labels.values())
    ke, ki = c.keep(("TCP", 9050))
    assert ke.tolist() == [1, 0] and ki.tolist() == [0, 1, 1, 1]
    assert c.keep(None) == (None, None)
    # a selector naming a key no pod carries selects nothing and isolates nobody
    ghost = k8s.NetworkPolicy("g", "shop", {"podSelector": {"matchLabels": {"zone": "x"}},
                                            "policyTypes": ["Ingress", "Egress"]})
    c = k8s.compile_conformant(pods, [ghost], nss)
    assert c.egress == [] and c.ingress == []


def test_load_manifests(tmp_path):
    from kano import k8s
    (tmp_path / "sub").mkdir()
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
kind: Service
metadata: {name: ignored}
---
apiVersion: networking.k8s.io/v1
kind: NetworkPolicy
metadata: {name: deny, namespace: shop}
spec: {podSelector: {}, policyTypes: [Ingress]}
""")
    (tmp_path / "sub" / "b.yml").write_text("""
apiVersion: v1
kind: List
items:
- {apiVersion: v1, kind: Pod, metadata: {name: mon, namespace: ops, labels: {app: mon}}}
- {apiVersion: v1, kind: Pod, metadata: {name: bare}}
- {apiVersion: v1, kind: ConfigMap, metadata: {name: ignored}}
""")
    (tmp_path / "notes.txt").write_text("not a manifest: [")
    pods, pols, nss = k8s.load_manifests([tmp_path])
    assert [(p.name, p.namespace) for p in pods] == [("web", "shop"), ("mon", "ops"),
                                                    ("bare", "default")]
    assert [(p.name, p.namespace, p.spec["policyTypes"]) for p in pols] == [
        ("deny", "shop", ["Ingress"])]
    by = {ns.name: ns.labels for ns in nss}
    assert by == {"shop": {"team": "a", "kubernetes.io/metadata.name": "shop"},
                  "ops": {"kubernetes.io/metadata.name": "ops"},
                  "default": {"kubernetes.io/metadata.name": "default"}}
    one = k8s.load_manifests(str(tmp_path / "a.yaml"))
    assert len(one[0]) == 1 and len(one[1]) == 1 and len(one[2]) == 1
    a, _, isoI = oracle(pods, pols, nss)
    c, _, ci = _compiled_matrix(pods, pols, nss, None, True)
    assert np.array_equal(a, c) and np.array_equal(isoI, ci) and isoI.tolist() == [1, 0, 0]


def test_host_errors():
    from kano import k8s
    nss = [k8s.Namespace("default")]
    pods = [k8s.Pod("a", None, {"x": "1"})]
    for op in ("in", "doesnotexists", "Gt", None):
        bad = k8s.NetworkPolicy("p", None, {"podSelector": {"matchExpressions": [
            {"key": "x", "operator": op, "values": ["1"]}]}})
        with pytest.raises(ValueError):
            k8s.compile_conformant(pods, [bad], nss)
    peer = k8s.NetworkPolicy("p", None, {"podSelector": {}, "ingress": [{"from": [
        {"namespaceSelector": {"matchExpressions": [{"key": "region", "operator": "bogus"}]}}]}]})
    with pytest.raises(ValueError):
        k8s.compile_conformant(pods, [peer], nss)
    with pytest.raises(KeyError):
        k8s.compile_conformant([k8s.Pod("a", "nowhere")], [], nss)
    with pytest.raises(ValueError):
        k8s.compile_conformant(pods, [], nss).keep(("TCP", "http"))
    with pytest.raises(ValueError):
        k8s.connectivity(pods, [], nss, form="rows")


# ---------------------------------------------------------------------------
# GPU tests
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_known_answers_gpu():
    from kano import k8s
    pods, pols, nss = _known()
    base = {True: k8s.connectivity(pods, pols, nss),
            False: k8s.connectivity(pods, pols, nss, allow_self=False)}
    for (port, allow_self), rows in KNOWN.items():
        want = _bits_of(rows)
        direct = k8s.connectivity(pods, pols, nss, port=port, allow_self=allow_self)
        again = base[allow_self].on_port(port)
        for r in (direct, again):
            assert np.array_equal(_rows(r.allowed), want), (port, allow_self)
            assert np.array_equal(r.egress_isolated, _bits_of(KNOWN_ISO_E)[0])
            assert np.array_equal(r.ingress_isolated, _bits_of(KNOWN_ISO_I)[0])
        # the same two resident builds, nothing uploaded again
        assert again.egress is base[allow_self].egress
        assert again.ingress is base[allow_self].ingress
    r = base[True]
    assert r.info["egress_isolated"] == 2 and r.info["ingress_isolated"] == 5
    assert r.info["kept_egress_entries"] == 2 and r.info["kept_ingress_entries"] == 4
    assert r.on_port(("TCP", 9050)).info["kept_ingress_entries"] == 3
    assert r.origin_egress == [(1, "egress", 0, 0), (3, "egress", 0, 0)]
    assert _rows(k8s.connectivity(pods, [], nss).allowed).all()


def _check(case, port, allow_self, r):
    assert np.array_equal(_rows(r.allowed), _ref(case, port, allow_self)), (port, allow_self)
    assert np.array_equal(r.egress_isolated, case[4])
    assert np.array_equal(r.ingress_isolated, case[5])


@pytest.mark.gpu
@pytest.mark.parametrize("allow_self", [True, False])
@pytest.mark.parametrize("seed", range(12))
def test_matches_oracle(seed, allow_self):
    from kano import k8s
    case = _case(seed)
    pods, pols, nss = case[:3]
    for form in ("auto", "direct", "stream"):
        r = k8s.connectivity(pods, pols, nss, allow_self=allow_self, form=form)
        _check(case, None, allow_self, r)
        for port in (QUERIES[seed % 3], QUERIES[(seed + 1) % 3]):
            _check(case, port, allow_self, r.on_port(port))


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["direct", "stream", "auto"])
@pytest.mark.parametrize("seed,n,P", [(21, 130, 20), (22, 1030, 30)])
def test_matches_oracle_more_blocks(seed, n, P, form):
    """n = 130: three words a row; n = 1030 crosses the 1024-destination
    block and the 64-row block, in both forms of the write.  Pad bits and pad
    words read as zero."""
    from kano import k8s
    case = _case(seed, n=n, P=P, nns=4)
    pods, pols, nss = case[:3]
    r = k8s.connectivity(pods, pols, nss, form=form)
    _check(case, None, True, r)
    for port in QUERIES[:2]:
        _check(case, port, True, r.on_port(port))
    words = r.allowed.engine.rows(0, n)
    assert words.shape == (n, (n + 63) // 64)
    assert np.array_equal(words, _pack(_ref(case, None, True)))
    assert not (words[:, -1] >> np.uint64(n & 63)).any()


@pytest.mark.gpu
def test_wide_class_rows_gather_from_global():
    """Every pod its own class on both sides (a selector and a peer name the
    pods' distinct "uid"): each class row exceeds 32 words and the two together
    the 64 words the expansion stages in LDS, so it gathers from global memory."""
    from kano import k8s
    n = 2200
    case = _case(31, n=n, P=24, nns=3, uid=True)
    pods, pols, nss = case[:3]
    r = k8s.connectivity(pods, pols, nss, form="direct")
    ie, ii = r.egress.engine.info(), r.ingress.engine.info()
    assert (ie["UA"] + 63) // 64 > 32 and (ii["U"] + 63) // 64 > 32
    _check(case, None, True, r)
    _check(case, QUERIES[0], True, r.on_port(QUERIES[0]))
    # auto is the direct form here (more class rows than rows / 2)
    assert ie["U"] + ii["UA"] > n // 2
    # streamed: one table's class rows a launch, staged (35 words each)
    _check(case, QUERIES[1], True, k8s.connectivity(pods, pols, nss, port=QUERIES[1],
                                                    form="stream"))


@pytest.mark.gpu
def test_streamed_expansion_gathers_from_global():
    """More than 4096 classes on each side: one table's class row alone exceeds
    the 64 words the expansion stages, so the streamed form's one-table
    expansions gather from global memory."""
    from kano import k8s
    n = 4200
    case = _case(32, n=n, P=24, nns=3, uid=True)
    pods, pols, nss = case[:3]
    r = k8s.connectivity(pods, pols, nss, form="stream")
    ie, ii = r.egress.engine.info(), r.ingress.engine.info()
    assert (ie["UA"] + 63) // 64 > 64 and (ii["U"] + 63) // 64 > 64
    _check(case, None, True, r)


@pytest.mark.gpu
def test_degenerate_inputs():
    from kano import k8s
    nss = [k8s.Namespace("a", {"team": "x"})]
    for n in (0, 1):
        pods = [k8s.Pod(f"p{i}", "a", {"app": "w"}) for i in range(n)]
        deny = k8s.NetworkPolicy("deny", "a", {"podSelector": {},
                                               "policyTypes": ["Ingress", "Egress"]})
        for pols in ([], [deny]):
            for allow_self in (True, False):
                r = k8s.connectivity(pods, pols, nss, allow_self=allow_self)
                want = oracle(pods, pols, nss, None, allow_self)[0]
                assert np.array_equal(_rows(r.allowed), want)
                assert r.egress_isolated.shape == (n,)
    pods = [k8s.Pod(f"p{i}", "a", {"app": "w" if i % 3 else "d"}) for i in range(70)]
    n = len(pods)
    # no policies: all ones; a source without classes on both sides
    assert _rows(k8s.connectivity(pods, [], nss, allow_self=False).allowed).all()
    # one namespace-wide deny-all of both types: the diagonal only
    deny = k8s.NetworkPolicy("deny", "a", {"podSelector": {},
                                           "policyTypes": ["Ingress", "Egress"]})
    r = k8s.connectivity(pods, [deny], nss)
    assert np.array_equal(_rows(r.allowed), np.eye(n, dtype=bool))
    assert r.egress_isolated.all() and r.ingress_isolated.all()
    assert not _rows(k8s.connectivity(pods, [deny], nss, allow_self=False).allowed).any()
    # policies of one direction only: the other source has no classes
    eg_only = k8s.NetworkPolicy("e", "a", {
        "podSelector": {"matchLabels": {"app": "d"}}, "policyTypes": ["Egress"],
        "egress": [{"to": [{"podSelector": {"matchLabels": {"app": "w"}}}]}]})
    in_only = k8s.NetworkPolicy("i", "a", {
        "podSelector": {"matchLabels": {"app": "d"}}, "policyTypes": ["Ingress"],
        "ingress": [{"from": [{"podSelector": {"matchLabels": {"app": "d"}}}],
                     "ports": [{"port": 80}]}]})
    for pol in (eg_only, in_only):
        for port in (None, ("TCP", 80), ("TCP", 81)):
            for allow_self in (True, False):
                a, isoE, isoI = oracle(pods, [pol], nss, port, allow_self)
                assert not a.all() and a.any()
                for form in ("direct", "stream"):
                    r = k8s.connectivity(pods, [pol], nss, port=port, allow_self=allow_self,
                                         form=form)
                    assert np.array_equal(_rows(r.allowed), a), form
                assert np.array_equal(r.egress_isolated, isoE)
                assert np.array_equal(r.ingress_isolated, isoI)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["direct", "stream"])
@pytest.mark.parametrize("cuts", [[0, 30, 60], [0, 1, 59, 60], [0, 20, 20, 45, 60]])
def test_row_shards(cuts, form):
    from kano import k8s
    case = _case(5)
    pods, pols, nss = case[:3]
    for port, allow_self in ((None, True), (QUERIES[0], False)):
        parts = []
        for r0, r1 in zip(cuts[:-1], cuts[1:]):
            r = k8s.connectivity(pods, pols, nss, port=port, allow_self=allow_self,
                                 rows=(r0, r1), form=form)
            parts.append(_rows(r.allowed, r0, r1))
            assert np.array_equal(r.egress_isolated, case[4])
        assert np.array_equal(np.concatenate(parts, axis=0), _ref(case, port, allow_self))


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
    """hop_distance, check_intents and matrix_diff read .allowed like any
    matrix: each result equals the same query on the oracle's bits."""
    from kano import algorithm as alg, k8s
    from kano.model import Container
    case = _case(7)
    pods, pols, nss = case[:3]
    n = len(pods)
    port = QUERIES[0]
    r = k8s.connectivity(pods, pols, nss)
    rp = r.on_port(port)
    ref, refp = _loaded(_ref(case, None, True)), _loaded(_ref(case, port, True))
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
    got, want = alg.matrix_diff(r.allowed, rp.allowed), alg.matrix_diff(ref, refp)
    assert got.removed == want.removed == int((_ref(case, None, True)
                                               & ~_ref(case, port, True)).sum()) > 0
    assert got.added == want.added == 0
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_explain():
    from kano import k8s
    pods, pols, nss = _known()
    r = k8s.connectivity(pods, pols, nss)
    # api -> db: B's egress rule and A's first ingress rule
    x = r.explain(1, 2)
    assert x["allowed"] and not x["self"] and x["blocked_by"] == []
    assert x["egress"] == {"isolated": True, "policies": [("B", 0, 0)]}
    assert x["ingress"] == {"isolated": True, "policies": [("A", 0, 0)]}
    # api -> web: B isolates api's egress and allows only db
    x = r.explain(1, 0)
    assert not x["allowed"] and x["blocked_by"] == ["egress", "ingress"]
    assert x["egress"] == {"isolated": True, "policies": []}
    # mon -> job: mon's egress is free, C isolates job's ingress with no rules
    x = r.explain(3, 4)
    assert not x["allowed"] and x["blocked_by"] == ["ingress"]
    assert x["egress"] == {"isolated": False, "policies": []}
    assert x["ingress"] == {"isolated": True, "policies": []}
    # web -> api on TCP 80: D's only egress rule is UDP 53
    x = r.on_port(("TCP", 80)).explain(0, 1)
    assert not x["allowed"] and x["blocked_by"] == ["egress"]
    assert r.explain(0, 1)["egress"]["policies"] == [("D", 0, 0)]
    x = r.explain(4, 4)
    assert x["allowed"] and x["self"] and x["blocked_by"] == ["ingress"]
    with pytest.raises(IndexError):
        r.explain(0, 6)
    # every pair of two queries: explain agrees with the matrix
    for port in (None, ("TCP", 9050)):
        rp, want = r.on_port(port), _bits_of(KNOWN[(port, True)])
        for s in range(6):
            for d in range(6):
                assert rp.explain(s, d)["allowed"] == bool(want[s, d]), (port, s, d)


@pytest.mark.gpu
def test_abi_errors_leave_the_contexts_usable():
    from kano import _native as nat, k8s
    from kano._engine import DeviceBuild
    from kano._intern import intern, intern_more
    case = _case(3)
    pods, pols, nss = case[:3]
    n = len(pods)
    c = k8s.compile_conformant(pods, pols, nss)
    lib = nat.load()

    def operand(entries, rows=None):
        b = DeviceBuild(intern(c.containers, entries), rows=rows, build=False)
        b.build_classes()
        return b

    eg, ing = operand(c.egress), operand(c.ingress)
    dst = DeviceBuild.empty(n)
    Pe, Pi = len(c.egress), len(c.ingress)

    def call(e, i, d, ne=Pe, ni=Pi):
        return lib.kano_k8s_conn(e and e.ctx, i and i.ctx, d and d.ctx, 1, ne, None, ni, None,
                                 None)

    def good():
        assert call(eg, ing, dst) == 0
        assert np.array_equal(_unpack(dst.rows(0, n), n), _ref(case, None, True))

    good()
    assert call(None, ing, dst) == -errno.EINVAL
    assert call(eg, ing, None) == -errno.EINVAL
    assert call(eg, ing, eg) == -errno.EINVAL
    assert call(eg, dst, dst) == -errno.EINVAL
    assert call(eg, ing, dst, ne=Pe + 1) == -errno.EINVAL
    assert call(eg, ing, dst, ni=Pi - 1) == -errno.EINVAL
    assert b"nids" in lib.kano_last_error(dst.ctx)
    small = DeviceBuild.empty(n - 1)
    assert call(eg, ing, small) == -errno.EINVAL
    assert lib.kano_k8s_isolated(eg.ctx, None) == -errno.EINVAL
    assert lib.kano_k8s_isolated(None, np.zeros(n, np.uint8).ctypes.data) == -errno.EINVAL
    good()
    shard = operand(c.egress, rows=(0, n // 2))
    assert call(shard, ing, dst) == -errno.ENOTSUP
    assert b"row shard" in lib.kano_last_error(dst.ctx)
    good()
    removed = operand(c.ingress)
    removed.remove_policies([0])
    assert call(eg, removed, dst) == -errno.ENOTSUP
    assert b"added or removed" in lib.kano_last_error(dst.ctx)
    good()
    added = operand(c.egress)
    added.add_policies(*intern_more(added.tables, c.egress[:1]))
    assert call(added, ing, dst) == -errno.ENOTSUP
    assert b"added or removed" in lib.kano_last_error(dst.ctx)
    assert call(added, ing, dst, ne=Pe + 1) == -errno.ENOTSUP
    good()
    # a context holding policy lists (kano_shadow_lists), as either source
    lst = DeviceBuild(None)
    loff, lflat = np.array([0, 1, 2], np.int64), np.array([0, 1], np.int32)
    law, lcnt = np.full((2, 1), 3, np.uint64), ctypes.c_int64()
    assert lib.kano_shadow_lists(lst.ctx, 2, 64, 2, loff.ctypes.data, lflat.ctypes.data,
                                 law.ctypes.data, ctypes.byref(lcnt)) == 0
    for e, i in ((lst, ing), (eg, lst)):
        assert call(e, i, dst, ne=2 if e is lst else Pe, ni=2 if i is lst else Pi) \
            == -errno.ENOTSUP
        assert b"policy lists" in lib.kano_last_error(dst.ctx)
        good()
    assert lib.kano_k8s_isolated(lst.ctx, np.zeros(64, np.uint8).ctypes.data) == -errno.ENOTSUP
    lst.close()
    edited = operand(c.egress)
    edited.set_bit(0, 0, 1)
    assert call(edited, ing, dst) == -errno.ENOTSUP
    assert lib.kano_k8s_isolated(edited.ctx, np.zeros(n, np.uint8).ctypes.data) == -errno.ENOTSUP
    good()
    # the sources still answer their own queries, the errors changed nothing
    assert np.array_equal(eg.k8s_isolated(), case[4])
    assert np.array_equal(ing.k8s_isolated(), case[5])
    keep = c.keep(QUERIES[1])
    info = dst.k8s_conn_from(eg, ing, False, *keep)
    assert info["egress_entries"] == int(keep[0].sum())
    assert info["egress_isolated"] == int(case[4].sum())
    assert np.array_equal(_unpack(dst.rows(0, n), n), _ref(case, QUERIES[1], False))
