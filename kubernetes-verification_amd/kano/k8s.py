"""kubesv's Kubernetes reading of NetworkPolicies, on kano's engine
(namespaces, namespaceSelector, per-direction rules,
self traffic and pods selected by no policy).

kano_py reads a policy as one (select, allow) pair of equality selectors.
kubesv (kubesv/kubesv/model.py, constraint.py) reads Kubernetes objects:

* ``selected_by_pol(pod, pol)`` -- pod in the policy's namespace matching its
  ``podSelector`` (model.py:496-514);
* ``ingress_allow_by_pol`` / ``egress_allow_by_pol(pod, pol)`` -- pod matching
  one peer of one rule: ``namespaceSelector`` on the pod's namespace's labels,
  ``podSelector`` on the pod's labels (model.py:296-307,349-362,420-483);
* ``ingress_traffic(src, sel)``, ``egress_traffic(dst, sel)``,
  ``edge(src, dst) :- ingress_traffic(src, sel), egress_traffic(dst, sel)``
  and ``path`` (constraint.py:168-237).

Here each (policy, peer) becomes one kano policy: select = the policy's pod
selector and namespace, allow = the peer's terms -- matchLabels as plain kano
values (the quick fail guarantees some pod carries the key, so kano's quirk
Q1 cannot fire), matchExpressions as requirement columns (``model.In``
etc.).  Two device builds give
InT[sel][src] and EgT[sel][dst]; ``kano_k8s_edge`` forms the edge matrix on
the device (kano_k8s.hpp).  Every check of ``kano.algorithm`` and the path
functions then read it like any matrix.

kubesv's behaviour is kept where it departs from the Kubernetes documents
(each was read off the code):

* K1 a peer's ``podSelector`` without ``namespaceSelector`` matches pods of
  every namespace (the ``namespace(pod, ns)`` atom leaves ``ns`` free,
  model.py:435-436);
* K2 a selector naming a label key no pod (for ``namespaceSelector``: no
  namespace) carries fails as a whole -- the policy selects nothing, the
  peer matches nothing (model.py:196-201,224-232, "quick fail");
* K3 matchExpressions operators compare lower-cased against ``in``,
  ``notin``, ``exists``, ``doesnotexists``; anything else (Kubernetes'
  ``DoesNotExist`` included) is dropped (model.py:149-156);
* K4 ingress rules count only when the policy also has ``egress``
  (model.py:474-476); ``ingress: null`` beside an ``egress`` list, and a rule
  whose ``from`` / ``to`` is null, raise ``TypeError`` (iterating None,
  model.py:478,436 via :352-356);
* K5 a peer with neither selector (an ``ipBlock``) matches every pod
  (model.py:296-307: no atoms beyond ``namespace(pod, ns)``);
* K6 with ``check_select_by_no_policy`` a pod selected by no policy receives
  from and sends to every pod, so edge(src, dst) holds for every pair
  (constraint.py:207-212,222-227,229-231);
* K7 ``policyTypes`` and ports are not used by the relations; a pod in a
  namespace missing from the namespace list raises ``KeyError``
  (constraint.py:251).

Two behaviours of kubesv's encoding are NOT reproduced (intentional
departures, both z3 sort/name artefacts rather than readings of the rules):

* K8 a ``namespaceSelector`` In / NotIn requirement: kubesv declares the
  membership relation over ``pod_sort`` and applies it to a namespace
  variable (model.py:211-221); z3 then raises a sort mismatch whenever the
  pod and namespace bit-vector widths differ, and otherwise ranges over
  namespace ids read as pod ids.  Here the requirement is evaluated on the
  namespace's labels (the Kubernetes meaning).
* K9 namespace label relations are declared as ``Function(k, nam_sort,
  ...)`` under the pod relation's name ``k`` (constraint.py:270, not
  ``k__namespace``); when the two sort widths match that is the same z3
  function as the pod label relation ``k``, so pod and namespace facts on a
  shared key mix.  Here the namespace's labels and the pods' labels stay
  separate columns.

Parity: against ``oracle/kano_oracle.py kubesv_edge_py``, a restatement of
the Datalog rules on Python sets -- unpinned against kubesv itself (it needs
z3 and the kubernetes client, both absent here).

The reading a cluster enforces (networking.k8s.io/v1: policyTypes, isolation
per direction, namespaced peers, ports) is the second half of this module:
``connectivity`` / ``compile_conformant`` / ``load_manifests``, over the same
objects.  ``build``, ``compile_policies`` and kubesv's quirks are untouched by
it.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np

from .model import (ReachabilityMatrix, Container, Policy, PolicySelect, PolicyAllow,
                    PolicyEgress, In, NotIn, Exists, DoesNotExist, LabelExpression)

_NS = ("__k8s_namespace__",)


class Namespace:
    """NamespaceAdapter (kubesv/kubesv/model.py:24-50)."""

    def __init__(self, name: str, labels: Optional[Dict[str, Any]] = None):
        self.name = name
        self.labels = dict(labels) if labels else {}


class Pod:
    """PodAdapter (model.py:52-84): namespace defaults to "default"."""

    def __init__(self, name: str, namespace: Optional[str] = None,
                 labels: Optional[Dict[str, Any]] = None):
        self.name = name
        self.namespace = namespace if namespace is not None else "default"
        self.labels = dict(labels) if labels else {}


class NetworkPolicy:
    """PolicyAdapter (model.py:389-553) over a NetworkPolicy spec dict in the
    manifest's camelCase (``podSelector``, ``ingress: [{from: [...]}]``,
    ``egress: [{to: [...]}]``, peers with ``podSelector`` /
    ``namespaceSelector`` / ``ipBlock``, selectors with ``matchLabels`` /
    ``matchExpressions``)."""

    def __init__(self, name: str, namespace: Optional[str] = None,
                 spec: Optional[Dict[str, Any]] = None):
        self.name = name
        self.namespace = namespace if namespace is not None else "default"
        self.spec = spec

    @staticmethod
    def from_manifest(obj: Dict[str, Any]) -> "NetworkPolicy":
        md = obj.get("metadata") or {}
        return NetworkPolicy(md.get("name"), md.get("namespace"), obj.get("spec"))


def from_dict(kind: str, data: Dict[str, Any]):
    """kubesv.parser.from_dict (kubesv/kubesv/parser.py:9-18) without the
    kubernetes client: a manifest dict as this module's Pod / Namespace /
    NetworkPolicy (kind 'V1Pod', 'V1Namespace', 'V1NetworkPolicy'; the 'V1'
    prefix is optional)."""
    k = kind[2:] if kind.startswith("V1") else kind
    md = (data or {}).get("metadata") or {}
    if k == "Pod":
        return Pod(md.get("name"), md.get("namespace"), md.get("labels"))
    if k == "Namespace":
        return Namespace(md.get("name"), md.get("labels"))
    if k == "NetworkPolicy":
        return NetworkPolicy.from_manifest(data)
    raise ValueError(f"unsupported kind {kind!r}")


def from_yaml(kind: str, yml: str):
    """kubesv.parser.from_yaml (parser.py:21-22)."""
    import yaml
    return from_dict(kind, yaml.safe_load(yml))


# ---------------------------------------------------------------------------
# selectors -> requirement terms
# ---------------------------------------------------------------------------

_OPS = {"in": In, "notin": NotIn, "exists": Exists, "doesnotexists": DoesNotExist}


def _terms(selector: Optional[Dict[str, Any]], known: set) -> Optional[List[tuple]]:
    """LabelSelectorAdapter.define_label_selector (model.py:178-233): the
    (key, requirement) terms of a selector, or None on a quick fail (K2)."""
    if selector is None:
        return []
    out = []
    exprs = selector.get("matchExpressions")
    if exprs is not None:
        for e in exprs:
            op = _OPS.get(str(e.get("operator", "")).lower())
            if op is None:
                continue                                  # K3
            if e.get("key") not in known:
                return None                               # K2
            if op in (In, NotIn):
                out.append((e["key"], op(e.get("values") or [])))
            else:
                out.append((e["key"], op()))
    labels = selector.get("matchLabels")
    if labels is not None:
        for k, v in labels.items():
            if k not in known:
                return None                               # K2
            # a plain kano value: key present and equal (Python ==), one
            # shared value column per key rather than a requirement column
            # per term; kano's quirk Q1 cannot fire, some pod carries the key
            out.append((k, v))
    return out


class _TermDict:
    """Terms of one kano selector dict: a key may carry several requirements
    (matchLabels and matchExpressions on one key, or the pod side and the
    namespace side), so repeats go to alias columns holding the same values."""

    def __init__(self, aliases: Dict[Any, Any]):
        self.d: Dict[Any, Any] = {}
        self.aliases = aliases

    def add(self, col, req) -> None:
        key, t = col, 0
        while key in self.d:
            t += 1
            key = ("__alias__", col, t)
            self.aliases[key] = col
        self.d[key] = req


class K8sReachability:
    """kubesv's relations over one cluster, resident on the device."""

    def __init__(self, edge, ingress_traffic, egress_traffic, selected_by_any, info):
        #: edge[src, dst] (constraint.py:229-231), a ReachabilityMatrix
        self.edge = edge
        #: ingress_traffic as [sel, src] and egress_traffic as [sel, dst]
        #: (constraint.py:191-227; the product's two operands)
        self.ingress_traffic = ingress_traffic
        self.egress_traffic = egress_traffic
        #: selected_by_any per pod (constraint.py:179-182), None unless
        #: check_select_by_no_policy asked for it
        self.selected_by_any = selected_by_any
        self.info = info

    def path(self, mode: str = "auto") -> ReachabilityMatrix:
        """path :- edge | edge . edge (constraint.py:233-237)."""
        from .algorithm import two_hop
        return two_hop(self.edge, mode=mode)


def _wrap(engine, n: int) -> ReachabilityMatrix:
    m = ReachabilityMatrix.__new__(ReachabilityMatrix)
    m.container_size = n
    m._engine = engine
    m._containers = None
    m._policies = None
    m._ncontainers = n
    m._lists = None
    return m


def compile_policies(pods: List[Pod], policies: List[NetworkPolicy],
                     namespaces: List[Namespace]):
    """kubesv's facts (constraint.py:242-282) as kano objects: the pods as
    Containers (own labels, namespace, namespace labels, alias columns) and
    three kano policy lists -- ingress peers, egress peers (select = the
    policy's pod selector and namespace, allow = the peer; egress direction,
    so that M[sel][peer pod]) and the bare pod selectors."""
    nam_map = {ns.name: i for i, ns in enumerate(namespaces)}
    by_name = {ns.name: ns for ns in namespaces}
    # define_pod_facts (constraint.py:242-275): the label keys any pod / any
    # namespace carries are the relations a selector may name
    pod_keys, ns_keys = set(), set()
    for p in pods:
        if p.namespace not in nam_map:
            raise KeyError(p.namespace)                  # K7
        pod_keys.update(p.labels.keys())
    for ns in namespaces:
        ns_keys.update(ns.labels.keys())
    # namespace label keys some pod sees (through its namespace)
    ns_pod_keys = set()
    for name in {p.namespace for p in pods}:
        ns_pod_keys.update(by_name[name].labels.keys())

    aliases: Dict[Any, Any] = {}
    ing, egr, sel_only = [], [], []
    for pol in policies:
        spec = pol.spec
        if spec is None:
            raise AttributeError("'NoneType' object has no attribute 'egress'")
        # define_pod_selector (model.py:496-514)
        sel = None
        if pol.namespace in nam_map:
            t = _terms(spec.get("podSelector"), pod_keys)
            if t is not None:
                sel = _TermDict(aliases)
                sel.add(_NS, pol.namespace)
                for k, r in t:
                    sel.add(k, r)
        # define_egress_rules, then define_ingress_rules (constraint.py:278-282)
        for direction, out in (("egress", egr), ("ingress", ing)):
            rules = spec.get(direction)
            if direction == "ingress" and spec.get("egress") is None:
                continue                                  # K4
            if rules is None:
                if direction == "ingress":
                    raise TypeError("'NoneType' object is not iterable")   # K4
                continue
            for rule in rules:
                peers = (rule or {}).get("to" if direction == "egress" else "from")
                if peers is None:
                    raise TypeError("'NoneType' object is not iterable")   # K4
                for peer in peers:
                    peer = peer or {}
                    nst = _terms(peer.get("namespaceSelector"), ns_keys)
                    if nst is None:
                        continue                          # K2
                    pt = _terms(peer.get("podSelector"), pod_keys)
                    if pt is None:
                        continue                          # K2
                    if sel is None:
                        continue                          # selects nothing
                    if any(not isinstance(r, LabelExpression) and k not in ns_pod_keys
                           for k, r in nst):
                        continue      # no pod lives in a namespace with the key
                    alw = _TermDict(aliases)
                    for k, r in nst:
                        alw.add(("__k8s_ns_label__", k), r)
                    for k, r in pt:
                        alw.add(k, r)
                    out.append((sel.d, alw.d))
        if sel is not None:
            sel_only.append((sel.d, {}))

    containers = []
    for p in pods:
        lab = dict(p.labels)
        lab[_NS] = p.namespace
        for k, v in by_name[p.namespace].labels.items():
            lab[("__k8s_ns_label__", k)] = v
        for a, col in aliases.items():
            if col in lab:
                lab[a] = lab[col]
        containers.append(Container(p.name, lab))

    def kano(pairs):
        return [Policy(f"k8s{q}", PolicySelect(s), PolicyAllow(a), PolicyEgress, None)
                for q, (s, a) in enumerate(pairs)]
    return containers, kano(ing), kano(egr), kano(sel_only)


def build(pods: List[Pod], policies: List[NetworkPolicy], namespaces: List[Namespace],
          check_self_ingress_traffic: bool = True, check_select_by_no_policy: bool = False,
          device: int = 0, path: str = "auto", form: str = "classes",
          rows: Optional[tuple] = None, self_term: str = "auto") -> K8sReachability:
    """kubesv's ``build`` (constraint.py:285-299) on the device: the edge
    relation as an n x n matrix (rows src, columns dst).  ``form``: the
    product over the builds' row / column classes ("classes") or over pods
    ("pods"); both give the same matrix.  ``rows=(r0, r1)``: only those rows
    of the edge matrix (a multi-GPU rank's shard; the class form).
    ``self_term``: "expand" (from the egress classes), "build" (the
    destination is a build of the egress policies) or "auto"."""
    from ._engine import DeviceBuild
    from ._intern import intern
    containers, ing, egr, sel_only = compile_policies(pods, policies, namespaces)
    n = len(pods)

    def operand(pols):
        b = DeviceBuild(intern(containers, pols), device=device, path=path, build=False)
        b.build_classes(path)          # Mc and classes; M written only if read
        return b

    in_t = operand(ing)
    eg_t = operand(egr)
    selected = None
    all_pairs = False
    if check_select_by_no_policy:
        # a pod is selected by some policy iff its row class's S(c) is not
        # empty: the class-level build only (no matrix is written or
        # allocated, whatever n and rows are)
        selected = np.zeros(n, dtype=bool)
        if n:
            ms = DeviceBuild(intern(containers, sel_only), device=device, path=path,
                             build=False)
            ms.build_classes(path)
            off, _ = ms.select_csr()
            selected = np.diff(off)[ms.classes()] > 0
            ms.close()
        all_pairs = bool(n) and not bool(selected.all())
    # the self term: expanded from the egress classes ("expand", the
    # default), or the destination is a build of the egress policies over its
    # rows, whose matrix write is the term ("build"; measured 0.89 vs 2.4 ms
    # at 100k pods, and 26-29 vs 22-428 ms for 1M pods' rank 0 of 8, where
    # the destination's 15.6 GB allocation inside the call varies widely)
    big = self_term == "build"
    in_place = (bool(check_self_ingress_traffic) and not all_pairs and form == "classes"
                and n > 0 and big)
    if in_place:
        # the destination is a build of the egress policies over its rows:
        # its matrix write is the self term (EgT's rows), the product is
        # OR-ed into it
        out = DeviceBuild(eg_t.tables, device=device, rows=rows, path=path)
    else:
        out = DeviceBuild.empty(n, device=device, rows=rows)
    added = out.k8s_edge_from(in_t, eg_t, bool(check_self_ingress_traffic), all_pairs,
                              pods=(form == "pods"), dst_is_egress=in_place)
    info = {"ingress_policies": len(ing), "egress_policies": len(egr),
            "product_bits": added, "all_pairs": all_pairs, "rows": rows}
    return K8sReachability(_wrap(out, n), _wrap(in_t, n), _wrap(eg_t, n), selected, info)


# ---------------------------------------------------------------------------
# The conformant reading (networking.k8s.io/v1): what a cluster enforces.
#
# Policy P of namespace N selects the pods of N matching spec.podSelector.
# Its types are spec.policyTypes as listed, or -- absent -- Ingress plus Egress
# iff the spec has an ``egress`` key.  A pod is egress-isolated iff some
# Egress-typed policy selects it (ingress likewise); isolation never depends
# on rules or ports.  A rule with an absent or empty ``from`` / ``to`` matches
# every pod; a peer's bare podSelector stays in N, a bare namespaceSelector
# takes every pod of the matching namespaces, both narrow each other, a peer
# with neither selector is every pod of N and an ipBlock peer is no pod.
#   allowed[s, d] = (allow_self and s == d)
#                   or ((not isoE[s] or E[s, d]) and (not isoI[d] or I[d, s]))
# Selectors AND matchLabels and matchExpressions (In, NotIn, Exists,
# DoesNotExist; anything else is a ValueError); a term on a key no pod (no
# namespace a pod lives in) carries is resolved here, before the engine sees
# it: matchLabels / In / Exists match nothing, NotIn / DoesNotExist always
# hold -- so neither kano's quirk Q1 nor kubesv's quick fail (K2) applies.
#
# Out of scope: named ports (a string ``port`` never matches a numeric query),
# ipBlock reachability (the matrix is pod to pod), AdminNetworkPolicy
# (kano.algorithm.verdict_matrix is the tool for tiers), host-network pods and
# sources with incremental updates (the two builds are made here, once).
# ---------------------------------------------------------------------------

_CONF_OPS = {"In": In, "NotIn": NotIn, "Exists": Exists, "DoesNotExist": DoesNotExist}
_NS_LABEL = "__k8s_ns_label__"


def _conformant_terms(selector: Optional[Dict[str, Any]], known: set) -> Optional[List[tuple]]:
    """The (key, requirement) terms of a selector over the keys in ``known``,
    or None when it matches nothing.  Terms on other keys are resolved here."""
    if not selector:
        return []
    out, nothing = [], False
    for e in selector.get("matchExpressions") or []:
        name = (e or {}).get("operator")
        op = _CONF_OPS.get(name) if isinstance(name, str) else None
        if op is None:
            raise ValueError(f"matchExpressions operator {name!r}: expected In, NotIn, Exists "
                             "or DoesNotExist")
        key = e.get("key")
        if key not in known:
            nothing = nothing or op in (In, Exists)       # NotIn / DoesNotExist: always true
        elif op in (In, NotIn):
            out.append((key, op(e.get("values") or [])))
        else:
            out.append((key, op()))
    for k, v in (selector.get("matchLabels") or {}).items():
        if k not in known:
            nothing = True
        else:
            out.append((k, v))
    return None if nothing else out


def policy_types(spec: Dict[str, Any]) -> List[str]:
    """spec.policyTypes as listed; absent: Ingress, plus Egress iff the spec
    has an ``egress`` key."""
    types = spec.get("policyTypes")
    if types is None:
        types = ["Ingress"] + (["Egress"] if "egress" in spec else [])
    return list(types)


def rule_counts(ports, port) -> bool:
    """Whether a rule with this ``ports`` list counts for the query ``port``
    (None: every rule counts -- an upper bound over ports; else (protocol,
    number)).  An entry's protocol defaults to TCP; a named port (a string)
    never matches."""
    if port is None or not ports:
        return True
    protocol, number = port
    for e in ports:
        e = e or {}
        if (e.get("protocol") or "TCP") != protocol:
            continue
        p, end = e.get("port"), e.get("endPort")
        if p is None:
            return True
        if isinstance(p, str):
            continue
        if (p <= number <= end) if end is not None else p == number:
            return True
    return False


def _port_query(port):
    if port is None:
        return None
    protocol, number = port
    if not isinstance(protocol, str) or isinstance(number, (str, bool)):
        raise ValueError("port must be None or (protocol, number)")
    return protocol, int(number)


class Conformant:
    """compile_conformant's result: the pods as Containers, the two kano
    policy lists (egress: E[src][dst]; ingress: I[dst][src]; select = the
    policy's namespace and podSelector, allow = one peer), and per list entry
    its ``origin`` (policy index, direction, rule index, peer index -- the peer
    index None for a rule matching every pod, both None for the entry that
    only isolates) and the rule's ``ports``."""

    def __init__(self, containers, egress, ingress, origin_egress, origin_ingress,
                 ports_egress, ports_ingress):
        self.containers = containers
        self.egress, self.ingress = egress, ingress
        self.origin_egress, self.origin_ingress = origin_egress, origin_ingress
        self.ports_egress, self.ports_ingress = ports_egress, ports_ingress

    def keep(self, port):
        """The keep masks (egress, ingress) of a port query: None for every
        entry, else uint8 flags, one per entry."""
        port = _port_query(port)
        if port is None:
            return None, None
        return tuple(np.array([rule_counts(p, port) for p in ports], dtype=np.uint8)
                     for ports in (self.ports_egress, self.ports_ingress))


def compile_conformant(pods: List[Pod], policies: List[NetworkPolicy],
                       namespaces: List[Namespace]) -> Conformant:
    """The conformant reading as kano objects (see the section's comment).
    Every policy of a type that selects a pod-bearing selector contributes at
    least one entry per type, so "selected by some entry" is "isolated": a
    policy of a type whose rules allow nothing gets one entry whose allow side
    no pod meets (DoesNotExist on the namespace column, which every pod
    carries).  A policy whose selector matches nothing isolates nobody and is
    dropped; so is a peer that matches nothing."""
    nam_map = {ns.name: i for i, ns in enumerate(namespaces)}
    by_name = {ns.name: ns for ns in namespaces}
    pod_keys = set()
    for p in pods:
        if p.namespace not in nam_map:
            raise KeyError(p.namespace)
        pod_keys.update(p.labels.keys())
    ns_pod_keys = set()                  # namespace label keys some pod sees
    for name in {p.namespace for p in pods}:
        ns_pod_keys.update(by_name[name].labels.keys())

    aliases: Dict[Any, Any] = {}
    lists = {"egress": [], "ingress": []}
    origin = {"egress": [], "ingress": []}
    ports = {"egress": [], "ingress": []}
    for pi, pol in enumerate(policies):
        spec = pol.spec or {}
        types = policy_types(spec)
        st = _conformant_terms(spec.get("podSelector"), pod_keys)
        sel = None
        if st is not None and pol.namespace in nam_map:
            sel = _TermDict(aliases)
            sel.add(_NS, pol.namespace)
            for k, r in st:
                sel.add(k, r)
        for direction, typ, side in (("egress", "Egress", "to"), ("ingress", "Ingress", "from")):
            if typ not in types:
                continue
            entries = []                 # (allow terms, rule index, peer index, ports)
            for ri, rule in enumerate(spec.get(direction) or []):
                rule = rule or {}
                peers = rule.get(side)
                if not peers:
                    entries.append(({}, ri, None, rule.get("ports")))
                    continue
                for pj, peer in enumerate(peers):
                    peer = peer or {}
                    nsel, psel = peer.get("namespaceSelector"), peer.get("podSelector")
                    nst = _conformant_terms(nsel, ns_pod_keys)
                    pt = _conformant_terms(psel, pod_keys)
                    if peer.get("ipBlock") is not None or nst is None or pt is None:
                        continue         # no pod
                    alw = _TermDict(aliases)
                    if nsel is None:
                        alw.add(_NS, pol.namespace)
                    for k, r in nst:
                        alw.add((_NS_LABEL, k), r)
                    for k, r in pt:
                        alw.add(k, r)
                    entries.append((alw.d, ri, pj, rule.get("ports")))
            if sel is None:
                continue                 # selects nothing: isolates nobody
            if not entries:
                entries.append(({_NS: DoesNotExist()}, None, None, None))
            for alw, ri, pj, rp in entries:
                lists[direction].append((sel.d, alw))
                origin[direction].append((pi, direction, ri, pj))
                ports[direction].append(rp)

    containers = []
    for p in pods:
        lab = dict(p.labels)
        lab[_NS] = p.namespace
        for k, v in by_name[p.namespace].labels.items():
            lab[(_NS_LABEL, k)] = v
        for a, col in aliases.items():
            if col in lab:
                lab[a] = lab[col]
        containers.append(Container(p.name, lab))

    def kano(pairs):
        return [Policy(f"k8s{q}", PolicySelect(s), PolicyAllow(a), PolicyEgress, None)
                for q, (s, a) in enumerate(pairs)]
    return Conformant(containers, kano(lists["egress"]), kano(lists["ingress"]),
                      origin["egress"], origin["ingress"], ports["egress"], ports["ingress"])


class K8sConnectivity:
    """The conformant reading of one cluster, resident on the device."""

    def __init__(self, allowed, egress, ingress, compiled, policies, port, allow_self, info,
                 isolated, device, rows, form="auto"):
        #: allowed[src, dst], a ReachabilityMatrix: every kano.algorithm query reads it
        self.allowed = allowed
        #: the wrapped class-level builds: E[src][dst] and I[dst][src]
        self.egress, self.ingress = egress, ingress
        #: per pod: some Egress-typed (Ingress-typed) policy selects it
        self.egress_isolated, self.ingress_isolated = isolated
        #: per entry of the builds: (policy index, direction, rule index, peer index)
        self.origin_egress = compiled.origin_egress
        self.origin_ingress = compiled.origin_ingress
        self.port = port
        self.allow_self = allow_self
        self.info = info
        self._compiled, self._policies, self._device, self._rows = compiled, policies, device, rows
        self._form = form

    def on_port(self, port) -> "K8sConnectivity":
        """The same cluster on another port: a new keep mask over the two
        resident builds and one kano_k8s_conn -- nothing is interned or
        uploaded again."""
        return _connect(self.egress, self.ingress, self._compiled, self._policies, port,
                        self.allow_self, (self.egress_isolated, self.ingress_isolated),
                        self._device, self._rows, self._form)

    def explain(self, src: int, dst: int) -> dict:
        """Why src may (not) talk to dst on this object's port: ``allowed``,
        ``self`` (the pair is allowed as self traffic) and per direction
        ``isolated`` and ``policies`` -- the (policy name, rule index, peer
        index) of the counted rules allowing the pair (kano_pair_policies on
        the two builds, filtered by the port's keep mask).  ``blocked_by``
        names the directions that block the pair."""
        src, dst = int(src), int(dst)
        n = self.allowed.container_size
        if not (0 <= src < n and 0 <= dst < n):
            raise IndexError("bitarray index out of range")
        keep = self._compiled.keep(self.port)
        out = {"self": bool(self.allow_self and src == dst), "blocked_by": []}
        for direction, m, pair, iso, org, kp in (
                ("egress", self.egress, (src, dst), self.egress_isolated,
                 self.origin_egress, keep[0]),
                ("ingress", self.ingress, (dst, src), self.ingress_isolated,
                 self.origin_ingress, keep[1])):
            ids = []
            if org:
                r = m.engine.pair_policies([pair], lists=True)
                ids = r["policies"][r["offsets"][0]:r["offsets"][1]].tolist()
            pols = [(self._policies[org[p][0]].name, org[p][2], org[p][3]) for p in ids
                    if kp is None or kp[p]]
            isolated = bool(iso[pair[0]])
            out[direction] = {"isolated": isolated, "policies": pols}
            if isolated and not pols:
                out["blocked_by"].append(direction)
        out["allowed"] = out["self"] or not out["blocked_by"]
        return out


def _connect(egress, ingress, compiled, policies, port, allow_self, isolated, device, rows,
             form="auto"):
    from ._engine import DeviceBuild
    n = len(compiled.containers)
    port = _port_query(port)
    keep_e, keep_i = compiled.keep(port)
    out = DeviceBuild.empty(n, device=device, rows=rows)
    # (the isolated pods are known from the builds: no counting on the device)
    out.k8s_conn_from(egress.engine, ingress.engine, allow_self, keep_e, keep_i, form,
                      counts=False)
    info = {"egress_entries": len(compiled.egress), "ingress_entries": len(compiled.ingress),
            "kept_egress_entries": (len(compiled.egress) if keep_e is None
                                    else int(np.count_nonzero(keep_e))),
            "kept_ingress_entries": (len(compiled.ingress) if keep_i is None
                                     else int(np.count_nonzero(keep_i))),
            "egress_isolated": int(np.count_nonzero(isolated[0])),
            "ingress_isolated": int(np.count_nonzero(isolated[1])),
            "port": port, "allow_self": bool(allow_self), "rows": rows}
    return K8sConnectivity(_wrap(out, n), egress, ingress, compiled, policies, port,
                           bool(allow_self), info, isolated, device, rows, form)


def connectivity(pods: List[Pod], policies: List[NetworkPolicy], namespaces: List[Namespace],
                 port=None, allow_self: bool = True, device: int = 0, path: str = "auto",
                 rows: Optional[tuple] = None, form: str = "auto") -> K8sConnectivity:
    """The connectivity a cluster enforces (networking.k8s.io/v1) as an n x n
    matrix on the device (rows src, columns dst).  ``port``: None -- every
    rule counts whatever its ports, an upper bound over ports -- or
    (protocol, number).  ``allow_self``: a pod always reaches itself.
    ``rows=(r0, r1)``: only those rows (a multi-GPU rank's shard).  ``form``:
    how the rows are written -- "direct" (gathered from the two class-level
    tables), "stream" (the tables' class rows expanded once, then streamed) or
    "auto" (streamed when the class rows are few beside the rows); the same
    bits."""
    from ._engine import DeviceBuild
    from ._intern import intern
    if form not in ("auto", "direct", "stream"):
        raise ValueError(f"form must be 'auto', 'direct' or 'stream', not {form!r}")
    policies = list(policies)
    compiled = compile_conformant(pods, policies, namespaces)

    def operand(pols):
        b = DeviceBuild(intern(compiled.containers, pols), device=device, path=path, build=False)
        b.build_classes(path)          # the class tables only: M is never written
        return b

    eg, ing = operand(compiled.egress), operand(compiled.ingress)
    isolated = (eg.k8s_isolated(), ing.k8s_isolated())
    n = len(pods)
    return _connect(_wrap(eg, n), _wrap(ing, n), compiled, policies, port, allow_self, isolated,
                    device, rows, form)


_NS_NAME_LABEL = "kubernetes.io/metadata.name"


def load_manifests(paths):
    """(pods, policies, namespaces) from files or directories (their *.yaml,
    *.yml and *.json files, sorted) of multi-document YAML: kinds Pod,
    Namespace, NetworkPolicy and the items of a ``List``; other kinds are
    ignored.  A namespace that is referenced but not declared is created, and
    every namespace gets the ``kubernetes.io/metadata.name`` label if it lacks
    it."""
    import os
    import yaml
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    files = []
    for p in paths:
        p = os.fspath(p)
        if os.path.isdir(p):
            for root, dirs, names in os.walk(p):
                dirs.sort()
                files += [os.path.join(root, f) for f in sorted(names)
                          if f.endswith((".yaml", ".yml", ".json"))]
        else:
            files.append(p)
    pods, pols, nss = [], [], {}

    def take(obj):
        if not isinstance(obj, dict):
            return
        kind = obj.get("kind")
        if isinstance(kind, str) and kind.endswith("List") and isinstance(obj.get("items"), list):
            for it in obj["items"]:
                take(it)
        elif kind == "Pod":
            pods.append(from_dict("Pod", obj))
        elif kind == "NetworkPolicy":
            pols.append(from_dict("NetworkPolicy", obj))
        elif kind == "Namespace":
            ns = from_dict("Namespace", obj)
            nss[ns.name] = ns

    for f in files:
        with open(f) as fh:
            for doc in yaml.safe_load_all(fh):
                take(doc)
    for o in pods + pols:
        if o.namespace not in nss:
            nss[o.namespace] = Namespace(o.namespace)
    for ns in nss.values():
        ns.labels.setdefault(_NS_NAME_LABEL, ns.name)
    return pods, pols, list(nss.values())
