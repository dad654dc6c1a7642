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

import collections
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


class AdminNetworkPolicy:
    """An AdminNetworkPolicy (policy.networking.k8s.io/v1alpha1, cluster
    scoped) over its spec dict in the manifest's camelCase: ``priority``,
    ``subject`` and ``ingress`` / ``egress`` rules ``{action, from / to,
    ports}``; the conformant reading's admin tier."""

    def __init__(self, name: str, spec: Optional[Dict[str, Any]] = None):
        self.name = name
        self.spec = spec

    @classmethod
    def from_manifest(cls, obj: Dict[str, Any]):
        return cls((obj.get("metadata") or {}).get("name"), obj.get("spec"))


class BaselineAdminNetworkPolicy(AdminNetworkPolicy):
    """The cluster's one BaselineAdminNetworkPolicy: ``subject`` and rules as
    an AdminNetworkPolicy's, no priority, actions Allow and Deny."""


def from_dict(kind: str, data: Dict[str, Any]):
    """kubesv.parser.from_dict (kubesv/kubesv/parser.py:9-18) without the
    kubernetes client: a manifest dict as this module's Pod / Namespace /
    NetworkPolicy (kind 'V1Pod', 'V1Namespace', 'V1NetworkPolicy'; the 'V1'
    prefix is optional), or AdminNetworkPolicy / BaselineAdminNetworkPolicy."""
    k = kind[2:] if kind.startswith("V1") else kind
    md = (data or {}).get("metadata") or {}
    if k == "Pod":
        return Pod(md.get("name"), md.get("namespace"), md.get("labels"))
    if k == "Namespace":
        return Namespace(md.get("name"), md.get("labels"))
    if k == "NetworkPolicy":
        return NetworkPolicy.from_manifest(data)
    if k == "AdminNetworkPolicy":
        return AdminNetworkPolicy.from_manifest(data or {})
    if k == "BaselineAdminNetworkPolicy":
        return BaselineAdminNetworkPolicy.from_manifest(data or {})
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
#
# With AdminNetworkPolicies (``admin``) and a BaselineAdminNetworkPolicy
# (``baseline``; policy.networking.k8s.io/v1alpha1) each direction D of a
# subject pod x and a peer pod y (egress: x = src, y = dst; ingress: x = dst,
# y = src) is read in three tiers:
#   1 the D rules of all ANPs ordered by (spec.priority, position in ``admin``,
#     rule index); a rule matches iff spec.subject selects x, one of its peers
#     (``from`` / ``to``) selects y and it counts for the port.  The first
#     matching rule decides: Allow, Deny, or Pass (on to 2, like no match);
#   2 if some NetworkPolicy of type D selects x: the reading above;
#   3 else the baseline's D rules in order, the first match decides, Allow or
#     Deny; no match, or no baseline: allowed.
#   allowed[s, d] = (allow_self and s == d) or (egress(s, d) and ingress(d, s))
# ``subject`` and a peer are ``namespaces: <selector>`` (the pods of the
# matching namespaces) or ``pods: {namespaceSelector, podSelector}`` (both
# match); ``nodes`` / ``networks`` / ``domainNames`` peers select no pod.  Ports:
# ``portNumber: {protocol, port}``, ``portRange: {protocol, start, end}``,
# ``namedPort`` never matches, no ``ports`` counts for every port.  Equal
# priorities (undefined upstream) fall back to the position in ``admin``.
#
# ``K8sConnectivity.explain`` says for one pair which tier and rule decided
# each direction; ``pair_verdicts`` says it for millions of pairs a call, on the
# device (kano_k8s_pair_verdicts), with or without admin tiers.
#
# Out of scope: named ports (a string ``port`` / ``namedPort`` never matches a
# numeric query), ipBlock reachability and the ``nodes`` / ``networks`` /
# ``domainNames`` peers (the matrix is pod to pod), host-network pods and sources
# with incremental updates (the two builds are made here, once).
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


def admin_rule_counts(ports, port) -> bool:
    """rule_counts for an AdminNetworkPolicy / baseline rule's ``ports``:
    ``portNumber: {protocol, port}``, ``portRange: {protocol, start, end}``;
    ``namedPort`` never matches."""
    if port is None or not ports:
        return True
    protocol, number = port
    for e in ports:
        e = e or {}
        pn, pr = e.get("portNumber"), e.get("portRange")
        if pn is not None and (pn.get("protocol") or "TCP") == protocol \
                and pn.get("port") == number:
            return True
        if pr is not None and (pr.get("protocol") or "TCP") == protocol \
                and pr.get("start") <= number <= pr.get("end"):
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
                 ports_egress, ports_ingress, tiers_egress=None, tiers_ingress=None,
                 np_level=(0, 0), tiered=False, admin_priority_ties=0):
        self.containers = containers
        self.egress, self.ingress = egress, ingress
        self.origin_egress, self.origin_ingress = origin_egress, origin_ingress
        self.ports_egress, self.ports_ingress = ports_egress, ports_ingress
        #: per entry (kind, level, action): kind "admin" / "network" /
        #: "baseline" says which list origin's policy index points into (0 for
        #: the baseline); a level is one rule -- the admin rules of the
        #: direction in evaluation order, then np_level, the one level of all
        #: NetworkPolicy entries, then the baseline's rules; action "Allow" /
        #: "Deny" / "Pass", or "Isolate" for the NetworkPolicy entry that only
        #: isolates
        network = lambda org: [("network", 0, "Allow" if o[2] is not None else "Isolate")  # noqa: E731
                               for o in org]
        self.tiers_egress = network(origin_egress) if tiers_egress is None else tiers_egress
        self.tiers_ingress = network(origin_ingress) if tiers_ingress is None else tiers_ingress
        #: the NetworkPolicy tier's level (egress, ingress) = the admin rules of the direction
        self.np_level = tuple(np_level)
        #: admin or baseline policies were compiled in: connectivity takes the tiered path
        self.tiered = tiered
        self.admin_priority_ties = admin_priority_ties

    def codes(self, port):
        """The per-entry codes (egress, ingress) of a port query, uint32:
        level * 4 + action (0 allow, 1 deny, 2 pass, 3 isolates only) --
        kano_k8s_conn_tiers' input.  An admin or baseline entry whose rule
        does not count on the port is dropped (0xffffffff); a NetworkPolicy
        entry's still isolates (action 3)."""
        port = _port_query(port)
        out = []
        for tiers, ports in ((self.tiers_egress, self.ports_egress),
                             (self.tiers_ingress, self.ports_ingress)):
            code = np.empty(len(tiers), dtype=np.uint32)
            for q, ((kind, level, action), rp) in enumerate(zip(tiers, ports)):
                if kind == "network":
                    act = 0 if action == "Allow" and rule_counts(rp, port) else 3
                elif admin_rule_counts(rp, port):
                    act = _ACTIONS[action]
                else:
                    code[q] = 0xFFFFFFFF
                    continue
                code[q] = level * 4 + act
            out.append(code)
        return tuple(out)

    def keep(self, port):
        """The keep masks (egress, ingress) of a port query: None for every
        entry, else uint8 flags, one per entry."""
        port = _port_query(port)
        if port is None:
            return None, None
        return tuple(np.array([rule_counts(p, port) for p in ports], dtype=np.uint8)
                     for ports in (self.ports_egress, self.ports_ingress))


_ACTIONS = {"Allow": 0, "Deny": 1, "Pass": 2}
_NO_POD_PEERS = ("nodes", "networks", "domainNames")


def _admin_terms(obj, what: str, ns_pod_keys: set, pod_keys: set, aliases, peer: bool):
    """An AdminNetworkPolicy ``subject`` or peer as one kano selector dict, or
    None when it selects no pod."""
    obj = obj or {}
    if peer and any(obj.get(k) is not None for k in _NO_POD_PEERS):
        if "namespaces" in obj or "pods" in obj:
            raise ValueError(f"{what}: more than one of namespaces / pods / "
                             f"{' / '.join(_NO_POD_PEERS)}")
        return None
    if ("namespaces" in obj) == ("pods" in obj):
        raise ValueError(f"{what}: exactly one of namespaces / pods expected")
    if "namespaces" in obj:
        nst, pt = _conformant_terms(obj["namespaces"], ns_pod_keys), []
    else:
        pd = obj["pods"] or {}
        nst = _conformant_terms(pd.get("namespaceSelector"), ns_pod_keys)
        pt = _conformant_terms(pd.get("podSelector"), pod_keys)
    if nst is None or pt is None:
        return None
    d = _TermDict(aliases)
    for k, r in nst:
        d.add((_NS_LABEL, k), r)
    for k, r in pt:
        d.add(k, r)
    return d.d


def _admin_entries(pol, kind: str, actions, ns_pod_keys, pod_keys, aliases):
    """The entries of one AdminNetworkPolicy (or the baseline) per direction:
    {direction: [per rule: (action, ports, [(peer index, select, allow)])]},
    one entry per pod-bearing peer; a subject selecting no pod leaves the
    rules without entries (they keep their levels)."""
    who = f"{kind} {pol.name!r}"
    spec = pol.spec or {}
    sel = _admin_terms(spec.get("subject"), f"{who}: subject", ns_pod_keys, pod_keys, aliases,
                       peer=False)
    out = {}
    for direction, side in (("egress", "to"), ("ingress", "from")):
        rules = []
        for ri, rule in enumerate(spec.get(direction) or []):
            rule = rule or {}
            at = f"{who}: {direction} rule {ri}"
            action = rule.get("action")
            if action not in actions:
                raise ValueError(f"{at}: action {action!r}, expected one of "
                                 f"{' / '.join(actions)}")
            peers = rule.get(side)
            if not isinstance(peers, list) or not peers:
                raise ValueError(f"{at}: a non-empty {side!r} list is required")
            entries = []
            for pj, peer in enumerate(peers):
                alw = _admin_terms(peer, f"{at}: peer {pj}", ns_pod_keys, pod_keys, aliases,
                                   peer=True)
                if alw is not None and sel is not None:
                    entries.append((pj, sel, alw))
            rules.append((action, rule.get("ports"), entries))
        out[direction] = rules
    return out


def compile_conformant(pods: List[Pod], policies: List[NetworkPolicy],
                       namespaces: List[Namespace], admin=None, baseline=None) -> Conformant:
    """The conformant reading as kano objects (see the section's comment).
    ``admin`` (AdminNetworkPolicy objects) and ``baseline`` (one
    BaselineAdminNetworkPolicy, or a list of at most one) add their rules to
    the same two lists, one entry per (rule, pod-bearing peer): select = the
    subject, allow = the peer; ``tiers_*`` says per entry which tier, level
    and action it carries.  Without them the result is the NetworkPolicy
    reading alone.
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
    tiers = {"egress": [], "ingress": []}

    def tier_entries(kind, pi, compiled, first_level):
        """One policy's rules appended from first_level[direction] on."""
        for direction, rules in compiled.items():
            for ri, (action, rp, entries) in enumerate(rules):
                for pj, sel, alw in entries:
                    lists[direction].append((sel, alw))
                    origin[direction].append((pi, direction, ri, pj))
                    ports[direction].append(rp)
                    tiers[direction].append((kind, first_level[direction] + ri, action))
            first_level[direction] += len(rules)

    admin = list(admin or [])
    if isinstance(baseline, (list, tuple)):
        if len(baseline) > 1:
            raise ValueError(f"{len(baseline)} BaselineAdminNetworkPolicies: a cluster has one")
        baseline = baseline[0] if baseline else None
    for pol in admin:
        prio = (pol.spec or {}).get("priority")
        if isinstance(prio, bool) or not isinstance(prio, int) or not 0 <= prio <= 1000:
            raise ValueError(f"admin {pol.name!r}: priority {prio!r}, expected an integer "
                             "in 0..1000")
    # the admin tier: the rules of a direction in (priority, position, rule) order
    level = {"egress": 0, "ingress": 0}
    for pi in sorted(range(len(admin)), key=lambda q: (admin[q].spec["priority"], q)):
        tier_entries("admin", pi, _admin_entries(admin[pi], "admin", tuple(_ACTIONS), ns_pod_keys,
                                                 pod_keys, aliases), level)
    np_level = (level["egress"], level["ingress"])
    prios = [a.spec["priority"] for a in admin]
    ties = len(prios) - len(set(prios))
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
                tiers[direction].append(("network", level[direction],
                                         "Allow" if ri is not None else "Isolate"))
    # the baseline tier: its rules in order, after the NetworkPolicy level
    if baseline is not None:
        tier_entries("baseline", 0, _admin_entries(baseline, "baseline", ("Allow", "Deny"),
                                                   ns_pod_keys, pod_keys, aliases),
                     {d: v + 1 for d, v in level.items()})

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
                      origin["egress"], origin["ingress"], ports["egress"], ports["ingress"],
                      tiers["egress"], tiers["ingress"], np_level,
                      tiered=bool(admin) or baseline is not None, admin_priority_ties=ties)


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
        uploaded again.  With tiers: new codes and one kano_k8s_conn_tiers."""
        if self._compiled.tiered:
            return _connect_tiers(self.egress, self.ingress, self._compiled, self._policies,
                                  port, self.allow_self, self._device, self._rows, self._form)
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
        if self._compiled.tiered:
            return self._explain_tiers(src, dst)
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

    def _explain_tiers(self, src: int, dst: int) -> dict:
        """explain with AdminNetworkPolicy tiers: per direction additionally
        ``tier`` ("admin" / "network" / "baseline" / "default"), ``verdict``
        ("allow" / "deny"), ``decider`` ((kind, policy name, rule index, peer
        index, action) or None) and -- where a Pass rule handed the pair down
        -- ``passed``, that rule named like a decider.  Resolved here from the
        entries matching the pair (kano_pair_policies) and the port's codes."""
        c = self._compiled
        codes = c.codes(self.port)
        out = {"self": bool(self.allow_self and src == dst), "blocked_by": []}
        for k, (direction, m, pair, iso, org, tiers) in enumerate((
                ("egress", self.egress, (src, dst), self.egress_isolated,
                 c.origin_egress, c.tiers_egress),
                ("ingress", self.ingress, (dst, src), self.ingress_isolated,
                 c.origin_ingress, c.tiers_ingress))):
            ids = []
            if org:
                r = m.engine.pair_policies([pair], lists=True)
                ids = r["policies"][r["offsets"][0]:r["offsets"][1]].tolist()
            code, np_level = codes[k], c.np_level[k]
            # the live matching entries in evaluation order: (code, id)
            live = sorted((int(code[p]), p) for p in ids if code[p] != 0xFFFFFFFF)

            def name(p):
                kind = tiers[p][0]
                return (kind, self._policies[kind][org[p][0]].name, org[p][2], org[p][3],
                        tiers[p][2])

            isolated = bool(iso[pair[0]])
            d = {"isolated": isolated,
                 "policies": [name(p)[1:4] for cd, p in live if cd == np_level * 4]}
            tier = verdict = decider = None
            if live and live[0][0] >> 2 < np_level:       # the first matching admin rule
                cd, p = live[0]
                if cd & 3 == 2:
                    d["passed"] = name(p)
                else:
                    tier, decider = "admin", name(p)
                    verdict = "allow" if cd & 3 == 0 else "deny"
            if tier is None and isolated:
                allow = [p for cd, p in live if cd == np_level * 4]
                tier, verdict = "network", "allow" if allow else "deny"
                decider = name(allow[0]) if allow else None
            if tier is None:
                tier, verdict = "default", "allow"
                for cd, p in live:
                    if cd >> 2 > np_level:
                        tier, decider = "baseline", name(p)
                        verdict = "allow" if cd & 3 == 0 else "deny"
                        break
            d.update(tier=tier, verdict=verdict, decider=decider)
            out[direction] = d
            if verdict == "deny":
                out["blocked_by"].append(direction)
        out["allowed"] = out["self"] or not out["blocked_by"]
        return out

    def pair_verdicts(self, pairs) -> "K8sPairVerdicts":
        """explain for many pairs at once: for every (src, dst) of ``pairs``
        (a (Q, 2) integer array or a list of tuples; any order, duplicates
        are fine) which tier and which rule decide each direction on this
        object's port, resolved on the device from the two resident builds
        and the port's codes (kano_k8s_pair_verdicts; one launch, millions of
        pairs a call).  Works with and without AdminNetworkPolicy tiers, and
        -- reading only the two full builds -- answers any pair of an object
        made with ``rows=``."""
        from ._engine import _as_pairs
        c = self._compiled
        n = len(c.containers)
        pr, Q = _as_pairs(pairs)
        if Q and (pr.min() < 0 or pr.max() >= n):
            raise IndexError("bitarray index out of range")
        code_e, code_i = c.codes(self.port)
        r = self.egress.engine.k8s_pair_verdicts(self.ingress.engine, pr, self.allow_self, code_e,
                                                 c.np_level[0], code_i, c.np_level[1])
        policies = self._policies if c.tiered else {"network": self._policies}
        return K8sPairVerdicts(r, c, policies)

    def rule_usage(self) -> "K8sRuleUsage":
        """Which rules do anything at all on this object's port, over every
        ordered pod pair: per entry the pairs it decides and the pairs it
        passes down, per NetworkPolicy rule the pairs only that rule allows
        (kano_k8s_rule_usage: one walk of the class lists, exact counts, no
        pair is enumerated).  With ``allow_self`` the n self pairs are left
        out: they are allowed before any rule is read.  Reads only the two
        full builds, so an object made with ``rows=`` answers the same.
        "Dead" is per port: a rule dead at ``port=None`` can be live on a port
        whose query drops the rule that shadows it."""
        c = self._compiled
        code_e, code_i = c.codes(self.port)
        (group_e, rules_e), (group_i, rules_i) = rule_groups(c)
        r = self.egress.engine.k8s_rule_usage(self.ingress.engine, self.allow_self, code_e,
                                              c.np_level[0], code_i, c.np_level[1], group_e,
                                              group_i)
        policies = self._policies if c.tiered else {"network": self._policies}
        return K8sRuleUsage(r, c, policies, (code_e, code_i), (group_e, group_i),
                            (rules_e, rules_i))

    def dead_rules(self, ports) -> List[tuple]:
        """The rules that are dead on every port of ``ports`` (None or
        (protocol, number) each): (direction, kind, policy name, rule index),
        in rule order.  One ``on_port`` and one ``rule_usage`` per port.
        Note: "dead" here means "counts on the port and still does nothing"
        (``K8sRuleUsage.dead_rules``).  A rule that some port's query drops
        decides nothing there either, but it is not dead there, so it is NOT
        returned: list only ports on which the rules in question count."""
        dead = None
        for port in ports:
            here = self.on_port(port).rule_usage().dead_rules()
            also = set(here)
            dead = here if dead is None else [r for r in dead if r in also]
        return dead or []


TIERS = ("default", "admin", "network", "baseline")
_COUNT_KEYS = ("allowed", "self") + tuple(
    f"{d}_{t}_{v}" for d in ("egress", "ingress") for t in TIERS for v in ("allow", "deny"))


class K8sPairVerdicts:
    """K8sConnectivity.pair_verdicts' result, arrays over the Q queried pairs:
    ``pairs`` (int32 (Q, 2): src, dst), ``allowed``, ``self_`` (bool) and per
    direction -- ``egress`` (subject src, peer dst) and ``ingress`` (subject
    dst, peer src) -- a K8sPairDirection.  ``counts``: the pairs allowed, the
    self pairs, and per direction, tier and verdict the pairs decided there
    (``egress_admin_deny``, ...)."""

    #: the names of the values of ``tier``
    TIERS = TIERS

    def __init__(self, r, compiled, policies):
        v = r["verdict"]
        self.pairs = r["pairs"]
        self.allowed = (v & 1).astype(bool)
        self.self_ = (v >> 1 & 1).astype(bool)
        self.egress = K8sPairDirection(v >> 2 & 3, (v >> 4 & 1).astype(bool), r["decider_e"],
                                       r["passed_e"], compiled.origin_egress,
                                       compiled.tiers_egress, policies)
        self.ingress = K8sPairDirection(v >> 5 & 3, (v >> 7 & 1).astype(bool), r["decider_i"],
                                        r["passed_i"], compiled.origin_ingress,
                                        compiled.tiers_ingress, policies)
        self.counts = dict(zip(_COUNT_KEYS, map(int, r["counts"])))

    def __len__(self):
        return len(self.allowed)

    def _direction(self, direction) -> "K8sPairDirection":
        if direction not in ("egress", "ingress"):
            raise ValueError(f"direction must be 'egress' or 'ingress', not {direction!r}")
        return getattr(self, direction)

    def _index(self, q) -> int:
        q = int(q)
        if not -len(self) <= q < len(self):
            raise IndexError("pair index out of range")
        return q

    def blocked_by(self, q: int) -> List[str]:
        """The directions that deny queried pair q (explain's ``blocked_by``;
        a self pair may be allowed all the same)."""
        q = self._index(q)
        return [d for d in ("egress", "ingress") if getattr(self, d).deny[q]]

    def name(self, direction: str, q: int):
        """The rule that decided ``direction`` of queried pair q: (kind, policy
        name, rule index, peer index, action) as explain's ``decider``, or
        None (the default tier, or a NetworkPolicy tier that denies)."""
        return self._direction(direction)._name("decider", self._index(q))

    def passed_name(self, direction: str, q: int):
        """The Pass rule that handed queried pair q down, named like a decider,
        or None."""
        return self._direction(direction)._name("passed", self._index(q))

    def blame(self, direction: str, deny_only: bool = True) -> Dict[tuple, int]:
        """{(kind, policy name, rule index): the queried pairs that rule
        decided} in ``direction``; ``deny_only``: over the denied pairs only.
        (A NetworkPolicy tier that denies has no deciding rule.)"""
        d = self._direction(direction)
        ids = d.decider[d.deny] if deny_only else d.decider
        per_id = np.bincount(ids[ids >= 0], minlength=len(d._origin))
        out: Dict[tuple, int] = {}
        for p in np.flatnonzero(per_id):
            key = d.entry(int(p))[:3]
            out[key] = out.get(key, 0) + int(per_id[p])
        return out


class K8sPairDirection:
    """One direction of K8sPairVerdicts: ``tier`` (uint8, an index into TIERS),
    ``deny`` (bool), ``decider`` and ``passed`` (int32: entries of the
    direction's build, -1 where there is none)."""

    def __init__(self, tier, deny, decider, passed, origin, tiers, policies):
        self.tier, self.deny, self.decider, self.passed = tier, deny, decider, passed
        self._origin, self._tiers, self._policies = origin, tiers, policies

    def tier_name(self, q: int) -> str:
        """The name of queried pair q's tier."""
        return TIERS[int(self.tier[q])]

    def entry(self, p: int):
        """(kind, policy name, rule index, peer index, action) of entry p of
        the direction's build."""
        kind, org = self._tiers[p][0], self._origin[p]
        return kind, self._policies[kind][org[0]].name, org[2], org[3], self._tiers[p][2]

    def _name(self, what: str, q: int):
        p = int(getattr(self, what)[q])
        return None if p < 0 else self.entry(p)


def rule_groups(compiled: Conformant):
    """Per direction (egress, ingress): (group, rules) -- ``group`` an int32
    per entry, one group per (kind, policy, rule) in entry order, and
    ``rules`` per group (kind, policy index, rule index, action, first entry,
    entries).  compile_conformant appends a rule's entries contiguously, so the
    groups are non-decreasing (asserted: kano_k8s_rule_usage relies on it).
    The entry of a NetworkPolicy that only isolates is a group of its own with
    rule index None."""
    out = []
    for origin, tiers in ((compiled.origin_egress, compiled.tiers_egress),
                          (compiled.origin_ingress, compiled.tiers_ingress)):
        group = np.empty(len(origin), dtype=np.int32)
        rules, seen, last = [], set(), None
        for p, (org, (kind, level, action)) in enumerate(zip(origin, tiers)):
            key = (kind, org[0], org[2])
            if key != last:
                assert key not in seen, f"the entries of rule {key} are not contiguous"
                seen.add(key)
                rules.append([kind, org[0], org[2], action, p, 0])
                last = key
            group[p] = len(rules) - 1
            rules[-1][5] += 1
        assert (np.diff(group) >= 0).all()
        out.append((group, [tuple(r) for r in rules]))
    return tuple(out)


K8sRuleRecord = collections.namedtuple(
    "K8sRuleRecord", "kind policy rule action on_port decided passed sole")


class K8sRuleDirection:
    """One direction of K8sRuleUsage: ``decided`` and ``passed`` (int64 per
    entry of the direction's build) and ``sole`` (int64 per rule, in the order
    of ``K8sRuleUsage.rules``; a rule = one group of ``group``)."""

    def __init__(self, decided, passed, sole, group):
        self.decided, self.passed, self.sole, self.group = decided, passed, sole, group


class K8sRuleUsage:
    """K8sConnectivity.rule_usage's result, counted over every ordered pod
    pair (x, y) -- without the n self pairs when the object allows self
    traffic -- per direction (``egress``: subject src, peer dst; ``ingress``:
    subject dst, peer src), a K8sRuleDirection each.
    ``counts``: per direction, tier and verdict the pairs decided there, named
    as K8sPairVerdicts.counts names them (``egress_default_allow`` ..
    ``ingress_baseline_deny``); a direction's eight sum to the pairs counted.
    decided == 0 and passed == 0: the rule is dead -- removing it changes no
    verdict on this port.  For a NetworkPolicy rule ``sole`` counts the pairs
    that rule alone allows in its tier: removing the rule (the policy keeping
    its types) denies exactly those pairs of that direction, so sole == 0 says
    the rule is redundant; sole <= decided summed over the rule's entries."""

    def __init__(self, r, compiled, policies, codes, groups, rules):
        self.egress = K8sRuleDirection(r["decided_e"], r["passed_e"], r["sole_e"], groups[0])
        self.ingress = K8sRuleDirection(r["decided_i"], r["passed_i"], r["sole_i"], groups[1])
        self.counts = dict(zip(_COUNT_KEYS[2:], map(int, r["tiers"])))
        self._policies = policies
        self._records = {}
        for direction, code, rl, np_level in (("egress", codes[0], rules[0], compiled.np_level[0]),
                                              ("ingress", codes[1], rules[1],
                                               compiled.np_level[1])):
            d = getattr(self, direction)
            G = len(rl)
            dec = np.zeros(G, np.int64)
            pas = np.zeros(G, np.int64)
            np.add.at(dec, d.group, d.decided)
            np.add.at(pas, d.group, d.passed)
            recs = []
            for g, (kind, pi, ri, action, first, cnt) in enumerate(rl):
                if action == "Isolate":
                    continue                    # not a rule: the policy's isolation alone
                cd = int(code[first])
                on_port = cd != 0xFFFFFFFF and (kind != "network" or cd == np_level * 4)
                recs.append(K8sRuleRecord(kind, policies[kind][pi].name, ri, action, on_port,
                                          int(dec[g]), int(pas[g]),
                                          int(d.sole[g]) if kind == "network" else None))
            self._records[direction] = recs

    def _direction(self, direction):
        if direction not in ("egress", "ingress"):
            raise ValueError(f"direction must be 'egress' or 'ingress', not {direction!r}")
        return self._records[direction]

    def rules(self, direction: str) -> List[K8sRuleRecord]:
        """One record per compiled rule of ``direction``, in entry order:
        (kind, policy name, rule index, action, on_port, decided, passed,
        sole).  ``on_port`` is False for a rule the port's query drops;
        ``sole`` is None outside the NetworkPolicy tier.  The entries that only
        isolate are not rules and are not listed, nor are rules without a
        compiled entry (ipBlock-only peers, selectors no pod can meet)."""
        return list(self._direction(direction))

    def blame(self, direction: str, deny_only: bool = True) -> Dict[tuple, int]:
        """{(kind, policy name, rule index): the pairs that rule decided} in
        ``direction``, over the whole domain -- what K8sPairVerdicts.blame
        returns for all pairs; ``deny_only``: the Deny rules only."""
        out: Dict[tuple, int] = {}
        for r in self._direction(direction):
            if r.decided and (r.action == "Deny" or not deny_only):
                key = (r.kind, r.policy, r.rule)
                out[key] = out.get(key, 0) + r.decided
        return out

    def dead_rules(self) -> List[tuple]:
        """The rules that count on the port and decide and pass nothing:
        (direction, kind, policy name, rule index)."""
        return [(d, r.kind, r.policy, r.rule) for d in ("egress", "ingress")
                for r in self._records[d] if r.on_port and not r.decided and not r.passed]

    def redundant_rules(self) -> List[tuple]:
        """The NetworkPolicy rules with sole == 0, dead ones and the rules the
        port drops included: removing one of them alone changes no verdict on
        this port.  (direction, kind, policy name, rule index)."""
        return [(d, r.kind, r.policy, r.rule) for d in ("egress", "ingress")
                for r in self._records[d] if r.kind == "network" and r.sole == 0]


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


def _connect_tiers(egress, ingress, compiled, policies, port, allow_self, device, rows,
                   form="auto"):
    """_connect with AdminNetworkPolicy tiers: the port's codes over the two
    resident builds and one kano_k8s_conn_tiers, which also answers the
    isolation flags."""
    from ._engine import DeviceBuild
    n = len(compiled.containers)
    port = _port_query(port)
    code_e, code_i = compiled.codes(port)
    out = DeviceBuild.empty(n, device=device, rows=rows)
    iso_e, iso_i, counts = out.k8s_conn_tiers_from(
        egress.engine, ingress.engine, allow_self, code_e, compiled.np_level[0], code_i,
        compiled.np_level[1], form)
    kinds = [t[0] for t in compiled.tiers_egress + compiled.tiers_ingress]
    info = {"egress_entries": len(compiled.egress), "ingress_entries": len(compiled.ingress),
            "kept_egress_entries": counts["egress_entries"],
            "kept_ingress_entries": counts["ingress_entries"],
            "egress_isolated": counts["egress_isolated"],
            "ingress_isolated": counts["ingress_isolated"],
            "port": port, "allow_self": bool(allow_self), "rows": rows,
            "admin_entries": kinds.count("admin"), "baseline_entries": kinds.count("baseline"),
            "admin_levels": sum(compiled.np_level),
            "admin_priority_ties": compiled.admin_priority_ties}
    return K8sConnectivity(_wrap(out, n), egress, ingress, compiled, policies, port,
                           bool(allow_self), info, (iso_e, iso_i), device, rows, form)


def connectivity(pods: List[Pod], policies: List[NetworkPolicy], namespaces: List[Namespace],
                 port=None, allow_self: bool = True, device: int = 0, path: str = "auto",
                 rows: Optional[tuple] = None, form: str = "auto", admin=None,
                 baseline=None) -> K8sConnectivity:
    """The connectivity a cluster enforces (networking.k8s.io/v1) as an n x n
    matrix on the device (rows src, columns dst).  ``port``: None -- every
    rule counts whatever its ports, an upper bound over ports -- or
    (protocol, number).  ``admin`` / ``baseline``: the cluster's
    AdminNetworkPolicies and its BaselineAdminNetworkPolicy (see the section's
    comment), resolved per tier on the device; with Deny or Pass rules that
    carry ``ports``, ``port=None`` still counts every rule and is then no
    longer an upper bound over ports.  ``info`` gains ``admin_entries``,
    ``baseline_entries``, ``admin_levels`` (rules, both directions) and
    ``admin_priority_ties`` (ANPs sharing their priority with an earlier one:
    the position in ``admin`` breaks the tie).  ``allow_self``: a pod always reaches itself.
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
    compiled = compile_conformant(pods, policies, namespaces, admin, baseline)

    def operand(pols):
        b = DeviceBuild(intern(compiled.containers, pols), device=device, path=path, build=False)
        b.build_classes(path)          # the class tables only: M is never written
        return b

    eg, ing = operand(compiled.egress), operand(compiled.ingress)
    n = len(pods)
    if compiled.tiered:
        if isinstance(baseline, (list, tuple)):
            baseline = baseline[0] if baseline else None
        by_kind = {"admin": list(admin or []), "network": policies, "baseline": [baseline]}
        return _connect_tiers(_wrap(eg, n), _wrap(ing, n), compiled, by_kind, port, allow_self,
                              device, rows, form)
    isolated = (eg.k8s_isolated(), ing.k8s_isolated())
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
    return _load(paths)[:3]


Cluster = collections.namedtuple("Cluster", "pods policies namespaces admin baseline")


def load_cluster(paths) -> Cluster:
    """load_manifests plus the kinds AdminNetworkPolicy (``admin``, in file
    order) and BaselineAdminNetworkPolicy (``baseline``: the one object, or
    None; a second one is a ValueError): a named tuple (pods, policies,
    namespaces, admin, baseline), ready for ``connectivity(*c[:3],
    admin=c.admin, baseline=c.baseline)``."""
    pods, pols, nss, admin, base = _load(paths)
    if len(base) > 1:
        raise ValueError(f"{len(base)} BaselineAdminNetworkPolicies: a cluster has one")
    return Cluster(pods, pols, nss, admin, base[0] if base else None)


def _load(paths):
    """(pods, policies, namespaces, AdminNetworkPolicies,
    BaselineAdminNetworkPolicies) of the manifests."""
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
    pods, pols, nss, admin, base = [], [], {}, [], []

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
        elif kind == "AdminNetworkPolicy":
            admin.append(from_dict(kind, obj))
        elif kind == "BaselineAdminNetworkPolicy":
            base.append(from_dict(kind, obj))

    for f in files:
        with open(f) as fh:
            for doc in yaml.safe_load_all(fh):
                take(doc)
    for o in pods + pols:
        if o.namespace not in nss:
            nss[o.namespace] = Namespace(o.namespace)
    for ns in nss.values():
        ns.labels.setdefault(_NS_NAME_LABEL, ns.name)
    return pods, pols, list(nss.values()), admin, base
