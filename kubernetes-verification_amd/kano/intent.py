"""User-declared intents: what the cluster is supposed to do.

An ``Intent`` names who sends (``src``), who receives (``dst``) and what must
hold between them: "deny" -- no src pod may reach a dst pod -- or "allow" --
every src pod must reach every dst pod.  ``kano.algorithm.check_intents``
checks a list of them against a matrix on the device; this module is the host
side: selectors resolved to pod bit sets, and intents read from YAML.

A selector is one of
  * a dict of label terms, all of which must hold.  A plain value ``v`` under
    key ``k`` holds iff ``k in labels and labels[k] == v`` (Python ``==``, as
    the default matcher); a ``kano.model`` ``In / NotIn / Exists /
    DoesNotExist`` holds iff ``expr.matches(labels, k)``; ``{}`` matches every
    pod.  This is the Kubernetes reading: a key that no pod carries matches no
    pod (kano_py's build skips such a term, its quirk Q1 -- not here);
  * an iterable of pod indices (negative or >= n: IndexError);
  * a length-n numpy bool array or BitArray.
Not part of kano_py.
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, List, NamedTuple, Union

import numpy as np

from ._bits import BitArray, _nwords, _tail_mask, bool_to_words
from .model import DoesNotExist, Exists, In, LabelExpression, NotIn

Selector = Union[Dict[Any, Any], Iterable[int], np.ndarray, BitArray]
KINDS = ("deny", "allow")


class Intent(NamedTuple):
    src: Selector              # who sends
    dst: Selector              # who receives
    kind: str                  # "deny": no src pod may reach a dst pod
                               # "allow": every src pod must reach every dst pod
    name: str = ""


class _KeyIndex:
    """One key's values over the pods, from one pass over the containers:
    who carries the key, and the pods of every distinct value."""

    def __init__(self, containers, key):
        n = len(containers)
        self.n = n
        present = []
        self.by_str: Dict[str, List[int]] = {}      # type(value) is str: exact by dict lookup
        self.by_other: Dict[Any, List[int]] = {}    # other hashable values (1, 1.0 and True share one)
        self.odd: List[tuple] = []                  # (pod, unhashable value)
        for i, c in enumerate(containers):
            labels = c.labels
            if key not in labels:
                continue
            present.append(i)
            v = labels[key]
            if type(v) is str:
                self.by_str.setdefault(v, []).append(i)
                continue
            try:
                self.by_other.setdefault(v, []).append(i)
            except TypeError:
                self.odd.append((i, v))
        self.present = self._mask(present)

    def _mask(self, idx) -> np.ndarray:
        m = np.zeros(self.n, bool)
        if len(idx):
            m[np.asarray(idx, dtype=np.int64)] = True
        return m

    def equal_to(self, v) -> np.ndarray:
        """Pods whose value under the key == v."""
        idx: List[int] = []
        if type(v) is str:
            idx += self.by_str.get(v, [])
        else:       # (a non-str against str values: == decides, one test per distinct value)
            for g, pods in self.by_str.items():
                if g == v:
                    idx += pods
        for g, pods in self.by_other.items():
            if g == v:
                idx += pods
        idx += [i for i, g in self.odd if g == v]
        return self._mask(idx)

    def term(self, containers, key, t) -> np.ndarray:
        if not isinstance(t, LabelExpression):
            return self.equal_to(t)
        if type(t) is Exists:
            return self.present
        if type(t) is DoesNotExist:
            return ~self.present
        if type(t) in (In, NotIn):
            listed = np.zeros(self.n, bool)
            for v in t.values:
                listed |= self.equal_to(v)
            return listed if type(t) is In else ~listed
        # an expression of the caller's own: its matches() decides, pod by pod
        return np.fromiter((bool(t.matches(c.labels, key)) for c in containers), bool, self.n)


def _all_pods(n: int) -> np.ndarray:
    w = np.full(_nwords(n), ~np.uint64(0), dtype=np.uint64)
    m = _tail_mask(n)
    if m is not None and w.size:
        w[-1] &= m
    return w


def resolve_selectors(containers, selectors) -> np.ndarray:
    """The pod sets of ``selectors`` over ``containers``: (len(selectors), W)
    uint64, LSB-first words (the layout of ``_bits.bool_to_words``).  The
    containers are passed over once per distinct key the dict selectors use,
    never once per selector; a term that several selectors share is evaluated
    once."""
    selectors = list(selectors)
    n = len(containers)
    W = _nwords(n)
    out = np.zeros((len(selectors), W), dtype=np.uint64)
    keys: Dict[Any, _KeyIndex] = {}
    for s in selectors:
        if isinstance(s, dict):
            for k in s:
                if k not in keys:
                    keys[k] = None
    for k in keys:
        keys[k] = _KeyIndex(containers, k)
    terms: Dict[tuple, np.ndarray] = {}
    everyone = _all_pods(n)
    for q, s in enumerate(selectors):
        if isinstance(s, dict):
            words = everyone
            for k, t in s.items():
                tag = (k, "s", t) if type(t) is str else (k, "o", id(t))
                tw = terms.get(tag)
                if tw is None:
                    tw = terms[tag] = bool_to_words(keys[k].term(containers, k, t))
                words = words & tw
            out[q] = words
        elif isinstance(s, BitArray):
            if len(s) != n:
                raise ValueError("bitarrays of equal length expected for bitwise operation")
            out[q] = s.words()
        elif isinstance(s, np.ndarray) and s.dtype == bool:
            if s.shape != (n,):
                raise ValueError(f"a bool selector needs one entry per pod ({n}), not {s.shape}")
            out[q] = bool_to_words(s)
        else:
            idx = np.asarray(list(s), dtype=np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= n):
                raise IndexError("pod index out of range")
            bits = np.zeros(n, bool)
            bits[idx] = True
            out[q] = bool_to_words(bits)
    return out


# ---------------------------------------------------------------------------
# YAML: a list of {name, kind, from, to}, from / to in the Kubernetes
# LabelSelector shape (matchLabels and / or matchExpressions).
_OPERATORS = {"In": In, "NotIn": NotIn, "Exists": Exists, "DoesNotExist": DoesNotExist}


def _selector_from(sel, where: str) -> dict:
    if not isinstance(sel, dict) or set(sel) - {"matchLabels", "matchExpressions"}:
        raise ValueError(f"{where}: a selector holds matchLabels and / or matchExpressions only")
    out: dict = {}
    labels = sel.get("matchLabels") or {}
    if not isinstance(labels, dict):
        raise ValueError(f"{where}: matchLabels must be a mapping")
    out.update(labels)
    exprs = sel.get("matchExpressions") or []
    if not isinstance(exprs, list):
        raise ValueError(f"{where}: matchExpressions must be a list")
    for e in exprs:
        if not isinstance(e, dict) or "key" not in e or set(e) - {"key", "operator", "values"}:
            raise ValueError(f"{where}: an expression holds key, operator and values")
        op = e.get("operator")
        if op not in _OPERATORS:
            raise ValueError(f"{where}: unknown operator {op!r} "
                             f"(one of {', '.join(_OPERATORS)})")
        if e["key"] in out:
            raise ValueError(f"{where}: key {e['key']!r} used twice")
        values = e.get("values") or []
        if not isinstance(values, list):
            raise ValueError(f"{where}: values must be a list")
        if op in ("In", "NotIn"):
            out[e["key"]] = _OPERATORS[op](values)
        elif values:
            raise ValueError(f"{where}: {op} takes no values")
        else:
            out[e["key"]] = _OPERATORS[op]()
    return out


def intents_from(doc) -> List[Intent]:
    """``load_intents`` on an already parsed document."""
    if not isinstance(doc, list):
        raise ValueError("an intents file holds a list of {name, kind, from, to}")
    out = []
    for q, e in enumerate(doc):
        name = e.get("name", "") if isinstance(e, dict) else ""
        where = f"intent {q} ({name!r})"
        if not isinstance(e, dict) or set(e) - {"name", "kind", "from", "to"}:
            raise ValueError(f"{where}: an entry holds name, kind, from and to only")
        if e.get("kind") not in KINDS:
            raise ValueError(f"{where}: unknown kind {e.get('kind')!r} (deny or allow)")
        for side in ("from", "to"):
            if side not in e:
                raise ValueError(f"{where}: no {side!r} selector")
        out.append(Intent(_selector_from(e["from"], where + " from"),
                          _selector_from(e["to"], where + " to"), e["kind"], str(name)))
    return out


def load_intents(path) -> List[Intent]:
    """The intents of a YAML file: a list of ``{name, kind, from, to}`` with
    ``kind`` deny or allow and ``from`` / ``to`` Kubernetes LabelSelectors
    (``matchLabels`` and / or ``matchExpressions`` with ``key / operator /
    values``).  An unknown kind or operator raises ValueError naming the
    entry."""
    import yaml
    with open(path) as f:
        return intents_from(yaml.safe_load(f))


__all__ = ["Intent", "Selector", "KINDS", "resolve_selectors", "load_intents", "intents_from"]
