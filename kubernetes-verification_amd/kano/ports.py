"""The ports of a policy list: keys, slots and per-policy bit masks.

Not part of kano_py, whose maths ignore ``Policy.protocol``.  ``ConfigParser``
and ``kano.bulk`` turn a NetworkPolicy rule's ``ports`` into
``policy.protocol = [protocol, port]``; the paper's example and ``kano.synth``
write ``PolicyProtocol([protocol, port])``.  This module reads either form:

* ``port_key(policy)``: ``None`` for a policy open on **any port** (protocol
  ``None``, ``[]``, ``PolicyProtocol([])`` or ``PolicyProtocol(None)``: the
  Kubernetes reading of a rule without ``ports``), else the tuple of its keys
  ``(str(protocol).upper(), str(port))`` -- one for the two-element forms,
  several for a ``PortSet``.
* ``port_table(policies)``: the distinct keys in first-appearance order and a
  bit mask per policy over the slots ``0 .. K-1`` (the named keys) and slot
  ``K`` = ``ANY_OTHER``: every port no policy names.

Keys are opaque: a port is equal to another or not.  There are no ranges
(``endPort``) and no named-port resolution -- a named port is its name.  The
queries over the table are kano.algorithm's port_matrix, pair_ports,
reachable_on and port_exposure.
"""
from __future__ import annotations

from typing import Iterable, List, NamedTuple, Optional, Tuple

import numpy as np

from .model import PolicyProtocol

PortKey = Tuple[str, str]


class _AnyOther:
    """The slot behind the named ones: every port no policy names."""
    __slots__ = ()

    def __repr__(self):
        return "ANY_OTHER"

    def __reduce__(self):
        return "ANY_OTHER"


ANY_OTHER = _AnyOther()


def _key(protocol, port) -> PortKey:
    return (str(protocol).upper(), str(port))


class PortSet:
    """Several (protocol, port) keys on one policy, as a Kubernetes rule's
    ``ports`` list: ``Policy(..., protocol=PortSet([("TCP", 80), ("TCP", 443)]))``.
    Each key is normalised like the two-element forms; an empty PortSet names
    no port and opens none."""

    __slots__ = ("keys",)

    def __init__(self, keys: Iterable):
        out: List[PortKey] = []
        for k in keys:
            if isinstance(k, (str, bytes)) or len(k) != 2:
                raise TypeError(f"PortSet wants (protocol, port) pairs, not {k!r}")
            key = _key(*k)
            if key not in out:
                out.append(key)
        self.keys = tuple(out)

    def __eq__(self, other):
        return isinstance(other, PortSet) and self.keys == other.keys

    def __hash__(self):
        return hash(self.keys)

    def __repr__(self):
        return f"PortSet({list(self.keys)!r})"


def port_key(policy) -> Optional[Tuple[PortKey, ...]]:
    """``None`` when the policy is open on any port, else the tuple of its
    normalised keys (see the module docstring).  Anything else raises
    TypeError naming the policy."""
    proto = policy.protocol
    if isinstance(proto, PortSet):
        return proto.keys
    if isinstance(proto, PolicyProtocol):
        proto = proto.protocols
    if proto is None:
        return None
    if isinstance(proto, (list, tuple)):
        if len(proto) == 0:
            return None
        if len(proto) == 2 and not any(isinstance(v, (list, tuple, dict, set)) or v is None
                                       for v in proto):
            return (_key(*proto),)
    raise TypeError(f"policy {getattr(policy, 'name', policy)!r}: protocol "
                    f"{policy.protocol!r} is neither None, [], [protocol, port], a "
                    "PolicyProtocol of those nor a PortSet")


def key_slot(keys: List[PortKey], port) -> int:
    """The slot of a (protocol, port) key or ANY_OTHER in a table's key list;
    a key the list does not hold maps to slot K = len(keys)."""
    if port is ANY_OTHER:
        return len(keys)
    if isinstance(port, (str, bytes)) or not hasattr(port, "__len__") or len(port) != 2:
        raise TypeError(f"a port is a (protocol, port) pair or ANY_OTHER, not {port!r}")
    key = _key(*port)
    return keys.index(key) if key in keys else len(keys)


def key_slots(keys: List[PortKey], port) -> List[int]:
    """The ascending distinct slots of one port or of a list of ports."""
    one = port is ANY_OTHER or (isinstance(port, (tuple, list)) and len(port) == 2 and
                                isinstance(port[0], (str, bytes)))
    return sorted({key_slot(keys, p) for p in ([port] if one else list(port))})


class PortTable(NamedTuple):
    keys: List[PortKey]        # the K distinct keys, first-appearance order
    masks: np.ndarray          # uint64 (P, KW), LSB first: bit k = slot k, slot K = ANY_OTHER
    any_port: np.ndarray       # bool (P,): the policy names no port

    @property
    def K(self) -> int:
        return len(self.keys)

    @property
    def KS(self) -> int:
        return len(self.keys) + 1

    @property
    def KW(self) -> int:
        return (len(self.keys) + 64) // 64

    def slot(self, port) -> int:
        """The slot of a (protocol, port) key or ANY_OTHER; a key no policy
        names maps to slot K."""
        return key_slot(self.keys, port)

    def slots(self, port) -> List[int]:
        """The ascending distinct slots of one port or a list of ports."""
        return key_slots(self.keys, port)

    def slot_mask(self, slots: Iterable[int]) -> np.ndarray:
        """uint64 (KW,) with the given slots' bits set."""
        m = np.zeros(self.KW, dtype=np.uint64)
        for s in slots:
            m[s >> 6] |= np.uint64(1) << np.uint64(s & 63)
        return m

    def carries(self, slots: Iterable[int]) -> np.ndarray:
        """bool (P,): the policies whose mask holds one of the slots."""
        return (self.masks & self.slot_mask(slots)).any(axis=1)


def port_table(policies) -> PortTable:
    """The port table of a policy list (see the module docstring): a policy
    with keys has their bits set, an any-port policy all KS = K + 1 bits, and
    the bits at positions >= KS are zero."""
    per = [port_key(p) for p in policies]
    index = {}
    for ks in per:
        for k in ks or ():
            index.setdefault(k, len(index))
    K = len(index)
    KS, KW = K + 1, (K + 64) // 64
    bits = np.zeros((len(per), KW * 64), dtype=np.uint8)
    any_port = np.array([ks is None for ks in per], dtype=bool)
    bits[any_port, :KS] = 1
    for p, ks in enumerate(per):
        for k in ks or ():
            bits[p, index[k]] = 1
    masks = np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(len(per), KW)
    return PortTable(list(index), masks, any_port)
