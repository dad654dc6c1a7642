"""The tiers of a policy list: an action and a priority per policy.

Not part of kano_py, whose policies only allow.  AdminNetworkPolicy and
BaselineAdminNetworkPolicy carry ``Allow`` and ``Deny`` rules with an integer
``priority``; Calico and Cilium policies have deny rules and an order.  Over
the working sets of a matrix's current policies every policy ``p`` carries

* an action, ``ALLOW`` or ``DENY``, and
* an integer priority: a smaller number is evaluated first (as
  AdminNetworkPolicy does); any int32 value is valid.

``p`` matches the pair ``(i, j)`` iff ``i`` is in its select set and ``j`` in
its allow set (source -> destination, the direction swap already applied).
With ``t*`` the smallest priority over the matching policies the verdict is

* **none** when nothing matches (the pair is unreachable: kano's reading),
* **deny** when some deny policy of priority ``t*`` matches (within one
  priority deny wins),
* **allow** otherwise,

and the deciding policy is the smallest current index among the matching
policies of priority ``t*`` with the winning action.  All-allow with any
priorities is the built matrix; one priority for all is
``subset(allows) & ~subset(denies)``.

The ``Policy`` dataclass keeps its fields: plain attributes set on instances
(``policy.action = "deny"; policy.priority = 10``) are the carrier, read by
``tiering(policies)``; a ``Tiering(actions, priorities)`` of explicit sequences
of the current policy list's length is accepted wherever tiers are.  ``Pass``,
the order of rules within a policy and YAML for AdminNetworkPolicy objects are
out of scope; ``kano.k8s`` and the parser stay as they are.  The queries over
the tiers are kano.algorithm's verdict_matrix, pair_verdicts, pair_verdict,
why_blocked and verdict_counts.
"""
from __future__ import annotations

import numbers
from typing import Optional

import numpy as np

ALLOW, DENY = 0, 1
NONE_VERDICT, ALLOW_VERDICT, DENY_VERDICT = 0, 1, 2
VERDICT_NAMES = ("none", "allow", "deny")

_I32 = np.iinfo(np.int32)


def _action(value, who="") -> int:
    if isinstance(value, str):
        low = value.lower()
        if low in ("allow", "deny"):
            return ALLOW if low == "allow" else DENY
    elif not isinstance(value, (bool, np.bool_)) and isinstance(value, (numbers.Integral,
                                                                       np.integer)):
        if int(value) in (ALLOW, DENY):
            return int(value)
    raise ValueError(f"{who}action {value!r} is neither 'allow' / 'deny' (any case) nor "
                     "ALLOW / DENY")


def _priority(value, who="") -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (numbers.Integral,
                                                                     np.integer)):
        raise ValueError(f"{who}priority {value!r} is not an int")
    if not _I32.min <= int(value) <= _I32.max:
        raise ValueError(f"{who}priority {value!r} is outside int32")
    return int(value)


class Tiering:
    """``actions`` ('allow' / 'deny' in any case, or ALLOW / DENY) and
    ``priorities`` (ints within int32; a bool or anything else raises
    ValueError), one of each per policy, kept as uint8 and int32 arrays."""

    __slots__ = ("actions", "priorities")

    def __init__(self, actions, priorities, names=None):
        actions, priorities = list(actions), list(priorities)
        if len(actions) != len(priorities):
            raise ValueError(f"{len(actions)} actions for {len(priorities)} priorities")
        who = ((lambda p: f"policy {names[p]!r}: ") if names is not None
               else (lambda p: f"entry {p}: "))
        self.actions = np.array([_action(a, who(p)) for p, a in enumerate(actions)],
                                dtype=np.uint8)
        self.priorities = np.array([_priority(v, who(p)) for p, v in enumerate(priorities)],
                                   dtype=np.int32)

    def __len__(self):
        return int(self.actions.shape[0])

    def __repr__(self):
        return f"Tiering({self.actions.tolist()!r}, {self.priorities.tolist()!r})"


def tiering(policies) -> Tiering:
    """The tiers the policies carry: ``getattr(p, "action", "allow")`` and
    ``getattr(p, "priority", 0)`` of each."""
    policies = list(policies)
    return Tiering([getattr(p, "action", "allow") for p in policies],
                   [getattr(p, "priority", 0) for p in policies],
                   [getattr(p, "name", p) for p in policies])


def resolve(policies, tiers: Optional[Tiering]) -> Tiering:
    """``tiers`` (a Tiering or an (actions, priorities) pair) checked against
    the current policy list, or the tiers the policies carry."""
    if tiers is None:
        return tiering(policies)
    if not isinstance(tiers, Tiering):
        try:
            actions, priorities = tiers
        except (TypeError, ValueError):
            raise ValueError("tiers is a Tiering or an (actions, priorities) pair") from None
        tiers = Tiering(actions, priorities)
    if len(tiers) != len(policies):
        raise ValueError(f"{len(tiers)} tiers for {len(policies)} current policies")
    return tiers
