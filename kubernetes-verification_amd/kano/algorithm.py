"""Kano verification queries, drop-in for ``kano.algorithm`` of kano_py.

Every query runs on the device-resident matrix (kano/_engine.py ->
libkano_hip.so) and returns the reference's Python types: ascending
``List[int]`` index lists and a ``List[Tuple[int, int]]`` for policy_shadow.
Reference: kano_py/kano/algorithm.py:4-100.
"""
from __future__ import annotations

from typing import DefaultDict, Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from .model import *  # noqa: F401,F403  (the reference does the same, algorithm.py:1)
from .model import BitArray, Container, Policy, ReachabilityMatrix
from ._bits import bool_to_words, set_bit_indices, words_to_bool
from ._intern import group_ids
try:
    from . import _kano_host   # csrc/kano_hostext.c (host-side loops, no GPU work)
except ImportError:            # (missing or built for another interpreter: the
    _kano_host = None          # Python loops below do the same work)


def _engine(matrix: ReachabilityMatrix, whole: bool = True):
    """The matrix's device context.  A context holding only a row shard
    (a multi-GPU rank's rows) cannot answer a whole-matrix query on its own:
    the column checks, getcol and policy_shadow need every row, so they raise
    instead of returning the shard's part (combine shards with
    kano.shard.ShardExchange)."""
    eng = getattr(matrix, "_engine", None)
    if eng is None:
        raise TypeError("expected a kano ReachabilityMatrix built by this package")
    if whole and getattr(eng, "is_shard", False):
        r0, r1 = eng.row_span
        raise ValueError(f"matrix holds only rows [{r0}, {r1}) of {matrix.container_size}: "
                         "whole-matrix checks need every row (combine the row shards "
                         "with kano.shard.ShardExchange)")
    return eng


def all_reachable(matrix: ReachabilityMatrix) -> List[int]:
    """Columns j with M[i, j] = 1 for every row i (algorithm.py:4-9)."""
    eng = _engine(matrix)
    n = matrix.container_size
    if n == 0:
        return []
    col_and, _ = eng.col_checks()
    return set_bit_indices(col_and, n).tolist()


def all_isolated(matrix: ReachabilityMatrix) -> List[int]:
    """Columns j with M[i, j] = 0 for every row i (algorithm.py:12-17)."""
    eng = _engine(matrix)
    n = matrix.container_size
    if n == 0:
        return []
    _, col_or = eng.col_checks()
    return np.flatnonzero(~words_to_bool(col_or, n)).tolist()


def user_hashmap(containers: List[Container], label: str) -> Dict[str, BitArray]:
    """Group bitsets keyed by container.getValueOrDefault(label, "")
    (algorithm.py:20-24)."""
    n = len(containers)
    gid = group_ids(containers, label)
    keys: Dict = {}
    for c in containers:
        keys.setdefault(c.getValueOrDefault(label, ""), None)
    out: Dict = DefaultDict(lambda: BitArray(n))
    for g, key in enumerate(keys):
        out[key] = BitArray.from_words(bool_to_words(gid == g), n)
    return out


def group_keys(containers: List[Container], label: str) -> Tuple[list, np.ndarray]:
    """user_hashmap's keys in its (first-appearance) order, a missing label
    as "", and group_ids' dense ids into them: (keys, int32 gid)."""
    keys: Dict = {}
    for c in containers:
        keys.setdefault(c.getValueOrDefault(label, ""), None)
    return list(keys), group_ids(containers, label)


def user_crosscheck(matrix: ReachabilityMatrix, containers: List[Container],
                    label: str) -> List[int]:
    """Containers j reachable from a container of another user group
    (algorithm.py:27-42): j such that M[i, j] and g(i) != g(j) for some i."""
    eng = _engine(matrix)
    n = matrix.container_size
    if len(containers) != n:
        # the reference indexes user_map bitsets (len(containers) bits) with
        # columns of the matrix: mismatched sizes raise there as well
        raise ValueError("bitarrays of equal length expected for bitwise operation")
    if n == 0:
        return []
    gid = group_ids(containers, label)
    cross = eng.crosscheck(gid)
    return set_bit_indices(cross, n).tolist()


def system_isolation(matrix: ReachabilityMatrix, idx: int) -> List[int]:
    """Containers j not reachable from container idx (algorithm.py:45-55).
    On a row shard, idx must be one of the shard's rows."""
    eng = _engine(matrix, whole=False)
    n = matrix.container_size
    i = int(idx)
    if i < 0:
        i += n
    if not 0 <= i < n:
        raise IndexError("list index out of range")
    row = eng.rows(i, 1)[0]
    return np.flatnonzero(~words_to_bool(row, n)).tolist()


def _pairs_to_list(pairs: np.ndarray, P: int = 0) -> List[Tuple[int, int]]:
    if pairs.shape[0] == 0:
        return []
    # (csrc/kano_hostext.c: the tuples built natively, policy ints shared)
    if _kano_host is None:
        return [tuple(p) for p in pairs.tolist()]
    return _kano_host.pairs_list(np.ascontiguousarray(pairs, dtype=np.int32), int(P))


def _fast_path(matrix, policies, containers) -> bool:
    """True when (policies, containers) are exactly what this matrix's build
    saw and every container's select_policies is still that build's list."""
    if getattr(matrix, "_lists", None) is None:
        return False
    if matrix._policies is not policies and list(matrix._policies) != list(policies):
        return False
    if len(containers) != matrix._ncontainers:
        return False
    lists = matrix._lists
    order = lists._containers        # (the build's container order, snapshotted)
    if (_kano_host is not None and type(containers) is list and type(order) is list and
            _kano_host.pending_is(containers, Container, lists, order)):
        return True                  # (the loop below, natively, for exact Containers)
    if len(order) != len(containers):
        return False
    for c, o in zip(containers, order):
        if not isinstance(c, Container) or c is not o:
            return False
        if c._sel or len(c._pending) != 1 or c._pending[0] is not lists:
            return False
    return True


def policy_shadow_pairs(matrix: ReachabilityMatrix, policies: List[Policy],
                        containers: List[Container]) -> np.ndarray:
    """policy_shadow as an (T, 2) int32 array (compact form, same order)."""
    if _fast_path(matrix, policies, containers):
        return _engine(matrix).shadow()
    from ._engine import shadow_from_lists
    n_lists, nbits, soff, flat, aw = _explicit_lists(policies, containers)
    return shadow_from_lists(n_lists, nbits, soff, flat, aw, device=_engine(matrix).device)


def _explicit_lists(policies: List[Policy], containers: List[Container], dedup: bool = False):
    """The general form's inputs: explicit per-container lists (accumulated
    builds, edited lists) and each policy's current working_allow_set, as
    (n_lists, nbits, soff, flat int32, allow words).  ``dedup``: every list
    as its set of ids."""
    lists = [list(c.select_policies) for c in containers]
    if dedup:
        lists = [sorted(set(l)) for l in lists]
    soff = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(l) for l in lists], out=soff[1:])
    flat = np.fromiter((x for l in lists for x in l), dtype=np.int64, count=int(soff[-1]))
    P = len(policies)
    if flat.size and (flat.min() < 0 or flat.max() >= P):
        raise IndexError("list index out of range")
    needed = np.unique(flat) if flat.size else np.zeros(0, np.int64)
    nbits = None
    for p in needed.tolist():
        s = policies[p].working_allow_set
        if s is None:
            raise AttributeError("'NoneType' object has no attribute '__and__'")
        if nbits is None:
            nbits = len(s)
        elif len(s) != nbits:
            raise ValueError("bitarrays of equal length expected for bitwise operation")
    nbits = nbits or 0
    W = (nbits + 63) >> 6
    aw = np.zeros((P, W), dtype=np.uint64)
    for p in needed.tolist():
        s = policies[p].working_allow_set
        b = s if isinstance(s, BitArray) else BitArray(s)
        aw[p] = b.words()[:W]
    return len(lists), nbits, soff, flat.astype(np.int32), aw


def policy_shadow(matrix: ReachabilityMatrix, policies: List[Policy],
                  containers: List[Container]) -> List[Tuple[int, int]]:
    """Pairs (j, k) of policies selecting a common container with allow_k a
    subset of allow_j, one entry per container, in container order
    (algorithm.py:58-80; duplicates kept, quirk Q4)."""
    return _pairs_to_list(policy_shadow_pairs(matrix, policies, containers), len(policies))


def policy_conflict(matrix: ReachabilityMatrix, policies: List[Policy],
                    containers: List[Container]) -> List[Tuple[int, int]]:
    """Reproduces algorithm.py:83-100 as written: the loop binds ``pj`` to a
    policy *index*, so the first container with two selecting policies raises
    ``AttributeError`` (quirk Q3); otherwise the result is []."""
    if _fast_path(matrix, policies, containers):
        raises = _engine(matrix).conflict_raises()
    else:
        raises = any(len(c.select_policies) >= 2 for c in containers)
    if raises:
        raise AttributeError("'int' object has no attribute 'working_allow_set'")
    return []


# ---------------------------------------------------------------------------
# The working policy_conflict.  policy_conflict above reproduces the
# reference's AttributeError; these answer the question its loop was written
# for: which policies selecting the same container have
# allow sets with no container in common?  Same iteration as policy_shadow:
# containers ascending, j then k in select_policies order, j == k skipped by
# value, one entry per container (duplicates kept, quirk Q4).  The relation is
# symmetric, so (j, k) and (k, j) both appear; an empty allow set conflicts
# with every other policy.

def policy_conflict_pairs(matrix: ReachabilityMatrix, policies: List[Policy],
                          containers: List[Container]) -> np.ndarray:
    """The conflicting pairs as an (T, 2) int32 array."""
    if _fast_path(matrix, policies, containers):
        return _engine(matrix).conflict()
    from ._engine import conflict_from_lists
    n_lists, nbits, soff, flat, aw = _explicit_lists(policies, containers)
    return conflict_from_lists(n_lists, nbits, soff, flat, aw, device=_engine(matrix).device)


def policy_conflicts(matrix: ReachabilityMatrix, policies: List[Policy],
                     containers: List[Container]) -> List[Tuple[int, int]]:
    """Pairs (j, k) of policies selecting a common container whose allow sets
    are disjoint, one entry per container, in container order."""
    return _pairs_to_list(policy_conflict_pairs(matrix, policies, containers), len(policies))


def policy_conflict_count(matrix: ReachabilityMatrix, policies: List[Policy],
                          containers: List[Container]) -> int:
    """len(policy_conflicts(...)) without the pairs (sparse clusters make
    nearly every candidate pair a conflict)."""
    if _fast_path(matrix, policies, containers):
        return _engine(matrix).conflict_count()
    from ._engine import conflict_from_lists
    n_lists, nbits, soff, flat, aw = _explicit_lists(policies, containers)
    return conflict_from_lists(n_lists, nbits, soff, flat, aw, device=_engine(matrix).device,
                               count_only=True)


def policy_conflict_summary(matrix: ReachabilityMatrix, policies: List[Policy],
                            containers: List[Container]) -> List[Tuple[int, int, int]]:
    """The distinct conflicting pairs j < k, ascending, each with the number
    of containers that both policies select: [(j, k, containers), ...].
    Aggregated on the host from the class-level lists (the per-container pair
    list of a large sparse cluster runs to ~1e8 entries)."""
    P = len(policies)
    if _fast_path(matrix, policies, containers):
        eng = _engine(matrix)
        if hasattr(eng, "conflict_classes"):
            off, pairs, members = eng.conflict_classes()
            weight = np.repeat(members.astype(np.int64), np.diff(off))
        else:                    # (a row-sharded group: its members' pair lists)
            pairs = eng.conflict()
            weight = np.ones(pairs.shape[0], dtype=np.int64)
    else:
        # (every list as a set: a repeated id would count its container twice)
        from ._engine import conflict_from_lists
        n_lists, nbits, soff, flat, aw = _explicit_lists(policies, containers, dedup=True)
        pairs = conflict_from_lists(n_lists, nbits, soff, flat, aw,
                                    device=_engine(matrix).device)
        weight = np.ones(pairs.shape[0], dtype=np.int64)
    keep = pairs[:, 0] < pairs[:, 1]
    key = pairs[keep, 0].astype(np.int64) * max(P, 1) + pairs[keep, 1]
    uniq, inv = np.unique(key, return_inverse=True)
    tot = np.bincount(inv, weights=weight[keep], minlength=uniq.size).astype(np.int64)
    return [(int(k // max(P, 1)), int(k % max(P, 1)), int(t)) for k, t in zip(uniq, tot)]


# ---------------------------------------------------------------------------
# What removing a policy changes.  Not part of kano_py's algorithm.py.  With
# cover(i, j) = #{p : i in working_select_set_p, j in working_allow_set_p},
#   impact[p] = #{(i, j) : i in select_p, j in allow_p, cover(i, j) == 1}
# is the number of pod pairs that lose reachability when p alone is removed,
# and p is redundant when impact[p] == 0: an empty select or allow set, a
# policy covered by the union of others (policy_shadow sees only the cover by
# one other policy), each of two identical policies.  Defined over the sets,
# so accumulated or edited select_policies lists (quirk Q5) do not change it.

def _set_lists(policies: List[Policy], containers: List[Container]):
    """The general form's inputs from the policies' working sets: per
    container the ascending, distinct ids of the policies selecting it, and
    each policy's allow words, as (n_lists, nbits, soff, flat int32, words)."""
    P, n = len(policies), len(containers)
    pods, nbits = [], None
    for p, pol in enumerate(policies):
        sel, alw = pol.working_select_set, pol.working_allow_set
        if sel is None or alw is None:
            raise ValueError(f"policy {p} has no working sets (build a matrix with it first)")
        if len(sel) != n:
            raise ValueError(f"policy {p}: working_select_set has {len(sel)} bits for "
                             f"{n} containers")
        if nbits is None:
            nbits = len(alw)
        elif len(alw) != nbits:
            raise ValueError("bitarrays of equal length expected for bitwise operation")
        b = sel if isinstance(sel, BitArray) else BitArray(sel)
        pods.append(set_bit_indices(b.words(), n))
    nbits = nbits or 0
    W = (nbits + 63) >> 6
    aw = np.zeros((P, W), dtype=np.uint64)
    for p, pol in enumerate(policies):
        s = pol.working_allow_set
        b = s if isinstance(s, BitArray) else BitArray(s)
        aw[p] = b.words()[:W]
    if W and nbits & 63:
        aw[:, -1] &= np.uint64((1 << (nbits & 63)) - 1)
    # (policy-major entries, a stable counting sort by pod: every list ascending)
    key = np.concatenate(pods) if pods else np.zeros(0, np.int64)
    ids = np.repeat(np.arange(P, dtype=np.int32), [x.size for x in pods])
    soff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key, minlength=n), out=soff[1:])
    flat = ids[np.argsort(key, kind="stable")]
    return n, nbits, soff, flat, aw


def policy_impact(matrix: ReachabilityMatrix, policies: List[Policy],
                  containers: List[Container]) -> np.ndarray:
    """impact[p] for every policy: int64 array of length len(policies)."""
    if _fast_path(matrix, policies, containers):
        return _engine(matrix).policy_impact()
    from ._engine import impact_from_lists
    n_lists, nbits, soff, flat, aw = _set_lists(policies, containers)
    return impact_from_lists(n_lists, nbits, soff, flat, aw, device=_engine(matrix).device)


def policy_redundant(matrix: ReachabilityMatrix, policies: List[Policy],
                     containers: List[Container]) -> List[int]:
    """Ascending indices of the policies whose removal changes no pair (the
    flags alone: no sums on the device)."""
    if _fast_path(matrix, policies, containers):
        ess = _engine(matrix).policy_essential()
    else:
        from ._engine import impact_from_lists
        n_lists, nbits, soff, flat, aw = _set_lists(policies, containers)
        ess = impact_from_lists(n_lists, nbits, soff, flat, aw, device=_engine(matrix).device,
                                flags_only=True)
    return np.flatnonzero(~ess).tolist()


# ---------------------------------------------------------------------------
# Which policies make a pair reachable.  Not part of kano_py's algorithm.py.
# Over the working sets of the matrix's current policies (matrix._policies:
# after add_policies / remove_policies the updated list, current indices),
#   pols(i, j)  = ascending indices p with i in select_p and j in allow_p
#   cover(i, j) = len(pols(i, j))
# computed on the device from the resident tables (kano_pair_policies), for
# built and incrementally updated matrices alike.  Defined over the sets (a
# policy appears once per pair; accumulated select_policies lists, quirk Q5,
# do not change it).  The query speaks about the policies, not about bits
# edited by hand: on a matrix without set-item / put_rows edits cover(i, j) > 0
# iff M[i, j] = 1.  A matrix holding a row shard answers for the pairs whose i
# it holds; the other pairs get cover 0.

class PairPolicies(NamedTuple):
    cover: np.ndarray          # int32, one per queried pair
    offsets: np.ndarray        # int64 (Q + 1)
    policies: np.ndarray       # int32: pair q's indices are policies[offsets[q]:offsets[q + 1]]

    def of(self, q: int) -> List[int]:
        """The ascending policy indices allowing queried pair q."""
        q = int(q)
        if not -len(self.cover) <= q < len(self.cover):
            raise IndexError("pair index out of range")
        q %= len(self.cover)
        return self.policies[self.offsets[q]:self.offsets[q + 1]].tolist()


def _pair_engine(matrix: ReachabilityMatrix, pairs):
    """The engine, the checked (Q, 2) int32 pairs and the map from engine ids
    to the indices of matrix._policies (None: they are equal)."""
    from ._engine import _as_pairs
    eng = _engine(matrix, whole=False)
    ps = getattr(matrix, "_policies", None)
    if ps is None:
        raise ValueError("the matrix has no policies (a wrapped, copied, loaded, path or edge "
                         "matrix holds rows only): pair_policies needs one from build_matrix")
    pr, _ = _as_pairs(pairs)
    n = matrix.container_size
    if pr.size and (pr.min() < 0 or pr.max() >= n):
        raise IndexError("bitarray index out of range")
    eids = getattr(matrix, "_eids", None)
    if eids is None or eids == list(range(len(ps))):
        return eng, pr, None, len(ps)
    back = np.full(max(eids) + 1 if eids else 0, -1, dtype=np.int32)
    back[np.asarray(eids, dtype=np.int64)] = np.arange(len(eids), dtype=np.int32)
    return eng, pr, (np.asarray(eids, dtype=np.int64), back), len(ps)


def pair_policies(matrix: ReachabilityMatrix, pairs) -> PairPolicies:
    """For every (i, j) of ``pairs`` (an (T, 2) int array as matrix_diff_pairs
    returns it, or a list of tuples; any order, duplicates allowed) the
    policies that select i and allow j (see PairPolicies)."""
    eng, pr, ids, P = _pair_engine(matrix, pairs)
    if P == 0:
        z = np.zeros(pr.shape[0], np.int32)
        return PairPolicies(z, np.zeros(pr.shape[0] + 1, np.int64), np.zeros(0, np.int32))
    r = eng.pair_policies(pr, lists=True)
    pol = r["policies"] if ids is None else ids[1][r["policies"]]
    return PairPolicies(r["cover"], r["offsets"], pol)


def pair_cover(matrix: ReachabilityMatrix, pairs) -> np.ndarray:
    """cover(i, j) for every queried pair, int32 (the counts alone: no lists
    on the device)."""
    eng, pr, _, P = _pair_engine(matrix, pairs)
    if P == 0:
        return np.zeros(pr.shape[0], np.int32)
    return eng.pair_policies(pr, lists=False)["cover"]


def why_reachable(matrix: ReachabilityMatrix, i: int, j: int) -> List[int]:
    """The ascending indices of the policies that select i and allow j."""
    return pair_policies(matrix, [(int(i), int(j))]).of(0)


def policy_blame(matrix: ReachabilityMatrix, pairs) -> np.ndarray:
    """blame[p] = the number of queried pairs policy p allows (a pair repeated
    in ``pairs`` counts each time): int64, one entry per current policy --
    a set of violating pairs ranked by the policies behind them."""
    eng, pr, ids, P = _pair_engine(matrix, pairs)
    if P == 0:
        return np.zeros(0, np.int64)
    hist = eng.pair_policies(pr, lists=False, hist=True)["hist"]
    return hist[:P].copy() if ids is None else hist[ids[0]]


# ---------------------------------------------------------------------------
# What a change adds and removes.  Not part of kano_py's algorithm.py.  For
# two matrices over the same pods (and, for row shards, the same rows),
#   added(i, j) = after[i, j] and not before[i, j]
#   removed(i, j) = before[i, j] and not after[i, j]
# computed on the device in one pass over both (kano_diff): before and after
# an incremental update (ReachabilityMatrix.snapshot), a matrix against its
# two_hop / closure, kano's reading against kubesv's, a loaded file against
# today's build.

class MatrixDiff(NamedTuple):
    added: int                 # pairs reachable in `after` only
    removed: int               # pairs reachable in `before` only
    row_added: np.ndarray      # int64, one per held row: the source's gained pairs
    row_removed: np.ndarray
    col_added: List[int]       # ascending destinations that gained at least one source
    col_removed: List[int]

    @property
    def equal(self) -> bool:
        return self.added == 0 and self.removed == 0


def _diff_engines(before: ReachabilityMatrix, after: ReachabilityMatrix):
    a, b = _engine(before, whole=False), _engine(after, whole=False)
    if before.container_size != after.container_size:
        raise ValueError(f"matrices of {before.container_size} and {after.container_size} "
                         "containers cannot be compared")
    if type(a) is not type(b) or getattr(a, "device", 0) != getattr(b, "device", 0):
        raise ValueError("matrix_diff needs both matrices on the same device(s)")
    if getattr(a, "row_span", None) != getattr(b, "row_span", None):
        raise ValueError(f"the matrices hold different rows: {a.row_span} and {b.row_span}")
    return a, b


def matrix_diff(before: ReachabilityMatrix, after: ReachabilityMatrix) -> MatrixDiff:
    """The pairs `after` holds and `before` does not, and the reverse: totals,
    per-row counts and the columns touched (see MatrixDiff)."""
    a, b = _diff_engines(before, after)
    n = before.container_size
    d = a.diff(b)
    return MatrixDiff(d["added"], d["removed"], d["row_added"].astype(np.int64),
                      d["row_removed"].astype(np.int64),
                      set_bit_indices(d["col_added"], n).tolist(),
                      set_bit_indices(d["col_removed"], n).tolist())


def matrix_diff_pairs(before: ReachabilityMatrix, after: ReachabilityMatrix,
                      kind: str = "added", limit: int = 1_000_000,
                      rows: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """The (i, j) pairs of one kind ("added" or "removed") as an int32 (T, 2)
    array, ascending by i then j; ``rows`` = (r0, r1) restricts the sources
    (default: every held row).  More than ``limit`` pairs raise OverflowError
    naming their number: narrow ``rows`` or raise the limit."""
    if kind not in ("added", "removed"):
        raise ValueError(f"kind must be 'added' or 'removed', not {kind!r}")
    a, b = _diff_engines(before, after)
    span = getattr(a, "row_span", None) or (0, before.container_size)
    r0, r1 = span if rows is None else (int(rows[0]), int(rows[1]))
    if not span[0] <= r0 <= r1 <= span[1]:
        raise ValueError(f"rows [{r0}, {r1}) outside the held rows [{span[0]}, {span[1]})")
    return a.diff_pairs(b, kind, r0, r1 - r0, limit=limit)


# ---------------------------------------------------------------------------
# Who reaches whom, by group.  Not part of kano_py's algorithm.py.
# user_crosscheck says which pods are reached from another group; these say
# which group reaches which, through how many pod pairs and from which pods:
#   counts[g][h] = #{(i, j) : M[i, j], group(i) = g, group(j) = h}
# computed on the device from the matrix itself (kano_group_counts), so it
# holds for built, updated, loaded, path and edge matrices alike.  A matrix
# holding a row shard answers for its rows: the counts of the shards add up.

class GroupReachability(NamedTuple):
    src_keys: list             # label values in first-appearance order (user_hashmap's; missing: "")
    dst_keys: list
    counts: np.ndarray         # int64 (len(src_keys), len(dst_keys)): pod pairs g -> h
    src_sizes: np.ndarray      # pods per source group among the held rows
    dst_sizes: np.ndarray      # pods per destination group

    def pairs(self, cross_only: bool = True) -> List[Tuple]:
        """[(src_key, dst_key, count)] for every count > 0, in row-major
        order; ``cross_only`` drops the entries with src_key == dst_key."""
        out = []
        for g, h in np.argwhere(np.asarray(self.counts) > 0).tolist():
            s, d = self.src_keys[g], self.dst_keys[h]
            if cross_only and s == d:
                continue
            out.append((s, d, int(self.counts[g][h])))
        return out


def _group_engine(matrix: ReachabilityMatrix, containers: List[Container]):
    eng = _engine(matrix, whole=False)
    n = matrix.container_size
    if len(containers) != n:
        raise ValueError("bitarrays of equal length expected for bitwise operation")
    return eng, n, (getattr(eng, "row_span", None) or (0, n))


def group_reachability(matrix: ReachabilityMatrix, containers: List[Container], label: str,
                       dst_label: Optional[str] = None) -> GroupReachability:
    """The pod pairs (i, j) with M[i, j] = 1 counted by the group of i under
    ``label`` and the group of j under ``dst_label`` (default: ``label``).
    A matrix holding a row shard counts its own rows' pairs."""
    eng, n, (r0, r1) = _group_engine(matrix, containers)
    skeys, gs = group_keys(containers, label)
    dkeys, gd = (skeys, gs) if dst_label is None else group_keys(containers, dst_label)
    Gs, Gd = len(skeys), len(dkeys)
    if n == 0:
        return GroupReachability([], [], np.zeros((0, 0), np.int64), np.zeros(0, np.int64),
                                 np.zeros(0, np.int64))
    counts = eng.group_counts(gs, gd, Gs, Gd)["counts"]
    return GroupReachability(skeys, dkeys, counts,
                             np.bincount(gs[r0:r1], minlength=Gs).astype(np.int64),
                             np.bincount(gd, minlength=Gd).astype(np.int64))


def group_fanout(matrix: ReachabilityMatrix, containers: List[Container], label: str,
                 rows: Optional[Tuple[int, int]] = None) -> Tuple[list, np.ndarray]:
    """Per held source pod, the number of pods it reaches in every group of
    ``label``: (dst_keys, int32 array (rows, G)), one row per held row in row
    order (a row shard: its rows); ``rows`` = (r0, r1) keeps those sources."""
    eng, n, span = _group_engine(matrix, containers)
    keys, gd = group_keys(containers, label)
    r0, r1 = span if rows is None else (int(rows[0]), int(rows[1]))
    if not span[0] <= r0 <= r1 <= span[1]:
        raise ValueError(f"rows [{r0}, {r1}) outside the held rows [{span[0]}, {span[1]})")
    if n == 0:
        return [], np.zeros((0, 0), np.int32)
    out = eng.group_counts(np.full(n, -1, np.int32), gd, 1, len(keys), rows=True)["row_counts"]
    return keys, out[r0 - span[0]:r1 - span[0]]


def reach_count(matrix: ReachabilityMatrix, sources, dests) -> int:
    """The pairs (i, j) with M[i, j] = 1, i in the index set ``sources`` and
    j in the index set ``dests``.  A matrix holding a row shard counts the
    sources among its rows."""
    eng = _engine(matrix, whole=False)
    n = matrix.container_size
    if n == 0:
        return 0
    gs, gd = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    gs[np.asarray(list(sources), dtype=np.int64)] = 0
    gd[np.asarray(list(dests), dtype=np.int64)] = 0
    return int(eng.group_counts(gs, gd, 1, 1)["counts"][0, 0])


# ---------------------------------------------------------------------------
# Multi-hop reachability.  Not part of kano_py's
# algorithm.py: kubesv's `path` relation (kubesv/kubesv/constraint.py:233-237,
# path(src, dst) :- edge(src, dst); path(src, dst) :- edge(src, sel),
# edge(sel, dst)) with kano's matrix as `edge`.  The result is a
# ReachabilityMatrix on the device, so every query above runs on it.

def _path_matrix(matrix: ReachabilityMatrix, hops: int, mode: str) -> ReachabilityMatrix:
    from ._engine import DeviceBuild
    from .multi import MultiBuild
    src = _engine(matrix)
    n = matrix.container_size
    out = ReachabilityMatrix.__new__(ReachabilityMatrix)
    out.container_size = n
    # a row-sharded group's path matrix is sharded the same way
    out._engine = (MultiBuild.empty(n, src.G, devices=src.devices)
                   if isinstance(src, MultiBuild) else DeviceBuild.empty(n, device=src.device))
    out._containers = None
    out._policies = None
    out._ncontainers = n
    out._lists = None
    out.path_info = out._engine.path_from(src, hops=hops, mode=mode)
    return out


def two_hop(matrix: ReachabilityMatrix, mode: str = "auto") -> ReachabilityMatrix:
    """kubesv's path relation: P = M | M.M (pairs joined by one or two
    edges)."""
    return _path_matrix(matrix, 2, mode)


def k_hop(matrix: ReachabilityMatrix, hops: int, mode: str = "auto") -> ReachabilityMatrix:
    """Pairs joined by a path of at most `hops` (>= 1) edges."""
    if int(hops) < 1:
        raise ValueError("hops must be >= 1")
    return _path_matrix(matrix, int(hops), mode)


def transitive_closure(matrix: ReachabilityMatrix, mode: str = "auto") -> ReachabilityMatrix:
    """M+: pairs joined by a path of any length >= 1 (the fixpoint of the
    path rule applied to itself)."""
    return _path_matrix(matrix, 0, mode)


# ---------------------------------------------------------------------------
# Through which pods, and in how many hops.  Not part of kano_py's
# algorithm.py.  two_hop / k_hop / transitive_closure answer with a matrix of
# bits; these answer with the distance and the route.  With an edge i -> j iff
# M[i, j] = 1,
#   dist(s, t) = the least k >= 1 such that a walk of k edges leads from s to
#                t, -1 if there is none (or none within max_hops; 0 = no bound)
# (k starts at 1 as the closure's paths do: dist(s, s) is 1 with a self-loop,
# else the shortest cycle through s, else -1), so
#   k_hop(M, k)[s, t] = 1  iff  1 <= dist(s, t) <= k,
#   transitive_closure(M)[s, t] = 1  iff  dist(s, t) >= 1.
# The canonical shortest path of a pair with d = dist(s, t) >= 1 is
# [s, t_1, .., t_{d-1}, t], built backwards from t_d = t with t_{k-1} = the
# smallest pod at distance k - 1 from s that has an edge to t_k.  Computed on
# the device by a breadth-first search over the matrix itself (kano_hops /
# kano_hop_pairs), so it holds for built, updated, edited, loaded, path and
# edge matrices alike.  The search reads every row: a matrix holding a row
# shard raises.  One host round trip per level: a chain of depth d costs d.

class HopPaths(NamedTuple):
    dist: np.ndarray           # int32, one per queried pair (-1: unreachable)
    offsets: np.ndarray        # int64 (Q + 1)
    nodes: np.ndarray          # int32: pair q's path is nodes[offsets[q]:offsets[q + 1]]

    def of(self, q: int) -> List[int]:
        """The canonical shortest path of queried pair q ([] when unreachable)."""
        q = int(q)
        if not -len(self.dist) <= q < len(self.dist):
            raise IndexError("pair index out of range")
        q %= len(self.dist)
        return self.nodes[self.offsets[q]:self.offsets[q + 1]].tolist()


def _hop_bound(max_hops) -> int:
    if int(max_hops) < 0:
        raise ValueError("max_hops must be >= 0 (0: no bound)")
    return int(max_hops)


def _hop_pairs(matrix: ReachabilityMatrix, pairs, max_hops, paths: bool) -> dict:
    from ._engine import _as_pairs
    eng = _engine(matrix, whole=True)
    pr, _ = _as_pairs(pairs)
    if pr.size and (pr.min() < 0 or pr.max() >= matrix.container_size):
        raise IndexError("bitarray index out of range")
    return eng.hop_pairs(pr, _hop_bound(max_hops), paths=paths)


def hop_levels(matrix: ReachabilityMatrix, sources, max_hops: int = 0) -> np.ndarray:
    """dist(s, v) for every source s of ``sources`` and every pod v: int32
    (len(sources), n); an ``int`` source gives (n,)."""
    eng = _engine(matrix, whole=True)
    one = isinstance(sources, (int, np.integer))
    src = np.asarray([sources] if one else list(sources), dtype=np.int64).reshape(-1)
    if src.size and (src.min() < 0 or src.max() >= matrix.container_size):
        raise IndexError("bitarray index out of range")
    dist = eng.hops(src.astype(np.int32), _hop_bound(max_hops))["dist"]
    return dist[0] if one else dist


def hop_distance(matrix: ReachabilityMatrix, pairs, max_hops: int = 0) -> np.ndarray:
    """dist(i, j) for every (i, j) of ``pairs`` (a (Q, 2) int array or a list
    of tuples; any order, duplicates allowed): int32 (Q,)."""
    return _hop_pairs(matrix, pairs, max_hops, False)["dist"]


def path_witnesses(matrix: ReachabilityMatrix, pairs, max_hops: int = 0) -> HopPaths:
    """The distance and the canonical shortest path of every queried pair
    (see HopPaths)."""
    r = _hop_pairs(matrix, pairs, max_hops, True)
    return HopPaths(r["dist"], r["offsets"], r["nodes"])


def path_witness(matrix: ReachabilityMatrix, i: int, j: int, max_hops: int = 0) -> List[int]:
    """The canonical shortest path from i to j as a list of pod indices
    ([] when j is unreachable from i, or not within max_hops)."""
    return path_witnesses(matrix, [(int(i), int(j))], max_hops).of(0)


# ---------------------------------------------------------------------------
# Who reaches a pod, and which pods can all reach each other.  Not part of
# kano_py's algorithm.py.  Every query above starts at a source row;
# reverse_matrix gives the matrix read by columns as a matrix of its own
# (R[t, s] = M[s, t], the bit transpose on the device: kano_reverse), so the
# same queries answer from the destination's side.  reach_zones turns the
# closure's bits into lateral-movement zones: with C = transitive_closure(M),
# "j = i, or C[i, j] and C[j, i]" is an equivalence relation whose classes are
# the strongly connected components of the reachability graph, and
#   label[i]   = the smallest pod of i's zone,
#   fan_out[i] = popcount(C[i]): the pods i eventually reaches,
#   fan_in[i]  = popcount(C[:, i]): the pods that eventually reach i,
#   cyclic[i]  = C[i, i]: i lies on a cycle
# from one pass over C and its reverse (kano_zones).  zone_graph counts M's
# own edges between the zones; between different zones it is acyclic.  Whole
# matrices on one device only: a row shard raises.  reach_zones holds M, C and
# the reverse of C at once (three n x n bit matrices); the closure of an
# edited matrix takes kano_path's pod-level form.  Not covered: row shards,
# groups of several members, a closure-free forward / backward search,
# incremental maintenance of the zones.

class Zones(NamedTuple):
    label: np.ndarray          # int32 (n): the smallest pod of the pod's zone
    fan_out: np.ndarray        # int32 (n): pods it eventually reaches
    fan_in: np.ndarray         # int32 (n): pods that eventually reach it
    cyclic: np.ndarray         # bool (n): it lies on a cycle

    def reps(self) -> np.ndarray:
        """The distinct labels, ascending: one representative per zone."""
        return np.unique(np.asarray(self.label, dtype=np.int32))

    def sizes(self) -> np.ndarray:
        """Pods per zone, aligned with ``reps()``."""
        return np.unique(np.asarray(self.label), return_counts=True)[1].astype(np.int64)

    def members(self, z: int) -> List[int]:
        """The pods of the zone whose representative is ``z``, ascending."""
        return np.flatnonzero(np.asarray(self.label) == int(z)).tolist()

    def nontrivial(self, min_size: int = 2) -> np.ndarray:
        """The representatives of the zones with at least ``min_size`` pods."""
        return self.reps()[self.sizes() >= int(min_size)]

    def index(self, min_size: int = 1) -> np.ndarray:
        """A dense zone id per pod (int32), in ``reps()`` order over the zones
        with at least ``min_size`` pods; -1 for the pods of smaller zones."""
        reps, inv, cnt = np.unique(np.asarray(self.label), return_inverse=True,
                                   return_counts=True)
        keep = cnt >= int(min_size)
        dense = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        return dense[inv.reshape(-1)]


class ZoneGraph(NamedTuple):
    reps: np.ndarray           # int32: the zones' representatives, ascending
    counts: np.ndarray         # int64 (Z, Z): M's edges from zone a into zone b


def reverse_matrix(matrix: ReachabilityMatrix) -> ReachabilityMatrix:
    """The matrix read by columns, as a new rows-only matrix on the device:
    row t of the result is the set of pods that reach t.  So
    ``hop_levels(reverse_matrix(m), t)`` is who reaches t and in how many
    hops, ``group_fanout`` on it is the per-pod fan-in by group, and
    ``check_intents`` on it reads the intents from the destination's side.
    Needs the whole matrix on one device (a row shard raises)."""
    from ._engine import DeviceBuild
    from .multi import MultiBuild
    src = _engine(matrix, whole=True)
    n = matrix.container_size
    if isinstance(src, MultiBuild):
        src._zones_member("reverse_matrix")
    out = ReachabilityMatrix.__new__(ReachabilityMatrix)
    out.container_size = n
    out._engine = (MultiBuild.empty(n, src.G, devices=src.devices)
                   if isinstance(src, MultiBuild) else DeviceBuild.empty(n, device=src.device))
    out._containers = None
    out._policies = None
    out._ncontainers = n
    out._lists = None
    try:
        out.reverse_info = src.reverse_into(out._engine)
    except BaseException:
        out._engine.close()
        raise
    return out


def reach_zones(matrix: ReachabilityMatrix,
                closure: Optional[ReachabilityMatrix] = None) -> Zones:
    """The lateral-movement zones of ``matrix`` (see Zones): the strongly
    connected components of its reachability graph with per-pod eventual
    fan-out and fan-in.  ``closure`` is ``transitive_closure(matrix)`` when
    the caller already holds it; else it is computed here.  Every temporary
    matrix the call creates is closed before it returns."""
    _engine(matrix, whole=True)
    n = matrix.container_size
    if closure is not None and closure.container_size != n:
        raise ValueError("the closure is of another size than the matrix")
    if n == 0:
        e = np.zeros(0, np.int32)
        return Zones(e, e.copy(), e.copy(), np.zeros(0, bool))
    made = []
    try:
        if closure is None:
            closure = transitive_closure(matrix)
            made.append(closure)
        rev = reverse_matrix(closure)
        made.append(rev)
        r = _engine(closure, whole=True).zones(rev._engine)
    finally:
        for m in made:
            m._engine.close()
    return Zones(r["label"], r["fan_out"], r["fan_in"], r["cyclic"])


def zone_graph(matrix: ReachabilityMatrix, zones: Zones, min_size: int = 1) -> ZoneGraph:
    """The graph between the zones of at least ``min_size`` pods on the
    matrix's own edges: ``counts[a, b]`` is the number of pairs (i, j) with
    M[i, j] = 1, i in zone ``reps[a]`` and j in zone ``reps[b]`` (the
    diagonal: the edges inside a zone).  Off the diagonal the graph is
    acyclic.  Counted on the device (kano_group_counts)."""
    eng = _engine(matrix, whole=True)
    n = matrix.container_size
    if len(zones.label) != n:
        raise ValueError("zones of another size than the matrix")
    reps = zones.nontrivial(min_size).astype(np.int32)
    Z = len(reps)
    if Z * Z > 1 << 27:
        raise ValueError(f"{Z} zones make {Z * Z} counts, beyond 2^27: raise min_size")
    if Z == 0:
        return ZoneGraph(reps, np.zeros((0, 0), np.int64))
    idx = zones.index(min_size)
    return ZoneGraph(reps, eng.group_counts(idx, idx, Z, Z)["counts"])


# ---------------------------------------------------------------------------
# What the cluster is supposed to do.  Not part of kano_py's algorithm.py.
# The checks above are fixed questions; an Intent (kano/intent.py) is the
# operator's own: "no src pod may reach a dst pod" (deny) or "every src pod
# must reach every dst pod" (allow), src and dst being selectors over the
# pods' labels, index sets or bit sets, free to overlap.  With S the src pods
# among the held rows, D the dst pods and the considered pairs
#   C = {(i, j) : i in S, j in D, and i != j unless self_pairs},
# a deny intent's violations are the pairs of C with M[i, j] = 1, an allow
# intent's those with M[i, j] = 0.  All intents of a call are checked in one
# pass on the device from the matrix itself (kano_intents), so it holds for
# built, updated, edited, loaded, snapshot, path and edge matrices alike.  A
# matrix holding a row shard answers for the sources among its rows.  A
# violating pair goes to why_reachable / path_witness, a violated intent's
# pairs (intent_violations) to policy_blame.

from .intent import Intent, Selector, load_intents, resolve_selectors  # noqa: E402,F401


class IntentReport(NamedTuple):
    n_src: np.ndarray          # int64, one entry per intent: src pods among the held rows
    n_dst: np.ndarray          # int64: dst pods
    pairs: np.ndarray          # int64: pairs considered
    reachable: np.ndarray      # int64: considered pairs with M[i, j] = 1
    violations: np.ndarray     # int64: deny: reachable; allow: pairs - reachable
    bad_sources: np.ndarray    # int64: src pods with at least one violating pair
    witness: np.ndarray        # int32 (K, 2): the smallest violating (i, j), or (-1, -1)
    ok: np.ndarray             # bool: violations == 0

    def failed(self) -> np.ndarray:
        """The indices of the violated intents, ascending."""
        return np.flatnonzero(~np.asarray(self.ok, dtype=bool))


def _intent_flags(eng, kind: str, self_pairs: bool) -> int:
    if kind not in ("deny", "allow"):
        raise ValueError(f"kind must be 'deny' or 'allow', not {kind!r}")
    return (eng.INTENT_ALLOW if kind == "allow" else 0) | (eng.INTENT_SELF if self_pairs else 0)


def check_intents(matrix: ReachabilityMatrix, containers: List[Container], intents,
                  self_pairs: bool = False) -> IntentReport:
    """Every intent of ``intents`` (Intent tuples, or (src, dst, kind)
    triples) against the matrix, in input order (see IntentReport)."""
    eng, n, _ = _group_engine(matrix, containers)
    intents = [Intent(*it) for it in intents]
    K = len(intents)
    flags = np.array([_intent_flags(eng, it.kind, self_pairs) for it in intents], dtype=np.int32)
    sets = resolve_selectors(containers, [it.src for it in intents] + [it.dst for it in intents])
    if n == 0 or K == 0:
        z = np.zeros(K, np.int64)
        return IntentReport(z, z.copy(), z.copy(), z.copy(), z.copy(), z.copy(),
                            np.full((K, 2), -1, np.int32), np.ones(K, bool))
    r = eng.intents(sets[:K], sets[K:], flags)
    o = r["out"]
    return IntentReport(*(o[:, f].copy() for f in range(6)), r["witness"], o[:, 4] == 0)


def intent_violations(matrix: ReachabilityMatrix, containers: List[Container], intent,
                      limit: int = 1_000_000, self_pairs: bool = False) -> np.ndarray:
    """One intent's violating (i, j) pairs as an int32 (T, 2) array, ascending
    by i then j (a row shard: the sources among its rows).  More than
    ``limit`` pairs raise OverflowError naming their number."""
    eng, n, _ = _group_engine(matrix, containers)
    it = Intent(*intent)
    flags = _intent_flags(eng, it.kind, self_pairs)
    if n == 0:
        return np.zeros((0, 2), np.int32)
    sets = resolve_selectors(containers, [it.src, it.dst])
    return eng.intent_pairs(sets[0], sets[1], flags, limit=limit)


# ---------------------------------------------------------------------------
# On which port.  Not part of kano_py's algorithm.py, whose maths ignore
# Policy.protocol: M[i, j] = 1 only says "reachable on some port".  With the
# port table of the matrix's current policies (kano/ports.py: slots 0 .. K-1
# the named (protocol, port) keys, slot K = ANY_OTHER, a bit mask per policy)
# and, as for pair_policies, the working sets of matrix._policies (current
# indices; accumulated lists, quirk Q5, and bits edited by hand do not enter),
#   subset(S)[i, j]  = 1 iff some p in S has i in select_p and j in allow_p
#   port_matrix(k)   = subset({p : masks[p] has bit k})   (several ports: the
#                      union of their slots)
#   pair_ports(i, j) = OR of masks[p] over pols(i, j)   (0 iff cover(i, j) = 0)
# computed on the device from the resident tables (kano_policy_subset /
# kano_pair_masks) without touching the matrix, for built and incrementally
# updated matrices alike.  A subset matrix is a rows-only ReachabilityMatrix
# on the device (over a row shard: the same rows), so every check above,
# matrix_diff, hop_*, group_reachability and check_intents read it.  Keys are
# opaque: no port ranges, no named-port resolution.  kano.k8s (kubesv ignores
# ports) and the parser stay as they are.

from .ports import ANY_OTHER, PortSet, PortTable, key_slots, port_key, port_table  # noqa: E402,F401


class PairPorts(NamedTuple):
    keys: list                 # the table's (protocol, port) keys, slot order
    masks: np.ndarray          # uint64 (Q, KW): bit k = open on slot k, bit K = ANY_OTHER

    def of(self, q: int) -> list:
        """The keys queried pair q is open on, in table order, ANY_OTHER last
        when the pair is open on the ports no policy names."""
        q = int(q)
        if not -len(self.masks) <= q < len(self.masks):
            raise IndexError("pair index out of range")
        names = list(self.keys) + [ANY_OTHER]
        return [names[k] for k in set_bit_indices(self.masks[q], len(names)).tolist()]

    def on(self, port) -> np.ndarray:
        """bool (Q,): the queried pairs open on the port (a (protocol, port)
        key, ANY_OTHER, or a list of those: open on any of them)."""
        m = np.zeros(self.masks.shape[1], dtype=np.uint64)
        for s in key_slots(list(self.keys), port):
            m[s >> 6] |= np.uint64(1) << np.uint64(s & 63)
        return (self.masks & m).any(axis=1)


def _engine_keep(eng, ids, indices, P: int) -> np.ndarray:
    """keep flags over the engine ids for current policy indices."""
    idx = np.asarray(list(indices), dtype=np.int64).reshape(-1)
    if idx.size and (idx.min() < -P or idx.max() >= P):
        raise IndexError("list index out of range")
    idx = np.where(idx < 0, idx + P, idx)
    keep = np.zeros(eng.nids(), dtype=np.uint8)
    keep[idx if ids is None else ids[0][idx]] = 1
    return keep


def _empty_like(matrix: ReachabilityMatrix) -> ReachabilityMatrix:
    """A rows-only matrix over the same pods, devices and rows, all zero."""
    from ._engine import DeviceBuild
    from .multi import MultiBuild
    src = _engine(matrix, whole=False)
    n = matrix.container_size
    out = ReachabilityMatrix.__new__(ReachabilityMatrix)
    out.container_size = n
    out._engine = (MultiBuild.empty(n, src.G, devices=src.devices)
                   if isinstance(src, MultiBuild)
                   else DeviceBuild.empty(n, device=src.device, rows=src.row_span))
    out._containers = None
    out._policies = None
    out._ncontainers = n
    out._lists = None
    return out


def policy_subset_matrix(matrix: ReachabilityMatrix, indices) -> ReachabilityMatrix:
    """The matrix of the policies ``indices`` alone (indices of the current
    policy list; duplicates are fine, an index out of range raises
    IndexError): what build_matrix over that sub-list gives, written on the
    device from the resident tables into a new rows-only matrix."""
    eng, _, ids, P = _pair_engine(matrix, [])
    keep = _engine_keep(eng, ids, indices, P) if P else None
    out = _empty_like(matrix)
    if P and matrix.container_size:
        try:
            out.subset_info = eng.subset_into(out._engine, keep)
        except BaseException:
            out._engine.close()
            raise
    return out


def _port_table(matrix: ReachabilityMatrix) -> PortTable:
    return port_table(matrix._policies)


def port_matrix(matrix: ReachabilityMatrix, port) -> ReachabilityMatrix:
    """The pairs reachable on ``port``: a (protocol, port) key, ANY_OTHER, or
    a list of those (reachable on any of them).  A key no policy names is
    ANY_OTHER's slot: only the any-port policies open it."""
    _pair_engine(matrix, [])
    t = _port_table(matrix)
    return policy_subset_matrix(matrix, np.flatnonzero(t.carries(t.slots(port))))


def pair_ports(matrix: ReachabilityMatrix, pairs) -> PairPorts:
    """For every (i, j) of ``pairs`` the ports the pair is open on (see
    PairPorts); a matrix holding a row shard answers for the pairs whose i it
    holds (the others get empty masks)."""
    eng, pr, ids, P = _pair_engine(matrix, pairs)
    t = _port_table(matrix)
    if P == 0 or pr.shape[0] == 0:
        return PairPorts(t.keys, np.zeros((pr.shape[0], t.KW), np.uint64))
    pm = np.zeros((eng.nids(), t.KW), dtype=np.uint64)
    pm[np.arange(P) if ids is None else ids[0]] = t.masks
    return PairPorts(t.keys, eng.pair_masks(pr, pm))


def reachable_on(matrix: ReachabilityMatrix, i: int, j: int, port) -> bool:
    """Whether pod i reaches pod j on ``port`` (as port_matrix's argument)."""
    return bool(pair_ports(matrix, [(int(i), int(j))]).on(port)[0])


def port_exposure(matrix: ReachabilityMatrix) -> Tuple[list, np.ndarray]:
    """(keys, int64 (K + 1,)): the pod pairs open on every slot of the port
    table, ANY_OTHER's last, over the held rows (the counts of row shards add
    up).  One subset matrix per slot into one reused destination, counted on
    the device."""
    eng, _, ids, P = _pair_engine(matrix, [])
    t = _port_table(matrix)
    n = matrix.container_size
    counts = np.zeros(t.KS, dtype=np.int64)
    if P == 0 or n == 0:
        return t.keys, counts
    out = _empty_like(matrix)
    try:
        z = np.zeros(n, dtype=np.int32)
        for k in range(t.KS):
            eng.subset_into(out._engine, _engine_keep(eng, ids, np.flatnonzero(t.carries([k])), P))
            counts[k] = out._engine.group_counts(z, z, 1, 1)["counts"][0, 0]
    finally:
        out._engine.close()
    return t.keys, counts


# ---------------------------------------------------------------------------
# Deny rules and tiers.  Not part of kano_py, whose policies only allow.  Over
# the working sets of the matrix's current policies every policy p carries an
# action (allow / deny) and an integer priority, a smaller number evaluated
# first (kano/verdicts.py: attributes set on the Policy objects, or an
# explicit Tiering).  p matches (i, j) iff i in select_p and j in allow_p;
# with t*(i, j) the smallest priority over the matching policies,
#   verdict(i, j) = none   nothing matches (unreachable: kano's reading)
#                   deny   some deny policy of priority t* matches (within one
#                          priority deny wins)
#                   allow  otherwise
#   verdict_matrix[i, j] = 1 iff verdict(i, j) = allow
# and the deciding policy is the smallest current index among the matching
# policies of priority t* with the winning action.  Computed on the device
# from the resident tables (kano_verdict_matrix / kano_pair_verdicts) without
# touching the matrix, for built and incrementally updated matrices alike.
# All-allow with any priorities is the built matrix; one priority for all is
# subset(allows) & ~subset(denies).  A verdict matrix is a rows-only
# ReachabilityMatrix like a subset matrix: every check above, matrix_diff,
# hop_*, group_reachability and check_intents read it.  Pass, the order of
# rules within a policy, YAML for AdminNetworkPolicy objects, bits edited by
# hand and the accumulated lists of quirk Q5 do not enter.

from .verdicts import ALLOW, DENY, VERDICT_NAMES, Tiering, tiering  # noqa: E402,F401
from . import verdicts as _verdicts  # noqa: E402


class PairVerdicts(NamedTuple):
    verdict: np.ndarray        # uint8 per queried pair: 0 none, 1 allow, 2 deny
    priority: np.ndarray       # int32: the deciding priority t* (0 where none)
    policy: np.ndarray         # int32: the deciding policy's current index, -1 where none

    def allowed(self) -> np.ndarray:
        """bool (Q,): the queried pairs whose verdict is allow."""
        return self.verdict == 1

    def denied(self) -> np.ndarray:
        """bool (Q,): the queried pairs a deny policy decides."""
        return self.verdict == 2

    def of(self, q: int) -> Tuple[str, Optional[int], Optional[int]]:
        """("allow" | "deny" | "none", priority or None, policy or None) of
        queried pair q."""
        q = int(q)
        if not -len(self.verdict) <= q < len(self.verdict):
            raise IndexError("pair index out of range")
        v = int(self.verdict[q])
        if v == 0:
            return "none", None, None
        return VERDICT_NAMES[v], int(self.priority[q]), int(self.policy[q])


def _engine_tiers(matrix: ReachabilityMatrix, eng, ids, tiers) -> Tuple[np.ndarray, np.ndarray]:
    """(priorities, actions) over the engine ids from the tiers of the current
    policies (the entries of removed ids stay 0: the engine ignores them)."""
    t = _verdicts.resolve(matrix._policies, tiers)
    prio = np.zeros(eng.nids(), dtype=np.int32)
    act = np.zeros(eng.nids(), dtype=np.uint8)
    at = np.arange(len(t)) if ids is None else ids[0]
    prio[at] = t.priorities
    act[at] = t.actions
    return prio, act


def verdict_matrix(matrix: ReachabilityMatrix, tiers=None) -> ReachabilityMatrix:
    """The pairs whose verdict is allow under the tiers (default: the ones the
    current policies carry, kano.verdicts.tiering), written on the device from
    the resident tables into a new rows-only matrix; ``verdict_info`` holds the
    alive allow and deny policies, the distinct priorities and the row classes
    with a deny policy."""
    eng, _, ids, P = _pair_engine(matrix, [])
    prio, act = _engine_tiers(matrix, eng, ids, tiers)
    out = _empty_like(matrix)
    out.verdict_info = dict(allow_policies=0, deny_policies=0, levels=0, deny_classes=0)
    if P and matrix.container_size:
        try:
            out.verdict_info = eng.verdict_into(out._engine, prio, act)
        except BaseException:
            out._engine.close()
            raise
    return out


def pair_verdicts(matrix: ReachabilityMatrix, pairs, tiers=None) -> PairVerdicts:
    """For every (i, j) of ``pairs`` the verdict, the deciding priority and the
    deciding policy (see PairVerdicts); a matrix holding a row shard answers
    for the pairs whose i it holds (the others get none)."""
    eng, pr, ids, P = _pair_engine(matrix, pairs)
    prio, act = _engine_tiers(matrix, eng, ids, tiers)
    Q = pr.shape[0]
    if P == 0 or Q == 0:
        return PairVerdicts(np.zeros(Q, np.uint8), np.zeros(Q, np.int32), np.full(Q, -1, np.int32))
    r = eng.pair_verdicts(pr, prio, act)
    pol = r["policy"]
    if ids is not None:
        pol = np.where(pol >= 0, ids[1][np.maximum(pol, 0)], -1).astype(np.int32)
    return PairVerdicts(r["verdict"], r["priority"], pol)


def pair_verdict(matrix: ReachabilityMatrix, i: int, j: int,
                 tiers=None) -> Tuple[str, Optional[int], Optional[int]]:
    """("allow" | "deny" | "none", priority or None, policy or None) of (i, j)."""
    return pair_verdicts(matrix, [(int(i), int(j))], tiers).of(0)


def why_blocked(matrix: ReachabilityMatrix, i: int, j: int, tiers=None) -> List[int]:
    """The ascending current indices of all deny policies of priority t* that
    match (i, j); [] when the pair is allowed or unmatched.  (pair_policies'
    list of the pair, filtered on the host.)"""
    hit = pair_policies(matrix, [(int(i), int(j))]).of(0)
    t = _verdicts.resolve(matrix._policies, tiers)      # (checked also where nothing matches)
    if not hit:
        return []
    best = min(int(t.priorities[p]) for p in hit)
    return [p for p in hit if int(t.priorities[p]) == best and t.actions[p] == DENY]


def verdict_counts(matrix: ReachabilityMatrix, tiers=None) -> Dict[str, int]:
    """{"allowed", "denied", "unmatched"}: the pod pairs of the held rows by
    verdict (the counts of row shards add up).  The verdict matrix and the
    matrix of all current policies are written into one reused destination and
    counted on the device, the way port_exposure counts."""
    eng, _, ids, P = _pair_engine(matrix, [])
    prio, act = _engine_tiers(matrix, eng, ids, tiers)
    n = matrix.container_size
    r0, r1 = getattr(eng, "row_span", None) or (0, n)
    total = (r1 - r0) * n
    if P == 0 or n == 0:
        return dict(allowed=0, denied=0, unmatched=total)
    out = _empty_like(matrix)
    try:
        z = np.zeros(n, dtype=np.int32)
        eng.verdict_into(out._engine, prio, act)
        allowed = int(out._engine.group_counts(z, z, 1, 1)["counts"][0, 0])
        eng.subset_into(out._engine, _engine_keep(eng, ids, range(P), P))
        matched = int(out._engine.group_counts(z, z, 1, 1)["counts"][0, 0])
    finally:
        out._engine.close()
    return dict(allowed=allowed, denied=matched - allowed, unmatched=total - matched)
