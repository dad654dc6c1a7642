"""One device-resident build of the reachability matrix (a kano_ctx).

Thin Python wrapper of the C ABI (include/kano_hip.h): uploads interned
tables, runs the build and the checks, and hands results back as numpy
arrays.  The drop-in API (model.py / algorithm.py) and the benchmark both
drive the engine through this class.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_int, c_int64, c_void_p
from typing import Optional, Tuple

import numpy as np

from . import _native as nat
from ._intern import Tables


def _ptr(a: Optional[np.ndarray]):
    # the address as an int: the argtypes are c_void_p, and ctypes converts
    # an int much faster than numpy's data_as builds a pointer object
    return None if a is None else a.ctypes.data


class PinnedBuffer:
    """Page-locked host memory (hipHostMalloc) viewed as a numpy array; D2H
    copies into it run at the full PCIe rate."""

    def __init__(self, nbytes: int):
        self._lib = nat.load()
        self._p = c_void_p()
        self.nbytes = max(int(nbytes), 16)
        nat.check(None, self._lib.kano_host_alloc(self.nbytes, byref(self._p)), "kano_host_alloc")

    def view(self, dtype, count: int) -> np.ndarray:
        dt = np.dtype(dtype)
        if count * dt.itemsize > self.nbytes:
            raise ValueError("pinned buffer too small")
        buf = (ctypes.c_char * (count * dt.itemsize)).from_address(self._p.value)
        return np.frombuffer(buf, dtype=dt, count=count)

    def close(self):
        if self._p:
            self._lib.kano_host_free(self._p)
            self._p = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuild:
    """A kano_ctx holding one build (or one row shard of it) on one GPU."""

    def __init__(self, tables: Optional[Tables] = None, device: int = 0,
                 rows: Optional[Tuple[int, int]] = None, path: str = "auto",
                 stream: Optional[int] = None, build: bool = True, lean: bool = False):
        self.lib = nat.load()
        self.ctx = c_void_p()
        self._owned = True            # close() destroys the context (not when adopted)
        # lean: kano_create_lean (no CU-masked write stream: builds the caller
        # waits for, the drop-in build_matrix)
        create = self.lib.kano_create_lean if lean else self.lib.kano_create
        rc = create(int(device), byref(self.ctx))
        if rc != 0:
            self.ctx = c_void_p()
            raise nat.KanoNativeError(
                f"kano_create(device={device}) failed (rc={rc}): no usable HIP device")
        self.device = device
        self.path = path
        self._counts = None
        self.row_span = None          # (r0, r1) when this context holds a row shard
        if stream is not None:
            self._chk(self.lib.kano_set_stream(self.ctx, c_void_p(stream)), "kano_set_stream")
        self.tables = None
        if tables is not None:
            self.upload(tables)
            if rows is not None:
                self.set_rows(*rows)
            if build:
                self.build(path)

    @classmethod
    def adopt(cls, ctx: c_void_p, device: int = 0, path: str = "auto") -> "DeviceBuild":
        """Wrap a context owned elsewhere (a kano_group member, kano/multi.py):
        its owner destroys it: this wrapper never does (close() only drops
        the handle)."""
        self = cls.__new__(cls)
        self.lib = nat.load()
        self.ctx = ctx
        self._owned = False
        self.device = device
        self.path = path
        self._counts = None
        self.row_span = None
        self.tables = None
        return self

    # -- plumbing -------------------------------------------------------
    def _chk(self, rc, what):
        nat.check(self.ctx, rc, what)

    def close(self):
        if self.ctx:
            if getattr(self, "_owned", True):
                self.lib.kano_destroy(self.ctx)
            self.ctx = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inputs / build -------------------------------------------------
    def set_policies(self, t: Tables) -> None:
        """kano_set_policies alone: another policy list over the pods already
        uploaded (t's pod columns must be the uploaded ones).  The engine keeps
        its pod classification when the new terms name the same label keys."""
        self.tables = t
        arrs = [np.ascontiguousarray(a, dtype=d) for a, d in (
            (t.sel_off, np.int64), (t.sel_col, np.int32), (t.sel_val, np.int32),
            (t.alw_off, np.int64), (t.alw_col, np.int32), (t.alw_val, np.int32))]
        self._chk(self.lib.kano_set_policies(self.ctx, t.P, *[_ptr(a) for a in arrs]),
                  "kano_set_policies")

    def upload(self, t: Tables) -> None:
        self.tables = t
        self.row_span = None          # kano_set_pods resets the engine to every row
        pv = np.ascontiguousarray(t.pod_val, dtype=np.int32)
        self._chk(self.lib.kano_set_pods(self.ctx, t.n, t.ncols, _ptr(pv)), "kano_set_pods")
        if getattr(t, "expr_col", None) is not None and len(t.expr_col):
            ex = [np.ascontiguousarray(a, dtype=d) for a, d in (
                (t.expr_col, np.int32), (t.expr_op, np.int32), (t.expr_off, np.int64),
                (t.expr_val, np.int32))]
            self._chk(self.lib.kano_set_expressions(self.ctx, len(ex[0]), *[_ptr(a) for a in ex]),
                      "kano_set_expressions")
        self.set_policies(t)

    def set_rows(self, r0: int, r1: int) -> None:
        self._chk(self.lib.kano_set_shard(self.ctx, int(r0), int(r1)), "kano_set_shard")
        n = self.info()["N"]          # the engine's own pod count (tables may be absent)
        self.row_span = None if (int(r0), int(r1)) == (0, n) else (int(r0), int(r1))

    @property
    def is_shard(self) -> bool:
        return self.row_span is not None

    def build(self, path: Optional[str] = None) -> None:
        p = nat.PATHS[path or self.path]
        self._chk(self.lib.kano_build(self.ctx, p), "kano_build")

    def build_classes(self, path: Optional[str] = None) -> None:
        """kano_build_classes: the build up to the class-level matrix; M is
        written on first use."""
        p = nat.PATHS[path or self.path]
        self._chk(self.lib.kano_build_classes(self.ctx, p), "kano_build_classes")

    def info(self) -> dict:
        out = np.zeros(nat.INFO_SLOTS, dtype=np.int64)
        self._chk(self.lib.kano_info(self.ctx, _ptr(out)), "kano_info")
        return {k: int(out[v]) for k, v in nat.INFO.items()}

    @property
    def n(self) -> int:
        return self.tables.n

    @property
    def W(self) -> int:
        return (self.tables.n + 63) >> 6

    @staticmethod
    def empty(n: int, device: int = 0, rows: Optional[Tuple[int, int]] = None) -> "DeviceBuild":
        """A context holding an n x n matrix (or its rows [r0, r1)) and no
        policies (the target of put_rows or of path_from / path_combine)."""
        z64 = np.zeros(1, np.int64)
        e = np.zeros(0, np.int32)
        t = Tables(int(n), 0, np.zeros((0, int(n)), np.int32), z64, e, e, z64, e, e)
        return DeviceBuild(t, device=device, rows=rows)

    def path_from(self, src: "DeviceBuild", hops: int = 2, mode: str = "auto") -> dict:
        """This context's matrix := the multi-hop reachability of src's
        matrix (kano_path; kubesv/kubesv/constraint.py:233-237)."""
        info = np.zeros(6, dtype=np.int64)
        self._chk(self.lib.kano_path(src.ctx, self.ctx, int(hops), nat.PATHS[mode], _ptr(info)),
                  "kano_path")
        keys = ("steps", "steps_run", "mfma_steps", "row_classes", "col_classes", "identity")
        return {k: int(v) for k, v in zip(keys, info)}

    def export_rows(self, r0: int, nrows: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Rows as bitarray bytes (big-endian bit order), (nrows, ceil(n/8))."""
        nb = (self.tables.n + 7) >> 3
        if out is None:
            out = np.empty((max(nrows, 0), nb), dtype=np.uint8)
        self._chk(self.lib.kano_export_rows(self.ctx, int(r0), int(nrows), _ptr(out)),
                  "kano_export_rows")
        return out

    def import_rows(self, r0: int, rows: np.ndarray) -> None:
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        self._chk(self.lib.kano_import_rows(self.ctx, int(r0), int(rows.shape[0]), _ptr(rows)),
                  "kano_import_rows")

    def k8s_edge_from(self, in_t: "DeviceBuild", eg_t: "DeviceBuild", self_traffic: bool,
                      all_pairs: bool, pods: bool = False, dst_is_egress: bool = False) -> int:
        """This context's matrix := kubesv's edge relation from the two
        per-direction builds (kano_k8s_edge; kubesv/kubesv/constraint.py:191-231).
        Returns the bits the product added beyond the self term."""
        info = np.zeros(1, dtype=np.int64)
        flags = ((1 if self_traffic else 0) | (2 if all_pairs else 0) | (4 if pods else 0) |
                 (8 if dst_is_egress else 0))
        self._chk(self.lib.kano_k8s_edge(in_t.ctx, eg_t.ctx, self.ctx, flags, _ptr(info)),
                  "kano_k8s_edge")
        return int(info[0])

    def k8s_conn_from(self, eg: "DeviceBuild", ing: "DeviceBuild", allow_self: bool = True,
                      keep_e=None, keep_i=None, form: str = "auto",
                      counts: bool = True) -> Optional[dict]:
        """This context's rows := the Kubernetes connectivity of the egress
        and ingress class-level builds (kano_k8s_conn).  ``keep_e`` /
        ``keep_i``: one flag per engine id of the build (None keeps all).
        ``form``: "direct", "stream" or "auto" (the engine picks); the same bits.
        ``counts``: return the call's info (the isolated pods, counted on the
        device, and the kept entries); False skips the counting and returns None."""
        fbits = (1 if allow_self else 0) | {"auto": 0, "direct": 2, "stream": 4}[form]
        def flags_of(keep, src):
            P = src.info()["P"]
            if keep is None:
                return P, None
            k = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, dtype=np.uint8)
            return int(k.shape[0]), k
        ne, ke = flags_of(keep_e, eg)
        ni, ki = flags_of(keep_i, ing)
        info = np.zeros(4, dtype=np.int64) if counts else None
        self._chk(self.lib.kano_k8s_conn(eg.ctx, ing.ctx, self.ctx, fbits, ne, _ptr(ke), ni,
                                         _ptr(ki), _ptr(info)), "kano_k8s_conn")
        if info is None:
            return None
        return dict(zip(("egress_isolated", "ingress_isolated", "egress_entries",
                         "ingress_entries"), map(int, info)))

    def k8s_conn_tiers_from(self, eg: "DeviceBuild", ing: "DeviceBuild", allow_self: bool,
                            code_e, np_level_e: int, code_i, np_level_i: int,
                            form: str = "auto"):
        """This context's rows := the connectivity of the two builds under
        AdminNetworkPolicy tiers (kano_k8s_conn_tiers).  ``code_e`` /
        ``code_i``: one uint32 per engine id, level * 4 + action (0 allow,
        1 deny, 2 pass, 3 isolates only; 0xffffffff dropped); ``np_level_*``:
        the NetworkPolicy tier's level.  Returns (egress_isolated,
        ingress_isolated, info): per pod "a live entry at np_level selects
        it", and the call's counts."""
        fbits = (1 if allow_self else 0) | {"auto": 0, "direct": 2, "stream": 4}[form]
        ce = np.ascontiguousarray(np.asarray(code_e).reshape(-1), dtype=np.uint32)
        ci = np.ascontiguousarray(np.asarray(code_i).reshape(-1), dtype=np.uint32)
        iso_e = np.zeros(self.n, dtype=np.uint8)
        iso_i = np.zeros(self.n, dtype=np.uint8)
        info = np.zeros(4, dtype=np.int64)
        self._chk(self.lib.kano_k8s_conn_tiers(
            eg.ctx, ing.ctx, self.ctx, fbits, int(ce.shape[0]), _ptr(ce), int(np_level_e),
            int(ci.shape[0]), _ptr(ci), int(np_level_i), _ptr(iso_e), _ptr(iso_i), _ptr(info)),
            "kano_k8s_conn_tiers")
        keys = ("egress_isolated", "ingress_isolated", "egress_entries", "ingress_entries")
        return iso_e.astype(bool), iso_i.astype(bool), dict(zip(keys, map(int, info)))

    def k8s_isolated(self) -> np.ndarray:
        """Per pod: some policy of this build selects it (kano_k8s_isolated)."""
        out = np.zeros(self.n, dtype=np.uint8)
        self._chk(self.lib.kano_k8s_isolated(self.ctx, _ptr(out)), "kano_k8s_isolated")
        return out.astype(bool)

    def k8s_conn_time(self) -> float:
        """The last k8s_conn_from's device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_k8s_conn_time(self.ctx, byref(ms)), "kano_k8s_conn_time")
        return float(ms.value)

    def k8s_pair_verdicts(self, ing: "DeviceBuild", pairs, allow_self: bool, code_e,
                          np_level_e: int, code_i, np_level_i: int) -> dict:
        """Which tier and entry decide each (src, dst) of ``pairs`` under the
        rule of k8s_conn_tiers_from (kano_k8s_pair_verdicts); this context is
        the egress build, ``ing`` the ingress build, codes and levels as
        there.  ``verdict`` (uint8: bit 0 allowed, 1 self, 2-3 egress tier,
        4 egress denies, 5-6 ingress tier, 7 ingress denies), per direction
        ``decider_*`` / ``passed_*`` (int32 engine ids, -1: none) and
        ``counts`` (int64[18])."""
        pairs, Q = _as_pairs(pairs)
        ce = np.ascontiguousarray(np.asarray(code_e).reshape(-1), dtype=np.uint32)
        ci = np.ascontiguousarray(np.asarray(code_i).reshape(-1), dtype=np.uint32)
        verdict = np.zeros(Q, dtype=np.uint8)
        ids = {k: np.full(Q, -1, dtype=np.int32)
               for k in ("decider_e", "passed_e", "decider_i", "passed_i")}
        counts = np.zeros(18, dtype=np.int64)
        self._chk(self.lib.kano_k8s_pair_verdicts(
            self.ctx, ing.ctx, 1 if allow_self else 0, Q, _ptr(pairs), int(ce.shape[0]), _ptr(ce),
            int(np_level_e), int(ci.shape[0]), _ptr(ci), int(np_level_i), _ptr(verdict),
            _ptr(ids["decider_e"]), _ptr(ids["passed_e"]), _ptr(ids["decider_i"]),
            _ptr(ids["passed_i"]), _ptr(counts)), "kano_k8s_pair_verdicts")
        return dict(pairs=pairs, verdict=verdict, counts=counts, **ids)

    def k8s_pair_verdicts_time(self) -> float:
        """The last k8s_pair_verdicts' device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_k8s_pair_verdicts_time(self.ctx, byref(ms)),
                  "kano_k8s_pair_verdicts_time")
        return float(ms.value)

    def k8s_rule_usage(self, ing: "DeviceBuild", allow_self: bool, code_e, np_level_e: int,
                       code_i, np_level_i: int, group_e=None, group_i=None) -> dict:
        """Per entry of the two builds the pairs of [0, n)^2 it decides and
        passes, per group the pairs only it allows, under the rule of
        k8s_pair_verdicts (kano_k8s_rule_usage); this context is the egress
        build, ``ing`` the ingress build, codes and levels as there.
        ``group_*``: an int32 per engine id, non-decreasing from 0 on (None:
        every id its own group).  ``allow_self`` leaves the n self pairs out.
        ``decided_*`` / ``passed_*`` (int64 per id), ``sole_*`` (int64 per
        group) and ``tiers`` (int64[16]: per direction and tier its (allow,
        deny) pairs)."""
        ce = np.ascontiguousarray(np.asarray(code_e).reshape(-1), dtype=np.uint32)
        ci = np.ascontiguousarray(np.asarray(code_i).reshape(-1), dtype=np.uint32)

        def groups_of(group, code):
            if group is None:
                return None, len(code)
            g = np.ascontiguousarray(np.asarray(group).reshape(-1), dtype=np.int32)
            if g.shape != code.shape:
                raise ValueError("one group per code expected")
            return g, int(g[-1]) + 1 if len(g) and g[-1] >= 0 else 0

        ge, ne = groups_of(group_e, ce)
        gi, ni = groups_of(group_i, ci)
        out = {"decided_e": np.zeros(len(ce), np.int64), "passed_e": np.zeros(len(ce), np.int64),
               "sole_e": np.zeros(ne, np.int64), "decided_i": np.zeros(len(ci), np.int64),
               "passed_i": np.zeros(len(ci), np.int64), "sole_i": np.zeros(ni, np.int64),
               "tiers": np.zeros(16, np.int64)}
        self._chk(self.lib.kano_k8s_rule_usage(
            self.ctx, ing.ctx, 1 if allow_self else 0, int(ce.shape[0]), _ptr(ce),
            int(np_level_e), _ptr(ge), int(ci.shape[0]), _ptr(ci), int(np_level_i), _ptr(gi),
            _ptr(out["decided_e"]), _ptr(out["passed_e"]), _ptr(out["sole_e"]),
            _ptr(out["decided_i"]), _ptr(out["passed_i"]), _ptr(out["sole_i"]),
            _ptr(out["tiers"])), "kano_k8s_rule_usage")
        return out

    def k8s_rule_usage_time(self) -> float:
        """The last k8s_rule_usage's device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_k8s_rule_usage_time(self.ctx, byref(ms)),
                  "kano_k8s_rule_usage_time")
        return float(ms.value)

    def path_shard_words(self) -> int:
        w = c_int64(0)
        self._chk(self.lib.kano_path_shard_words(self.ctx, byref(w)), "kano_path_shard_words")
        return int(w.value)

    def path_shard(self, t_dev_ptr: int) -> None:
        """This row shard's part of the path's one-hop table (device memory)."""
        self._chk(self.lib.kano_path_shard(self.ctx, c_void_p(t_dev_ptr)), "kano_path_shard")

    def path_combine(self, src: "DeviceBuild", gathered_dev_ptr: int, nranks: int,
                     hops: int = 2, mode: str = "auto") -> dict:
        """This context's rows := src's shard of the path matrix, from the
        ranks' gathered parts."""
        info = np.zeros(6, dtype=np.int64)
        self._chk(self.lib.kano_path_combine(src.ctx, self.ctx, c_void_p(gathered_dev_ptr),
                                             int(nranks), int(hops), nat.PATHS[mode],
                                             _ptr(info)), "kano_path_combine")
        keys = ("steps", "steps_run", "mfma_steps", "row_classes", "col_classes", "identity")
        return {k: int(v) for k, v in zip(keys, info)}

    # -- incremental updates ---------------------
    def add_policies(self, xval: np.ndarray, sel_csr, alw_csr) -> int:
        """Append policies (terms in this build's id space, kano._intern.
        intern_more); returns the first new engine id."""
        so, sc, sv = (np.ascontiguousarray(a, dtype=d) for a, d in
                      zip(sel_csr, (np.int64, np.int32, np.int32)))
        ao, ac, av = (np.ascontiguousarray(a, dtype=d) for a, d in
                      zip(alw_csr, (np.int64, np.int32, np.int32)))
        xv = np.ascontiguousarray(xval, dtype=np.int32)
        first = c_int64(0)
        self._chk(self.lib.kano_add_policies(
            self.ctx, int(so.shape[0] - 1), int(xv.shape[0]), _ptr(xv), _ptr(so), _ptr(sc),
            _ptr(sv), _ptr(ao), _ptr(ac), _ptr(av), byref(first)), "kano_add_policies")
        # (engine ids in use: the build's and every added one, removed or not)
        self._id_end = int(first.value) + int(so.shape[0] - 1)
        return int(first.value)

    def remove_policies(self, ids) -> None:
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        self._chk(self.lib.kano_remove_policies(self.ctx, int(a.shape[0]), _ptr(a)),
                  "kano_remove_policies")

    def added_policy_sets(self, eid: int) -> Tuple[np.ndarray, np.ndarray]:
        W = self.W
        s = np.zeros(W, dtype=np.uint64)
        a = np.zeros(W, dtype=np.uint64)
        self._chk(self.lib.kano_added_policy_sets(self.ctx, int(eid), _ptr(s), _ptr(a)),
                  "kano_added_policy_sets")
        return s, a

    # -- checks ---------------------------------------------------------
    def col_checks(self) -> Tuple[np.ndarray, np.ndarray]:
        W = self.W
        ca = np.zeros(W, dtype=np.uint64)
        co = np.zeros(W, dtype=np.uint64)
        self._chk(self.lib.kano_col_checks(self.ctx, _ptr(ca), _ptr(co)), "kano_col_checks")
        return ca, co

    def crosscheck(self, gid: np.ndarray) -> np.ndarray:
        gid = np.ascontiguousarray(gid, dtype=np.int32)
        if gid.shape[0] != self.n:
            raise ValueError("gid must have one entry per pod")
        out = np.zeros(self.W, dtype=np.uint64)
        self._chk(self.lib.kano_crosscheck(self.ctx, _ptr(gid), _ptr(out)), "kano_crosscheck")
        return out

    def col_flags_dev(self, flags_dev_ptr: int) -> None:
        self._chk(self.lib.kano_col_flags_dev(self.ctx, c_void_p(flags_dev_ptr)),
                  "kano_col_flags_dev")

    def crosscheck_dev(self, gid: np.ndarray, flags_dev_ptr: int) -> None:
        gid = np.ascontiguousarray(gid, dtype=np.int32)
        self._chk(self.lib.kano_crosscheck_dev(self.ctx, _ptr(gid), c_void_p(flags_dev_ptr)),
                  "kano_crosscheck_dev")

    # -- matrix access --------------------------------------------------
    def rows(self, r0: int, nrows: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        if out is None:
            out = np.zeros((nrows, self.W), dtype=np.uint64)
        self._chk(self.lib.kano_get_rows(self.ctx, int(r0), int(nrows), _ptr(out)),
                  "kano_get_rows")
        return out

    def rows_digest(self, r0: int, nrows: int) -> np.ndarray:
        """kano_rows_digest: one 64-bit digest per row (tests/_golden.py
        row_digest computes the same on the host)."""
        out = np.zeros(max(nrows, 1), dtype=np.uint64)
        self._chk(self.lib.kano_rows_digest(self.ctx, int(r0), int(nrows), _ptr(out)),
                  "kano_rows_digest")
        return out[:nrows]

    def put_rows(self, r0: int, words: np.ndarray) -> None:
        words = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, self.W)
        self._chk(self.lib.kano_put_rows(self.ctx, int(r0), words.shape[0], _ptr(words)),
                  "kano_put_rows")

    def col(self, j: int) -> np.ndarray:
        info = self.info()
        rl = info["ROW1"] - info["ROW0"]
        out = np.zeros((rl + 63) >> 6, dtype=np.uint64)
        self._chk(self.lib.kano_get_col(self.ctx, int(j), _ptr(out)), "kano_get_col")
        return out

    def get_bit(self, i: int, j: int) -> int:
        v = c_int()
        self._chk(self.lib.kano_get_bit(self.ctx, int(i), int(j), byref(v)), "kano_get_bit")
        return int(v.value)

    def set_bit(self, i: int, j: int, value) -> None:
        self._chk(self.lib.kano_set_bit(self.ctx, int(i), int(j), 1 if value else 0),
                  "kano_set_bit")

    def policy_sets(self, p: int, sel: bool = True, allow: bool = True):
        if self.tables is not None and p >= self.tables.P:   # an added policy
            s, a = self.added_policy_sets(p)
            return (s if sel else None), (a if allow else None)
        W = self.W
        s = np.zeros(W, dtype=np.uint64) if sel else None
        a = np.zeros(W, dtype=np.uint64) if allow else None
        self._chk(self.lib.kano_get_policy_sets(self.ctx, int(p), _ptr(s), _ptr(a)),
                  "kano_get_policy_sets")
        return s, a

    def classes(self) -> np.ndarray:
        out = np.zeros(self.n, dtype=np.int32)
        self._chk(self.lib.kano_get_classes(self.ctx, _ptr(out)), "kano_get_classes")
        return out

    def select_csr(self) -> Tuple[np.ndarray, np.ndarray]:
        info = self.info()
        off = np.zeros(info["U"] + 1, dtype=np.int64)
        pol = np.zeros(max(info["NNZ_SEL"], 1), dtype=np.int32)
        self._chk(self.lib.kano_get_select_csr(self.ctx, _ptr(off), _ptr(pol)),
                  "kano_get_select_csr")
        return off, pol[: info["NNZ_SEL"]]

    def allow_csr(self) -> Tuple[np.ndarray, np.ndarray]:
        info = self.info()
        off = np.zeros(info["P"] + 1, dtype=np.int64)
        pods = np.zeros(max(info["NNZ_ALW"], 1), dtype=np.int32)
        self._chk(self.lib.kano_get_allow_csr(self.ctx, _ptr(off), _ptr(pods)),
                  "kano_get_allow_csr")
        return off, pods[: info["NNZ_ALW"]]

    # -- policy checks --------------------------------------------------
    def shadow_count(self) -> int:
        cnt = c_int64()
        self._chk(self.lib.kano_shadow(self.ctx, byref(cnt)), "kano_shadow")
        return int(cnt.value)

    def shadow_fetch(self, count: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        if out is None:
            out = np.zeros((count, 2), dtype=np.int32)
        self._chk(self.lib.kano_shadow_fetch(self.ctx, _ptr(out)), "kano_shadow_fetch")
        return out

    def shadow(self) -> np.ndarray:
        return self.shadow_fetch(self.shadow_count())

    def set_groups(self, gid: np.ndarray, ngroups: int = 0) -> None:
        """kano_set_groups: upload the pods' group ids once (resident input);
        then ``verify(gid="stored")`` runs user_crosscheck on them."""
        gid = np.ascontiguousarray(gid, dtype=np.int32)
        if gid.shape[0] != self.n:
            raise ValueError("gid must have one entry per pod")
        self._chk(self.lib.kano_set_groups(self.ctx, _ptr(gid), int(ngroups)), "kano_set_groups")

    def _result_slots(self) -> None:
        # reused result slots (no per-call allocation)
        self._counts = np.zeros(4, dtype=np.int64)
        self._counts_p = self._counts.ctypes.data
        self._cnt = c_int64(0)
        self._cnt_ref = byref(self._cnt)
        self._bufs = (None, None, None, None)

    def _buf_ptrs(self, idx, pairs):
        # the caller's reused idx / pairs buffers: their addresses once (the
        # held references keep both arrays, and so their addresses, alive)
        b_idx, p_idx, b_pairs, p_pairs = self._bufs
        if idx is not b_idx or pairs is not b_pairs:
            b_idx, p_idx, b_pairs, p_pairs = idx, _ptr(idx), pairs, _ptr(pairs)
            self._bufs = (b_idx, p_idx, b_pairs, p_pairs)
        return p_idx, p_pairs

    def verify(self, gid=None, sys_row: int = 0, shadow: bool = True,
               pairs: Optional[np.ndarray] = None, idx: Optional[np.ndarray] = None,
               ngroups: int = 0, path: Optional[str] = None,
               shadow_count_only: bool = False) -> dict:
        """kano_verify: build + every check in one call (three host syncs).

        Returns the reference's result lists as int32 index arrays
        (``all_reachable``, ``all_isolated``, ``user_crosscheck`` (None without
        gid), ``system_isolation`` (None when sys_row is not in this shard))
        and, with ``shadow``, ``shadow_count`` plus ``pairs`` (a (count, 2)
        view of the given buffer when it is large enough, else fetched
        afterwards).  ``idx`` (>= 4*n int32, e.g. pinned) receives the lists.
        ``ngroups`` > 0 declares ``gid < ngroups`` (checked on the device).
        ``shadow_count_only``: policy_shadow's subset tests run and its pair
        count is returned, the pairs are not emitted (``pairs`` is None)."""
        n = self.n
        if idx is None:
            idx = np.empty(max(4 * n, 1), dtype=np.int32)
        elif idx.size < 4 * n:
            raise ValueError("idx buffer needs 4*n entries")
        stored = isinstance(gid, str) and gid == "stored"
        if stored:
            gid, ngroups = None, nat.STORED_GROUPS
        elif gid is not None:
            if not (isinstance(gid, np.ndarray) and gid.dtype == np.int32
                    and gid.flags.c_contiguous):
                gid = np.ascontiguousarray(gid, dtype=np.int32)
            if gid.shape[0] != n:
                raise ValueError("gid must have one entry per pod")
        if self._counts is None:
            self._result_slots()
        counts, cnt = self._counts, self._cnt
        cap = 0 if pairs is None else pairs.size // 2
        if shadow_count_only:
            cap = -1
        p_idx, p_pairs = self._buf_ptrs(idx, pairs)
        pth = nat.PATHS[path or self.path]
        rc = self.lib.kano_verify(self.ctx, pth, _ptr(gid), int(ngroups), int(sys_row), p_idx,
                                  self._counts_p, p_pairs, int(cap),
                                  self._cnt_ref if shadow else None)
        if rc != 0:
            self._chk(rc, "kano_verify")
        out, o = {}, 0
        for name, k in zip(("all_reachable", "all_isolated", "user_crosscheck",
                            "system_isolation"), counts.tolist()):
            out[name] = idx[o:o + k] if k >= 0 else None
            o += max(k, 0)
        if gid is None and not stored:
            out["user_crosscheck"] = None
        if shadow:
            k = int(cnt.value)
            out["shadow_count"] = k
            if shadow_count_only:
                out["pairs"] = None
            elif pairs is not None and k <= cap:
                out["pairs"] = pairs.reshape(-1)[:2 * k].reshape(k, 2)
            else:
                out["pairs"] = self.shadow_fetch(k)
        return out

    def verify_shard(self, words_dev_ptr: int, gid=None, sys_row: int = 0, shadow: bool = True,
                     ngroups: int = 0, path: Optional[str] = None,
                     shadow_count_only: bool = False) -> None:
        """kano_verify_shard: build this row shard and run its checks up to the
        column words, written (3*W u64, [OR | cross | NAND]) to the device
        buffer at ``words_dev_ptr``.  Asynchronous on the engine's stream;
        gather the ranks' words on that stream, then ``verify_combine``."""
        self._gid_keep = None
        if isinstance(gid, str) and gid == "stored":
            gid, ngroups = None, nat.STORED_GROUPS
        elif gid is not None:
            gid = np.ascontiguousarray(gid, dtype=np.int32)
            if gid.shape[0] != self.n:
                raise ValueError("gid must have one entry per pod")
            self._gid_keep = gid
        self._shard_shadow = bool(shadow)
        pth = nat.PATHS[path or self.path]
        mode = (2 if shadow_count_only else 1) if shadow else 0
        self._chk(self.lib.kano_verify_shard(self.ctx, pth, _ptr(gid), int(ngroups), int(sys_row),
                                             mode, c_void_p(words_dev_ptr)),
                  "kano_verify_shard")

    def verify_gather(self, comm_ptr: int, nranks: int, gid=None, sys_row: int = 0,
                      shadow: bool = True, pairs: Optional[np.ndarray] = None,
                      idx: Optional[np.ndarray] = None, ngroups: int = 0,
                      path: Optional[str] = None, shadow_count_only: bool = False) -> dict:
        """kano_verify_gather: ``verify_shard``, the ranks' all-gather and
        ``verify_combine`` in one engine call, the all-gather issued by the
        engine on its stream through the RCCL communicator ``comm_ptr``
        (an ncclComm_t over ``nranks`` ranks, e.g. torch's
        ``ProcessGroupNCCL._comm_ptr()``).  Results as ``verify_combine``."""
        if isinstance(gid, str) and gid == "stored":
            gid, ngroups = None, nat.STORED_GROUPS
        elif gid is not None:
            gid = np.ascontiguousarray(gid, dtype=np.int32)
            if gid.shape[0] != self.n:
                raise ValueError("gid must have one entry per pod")
        self._shard_shadow = bool(shadow)
        pth = nat.PATHS[path or self.path]
        mode = (2 if shadow_count_only else 1) if shadow else 0
        return self._combine_call(
            lambda idx_p, cnt_p, pairs_p, cap, cnt_ref: self.lib.kano_verify_gather(
                self.ctx, pth, _ptr(gid), int(ngroups), int(sys_row), mode, c_void_p(comm_ptr),
                int(nranks), idx_p, cnt_p, pairs_p, cap, cnt_ref),
            "kano_verify_gather", pairs, idx, shadow_count_only)

    def checks_shard(self, words_dev_ptr: int, gid=None, sys_row: int = 0,
                     ngroups: int = 0) -> None:
        """kano_checks_shard: this shard's column words from the matrix as
        it stands (after add_policies / remove_policies); finish with
        ``verify_combine``."""
        self._gid_keep = None
        if isinstance(gid, str) and gid == "stored":
            gid, ngroups = None, nat.STORED_GROUPS
        elif gid is not None:
            gid = np.ascontiguousarray(gid, dtype=np.int32)
            if gid.shape[0] != self.n:
                raise ValueError("gid must have one entry per pod")
            self._gid_keep = gid
        self._shard_shadow = False
        self._chk(self.lib.kano_checks_shard(self.ctx, _ptr(gid), int(ngroups), int(sys_row),
                                             c_void_p(words_dev_ptr)), "kano_checks_shard")

    def verify_combine(self, gathered_dev_ptr: int, nranks: int, cross: bool = True,
                       pairs: Optional[np.ndarray] = None,
                       idx: Optional[np.ndarray] = None,
                       shadow_count_only: bool = False) -> dict:
        """kano_verify_combine: OR the gathered word sets of ``nranks`` shards
        and return the results like ``verify`` (column lists global, the
        system row and the shadow pairs of this shard)."""
        out = self._combine_call(
            lambda idx_p, cnt_p, pairs_p, cap, cnt_ref: self.lib.kano_verify_combine(
                self.ctx, c_void_p(gathered_dev_ptr), int(nranks), idx_p, cnt_p, pairs_p, cap,
                cnt_ref),
            "kano_verify_combine", pairs, idx, shadow_count_only)
        if not cross:
            out["user_crosscheck"] = None
        return out

    def _combine_call(self, call, what, pairs, idx, shadow_count_only) -> dict:
        """The combine half's outputs (verify_combine, verify_gather)."""
        n = self.n
        if idx is None:
            idx = np.empty(max(4 * n, 1), dtype=np.int32)
        elif idx.size < 4 * n:
            raise ValueError("idx buffer needs 4*n entries")
        if self._counts is None:
            self._result_slots()
        counts, cnt = self._counts, self._cnt
        shadow = self._shard_shadow
        cap = 0 if pairs is None else pairs.size // 2
        if shadow_count_only:
            cap = -1
        p_idx, p_pairs = self._buf_ptrs(idx, pairs)
        rc = call(p_idx, self._counts_p, p_pairs, int(cap), self._cnt_ref if shadow else None)
        if rc != 0:
            self._chk(rc, what)
        out, o = {}, 0
        for name, k in zip(("all_reachable", "all_isolated", "user_crosscheck",
                            "system_isolation"), counts.tolist()):
            out[name] = idx[o:o + k] if k >= 0 else None
            o += max(k, 0)
        if shadow:
            k = int(cnt.value)
            out["shadow_count"] = k
            if shadow_count_only:
                out["pairs"] = None
            elif pairs is not None and k <= cap:
                out["pairs"] = pairs.reshape(-1)[:2 * k].reshape(k, 2)
            else:
                out["pairs"] = self.shadow_fetch(k)
        return out

    def conflict_raises(self) -> bool:
        v = c_int()
        self._chk(self.lib.kano_conflict(self.ctx, byref(v)), "kano_conflict")
        return bool(v.value)

    # -- the working policy_conflict (kano_conflict_pairs) ---------------
    def _conflict_run(self, mode: int) -> Tuple[int, int]:
        cnt, ncls = c_int64(), c_int64()
        self._chk(self.lib.kano_conflict_pairs(self.ctx, int(mode), byref(cnt), byref(ncls)),
                  "kano_conflict_pairs")
        return int(cnt.value), int(ncls.value)

    def conflict_count(self) -> int:
        """Pairs (j, k) of policies selecting a common pod of this context's
        rows with disjoint allow sets, counted only (no pairs on the device)."""
        return self._conflict_run(1)[0]

    def conflict_fetch(self, count: int, out: Optional[np.ndarray] = None) -> np.ndarray:
        if out is None:
            out = np.zeros((count, 2), dtype=np.int32)
        self._chk(self.lib.kano_conflict_fetch(self.ctx, _ptr(out)), "kano_conflict_fetch")
        return out

    def conflict(self) -> np.ndarray:
        """The pairs as a (count, 2) int32 array, in container order."""
        return self.conflict_fetch(self._conflict_run(0)[0])

    def conflict_classes(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Class level: (off, pairs, members) -- row class c's conflicting
        pairs are pairs[off[c]:off[c + 1]], shared by its members[c] pods."""
        ncls = self._conflict_run(1)[1]
        U = self.info()["U"]
        off = np.zeros(U + 1, dtype=np.int64)
        pairs = np.zeros((ncls, 2), dtype=np.int32)
        members = np.zeros(U, dtype=np.int32)
        self._chk(self.lib.kano_conflict_classes(self.ctx, _ptr(off), _ptr(pairs), _ptr(members)),
                  "kano_conflict_classes")
        return off, pairs, members

    # -- policy_impact / policy_redundant (kano_policy_impact) -----------
    def policy_impact(self) -> np.ndarray:
        """impact[p]: the pod pairs (i, j), i in this context's rows, that only
        policy p allows -- what removing p alone takes away.  int64, length P."""
        out = np.zeros(self.info()["P"], dtype=np.int64)
        self._chk(self.lib.kano_policy_impact(self.ctx, 0, _ptr(out), None, None),
                  "kano_policy_impact")
        return out

    def policy_essential(self) -> np.ndarray:
        """essential[p]: impact[p] > 0, without the sums.  bool, length P."""
        out = np.zeros(self.info()["P"], dtype=np.uint8)
        self._chk(self.lib.kano_policy_impact(self.ctx, 1, None, _ptr(out), None),
                  "kano_policy_impact")
        return out.astype(bool)

    # -- pair_policies (kano_pair_policies) -------------------------------
    def pair_policies(self, pairs, lists: bool = True, hist: bool = False,
                      nids: Optional[int] = None) -> dict:
        """Which of the matrix's current policies allow each pod pair of
        ``pairs`` ((Q, 2) int32: i selected, j allowed): ``cover`` (int32, Q),
        with ``lists`` also ``offsets`` (int64, Q + 1) and ``policies`` (int32:
        pair q's ascending engine ids are policies[offsets[q]:offsets[q + 1]];
        else both None), with ``hist`` the queried pairs every engine id
        allows (int64; else None).  Works after add_policies /
        remove_policies; a row shard answers for the pairs whose i it holds
        (the others get cover 0).  ``nids``: the engine ids in use (default:
        the build's policies and the ones added through this object)."""
        pr, Q = _as_pairs(pairs)
        if nids is None:            # (the added ids follow the build's P)
            nids = max(self.info()["P"], getattr(self, "_id_end", 0))
        return _pair_call(
            lambda *out: self.lib.kano_pair_policies(self.ctx, Q, _ptr(pr), 0 if lists else 1,
                                                     *out),
            self, "kano_pair_policies", Q, lists, int(nids) if hist else None)

    def pair_policies_time(self) -> float:
        """The last pair_policies' device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_pair_policies_time(self.ctx, byref(ms)),
                  "kano_pair_policies_time")
        return float(ms.value)

    # -- port_matrix / pair_ports (kano_policy_subset / kano_pair_masks) --
    def nids(self) -> int:
        """The engine ids in use: the build's and every added one, removed or
        not (the length of subset_into's ``keep`` and pair_masks' ``pmask``)."""
        return max(self.info()["P"], getattr(self, "_id_end", 0))

    def subset_into(self, dst: "DeviceBuild", keep) -> dict:
        """dst's rows := the matrix of the kept policies (kano_policy_subset):
        ``keep`` holds one flag per engine id (the build's, then the added
        ones; removed ids are ignored).  ``dst`` is a matrix context of the
        same n, device and rows (DeviceBuild.empty(n, rows=...)); this
        context's matrix and tables are not written."""
        k = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, dtype=np.uint8)
        info = np.zeros(3, dtype=np.int64)
        dst._chk(self.lib.kano_policy_subset(self.ctx, dst.ctx, int(k.shape[0]), _ptr(k),
                                             _ptr(info)), "kano_policy_subset")
        return dict(zip(("kept_build", "kept_added", "kept_classes"), map(int, info)))

    def pair_masks(self, pairs, pmask) -> np.ndarray:
        """The OR of ``pmask``'s rows ((engine ids, KW) uint64) over the
        policies allowing each pod pair of ``pairs`` (kano_pair_masks): uint64
        (Q, KW), zero where no policy does.  A row shard answers for the pairs
        whose i it holds (the others get zeros)."""
        pr, Q = _as_pairs(pairs)
        pm = np.ascontiguousarray(pmask, dtype=np.uint64)
        if pm.ndim != 2 or pm.shape[1] < 1:
            raise ValueError("pmask must be an (engine ids, KW >= 1) array")
        out = np.zeros((Q, pm.shape[1]), dtype=np.uint64)
        self._chk(self.lib.kano_pair_masks(self.ctx, Q, _ptr(pr), int(pm.shape[0]),
                                           int(pm.shape[1]), _ptr(pm), _ptr(out)),
                  "kano_pair_masks")
        return out

    def subset_time(self) -> float:
        """The last subset_into's device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_policy_subset_time(self.ctx, byref(ms)),
                  "kano_policy_subset_time")
        return float(ms.value)

    def pair_masks_time(self) -> float:
        """The last pair_masks' device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_pair_masks_time(self.ctx, byref(ms)), "kano_pair_masks_time")
        return float(ms.value)

    # -- verdict_matrix / pair_verdicts (kano_verdict_matrix / kano_pair_verdicts)
    @staticmethod
    def _tiers(prio, action):
        """int32 priorities and uint8 actions (0 allow, 1 deny), one per engine id."""
        pr = np.ascontiguousarray(np.asarray(prio).reshape(-1), dtype=np.int32)
        ac = np.ascontiguousarray(np.asarray(action).reshape(-1), dtype=np.uint8)
        if pr.shape != ac.shape:
            raise ValueError(f"{pr.shape[0]} priorities for {ac.shape[0]} actions")
        return pr, ac

    def verdict_into(self, dst: "DeviceBuild", prio, action) -> dict:
        """dst's rows := the pairs whose verdict is allow (kano_verdict_matrix):
        ``prio`` (int32: a smaller number is evaluated first) and ``action``
        (0 allow, 1 deny) hold one entry per engine id (the build's, then the
        added ones; removed ids are ignored).  ``dst`` as subset_into's; this
        context's matrix and tables are not written."""
        pr, ac = self._tiers(prio, action)
        info = np.zeros(4, dtype=np.int64)
        dst._chk(self.lib.kano_verdict_matrix(self.ctx, dst.ctx, int(pr.shape[0]), _ptr(pr),
                                              _ptr(ac), _ptr(info)), "kano_verdict_matrix")
        return dict(zip(("allow_policies", "deny_policies", "levels", "deny_classes"),
                        map(int, info)))

    def pair_verdicts(self, pairs, prio, action) -> dict:
        """The verdict of each pod pair of ``pairs`` (kano_pair_verdicts):
        ``verdict`` (uint8: 0 none, 1 allow, 2 deny), ``priority`` (int32: the
        deciding priority, 0 where none), ``policy`` (int32: the deciding
        engine id, -1 where none) and ``counts`` (int64: none, allow, deny over
        the pairs whose i this context holds).  A row shard answers for the
        pairs whose i it holds (the others get verdict 0 and policy -1)."""
        pairs, Q = _as_pairs(pairs)
        pr, ac = self._tiers(prio, action)
        verdict = np.zeros(Q, dtype=np.uint8)
        priority = np.zeros(Q, dtype=np.int32)
        policy = np.full(Q, -1, dtype=np.int32)
        counts = np.zeros(3, dtype=np.int64)
        self._chk(self.lib.kano_pair_verdicts(self.ctx, Q, _ptr(pairs), int(pr.shape[0]), _ptr(pr),
                                              _ptr(ac), _ptr(verdict), _ptr(priority),
                                              _ptr(policy), _ptr(counts)), "kano_pair_verdicts")
        return dict(verdict=verdict, priority=priority, policy=policy, counts=counts)

    def verdict_time(self) -> float:
        """The last verdict_into's device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_verdict_matrix_time(self.ctx, byref(ms)),
                  "kano_verdict_matrix_time")
        return float(ms.value)

    def pair_verdicts_time(self) -> float:
        """The last pair_verdicts' device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_pair_verdicts_time(self.ctx, byref(ms)),
                  "kano_pair_verdicts_time")
        return float(ms.value)

    # -- matrix_diff (kano_diff / kano_diff_pairs / kano_copy_matrix) -----
    DIFF_KINDS = {"added": 0, "removed": 1}

    def diff(self, other: "DeviceBuild", rows: bool = True, cols: bool = True) -> dict:
        """What ``other`` (B) holds and this context (A) does not, and the
        reverse, over the rows both hold: ``added`` / ``removed`` (int),
        ``row_added`` / ``row_removed`` (int32 per local row) and
        ``col_added`` / ``col_removed`` (u64 words: columns that gained / lost
        a source).  ``rows=False`` / ``cols=False`` leave those arrays out
        (None); without both only the totals are computed."""
        info = self.info()
        rl, W = max(info["ROW1"] - info["ROW0"], 0), info["W"]
        tot = np.zeros(2, dtype=np.int64)
        ra = np.zeros(rl, dtype=np.int32) if rows else None
        rr = np.zeros(rl, dtype=np.int32) if rows else None
        ca = np.zeros(W, dtype=np.uint64) if cols else None
        cr = np.zeros(W, dtype=np.uint64) if cols else None
        # (errors are reported on the second context)
        nat.check(other.ctx, self.lib.kano_diff(self.ctx, other.ctx, _ptr(tot), _ptr(ra), _ptr(rr),
                                                _ptr(ca), _ptr(cr)), "kano_diff")
        return dict(added=int(tot[0]), removed=int(tot[1]), row_added=ra, row_removed=rr,
                    col_added=ca, col_removed=cr)

    def diff_count(self, other: "DeviceBuild", kind, r0: int, nrows: int) -> int:
        """The number of pairs ``diff_pairs`` would return."""
        cnt = c_int64(0)
        k = self.DIFF_KINDS.get(kind, kind)
        nat.check(other.ctx, self.lib.kano_diff_pairs(self.ctx, other.ctx, int(k), int(r0),
                                                      int(nrows), 0, byref(cnt), None),
                  "kano_diff_pairs")
        return int(cnt.value)

    def diff_pairs(self, other: "DeviceBuild", kind, r0: int, nrows: int,
                   limit: int = 1_000_000) -> np.ndarray:
        """The (i, j) pairs of one kind ("added": in ``other`` only, "removed":
        in this context only; or 0 / 1) in rows [r0, r0 + nrows), int32 (T, 2),
        ascending by i then j.  More than ``limit`` pairs raise OverflowError."""
        count = self.diff_count(other, kind, r0, nrows)
        if count > int(limit):
            raise OverflowError(f"{count} pairs exceed the limit of {int(limit)}")
        out = np.empty((count, 2), dtype=np.int32)
        if count:
            cnt = c_int64(0)
            k = self.DIFF_KINDS.get(kind, kind)
            nat.check(other.ctx, self.lib.kano_diff_pairs(self.ctx, other.ctx, int(k), int(r0),
                                                          int(nrows), count, byref(cnt),
                                                          _ptr(out)), "kano_diff_pairs")
        return out

    def copy_from(self, src: "DeviceBuild") -> None:
        """This context's rows := src's rows, on the device (kano_copy_matrix)."""
        self._chk(self.lib.kano_copy_matrix(src.ctx, self.ctx), "kano_copy_matrix")

    def diff_time(self) -> float:
        """The last diff's device time (ms) with this context as ``other``
        (KANO_TUNE=timing=1; kano_diff_time)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_diff_time(self.ctx, byref(ms)), "kano_diff_time")
        return float(ms.value)

    # -- group_reachability (kano_group_counts) ----------------------------
    def group_counts(self, gs, gd, Gs: Optional[int] = None, Gd: Optional[int] = None,
                     rows: bool = False) -> dict:
        """The matrix's quotient by a source and a destination labelling of
        the pods (int32 ids over all n pods; a negative id leaves the pod
        out): ``counts`` (int64, Gs x Gd) over the rows this context holds
        and, with ``rows``, ``row_counts`` (int32, one row of Gd counts per
        held row; else None).  ``Gs`` / ``Gd`` default to the largest id + 1
        (at least 1)."""
        info = self.info()
        n, rl = info["N"], max(info["ROW1"] - info["ROW0"], 0)
        gs = np.ascontiguousarray(gs, dtype=np.int32).reshape(-1)
        gd = np.ascontiguousarray(gd, dtype=np.int32).reshape(-1)
        if gs.shape[0] != n or gd.shape[0] != n:
            raise ValueError("gs and gd must have one entry per pod")
        if Gs is None:
            Gs = max(int(gs.max()) + 1, 1) if n else 1
        if Gd is None:
            Gd = max(int(gd.max()) + 1, 1) if n else 1
        Gs, Gd = int(Gs), int(Gd)
        counts = np.zeros((max(Gs, 0), max(Gd, 0)), dtype=np.int64)
        rc = np.zeros((rl, max(Gd, 0)), dtype=np.int32) if rows else None
        self._chk(self.lib.kano_group_counts(self.ctx, _ptr(gs), Gs, _ptr(gd), Gd, _ptr(counts),
                                             _ptr(rc)), "kano_group_counts")
        return dict(counts=counts, row_counts=rc)

    def group_counts_time(self) -> float:
        """The last group_counts' device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_group_counts_time(self.ctx, byref(ms)), "kano_group_counts_time")
        return float(ms.value)

    # -- hop_distance / path_witness (kano_hops / kano_hop_pairs) -----------
    HOPS_INFO = ("levels", "rows_ored", "batches", "reached")

    def hops(self, sources, max_hops: int = 0) -> dict:
        """Shortest distances from every pod of ``sources`` over the matrix
        read as a graph: ``dist`` (int32, (S, n); -1: no walk of >= 1 edges,
        or none within ``max_hops`` > 0) and ``info`` (levels run, rows OR-ed,
        batches, pods reached).  The context must hold every row."""
        src = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        n = self.info()["N"]
        dist = np.empty((src.shape[0], n), dtype=np.int32)
        info = np.zeros(4, dtype=np.int64)
        self._chk(self.lib.kano_hops(self.ctx, int(src.shape[0]), _ptr(src), int(max_hops),
                                     _ptr(dist), _ptr(info)), "kano_hops")
        return dict(dist=dist, info={k: int(v) for k, v in zip(self.HOPS_INFO, info)})

    def hop_pairs(self, pairs, max_hops: int = 0, paths: bool = False) -> dict:
        """``dist`` (int32, Q) of every (source, target) pair of ``pairs``
        ((Q, 2) int32, any order, duplicates allowed) and, with ``paths``, the
        canonical shortest paths: pair q's nodes are
        nodes[offsets[q]:offsets[q + 1]] (dist[q] + 1 of them, none when
        dist[q] < 0); else ``offsets`` and ``nodes`` are None."""
        pr, Q = _as_pairs(pairs)
        dist = np.empty(Q, dtype=np.int32)
        total = c_int64(0)
        self._chk(self.lib.kano_hop_pairs(self.ctx, Q, _ptr(pr), int(max_hops), int(bool(paths)),
                                          _ptr(dist), byref(total)), "kano_hop_pairs")
        if not paths:
            return dict(dist=dist, offsets=None, nodes=None)
        off = np.zeros(Q + 1, dtype=np.int64)
        np.cumsum(np.where(dist >= 1, dist.astype(np.int64) + 1, 0), out=off[1:])
        nodes = np.zeros(int(total.value), dtype=np.int32)
        self._chk(self.lib.kano_hop_pairs_fetch(self.ctx, _ptr(nodes)), "kano_hop_pairs_fetch")
        return dict(dist=dist, offsets=off, nodes=nodes)

    def hops_time(self) -> float:
        """The last hops / hop_pairs' device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_hops_time(self.ctx, byref(ms)), "kano_hops_time")
        return float(ms.value)

    # -- reverse_matrix / reach_zones (kano_reverse / kano_zones) -----------
    def reverse_into(self, dst: "DeviceBuild") -> dict:
        """``dst``'s matrix := this context's matrix transposed, on the device
        (kano_reverse): row t of ``dst`` is the set of pods that reach t.
        Both contexts hold every row of matrices of the same n.  Returns
        ``bits`` (set in the result) and ``tiles`` (launched)."""
        info = np.zeros(2, dtype=np.int64)
        # (errors are reported on the destination)
        nat.check(dst.ctx, self.lib.kano_reverse(self.ctx, dst.ctx, _ptr(info)), "kano_reverse")
        return dict(bits=int(info[0]), tiles=int(info[1]))

    def reverse_time(self) -> float:
        """The last reverse_into's device time with this context as ``dst``
        (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_reverse_time(self.ctx, byref(ms)), "kano_reverse_time")
        return float(ms.value)

    def zones(self, other: "DeviceBuild", counts: bool = True) -> dict:
        """Per pod i over this context's matrix A and ``other``'s B (the same
        n, every row): ``label`` = min({i} | {j : A[i,j] and B[i,j]}) (int32)
        and, with ``counts``, ``fan_out`` = popcount(A[i]), ``fan_in`` =
        popcount(B[i]) (int32) and ``cyclic`` = A[i,i] (bool); else those are
        None and a row stops at its first common bit.  ``zones`` is the number
        of distinct labels, ``moved`` the pods with label[i] != i."""
        n = self.info()["N"]
        label = np.empty(n, dtype=np.int32)
        fo = np.empty(n, dtype=np.int32) if counts else None
        fi = np.empty(n, dtype=np.int32) if counts else None
        cy = np.empty(n, dtype=np.uint8) if counts else None
        info = np.zeros(2, dtype=np.int64)
        self._chk(self.lib.kano_zones(self.ctx, other.ctx, _ptr(label), _ptr(fo), _ptr(fi),
                                      _ptr(cy), _ptr(info)), "kano_zones")
        return dict(label=label, fan_out=fo, fan_in=fi,
                    cyclic=cy.astype(bool) if counts else None,
                    zones=int(info[0]), moved=int(info[1]))

    def zones_time(self) -> float:
        """The last zones' device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_zones_time(self.ctx, byref(ms)), "kano_zones_time")
        return float(ms.value)

    # -- check_intents (kano_intents / kano_intent_pairs) -------------------
    INTENT_ALLOW, INTENT_SELF = 1, 2     # flag bits
    INTENT_RUN_ROWS = 16                 # csrc/kano_intents.hpp INTENT_R: rows of a work item at least
    INTENT_MAX_WORDS = 1 << 27           # K * W words of one kano_intents call
    INTENT_FIELDS = ("n_src", "n_dst", "pairs", "reachable", "violations", "bad_sources")

    def _intent_sets(self, src, dst, K: int) -> Tuple[np.ndarray, np.ndarray, int]:
        W = self.info()["W"]
        sets = []
        for a in (src, dst):
            a = np.ascontiguousarray(a, dtype=np.uint64)
            if a.size != K * W:
                raise ValueError(f"{K} sets of {W} words expected, got {a.size} words")
            sets.append(a.reshape(K, W))
        return sets[0], sets[1], W

    def intents(self, src, dst, flags) -> dict:
        """K intents at once: ``src`` / ``dst`` are (K, W) u64 bit sets over
        the pods, ``flags`` K int32 (INTENT_ALLOW: an allow intent, else deny;
        INTENT_SELF: the pairs (i, i) count).  Returns ``out`` (int64 (K, 6):
        INTENT_FIELDS, over the sources among the rows this context holds)
        and ``witness`` (int32 (K, 2): the smallest violating (i, j), or
        (-1, -1)).  A call of more than INTENT_MAX_WORDS set words a side goes
        to the library in slices of K."""
        flags = np.ascontiguousarray(flags, dtype=np.int32).reshape(-1)
        K = int(flags.shape[0])
        src, dst, W = self._intent_sets(src, dst, K)
        out = np.zeros((K, 6), dtype=np.int64)
        wit = np.full((K, 2), -1, dtype=np.int32)
        step = max(1, self.INTENT_MAX_WORDS // max(W, 1))
        for k0 in range(0, K, step):
            k1 = min(K, k0 + step)
            self._chk(self.lib.kano_intents(self.ctx, k1 - k0, _ptr(src[k0:k1]), _ptr(dst[k0:k1]),
                                            _ptr(flags[k0:k1]), _ptr(out[k0:k1]),
                                            _ptr(wit[k0:k1])), "kano_intents")
        return dict(out=out, witness=wit)

    def intent_count(self, src, dst, flags: int) -> int:
        """The number of pairs ``intent_pairs`` would return."""
        src, dst, _ = self._intent_sets(src, dst, 1)
        cnt = c_int64(0)
        self._chk(self.lib.kano_intent_pairs(self.ctx, _ptr(src), _ptr(dst), int(flags), 0,
                                             byref(cnt), None), "kano_intent_pairs")
        return int(cnt.value)

    def intent_pairs(self, src, dst, flags: int, limit: int = 1_000_000) -> np.ndarray:
        """One intent's violating (i, j) pairs among the held rows, int32
        (T, 2), ascending by i then j.  More than ``limit`` pairs raise
        OverflowError."""
        count = self.intent_count(src, dst, flags)
        if count > int(limit):
            raise OverflowError(f"{count} pairs exceed the limit of {int(limit)}")
        out = np.empty((count, 2), dtype=np.int32)
        if count:
            src, dst, _ = self._intent_sets(src, dst, 1)
            cnt = c_int64(0)
            self._chk(self.lib.kano_intent_pairs(self.ctx, _ptr(src), _ptr(dst), int(flags), count,
                                                 byref(cnt), _ptr(out)), "kano_intent_pairs")
        return out

    def intents_time(self) -> float:
        """The last intents' device time (ms; KANO_TUNE=timing=1)."""
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.kano_intents_time(self.ctx, byref(ms)), "kano_intents_time")
        return float(ms.value)

    def rows_timing(self, reset: bool = False) -> dict:
        """k_rows launch times (HIP events) since the last reset: sum, count,
        min, max (ms); waits for the context's work."""
        out = np.zeros(4, dtype=np.float64)
        self._chk(self.lib.kano_rows_timing(self.ctx, _ptr(out), int(bool(reset))),
                  "kano_rows_timing")
        return dict(sum_ms=float(out[0]), launches=int(out[1]), min_ms=float(out[2]),
                    max_ms=float(out[3]))

    def mfma_timing(self, reset: bool = False) -> dict:
        """k_heavy_mc_mfma per build since the last reset: sum ms, builds,
        algorithmic int8 ops (kano_mfma_timing)."""
        out = np.zeros(4, dtype=np.float64)
        self._chk(self.lib.kano_mfma_timing(self.ctx, _ptr(out), int(bool(reset))),
                  "kano_mfma_timing")
        return dict(sum_ms=float(out[0]), builds=int(out[1]), ops_sum=float(out[2]),
                    ops_last=float(out[3]))

    def set_pipeline(self, on: bool = True) -> None:
        """kano_set_pipeline: each asynchronously completing verify queues the
        next call's prologue behind a gate that the next verify opens (a loop
        of verify calls on the resident inputs).  Call ``settle()`` before a
        device-wide synchronisation outside the engine."""
        self._chk(self.lib.kano_set_pipeline(self.ctx, int(bool(on))), "kano_set_pipeline")

    def settle(self) -> None:
        """kano_settle: no engine work left pending on the device (a queued
        prologue run and put back, the last matrix write finished)."""
        self._chk(self.lib.kano_settle(self.ctx), "kano_settle")

    def gate_timing(self, reset: bool = False) -> dict:
        """kano_gate_timing: how long the pipelined calls' gates held the engine
        stream (its idle time at the step boundary), over the last min(64,
        gates since the last reset) gates; settles first."""
        import ctypes
        g, mean, mx = ctypes.c_int64(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        self._chk(self.lib.kano_gate_timing(self.ctx, int(bool(reset)), ctypes.byref(g),
                                            ctypes.byref(mean), ctypes.byref(mx)),
                  "kano_gate_timing")
        return dict(gates=int(g.value), mean_us=float(mean.value), max_us=float(mx.value))

    def host_times(self, reset: bool = False) -> dict:
        """kano_verify's host time by phase (us): sums and maxima since the
        last reset (kano_host_times)."""
        out = np.zeros(20, dtype=np.float64)
        self._chk(self.lib.kano_host_times(self.ctx, _ptr(out), int(bool(reset))),
                  "kano_host_times")
        k = ("calls", "front_sum", "back_sum", "wait_sum", "gap_sum", "front_max", "back_max",
             "wait_max", "call_max", "wait1_max", "wait2_max", "wait3_max", "back_launch_max",
             "back_emit_max", "back_tailwait_max", "back_copy_idx_max", "back_copy_pairs_max",
             "back_events_max", "tailwait_sum")
        return {name: float(v) for name, v in zip(k, out)}

    def stage_times(self) -> dict:
        ms = np.zeros(8, dtype=np.float32)
        self._chk(self.lib.kano_stage_times(self.ctx, _ptr(ms)), "kano_stage_times")
        return dict(classes=float(ms[0]), allow=float(ms[1]), select=float(ms[2]),
                    rows=float(ms[3]), shadow=float(ms[4]), build=float(ms[5]),
                    k_rows=float(ms[6]), impact=float(ms[7]))


def _as_pairs(pairs) -> Tuple[np.ndarray, int]:
    """Query pairs as a C-contiguous (Q, 2) int32 array (what diff_pairs
    returns, or a list of (i, j) tuples) and Q."""
    a = np.asarray(pairs)
    if a.size == 0:
        return np.zeros((0, 2), dtype=np.int32), 0
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("pairs must be a (Q, 2) array or a list of (i, j) tuples")
    if a.dtype != np.int32:
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError("pairs must hold integers")
        if a.min() < -2 ** 31 or a.max() >= 2 ** 31:
            raise IndexError("pair index out of range")
    return np.ascontiguousarray(a, dtype=np.int32), int(a.shape[0])


def _pair_call(call, b: DeviceBuild, what: str, Q: int, lists: bool, nids: Optional[int]) -> dict:
    """One pair_policies entry point: ``call(cover, off, hist, total)``, then
    the fetch of the id lists."""
    cover = np.zeros(Q, dtype=np.int32)
    off = np.zeros(Q + 1, dtype=np.int64) if lists else None
    hist = None if nids is None else np.zeros(nids, dtype=np.int64)
    total = c_int64(0)
    b._chk(call(_ptr(cover), _ptr(off), _ptr(hist), byref(total)), what)
    pol = None
    if lists:
        pol = np.zeros(int(total.value), dtype=np.int32)
        b._chk(b.lib.kano_pair_policies_fetch(b.ctx, _ptr(pol)), "kano_pair_policies_fetch")
    return dict(cover=cover, offsets=off, policies=pol, hist=hist)


def pairs_from_lists(n_lists: int, nbits: int, soff: np.ndarray, slist: np.ndarray,
                     allow_words: np.ndarray, pairs, device: int = 0, lists: bool = True,
                     hist: bool = False, mode: Optional[int] = None) -> dict:
    """pair_policies over explicit per-container policy lists and allow sets
    (kano_pair_policies_lists): for every pair (list c, bit x) the ascending
    ids of list c whose allow set holds x, as DeviceBuild.pair_policies
    returns them.  An id repeated within a list counts once.  ``mode`` passes
    a raw mode to the entry point."""
    lib = nat.load()
    b = DeviceBuild(None, device=device)
    try:
        aw = np.ascontiguousarray(allow_words, dtype=np.uint64)
        P = aw.shape[0]
        soff = np.ascontiguousarray(soff, dtype=np.int64)
        slist = np.ascontiguousarray(slist, dtype=np.int32)
        pr, Q = _as_pairs(pairs)
        if mode is None:
            mode = 0 if lists else 1
        return _pair_call(
            lambda *out: lib.kano_pair_policies_lists(b.ctx, int(n_lists), int(nbits), int(P),
                                                      _ptr(soff), _ptr(slist), _ptr(aw), Q,
                                                      _ptr(pr), int(mode), *out),
            b, "kano_pair_policies_lists", Q, mode == 0, P if hist else None)
    finally:
        b.close()


def shadow_from_lists(n_lists: int, nbits: int, soff: np.ndarray, slist: np.ndarray,
                      allow_words: np.ndarray, device: int = 0) -> np.ndarray:
    """policy_shadow over explicit per-container policy lists and allow sets
    (the general form of kano_py/kano/algorithm.py:58-80, used when the lists
    are not the ones a single build produced)."""
    lib = nat.load()
    b = DeviceBuild(None, device=device)
    P = allow_words.shape[0]
    soff = np.ascontiguousarray(soff, dtype=np.int64)
    slist = np.ascontiguousarray(slist, dtype=np.int32)
    aw = np.ascontiguousarray(allow_words, dtype=np.uint64)
    cnt = c_int64()
    b._chk(lib.kano_shadow_lists(b.ctx, int(n_lists), int(nbits), int(P), _ptr(soff),
                                 _ptr(slist), _ptr(aw), byref(cnt)), "kano_shadow_lists")
    out = np.zeros((int(cnt.value), 2), dtype=np.int32)
    b._chk(lib.kano_shadow_fetch(b.ctx, _ptr(out)), "kano_shadow_fetch")
    b.close()
    return out


def conflict_from_lists(n_lists: int, nbits: int, soff: np.ndarray, slist: np.ndarray,
                        allow_words: np.ndarray, device: int = 0,
                        count_only: bool = False):
    """The working policy_conflict over explicit per-container policy lists
    and allow sets (kano_conflict_lists): the (count, 2) pairs, or with
    ``count_only`` their number."""
    lib = nat.load()
    b = DeviceBuild(None, device=device)
    try:
        P = allow_words.shape[0]
        soff = np.ascontiguousarray(soff, dtype=np.int64)
        slist = np.ascontiguousarray(slist, dtype=np.int32)
        aw = np.ascontiguousarray(allow_words, dtype=np.uint64)
        cnt = c_int64()
        b._chk(lib.kano_conflict_lists(b.ctx, int(n_lists), int(nbits), int(P), _ptr(soff),
                                       _ptr(slist), _ptr(aw), 1 if count_only else 0,
                                       byref(cnt)), "kano_conflict_lists")
        if count_only:
            return int(cnt.value)
        out = np.zeros((int(cnt.value), 2), dtype=np.int32)
        b._chk(lib.kano_conflict_fetch(b.ctx, _ptr(out)), "kano_conflict_fetch")
        return out
    finally:
        b.close()


def impact_from_lists(n_lists: int, nbits: int, soff: np.ndarray, slist: np.ndarray,
                      allow_words: np.ndarray, device: int = 0, flags_only: bool = False,
                      mode: Optional[int] = None) -> np.ndarray:
    """policy_impact over explicit per-container policy lists and allow sets
    (kano_policy_impact_lists): impact[p] as int64 of length P, or with
    ``flags_only`` the essential flags (impact > 0) as bool.  The ids within
    one list must be distinct.  ``mode`` passes a raw mode to the entry point."""
    lib = nat.load()
    b = DeviceBuild(None, device=device)
    try:
        P = allow_words.shape[0]
        soff = np.ascontiguousarray(soff, dtype=np.int64)
        slist = np.ascontiguousarray(slist, dtype=np.int32)
        aw = np.ascontiguousarray(allow_words, dtype=np.uint64)
        if mode is None:
            mode = 1 if flags_only else 0
        impact = np.zeros(P, dtype=np.int64)
        ess = np.zeros(P, dtype=np.uint8)
        b._chk(lib.kano_policy_impact_lists(b.ctx, int(n_lists), int(nbits), int(P), _ptr(soff),
                                            _ptr(slist), _ptr(aw), int(mode), _ptr(impact),
                                            _ptr(ess), None), "kano_policy_impact_lists")
        return ess.astype(bool) if mode == 1 else impact
    finally:
        b.close()
