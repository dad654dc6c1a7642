"""The kept pod classification: a build after the first on one upload skips
the classification launches (kano_info's CLS_REUSED counts those builds) and
gives the same results; whatever changes the classification's inputs -- the
pod labels, a side's key columns, the row shard -- classifies again.

Expectations come from kano_py's golden records where one exists, else from
the CPU oracle on the changed policy or pod list; never from a GPU build."""
import copy

import numpy as np
import pytest

from _golden import (allow_lists_csr, cluster, container_lists_csr, csr_sha, expected,
                     row_digest, sha)

pytestmark = pytest.mark.gpu

NAMES = ["s_sparse_2000", "s_broad_300", "q_unknown_key", "q_missing_label"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from kano import _native
    if not _native.gpu_available():
        pytest.fail("GPU test run without a usable HIP device / libkano_hip.so")


def _tables(obj):
    from kano import model
    from kano._intern import intern
    from kano.synth import objects_from_json
    return intern(*objects_from_json(obj, model))


def _gid(obj):
    from oracle.kano_oracle import group_ids_json
    return group_ids_json(obj, obj.get("label", "app"))


def _from_record(name):
    e = expected(name)
    return {"M_sha": e["M_sha256"], "reach": e["all_reachable"], "iso": e["all_isolated"],
            "cross": e["user_crosscheck"]["result"], "sys": e["system_isolation"]["result"],
            "sh_count": e["policy_shadow"]["count"], "sh_sha": e["policy_shadow"]["sha256"],
            "sel_sha": e["select_policies_sha256"], "alw_sha": e["allow_policies_sha256"]}


_ORACLE = {}


def _from_oracle(obj, key):
    """The CPU oracle's results on obj, computed once per key."""
    if key not in _ORACLE:
        from oracle import kano_oracle as orc
        r = orc.run_c(obj, label=obj.get("label", "app"))
        _ORACLE[key] = {
            "M": r["M"], "M_sha": sha(r["M"]), "reach": r["all_reachable"],
            "iso": r["all_isolated"], "cross": r["user_crosscheck"],
            "sys": r["system_isolation"], "sh_count": r["shadow_count"],
            "sh_sha": sha(np.ascontiguousarray(r["shadow"], dtype=np.int32)),
            "sel_sha": csr_sha(r["select_off"], r["select_list"]),
            "alw_sha": csr_sha(r["allow_off"], r["allow_list"])}
    return _ORACLE[key]


def _check_verify(r, E):
    assert r["all_reachable"].tolist() == E["reach"]
    assert r["all_isolated"].tolist() == E["iso"]
    assert r["user_crosscheck"].tolist() == E["cross"]
    assert r["system_isolation"].tolist() == E["sys"]
    assert r["shadow_count"] == E["sh_count"]
    assert sha(np.ascontiguousarray(r["pairs"], dtype=np.int32).reshape(-1, 2)) == E["sh_sha"]


def _check_state(eng, E):
    """The matrix and the per-pod lists (these reads settle a queued prologue)."""
    n = eng.n
    assert sha(eng.rows(0, n)) == E["M_sha"]
    cls = eng.classes()
    assert csr_sha(*container_lists_csr(cls, *eng.select_csr())) == E["sel_sha"]
    assert csr_sha(*allow_lists_csr(n, *eng.allow_csr())) == E["alw_sha"]


def _reused(eng):
    return eng.info()["CLS_REUSED"]


def _subset(t, keep):
    """Tables with the policies keep[0], keep[1], ... of t over t's pods."""
    def rows(off, *arrs):
        off = np.asarray(off, np.int64)
        idx = np.concatenate([np.arange(off[k], off[k + 1]) for k in keep] or
                             [np.zeros(0, np.int64)]).astype(np.int64)
        new = np.zeros(len(keep) + 1, np.int64)
        new[1:] = np.cumsum([off[k + 1] - off[k] for k in keep])
        return (new,) + tuple(np.asarray(a)[idx] for a in arrs)
    t2 = copy.copy(t)
    t2.sel_off, t2.sel_col, t2.sel_val = rows(t.sel_off, t.sel_col, t.sel_val)
    t2.alw_off, t2.alw_col, t2.alw_val = rows(t.alw_off, t.alw_col, t.alw_val)
    return t2


def _with_policies(obj, keep):
    o = dict(obj)
    o["policies"] = [obj["policies"][k] for k in keep]
    return o


def _edit_keep(t):
    """A reordered subset of the policies that still names every key column
    of both sides (asserted)."""
    P = len(t.sel_off) - 1
    keep = [k for k in reversed(range(P)) if k % 3 != 1]
    t2 = _subset(t, keep)
    assert set(t2.sel_col.tolist()) == set(np.asarray(t.sel_col).tolist())
    assert set(t2.alw_col.tolist()) == set(np.asarray(t.alw_col).tolist())
    assert 0 < len(keep) < P
    return keep, t2


def _working_selector(q):
    return q["allow"] if q["direction"] == "ingress" else q["select"]


def _drop_select_key(obj, t):
    """Every working-selector term on one key dropped: the JSON for the oracle
    and the same edit on the interned tables (the key's column is the one
    whose value ids partition the pods as the labels do)."""
    known = {k for p in obj["pods"] for k in p["labels"]}
    used = {}
    for q in obj["policies"]:
        for k in _working_selector(q):
            if k in known:
                used[k] = used.get(k, 0) + 1
    key = sorted(used, key=lambda k: (used[k], k))[0]
    o = copy.deepcopy(obj)
    for q in o["policies"]:
        _working_selector(q).pop(key, None)
    lab = [p["labels"].get(key) for p in obj["pods"]]
    ids = {v: i for i, v in enumerate(dict.fromkeys(lab))}
    part = np.array([ids[v] for v in lab])
    cols = []
    for c in sorted(set(np.asarray(t.sel_col).tolist())):
        pairs = set(zip(np.asarray(t.pod_val)[c].tolist(), part.tolist()))
        if len(pairs) == len(ids) == len(set(np.asarray(t.pod_val)[c].tolist())):
            cols.append(c)
    assert len(cols) == 1, (key, cols)
    off = np.asarray(t.sel_off, np.int64)
    live = np.asarray(t.sel_col) != cols[0]
    t2 = copy.copy(t)
    t2.sel_off = np.concatenate([[0], np.cumsum(live)])[off]
    t2.sel_col = np.asarray(t.sel_col)[live]
    t2.sel_val = np.asarray(t.sel_val)[live]
    assert cols[0] not in set(t2.sel_col.tolist()) and len(t2.sel_col) < len(t.sel_col)
    return o, t2


def _permuted(obj):
    o = dict(obj)
    n = len(obj["pods"])
    perm = np.random.default_rng(5).permutation(n)
    o["pods"] = [obj["pods"][int(i)] for i in perm]
    return o


@pytest.mark.parametrize("mode", ["plain", "pipelined", "build_between"])
@pytest.mark.parametrize("name", NAMES)
def test_reuse_happens_and_is_right(name, mode):
    """Three verifies on one context: the counter reads 0, 1, 2 and every call
    equals kano_py's record."""
    from kano._engine import DeviceBuild
    obj, E = cluster(name), _from_record(name)
    eng = DeviceBuild(_tables(obj), build=False)
    if mode == "pipelined":
        eng.set_pipeline(True)
    gid = _gid(obj)
    want = 0
    for k in range(3):
        _check_verify(eng.verify(gid, sys_row=0, shadow=True), E)
        assert _reused(eng) == want
        want += 1
        if mode == "build_between" and k == 0:
            eng.build()
            assert _reused(eng) == want
            want += 1
            _check_state(eng, E)
    _check_state(eng, E)
    eng.close()


@pytest.mark.parametrize("name", ["s_sparse_2000", "s_broad_300"])
def test_policy_edit_same_keys(name):
    from kano._engine import DeviceBuild
    obj = cluster(name)
    t = _tables(obj)
    keep, t2 = _edit_keep(t)
    E2 = _from_oracle(_with_policies(obj, keep), (name, "edit"))
    eng = DeviceBuild(t, build=False)
    gid = _gid(obj)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), _from_record(name))
    eng.set_policies(t2)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E2)
    assert _reused(eng) == 1
    _check_state(eng, E2)
    eng.close()


@pytest.mark.parametrize("name", ["s_sparse_2000", "s_broad_300"])
def test_key_set_changes(name):
    from kano._engine import DeviceBuild
    obj, E = cluster(name), _from_record(name)
    t = _tables(obj)
    obj3, t3 = _drop_select_key(obj, t)
    E3 = _from_oracle(obj3, (name, "dropkey"))
    eng = DeviceBuild(t, build=False)
    gid = _gid(obj)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E)
    assert _reused(eng) == 1
    eng.set_policies(t3)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E3)
    assert _reused(eng) == 1            # classified again
    _check_state(eng, E3)
    eng.set_policies(t)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E)
    assert _reused(eng) == 1            # and again on the full key set
    _check_state(eng, E)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E)
    assert _reused(eng) == 2
    eng.close()


@pytest.mark.parametrize("name", ["s_sparse_2000", "s_broad_300", "q_missing_label"])
def test_same_shapes_different_pods(name):
    """A re-upload with the pod rows permuted: n and ncols as before, other
    labels per row -- stale classes would go unnoticed by every size check."""
    from kano._engine import DeviceBuild
    obj, E = cluster(name), _from_record(name)
    obj4 = _permuted(obj)
    E4 = _from_oracle(obj4, (name, "perm"))
    t, t4 = _tables(obj), _tables(obj4)
    assert (t.n, t.ncols) == (t4.n, t4.ncols)
    assert not np.array_equal(t.pod_val, t4.pod_val)
    eng = DeviceBuild(t, build=False)
    _check_verify(eng.verify(_gid(obj), sys_row=0, shadow=True), E)
    _check_verify(eng.verify(_gid(obj), sys_row=0, shadow=True), E)
    assert _reused(eng) == 1
    eng.upload(t4)
    _check_verify(eng.verify(_gid(obj4), sys_row=0, shadow=True), E4)
    assert _reused(eng) == 1
    _check_state(eng, E4)
    _check_verify(eng.verify(_gid(obj4), sys_row=0, shadow=True), E4)
    assert _reused(eng) == 2
    eng.close()


@pytest.mark.parametrize("name", ["s_sparse_2000", "s_broad_300"])
def test_shards(name):
    from kano._engine import DeviceBuild
    obj = cluster(name)
    Eo = _from_oracle(obj, (name, "full"))
    assert Eo["M_sha"] == expected(name)["M_sha256"]
    dig = row_digest(Eo["M"])
    eng = DeviceBuild(_tables(obj), build=False)
    n = eng.n
    want = 0
    for r0, r1 in ((0, n // 2), (n // 2, n), (0, n)):
        eng.set_rows(r0, r1)
        for k in range(2):
            eng.verify(None, sys_row=0, shadow=True, shadow_count_only=True)
            want += k
            assert _reused(eng) == want
            assert np.array_equal(eng.rows_digest(r0, r1 - r0), dig[r0:r1])
    eng.close()


@pytest.mark.parametrize("name", ["s_sparse_2000", "s_broad_300"])
def test_behind_a_queued_prologue(name):
    """Pipelined calls: the inputs change while the next call's prologue is
    queued behind its gate."""
    from kano._engine import DeviceBuild
    obj, E = cluster(name), _from_record(name)
    t = _tables(obj)
    keep, t2 = _edit_keep(t)
    E2 = _from_oracle(_with_policies(obj, keep), (name, "edit"))
    obj4 = _permuted(obj)
    E4 = _from_oracle(obj4, (name, "perm"))
    eng = DeviceBuild(t, build=False)
    eng.set_pipeline(True)
    gid = _gid(obj)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E)
    eng.set_policies(t2)
    for k in range(3):
        _check_verify(eng.verify(gid, sys_row=0, shadow=True), E2)
        assert _reused(eng) == k + 1
    _check_state(eng, E2)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E2)
    eng.upload(_tables(obj4))
    for k in range(3):
        _check_verify(eng.verify(_gid(obj4), sys_row=0, shadow=True), E4)
        assert _reused(eng) == 4 + k
    _check_state(eng, E4)
    _check_verify(eng.verify(_gid(obj4), sys_row=0, shadow=True), E4)
    eng.close()                         # with a prologue queued


def test_extra_pod_column():
    """add_policies with a policy on a key no build policy names, then a
    verify: rebuilt from the tables, classified again, equal to the record."""
    from kano import model
    from kano.model import ReachabilityMatrix
    from kano.synth import objects_from_json
    name = "s_sparse_2000"
    obj, E = cluster(name), _from_record(name)
    cs, ps = objects_from_json(obj, model)
    m = ReachabilityMatrix.build_matrix(cs, ps)
    eng = m.engine
    gid = _gid(obj)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E)
    base = _reused(eng)
    used = {k for p in ps for k in list(p.selector.labels) + list(p.allow.labels)}
    fresh = [k for k in dict.fromkeys(k for c in cs for k in c.labels) if k not in used]
    assert fresh
    v0 = next(c.labels[fresh[0]] for c in cs if fresh[0] in c.labels)
    extra = model.Policy("x_newkey", model.PolicySelect({fresh[0]: v0}), model.PolicyAllow({}),
                         model.PolicyEgress, model.PolicyProtocol(["TCP"]))
    m.add_policies([extra])
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E)
    assert _reused(eng) == base
    _check_state(eng, E)
    _check_verify(eng.verify(gid, sys_row=0, shadow=True), E)
    assert _reused(eng) == base + 1
    eng.close()
