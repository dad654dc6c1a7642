"""Both forms of the policy -> class matching (csrc/kano_hip.hip prepare_side /
match_both): the hash join of a side whose policies use at most 64 distinct
slot sets, and the dense evaluation (match_dense: k_class_eval, k_popc_rows,
the scan, k_bits_to_lists) past that.  Everything downstream reads the class
lists either form leaves behind, so every case asserts the form it means to
take (kano_info's MATCH_FORM: bit 0 the select side is dense, bit 1 the allow
side) and compares with the C oracle on inputs whose matrices are neither
empty nor full.

The generator: 8 keys k0..k7, each pod carries each with probability 0.8 and
a value of v0..v2, plus tenant = t(i % 5).  The slot sets are the 92 key
subsets of size 1..3 in itertools.combinations order; policy p's working
select side uses subset p % ns_sel, its working allow side subset p % ns_alw
(the sides are swapped afterwards for the ingress policies, every third one).
Values: with probability 0.7 a random pod's own (v0..v3 where it lacks the
key), else random ones of v0..v3; no pod has v3.  ``full`` appends a policy
naming all eight keys on both sides with pod 0's values: on a packed side of
the join that is the single-class lookup (pmask -3).

Exact bits and integers throughout.
"""
import functools
import itertools
import random

import numpy as np
import pytest

from _golden import allow_lists_csr, container_lists_csr, lists_to_csr
import test_conflict as tc
import test_explain as te
import test_ports as tp
import test_redundancy as tr
import test_verdicts as tv

KEYS = [f"k{i}" for i in range(8)]
SUBSETS = [c for r in (1, 2, 3) for c in itertools.combinations(range(8), r)]
MAX_MASKS = 64       # csrc/kano_hip.hip: more distinct slot sets than this go dense


def generate(n, P, ns_sel, ns_alw, seed, full=False):
    """The cluster as the JSON object oracle.run_c reads."""
    rnd = random.Random(seed)
    pods = []
    for i in range(n):
        lab = {k: f"v{rnd.randrange(3)}" for k in KEYS if rnd.random() < 0.8}
        lab["tenant"] = f"t{i % 5}"
        pods.append({"name": f"c{i}", "labels": lab})

    def side(sub):
        if rnd.random() < 0.7:
            own = pods[rnd.randrange(n)]["labels"]
            return {KEYS[k]: own.get(KEYS[k], f"v{rnd.randrange(4)}") for k in sub}
        return {KEYS[k]: f"v{rnd.randrange(4)}" for k in sub}

    pols = []
    for p in range(P):
        ws, wa = side(SUBSETS[p % ns_sel]), side(SUBSETS[p % ns_alw])
        ing = p % 3 == 2
        pols.append({"name": f"q{p}", "select": wa if ing else ws, "allow": ws if ing else wa,
                     "direction": "ingress" if ing else "egress", "protocol": ["TCP", "80"]})
    if full:
        own = pods[0]["labels"]
        assert all(k in own for k in KEYS), "pod 0 lacks a key: choose another seed"
        pols.append({"name": "full", "select": {k: own[k] for k in KEYS},
                     "allow": {k: own[k] for k in KEYS}, "direction": "egress",
                     "protocol": ["TCP", "80"]})
    return {"label": "tenant", "pods": pods, "policies": pols}


def slot_sets(obj):
    """Distinct key sets of the non-empty working select / working allow sides."""
    out = [set(), set()]
    for q in obj["policies"]:
        ws, wa = (q["allow"], q["select"]) if q["direction"] == "ingress" else \
            (q["select"], q["allow"])
        for which, d in enumerate((ws, wa)):
            if d:
                out[which].add(frozenset(d))
    return len(out[0]), len(out[1])


def form_of(counts):
    return (1 if counts[0] > MAX_MASKS else 0) | (2 if counts[1] > MAX_MASKS else 0)


# name: (n, P before the full policy, ns_sel, ns_alw, full, seed, slot sets, MATCH_FORM)
CASES = {
    "join-64": (130, 128, 63, 63, True, 28, (64, 64), 0),
    "dense-65": (130, 130, 64, 64, True, 28, (65, 65), 3),     # (join-64's pods: one seed)
    "dense-select": (130, 130, 65, 3, False, 1, (65, 3), 1),
    "dense-allow": (130, 130, 3, 65, False, 5, (3, 65), 2),
    "dense-600": (600, 200, 92, 92, True, 28, (93, 93), 3),
    "dense-wide": (65, 193, 92, 92, False, 1, (92, 92), 3),
}
NAMES = sorted(CASES)
DENSE_130 = ("dense-65", "dense-select", "dense-allow")


def unpack(words, n):
    return tr._unpack(words, n).astype(bool)


def to_words(bits):
    bits = np.asarray(bits, dtype=bool).reshape(len(bits), -1)
    n = bits.shape[1]
    buf = np.zeros((bits.shape[0], ((n + 63) // 64) * 64), np.uint8)
    buf[:, :n] = bits
    return np.packbits(buf, axis=1, bitorder="little").view("<u8").astype(np.uint64)


def system_isolation(ref, row):
    return np.flatnonzero(~unpack(ref["M"][row:row + 1], ref["n"])[0]).tolist()


def ones(ref):
    return int(unpack(ref["M"], ref["n"]).sum())


@functools.lru_cache(maxsize=None)
def case(name):
    """(JSON object, the C oracle's record) of a case; shared, read only."""
    from oracle import kano_oracle as orc
    n, P, ns_sel, ns_alw, full, seed, _, _ = CASES[name]
    obj = generate(n, P, ns_sel, ns_alw, seed, full)
    return obj, orc.run_c(obj, label="tenant")


def objects(obj):
    from kano import model
    from kano.synth import objects_from_json
    return objects_from_json(obj, model)


def tables(obj):
    from kano._intern import intern
    return intern(*objects(obj))


def group_of(n):
    return (np.arange(n) % 5).astype(np.int32)       # tenant = t(i % 5)


def assert_says_something(ref, rows):
    """The conditions of a case, from the reference alone."""
    n = ref["n"]
    assert 0 < ones(ref) < n * n
    assert ref["user_crosscheck"] and ref["shadow_count"] > 0 and len(ref["shadow"])
    for row in rows:
        assert system_isolation(ref, row)


# --------------------------------------------------------------------------
# the restatement over the integer tables (what the C ABI is given)
# --------------------------------------------------------------------------
def table_sets(t):
    """(sel, allow) bool (P, n): every term (col, v) holds, literally."""
    pv = np.asarray(t.pod_val)

    def side(off, col, val):
        out = np.ones((t.P, t.n), bool)
        for p in range(t.P):
            for k in range(int(off[p]), int(off[p + 1])):
                out[p] &= pv[col[k]] == val[k]
        return out
    return side(t.sel_off, t.sel_col, t.sel_val), side(t.alw_off, t.alw_col, t.alw_val)


def table_reference(t, gid):
    """The record oracle.run_c gives, from the tables alone."""
    sel, alw = table_sets(t)
    n = t.n
    M = (sel.T.astype(np.int64) @ alw.astype(np.int64)) > 0
    lists = [np.flatnonzero(sel[:, i]) for i in range(n)]
    # sub[k, j]: allow_k is a subset of allow_j
    sub = (alw.astype(np.int64) @ (~alw).astype(np.int64).T) == 0
    pairs = []
    for S in lists:
        jj, kk = np.repeat(S, S.size), np.tile(S, S.size)
        keep = (jj != kk) & sub[kk, jj]
        pairs.append(np.stack([jj[keep], kk[keep]], axis=1))
    pairs = np.concatenate(pairs).astype(np.int32).reshape(-1, 2)
    so, sl = lists_to_csr([S.tolist() for S in lists])
    ao, al = lists_to_csr([np.flatnonzero(alw[:, i]).tolist() for i in range(n)])
    g = np.asarray(gid)
    return dict(n=n, P=t.P, M=to_words(M), sel=to_words(sel), allow=to_words(alw),
                select_off=so, select_list=sl, allow_off=ao, allow_list=al,
                all_reachable=np.flatnonzero(M.all(axis=0)).tolist(),
                all_isolated=np.flatnonzero(~M.any(axis=0)).tolist(),
                user_crosscheck=np.flatnonzero(
                    (M & (g[:, None] != g[None, :])).any(axis=0)).tolist(),
                shadow=pairs, shadow_count=int(pairs.shape[0]),
                conflict_raises=bool(max(len(S) for S in lists) >= 2))


def table_slot_sets(t):
    """prepare_side's masks: the distinct column sets of the policies that are
    neither empty nor contradictory, per side."""
    def side(off, col, val):
        masks = set()
        for p in range(t.P):
            terms = sorted(set(zip(col[off[p]:off[p + 1]].tolist(),
                                   val[off[p]:off[p + 1]].tolist())))
            cols = [c for c, _ in terms]
            if cols and len(cols) == len(set(cols)):
                masks.add(tuple(cols))
        return len(masks)
    return side(t.sel_off, t.sel_col, t.sel_val), side(t.alw_off, t.alw_col, t.alw_val)


# the appended policies: (name, select terms, allow terms) over the names below
EXTRA = [("single-select", "one", "nar"), ("repeat-select", "rep", "nar"),
         ("contra-select", "con", "nar"),
         ("single-allow", "nar", "one"), ("repeat-allow", "nar", "rep"),
         ("contra-allow", "nar", "con"),
         ("single-both", "one", "one"), ("repeat-both", "rep", "rep"),
         ("contra-both", "con", "con"),
         ("no-match-rule", "nomatch", "nar"), ("never-match", "nar", "never"),
         ("empty-select", "none", "nar"), ("empty-allow", "nar", "none")]
SAME_AS = {"repeat-select": "single-select", "repeat-allow": "single-allow",
           "repeat-both": "single-both"}
EMPTY = {"contra-select": (True, False), "contra-allow": (False, True),
         "contra-both": (True, True), "no-match-rule": (True, False),
         "never-match": (False, True)}


def extended(t):
    """(tables with EXTRA appended, index of the first appended policy)."""
    from kano._intern import NEVER_MATCH_VALUE, NO_MATCH_RULE, Tables
    pv = np.asarray(t.pod_val)
    # (the narrow term selects neither system row: "empty-allow" would fill it)
    i0 = next(i for i in range(t.n) if pv[0, i] >= 0 and pv[1, i] >= 0 and
              pv[1, i] not in (pv[1, 0], pv[1, t.n - 1]))
    v = int(pv[0, i0])
    v2 = int(next(x for x in np.unique(pv[0]) if x >= 0 and x != v))
    terms = {"one": [(0, v)], "rep": [(0, v), (0, v)], "con": [(0, v), (0, v2)],
             "nar": [(1, int(pv[1, i0]))], "nomatch": [(0, NO_MATCH_RULE)],
             "never": [(0, NEVER_MATCH_VALUE)], "none": []}

    def grow(off, col, val, which):
        add = [terms[x[which]] for x in EXTRA]
        o = np.concatenate([off, off[-1] + np.cumsum([len(a) for a in add])]).astype(np.int64)
        c = np.concatenate([col, [c for a in add for c, _ in a]]).astype(np.int32)
        w = np.concatenate([val, [w for a in add for _, w in a]]).astype(np.int32)
        return o, c, w
    return Tables(t.n, t.ncols, t.pod_val, *grow(t.sel_off, t.sel_col, t.sel_val, 1),
                  *grow(t.alw_off, t.alw_col, t.alw_val, 2)), t.P


# --------------------------------------------------------------------------
# CPU: the generator's conditions and the restatement
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_cases_say_something(name):
    n, P, _, _, full, _, sets, form = CASES[name]
    obj, ref = case(name)
    assert (ref["n"], ref["P"]) == (n, P + full)
    assert slot_sets(obj) == sets and form_of(sets) == form
    assert_says_something(ref, (0, n - 1))
    assert table_slot_sets(tables(obj)) == sets


def test_some_case_isolates_and_some_case_reaches():
    assert any(case(k)[1]["all_isolated"] for k in NAMES)
    assert any(case(k)[1]["all_reachable"] for k in NAMES)


def class_counts(obj):
    """(row classes, column classes): the pods' distinct value tuples on the
    keys the working select / working allow sides name."""
    out = []
    for which in (0, 1):
        keys = sorted({k for q in obj["policies"]
                       for k in ((q["allow"], q["select"]) if q["direction"] == "ingress"
                                 else (q["select"], q["allow"]))[which]})
        out.append(len({tuple(p["labels"].get(k) for k in keys) for p in obj["pods"]}))
    return tuple(out)


def test_class_counts_of_the_cases():
    """dense-600: three 256-class blocks of k_class_eval, the last not full;
    the 130-pod cases: an odd count of 64-class words on the dense side;
    dense-wide: 65 classes, one bit into a second word."""
    U, UA = class_counts(case("dense-600")[0])
    assert 512 < U <= 600 and U % 256 and 512 < UA <= 600 and UA % 256
    for name, which in (("dense-65", 0), ("dense-65", 1), ("dense-select", 0),
                        ("dense-allow", 1)):
        assert (class_counts(case(name)[0])[which] + 63) // 64 == 3
    assert class_counts(case("dense-wide")[0]) == (65, 65)
    assert case("join-64")[0]["pods"] == case("dense-65")[0]["pods"]
    tj, td = tables(case("join-64")[0]), tables(case("dense-65")[0])
    assert np.array_equal(tj.pod_val, td.pod_val)


@pytest.mark.parametrize("name", ["join-64", "dense-65"])
def test_table_restatement_equals_oracle(name):
    obj, ref = case(name)
    got = table_reference(tables(obj), group_of(ref["n"]))
    for k in ("M", "sel", "allow", "select_off", "select_list", "allow_off", "allow_list",
              "shadow"):
        assert np.array_equal(got[k], ref[k]), k
    for k in ("all_reachable", "all_isolated", "user_crosscheck", "shadow_count",
              "conflict_raises"):
        assert got[k] == ref[k], k


@pytest.mark.parametrize("name", ["join-64", "dense-65"])
def test_extended_tables(name):
    """The appended policies keep the form, and the restatement gives them the
    sets their construction says."""
    t, P0 = extended(tables(case(name)[0]))
    assert form_of(table_slot_sets(t)) == CASES[name][7]
    sel, alw = table_sets(t)
    at = {x[0]: P0 + k for k, x in enumerate(EXTRA)}
    for a, b in SAME_AS.items():
        assert np.array_equal(sel[at[a]], sel[at[b]]) and np.array_equal(alw[at[a]], alw[at[b]])
        assert sel[at[a]].any() and alw[at[a]].any()
    for a, (s, w) in EMPTY.items():
        assert sel[at[a]].any() != s and alw[at[a]].any() != w
    assert sel[at["empty-select"]].all() and alw[at["empty-allow"]].all()
    assert not alw[at["empty-select"]].all() and not sel[at["empty-allow"]].all()
    ref = table_reference(t, group_of(t.n))
    assert_says_something(ref, (0, t.n - 1))


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def need_gpu():
    from kano import _native
    if not _native.gpu_available():
        pytest.fail("GPU test run without a usable HIP device / libkano_hip.so")


gpu = pytest.mark.gpu


def check_verify(r, ref, sys_row, count_only=False):
    assert r["all_reachable"].tolist() == ref["all_reachable"]
    assert r["all_isolated"].tolist() == ref["all_isolated"]
    assert r["user_crosscheck"].tolist() == ref["user_crosscheck"]
    if sys_row is not None:
        assert r["system_isolation"].tolist() == system_isolation(ref, sys_row)
    assert r["shadow_count"] == ref["shadow_count"]
    if count_only:
        assert r["pairs"] is None
    else:
        assert np.array_equal(np.asarray(r["pairs"]).reshape(-1, 2), ref["shadow"].reshape(-1, 2))


def check_state(eng, ref, policies=None):
    """The matrix, both lists and the policies' sets of a built context."""
    n = ref["n"]
    assert np.array_equal(eng.rows(0, n), ref["M"])
    so, sl = container_lists_csr(eng.classes(), *eng.select_csr())
    assert np.array_equal(so, ref["select_off"]) and np.array_equal(sl, ref["select_list"])
    ao, al = allow_lists_csr(n, *eng.allow_csr())
    assert np.array_equal(ao, ref["allow_off"]) and np.array_equal(al, ref["allow_list"])
    for p in (range(ref["P"]) if policies is None else policies):
        s, a = eng.policy_sets(p)
        assert np.array_equal(s, ref["sel"][p]) and np.array_equal(a, ref["allow"][p]), p
    assert eng.conflict_raises() == ref["conflict_raises"]


@gpu
@pytest.mark.parametrize("tune", ["", "packed=0"])
@pytest.mark.parametrize("name", NAMES)
def test_forms_vs_oracle(name, tune, monkeypatch, need_gpu):
    from kano._engine import DeviceBuild
    monkeypatch.setenv("KANO_TUNE", tune)
    obj, ref = case(name)
    n = ref["n"]
    gid = group_of(n)
    eng = DeviceBuild(tables(obj), build=False)
    assert eng.info()["MATCH_FORM"] == CASES[name][7]
    for sys_row in (0, n - 1):
        check_verify(eng.verify(gid, sys_row=sys_row, shadow=True), ref, sys_row)
        assert eng.info()["MATCH_FORM"] == CASES[name][7]
        check_state(eng, ref)
        check_verify(eng.verify(gid, sys_row=sys_row, shadow=True, shadow_count_only=True), ref,
                     sys_row, count_only=True)
    info = eng.info()
    assert (info["U"], info["UA"]) == class_counts(obj)
    eng.close()


@gpu
@pytest.mark.parametrize("path", ["bitwise", "mfma"])
@pytest.mark.parametrize("name", DENSE_130)
def test_dense_forms_on_both_paths(name, path, need_gpu):
    from kano._engine import DeviceBuild
    obj, ref = case(name)
    eng = DeviceBuild(tables(obj), path=path)
    assert eng.info()["MATCH_FORM"] == CASES[name][7]
    assert np.array_equal(eng.rows(0, ref["n"]), ref["M"])
    eng.close()


@gpu
def test_dense_form_on_row_shards(need_gpu):
    """Row shards of dense-600, two of them empty or one row: the shards' rows
    concatenate to the oracle's matrix, their column words (kano_checks_shard)
    combine to its lists."""
    import torch
    from kano._engine import DeviceBuild
    obj, ref = case("dense-600")
    n = ref["n"]
    W = (n + 63) // 64
    t = tables(obj)
    gid = group_of(n)
    spans = [(0, 0), (0, 1), (1, 300), (300, 600)]
    gathered = torch.zeros(len(spans) * 3 * W, dtype=torch.int64, device="cuda")
    engs, rows = [], []
    for k, (r0, r1) in enumerate(spans):
        e = DeviceBuild(t, rows=(r0, r1))
        assert e.info()["MATCH_FORM"] == 3
        rows.append(e.rows(r0, r1 - r0))
        e.checks_shard(gathered.data_ptr() + 8 * 3 * W * k, gid=gid, sys_row=0)
        engs.append(e)
    assert np.array_equal(np.concatenate(rows), ref["M"])
    torch.cuda.synchronize()
    for (r0, r1), e in zip(spans, engs):
        r = e.verify_combine(gathered.data_ptr(), len(spans))
        assert r["all_reachable"].tolist() == ref["all_reachable"]
        assert r["all_isolated"].tolist() == ref["all_isolated"]
        assert r["user_crosscheck"].tolist() == ref["user_crosscheck"]
        if r0 <= 0 < r1:
            assert r["system_isolation"].tolist() == system_isolation(ref, 0)
        else:
            assert r["system_isolation"] is None
        e.close()


@gpu
@pytest.mark.parametrize("tune", ["", "packed=0"])
@pytest.mark.parametrize("name", ["join-64", "dense-65"])
def test_terms_only_the_c_abi_can_express(name, tune, monkeypatch, need_gpu):
    """A key named twice on one side (equal values: the single term; different
    values: nothing, in the dense form through the sentinel term), rule values
    no pod carries and empty sides, appended to the case's tables."""
    from kano._engine import DeviceBuild
    monkeypatch.setenv("KANO_TUNE", tune)
    base = tables(case(name)[0])
    t, P0 = extended(base)
    gid = group_of(t.n)
    ref = table_reference(t, gid)
    eng = DeviceBuild(t, build=False)
    assert eng.info()["MATCH_FORM"] == CASES[name][7]
    for sys_row in (0, t.n - 1):
        check_verify(eng.verify(gid, sys_row=sys_row, shadow=True), ref, sys_row)
    check_state(eng, ref)                     # every policy's sets, the appended ones too
    at = {x[0]: P0 + k for k, x in enumerate(EXTRA)}
    zero = np.zeros((t.n + 63) // 64, np.uint64)
    for a, (s, w) in EMPTY.items():
        got = eng.policy_sets(at[a])
        assert np.array_equal(got[0], zero) == s and np.array_equal(got[1], zero) == w, a
    for a, b in SAME_AS.items():
        assert all(np.array_equal(x, y) for x, y in zip(eng.policy_sets(at[a]),
                                                        eng.policy_sets(at[b]))), a
    # the neighbours of the contradictory policies, and the build's own
    # policies, keep the sets the unextended tables give them
    sel, alw = table_sets(base)
    for p in range(P0):
        s, a = eng.policy_sets(p)
        assert np.array_equal(s, to_words(sel[p:p + 1])[0]), p
        assert np.array_equal(a, to_words(alw[p:p + 1])[0]), p
    eng.close()


# ---- what reads the class lists, on a densely matched build --------------
QUERY = np.array([(i, j) for i in (0, 1, 63, 64, 65, 129) for j in range(130)], np.int32)


def dense_matrix(dress=lambda ps: None):
    """(matrix, containers, policies, oracle record, sel, allow) of dense-65
    through the drop-in API, MATCH_FORM 3 asserted."""
    from kano.model import ReachabilityMatrix
    obj, ref = case("dense-65")
    cs, ps = objects(obj)
    dress(ps)
    m = ReachabilityMatrix.build_matrix(cs, ps)
    assert m.engine.info()["MATCH_FORM"] == 3
    n = ref["n"]
    assert np.array_equal(m.engine.rows(0, n), ref["M"])
    return m, cs, ps, ref, unpack(ref["sel"], n), unpack(ref["allow"], n)


@gpu
@pytest.mark.parametrize("form", ["ppf=1", "ppf=2"])
def test_dense_pair_policies(form, monkeypatch, need_gpu):
    monkeypatch.setenv("KANO_TUNE", form)
    m, cs, ps, ref, sel, allow = dense_matrix()
    n = ref["n"]
    want = te.want_pairs(ref["select_off"], ref["select_list"], ref["allow"], n, QUERY)
    assert want[0].max() > 1 and (want[0] == 0).any()
    assert te.same(te._check_against_sets(m, ps, n, QUERY), want)
    m.engine.close()


@gpu
def test_dense_impact_and_conflicts(need_gpu):
    from kano import algorithm as alg
    m, cs, ps, ref, sel, allow = dense_matrix()
    n = ref["n"]
    impact = tr.want_impact(ref["select_off"], ref["select_list"], ref["allow"], n)
    assert impact.any() and (impact == 0).any()
    assert alg.policy_impact(m, ps, cs).tolist() == impact.tolist()
    assert alg.policy_redundant(m, ps, cs) == np.flatnonzero(impact == 0).tolist()
    want = tc.want_pairs(ref["select_off"], ref["select_list"], ref["allow"], n)
    assert 0 < want.shape[0]
    assert alg._fast_path(m, ps, cs)
    assert np.array_equal(alg.policy_conflict_pairs(m, ps, cs), want)
    # the containers in the other order: their lists, explicitly
    back = cs[::-1]
    assert not alg._fast_path(m, ps, back)
    lists = [ref["select_list"][ref["select_off"][i]:ref["select_off"][i + 1]].tolist()
             for i in range(n)][::-1]
    want = tc.want_pairs(*lists_to_csr(lists), ref["allow"], n)
    assert np.array_equal(alg.policy_conflict_pairs(m, ps, back), want)
    m.engine.close()


@gpu
def test_dense_verdicts_and_ports(need_gpu):
    from kano.ports import port_table
    P = case("dense-65")[1]["P"]
    deny, prio = tv.tier_rule(P, 3)

    def dress(ps):
        tv.carry(ps, deny, prio)
        for p, pol in enumerate(ps):
            pol.protocol = tp.protocol_for(p, 5)
    m, cs, ps, ref, sel, allow = dense_matrix(dress)
    _, _, (verdict, _, _) = tv.check_verdicts(m, sel, allow, deny, prio, QUERY)
    assert set(verdict.tolist()) == {0, 1, 2}
    t = port_table(ps)
    masks, pops = tp.check_ports(m, sel, allow, t, QUERY, slots=(1,), exposure=False)
    assert 0 < pops[0] < ones(ref) and masks.any()
    m.engine.close()


@gpu
def test_dense_remove_then_add(need_gpu):
    """remove_policies (the full policy among them: the lists left use 64 slot
    sets), then add_policies of two of them (65 again), each step against the
    oracle over the updated list."""
    import test_incremental as ti
    from kano import model
    m, cs, ps, ref, _, _ = dense_matrix()
    obj = case("dense-65")[0]
    P = ref["P"]
    gone = [0, P // 3, P - 1]
    keep = [p for p in range(P) if p not in gone]
    left = dict(obj, policies=[obj["policies"][k] for k in keep])
    assert slot_sets(left) == (64, 64)
    m.remove_policies(gone)
    form = m.engine.info()["MATCH_FORM"]
    try:
        ti._check_vs_oracle(m, cs, ps, ti._oracle(obj, keep), "tenant")
    except AssertionError as e:
        raise AssertionError(f"after remove_policies (MATCH_FORM {form}): {e}") from e
    back = [obj["policies"][gone[0]], obj["policies"][gone[-1]]]
    assert slot_sets(dict(obj, policies=left["policies"] + back)) == (65, 65)
    m.add_policies([ti._policy(model, q) for q in back])
    form = m.engine.info()["MATCH_FORM"]
    try:
        ti._check_vs_oracle(m, cs, ps, ti._oracle(obj, keep, back), "tenant")
    except AssertionError as e:
        raise AssertionError(f"after add_policies (MATCH_FORM {form}): {e}") from e
    m.engine.close()


@gpu
def test_dense_two_hops(need_gpu):
    from kano import algorithm as alg
    from oracle import kano_oracle as orc
    m, cs, ps, ref, _, _ = dense_matrix()
    n = ref["n"]
    want = orc.path_c(ref["M"], n, 2)[0]
    assert not np.array_equal(want, ref["M"])
    pm = alg.k_hop(m, 2, "bitwise")
    assert np.array_equal(pm.engine.rows(0, n), want)
    pm.engine.close()
    m.engine.close()


# ---- changing form on one context ------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["plain", "pipelined"])
def test_form_changes_on_one_context(mode, need_gpu):
    """kano_set_policies join -> dense -> join over the same pods: the lists
    name the same key columns, so the kept classification is reused; pipelined,
    a queued prologue meets the changed form."""
    from kano._engine import DeviceBuild
    (oj, rj), (od, rd) = case("join-64"), case("dense-65")
    tj, td = tables(oj), tables(od)
    assert np.array_equal(tj.pod_val, td.pod_val)       # the same pods, the same columns
    n = rj["n"]
    gid = group_of(n)
    eng = DeviceBuild(tj, build=False)
    calls = 1
    if mode == "pipelined":
        eng.set_pipeline(True)
        calls = 4
    reused = eng.info()["CLS_REUSED"]
    for k, (t, ref, form) in enumerate(((tj, rj, 0), (td, rd, 3), (tj, rj, 0))):
        if k:
            eng.set_policies(t)
        assert eng.info()["MATCH_FORM"] == form
        for _ in range(calls):
            check_verify(eng.verify(gid, sys_row=0, shadow=True), ref, 0)
        now = eng.info()["CLS_REUSED"]
        assert now - reused == calls - (k == 0), (k, now, reused)
        reused = now
    eng.settle()
    assert np.array_equal(eng.rows(0, n), rj["M"])
    check_state(eng, rj, policies=(0, 1, 63, 64, rj["P"] - 1))
    eng.close()
