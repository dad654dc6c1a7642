"""matchExpressions requirements (an extension of
kano_py's equality selectors): In / NotIn / Exists / DoesNotExist values in
PolicySelect / PolicyAllow, evaluated on the device (kano_set_expressions,
k_expr_cols) and joined like any other term.  Semantics: the label-selector
requirements kubesv adapts (kubesv/kubesv/model.py:127-160).  kubesv needs z3
and the kubernetes client (absent), so parity is against the restated
semantics in oracle/kano_oracle.py ref_py: parity unpinned against a
reference run."""
import functools
import random

import numpy as np
import pytest


def _cluster(seed, n=120, P=40):
    from kano import model
    rnd = random.Random(seed)
    apps = ["web", "db", "cache", "api", 7, 7.0]
    cs = []
    for i in range(n):
        lab = {"app": rnd.choice(apps)}
        if rnd.random() < 0.6:
            lab["tier"] = rnd.choice(["fe", "be"])
        if rnd.random() < 0.3:
            lab["env"] = rnd.choice(["prod", "dev", float("nan")])
        cs.append(model.Container(f"c{i}", lab))

    def side():
        d = {}
        for _ in range(rnd.randint(0, 3)):
            k = rnd.choice(["app", "tier", "env", "zone"])      # zone: no pod has it
            r = rnd.random()
            if r < 0.2:
                d[k] = model.In(rnd.sample(["web", "db", "fe", "prod", 7, "x"], 2))
            elif r < 0.4:
                d[k] = model.NotIn(rnd.sample(["web", "db", "be", "dev", 7], 2))
            elif r < 0.5:
                d[k] = model.Exists()
            elif r < 0.6:
                d[k] = model.DoesNotExist()
            else:
                d[k] = rnd.choice(["web", "db", "fe", "be", "prod", 7])
        return d

    ps = [model.Policy(f"p{p}", model.PolicySelect(side()), model.PolicyAllow(side()),
                       rnd.choice([model.PolicyIngress, model.PolicyEgress]),
                       model.PolicyProtocol(["TCP"])) for p in range(P)]
    return cs, ps


REAL = {"app": ["web", "db", "cache", "api", 7], "tier": ["fe", "be"], "env": ["prod", "dev"]}


def _cluster2(seed, n, P):
    """_cluster's pods; every side holds one positive term -- a plain value of
    a key pods carry, or In of two of that key's real values plus "x" -- and
    then 0 to 2 further terms of any kind on other keys, so no side is empty
    and few match every pod: the matrix is neither empty nor full."""
    from kano import model
    cs, _ = _cluster(seed, n=n, P=0)
    rnd = random.Random(seed * 7919 + 1)

    def side():
        k0 = rnd.choice(sorted(REAL))
        if rnd.random() < 0.5:
            d = {k0: rnd.choice(REAL[k0])}
        else:
            d = {k0: model.In(rnd.sample(REAL[k0], 2) + ["x"])}
        others = [k for k in ["app", "tier", "env", "zone"] if k != k0]
        for k in rnd.sample(others, rnd.randint(0, 2)):
            r = rnd.random()
            if r < 0.2:
                d[k] = model.In(rnd.sample(["web", "db", "fe", "prod", 7, "x"], 2))
            elif r < 0.4:
                d[k] = model.NotIn(rnd.sample(["web", "db", "be", "dev", 7], 2))
            elif r < 0.5:
                d[k] = model.Exists()
            elif r < 0.6:
                d[k] = model.DoesNotExist()
            else:
                d[k] = rnd.choice(["web", "db", "fe", "be", "prod", 7])
        return d

    ps = [model.Policy(f"p{p}", model.PolicySelect(side()), model.PolicyAllow(side()),
                       rnd.choice([model.PolicyIngress, model.PolicyEgress]),
                       model.PolicyProtocol(["TCP"])) for p in range(P)]
    return cs, ps


def test_host_predicate_matches_oracle():
    """Policy.select_policy / allow_policy (model.py:95-111 plus requirements)
    agree with the oracle's restatement on every container."""
    from oracle import kano_oracle as orc
    for seed in range(5):
        cs, ps = _cluster(seed)
        ref = orc.ref_py(cs, ps)
        keys = {k for c in cs for k in c.labels}
        for p, pol in enumerate(ps):
            for i, c in enumerate(cs):
                pres = all(k in c.labels for k, r in pol.working_selector.labels.items()
                           if k in keys and not hasattr(r, "matches"))
                assert int(pres and pol.select_policy(c)) == int(ref["sel"][p][i])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_expressions_match_oracle(seed):
    from kano import algorithm as alg
    from kano.model import ReachabilityMatrix
    from oracle import kano_oracle as orc
    cs, ps = _cluster(seed)
    ref = orc.ref_py(cs, ps)
    m = ReachabilityMatrix.build_matrix(cs, ps)
    n = m.container_size
    from _golden import words_to_rows01
    assert words_to_rows01(m.engine.rows(0, n), n) == ref["M"]
    assert ["".join(str(int(b)) for b in p.working_select_set.tolist()) for p in ps] == ref["sel"]
    assert ["".join(str(int(b)) for b in p.working_allow_set.tolist()) for p in ps] == ref["allow"]
    assert [list(c.select_policies) for c in cs] == ref["select_policies"]
    assert alg.all_isolated(m) == ref["all_isolated"]
    assert alg.policy_shadow(m, ps, cs) == ref["policy_shadow"]


# (seed, n, P, MATCH_FORM): every expression occurrence is a column, and so a
# slot set, of its own -- 140 policies go dense on both sides, 40 stay joined
FAILING = [(4, 96, 140, 3), (22, 96, 140, 3), (6, 130, 40, 0)]


@functools.lru_cache(maxsize=None)
def _failing(seed, n, P):
    """(containers, policies, oracle record) of _cluster2; shared: the GPU
    tests build on copies of the objects."""
    from oracle import kano_oracle as orc
    cs, ps = _cluster2(seed, n, P)
    return cs, ps, orc.ref_py(cs, ps)


def _ones(ref):
    return sum(r.count("1") for r in ref["M"])


@pytest.mark.parametrize("seed,n,P,form", FAILING)
def test_failing_expressions_say_something(seed, n, P, form):
    """The second generator's conditions, from the oracle alone: a matrix
    neither empty nor full and no empty check but the column ones, one of
    which is non-empty in some seed; the slot sets give the form."""
    import test_match_forms as tm
    from kano._intern import intern
    cs, ps, ref = _failing(seed, n, P)
    assert 0 < _ones(ref) < n * n
    assert ref["system_isolation"] and ref["user_crosscheck"] and ref["policy_shadow"]
    assert any(_failing(*k[:3])[2]["all_isolated"] for k in FAILING)
    assert any(_failing(*k[:3])[2]["all_reachable"] for k in FAILING)
    t = intern(cs, ps)
    assert tm.form_of(tm.table_slot_sets(t)) == form
    assert len(t.expr_col) > P


def test_incremental_prefix_is_dense():
    """test_expressions_incremental's build list (the first 100 policies of
    seed 20) is matched densely on both sides."""
    import test_match_forms as tm
    from kano._intern import intern
    cs, ps = _cluster2(20, 96, 140)
    assert tm.form_of(tm.table_slot_sets(intern(cs, ps[:100]))) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,P,form", FAILING)
def test_failing_expressions_match_oracle(seed, n, P, form):
    import copy
    from kano import algorithm as alg
    from kano._engine import DeviceBuild
    from kano._intern import group_ids, intern
    from kano.model import ReachabilityMatrix
    from _golden import words_to_rows01
    cs, ps, ref = _failing(seed, n, P)
    cs, ps = copy.deepcopy((cs, ps))
    m = ReachabilityMatrix.build_matrix(cs, ps)
    assert m.engine.info()["MATCH_FORM"] == form
    assert words_to_rows01(m.engine.rows(0, n), n) == ref["M"]
    assert ["".join(str(int(b)) for b in p.working_select_set.tolist()) for p in ps] == ref["sel"]
    assert ["".join(str(int(b)) for b in p.working_allow_set.tolist()) for p in ps] == ref["allow"]
    assert [list(c.select_policies) for c in cs] == ref["select_policies"]
    assert [list(c.allow_policies) for c in cs] == ref["allow_policies"]
    assert alg.policy_shadow(m, ps, cs) == ref["policy_shadow"]
    # all five checks in one kano_verify on a context of its own
    eng = DeviceBuild(intern(cs, ps), build=False)
    r = eng.verify(group_ids(cs, "app"), sys_row=0, shadow=True)
    assert eng.info()["MATCH_FORM"] == form
    assert r["all_reachable"].tolist() == ref["all_reachable"]
    assert r["all_isolated"].tolist() == ref["all_isolated"]
    assert r["user_crosscheck"].tolist() == ref["user_crosscheck"]
    assert r["system_isolation"].tolist() == ref["system_isolation"]
    assert [tuple(x) for x in np.asarray(r["pairs"]).reshape(-1, 2).tolist()] == \
        ref["policy_shadow"]
    assert words_to_rows01(eng.rows(0, n), n) == ref["M"]
    eng.close()
    m.engine.close()


E_WIDE = 65537


def _wide_requirements(n=70, E=E_WIDE):
    """(tables without policies, match bool (E, n)): one base column with the
    values -1 (absent) and 0..4, E requirements on it alternating over In,
    NotIn, Exists, DoesNotExist, each evaluated in numpy."""
    from kano._intern import Tables
    rng = np.random.default_rng(70)
    pv = rng.integers(-1, 5, size=(1, n)).astype(np.int32)
    e = np.arange(E)
    op = (e % 4).astype(np.int32)
    a, b = e % 5, (e // 3) % 5
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    cnt = np.where(op < 2, 1 + (lo != hi), 0)             # In / NotIn carry a sorted set
    off = np.zeros(E + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    vals = np.zeros(int(off[-1]), np.int32)
    vals[off[:-1][cnt > 0]] = lo[cnt > 0]
    vals[off[:-1][cnt == 2] + 1] = hi[cnt == 2]
    v = pv[0][None, :]
    listed = (v == lo[:, None]) | (v == hi[:, None])
    present = v != -1
    match = np.where(op[:, None] == 0, listed, np.where(op[:, None] == 1, ~listed, np.where(
        op[:, None] == 2, present, ~present)))
    z = np.zeros(1, np.int64)
    none = np.zeros(0, np.int32)
    t = Tables(n, 1, pv, z, none, none, z, none, none)
    t.expr_col, t.expr_op, t.expr_off, t.expr_val = np.zeros(E, np.int32), op, off, vals
    return t, match


def _naming(t, cols):
    """t with one policy per expression column of cols: select and allow both
    name it."""
    import dataclasses
    off = np.arange(len(cols) + 1, dtype=np.int64)
    col = (t.ncols + np.asarray(cols)).astype(np.int32)
    one = np.ones(len(cols), np.int32)
    return dataclasses.replace(t, sel_off=off, sel_col=col, sel_val=one, alw_off=off,
                               alw_col=col, alw_val=one)


def test_wide_requirements_restatement():
    t, match = _wide_requirements()
    assert match.shape == (E_WIDE, 70) and t.expr_off[-1] == t.expr_val.shape[0]
    for e in (0, 1, 2, 3, E_WIDE - 1):
        v = t.pod_val[0]
        s = set(t.expr_val[t.expr_off[e]:t.expr_off[e + 1]].tolist())
        want = [[x in s, x not in s, x != -1, x == -1][e % 4] for x in v.tolist()]
        assert match[e].tolist() == want and 0 < sum(want) < 70


@pytest.mark.gpu
def test_more_requirements_than_grid_rows():
    """k_expr_cols over E = 65 537 requirements: it launches one grid row per
    requirement, E counts occurrences, and 65 535 rows is where other runtimes
    stop (HIP on the MI355X accepts the launch).  Two policies name two
    expression columns, so the class keys stay at two; the columns named span
    both ends of the grid and all four operators."""
    from kano._engine import DeviceBuild
    import test_match_forms as tm
    t, match = _wide_requirements()
    n = t.n
    eng = None
    for cols in ((0, E_WIDE - 1), (16383, 16385), (32770, 65535)):
        tp_ = _naming(t, cols)
        if eng is None:
            eng = DeviceBuild(tp_)
        else:
            eng.set_policies(tp_)
            eng.build()
        sets = match[list(cols)]
        M = (sets.T.astype(np.int64) @ sets.astype(np.int64)) > 0
        assert 0 < M.sum() < n * n
        assert np.array_equal(eng.rows(0, n), tm.to_words(M)), cols
        for p in range(2):
            s, a = eng.policy_sets(p)
            assert np.array_equal(s, tm.to_words(sets[p:p + 1])[0]), (cols, p)
            assert np.array_equal(a, tm.to_words(sets[p:p + 1])[0]), (cols, p)
    eng.close()


@pytest.mark.gpu
def test_expressions_incremental():
    """An added policy with requirements (host-evaluated extra columns)
    equals a build over the full list."""
    from kano.model import ReachabilityMatrix
    cs, ps = _cluster(11)
    cs2, ps2 = _cluster(11)
    m = ReachabilityMatrix.build_matrix(cs, ps[:30])
    m.add_policies(ps[30:])
    m2 = ReachabilityMatrix.build_matrix(cs2, ps2)
    n = len(cs)
    assert np.array_equal(m.engine.rows(0, n), m2.engine.rows(0, n))
    assert [c.select_policies for c in cs] == [c.select_policies for c in cs2]
    # requirements that can fail, added to a densely matched build: against
    # the oracle over the full list
    from oracle import kano_oracle as orc
    from _golden import words_to_rows01
    n, P = 96, 140
    cs, ps = _cluster2(20, n, P)
    ref = orc.ref_py(cs, ps)
    assert 0 < _ones(ref) < n * n and ref["all_isolated"] and ref["all_reachable"]
    m = ReachabilityMatrix.build_matrix(cs, ps[:100])
    assert m.engine.info()["MATCH_FORM"] == 3
    m.add_policies(ps[100:])
    assert words_to_rows01(m.engine.rows(0, n), n) == ref["M"]
    assert [list(c.select_policies) for c in cs] == ref["select_policies"]
    assert [list(c.allow_policies) for c in cs] == ref["allow_policies"]
    assert ["".join(str(int(b)) for b in p.working_select_set.tolist()) for p in m._policies] == \
        ref["sel"]
