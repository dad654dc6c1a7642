"""Golden records of pair_policies (which policies allow a pod pair), from the
reference's own sets (kano_py), for tests/test_explain.py.

Runs ONLY in the build container, under the interpreter that has the
reference's dependencies (bitarray, PyYAML), like make_redundancy_golden.py
(whose loaders it uses):

    /opt/conda/bin/python3.9 tests/golden/make_explain_golden.py

kano_py has no such query, so there is no reference output to record.  The
reference supplies the inputs instead: ReachabilityMatrix.build_matrix gives
every policy its working_select_set and working_allow_set (the ingress /
egress swap, quirk Q2, applied), and the definition is applied to them here,
in this project's words:

    pols(i, j)  = ascending p with i in select_p and j in allow_p
    cover(i, j) = len(pols(i, j))

The definition is over the sets, so the rebuilt paper example (quirk Q5:
accumulated select_policies lists) gives the record of the plain one.
Covered: every cluster of tests/golden/clusters/, the paper example and its
rebuilt form.  Each record goes to tests/golden/explain/<name>.json: n, P,
the queried pairs (all n * n in row-major order when n <= 64 -- "pairs" is
then left out -- else a seeded sample of 2,048, unsorted, duplicates
possible), their covers and their id lists, flattened in pair order.  Nothing
of the reference is copied: only results on its sets are stored.

The sample is uniform, so most of its pairs have cover 0; on every cluster
whose redundancy record shows popcount_M > sum(impact) (some pair is allowed
by two policies) the sample must hold pairs with cover 0, 1 and >= 2.  SEED
is the first seed for which that holds on all of them (--find-seed searches).
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
from make_redundancy_golden import (CLUSTERS, ReachabilityMatrix, bits, objects,  # noqa: E402
                                    ref_sample)

OUT = os.path.join(HERE, "explain")
REDUNDANCY = os.path.join(HERE, "redundancy")
ALL_PAIRS_MAX_N = 64
SAMPLE = 2048
SEED = 4


def sets(containers, policies):
    n = len(containers)
    sel = np.array([bits(p.working_select_set, n) for p in policies], dtype=np.int32)
    alw = np.array([bits(p.working_allow_set, n) for p in policies], dtype=np.int32)
    return sel.reshape(len(policies), n), alw.reshape(len(policies), n)


def query(n, P, seed):
    if n <= ALL_PAIRS_MAX_N:
        i, j = np.divmod(np.arange(n * n), n)
        return np.stack([i, j], axis=1), True
    rng = np.random.default_rng([seed, n, P])
    return rng.integers(0, n, size=(SAMPLE, 2)), False


def record(name, containers, policies, seed=SEED):
    n, P = len(containers), len(policies)
    sel, alw = sets(containers, policies)
    pairs, every = query(n, P, seed)
    lists = [np.flatnonzero(sel[:, i] & alw[:, j]).tolist() for i, j in pairs.tolist()]
    rec = {"name": name, "n": n, "P": P, "all_pairs": every,
           "cover": [len(l) for l in lists], "policies": [p for l in lists for p in l]}
    if not every:
        rec["pairs"] = pairs.tolist()
    return rec


def overlapping(name):
    """True when the redundancy record shows a pair allowed by two policies."""
    with open(os.path.join(REDUNDANCY, name + ".json")) as f:
        r = json.load(f)
    return r["popcount_M"] > sum(r["impact"])


def mixed(rec):
    c = rec["cover"]
    return 0 in c and 1 in c and any(v >= 2 for v in c)


def inputs():
    c, p = ref_sample.paper_example()
    ReachabilityMatrix.build_matrix(c, p)
    yield "paper_example", c, p
    ReachabilityMatrix.build_matrix(c, p)      # quirk Q5: the lists accumulate, the sets do not
    yield "paper_example_rebuilt", c, p
    for fname in sorted(os.listdir(CLUSTERS)):
        c, p = objects(json.load(open(os.path.join(CLUSTERS, fname))))
        ReachabilityMatrix.build_matrix(c, p)
        yield fname[:-5], c, p


def find_seed(limit=4096):
    built = [(name, c, p) for name, c, p in inputs()
             if len(c) > ALL_PAIRS_MAX_N and overlapping(name)]
    for seed in range(limit):
        if all(mixed(record(name, c, p, seed)) for name, c, p in built):
            return seed
    raise SystemExit("no seed found")


def main():
    if "--find-seed" in sys.argv:
        print("SEED =", find_seed())
        return
    os.makedirs(OUT, exist_ok=True)
    for name, c, p in inputs():
        rec = record(name, c, p)
        if overlapping(name) and not rec["all_pairs"]:
            assert mixed(rec), f"{name}: the sample lacks a cover of 0, 1 or >= 2 (SEED)"
        with open(os.path.join(OUT, name + ".json"), "w") as f:
            json.dump(rec, f, separators=(",", ":"))
        cv = rec["cover"]
        print(f"{name}: n {rec['n']} P {rec['P']} pairs {len(cv)} covered "
              f"{sum(1 for v in cv if v)} twice {sum(1 for v in cv if v >= 2)} "
              f"max {max(cv) if cv else 0} ids {len(rec['policies'])}", flush=True)


if __name__ == "__main__":
    main()
