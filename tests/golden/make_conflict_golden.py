"""Golden records of the working policy_conflict, from the reference's own
sets (kano_py), for tests/test_conflict.py.

Runs ONLY in the build container, under the interpreter that has the
reference's dependencies (bitarray, PyYAML):

    /opt/conda/bin/python3.9 tests/golden/make_conflict_golden.py [--big]

kano_py's policy_conflict (algorithm.py:83-100) raises before it answers, so
there is no reference output to record.  The reference supplies the inputs
instead: ReachabilityMatrix.build_matrix gives every policy its
working_allow_set and every container its select_policies, and the predicate
is applied to them here, in this project's words:

    for containers i ascending, for j in S(i), for k in S(i), both in list
    order, j == k skipped by value:  emit (j, k) iff allow_j & allow_k is empty

with S(i) = containers[i].select_policies and allow_p =
policies[p].working_allow_set.  Duplicates are kept (one entry per
container).  Covered: every cluster of tests/golden/clusters/, the paper
example and its rebuilt form (quirk Q5: accumulated lists); with --big also
C2 (written by make_clusters.py --big to /tmp).  Each record goes to
tests/golden/conflict/<name>.json: candidate pairs, count, sha256 of the
(count, 2) int32 pairs, and the first 64 pairs.  Nothing of the reference is
copied: only results on its sets are stored.
"""
import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
REF = "/root/reference/kano_py"
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
from kano import model as ref_model  # noqa: E402
from kano.model import ReachabilityMatrix  # noqa: E402
import sample as ref_sample  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CLUSTERS = os.path.join(HERE, "clusters")
OUT = os.path.join(HERE, "conflict")
HEAD = 64


def objects(obj):
    containers = [ref_model.Container(p["name"], p["labels"]) for p in obj["pods"]]
    policies = []
    for q in obj["policies"]:
        d = ref_model.PolicyIngress if q["direction"] == "ingress" else ref_model.PolicyEgress
        policies.append(ref_model.Policy(q["name"], ref_model.PolicySelect(q["select"]),
                                         ref_model.PolicyAllow(q["allow"]), d,
                                         ref_model.PolicyProtocol(q.get("protocol") or [])))
    return containers, policies


def conflict_pairs(containers, policies):
    """(candidate pairs, the conflicting pairs in emission order)."""
    disjoint = {}

    def test(j, k):
        key = (j, k) if j < k else (k, j)
        hit = disjoint.get(key)
        if hit is None:
            hit = not (policies[j].working_allow_set & policies[k].working_allow_set).any()
            disjoint[key] = hit
        return hit

    pairs, candidates = [], 0
    for c in containers:
        S = list(c.select_policies)
        for j in S:
            for k in S:
                if j == k:
                    continue
                candidates += 1
                if test(j, k):
                    pairs.append((j, k))
    return candidates, pairs


def record(name, containers, policies):
    candidates, pairs = conflict_pairs(containers, policies)
    arr = np.array(pairs, dtype=np.int32).reshape(-1, 2)
    return {"name": name, "n": len(containers), "P": len(policies),
            "candidate_pairs": candidates, "count": len(pairs),
            "sha256": hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest(),
            "head": [list(p) for p in pairs[:HEAD]]}


def write(rec):
    with open(os.path.join(OUT, rec["name"] + ".json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    print(f"{rec['name']}: {rec['candidate_pairs']} candidates, {rec['count']} conflicts",
          flush=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    c, p = ref_sample.paper_example()
    ReachabilityMatrix.build_matrix(c, p)
    write(record("paper_example", c, p))
    ReachabilityMatrix.build_matrix(c, p)      # quirk Q5: the lists accumulate
    write(record("paper_example_rebuilt", c, p))
    for fname in sorted(os.listdir(CLUSTERS)):
        c, p = objects(json.load(open(os.path.join(CLUSTERS, fname))))
        ReachabilityMatrix.build_matrix(c, p)
        write(record(fname[:-5], c, p))
    if "--big" in sys.argv:
        c, p = objects(json.load(open("/tmp/kano_golden_C2.json")))
        ReachabilityMatrix.build_matrix(c, p)
        write(record("C2", c, p))


if __name__ == "__main__":
    main()
