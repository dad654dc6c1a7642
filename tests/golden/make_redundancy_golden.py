"""Golden records of policy_impact / policy_redundant, from the reference's
own sets (kano_py), for tests/test_redundancy.py.

Runs ONLY in the build container, under the interpreter that has the
reference's dependencies (bitarray, PyYAML):

    /opt/conda/bin/python3.9 tests/golden/make_redundancy_golden.py

kano_py has no such check, so there is no reference output to record.  The
reference supplies the inputs instead: ReachabilityMatrix.build_matrix gives
every policy its working_select_set and working_allow_set (the ingress /
egress swap, quirk Q2, applied), and the definition is applied to them here,
in this project's words:

    cover(i, j) = #{p : i in select_p and j in allow_p}
    impact[p]   = #{(i, j) : i in select_p, j in allow_p, cover(i, j) == 1}
    p redundant iff impact[p] == 0

The definition is over the sets, so the rebuilt paper example (quirk Q5:
accumulated select_policies lists) gives the record of the plain one.
Covered: every cluster of tests/golden/clusters/, the paper example and its
rebuilt form.  Each record goes to tests/golden/redundancy/<name>.json: n, P,
popcount_M (pairs with cover >= 1), the full impact list and the redundant
indices.  Nothing of the reference is copied: only results on its sets are
stored.
"""
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
OUT = os.path.join(HERE, "redundancy")


def objects(obj):
    containers = [ref_model.Container(p["name"], p["labels"]) for p in obj["pods"]]
    policies = []
    for q in obj["policies"]:
        d = ref_model.PolicyIngress if q["direction"] == "ingress" else ref_model.PolicyEgress
        policies.append(ref_model.Policy(q["name"], ref_model.PolicySelect(q["select"]),
                                         ref_model.PolicyAllow(q["allow"]), d,
                                         ref_model.PolicyProtocol(q.get("protocol") or [])))
    return containers, policies


def bits(b, n):
    v = np.array(b.tolist(), dtype=np.int32)
    assert v.shape == (n,)
    return v


def record(name, containers, policies):
    n, P = len(containers), len(policies)
    sel = [bits(p.working_select_set, n) for p in policies]
    alw = [bits(p.working_allow_set, n) for p in policies]
    cover = np.zeros((n, n), dtype=np.int32)
    for s, a in zip(sel, alw):
        cover += np.outer(s, a)
    once = cover == 1
    impact = [int((once & (np.outer(s, a) > 0)).sum()) for s, a in zip(sel, alw)]
    return {"name": name, "n": n, "P": P, "popcount_M": int((cover > 0).sum()),
            "impact": impact, "redundant": [p for p in range(P) if impact[p] == 0]}


def write(rec):
    with open(os.path.join(OUT, rec["name"] + ".json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"))
    imp = rec["impact"]
    print(f"{rec['name']}: n {rec['n']} P {rec['P']} redundant {len(rec['redundant'])} "
          f"sum {sum(imp)} max {max(imp) if imp else 0} popcount_M {rec['popcount_M']}",
          flush=True)


def main():
    os.makedirs(OUT, exist_ok=True)
    c, p = ref_sample.paper_example()
    ReachabilityMatrix.build_matrix(c, p)
    write(record("paper_example", c, p))
    ReachabilityMatrix.build_matrix(c, p)      # quirk Q5: the lists accumulate, the sets do not
    write(record("paper_example_rebuilt", c, p))
    for fname in sorted(os.listdir(CLUSTERS)):
        c, p = objects(json.load(open(os.path.join(CLUSTERS, fname))))
        ReachabilityMatrix.build_matrix(c, p)
        write(record(fname[:-5], c, p))


if __name__ == "__main__":
    main()
