"""policy_impact's time on a BASELINE config, beside a plain build and
kano_conflict_pairs count-only on the same context in the same run.

Per mode (0: impacts, 1: flags only):
  call_ms    a host clock around kano_policy_impact plus a device
             synchronisation: the fill, the kernel and the copy of the P
             results to the host
  device_ms  HIP events around the fill and the kernel alone (a second
             context created with KANO_TUNE=timing=1; kano_stage_times slot 7)
and device_ms again with each kernel form forced (impf=1 list, impf=2 rows),
which is what the crossover between them is read from.  Medians over --reps
calls after --warmup, the calls of the different kinds alternating.  One JSON
line, appended to --out when given.

    python scripts/redundancy_bench.py [--config C3] [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kubernetes-verification_amd")]

import torch  # noqa: E402,F401  (first: its HIP runtime serves the process, as in bench.py)


def stats(v):
    if not v:
        return None
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
            "max_ms": round(max(v), 4), "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from kano._engine import DeviceBuild
    from kano._intern import tables_from_cluster
    from kano.synth import make_config
    cl = make_config(a.config)
    tables = tables_from_cluster(cl)
    base_tune = os.environ.get("KANO_TUNE", "")

    def context(tune):
        os.environ["KANO_TUNE"] = ",".join(x for x in (base_tune, tune) if x)
        try:
            return DeviceBuild(tables)
        finally:
            os.environ["KANO_TUNE"] = base_tune

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    eng = context("")
    info = eng.info()
    want = eng.policy_impact()
    ess = eng.policy_essential()
    assert np.array_equal(ess, want > 0)
    ts = {"build": [], "conflict_count": [], "impact_call": [], "flags_call": []}
    for rep in range(a.warmup + a.reps):
        ms_b, _ = timed(eng.build)
        ms_c, _ = timed(eng.conflict_count)
        ms_i, got = timed(eng.policy_impact)
        assert np.array_equal(got, want)
        ms_f, got = timed(eng.policy_essential)
        assert np.array_equal(got, ess)
        if rep >= a.warmup:
            for k, v in zip(ts, (ms_b, ms_c, ms_i, ms_f)):
                ts[k].append(v)
    eng.close()

    device = {}
    for label, tune in (("auto", "timing=1"), ("list", "timing=1,impf=1"),
                        ("rows", "timing=1,impf=2")):
        e = context(tune)
        dt = {"impact": [], "flags": []}
        for rep in range(a.warmup + a.reps):
            assert np.array_equal(e.policy_impact(), want)
            ms_i = e.stage_times()["impact"]
            assert np.array_equal(e.policy_essential(), ess)
            ms_f = e.stage_times()["impact"]
            if rep >= a.warmup:
                dt["impact"].append(ms_i)
                dt["flags"].append(ms_f)
        e.close()
        device[label] = {k: stats(v) for k, v in dt.items()}

    out = {"config": a.config, "n": cl.n, "P": cl.P, "row_classes": info.get("U"),
           "col_classes": info.get("UA"), "select_entries": info.get("NNZ_SEL"),
           "tune": base_tune, "redundant": int((want == 0).sum()),
           "impact_sum": int(want.sum()), "impact_max": int(want.max()) if want.size else 0,
           "kano_build": stats(ts["build"]),
           "kano_conflict_pairs_count_only": stats(ts["conflict_count"]),
           "kano_policy_impact_mode0_call": stats(ts["impact_call"]),
           "kano_policy_impact_mode1_call": stats(ts["flags_call"]),
           "device_ms": device}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
