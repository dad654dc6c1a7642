"""kano_diff's time on a BASELINE config against the bytes it must move.

Three cases, each against the config's own build A:
  identical  a second build of the same tables (nothing differs)
  removed    the same build after remove_policies of its largest-impact policy
  empty      a matrix with no bit set (everything A holds is "removed")
Per case and form (full: totals + row counts + column words; totals: the
totals-only kernel):
  device_ms  HIP events around the result fill and k_diff_rows alone (the
             contexts are created with KANO_TUNE=timing=1; kano_diff_time)
  call_ms    a host clock around kano_diff plus a device synchronisation: fill,
             kernel and the copies of the results to the host
  hbm_frac   2 * rows * W * 8 bytes (every word of both matrices once) over
             device_ms, as a fraction of the 8 TB/s HBM peak
Medians over --reps calls after --warmup, the cases and forms alternating.
One JSON line, appended to --out when given.

    python scripts/diff_bench.py [--config C3] [--reps 30] [--warmup 5] [--out FILE]
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

HBM_PEAK = 8.0e12   # bytes/s: the figure of the project's roofline lines


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
    os.environ["KANO_TUNE"] = ",".join(x for x in (base_tune, "timing=1") if x)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    A = DeviceBuild(tables)
    info = A.info()
    n, W = info["N"], info["W"]
    impact = A.policy_impact()
    p = int(np.argmax(impact))
    others = {"identical": DeviceBuild(tables), "removed": DeviceBuild(tables),
              "empty": DeviceBuild.empty(n)}
    others["removed"].remove_policies([p])
    bits = A.diff(others["empty"], rows=False, cols=False)["removed"]
    expect = {"identical": (0, 0), "removed": (0, int(impact[p])), "empty": (0, bits)}
    nbytes = 2 * n * W * 8
    ts = {(c, f, k): [] for c in others for f in ("full", "totals") for k in ("device", "call")}
    for rep in range(a.warmup + a.reps):
        for c, B in others.items():
            for f in ("full", "totals"):
                full = f == "full"
                ms, d = timed(lambda: A.diff(B, rows=full, cols=full))
                assert (d["added"], d["removed"]) == expect[c], (c, f, d["added"], d["removed"])
                if full:
                    assert int(d["row_removed"].sum()) == expect[c][1]
                if rep >= a.warmup:
                    ts[(c, f, "device")].append(B.diff_time())
                    ts[(c, f, "call")].append(ms)
    cases = {}
    for c in others:
        cases[c] = {"added": expect[c][0], "removed": expect[c][1]}
        for f in ("full", "totals"):
            dev = stats(ts[(c, f, "device")])
            cases[c][f] = {"device_ms": dev, "call_ms": stats(ts[(c, f, "call")]),
                           "hbm_frac": round(nbytes / (dev["median_ms"] * 1e-3) / HBM_PEAK, 3)}
    for e in list(others.values()) + [A]:
        e.close()
    out = {"config": a.config, "n": n, "W": W, "P": cl.P, "tune": base_tune,
           "removed_policy": p, "bytes": nbytes,
           "floor_ms_at_8TBps": round(nbytes / HBM_PEAK * 1e3, 4), "cases": cases}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
