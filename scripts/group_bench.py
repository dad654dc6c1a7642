"""kano_group_counts' time on a BASELINE config, next to a streamed read.

The config's build is grouped by three of its labels, source and destination
side alike: ``tenant`` (64 groups, one batch of destination groups), ``ns``
(about 100 groups, two batches) and ``app`` (about 5,000 groups, many
batches).  Per label (counts only; ``--rows`` adds the label's row_counts
form where that array stays under 1 GiB):
  device_ms  HIP events around the fills, k_group_masks and k_group_rows (the
             context is created with KANO_TUNE=timing=1; kano_group_counts_time)
  call_ms    a host clock around kano_group_counts plus a device
             synchronisation: the host's argsort and uploads, the kernels, the
             copy of the counts
  ratio      device_ms and call_ms over the yardstick's
The yardstick is kano_diff(a, a) totals-only on the same context: one
streamed read of two matrices (2 * rows * W * 8 bytes).  Medians over --reps
calls after --warmup, the cases alternating.  One JSON line, appended to
--out when given.

    python scripts/group_bench.py [--config C3] [--reps 20] [--warmup 3] [--out FILE]
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
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
            "max_ms": round(max(v), 4), "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--labels", default="tenant,ns,app")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from kano._engine import DeviceBuild
    from kano._intern import tables_from_cluster
    from kano.synth import KEY_NAMES, make_config
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
    empty = DeviceBuild.empty(n)
    bits = A.diff(empty, rows=False, cols=False)["removed"]    # the set bits, by k_diff_rows
    empty.close()
    gids = {}
    for label in a.labels.split(","):
        # (a pod without the label: value -1, a group of its own -- user_hashmap's "")
        g = np.unique(cl.vals[KEY_NAMES.index(label)], return_inverse=True)[1].astype(np.int32)
        gids[label] = (g, int(g.max()) + 1)
    cases = [(label, False) for label in gids]
    if a.rows:
        cases += [(label, True) for label, (_, G) in gids.items() if n * G * 4 <= 1 << 30]
    ts = {(c, k): [] for c in cases + ["diff"] for k in ("device", "call")}
    for rep in range(a.warmup + a.reps):
        ms, d = timed(lambda: A.diff(A, rows=False, cols=False))
        assert (d["added"], d["removed"]) == (0, 0)
        if rep >= a.warmup:
            ts[("diff", "device")].append(A.diff_time())
            ts[("diff", "call")].append(ms)
        for c in cases:
            g, G = gids[c[0]]
            ms, r = timed(lambda: A.group_counts(g, g, G, G, rows=c[1]))
            assert int(r["counts"].sum()) == bits, (c, int(r["counts"].sum()), bits)
            if c[1]:
                assert int(r["row_counts"].sum(dtype=np.int64)) == bits
            if rep >= a.warmup:
                ts[(c, "device")].append(A.group_counts_time())
                ts[(c, "call")].append(ms)
    A.close()
    yard = {"device_ms": stats(ts[("diff", "device")]), "call_ms": stats(ts[("diff", "call")])}
    out_cases = {}
    for c in cases:
        g, G = gids[c[0]]
        dev, call = stats(ts[(c, "device")]), stats(ts[(c, "call")])
        out_cases[c[0] + ("+rows" if c[1] else "")] = {
            "groups": G, "batches": (G + 63) // 64, "device_ms": dev, "call_ms": call,
            "device_ratio": round(dev["median_ms"] / yard["device_ms"]["median_ms"], 2),
            "call_ratio": round(call["median_ms"] / yard["call_ms"]["median_ms"], 2),
            "device_ms_per_batch": round(dev["median_ms"] / ((G + 63) // 64), 4)}
    out = {"config": a.config, "n": n, "W": W, "P": cl.P, "tune": base_tune, "bits": bits,
           "matrix_bytes": n * W * 8,
           "read_floor_ms_at_8TBps": round(n * W * 8 / HBM_PEAK * 1e3, 4),
           "yardstick_diff_a_a_totals": yard, "cases": out_cases}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
