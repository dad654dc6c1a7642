"""kano_intents' time on a BASELINE config, next to the byte model and to the
parent commit's only route to the same numbers.

K = 64, 1,000 and 5,000 intents (``--ks``) are drawn from the synthetic
cluster's own ``tenant`` / ``ns`` / ``app`` values: each side of an intent is
one (key, value) selector, kinds mixed half and half, and the sets overlap (a
tenant holds its namespaces, apps cut across both, one side in sixteen is
every pod).  Per K:
  device_ms   kano_intents_time (the context is created with KANO_TUNE=timing=1):
              the list and row kernels, no copies
  call_ms     a host clock around DeviceBuild.intents plus a device synchronise:
              the upload of both set arrays and the host's popcounts included
  model_bytes 8 * W * (sum of n_src): every source row of every intent read
              once -- an upper bound on what reaches HBM, since intents that
              share a source row re-read it, from cache when they run together
  model_GBps  model_bytes over device_ms; `hbm_fraction` is that over 8 TB/s
The yardstick is a loop of reach_count over the same intents (one
kano_group_counts call each: two n-entry id arrays uploaded, the column masks
rebuilt), timed on at most 64 of them and reported per intent; its counts
must equal the batched call's `reachable`.  `per_intent_speedup` is the
loop's time per intent over call_ms / K.  One JSON line per K, appended to
--out as it is measured.

    python scripts/intents_bench.py [--config C3] [--ks 64,1000,5000] [--reps 3]
                                    [--out profiles/intents_bench.jsonl]
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
LOOP_MAX = 64       # intents the reach_count loop is timed on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--ks", default="64,1000,5000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intents_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    from kano import algorithm as alg
    from kano._bits import bool_to_words
    from kano._engine import DeviceBuild
    from kano._intern import tables_from_cluster
    from kano.model import ReachabilityMatrix
    from kano.synth import K_APP, K_NS, K_TENANT, make_config
    cl = make_config(a.config)
    base_tune = os.environ.get("KANO_TUNE", "")
    os.environ["KANO_TUNE"] = ",".join(x for x in (base_tune, "timing=1") if x)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    def note(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    eng = DeviceBuild(tables_from_cluster(cl))
    n, W = eng.info()["N"], eng.info()["W"]
    m = ReachabilityMatrix.__new__(ReachabilityMatrix)
    m.container_size, m._engine = n, eng
    rng = np.random.default_rng(a.seed)
    keys = (K_TENANT, K_NS, K_APP)
    present = {k: np.unique(cl.vals[k][cl.vals[k] >= 0]) for k in keys}
    words = {}

    def side():
        """One selector's word set and its pods: a (key, value) of the cluster,
        one time in sixteen every pod."""
        if rng.integers(16) == 0:
            tag = ("all",)
        else:
            k = keys[int(rng.integers(len(keys)))]
            tag = (k, int(rng.choice(present[k])))
        if tag not in words:
            mask = np.ones(n, bool) if tag == ("all",) else cl.vals[tag[0]] == tag[1]
            words[tag] = (bool_to_words(mask), np.flatnonzero(mask))
        return words[tag]

    eng.intents(*(side()[0][None] for _ in range(2)), [0])      # (the first call's warm-up)
    for K in (int(x) for x in a.ks.split(",")):
        picks = [(side(), side()) for _ in range(K)]
        src = np.stack([s[0] for s, _ in picks])
        dst = np.stack([d[0] for _, d in picks])
        flags = (np.arange(K) % 2 * eng.INTENT_ALLOW | eng.INTENT_SELF).astype(np.int32)
        dev, call, r = [], [], None
        try:
            for _ in range(a.reps):
                ms, r = timed(lambda: eng.intents(src, dst, flags))
                call.append(ms)
                dev.append(eng.intents_time())
        except Exception as e:                                   # (the guard on the row reads)
            emit(dict(config=a.config, K=K, n=n, W=W, error=str(e)))
            continue
        dev_ms, call_ms = statistics.median(dev), statistics.median(call)
        rows = int(r["out"][:, 0].sum())
        nbytes = 8 * W * rows
        note(f"K={K}: device {dev_ms:.3f} ms, call {call_ms:.3f} ms, {rows} source rows")
        # the yardstick: one reach_count per intent, the same counts
        L = min(K, LOOP_MAX)
        loop = []
        for _ in range(a.reps):
            ms, got = timed(lambda: [alg.reach_count(m, s[1], d[1]) for s, d in picks[:L]])
            loop.append(ms)
            assert got == r["out"][:L, 3].tolist(), "reach_count disagrees with kano_intents"
        loop_ms = statistics.median(loop) / L
        emit(dict(config=a.config, K=K, n=n, W=W, tune=base_tune, reps=a.reps,
                  device_ms=round(dev_ms, 4), call_ms=round(call_ms, 4), source_rows=rows,
                  violated=int((r["out"][:, 4] > 0).sum()), model_bytes=nbytes,
                  model_GBps=round(nbytes / (dev_ms * 1e-3) / 1e9, 1),
                  hbm_fraction=round(nbytes / (dev_ms * 1e-3) / HBM_PEAK, 4),
                  call_ms_per_intent=round(call_ms / K, 5),
                  device_ms_per_intent=round(dev_ms / K, 5),
                  loop_intents=L, loop_ms_per_intent=round(loop_ms, 4),
                  per_intent_speedup=round(loop_ms / (call_ms / K), 2)))
    eng.close()


if __name__ == "__main__":
    main()
