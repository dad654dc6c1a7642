"""kano_hops / kano_hop_pairs' time on a BASELINE config, next to what the
path matrices offer for the same question and to the traffic bound.

On the config's matrix M and on two_hop(M) (``--bases``), four cases:
  levels_1, levels_64   hop_levels for 1 and for 64 random sources
  pairs                 hop_distance for --pairs random pairs
  witnesses             path_witnesses for the reachable ones among them
Per case:
  device_ms   kano_hops_time (the context is created with KANO_TUNE=timing=1):
              the searches' stream time, the per-level waits included
  call_ms     a host clock around the call
  info        kano_hops' info (levels, rows OR-ed, batches, pods reached; the
              pair calls do not return one)
Two yardsticks, neither of them the code under test:
  (a) the same answer from the path matrices, timed in the same run:
      k_hop(m, k) for k = 1 .. the largest finite distance the case found, then
      transitive_closure(m), then one read per query and matrix -- a row per
      source for the levels cases, a kano_get_bit per pair for the pair cases
      (a route cannot be had from them at all: the witnesses case is held to
      the distances' yardstick).  `faster_than_a` is the one condition.
  (b) the traffic bound: a search reads each reached pod's row once, at most
      8 * W * rows_ored bytes; `hbm_fraction` is that over device_ms as a
      fraction of 8 TB/s.  No pass mark.
One JSON line per case and base, appended to --out as it is measured.

    python scripts/hops_bench.py [--config C3] [--bases M,two_hop] [--pairs 10000]
                                 [--reps 5] [--out profiles/hops_bench.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--bases", default="M,two_hop")
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hops_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    from kano import algorithm as alg
    from kano._engine import DeviceBuild
    from kano._intern import tables_from_cluster
    from kano.model import ReachabilityMatrix
    from kano.synth import make_config
    cl = make_config(a.config)
    base_tune = os.environ.get("KANO_TUNE", "")
    os.environ["KANO_TUNE"] = ",".join(x for x in (base_tune, "timing=1") if x)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    def wrap(eng, n):
        m = ReachabilityMatrix.__new__(ReachabilityMatrix)
        m.container_size, m._engine = n, eng
        m._containers = m._policies = m._lists = None
        m._ncontainers = n
        return m

    def note(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")

    built = DeviceBuild(tables_from_cluster(cl))
    n, W = built.info()["N"], built.info()["W"]
    rng = np.random.default_rng(a.seed)
    sources = rng.choice(n, size=64, replace=False).astype(np.int32)
    pairs = rng.integers(0, n, size=(a.pairs, 2)).astype(np.int32)

    for base in a.bases.split(","):
        m = wrap(built, n)
        if base == "two_hop":
            m = alg.two_hop(m)
        elif base != "M":
            raise SystemExit(f"unknown base {base!r}")
        eng = m.engine
        set_bits = int(eng.group_counts(np.zeros(n, np.int32), np.zeros(n, np.int32), 1, 1)
                       ["counts"][0, 0])
        eng.hops(sources[:1])                        # (first call: the allocations' warm-up)
        note(f"{base}: {set_bits} set bits")

        def run(fn, reps):
            dev, call, out = [], [], None
            for _ in range(reps):
                ms, out = timed(fn)
                call.append(ms)
                dev.append(eng.hops_time())
            return statistics.median(dev), statistics.median(call), out

        cases = {}
        for name, src in (("levels_1", sources[:1]), ("levels_64", sources)):
            dev, call, r = run(lambda: eng.hops(src), a.reps)
            cases[name] = dict(device_ms=dev, call_ms=call, info=r["info"], queries=len(src),
                               dmax=int(r["dist"].max()), src=src)
            note(f"{base} {name}: {call:.3f} ms, {r['info']}")
        dev, call, r = run(lambda: eng.hop_pairs(pairs), 1)
        dist = r["dist"]
        cases["pairs"] = dict(device_ms=dev, call_ms=call, info=None, queries=len(pairs),
                              dmax=int(dist.max()), reachable=int((dist >= 1).sum()),
                              distinct_sources=int(np.unique(pairs[:, 0]).shape[0]))
        reach = pairs[dist >= 1]
        note(f"{base} pairs: {call:.3f} ms, {len(reach)} reachable")
        dev, call, r = run(lambda: eng.hop_pairs(reach, paths=True), 1)
        assert np.array_equal(r["dist"], dist[dist >= 1])
        cases["witnesses"] = dict(device_ms=dev, call_ms=call, info=None, queries=len(reach),
                                  dmax=int(r["dist"].max(initial=-1)),
                                  path_nodes=int(r["nodes"].shape[0]))

        # yardstick (a): the path matrices of the parent commit, built once up
        # to the largest distance any case found and timed one by one
        kmax = max(max(c["dmax"] for c in cases.values()), 1)
        mats, build_ms = [], []
        for k in list(range(1, kmax + 1)) + [0]:
            ms, pm = timed(lambda: alg.k_hop(m, k) if k else alg.transitive_closure(m))
            mats.append(pm)
            build_ms.append(ms)
            note(f"{base} yardstick matrix k={k}: {ms:.3f} ms")

        def yardstick(c, probe):
            """k_hop for k = 1 .. the case's dmax and the closure, then the reads."""
            use = list(range(max(c["dmax"], 1))) + [kmax]
            ms, got = timed(lambda: [probe(mats[k].engine) for k in use])
            return dict(matrices=len(use), build_ms=round(sum(build_ms[k] for k in use), 3),
                        read_ms=round(ms, 3)), got

        for name, c in cases.items():
            if name.startswith("levels"):
                src = c.pop("src")
                y, got = yardstick(c, lambda e: np.concatenate([e.rows(int(s), 1) for s in src]))
            else:
                q = pairs if name == "pairs" else reach
                y, got = yardstick(c, lambda e: [e.get_bit(int(i), int(j)) for i, j in q])
                # the same answer: the first matrix holding the pair's bit
                if len(q):
                    bits = np.array(got[:-1], dtype=bool).reshape(len(got) - 1, len(q))
                    first = np.where(bits.any(axis=0), bits.argmax(axis=0) + 1, -1)
                    want = dist if name == "pairs" else dist[dist >= 1]
                    assert np.array_equal(first, want), name
            y["total_ms"] = round(y["build_ms"] + y["read_ms"], 3)
            rec = dict(config=a.config, base=base, case=name, n=n, W=W, set_bits=set_bits,
                       tune=base_tune, yardstick_a=y,
                       faster_than_a=bool(c["call_ms"] < y["total_ms"]),
                       speedup_vs_a=round(y["total_ms"] / c["call_ms"], 2))
            rec.update({k: (round(v, 4) if isinstance(v, float) else v) for k, v in c.items()})
            if c["info"]:
                nbytes = 8 * W * c["info"]["rows_ored"]
                rec["bound_bytes"] = nbytes
                rec["hbm_fraction"] = round(nbytes / (c["device_ms"] * 1e-3) / HBM_PEAK, 4)
                rec["device_ms_per_level"] = round(c["device_ms"] /
                                                   max(c["info"]["levels"] + 1, 1) /
                                                   c["info"]["batches"], 4)
            emit(rec)
        for pm in mats:
            pm.engine.close()
        if base != "M":
            eng.close()
    built.close()


if __name__ == "__main__":
    main()
