"""The working policy_conflict's time beside policy_shadow's on a BASELINE
config: on one context with the matrix built, kano_shadow, kano_conflict_pairs
count-only and kano_conflict_pairs in pairs mode alternate; a host clock
around each call plus a device synchronisation (the calls return with their
emission still queued).  Pairs mode is skipped when the pairs would take more
than 4 GB (8 bytes each).  One JSON line.

    python scripts/conflict_bench.py [--config C3] [--reps 20] [--warmup 3] [--no-shadow]
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

PAIRS_BYTES_MAX = 4 << 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-shadow", action="store_true",
                    help="leave kano_shadow out (C4: its ~1e11 pairs fit no buffer)")
    a = ap.parse_args()
    from kano._engine import DeviceBuild
    from kano._native import KanoNativeError
    from kano._intern import tables_from_cluster
    from kano.synth import make_config
    cl = make_config(a.config)
    eng = DeviceBuild(tables_from_cluster(cl))
    info = eng.info()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    _, (count, class_pairs) = timed(lambda: eng._conflict_run(1))
    with_pairs = 8 * count <= PAIRS_BYTES_MAX
    ts = {"shadow": [], "conflict_count": [], "conflict_pairs": []}
    shadow_count, ms_s = None, None
    shadow_err = "not run (--no-shadow)" if a.no_shadow else None
    for rep in range(a.warmup + max(a.reps, 20)):
        if shadow_err is None:
            try:
                ms_s, shadow_count = timed(eng.shadow_count)
            except KanoNativeError as e:   # (C4: ~1e11 shadow pairs do not fit)
                shadow_err, ms_s = str(e), None
        ms_c, (c1, _) = timed(lambda: eng._conflict_run(1))
        assert c1 == count
        ms_p = None
        if with_pairs:
            ms_p, (c0, _) = timed(lambda: eng._conflict_run(0))
            assert c0 == count
        if rep >= a.warmup:
            if shadow_err is None:
                ts["shadow"].append(ms_s)
            ts["conflict_count"].append(ms_c)
            if ms_p is not None:
                ts["conflict_pairs"].append(ms_p)

    def stats(v):
        if not v:
            return None
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
                "max_ms": round(max(v), 4), "reps": len(v)}

    out = {"config": a.config, "n": cl.n, "P": cl.P, "row_classes": info.get("U"),
           "col_classes": info.get("UA"), "tune": os.environ.get("KANO_TUNE", ""),
           "shadow_pairs": None if shadow_count is None else int(shadow_count),
           "shadow_error": shadow_err, "conflict_pairs": int(count),
           "conflict_class_pairs": int(class_pairs),
           "pairs_mode": "run" if with_pairs else "skipped: the pairs exceed 4 GB",
           "kano_shadow": stats(ts["shadow"]),
           "kano_conflict_pairs_count_only": stats(ts["conflict_count"]),
           "kano_conflict_pairs_pairs": stats(ts["conflict_pairs"])}
    eng.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
