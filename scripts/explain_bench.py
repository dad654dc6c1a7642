"""pair_policies' time on a BASELINE config for Q query pairs, beside the host
route it replaces.

Two sets of pairs:
  random  uniformly random (i, j)
  added   the pairs a diff reports as added after adding 10 synthetic policies
          (each the select terms of one build policy with the allow terms of
          another), ascending by i then j, truncated to Q; the query then runs
          on the updated matrix
Per set and mode (1: the counts and the per-policy histogram, "blame"; 0: the
counts, the offsets and the id lists, no histogram):
  device_ms  kano_pair_policies_time under KANO_TUNE=timing=1: HIP events
             around the fill, the count pass, the offsets' scan and the emit
             pass, no copies -- with the form the engine picks and with each
             form forced (ppf=1 a lane per pair, ppf=2 a wave per pair)
  call_ms    a host clock around DeviceBuild.pair_policies plus a device
             synchronisation: the upload of the pairs, the passes and the
             copies of the results to the host
  floor_ms   the bytes the query must move (pairs read; cover, offsets and ids
             written) at the 8 TB/s spec figure DESIGN.md uses
  host_route kano_get_policy_sets for --host-policies of the policies plus the
             numpy test of the same pairs against both sets, timed and scaled
             to all P policies (scaled: true in the output)
Medians over --reps calls after --warmup.  One JSON line, appended to --out.

    python scripts/explain_bench.py [--config C3] [--pairs 1000000] [--reps 30] [--warmup 5]
                                    [--out profiles/explain_bench.jsonl]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kubernetes-verification_amd")]

import torch  # noqa: E402,F401  (first: its HIP runtime serves the process, as in bench.py)

HBM_PEAK = 8e12
FORMS = (("auto", ""), ("lane", "ppf=1"), ("wave", "ppf=2"))


def stats(v):
    if not v:
        return None
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
            "max_ms": round(max(v), 4), "reps": len(v)}


def digest(r):
    h = hashlib.sha256()
    for k in ("cover", "offsets", "policies", "hist"):
        if r.get(k) is not None:
            h.update(r[k].tobytes())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-policies", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    from kano._engine import DeviceBuild
    from kano._intern import tables_from_cluster
    from kano.synth import make_config
    cl = make_config(a.config)
    t = tables_from_cluster(cl)
    n, P, Q = t.n, t.P, a.pairs
    base_tune = os.environ.get("KANO_TUNE", "")
    rng = np.random.default_rng(20251020)

    def context(tune):
        os.environ["KANO_TUNE"] = ",".join(x for x in (base_tune, "timing=1", tune) if x)
        try:
            return DeviceBuild(t)
        finally:
            os.environ["KANO_TUNE"] = base_tune

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, v

    # the 10 synthetic policies: select terms of policy sa[k], allow terms of policy al[k]
    sa, al = rng.integers(0, P, 10), rng.integers(0, P, 10)

    def terms(off, col, val, which):
        o = np.zeros(len(which) + 1, np.int64)
        np.cumsum([off[p + 1] - off[p] for p in which], out=o[1:])
        pick = np.concatenate([np.arange(off[p], off[p + 1]) for p in which]).astype(np.int64)
        return o, col[pick], val[pick]

    new_sel = terms(t.sel_off, t.sel_col, t.sel_val, sa.tolist())
    new_alw = terms(t.alw_off, t.alw_col, t.alw_val, al.tolist())

    def update(e):
        e.add_policies(np.zeros((0, n), np.int32), new_sel, new_alw)

    # the query sets
    sets = {"random": np.stack([rng.integers(0, n, Q), rng.integers(0, n, Q)],
                               axis=1).astype(np.int32)}
    eng = {label: context(tune) for label, tune in FORMS}
    info = eng["auto"].info()
    snap = DeviceBuild.empty(n)
    snap.copy_from(eng["auto"])
    results = {}

    def measure(name, pairs, updated):
        out = {"Q": int(pairs.shape[0]), "updated": updated}
        ref = {}
        for label, _ in FORMS:
            e = eng[label]
            dev = {0: [], 1: []}
            call = {0: [], 1: []}
            for rep in range(a.warmup + a.reps):
                for mode in (1, 0):
                    ms, r = timed(lambda: e.pair_policies(pairs, lists=mode == 0, hist=mode == 1))
                    d = digest(r)
                    assert ref.setdefault(mode, d) == d, (name, label, mode)
                    if rep >= a.warmup:
                        dev[mode].append(e.pair_policies_time())
                        call[mode].append(ms)
            print(f"[{a.config}] {name} {label} done", file=sys.stderr, flush=True)
            out[label] = {"mode1_device": stats(dev[1]), "mode0_device": stats(dev[0]),
                          "mode1_call": stats(call[1]), "mode0_call": stats(call[0])}
        r = eng["auto"].pair_policies(pairs, hist=True)
        total = int(r["offsets"][-1])
        q = pairs.shape[0]
        # cover > 0 is the matrix bit (no edits): a spot check of 256 pairs
        for k in rng.integers(0, max(q, 1), 256 if q else 0).tolist():
            assert (r["cover"][k] > 0) == bool(eng["auto"].get_bit(*pairs[k].tolist()))
        out.update(total_ids=total, covered=int((r["cover"] > 0).sum()),
                   max_cover=int(r["cover"].max()) if q else 0)
        fl = {1: 8 * q + 4 * q, 0: 8 * q + 4 * q + 8 * (q + 1) + 4 * total}
        out["bytes"] = {"mode1": fl[1], "mode0": fl[0]}
        out["floor_ms_at_8TBps"] = {"mode1": round(fl[1] / HBM_PEAK * 1e3, 5),
                                    "mode0": round(fl[0] / HBM_PEAK * 1e3, 5)}
        for mode in (1, 0):
            med = out["auto"][f"mode{mode}_device"]["median_ms"]
            out[f"mode{mode}_floor_ratio"] = round(med / (fl[mode] / HBM_PEAK * 1e3), 1) \
                if med else None
        # the host route: every policy's sets to the host, the pairs tested in numpy
        k = min(a.host_policies, P)
        sub = rng.choice(P, size=k, replace=False)
        iw, ib = pairs[:, 0] >> 6, (pairs[:, 0] & 63).astype(np.uint64)
        jw, jb = pairs[:, 1] >> 6, (pairs[:, 1] & 63).astype(np.uint64)
        t0 = time.perf_counter()
        cover = np.zeros(q, np.int32)
        for p in sub.tolist():
            s, al_ = eng["auto"].policy_sets(p)
            hit = ((s[iw] >> ib) & (al_[jw] >> jb) & np.uint64(1)).astype(bool)
            cover += hit
        host_ms = (time.perf_counter() - t0) * 1e3
        out["host_route"] = {"policies_timed": int(k), "ms_timed": round(host_ms, 1),
                             "ms_all_policies": round(host_ms * P / k, 1), "scaled": k < P}
        results[name] = out

    measure("random", sets["random"], False)
    for e in eng.values():
        update(e)
    # the added pairs, ascending by i, from the first rows that hold Q of them
    d = snap.diff(eng["auto"], cols=False)
    csum = np.cumsum(d["row_added"].astype(np.int64))
    r1 = int(np.searchsorted(csum, Q)) + 1 if csum.size and csum[-1] > Q else n
    added = snap.diff_pairs(eng["auto"], "added", 0, r1, limit=int(csum[r1 - 1]) + 1)[:Q]
    measure("added", np.ascontiguousarray(added), True)
    results["added"]["diff_added_total"] = int(d["added"])
    for e in list(eng.values()) + [snap]:
        e.close()

    sbar = info["NNZ_SEL"] / max(info["U"], 1)
    ceil_s = -(-info["NNZ_SEL"] // max(info["U"], 1))      # (the engine's rule, PAIR_WAVE_MIN)
    out = {"config": a.config, "n": n, "P": P, "row_classes": info["U"],
           "col_classes": info["UA"], "select_entries": info["NNZ_SEL"],
           "mean_list": round(sbar, 2), "max_list": info["MAXSEL"],
           "form_taken": {"built": "wave" if ceil_s > 16 else "lane",
                          "updated": "wave" if ceil_s + 10 > 16 else "lane"},
           "tune": base_tune, "sets": results}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
