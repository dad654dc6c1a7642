"""kano_verdict_matrix / kano_pair_verdicts' time on a BASELINE config, next to
the subset write of all policies and to pair_ports.

Every policy of the config gets the tests' tier rule: deny[p] = (p % 3 == 1),
level (p*5 + p//7) % L, the levels mapped to priorities by the tests' tables
(the int32 extremes at L = 3, a shuffled, gapped, partly negative table at
L = 70).  Per config one JSON line, appended to --out:
  verdict_device_ms   {L: kano_verdict_matrix_time} for L = 1, 3, 70 (the
                      context is created with KANO_TUNE=timing=1): the fills,
                      the ordered copy of the class lists, the class rows,
                      their expansion and the write of every held row
  subset_device_ms    kano_policy_subset_time for policy_subset_matrix(all
                      policies): the same n^2 write from one OR a class
  verdict_over_subset {L: verdict_device_ms / subset_device_ms}
  *_call_ms           a host clock around the calls (the destination's
                      creation and allocation included)
  pair_verdicts_*     pair_verdicts (L = 3) for --pairs random pairs: device
                      time (kano_pair_verdicts_time) and call time, next to
  pair_ports_*        pair_ports on the same pairs (kano_pair_masks_time)
The calls alternate within a repetition; the medians are reported.  The
verdict rows are checked once against subset(allows) & ~subset(denies) at
L = 1 by digest of the packed rows.  No pass mark.

    python scripts/verdict_bench.py [--configs C3] [--pairs 1000000] [--reps 7]
                                    [--out profiles/verdict_bench.jsonl]
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

LEVELS = (1, 3, 70)


def priority_table(L):
    """tests/test_verdicts.py's level -> priority tables."""
    if L == 1:
        return (5,)
    if L == 3:
        return (-2147483648, 0, 2147483647)
    return tuple(((l * 37) % L - 30) * 1000 + 7 * (l % 3) for l in range(L))


def tier_rule(P, L):
    import numpy as np
    p = np.arange(P)
    table = np.array(priority_table(L), dtype=np.int64)
    return (p % 3 == 1).astype(np.uint8), table[(p * 5 + p // 7) % L].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C3")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verdict_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    from kano import algorithm as alg
    from kano import model
    from kano.synth import make_config, objects_from_json
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

    med = statistics.median
    for config in a.configs.split(","):
        obj = make_config(config).to_json_obj()
        cs, ps = objects_from_json(obj, model)
        P = len(ps)
        note(f"{config}: {len(cs)} pods, {P} policies")
        m = model.ReachabilityMatrix.build_matrix(cs, ps)
        eng = m.engine
        info = eng.info()
        n, W = info["N"], info["W"]
        tiers = {L: alg.Tiering(*tier_rule(P, L)) for L in LEVELS}
        rng = np.random.default_rng(a.seed)
        pairs = rng.integers(0, n, size=(a.pairs, 2)).astype(np.int32)

        # L = 1 against the two subsets (and the warm-up of every call timed below)
        deny = tiers[1].actions.astype(bool)
        v1 = alg.verdict_matrix(m, tiers[1])
        sa = alg.policy_subset_matrix(m, np.flatnonzero(~deny))
        sd = alg.policy_subset_matrix(m, np.flatnonzero(deny))
        same = True
        for r0 in range(0, n, 4096):
            k = min(4096, n - r0)
            same &= bool(np.array_equal(v1.engine.rows(r0, k),
                                        sa.engine.rows(r0, k) & ~sd.engine.rows(r0, k)))
        vinfo = {1: v1.verdict_info}
        for x in (v1, sa, sd):
            x.engine.close()
        for L in LEVELS[1:]:
            vm = alg.verdict_matrix(m, tiers[L])
            vinfo[L] = vm.verdict_info
            vm.engine.close()
        alg.policy_subset_matrix(m, range(P)).engine.close()

        dev = {L: [] for L in LEVELS}
        call = {L: [] for L in LEVELS}
        sub_dev, sub_call = [], []
        for _ in range(a.reps):                              # alternating within a repetition
            for L in LEVELS:
                ms, vm = timed(lambda: alg.verdict_matrix(m, tiers[L]))
                call[L].append(ms)
                dev[L].append(eng.verdict_time())
                vm.engine.close()
            ms, sm = timed(lambda: alg.policy_subset_matrix(m, range(P)))
            sub_call.append(ms)
            sub_dev.append(eng.subset_time())
            sm.engine.close()
        subset_ms = med(sub_dev)
        note(f"{config} subset(all): {subset_ms:.3f} ms device; verdict: " +
             ", ".join(f"L={L} {med(dev[L]):.3f} ms" for L in LEVELS))

        for p, pol in enumerate(ps):                         # pair_ports' table: 8 keys
            pol.protocol = None if p % 10 == 9 else model.PolicyProtocol(["TCP", str(8000 + p % 8)])
        alg.pair_verdicts(m, pairs[:1024], tiers[3])
        alg.pair_ports(m, pairs[:1024])
        pv_dev, pv_call, pp_dev, pp_call = [], [], [], []
        for _ in range(a.reps):
            ms, pv = timed(lambda: alg.pair_verdicts(m, pairs, tiers[3]))
            pv_call.append(ms)
            pv_dev.append(eng.pair_verdicts_time())
            ms, pp = timed(lambda: alg.pair_ports(m, pairs))
            pp_call.append(ms)
            pp_dev.append(eng.pair_masks_time())
        assert np.array_equal(pp.masks.any(axis=1), pv.verdict > 0)

        nbytes = 8 * n * ((W + 15) // 16 * 16)
        rec = dict(config=config, n=n, W=W, P=P, tune=base_tune, matrix_bytes=nbytes, reps=a.reps,
                   verdict_info={str(L): vinfo[L] for L in LEVELS},
                   verdict_device_ms={str(L): round(med(dev[L]), 4) for L in LEVELS},
                   verdict_device_min_max={str(L): [round(min(dev[L]), 4), round(max(dev[L]), 4)]
                                           for L in LEVELS},
                   verdict_call_ms={str(L): round(med(call[L]), 3) for L in LEVELS},
                   subset_device_ms=round(subset_ms, 4),
                   subset_device_min_max=[round(min(sub_dev), 4), round(max(sub_dev), 4)],
                   subset_call_ms=round(med(sub_call), 3),
                   verdict_over_subset={str(L): round(med(dev[L]) / subset_ms, 3) if subset_ms
                                        else None for L in LEVELS},
                   verdict_gbps={str(L): round(nbytes / (med(dev[L]) * 1e-3) / 1e9, 1)
                                 if med(dev[L]) else None for L in LEVELS},
                   l1_equals_allow_andnot_deny=same,
                   pairs=a.pairs, matched_pairs=int((pv.verdict > 0).sum()),
                   denied_pairs=int((pv.verdict == 2).sum()),
                   pair_verdicts_device_ms=round(med(pv_dev), 4),
                   pair_verdicts_call_ms=round(med(pv_call), 3),
                   pair_ports_device_ms=round(med(pp_dev), 4),
                   pair_ports_call_ms=round(med(pp_call), 3))
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        assert same, "verdict_matrix at L = 1 differs from subset(allows) & ~subset(denies)"
        eng.close()


if __name__ == "__main__":
    main()
