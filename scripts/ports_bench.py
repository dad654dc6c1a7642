"""kano_policy_subset / kano_pair_masks' time on a BASELINE config, next to the
build's own matrix write, to pair_cover and to today's way to a port's matrix.

Every policy of the config gets one of 8 (protocol, port) keys by its index;
one in ten is open on any port.  Per config one JSON line, appended to --out:
  subset_device_ms   kano_policy_subset_time for one slot's matrix (the context
                     is created with KANO_TUNE=timing=1): the fills, the class
                     rows, their expansion and the write of every held row
  rows_device_ms     the same context's own k_rows write (kano_rows_timing)
  write_fraction     the bytes of the matrix over subset_device_ms as a
                     fraction of the same bytes over rows_device_ms
  subset_call_ms     a host clock around port_matrix (the destination's
                     creation and allocation included)
  pair_ports_*       pair_ports for --pairs random pairs: device time
                     (kano_pair_masks_time) and call time, next to
  pair_cover_*       pair_cover on the same pairs (kano_pair_policies_time)
  rebuild_wall_ms    today's way: build_matrix over the host-filtered policy
                     list (interning, upload, build), its rows checked against
                     port_matrix's by digest
No pass mark.

    python scripts/ports_bench.py [--configs C2,C3] [--pairs 1000000] [--reps 5]
                                  [--out profiles/ports_bench.jsonl]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--pairs", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ports_bench.jsonl"))
    a = ap.parse_args()
    import numpy as np
    from kano import algorithm as alg
    from kano import model
    from kano.ports import port_table
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

    def protocol(p):
        return None if p % 10 == 9 else model.PolicyProtocol(["TCP", str(8000 + p % 8)])

    for config in a.configs.split(","):
        obj = make_config(config).to_json_obj()
        cs, ps = objects_from_json(obj, model)
        for p, pol in enumerate(ps):
            pol.protocol = protocol(p)
        note(f"{config}: {len(cs)} pods, {len(ps)} policies")
        m = model.ReachabilityMatrix.build_matrix(cs, ps)
        eng = m.engine
        info = eng.info()
        n, W = info["N"], info["W"]
        rows = eng.rows_timing()
        t = port_table(ps)
        key = t.keys[0]
        kept = np.flatnonzero(t.carries([0]))
        rng = np.random.default_rng(a.seed)
        pairs = rng.integers(0, n, size=(a.pairs, 2)).astype(np.int32)

        alg.port_matrix(m, key).engine.close()           # (first call: the warm-up)
        dev, call, sub_info = [], [], None
        for _ in range(a.reps):
            ms, pm = timed(lambda: alg.port_matrix(m, key))
            call.append(ms)
            dev.append(eng.subset_time())
            sub_info = pm.subset_info
            digest = pm.engine.rows_digest(0, n)
            pm.engine.close()
        subset_ms, subset_call = statistics.median(dev), statistics.median(call)
        note(f"{config} subset: {subset_ms:.3f} ms device, {subset_call:.3f} ms call")

        pp_dev, pp_call, pc_dev, pc_call = [], [], [], []
        for _ in range(a.reps):
            ms, masks = timed(lambda: alg.pair_ports(m, pairs))
            pp_call.append(ms)
            pp_dev.append(eng.pair_masks_time())
            ms, cover = timed(lambda: alg.pair_cover(m, pairs))
            pc_call.append(ms)
            pc_dev.append(eng.pair_policies_time())
        assert np.array_equal(masks.masks.any(axis=1), cover > 0)

        # today's way: the policy list filtered on the host and built again
        cs2, ps2 = objects_from_json(obj, model)
        wall, m2 = timed(lambda: model.ReachabilityMatrix.build_matrix(
            cs2, [ps2[p] for p in kept.tolist()]))
        same = bool(np.array_equal(m2.engine.rows_digest(0, n), digest))
        m2.engine.close()

        nbytes = 8 * info["N"] * ((W + 15) // 16 * 16)
        rows_ms = rows["sum_ms"] / max(rows["launches"], 1)
        rec = dict(config=config, n=n, W=W, P=len(ps), keys=t.K, kept_policies=int(kept.shape[0]),
                   subset_info=sub_info, tune=base_tune, matrix_bytes=nbytes,
                   subset_device_ms=round(subset_ms, 4), subset_call_ms=round(subset_call, 3),
                   rows_device_ms=round(rows_ms, 4),
                   subset_gbps=round(nbytes / (subset_ms * 1e-3) / 1e9, 1) if subset_ms else None,
                   write_fraction=round(rows_ms / subset_ms, 3) if subset_ms else None,
                   pairs=a.pairs, open_pairs=int((cover > 0).sum()),
                   pair_ports_device_ms=round(statistics.median(pp_dev), 4),
                   pair_ports_call_ms=round(statistics.median(pp_call), 3),
                   pair_cover_device_ms=round(statistics.median(pc_dev), 4),
                   pair_cover_call_ms=round(statistics.median(pc_call), 3),
                   rebuild_wall_ms=round(wall, 3), rebuild_rows_equal=same)
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        assert same, "the rebuilt matrix differs from port_matrix"
        eng.close()


if __name__ == "__main__":
    main()
