"""kubesv's edge relation at scale (kano.k8s): a
synthetic Kubernetes cluster -- pods spread over namespaces (Zipf), apps per
namespace, one NetworkPolicy per (namespace, app) that admits ingress from a
few apps of its namespace and of namespaces with a team label, and sends
egress to a few apps -- timed per stage.  One JSON line per size.

Usage: python scripts/k8s_bench.py [--pods 10000 100000] [--reps 3]
       python scripts/k8s_bench.py --conn ...   (the conformant reading,
       kano.k8s.connectivity, over the same cluster)
       python scripts/k8s_bench.py --conn --admin 50 --baseline ...   (the same
       with 50 generated AdminNetworkPolicies and a default-deny baseline: the
       tiered call's times next to the plain call's of the same run)
       python scripts/k8s_bench.py --conn --pairs 1000000 [--admin 50 --baseline]
       (K8sConnectivity.pair_verdicts' call, kano_k8s_pair_verdicts, on that
       many random pairs: wall and device time, the lane and the wave form
       forced, and beside them the device time of one kano_pair_verdicts on
       each of the two builds -- a call that walks one list per pair)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "kubernetes-verification_amd")]


def cluster(n, seed=0):
    from kano import k8s
    rng = np.random.default_rng(seed)
    nns = max(4, n // 500)
    teams = ["a", "b", "c", "d"]
    nss = [k8s.Namespace(f"ns{i}", {"team": teams[i % 4], **({"env": "prod"} if i % 3 else {})})
           for i in range(nns)]
    z = 1.0 / np.arange(1, nns + 1) ** 1.1
    ns_of = rng.choice(nns, size=n, p=z / z.sum())
    apps_per_ns = 20
    app_of = rng.integers(0, apps_per_ns, size=n)
    tier = rng.integers(0, 3, size=n)
    pods = [k8s.Pod(f"p{i}", f"ns{ns_of[i]}", {"app": f"a{app_of[i]}", "tier": f"t{tier[i]}"})
            for i in range(n)]
    pols = []
    for ns in range(nns):
        for a in range(apps_per_ns):
            if rng.random() < 0.5:
                continue
            ing = [{"podSelector": {"matchLabels": {"app": f"a{int(b)}"}}}
                   for b in rng.choice(apps_per_ns, size=2, replace=False)]
            if rng.random() < 0.2:
                ing.append({"namespaceSelector": {"matchLabels": {"team": teams[ns % 4]}},
                            "podSelector": {"matchLabels": {"tier": "t0"}}})
            egr = [{"podSelector": {"matchLabels": {"app": f"a{int(b)}"}},
                    "namespaceSelector": {"matchLabels": {"team": teams[ns % 4]}}}
                   for b in rng.choice(apps_per_ns, size=2, replace=False)]
            pols.append(k8s.NetworkPolicy(f"np{ns}-{a}", f"ns{ns}", {
                "podSelector": {"matchLabels": {"app": f"a{a}"}},
                "ingress": [{"from": ing}], "egress": [{"to": egr}]}))
    return pods, pols, nss


def admin_policies(K, baseline, nns, seed=1):
    """K AdminNetworkPolicies over cluster()'s labels -- mixed actions,
    namespace and pod subjects, some rules with ports -- and, on request, a
    default-deny BaselineAdminNetworkPolicy."""
    from kano import k8s
    rng = np.random.default_rng(seed)
    teams = ["a", "b", "c", "d"]

    def who():
        r = rng.random()
        if r < 0.4:
            return {"namespaces": {"matchLabels": {"team": teams[int(rng.integers(4))]}}}
        pods = {"podSelector": {"matchLabels": {"app": f"a{int(rng.integers(20))}"}}}
        if r < 0.7:
            pods["namespaceSelector"] = {"matchLabels": {"team": teams[int(rng.integers(4))]}}
        return {"pods": pods}

    def rules(side):
        out = []
        for _ in range(int(rng.integers(1, 4))):
            rule = {"action": ["Allow", "Deny", "Pass"][int(rng.integers(3))],
                    side: [who() for _ in range(int(rng.integers(1, 3)))]}
            if rng.random() < 0.3:
                rule["ports"] = [{"portNumber": {"protocol": "TCP", "port": 80}},
                                 {"portRange": {"protocol": "TCP", "start": 8000, "end": 8100}}][
                                     :int(rng.integers(1, 3))]
            out.append(rule)
        return out

    admin = [k8s.AdminNetworkPolicy(f"anp{q}", {
        "priority": int(rng.integers(0, 1001)), "subject": who(),
        "egress": rules("to"), "ingress": rules("from")}) for q in range(K)]
    base = None
    if baseline:
        base = k8s.BaselineAdminNetworkPolicy("default", {
            "subject": {"namespaces": {}},
            "egress": [{"action": "Allow", "to": [{"namespaces": {"matchLabels": {"team": "a"}}}]},
                       {"action": "Deny", "to": [{"namespaces": {}}]}],
            "ingress": [{"action": "Deny", "from": [{"namespaces": {}}]}]})
    return admin, base


def pair_times(args, n, te, ti, codes, np_level):
    """--pairs: one kano_k8s_pair_verdicts on args.pairs random pairs over the
    builds of the tables te / ti -- as the engine picks the form, then the lane
    and the wave form forced (kpf=1 / 2; KANO_TUNE is read when a context is
    created, so each form gets builds of its own) -- and one kano_pair_verdicts
    on each build for the same pairs (all-allow tiers of one priority; the
    ingress build with the pairs reversed, as the new call reads it).  The
    best device time of args.reps calls each."""
    from kano._engine import DeviceBuild
    Q = args.pairs
    pr = np.random.default_rng(2).integers(0, n, size=(Q, 2), dtype=np.int32)
    rev = np.ascontiguousarray(pr[:, ::-1])
    tune = os.environ.get("KANO_TUNE", "")
    out = {"pairs": Q}
    for form, knob in (("auto", ""), ("lane", "kpf=1"), ("wave", "kpf=2")):
        os.environ["KANO_TUNE"] = ",".join(x for x in (tune, knob) if x)
        eg, ing = DeviceBuild(te, build=False), DeviceBuild(ti, build=False)
        eg.build_classes()
        ing.build_classes()
        wall = dev = None
        for _ in range(args.reps + 1):                     # (the first call warms up)
            t = time.perf_counter()
            r = eg.k8s_pair_verdicts(ing, pr, True, codes[0], np_level[0], codes[1], np_level[1])
            w, d = time.perf_counter() - t, eg.k8s_pair_verdicts_time()
            if _ and (dev is None or d < dev):
                wall, dev = w, d
        out[form] = {"wall_ms": round(wall * 1e3, 3), "device_ms": round(dev, 4),
                     "pairs_per_s": round(Q / (dev * 1e-3)) if dev > 0 else None}
        if form == "auto":
            out["allowed"] = int(r["counts"][0])
            ie, ii = eg.info(), ing.info()
            out["mean_list"] = [round(ie["NNZ_SEL"] / max(1, ie["U"]), 2),
                                round(ii["NNZ_SEL"] / max(1, ii["U"]), 2)]
            # the yardstick: the existing single-build call, one list per pair
            for name, b, q in (("egress", eg, pr), ("ingress", ing, rev)):
                P = b.info()["P"]
                best = None
                if P:
                    z = np.zeros(P, dtype=np.int32)
                    for _ in range(args.reps + 1):
                        b.pair_verdicts(q, z, z.astype(np.uint8))
                        d = b.pair_verdicts_time()
                        best = d if _ and (best is None or d < best) else best
                out[f"pair_verdicts_{name}_device_ms"] = None if best is None else round(best, 4)
        del eg, ing
    os.environ["KANO_TUNE"] = tune
    both = [out[f"pair_verdicts_{k}_device_ms"] or 0.0 for k in ("egress", "ingress")]
    out["yardstick_sum_device_ms"] = round(sum(both), 4)
    for form in ("auto", "lane", "wave"):
        out[form]["ratio_to_yardstick_sum"] = (round(out[form]["device_ms"] / sum(both), 3)
                                               if sum(both) > 0 else None)
    return out


def conn_tiers(args, n, pods, pols, nss, rows):
    """The tiered call (kano_k8s_conn_tiers) over the builds of the same
    cluster with the generated admin and baseline policies compiled in."""
    from kano import k8s
    from kano._engine import DeviceBuild
    from kano._intern import intern
    admin, base = admin_policies(args.admin, args.baseline, len(nss))
    t = time.perf_counter()
    c = k8s.compile_conformant(pods, pols, nss, admin, base)
    t_compile = time.perf_counter() - t
    te, ti = intern(c.containers, c.egress), intern(c.containers, c.ingress)
    code, code_port = c.codes(None), c.codes(("TCP", 8050))   # (drops the port-80-only rules)
    best = None
    for _ in range(args.reps):
        eg, ing = DeviceBuild(te, build=False), DeviceBuild(ti, build=False)
        eg.build_classes()
        ing.build_classes()
        out = DeviceBuild.empty(n, rows=rows)
        out.k8s_conn_tiers_from(eg, ing, True, code_port[0], c.np_level[0], code_port[1],
                                c.np_level[1], args.conn_form)          # a port query first
        dev_port = out.k8s_conn_time()
        t2 = time.perf_counter()
        _, _, info = out.k8s_conn_tiers_from(eg, ing, True, code[0], c.np_level[0], code[1],
                                             c.np_level[1], args.conn_form)
        t3 = time.perf_counter()
        r = (t3 - t2, out.k8s_conn_time(), dev_port)
        best = r if best is None or r[1] < best[1] else best
        ie, ii = eg.info(), ing.info()
        del eg, ing
    kinds = [t[0] for t in c.tiers_egress + c.tiers_ingress]
    pairs = {}
    if args.pairs > 0:
        pairs = {"pair_verdicts": pair_times(args, n, te, ti, code, c.np_level)}
    return {**pairs, "admin_policies": len(admin), "baseline": base is not None,
            "admin_entries": kinds.count("admin"), "baseline_entries": kinds.count("baseline"),
            "admin_levels": list(c.np_level), "admin_priority_ties": c.admin_priority_ties,
            "egress_entries": len(c.egress), "ingress_entries": len(c.ingress),
            "egress_classes": [ie["U"], ie["UA"]], "ingress_classes": [ii["U"], ii["UA"]],
            "host_compile_s": round(t_compile, 3),
            "conn_tiers_ms": round(best[0] * 1e3, 3), "conn_tiers_device_ms": round(best[1], 4),
            "conn_tiers_port_device_ms": round(best[2], 4),
            "egress_isolated": info["egress_isolated"],
            "ingress_isolated": info["ingress_isolated"]}


def usage_times(args, n, pods, pols, nss):
    """--usage: K8sConnectivity.rule_usage on the cluster (with the generated
    admin and baseline policies of --admin / --baseline): its call time, its
    device time and, beside it, kano_k8s_conn_tiers' whole device time on the
    same builds (``conn_tiers_whole_device_ms``: the order and class kernels,
    which walk the same lists, plus the transpose, the expansion and the
    matrix write -- the class step alone is read off a kernel trace, see
    DESIGN.md).  Up to 4000 pods also the route through pair_verdicts over all
    n * n pairs, whose blame must equal rule_usage's."""
    import numpy as np
    from kano import k8s
    admin, base = admin_policies(args.admin, args.baseline, len(nss))
    conn = k8s.connectivity(pods, pols, nss, allow_self=False, admin=admin, baseline=base)
    out = {"conn_tiers_whole_device_ms": round(conn.allowed._engine.k8s_conn_time(), 4)}
    best = None
    for _ in range(args.reps):
        t = time.perf_counter()
        u = conn.rule_usage()
        r = (time.perf_counter() - t, conn.egress.engine.k8s_rule_usage_time())
        best = r if best is None or r[1] < best[1] else best
    out.update(rule_usage_ms=round(best[0] * 1e3, 3), rule_usage_device_ms=round(best[1], 4),
               egress_entries=len(conn.origin_egress), ingress_entries=len(conn.origin_ingress),
               dead_rules=len(u.dead_rules()), redundant_rules=len(u.redundant_rules()),
               counts=u.counts)
    if n <= 4000:
        pr = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1)
        pr = pr.reshape(-1, 2).astype(np.int32)
        t = time.perf_counter()
        v = conn.pair_verdicts(pr)
        blames = {d: v.blame(d, False) for d in ("egress", "ingress")}
        out["all_pairs_route_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        out["all_pairs_device_ms"] = round(conn.egress.engine.k8s_pair_verdicts_time(), 4)
        for d, b in blames.items():
            assert b == u.blame(d, False), f"{d}: rule_usage and pair_verdicts disagree"
        out["blame_equal"] = True
    return out


HBM_SPEC = 8.0e12   # MI355X HBM3E, bytes per second


def conn(args):
    """--conn: the same cluster read conformantly (kano.k8s.connectivity's
    steps): the two class builds, then kano_k8s_conn -- its wall time, its
    device time (kano_k8s_conn_time, KANO_TUNE timing=1) and the write's
    fraction of the HBM spec for the matrix's n * n / 8 bytes."""
    os.environ["KANO_TUNE"] = ",".join(
        x for x in (os.environ.get("KANO_TUNE", ""), "timing=1") if x)
    import torch  # noqa: F401  (HIP runtime first, as the bench does)
    from kano import k8s
    from kano._engine import DeviceBuild
    from kano._intern import intern
    for n in args.pods:
        pods, pols, nss = cluster(n)
        t = time.perf_counter()
        c = k8s.compile_conformant(pods, pols, nss)
        t_compile = time.perf_counter() - t
        t = time.perf_counter()
        te, ti = intern(c.containers, c.egress), intern(c.containers, c.ingress)
        t_intern = time.perf_counter() - t
        keep = c.keep(("TCP", 80))
        rows = (0, n // args.ranks) if args.ranks > 1 else None
        best = None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            eg, ing = DeviceBuild(te, build=False), DeviceBuild(ti, build=False)
            tu = time.perf_counter()
            eg.build_classes()
            ing.build_classes()
            t1 = time.perf_counter()
            out = DeviceBuild.empty(n, rows=rows)
            out.k8s_conn_from(eg, ing, True, *keep, form=args.conn_form)   # a port query first
            dev_port = out.k8s_conn_time()
            t2 = time.perf_counter()
            info = out.k8s_conn_from(eg, ing, True, form=args.conn_form)
            t3 = time.perf_counter()
            dev = out.k8s_conn_time()
            r = (t1 - t0, t3 - t2, tu - t0, dev, dev_port)
            best = r if best is None or r[3] < best[3] else best
            ie, ii = eg.info(), ing.info()
            del eg, ing
        W = (n + 63) // 64
        nbytes = n * n / 8 / args.ranks
        from kano import algorithm as alg
        em = k8s._wrap(out, n)
        tiers = {}
        if args.pairs > 0:
            tiers["pair_verdicts"] = pair_times(args, n, te, ti, c.codes(None), c.np_level)
        if args.admin > 0 or args.baseline:
            tiers["tiers"] = conn_tiers(args, n, pods, pols, nss, rows)
        if args.usage:
            tiers["rule_usage"] = usage_times(args, n, pods, pols, nss)
        print(json.dumps({
            "workload": "k8s.connectivity (conformant reading), synthetic K8s cluster",
            "form": args.conn_form,
            "pods": n, "namespaces": len(nss), "policies": len(pols),
            "egress_entries": len(c.egress), "ingress_entries": len(c.ingress),
            "egress_classes": [ie["U"], ie["UA"]], "ingress_classes": [ii["U"], ii["UA"]],
            "host_compile_s": round(t_compile, 3), "host_intern_s": round(t_intern, 3),
            "builds_ms": round(best[0] * 1e3, 3), "of_which_upload_ms": round(best[2] * 1e3, 3),
            "conn_ms": round(best[1] * 1e3, 3), "conn_device_ms": round(best[3], 4),
            "conn_port_device_ms": round(best[4], 4),
            "write_fraction_of_hbm_spec": round(nbytes / (best[3] * 1e-3) / HBM_SPEC, 4)
            if best[3] > 0 else None,
            "egress_isolated": info["egress_isolated"],
            "ingress_isolated": info["ingress_isolated"],
            "matrix_bytes": 8 * n * W, "ranks": args.ranks, "rows": n // args.ranks,
            "all_isolated": len(alg.all_isolated(em)) if args.ranks == 1 else None, **tiers}),
            flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conn", action="store_true",
                    help="the conformant reading (kano.k8s.connectivity) instead of kubesv's edge")
    ap.add_argument("--conn-form", default="auto", choices=["auto", "direct", "stream"],
                    help="--conn: how kano_k8s_conn writes the rows")
    ap.add_argument("--admin", type=int, default=0,
                    help="--conn: also time kano_k8s_conn_tiers with this many generated "
                         "AdminNetworkPolicies")
    ap.add_argument("--baseline", action="store_true",
                    help="--conn: ... and a default-deny BaselineAdminNetworkPolicy")
    ap.add_argument("--pairs", type=int, default=0,
                    help="--conn: also time K8sConnectivity.pair_verdicts' call on this many "
                         "random pairs (with --admin / --baseline: over the tiered builds too)")
    ap.add_argument("--usage", action="store_true",
                    help="--conn: also time K8sConnectivity.rule_usage (with --admin / --baseline: "
                         "over the tiered cluster); up to 4000 pods against the all-pairs route")
    ap.add_argument("--pods", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--form", default="classes", choices=["classes", "pods"])
    ap.add_argument("--inplace", type=int, default=-1,
                    help="1: build the destination from the egress policies (the self term), "
                         "0: expand the self term, -1: as kano.k8s.build (expand)")
    ap.add_argument("--ranks", type=int, default=1,
                    help="time rank 0's row shard of an N-rank split (the edge rows [0, n/N))")
    args = ap.parse_args()
    if args.conn:
        return conn(args)
    import torch  # noqa: F401  (HIP runtime first, as the bench does)
    from kano import k8s
    from kano._engine import DeviceBuild
    from kano._intern import intern
    for n in args.pods:
        pods, pols, nss = cluster(n)
        t = time.perf_counter()
        cs, ing, egr, _ = k8s.compile_policies(pods, pols, nss)
        t_compile = time.perf_counter() - t
        t = time.perf_counter()
        ti, te = intern(cs, ing), intern(cs, egr)
        t_intern = time.perf_counter() - t
        best = None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            in_t = DeviceBuild(ti, build=False)
            eg_t = DeviceBuild(te, build=False)
            tu = time.perf_counter()
            in_t.build_classes()      # Mc and classes only (kano.k8s.build's operands)
            eg_t.build_classes()
            if args.form == "pods":   # the pod-level product reads both matrices
                in_t.rows(0, 1)
                eg_t.rows(0, 1)
            t1 = time.perf_counter()
            rows = (0, n // args.ranks) if args.ranks > 1 else None
            inplace = args.inplace if args.inplace >= 0 else 0
            if args.form == "classes" and inplace:
                # as kano.k8s.build: the destination is the egress build of the
                # rows (its matrix write is the self term); timed with the edge
                t2 = time.perf_counter()
                out = DeviceBuild(te, rows=rows)
                added = out.k8s_edge_from(in_t, eg_t, True, False, dst_is_egress=True)
            else:
                out = DeviceBuild.empty(n, rows=rows)
                t2 = time.perf_counter()
                added = out.k8s_edge_from(in_t, eg_t, True, False, pods=args.form == "pods")
            t3 = time.perf_counter()
            r = (t1 - t0, t3 - t2, tu - t0)
            best = r if best is None or r[0] + r[1] < best[0] + best[1] else best
            del in_t, eg_t
        W = (n + 63) // 64
        # edge density from the matrix itself
        from kano import algorithm as alg
        from kano.k8s import _wrap
        em = _wrap(out, n)
        iso = len(alg.all_isolated(em)) if args.ranks == 1 else None
        print(json.dumps({
            "workload": "kubesv edge relation (kano.k8s), synthetic K8s cluster",
            "form": args.form + ("+inplace" if args.form == "classes" and inplace else ""),
            "pods": n, "namespaces": len(nss), "policies": len(pols),
            "ingress_peers": len(ing), "egress_peers": len(egr),
            "host_compile_s": round(t_compile, 3), "host_intern_s": round(t_intern, 3),
            "builds_ms": round(best[0] * 1e3, 3), "of_which_upload_ms": round(best[2] * 1e3, 3), "edge_ms": round(best[1] * 1e3, 3),
            "product_bits": added, "edge_matrix_bytes": 8 * n * W,
            "ranks": args.ranks, "rows": n // args.ranks, "all_isolated": iso,
            "all_reachable": len(alg.all_reachable(em)) if args.ranks == 1 else None}),
            flush=True)


if __name__ == "__main__":
    main()
