"""Measure model=mbnsf on tools/fastnsf_bench.py's input -- one pair of 80 000 + 80 000 synthetic rows (B = 1) in the default range, depth 7
-- and write profiles/mbnsf_flow.json: one df_iso_plan (with the ordered lists it needs), one df_iso_pairs alone, ms per whole iteration,
eager and as a replayed HIP graph, and -- in the same session on the same box, for comparison -- model=fastnsf's iteration.  Medians of
10, by device events.  No thresholds: the numbers are written down with the box they came from.

The rows are uniformly random, so DBSCAN finds next to no cluster in them (its time and its count of pair instances are recorded all the
same); the term is measured on GIVEN labels instead: every row in one of rows / 100 clusters, assigned at random, so that every row has
its 2 P partners and they lie anywhere in the sweep (no locality for the gather).

    python tools/mbnsf_bench.py [--rows 80000] [--depth 7] [--out profiles/mbnsf_flow.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deflow_amd import fastnsf, mbnsf, nsfp, pairopt  # noqa: E402
from deflow_amd.cluster import dbscan  # noqa: E402
from nsfp_bench import median_ms  # noqa: E402

RANGE = (-51.2, -51.2, -3.0, 51.2, 51.2, 3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mbnsf_flow.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    N, depth = a.rows, a.depth
    gen = torch.Generator().manual_seed(0)
    scale = torch.tensor([50.0, 50.0, 2.0])
    p0 = ((torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale).to(dev)
    p1 = ((torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale + torch.tensor([0.4, 0.1, 0.0])).to(dev)
    cnt = torch.full((1,), N, dtype=torch.int32, device=dev)
    D = mbnsf.DEFAULTS
    P, cap, delta = D["rigid_pairs"], D["max_cluster_points"], D["rigid_delta"]
    K = mbnsf.kcap(N, D["min_cluster_size"])
    clusters = max(N // 100, 1)
    labels = (torch.randint(0, clusters, (1, N), generator=gen) + 1).to(torch.int32).to(dev)
    res = {"shape": {"batch": 1, "rows_pc0": N, "rows_pc1": N, "depth": depth, "width": nsfp.WIDTH, "rigid_pairs": P, "rigid_delta": delta,
                     "kcap": K, "given_clusters": clusters},
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "method": "device events, median of 10"}

    cl_kw = dict(eps=D["eps"], min_points=D["min_points"], min_cluster_size=D["min_cluster_size"], grid_range=(RANGE[0], RANGE[1], RANGE[3], RANGE[4]))
    own, _ = dbscan(p0, cnt, **cl_kw)
    res["dbscan"] = {"ms": round(median_ms(lambda: dbscan(p0, cnt, **cl_kw)), 4), "clusters": int(own.max()),
                     "pair_instances": int(mbnsf.iso_plan(p0, cnt, own, pairs=P, max_cluster_points=cap, kcap=K)[2])}
    plan = lambda: mbnsf.iso_plan(p0, cnt, labels, pairs=P, max_cluster_points=cap, kcap=K)
    nbr, r0, m = plan()
    w = p0 + 0.1 * torch.randn(1, N, 3, generator=gen).to(dev)
    ms_pairs = median_ms(lambda: mbnsf.iso_pairs(w, nbr, r0, delta=delta))
    # per row: 2 P x (4 + 4) bytes of table, 12 bytes of w, 2 P gathered partner rows of 12 bytes, 4 + 12 bytes of outputs
    row_bytes = 2 * P * 8 + 12 + 2 * P * 12 + 16
    res["iso_plan"] = {"ms": round(median_ms(plan), 4), "pair_instances": int(m), "note": "labels masked and padded in torch, df_rigid_segments, df_iso_plan"}
    res["iso_pairs"] = {"ms": round(ms_pairs, 4), "rows": N, "bytes_per_row_without_sector_overfetch": row_bytes,
                        "gb_per_s": round(N * row_bytes / ms_pairs / 1e6, 1)}

    def loop(opt, iters, graph, **kw):
        return lambda: opt(p0, cnt, p1, cnt, grid_range=RANGE, depth=depth, iters=iters, check_every=0, graph=graph, **kw)

    lo, hi = 3, 13
    for model, opt, kw in (("mbnsf", mbnsf.mbnsf_optimize, {"labels": labels}), ("fastnsf", fastnsf.fastnsf_optimize, {})):
        out = {}
        for name, graph in (("eager", False), ("graph", True)):
            t_lo, t_hi = median_ms(loop(opt, lo, graph, **kw)), median_ms(loop(opt, hi, graph, **kw))
            out[f"ms_per_iteration_{name}"] = round((t_hi - t_lo) / (hi - lo), 4)
            out[f"ms_{name}_{lo}_iterations"], out[f"ms_{name}_{hi}_iterations"] = round(t_lo, 3), round(t_hi, 3)
        res[model] = out
    res["mbnsf"]["note"] = (f"the {lo}- and {hi}-iteration calls both include one dt_build and one iso_plan on the given labels; the "
                            "difference does not")
    v = mbnsf.iso_pairs(w, nbr, r0, delta=delta)[0]
    res["mbnsf"]["split_ms"] = {"iso_pairs": round(ms_pairs, 4),
                                "iso reduction": round(median_ms(lambda: pairopt.sample_sum(v)), 4)}
    res["unexamined"] = ("no hardware counters were collected: how much of the partner gather hits L2 is not examined; the given clusters "
                         "are random sets of rows, a real cluster's rows lie closer together in memory")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
