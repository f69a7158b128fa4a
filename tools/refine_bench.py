"""Measure the per-cluster rigid snap (deflow_amd/refine.py) and write profiles/refine_flow.json.  The input is
tools/fastnsf_bench.py's -- one pair of 80 000 + 80 000 rows (B = 1) in the default range -- with planted clusters: 100 box-shaped bodies
of 100 to 1000 rows take the place of as many of the uniformly random rows, each body moves by its own yaw and translation, the input
flow is that motion plus N(0, 0.05) noise with a quarter of every body's rows set to zero (the network's typical failure), and the second
sweep holds the moved bodies.  The uniformly random rows are too sparse to cluster and keep their flow.

`rigid_refine` as a whole and its stages -- the DBSCAN labels, df_rigid_segments, df_refine_fit, the check (provisional apply, one grid
build, two nearest-neighbour searches, df_refine_score) and df_refine_apply -- as medians of 10 by device events; the three kernels of
csrc/refine.hip also as 20 calls replayed in one HIP graph, per call, since a single eager call of a kernel of tens of microseconds is
timed together with its launch gap.  No thresholds and no claim: the numbers are written down with the box they came from.

    python tools/refine_bench.py [--rows 80000] [--bodies 100] [--out profiles/refine_flow.json]"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deflow_amd import refine  # noqa: E402
from deflow_amd.cluster import dbscan  # noqa: E402
from floxels_bench import graph_ms  # noqa: E402
from nsfp_bench import median_ms  # noqa: E402

RANGE = (-51.2, -51.2, -3.0, 51.2, 51.2, 3.0)


def planted(N: int, bodies: int, gen: torch.Generator):
    """x, flow, pc1 [1,N,3] on the host and the planted rows' count"""
    scale = torch.tensor([50.0, 50.0, 2.0])
    x = (torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale
    p1 = (torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale + torch.tensor([0.4, 0.1, 0.0])
    flow = 0.05 * torch.randn(1, N, 3, generator=gen)
    side = int(math.ceil(math.sqrt(bodies)))
    at = 0
    for i in range(bodies):
        n = int(torch.randint(100, 1001, (1,), generator=gen))
        if at + n > N:
            break
        centre = torch.tensor([-45.0 + 90.0 * (i % side) / max(side - 1, 1), -45.0 + 90.0 * (i // side) / max(side - 1, 1), 0.0])
        pts = (torch.rand(n, 3, generator=gen) * 2 - 1) * torch.tensor([2.2, 0.9, 0.8]) + centre
        yaw = float(torch.rand(1, generator=gen)) * 0.2 - 0.1
        t = torch.cat([torch.rand(2, generator=gen) * 3.0 - 1.5, torch.zeros(1)])
        c, s = math.cos(yaw), math.sin(yaw)
        rel = pts - centre
        moved = torch.stack([c * rel[:, 0] - s * rel[:, 1], s * rel[:, 0] + c * rel[:, 1], rel[:, 2]], dim=1) + centre + t
        f = moved - pts + 0.05 * torch.randn(n, 3, generator=gen)
        f[torch.randperm(n, generator=gen)[: n // 4]] = 0.0
        x[0, at:at + n], flow[0, at:at + n], p1[0, at:at + n] = pts, f, moved
        at += n
    return x, flow, p1, at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--bodies", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "refine_flow.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    N = a.rows
    x, flow, p1, n_planted = (t.to(dev) if isinstance(t, torch.Tensor) else t for t in planted(N, a.bodies, torch.Generator().manual_seed(0)))
    cnt = torch.full((1,), N, dtype=torch.int32, device=dev)
    D = refine.DEFAULTS
    K = refine.kcap(N, D["min_cluster_size"])
    rng = (RANGE[0], RANGE[1], RANGE[3], RANGE[4])
    res = {"shape": {"batch": 1, "rows_pc0": N, "rows_pc1": N, "planted_bodies": a.bodies, "planted_rows": n_planted, "slots": K,
                     "iters": D["iters"]},
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": "device events, median of 10; ms_graph: 20 calls replayed as one HIP graph, per call (ms: one eager call, with its "
                     "launch gap and the wrapper's allocations)"}

    labels_fn = lambda: dbscan(x, cnt, eps=D["eps"], min_points=D["min_points"], min_cluster_size=D["min_cluster_size"], grid_range=rng)[0]
    labels = labels_fn()
    lab, seg_off, seg_rows = refine.segments(labels, cnt, K)
    fit_kw = {k: D[k] for k in ("min_rows", "max_cluster_points", "iters", "delta", "inlier_dist", "min_inlier_frac", "max_yaw", "max_disp",
                                "static_disp", "static_yaw")}
    fit = lambda: refine.refine_fit(x, cnt, flow, seg_off, seg_rows, **fit_kw)
    table, anchor = fit()
    apply = lambda: refine.refine_apply(x, cnt, flow, lab, table, anchor)
    prov, _ = apply()
    nn = lambda: refine._nn_d2([x + flow, x + prov], cnt, p1, cnt, D["check_trunc"] ** 2, rng)
    d2b, d2a = nn()
    score = lambda: refine.refine_score(x, cnt, flow, cnt, seg_off, seg_rows, d2b, d2a, table.clone())

    def check():
        pr, _ = apply()
        b, c = refine._nn_d2([x + flow, x + pr], cnt, p1, cnt, D["check_trunc"] ** 2, rng)
        return refine.refine_score(x, cnt, flow, cnt, seg_off, seg_rows, b, c, table.clone())

    whole = lambda: refine.rigid_refine(x, cnt, flow, p1, cnt, grid_range=rng)
    res["rigid_refine_ms"] = round(median_ms(whole), 4)
    res["rigid_refine_check_false_ms"] = round(median_ms(lambda: refine.rigid_refine(x, cnt, flow, p1, cnt, grid_range=rng, check=False)), 4)
    res["stages_ms"] = {"dbscan_labels": round(median_ms(labels_fn), 4),
                        "segments": round(median_ms(lambda: refine.segments(labels, cnt, K)), 4),
                        "df_refine_fit": round(median_ms(fit), 4),
                        "check (apply, grid build, 2 searches, score)": round(median_ms(check), 4),
                        "grid build and 2 searches": round(median_ms(nn), 4),
                        "df_refine_score": round(median_ms(score), 4),
                        "df_refine_apply": round(median_ms(apply), 4)}
    res["kernels_ms_graph"] = {"df_refine_fit": round(graph_ms(fit), 4), "df_refine_score": round(graph_ms(score), 4),
                               "df_refine_apply": round(graph_ms(apply), 4)}
    # what the run did (read back after the timing)
    out, info = whole()
    st = info["table"][0, :, 7].long()
    rows_used = info["table"][0, :, 6]
    res["slots_by_status"] = {refine.STATUS_NAMES[s]: int((st == s).sum()) for s in sorted(refine.STATUS_NAMES)}
    res["rows_snapped"] = int((info["rigid_id"] > 0).sum())
    res["largest_fitted_cluster_rows"] = int(rows_used[(st != 0) & (st != 3)].max()) if bool(((st != 0) & (st != 3)).any()) else 0
    # per fit pass a row costs its list entry, x and f: 4 + 12 + 12 bytes; 2 (iters + 1) + 2 passes over the rows of the fitted clusters
    fitted = float(rows_used[(st != 0) & (st != 2) & (st != 3)].sum())
    passes = 2 * (D["iters"] + 1) + 2
    res["df_refine_fit_bytes_each_pass_from_memory"] = int(fitted * 28 * passes)
    res["unexamined"] = ("no hardware counters were collected; the re-read rows of a cluster are expected to come from L2, which was not "
                         "checked; the input is synthetic (box-shaped bodies on a lattice of positions, uniformly random rows between them), "
                         "not a real sweep; B > 1 was not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
