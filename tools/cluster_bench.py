"""What the online cluster labels cost on the GPU, measured: usage  python tools/cluster_bench.py [--batch 16] [--points 80000]
[--grid 512] [--eps 0.7] [--reps 20] [--out profiles/cluster_step.json]

At the configs[2] shape (B = 16, 80 000 rows per cloud, 512 x 512; ~70 000 rows in range) it times with device events, after a warm-up,

  * the stages of csrc/cluster.hip on the compact pc0 of a real forward: the grid build at the clustering's cell, df_dbscan_core,
    df_dbscan_link and df_dbscan_finish (the later stages as differences of cumulative sequences: a link pass repeated on a finished
    forest would be a different, cheaper pass), next to the yardstick timed in the same run: the whole-cloud df_chamfer_nn search
    pc0 -> pc1 and its df_nn_grid_build;
  * cluster.dynamic_cluster_labels as a whole, per cloud;
  * one Trainer.step with seflowLoss and online labels for both clouds next to the same step with those labels supplied in the batch,
    alternating: the difference is the feature's cost per step;
  * one sample on the CPU with sklearn.cluster.DBSCAN, for scale only, when sklearn imports.

A measuring tool, not a bench.py leg; needs the GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import deflow_amd
from deflow_amd import chamfer, cluster
from deflow_amd._lib import call, ptr, stream
from deflow_amd.optim import Trainer
from deflow_amd.synth import synth_batch, synth_cluster_labels


def timed(fn, reps):
    """median of `reps` event-timed calls after three warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return sorted(out)[len(out) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--eps", type=float, default=0.7)
    ap.add_argument("--min-points", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cluster_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/cluster_bench.py measures on the GPU"
    dev = torch.device("cuda")
    B, N, H, eps = a.batch, a.points, a.grid, a.eps
    half = 0.1 * H
    rng = [-half, -half, -3, half, half, 3]
    grid_range = (rng[0], rng[1], rng[3], rng[4])
    torch.manual_seed(0)

    def model():
        return deflow_amd.DeFlow(voxel_size=[0.2, 0.2, 6], point_cloud_range=rng, grid_feature_size=[H, H]).to(dev).train()

    batches = []
    for i in range(2):
        b = synth_batch(B, N, seed=20240116 + i * B, grid_hw=(H, H), device=dev)
        l0, l1 = synth_cluster_labels(b)
        b["pc0_dufo"], b["pc1_dufo"] = l0 > 0, l1 > 0
        batches.append(b)

    m = model()
    with torch.no_grad():
        st = m.forward_padded(batches[0])
    p0, p1 = st["p0"], st["p1"]
    pc0, pc1, c0, c1 = p0.points_c.contiguous(), p1.points_c.contiguous(), p0.counts, p1.counts
    Nc = pc0.shape[1]
    g = lambda l, ix: torch.gather(l.long(), 1, ix.clamp(0, l.shape[1] - 1))
    f0 = g(batches[0]["pc0_dufo"], p0.idx_c).to(torch.int32).contiguous()
    report = {"shape": {"batch": B, "points_per_cloud": N, "grid": [H, H], "valid_rows_pc0": c0.tolist(), "valid_rows_pc1": c1.tolist()},
              "eps": eps, "min_points": a.min_points, "device": torch.cuda.get_device_name(0)}

    # ---- the yardstick: the whole-cloud chamfer search and its grid build ------------------------------------------------------------
    ygrid = chamfer.RowGrid(B, grid_range, chamfer.CELL, dev)
    G = ygrid.G
    filed = ygrid.file(pc1, c1)
    t_ybuild = timed(lambda: ygrid.file(pc1, c1), a.reps)
    t_ysearch = timed(lambda: ygrid.nn(pc0, c0, None, filed, float("inf")), a.reps)
    report["yardstick"] = {"chamfer_grid_build_ms": round(t_ybuild, 4), "chamfer_nn_pc0_to_pc1_ms": round(t_ysearch, 4),
                           "cell_m": chamfer.CELL, "grid_cells_per_side": G}
    print(json.dumps(report["yardstick"]), flush=True)
    del filed

    # ---- the stages ----------------------------------------------------------------------------------------------------------------
    cell = max(cluster.CELL_SLACK * eps, 2 * half / 4096.0)
    grid = chamfer.RowGrid(B, grid_range, cell, dev)
    minx, miny, G = grid.minx, grid.miny, grid.G
    cell_rng, rows = grid.file(pc0, c0)
    ws = torch.empty(call("df_dbscan_ws_bytes", B, Nc), dtype=torch.uint8, device=dev)
    labels = torch.empty(B, Nc, dtype=torch.int32, device=dev)
    ncl = torch.empty(B, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    build = lambda: grid.file(pc0, c0)
    core = lambda: call("df_dbscan_core", ptr(cell_rng), ptr(rows), B, Nc, minx, miny, cell, G, eps, a.min_points, ptr(ws), stream())
    link = lambda: call("df_dbscan_link", ptr(cell_rng), B, Nc, minx, miny, cell, G, eps, ptr(status), ptr(ws), stream())
    fin = lambda: call("df_dbscan_finish", ptr(cell_rng), ptr(f0), B, Nc, minx, miny, cell, G, eps, 20, 0.3, ptr(labels), ptr(ncl),
                       ptr(status), ptr(ws), stream())
    t_build = timed(build, a.reps)
    t_core = timed(core, a.reps)
    t_core_link = timed(lambda: (core(), link()), a.reps)
    t_all = timed(lambda: (core(), link(), fin()), a.reps)
    report["stages_pc0"] = {"grid_build_ms": round(t_build, 4), "core_ms": round(t_core, 4), "link_ms": round(t_core_link - t_core, 4),
                            "finish_ms": round(t_all - t_core_link, 4), "core_link_finish_ms": round(t_all, 4), "cell_m": round(cell, 5),
                            "grid_cells_per_side": G, "core_over_chamfer_nn": round(t_core / t_ysearch, 2),
                            "link_over_chamfer_nn": round((t_core_link - t_core) / t_ysearch, 2),
                            "n_clusters": ncl.tolist(), "labelled_rows": int((labels > 0).sum()), "status": int(status)}
    print(json.dumps(report["stages_pc0"]), flush=True)

    # ---- the op as a whole -----------------------------------------------------------------------------------------------------------
    f1 = g(batches[0]["pc1_dufo"], p1.idx_c).to(torch.int32).contiguous()
    kw = dict(eps=eps, min_points=a.min_points, grid_range=grid_range)
    t_op0 = timed(lambda: cluster.dynamic_cluster_labels(pc0, c0, f0, **kw), a.reps)
    t_op1 = timed(lambda: cluster.dynamic_cluster_labels(pc1, c1, f1, **kw), a.reps)
    everything = cluster.dbscan(pc0, c0, eps=eps, min_points=a.min_points, grid_range=grid_range)
    report["op"] = {"dynamic_cluster_labels_pc0_ms": round(t_op0, 4), "dynamic_cluster_labels_pc1_ms": round(t_op1, 4),
                    "clusters_without_filters_pc0": everything[1].tolist()}
    print(json.dumps(report["op"]), flush=True)

    # ---- one sample on the CPU, for scale --------------------------------------------------------------------------------------------
    try:
        from sklearn.cluster import DBSCAN
        x = pc0[0, : int(c0[0])].double().cpu().numpy()
        t0 = time.perf_counter()
        sk = DBSCAN(eps=eps, min_samples=a.min_points).fit(x)
        report["cpu_one_sample"] = {"sklearn_dbscan_ms": round((time.perf_counter() - t0) * 1e3, 1), "rows": int(x.shape[0]),
                                    "clusters": int(sk.labels_.max()) + 1, "gpu_clusters_without_filters": int(everything[1][0])}
    except ImportError:
        report["cpu_one_sample"] = "sklearn is not available on this machine"
    print(json.dumps(report["cpu_one_sample"]), flush=True)
    del m, st

    # ---- the step: online labels next to supplied labels, alternating ----------------------------------------------------------------
    cl = dict(eps=eps, min_points=a.min_points)
    torch.manual_seed(0)
    t_on = Trainer(model(), lr=2e-4, loss_fn="seflowLoss", cluster_labels=cl)
    t_sup = Trainer(model(), lr=2e-4, loss_fn="seflowLoss")
    supplied = []
    for b in batches:                  # the same labels, scattered back to input rows, as a labelled file would hold them
        with torch.no_grad():
            s = t_sup.model.forward_padded(b)
        sb = {k: v for k, v in b.items() if k not in ("pc0_dufo", "pc1_dufo")}
        for p, src, dst in ((s["p0"], "pc0_dufo", "pc0_dynamic"), (s["p1"], "pc1_dufo", "pc1_dynamic")):
            lab, _, _ = cluster.dynamic_cluster_labels(p.points_c, p.counts, g(b[src], p.idx_c), grid_range=grid_range, **cl)
            valid = torch.arange(lab.shape[1], device=dev)[None, :] < p.counts[:, None]
            full = torch.zeros(b[src].shape, dtype=torch.int64, device=dev)
            bi = torch.arange(B, device=dev)[:, None].expand_as(lab)
            full[bi[valid], p.idx_c[valid]] = lab.long()[valid]
            sb[dst] = full
        supplied.append(sb)
    for _ in range(2):
        for i in range(2):
            t_on.step(batches[i])
            t_sup.step(supplied[i])
    torch.cuda.synchronize()
    times = {"online": [], "supplied": []}
    for i in range(max(4, a.reps // 2)):
        for name, t, bs in (("online", t_on, batches), ("supplied", t_sup, supplied)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t.step(bs[i % 2])
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    report["step"] = {"seflowLoss_online_labels_ms": round(med["online"], 3), "seflowLoss_supplied_labels_ms": round(med["supplied"], 3),
                      "added_ms": round(med["online"] - med["supplied"], 3),
                      "online_ms_min_max": [round(min(times["online"]), 3), round(max(times["online"]), 3)],
                      "supplied_ms_min_max": [round(min(times["supplied"]), 3), round(max(times["supplied"]), 3)],
                      "steps_timed_each": len(times["online"]), "last_loss_terms_mean": t_on.last_loss_terms.mean(0).tolist(),
                      "label_overflow": int(t_on.last_label_overflow), "cluster_status": int(t_on.last_cluster_status)}
    print(json.dumps(report["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
