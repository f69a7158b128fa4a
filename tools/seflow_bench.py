"""What the self-supervised loss costs on the GPU, measured: usage  python tools/seflow_bench.py [--batch 16] [--points 80000]
[--grid 512] [--reps 20] [--out profiles/seflow_step.json]

At the configs[2] shape (B = 16, 80 000 rows per cloud, 512 x 512) it times with device events, after a warm-up of every shape,

  * each of the six searches of losses.seflow_loss -- the grid build (df_nn_grid_build) and the search (df_chamfer_nn) separately --
    on the clouds of a real forward (the compacted points and the model's flow), with the share of queries that had to look past
    the 3 x 3 cells around their own, and next to each the arithmetic floor of the all-pairs form the grid search replaces:
    sum_b Nq_b Nr_b x 4 lane-operations (three FMA-class operations and one min per pair) / 78.6e12 per second (157.3 TFLOP/s
    vector fp32 = 78.6e12 FMA/s).  A search must be faster than that floor;
  * the backward: df_chamfer_bwd's gather half (p -> pc1) and its segmented scatter half (pc1 -> p);
  * one whole Trainer.step with seflowLoss next to one with deflowLoss on the same batches, alternating.

A measuring tool, not a bench.py leg; needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import deflow_amd
from deflow_amd import chamfer
from deflow_amd.optim import Trainer
from deflow_amd.synth import synth_batch, synth_cluster_labels

FMA_PER_S = 78.6e12


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "seflow_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/seflow_bench.py measures on the GPU"
    dev = torch.device("cuda")
    B, N, H = a.batch, a.points, a.grid
    half = 0.1 * H
    rng = [-half, -half, -3, half, half, 3]
    torch.manual_seed(0)

    def model():
        return deflow_amd.DeFlow(voxel_size=[0.2, 0.2, 6], point_cloud_range=rng, grid_feature_size=[H, H]).to(dev).train()

    batches = []
    for i in range(2):
        b = synth_batch(B, N, seed=20240116 + i * B, grid_hw=(H, H), device=dev)
        b["pc0_dynamic"], b["pc1_dynamic"] = synth_cluster_labels(b)
        batches.append(b)

    # ---- the searches, on the clouds of a real forward -----------------------------------------------------------------------------
    m = model()
    with torch.no_grad():
        st = m.forward_padded(batches[0])
    p0, p1 = st["p0"], st["p1"]
    pc0, pc1, c0, c1 = p0.points_c.contiguous(), p1.points_c.contiguous(), p0.counts, p1.counts
    g = lambda l, ix: torch.gather(l.long(), 1, ix.clamp(0, l.shape[1] - 1))
    valid0 = torch.arange(pc0.shape[1], device=dev)[None, :] < c0[:, None]
    valid1 = torch.arange(pc1.shape[1], device=dev)[None, :] < c1[:, None]
    l0 = torch.where(valid0, g(batches[0]["pc0_dynamic"], p0.idx_c), 0).to(torch.int32).contiguous()
    l1 = torch.where(valid1, g(batches[0]["pc1_dynamic"], p1.idx_c), 0).to(torch.int32).contiguous()
    p = torch.where(valid0[..., None], pc0 + st["flow"], torch.full_like(pc0, float("nan"))).contiguous()
    n0, n1 = c0.double(), c1.double()
    d0, d1 = (l0 > 0).sum(1).double(), (l1 > 0).sum(1).double()
    grid = chamfer.RowGrid(B, (rng[0], rng[1], rng[3], rng[4]), chamfer.CELL, dev)
    T = 4.0
    searches = [  # name, query, qcount, qlabel, ref, rcount, rlabel, max_dist2, participating rows per sample (query, ref)
        ("p->pc1", p, c0, None, pc1, c1, None, T, n0, n1), ("pc1->p", pc1, c1, None, p, c0, None, T, n1, n0),
        ("p[dyn]->pc1[dyn]", p, c0, l0, pc1, c1, l1, T, d0, d1), ("pc1[dyn]->p[dyn]", pc1, c1, l1, p, c0, l0, T, d1, d0),
        ("pc0->pc1 raw, unbounded", pc0, c0, None, pc1, c1, None, float("inf"), n0, n1),
        ("pc1->pc0 raw, unbounded", pc1, c1, None, pc0, c0, None, float("inf"), n1, n0)]
    report = {"shape": {"batch": B, "points_per_cloud": N, "grid": [H, H], "valid_rows_pc0": c0.tolist(), "valid_rows_pc1": c1.tolist(),
                        "dynamic_rows_pc0": (l0 > 0).sum(1).tolist(), "dynamic_rows_pc1": (l1 > 0).sum(1).tolist()},
              "grid_cells_per_side": grid.G, "cell_m": chamfer.CELL, "device": torch.cuda.get_device_name(0), "searches": []}
    keep = {}
    for name, q, qc, ql, r, rc, rl, md, nq, nr in searches:
        far = torch.zeros(1, dtype=torch.int32, device=dev)
        filed = grid.file(r, rc, rl)
        t_build = timed(lambda: grid.file(r, rc, rl), a.reps)
        t_search = timed(lambda: grid.nn(q, qc, ql, filed, md), a.reps)
        _, idx = grid.nn(q, qc, ql, filed, md, far)
        torch.cuda.synchronize()
        floor_ms = float((nq * nr).sum()) * 4 / FMA_PER_S * 1e3
        row = {"search": name, "grid_build_ms": round(t_build, 4), "search_ms": round(t_search, 4),
               "all_pairs_floor_ms": round(floor_ms, 4), "below_floor": bool(t_search < floor_ms),
               "queries": int(nq.sum()), "far_share": round(int(far) / max(int(nq.sum()), 1), 4),
               "with_neighbour": int((idx >= 0).sum())}
        print(json.dumps(row), flush=True)
        report["searches"].append(row)
        keep[name] = (q, r, idx.clone())

    # ---- the backward -------------------------------------------------------------------------------------------------------------
    q, r, idx = keep["p->pc1"]
    gq = torch.rand(B, q.shape[1], device=dev)
    dq = torch.zeros_like(q)
    t_gather = timed(lambda: chamfer.chamfer_bwd(q, r, idx, gq, dq, None), a.reps)
    q, r, idx = keep["pc1->p"]
    gr = torch.rand(B, q.shape[1], device=dev)
    dr = torch.zeros_like(r)
    t_scatter = timed(lambda: chamfer.chamfer_bwd(q, r, idx, gr, None, dr), a.reps)
    report["backward"] = {"gather_p_to_pc1_ms": round(t_gather, 4), "segmented_scatter_pc1_to_p_ms": round(t_scatter, 4)}
    print(json.dumps(report["backward"]), flush=True)
    del m, st, keep

    # ---- the whole step, seflowLoss next to deflowLoss, alternating --------------------------------------------------------------------
    torch.manual_seed(0)
    ts = Trainer(model(), lr=2e-4, loss_fn="seflowLoss")
    td = Trainer(model(), lr=2e-4, loss_fn="deflowLoss")
    for t in (ts, td):
        for b in batches:
            t.step(b)
    torch.cuda.synchronize()
    times = {"seflowLoss": [], "deflowLoss": []}
    for i in range(max(4, a.reps // 2)):
        for name, t in (("seflowLoss", ts), ("deflowLoss", td)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t.step(batches[i % 2])
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    report["step"] = {"seflowLoss_ms": round(med["seflowLoss"], 3), "deflowLoss_ms": round(med["deflowLoss"], 3),
                      "added_ms": round(med["seflowLoss"] - med["deflowLoss"], 3),
                      "seflowLoss_ms_min_max": [round(min(times["seflowLoss"]), 3), round(max(times["seflowLoss"]), 3)],
                      "deflowLoss_ms_min_max": [round(min(times["deflowLoss"]), 3), round(max(times["deflowLoss"]), 3)],
                      "steps_timed_each": len(times["seflowLoss"]), "last_loss_terms_mean": ts.last_loss_terms.mean(0).tolist(),
                      "label_overflow": int(ts.last_label_overflow)}
    print(json.dumps(report["step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
