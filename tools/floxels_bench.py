"""Measure model=floxels on tools/fastnsf_bench.py's input -- one pair of 80 000 + 80 000 uniformly random rows (B = 1) in the default
range -- and write profiles/floxels_flow.json: one df_vox_plan; df_vox_sample, df_vox_scatter and df_vox_smooth alone, each with the bytes
it has to move and its GB/s; ms per whole iteration, eager and as a replayed HIP graph, with the share of it that is torch's elementwise
ops and reductions; and -- in the same session on the same box, for comparison -- model=fastnsf's iteration.  Medians of 10, by device
events.  No thresholds: the numbers are written down with the box they came from.

Uniform rows put about one row in every tenth cell, so the scatter's segments are short.  A second input, 2 000 rows in each of 40 cells,
shows its long segments (one thread walks a node's rows).  Neither input is a real sweep.

    python tools/floxels_bench.py [--rows 80000] [--depth 7] [--out profiles/floxels_flow.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deflow_amd import fastnsf, floxels, pairopt  # noqa: E402
from deflow_amd._lib import call, ptr, stream  # noqa: E402
from nsfp_bench import median_ms  # noqa: E402

RANGE = (-51.2, -51.2, -3.0, 51.2, 51.2, 3.0)
CALLS = 20


def graph_ms(fn):
    """ms per call of fn: CALLS calls captured into one HIP graph, the median of 10 replays by device events over CALLS.  A single eager
    call of a kernel of tens of microseconds is timed together with the gap the host needs to launch it; the replayed graph has none."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(CALLS):
            fn()
    return median_ms(graph.replay) / CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--depth", type=int, default=7, help="of model=fastnsf's net, measured for comparison")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "floxels_flow.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    N = a.rows
    gen = torch.Generator().manual_seed(0)
    scale = torch.tensor([50.0, 50.0, 2.0])
    p0 = ((torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale).to(dev)
    p1 = ((torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale + torch.tensor([0.4, 0.1, 0.0])).to(dev)
    cnt = torch.full((1,), N, dtype=torch.int32, device=dev)
    D = floxels.DEFAULTS
    vorigin, vdims = floxels.vox_grid(RANGE, D["voxel"])
    VX, VY, VZ = vdims
    NV, NC = VX * VY * VZ, (VX - 1) * (VY - 1) * (VZ - 1)
    origin, dims, R = fastnsf.dt_grid(RANGE, D["cell"], D["trunc"])
    # the second input: 2 000 rows in each of 40 cells
    per, ncl = 2000, max(N // 2000, 1)
    cells = torch.stack([torch.randint(0, v - 1, (ncl,), generator=gen) for v in vdims], dim=1).float()
    q0 = (torch.tensor(vorigin) + D["voxel"] * (cells.repeat_interleave(per, dim=0) + torch.rand(ncl * per, 3, generator=gen)))[None].to(dev)
    qcnt = torch.full((1,), ncl * per, dtype=torch.int32, device=dev)
    res = {"shape": {"batch": 1, "rows_pc0": N, "rows_pc1": N, "voxel": D["voxel"], "nodes": list(vdims), "NV": NV, "NC": NC, "cell": D["cell"],
                     "trunc": D["trunc"], "dt_grid": list(dims)},
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": "device events, median of 10; the kernels and the parts of the split: 20 calls replayed as one HIP graph, per call "
                     "(ms_single_eager_call: one eager call, with its launch gap)"}

    def kernels(x, count, name):
        n = int(x.shape[1])
        plan = lambda: floxels.vox_plan(x, count, origin=vorigin, voxel=D["voxel"], dims=vdims)
        pl = plan()
        theta = 0.1 * torch.randn(1, VZ, VY, VX, 3, generator=gen).to(dev)
        dF = torch.randn(1, n, 3, generator=gen).to(dev)
        per_cell = (pl["cell_rng"][:, 1] - pl["cell_rng"][:, 0])
        out = {"rows": n, "occupied_cells": int((per_cell > 0).sum()), "longest_cell": int(per_cell.max()), "active_nodes": int(pl["active"].sum()),
               "pairs": int(pl["pairs"][0]), "vox_plan_ms": round(median_ms(plan), 4)}
        sample = lambda: floxels.vox_sample(theta, pl["cell"], pl["frac"])
        scatter = lambda: floxels.vox_scatter(dF, pl["frac"], pl["idx_sorted"], pl["cell_rng"], dims=vdims)
        smooth = lambda: floxels.vox_smooth(theta, pl["active"])
        ms = graph_ms(sample)
        b = n * (4 + 12 + 8 * 12 + 12)      # per row: cell, frac, 8 corners of 12 bytes (4 runs of 24), F
        out["vox_sample"] = {"ms": round(ms, 4), "ms_single_eager_call": round(median_ms(sample), 4),
                             "bytes_without_sector_overfetch": b, "gb_per_s": round(b / ms / 1e6, 1)}
        ms = graph_ms(scatter)
        b = NC * 8 + n * (4 + 12 + 12) + NV * 12      # every input once (a range and a row are read by 8 nodes each: L2), dtheta
        out["vox_scatter"] = {"ms": round(ms, 4), "ms_single_eager_call": round(median_ms(scatter), 4),
                              "bytes_each_input_once": b, "gb_per_s": round(b / ms / 1e6, 1)}
        ms = graph_ms(smooth)
        b = NV * (12 + 1 + 4 + 12)          # theta, active, v, g (the neighbours' theta and flags: L2)
        out["vox_smooth"] = {"ms": round(ms, 4), "ms_single_eager_call": round(median_ms(smooth), 4),
                             "bytes_each_array_once": b, "gb_per_s": round(b / ms / 1e6, 1)}
        res[name] = out
        return pl, theta, dF

    pl, theta, dF = kernels(p0, cnt, "uniform_rows")
    kernels(q0, qcnt, "rows_2000_in_each_of_40_cells")

    def loop(opt, x, count, iters, graph, **kw):
        return lambda: opt(x, count, p1, cnt, grid_range=RANGE, iters=iters, check_every=0, graph=graph, **kw)

    lo, hi = 3, 13
    for model, opt, x, count, kw in (("floxels", floxels.floxels_optimize, p0, cnt, {}),
                                     ("floxels_rows_2000_in_each_of_40_cells", floxels.floxels_optimize, q0, qcnt, {}),
                                     ("fastnsf", fastnsf.fastnsf_optimize, p0, cnt, {"depth": a.depth})):
        out = {}
        for name, graph in (("eager", False), ("graph", True)):
            t_lo, t_hi = median_ms(loop(opt, x, count, lo, graph, **kw)), median_ms(loop(opt, x, count, hi, graph, **kw))
            out[f"ms_per_iteration_{name}"] = round((t_hi - t_lo) / (hi - lo), 4)
            out[f"ms_{name}_{lo}_iterations"], out[f"ms_{name}_{hi}_iterations"] = round(t_lo, 3), round(t_hi, 3)
        res[model] = out
    res["floxels"]["note"] = f"the {lo}- and {hi}-iteration calls both include one vox_plan and one dt_build; the difference does not"

    # the split of one floxels iteration on the uniform rows, every part timed alone on tensors of the loop's shapes
    dt2 = fastnsf.dt_build(p1, cnt, origin=origin, cell=D["cell"], dims=dims, radius=R)
    d, g = fastnsf.dt_lookup(p0, cnt, dt2, origin=origin, cell=D["cell"], radius=R)
    v, gs = floxels.vox_smooth(theta, pl["active"])
    dth = floxels.vox_scatter(dF, pl["frac"], pl["idx_sorted"], pl["cell_rng"], dims=vdims)
    n_par = 3 * NV
    arena, grads, m1, m2 = (torch.zeros((n_par + 3) // 4 * 4, device=dev) for _ in range(4))
    gview = grads[:n_par].view(1, NV, 3)
    step = torch.ones(1, dtype=torch.int32, device=dev)
    weight = torch.full((1, N), 1.0 / N, device=dev)
    scale1 = torch.full((1, 1, 1), 1e-3, device=dev)
    state = pairopt.Loop(torch.zeros(4, device=dev), p0, dict(D, iters=4))
    loss = torch.ones(1, device=dev)

    def snapshot():
        state.t_dev.zero_()
        state.snapshot(loss, dF)

    hip = {"vox_sample": res["uniform_rows"]["vox_sample"]["ms"],
           "dt_lookup": round(graph_ms(lambda: fastnsf.dt_lookup(p0, cnt, dt2, origin=origin, cell=D["cell"], radius=R, return_cells=True)), 4),
           "vox_smooth": res["uniform_rows"]["vox_smooth"]["ms"], "vox_scatter": res["uniform_rows"]["vox_scatter"]["ms"],
           "adam_step": round(graph_ms(lambda: call("df_adam_step_dev", ptr(arena), ptr(grads), ptr(m1), ptr(m2), arena.numel(), D["lr"],
                                                     pairopt.BETAS[0], pairopt.BETAS[1], pairopt.EPS, ptr(step), 1.0, stream())), 4)}
    tor = {"x0 + F": round(graph_ms(lambda: p0 + dF), 4),
           "data mean and weight": round(graph_ms(lambda: pairopt.mean_and_weight(d)), 4),
           "g x weight": round(graph_ms(lambda: g * weight[..., None]), 4),
           "smooth reduction": round(graph_ms(lambda: pairopt.sample_sum(v)), 4),
           "gradient addcmul": round(graph_ms(lambda: torch.addcmul(dth, gs, scale1, out=gview)), 4),
           "snapshot and freeze": round(graph_ms(snapshot), 4)}
    it = res["floxels"]["ms_per_iteration_graph"]
    res["floxels"]["split_ms"] = {"hip_entries": hip, "torch_ops": tor, "hip_sum": round(sum(hip.values()), 4), "torch_sum": round(sum(tor.values()), 4)}
    res["floxels"]["torch_share_of_graph_iteration"] = round(1.0 - sum(hip.values()) / it, 3) if it > 0 else None
    res["floxels"]["note_split"] = ("the parts are timed alone, each as 20 calls replayed in one graph; the share is 1 - (sum of the HIP "
                                    "entries) / (the replayed graph's iteration)")
    res["unexamined"] = ("no hardware counters were collected: how much of the scatter's and the stencil's neighbour reads hits L2 is not "
                         "examined; neither input is a real sweep (uniform rows occupy far more cells, the 40-cell input far fewer)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
