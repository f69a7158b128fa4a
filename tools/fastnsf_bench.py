"""Measure model=fastnsf on one pair of 80 000 + 80 000 synthetic rows (B = 1) in the default range and write profiles/fastnsf_flow.json:
one df_dt_build, one df_dt_lookup, ms per whole iteration, eager and as a replayed HIP graph, and -- in the same session on the same box,
for comparison -- model=nsfp's iteration.  Medians of 10, by device events.  For the transform and the lookup the bytes the algorithm
has to move over the time.  No thresholds: the numbers are written down with the box they came from.

    python tools/fastnsf_bench.py [--rows 80000] [--depth 7] [--out profiles/fastnsf_flow.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deflow_amd import fastnsf, nsfp, pairopt  # noqa: E402
from nsfp_bench import median_ms  # noqa: E402

RANGE = (-51.2, -51.2, -3.0, 51.2, 51.2, 3.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fastnsf_flow.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    N, depth = a.rows, a.depth
    gen = torch.Generator().manual_seed(0)
    scale = torch.tensor([50.0, 50.0, 2.0])
    p0 = ((torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale).to(dev)
    p1 = ((torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale + torch.tensor([0.4, 0.1, 0.0])).to(dev)
    cnt = torch.full((1,), N, dtype=torch.int32, device=dev)
    cell, trunc = fastnsf.DEFAULTS["cell"], fastnsf.DEFAULTS["trunc"]
    origin, dims, R = fastnsf.dt_grid(RANGE, cell, trunc)
    vox = dims[0] * dims[1] * dims[2]
    res = {"shape": {"batch": 1, "rows_pc0": N, "rows_pc1": N, "depth": depth, "width": nsfp.WIDTH, "cell": cell, "trunc": trunc,
                     "grid": list(dims), "voxels": vox, "radius": R},
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "method": "device events, median of 10"}

    grid_kw = dict(origin=origin, cell=cell, dims=dims, radius=R)
    ms_build = median_ms(lambda: fastnsf.dt_build(p1, cnt, **grid_kw))
    dt2 = fastnsf.dt_build(p1, cnt, **grid_kw)
    ms_lookup = median_ms(lambda: fastnsf.dt_lookup(p0, cnt, dt2, origin=origin, cell=cell, radius=R, return_cells=True))
    # what the algorithm has to move: the clear writes the grid once, every pass reads and writes it once (2 bytes per voxel)
    build_bytes = 2.0 * vox * (1 + 3 * 2)
    res["dt_build"] = {"ms": round(ms_build, 4), "algorithmic_gb": round(build_bytes / 1e9, 3), "gb_per_s": round(build_bytes / ms_build / 1e6, 1),
                       "window_reads_per_voxel_and_pass": 2 * R + 1}
    # per row: 12 bytes of query, eight 2-byte corners (their 32-byte sectors are what moves), 4 + 12 + 12 + 1 bytes of outputs
    res["dt_lookup"] = {"ms": round(ms_lookup, 4), "rows": N, "bytes_per_row_without_sector_overfetch": 12 + 16 + 29}

    def loop(opt, iters, graph, **kw):
        return lambda: opt(p0, cnt, p1, cnt, depth=depth, iters=iters, check_every=0, graph=graph, **kw)

    lo, hi = 3, 13
    for model, opt, kw in (("fastnsf", fastnsf.fastnsf_optimize, {"grid_range": RANGE}), ("nsfp", nsfp.nsfp_optimize, {})):
        out = {}
        for name, graph in (("eager", False), ("graph", True)):
            t_lo, t_hi = median_ms(loop(opt, lo, graph, **kw)), median_ms(loop(opt, hi, graph, **kw))
            out[f"ms_per_iteration_{name}"] = round((t_hi - t_lo) / (hi - lo), 4)
            out[f"ms_{name}_{lo}_iterations"], out[f"ms_{name}_{hi}_iterations"] = round(t_lo, 3), round(t_hi, 3)
        res[model] = out
    res["fastnsf"]["note"] = f"the {lo}- and {hi}-iteration calls both include one dt_build; the difference does not"

    # the split of one fastnsf iteration, every part timed alone on the tensors the loop hands it
    arena = fastnsf.start_params(depth, 0).to(dev)[None].contiguous()
    par = arena[:, 0]
    y, acts = nsfp.mlp_forward(p0, cnt, par, depth)
    dy = torch.randn_like(y)
    d = fastnsf.dt_lookup(p0, cnt, dt2, origin=origin, cell=cell, radius=R)[0]
    res["fastnsf"]["split_ms"] = {
        "mlp_forward": round(median_ms(lambda: nsfp.mlp_forward(p0, cnt, par, depth)), 4),
        "lookup": round(ms_lookup, 4),
        "loss_reduction": round(median_ms(lambda: pairopt.mean_and_weight(d)), 4),
        "mlp_backward without dx": round(median_ms(lambda: nsfp.mlp_backward(p0, cnt, par, depth, acts, dy, need_dx=False)), 4)}
    res["unexamined"] = ("no hardware counters were collected: where the transform's passes spend their time (L2 hits of the window reads, "
                         "the 2-byte accesses) is not examined; the rows are uniformly random, so the grid is far more occupied than a real "
                         "sweep's and the lookups are less local")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
