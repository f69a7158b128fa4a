"""What the ground segmenter (csrc/ground.hip) costs on the GPU, measured: usage  python tools/ground_bench.py
[--points 100000] [--batches 1 16] [--reps 20] [--sweeps 150] [--out profiles/ground_step.json]

At each batch size, --points rows per cloud (a synthetic street sweep: a gently tilted road, boxes, walls) on the default 205 x 205 grid,
it times with device events, after a warm-up, the medians of --reps calls of

  * df_ground_cells (its async fill of zmin included), df_ground_height, df_ground_mask;
  * df_nn_grid_build on the same cloud in the same run -- the yardstick: it also files rows under an xy grid;

and reports each next to its byte floor at the achieved fraction of --hbm-gbps: rows x 12 B read (+ 1 B written for the mask) for the row
entries, Gx Gy 4 B read + 5 B per cell written for the height entry (whose time is the serial chain, not bytes).  Then it segments a
synthetic scene of --sweeps sweeps end to end (ground.label_sweeps: upload, three entries, read the mask back, per sweep), wall-clock.

Nothing exists to time this against: it is a new capability, and no number here is a pass condition.  Real scenes were not measured.
A measuring tool, not a bench.py leg; needs the GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deflow_amd import chamfer, ground
from deflow_amd._lib import call, ptr, stream


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


def synth_sweep(g, n):
    """a lidar-like sweep in the vehicle frame: 70 % road returns (range uniform in 3 .. 70 m: denser near the vehicle) on a plane tilted
    by 2 % per axis 0.33 m below the frame, 15 % on 40 car-sized boxes from 0.25 m above the road, 15 % on walls 12 .. 50 m away"""
    surface = lambda x, y: -0.33 + 0.02 * x - 0.02 * y
    nr, nc = int(0.7 * n), int(0.15 * n)
    r, a = g.uniform(3.0, 70.0, nr), g.uniform(0, 2 * np.pi, nr)
    parts = [(r * np.cos(a), r * np.sin(a), g.normal(0.0, 0.02, nr))]
    r, a = g.uniform(6.0, 48.0, 40), g.uniform(0, 2 * np.pi, 40)
    k = g.integers(0, 40, nc)
    parts.append((r[k] * np.cos(a[k]) + g.uniform(-2.25, 2.25, nc), r[k] * np.sin(a[k]) + g.uniform(-0.95, 0.95, nc), g.uniform(0.25, 1.6, nc)))
    nw = n - nr - nc
    r, a = g.uniform(12.0, 50.0, nw), g.uniform(0, 2 * np.pi, nw)
    parts.append((r * np.cos(a), r * np.sin(a), g.uniform(0.0, 6.0, nw)))
    x, y, above = (np.concatenate([p[i] for p in parts]) for i in range(3))
    return np.stack([x, y, surface(x, y) + above], 1).astype(np.float32)


def stages(B, n, reps, g, dev, hbm):
    pts = torch.from_numpy(np.stack([synth_sweep(g, n) for _ in range(B)])).to(dev)
    cnt = torch.full((B,), n, dtype=torch.int32, device=dev)
    seg = ground.GroundSegmenter(B, device=dev)
    Gx, Gy = seg.dims
    mask = torch.empty(B, n, dtype=torch.uint8, device=dev)
    rows = (*seg.xy_min, seg.kxy, seg.z_min, seg.kz, Gx, Gy, seg.z_levels)
    cells = lambda: call("df_ground_cells", ptr(pts), ptr(cnt), B, n, *rows, ptr(seg._zmin), stream())
    height = lambda: call("df_ground_height", ptr(seg._zmin), B, Gx, Gy, seg.ox, seg.oy, seg.seed, seg.RISE, seg.DROP, seg.WIDEN, seg.miss_cap,
                          ptr(seg._height), ptr(seg._observed), stream())
    masks = lambda: call("df_ground_mask", ptr(pts), ptr(cnt), B, n, *rows, ptr(seg._height), seg.TOL, ptr(mask), stream())
    # the yardstick: the chamfer search's grid build over the same rows (the grid chamfer.py would choose for this cloud)
    grid = chamfer.RowGrid(B, chamfer.GRID_RANGE, chamfer.CELL, dev)
    build = lambda: grid.file(pts, cnt)
    t = {"cells_ms": timed(cells, reps), "height_ms": timed(height, reps), "mask_ms": timed(masks, reps), "nn_grid_build_ms": timed(build, reps),
         "zmin_fill_ms": timed(lambda: seg._zmin.fill_(ground.EMPTY), reps)}
    whole = timed(lambda: seg.segment(pts, cnt), reps)
    floor = lambda nbytes: nbytes / (hbm * 1e9) * 1e3
    fl = {"cells": floor(B * n * 12), "mask": floor(B * n * 13), "height": floor(B * Gx * Gy * 9)}
    out = {"batch": B, "rows_per_cloud": n, "dims": [Gx, Gy], **{k: round(v, 4) for k, v in t.items()}, "segment_ms": round(whole, 4),
           "cells_floor_ms_rows_x12B": round(fl["cells"], 5), "mask_floor_ms_rows_x13B": round(fl["mask"], 5),
           "height_floor_ms_cells_x9B": round(fl["height"], 6),
           "cells_x_floor": round(t["cells_ms"] / fl["cells"], 1), "mask_x_floor": round(t["mask_ms"] / fl["mask"], 1),
           "height_x_floor": round(t["height_ms"] / fl["height"], 1),
           "cells_vs_nn_grid_build": round(t["cells_ms"] / t["nn_grid_build_ms"], 3),
           "three_entries_vs_nn_grid_build": round((t["cells_ms"] + t["height_ms"] + t["mask_ms"]) / t["nn_grid_build_ms"], 3),
           "longest_chain_steps": int(max(seg.ox, Gx - 1 - seg.ox, seg.oy, Gy - 1 - seg.oy)) + 1,
           "cells_with_rows": int((seg.cell_min != ground.EMPTY).sum()), "observed_cells": int(seg.observed.sum()),
           "ground_rows": int(seg.segment(pts, cnt).sum())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=150)
    ap.add_argument("--hbm-gbps", type=float, default=8000.0, help="the HBM rate the byte floors are computed at (MI355X: 8 TB/s nominal)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ground_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/ground_bench.py measures on the GPU"
    dev = torch.device("cuda")
    g = np.random.default_rng(20240611)
    report = {"device": torch.cuda.get_device_name(0), "hbm_gbps_of_the_floors": a.hbm_gbps, "params": ground.GroundSegmenter(1, device=dev).params(),
              "stages": []}
    for B in a.batches:
        report["stages"].append(stages(B, a.points, a.reps, g, dev, a.hbm_gbps))
        print(json.dumps(report["stages"][-1]), flush=True)

    # ---- a synthetic scene end to end ------------------------------------------------------------------------------------------------
    lidars = [synth_sweep(g, a.points) for _ in range(a.sweeps)]
    rep = {}
    ground.label_sweeps(lidars[:2], device=dev)                                # warm-up: the library, the allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = ground.label_sweeps(lidars, device=dev, report=rep)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rows = sum(len(o) for o in out)
    report["scene"] = {"sweeps": a.sweeps, "rows": rows, "seconds": round(dt, 3), "ms_per_sweep": round(dt / a.sweeps * 1e3, 3),
                       "ground_fraction": round(sum(int(o.sum()) for o in out) / rows, 6),
                       "observed_cell_fraction": round(rep["observed_cell_fraction"], 6)}
    print(json.dumps(report["scene"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
