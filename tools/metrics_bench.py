"""What the device-resident validation metrics (csrc/metrics.hip) cost, measured: usage  python tools/metrics_bench.py
[--batch 16] [--points 80000] [--reps 20] [--out profiles/metrics_step.json]

At BASELINE.json configs[2]'s shape (B = 16, 80k-point synthetic pairs, 512 x 512 grid, 4 GRU iterations; the batch also gets random
is_valid / eval_mask / category labels so that every optional input is read), in one process, medians of --reps after a warm-up:

  * df_metrics_rows and df_metrics_accumulate, timed with device events, next to their byte floors at --hbm-gbps;
  * one validation iteration by host wall-clock, torch.cuda.synchronize() at the end: forward + metrics with metrics_impl=host
    (evaluate_batch(model(batch), batch, OfficialMetrics)) and with metrics_impl=device (evaluate_batch_device);
  * the forward alone (forward_padded), the yardstick.

No number here is a pass condition.  Not measured: real scenes (whose masks and categories are not random), and B = 1.
A measuring tool, not a bench.py leg; needs the GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import deflow_amd
from deflow_amd._lib import call, ptr, stream
from deflow_amd.metrics import OfficialMetrics, evaluate_batch
from deflow_amd.metrics_device import DeviceMetrics, evaluate_batch_device, rows_per_block
from deflow_amd.synth import synth_batch


def median(v):
    return sorted(v)[len(v) // 2]


def events(fn, reps):
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
    return median(out)


def wall(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--hbm-gbps", type=float, default=8000.0, help="the HBM rate the byte floors are computed at (MI355X: 8 TB/s nominal)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "metrics_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/metrics_bench.py measures on the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    model = deflow_amd.DeFlow().to(dev).eval()
    B, N = a.batch, a.points
    batch = synth_batch(B, N, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    batch["flow_is_valid"] = torch.rand(B, N, device=dev, generator=g) < 0.9
    batch["eval_mask"] = torch.rand(B, N, device=dev, generator=g) < 0.8
    batch["flow_category_indices"] = (torch.randint(0, 31, (B, N), device=dev, generator=g)
                                      * (torch.rand(B, N, device=dev, generator=g) < 0.6)).to(torch.uint8)
    batch["has_eval_mask"] = torch.ones(B, dtype=torch.bool, device=dev)

    dm = DeviceMetrics(dev)
    with torch.no_grad():
        st = model.forward_padded(batch)
    flow, pose_flow, idx_c, counts = st["flow"].clone(), st["pose_flow"].clone(), st["idx_c0"].clone(), st["counts0"].clone()
    pc0, gt = batch["pc0"].float().contiguous(), batch["flow"].float().contiguous()
    valid, emask = batch["flow_is_valid"].view(torch.uint8), batch["eval_mask"].view(torch.uint8)
    cats, has = batch["flow_category_indices"], batch["has_eval_mask"].view(torch.uint8)
    dm.reserve(B, N)
    rows = lambda: call("df_metrics_rows", ptr(flow), ptr(pose_flow), ptr(pc0), ptr(gt), ptr(idx_c), ptr(counts), ptr(valid), ptr(emask),
                        ptr(cats), B, N, ptr(dm._edges), ptr(dm._ws), ptr(dm._status), stream())
    acc = lambda: call("df_metrics_accumulate", ptr(counts), ptr(has), B, N, ptr(dm._ws), ptr(dm._sf), ptr(dm._si), stream())
    rows_ms, acc_ms = events(rows, a.reps), events(acc, a.reps)
    update_ms = events(lambda: dm.update(flow, pose_flow, pc0, gt, idx_c, counts, is_valid=batch["flow_is_valid"], eval_mask=batch["eval_mask"],
                                         categories=cats, has_eval_mask=batch["has_eval_mask"]), a.reps)

    def host_iter():
        with torch.no_grad():
            evaluate_batch(model(batch), batch, OfficialMetrics())

    dm2 = DeviceMetrics(dev)

    def fwd():
        with torch.no_grad():
            model.forward_padded(batch)

    fwd_ms = wall(fwd, a.reps)
    dev_ms = wall(lambda: evaluate_batch_device(model, batch, dm2), a.reps)
    host_ms = wall(host_iter, a.reps)

    R = rows_per_block()
    n_rows = int(counts.sum())
    blocks = int(((counts.clamp(0, N) + R - 1) // R).sum())
    per_partial = 519 * 8 + 270 * 4
    rows_bytes = n_rows * (8 + 4 * 12 + 3) + blocks * per_partial
    acc_bytes = blocks * per_partial + 2 * B * per_partial
    floor = lambda nbytes: nbytes / (a.hbm_gbps * 1e9) * 1e3
    report = {"device": torch.cuda.get_device_name(0), "batch": B, "points_per_cloud": N, "reps": a.reps, "rows_per_block": R,
              "compact_rows": n_rows, "blocks_with_rows": blocks, "hbm_gbps_of_the_floors": a.hbm_gbps,
              "rows_ms": round(rows_ms, 4), "rows_bytes": rows_bytes, "rows_floor_ms": round(floor(rows_bytes), 5),
              "rows_x_floor": round(rows_ms / floor(rows_bytes), 1),
              "accumulate_ms": round(acc_ms, 4), "accumulate_bytes": acc_bytes, "accumulate_floor_ms": round(floor(acc_bytes), 5),
              "accumulate_x_floor": round(acc_ms / floor(acc_bytes), 1),
              "update_ms_events": round(update_ms, 4),
              "forward_ms_wall": round(fwd_ms, 3), "iteration_device_ms_wall": round(dev_ms, 3), "iteration_host_ms_wall": round(host_ms, 3),
              "metrics_device_ms_beside_forward": round(dev_ms - fwd_ms, 3), "metrics_host_ms_beside_forward": round(host_ms - fwd_ms, 3),
              "not_measured": ["real scenes", "B = 1"]}
    print(json.dumps(report), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
