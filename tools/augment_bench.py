"""What the training augmentation (csrc/augment.hip, deflow_amd/augment.py) costs at the training shape, measured:
usage  python tools/augment_bench.py [--batch 16] [--points 80000] [--reps 200] [--windows 7] [--out profiles/augment_step.json]

One synthetic batch of --batch pairs, --points rows per cloud, with flow, ego motion and poses.  For each form -- the default arguments
(flips, height, jitter: per-row words drawn), everything on (yaw and dropout too), flips and height only (no per-row words), and the
default arguments at --points + 1 rows (the 4-byte path) -- after a warm-up, the median over --windows windows of

  * kernel:     --reps back-to-back df_augment launches into preallocated outputs between two device events, per launch.  The host
                enqueues a launch faster than it runs only if the figure is well above the enqueue time, which is reported beside it
                (the same loop, wall-clock, not synchronised until its end); a kernel figure close to it is an upper bound.
  * augmenter:  ``Augmenter.__call__`` (its allocations and batch_transform included), wall-clock with the project's synchronising timer.

bytes = what the op must move: both clouds and the flow, read once and written once.  Nothing here is a pass condition.  A measuring tool,
not a bench.py leg; needs the GPU."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deflow_amd._lib import call, ptr, stream
from deflow_amd.augment import Augmenter
from deflow_amd.timer import Timing

FORMS = {"default": {}, "all_on": {"yaw_deg": 45.0, "drop_p": 0.1}, "flips_height_only": {"jitter_sigma": 0.0}}


def median(v):
    return sorted(v)[len(v) // 2]


def make_batch(B, n, dev):
    g = torch.Generator().manual_seed(20241019)
    pc0 = torch.randn(B, n, 3, generator=g) * torch.tensor([20.0, 20.0, 1.5])
    pc0[:, -n // 50:] = float("nan")
    pc1 = pc0 + torch.randn(B, n, 3, generator=g) * 0.05
    T = torch.eye(4).repeat(B, 1, 1)
    T[:, 0, 3] = 0.8
    return {"pc0": pc0.to(dev), "pc1": pc1.to(dev), "flow": (pc1 - pc0).to(dev), "ego_motion": T.to(dev), "pose0": T.to(dev), "pose1": T.to(dev)}


def measure(aug, batch, ids, reps, windows):
    B, n, _ = batch["pc0"].shape
    outs = {k: torch.empty_like(v) for k, v in batch.items()}
    args = (aug.seed, 1, aug.flip_x_p, aug.flip_y_p, math.radians(aug.yaw_deg), aug.height, aug.jitter_sigma, aug.drop_p)

    def launch():
        call("df_augment", ptr(batch["pc0"]), ptr(batch["pc1"]), ptr(batch["flow"]), ptr(ids), B, n, n, *args, ptr(batch["ego_motion"]),
             ptr(batch["pose0"]), ptr(batch["pose1"]), ptr(outs["pc0"]), ptr(outs["pc1"]), ptr(outs["flow"]), ptr(outs["ego_motion"]),
             ptr(outs["pose0"]), ptr(outs["pose1"]), stream())

    for _ in range(20):
        launch()
        aug(batch, ids, 1)
    torch.cuda.synchronize()
    kernel, enqueue, whole = [], [], []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            launch()
        e1.record()
        enqueue.append((time.perf_counter() - t0) * 1e6 / reps)
        torch.cuda.synchronize()
        kernel.append(e0.elapsed_time(e1) * 1e3 / reps)
        t = Timing(sync=True)
        t.start("augmenter")
        for _ in range(reps):
            aug(batch, ids, 1)
        t.stop()
        whole.append(t.total * 1e6 / reps)
    moved = 6 * B * n * 12                       # pc0, pc1, flow: read + written
    k = median(kernel)
    return {"rows_per_cloud": n, "bytes_moved": moved, "kernel_us": round(k, 2), "kernel_us_min": round(min(kernel), 2),
            "kernel_us_max": round(max(kernel), 2), "enqueue_us": round(median(enqueue), 2), "achieved_GB_per_s": round(moved / k / 1e3, 1),
            "augmenter_call_wall_us": round(median(whole), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "augment_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/augment_bench.py measures on the GPU"
    dev = torch.device("cuda")
    B = a.batch
    ids = torch.arange(B, dtype=torch.int64, device=dev) + 20240116
    batch = make_batch(B, a.points, dev)
    report = {"device": torch.cuda.get_device_name(0), "batch": B, "reps_per_window": a.reps, "windows": a.windows, "forms": {}}
    for name, kw in FORMS.items():
        report["forms"][name] = measure(Augmenter(20240116, **kw), batch, ids, a.reps, a.windows)
    report["forms"]["default_4_byte_path"] = measure(Augmenter(20240116), make_batch(B, a.points + 1, dev), ids, a.reps, a.windows)
    print(json.dumps(report), flush=True)
    if a.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
        print("wrote", a.out)


if __name__ == "__main__":
    main()
