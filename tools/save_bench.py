"""What the whole-sweep flow (csrc/sweep.hip, deflow_amd/sweeps.py) costs on the GPU next to the host formulation it
replaces, measured: usage  python tools/save_bench.py [--batch 16] [--points 110000] [--ground 0.3] [--reps 10] [--out profiles/save_step.json]

One batch of --batch synthetic sweep pairs, --points raw rows per sweep, --ground of them flagged, the default 512 x 512 model with seeded
weights in eval mode.  After a warm-up, alternating in one process, the medians of --reps repetitions of

  * device:  compact_rows of both sweeps + compose_flow on the forward's outputs (device events; the forward itself is not in this number);
  * host:    what they replace -- boolean indexing and NaN padding on CPU tensors plus the host-to-device copy of the padded clouds (as
             collate_fn_pad and the loader do), then per sample an index_put of pose flow + flow through the counts read back (wall-clock,
             synchronised; the forward itself is not in this number either);
  * infer:   the whole SweepFlow.infer of the batch (device events), and the forward alone for scale.

Nothing here is a pass condition.  Real scenes were not measured.  A measuring tool, not a bench.py leg; needs the GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import deflow_amd
from deflow_amd import sweeps
from deflow_amd._lib import call, ptr, stream
from deflow_amd.data import _pad
from deflow_amd.deflow import batch_transform


def median(v):
    return sorted(v)[len(v) // 2]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def synth(g, B, n, ground):
    """sweeps in the vehicle frame: `ground` of the rows on the road plane (flagged), the rest up to 4 m above it, x / y within +-60 m"""
    raw = np.empty((B, n, 3), dtype=np.float32)
    raw[..., :2] = g.uniform(-60.0, 60.0, (B, n, 2))
    drop = g.random((B, n)) < ground
    raw[..., 2] = np.where(drop, g.normal(-0.33, 0.02, (B, n)), g.uniform(-0.1, 4.0, (B, n)))
    return torch.from_numpy(raw), torch.from_numpy(drop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=110000)
    ap.add_argument("--ground", type=float, default=0.3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "save_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/save_bench.py measures on the GPU"
    dev = torch.device("cuda")
    g = np.random.default_rng(20240912)
    B, n = a.batch, a.points
    torch.manual_seed(5)
    model = deflow_amd.DeFlow().to(dev).eval()
    raw0_h, drop0_h = synth(g, B, n, a.ground)
    raw1_h, drop1_h = synth(g, B, n, a.ground)
    raw0_h, raw1_h = raw0_h.pin_memory(), raw1_h.pin_memory()
    raw0, drop0, raw1, drop1 = raw0_h.to(dev), drop0_h.to(dev), raw1_h.to(dev), drop1_h.to(dev)
    cnt = torch.full((B,), n, dtype=torch.int32, device=dev)
    pose0 = torch.eye(4, device=dev).repeat(B, 1, 1)
    pose1 = pose0.clone()
    pose1[:, 0, 3] = 0.8
    sf = sweeps.SweepFlow(model)

    # ---- device: compaction of both sweeps + composition on a forward's outputs
    pc0, _, pos0, _ = sweeps.compact_rows(raw0, cnt, drop0)
    pc1, _, _, _ = sweeps.compact_rows(raw1, cnt, drop1)
    batch = {"pc0": pc0, "pc1": pc1, "pose0": pose0, "pose1": pose1}
    with torch.no_grad():
        st = model.forward_padded(batch)
    T = batch_transform(batch, dev)
    flow, idx_c, counts = st["flow"].detach().clone(), st["idx_c0"].clone(), st["counts0"].clone()

    def device_path():
        sweeps.compact_rows(raw0, cnt, drop0)
        sweeps.compact_rows(raw1, cnt, drop1)
        return sweeps.compose_flow(raw0, cnt, T, pos0, flow, idx_c, counts)

    # ---- host: boolean indexing + padding on the CPU, the copies, then an index_put per sample through the counts read back
    def host_path():
        keep0, keep1 = ~drop0_h, ~drop1_h
        rows = [torch.nonzero(keep0[b]).reshape(-1) for b in range(B)]
        h0 = _pad([raw0_h[b][keep0[b]] for b in range(B)], float("nan")).pin_memory().to(dev, non_blocking=True)
        _pad([raw1_h[b][keep1[b]] for b in range(B)], float("nan")).pin_memory().to(dev, non_blocking=True)
        rows_d = [r.to(dev) for r in rows]
        est = torch.empty_like(raw0)
        scratch = torch.empty_like(raw0)
        call("df_ego_transform", ptr(raw0), ptr(T), B, n, ptr(scratch), ptr(est), stream())          # the pose flow of every raw row
        m = counts.tolist()
        width = h0.shape[1]
        for b in range(B):
            i = idx_c[b, : m[b]].clamp(max=width - 1)
            est[b].index_put_((rows_d[b][i],), flow[b, : m[b]], accumulate=True)
        return est

    def forward_only():
        with torch.no_grad():
            model.forward_padded(batch)

    infer = lambda: sf.infer(raw0, cnt, drop0, raw1, cnt, drop1, pose0, pose1)
    for fn in (device_path, host_path, infer, forward_only):                   # warm-up: the library, the allocator, the canvases
        fn()
        fn()
    torch.cuda.synchronize()
    t = {"device_ms": [], "device_wall_ms": [], "host_wall_ms": [], "infer_ms": [], "forward_ms": []}
    for _ in range(a.reps):                                                    # alternating
        t["device_ms"].append(event_ms(device_path))
        t["host_wall_ms"].append(wall_ms(host_path))
        t["device_wall_ms"].append(wall_ms(device_path))
        t["infer_ms"].append(event_ms(infer))
        t["forward_ms"].append(event_ms(forward_only))
    # the two formulations agree on the finite rows the model decoded or not (the host one knows no NaN / padded rows: none here)
    same = bool(torch.equal(device_path()[0], host_path()))
    report = {"device": torch.cuda.get_device_name(0), "batch": B, "rows_per_sweep": n, "ground_fraction": a.ground, "reps": a.reps,
              "decoded_rows": int(counts.sum()), **{k: round(median(v), 4) for k, v in t.items()},
              "host_over_device_wall": round(median(t["host_wall_ms"]) / median(t["device_wall_ms"]), 2),
              "device_share_of_infer": round(median(t["device_ms"]) / median(t["infer_ms"]), 4), "host_and_device_flow_equal": same}
    print(json.dumps(report), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
