"""What packing the submission bodies on the GPU (csrc/submit.hip, deflow_amd/submit.py) costs next to the host
formulation it replaces, measured: usage  python tools/submit_bench.py [--batch 16] [--points 110000] [--masked 0.5] [--reps 10]
[--out profiles/submit_step.json]

One batch of --batch synthetic sweeps' composed flow (``flow_est`` f32 [B,N,3], ``dynamic`` u8 [B,N], as df_flow_compose leaves them on the
device), --points raw rows per sweep, --masked of them outside the benchmark's mask.  After a warm-up, alternating in one process, the
medians of --reps repetitions of

  * device:  pack_rows -- the mask's negation, df_sweep_compact, df_submit_pack -- by device events and by synchronised wall-clock, and the
             same followed by the copy of ``body`` and ``kept`` into pinned memory (what the command does per batch);
  * host:    what it replaces -- the copy of ``flow_est`` and ``dynamic`` into pinned memory, then per sample boolean indexing,
             ``astype(float16)`` per column, ``np.packbits(bitorder="little")`` and the padded concatenation (wall-clock, synchronised).

Both produce every sample's body; they are compared byte for byte once.  The model's forward is in neither number.  Nothing here is a pass
condition.  Real scenes, the feather metadata and the zip writer were not measured.  A measuring tool, not a bench.py leg; needs the GPU."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deflow_amd import submit
from deflow_amd.feather import body_len


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


def pad8(raw: bytes) -> bytes:
    return raw + bytes(-len(raw) % 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=110000)
    ap.add_argument("--masked", type=float, default=0.5)
    ap.add_argument("--version", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "submit_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/submit_bench.py measures on the GPU"
    dev = torch.device("cuda")
    g = np.random.default_rng(20241019)
    B, n, version = a.batch, a.points, a.version
    flow_est = torch.from_numpy((g.standard_normal((B, n, 3)) * (1.0, 0.2, 0.02)).astype(np.float32)).to(dev)
    dynamic = torch.from_numpy((g.random((B, n)) < 0.1).astype(np.uint8)).to(dev)
    mask_h = (g.random((B, n)) >= a.masked)
    mask = torch.from_numpy(mask_h.astype(np.uint8)).to(dev)
    cnt = torch.full((B,), n, dtype=torch.int32, device=dev)
    S = submit.body_stride(n)
    pin = {"body": torch.empty(B, S, dtype=torch.uint8, pin_memory=True), "kept": torch.empty(B, dtype=torch.int32, pin_memory=True),
           "flow": torch.empty(B, n, 3, dtype=torch.float32, pin_memory=True), "dyn": torch.empty(B, n, dtype=torch.uint8, pin_memory=True)}

    def device_pack():
        return submit.pack_rows(flow_est, dynamic, mask, cnt, version)

    def device_path():                                   # pack + the batch's one copy back
        body, kept = device_pack()
        pin["body"].copy_(body, non_blocking=True)
        pin["kept"].copy_(kept, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        hb, hk = pin["body"].numpy(), pin["kept"].tolist()
        return [hb[b, : body_len(hk[b])] for b in range(B)]

    def host_path():                                     # copy everything back, then numpy per sample
        pin["flow"].copy_(flow_est, non_blocking=True)
        pin["dyn"].copy_(dynamic, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        hf, hd = pin["flow"].numpy(), pin["dyn"].numpy()
        out = []
        for b in range(B):
            keep = mask_h[b]
            sel = hf[b][keep]
            cols = b"".join(pad8(sel[:, i].astype(np.float16).tobytes()) for i in range(3))
            flags = hd[b][keep] != 0 if version == 1 else np.ones(sel.shape[0], dtype=bool)
            bits = pad8(np.packbits(flags, bitorder="little").tobytes())
            out.append(cols + bits if version == 1 else bits + cols)
        return out

    for fn in (device_pack, device_path, host_path):     # warm-up: the library, the allocator
        fn()
        fn()
    torch.cuda.synchronize()
    t = {"device_pack_ms": [], "device_pack_wall_ms": [], "device_with_copy_wall_ms": [], "host_wall_ms": []}
    for _ in range(a.reps):                              # alternating
        t["device_pack_ms"].append(event_ms(device_pack))
        t["host_wall_ms"].append(wall_ms(host_path))
        t["device_pack_wall_ms"].append(wall_ms(device_pack))
        t["device_with_copy_wall_ms"].append(wall_ms(device_path))
    same = all(d.tobytes() == h for d, h in zip(device_path(), host_path()))
    rows = int(mask_h.sum())
    report = {"device": torch.cuda.get_device_name(0), "batch": B, "rows_per_sweep": n, "masked_fraction": a.masked, "selected_rows": rows,
              "leaderboard_version": version, "reps": a.reps, "body_stride_bytes": S, "body_bytes": sum(body_len(int(m)) for m in mask_h.sum(axis=1)),
              "bytes_back_device_path": B * S + 4 * B, "bytes_back_host_path": B * n * 13,
              **{k: round(median(v), 4) for k, v in t.items()},
              "host_over_device_with_copy_wall": round(median(t["host_wall_ms"]) / median(t["device_with_copy_wall_ms"]), 2),
              "host_and_device_bodies_equal": same}
    print(json.dumps(report), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
