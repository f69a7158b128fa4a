"""What the bird's-eye-view rasteriser (csrc/render.hip, deflow_amd/render.py) costs on the GPU next to the host
formulation it replaces, measured: usage  python tools/vis_bench.py [--batch 16] [--points 110000] [--side 1024] [--radius 1] [--reps 10]
[--out profiles/vis_step.json]

One batch of --batch synthetic sweeps, --points raw rows each (30 % on the road plane, class 2; the rest coloured by a synthetic vector),
a --side x --side image at 0.1 m per pixel.  After a warm-up, alternating in one process, the medians of --reps repetitions of

  * device:  render_rows -- the image's memset, df_render_splat, df_render_resolve -- by device events and by synchronised wall-clock, and
             the same followed by the copy of the scanlines into pinned memory (wall-clock);
  * parts:   the memset, the splat and the resolve one by one through the binding (device events);
  * host:    what it replaces -- the rows, vectors and classes copied to the host, then rasterised by the numpy restatement of the
             definition (tests/helpers/render_ref.py) (wall-clock, synchronised).

Both give the same bytes, which the report records.  Nothing here is a pass condition.  Real scenes, ``flow_source=model`` end to end and
zlib's time were not measured.  A measuring tool, not a bench.py leg; needs the GPU (no fallback)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import numpy as np
import torch

import render_ref as RR
from deflow_amd import render
from deflow_amd._lib import call, ptr, stream


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=110000)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vis_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/vis_bench.py measures on the GPU"
    dev = torch.device("cuda")
    g = np.random.default_rng(20241019)
    B, n, side = a.batch, a.points, a.side
    half = 0.05 * side
    view, size, vmax, legend = (-half, -half, 10.0), (side, side), 1.0, 32
    # sweeps in the vehicle frame: denser near the sensor (a normal in x / y, some of it outside the view), 30 % ground
    pts = np.empty((B, n, 3), dtype=np.float32)
    pts[..., :2] = g.normal(0.0, 0.45 * half, (B, n, 2))
    ground = g.random((B, n)) < 0.3
    pts[..., 2] = np.where(ground, g.normal(-0.33, 0.02, (B, n)), g.uniform(-0.1, 4.0, (B, n)))
    vec = (g.standard_normal((B, n, 3)) * 0.4).astype(np.float32)
    vec[g.random((B, n)) < 0.6] = 0.0                                    # most rows are static
    cls = np.where(ground, 2, 1).astype(np.uint8)
    cnt = np.full(B, n, dtype=np.int32)
    d = lambda x: torch.from_numpy(x).to(dev)
    pts_d, vec_d, cls_d, cnt_d = d(pts), d(vec), d(cls), d(cnt)
    pinned = torch.empty(B, side, 1 + 3 * side, dtype=torch.uint8, pin_memory=True)
    kw = dict(view=view, size=size, vmax=vmax, radius=a.radius, legend=legend)

    def device_path():
        return render.render_rows(pts_d, cnt_d, vec_d, cls_d, **kw)

    # the three launches of render_rows one by one, through the binding (device events)
    image = torch.zeros(B, side, side, dtype=torch.int64, device=dev)
    lines = torch.empty(B, side, 1 + 3 * side, dtype=torch.uint8, device=dev)
    zero = lambda: image.zero_()
    splat = lambda: call("df_render_splat", ptr(pts_d), ptr(vec_d), ptr(cls_d), ptr(cnt_d), B, n, view[0], view[1], view[2], side, side, vmax,
                         a.radius, ptr(image), stream())
    resolve = lambda: call("df_render_resolve", ptr(image), B, side, side, 0x181818, legend, ptr(lines), stream())

    def device_and_copy():
        pinned.copy_(device_path(), non_blocking=True)

    def host_path():
        p, v, c, k = pts_d.cpu().numpy(), vec_d.cpu().numpy(), cls_d.cpu().numpy(), cnt_d.cpu().numpy()
        return RR.render_rows(p, k, v, c, view, size, vmax, radius=a.radius, legend=legend)

    for fn in (device_path, device_and_copy, host_path):                 # warm-up: the library, the allocator, numpy's buffers
        fn()
    torch.cuda.synchronize()
    t = {"device_ms": [], "device_wall_ms": [], "device_and_copy_wall_ms": [], "host_wall_ms": [], "zero_ms": [], "splat_ms": [], "resolve_ms": []}
    for _ in range(a.reps):                                              # alternating
        t["device_ms"].append(event_ms(device_path))
        t["host_wall_ms"].append(wall_ms(host_path))
        t["device_wall_ms"].append(wall_ms(device_path))
        t["device_and_copy_wall_ms"].append(wall_ms(device_and_copy))
        for name, fn in (("zero_ms", zero), ("splat_ms", splat), ("resolve_ms", resolve)):      # in this order: splat needs the zeroed image
            t[name].append(event_ms(fn))
    assert torch.equal(lines, device_path()), "the launches one by one and render_rows differ"
    got = device_path().cpu().numpy()
    want = host_path()
    drawn = int((RR.pixels(want) != 24).any(axis=-1).sum())
    report = {"device": torch.cuda.get_device_name(0), "batch": B, "rows_per_sweep": n, "image": [side, side], "radius": a.radius,
              "legend": legend, "reps": a.reps, "pixels_drawn": drawn, "pixels": B * side * side,
              "scanline_bytes": int(got.size), **{k: round(median(v), 4) for k, v in t.items()},
              "host_over_device_wall": round(median(t["host_wall_ms"]) / median(t["device_wall_ms"]), 1),
              "host_and_device_bytes_equal": bool(np.array_equal(got, want)),
              "not_measured": ["real scenes", "flow_source=model end to end", "zlib (png.write_png) time"]}
    print(json.dumps(report), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
