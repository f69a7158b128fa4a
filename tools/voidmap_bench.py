"""What the void map (csrc/voidmap.hip) costs on the GPU, measured: usage  python tools/voidmap_bench.py
[--points 100000] [--voxel 0.1] [--dims 1024 1024 80] [--reps 20] [--sweeps 150] [--out profiles/voidmap_step.json]

At B = 1, one synthetic sweep of --points rows (a ground disc and walls around a sensor 1.7 m up) on a --dims grid, it times with device
events, after a warm-up,

  * df_void_cast with the plain test before the atomic OR and without it (the entry's two async memsets of F and O included, and timed
    on their own next to it), with the number of free-bit sets the rays asked for and the bits that ended up set;
  * df_void_merge at the map's erosion radius, and df_void_query;
  * the two floors the numbers can be read against: attempted sets x 4 B over the chip-wide atomic rate for the cast, the bitset bytes
    the merge must move (F, O and V read once, V's changed words written) for the merge;

and labels a synthetic scene of --sweeps sweeps end to end (voidmap.label_sweeps: host transform, upload, integrate every sweep, query
every sweep, read the flags back), wall-clock.

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

from deflow_amd import voidmap
from deflow_amd._lib import call, ptr, stream

ATOMIC_RATE = 1.3e12       # bytes / s: the chip-wide rate of global atomics measured for the MI355X (float adds; taken as the yardstick
                           # for the integer OR, which was not measured on its own)


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


def synth_sweep(g, n, sensor, box_centre=None, reach=45.0):
    """a lidar-like sweep around `sensor`: 60 % ground returns (range uniform in 2 .. reach: denser near the sensor, as a spinning
    lidar's are), 40 % returns on walls 15 .. reach away, 0 .. 4 m up; optionally 300 rows on a 4 x 2 x 1.6 m box"""
    ng = int(0.6 * n)
    r, a = g.uniform(2.0, reach, ng), g.uniform(0, 2 * np.pi, ng)
    ground = np.stack([sensor[0] + r * np.cos(a), sensor[1] + r * np.sin(a), g.normal(0.0, 0.02, ng)], 1)
    nw = n - ng - (300 if box_centre is not None else 0)
    r, a = g.uniform(15.0, reach, nw), g.uniform(0, 2 * np.pi, nw)
    walls = np.stack([sensor[0] + r * np.cos(a), sensor[1] + r * np.sin(a), g.uniform(0.0, 4.0, nw)], 1)
    parts = [ground, walls]
    if box_centre is not None:
        parts.append(np.asarray(box_centre) + g.uniform(-0.5, 0.5, (300, 3)) * np.array([4.0, 2.0, 1.6]))
    return np.concatenate(parts).astype(np.float32)


def popcount(t):
    return int(np.unpackbits(t.cpu().view(torch.uint8).numpy()).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--voxel", type=float, default=0.1)
    ap.add_argument("--dims", type=int, nargs=3, default=[1024, 1024, 80])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "voidmap_step.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/voidmap_bench.py measures on the GPU"
    dev = torch.device("cuda")
    g = np.random.default_rng(20240117)
    Gx, Gy, Gz = a.dims
    gmin = (-0.5 * Gx * a.voxel, -0.5 * Gy * a.voxel, -3.0)
    sensor = np.array([0.0, 0.0, 1.7])
    pts = torch.from_numpy(synth_sweep(g, a.points, sensor)).to(dev)[None]
    cnt = torch.full((1,), a.points, dtype=torch.int32, device=dev)
    org = torch.from_numpy(sensor.astype(np.float32)).to(dev)[None]
    vm = voidmap.VoidMap(1, gmin, a.dims, a.voxel, device=dev)
    W = Gx * Gy * Gz // 32
    report = {"shape": {"batch": 1, "rows": a.points, "voxel": a.voxel, "dims": list(a.dims), "bitset_bytes": 4 * W},
              "hit_margin": vm.hit_margin, "erode": vm.erode, "max_range": vm.max_range, "device": torch.cuda.get_device_name(0)}

    # ---- the stages ----------------------------------------------------------------------------------------------------------------
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    attempts = torch.zeros(1, dtype=torch.int64, device=dev)
    grid = (*vm.grid_min, vm.k, *vm.dims)
    cast = lambda always=0, att=None: call("df_void_cast_probe", ptr(pts), ptr(cnt), ptr(org), 1, a.points, *grid, vm.hit_margin, vm.R, ptr(vm._f),
                                           ptr(vm._o), ptr(status), ptr(att), always, stream())
    merge = lambda: call("df_void_merge", ptr(vm._f), ptr(vm._o), ptr(vm._v), 1, *vm.dims, vm.erode, stream())
    flags = torch.empty(1, a.points, dtype=torch.int32, device=dev)
    query = lambda: call("df_void_query", ptr(pts), ptr(cnt), 1, a.points, *grid, ptr(vm._v), ptr(flags), stream())
    cast(0, attempts)
    n_att = int(attempts)
    free_bits, occ_bits = popcount(vm._f), popcount(vm._o)
    t_memset = timed(lambda: (vm._f.zero_(), vm._o.zero_()), a.reps)
    t_cast = timed(lambda: cast(0), a.reps)
    t_cast_always = timed(lambda: cast(1), a.reps)
    vm._v.zero_()
    t_merge_first = timed(lambda: (vm._v.zero_(), merge()), a.reps)          # every void word is new: V is written
    t_vzero = timed(lambda: vm._v.zero_(), a.reps)
    merge()
    t_merge = timed(merge, a.reps)                                           # the steady state of a standing sensor: V already holds the bits
    void_bits = popcount(vm._v)
    t_query = timed(query, a.reps)
    floor_cast = n_att * 4 / ATOMIC_RATE * 1e3
    merge_bytes = 3 * 4 * W
    report["stages"] = {
        "cast_ms": round(t_cast, 4), "cast_always_atomic_ms": round(t_cast_always, 4), "memset_F_O_ms": round(t_memset, 4),
        "merge_ms": round(t_merge, 4), "merge_into_empty_map_ms": round(t_merge_first - t_vzero, 4), "query_ms": round(t_query, 4),
        "attempted_sets": n_att, "free_bits": free_bits, "occupied_bits": occ_bits, "void_bits_after_one_sweep": void_bits,
        "attempted_sets_per_free_bit": round(n_att / max(free_bits, 1), 2), "flagged_rows": int((flags != 0).sum()), "status": int(status),
        "cast_floor_ms_attempted_sets_x4B_over_atomic_rate": round(floor_cast, 4), "atomic_rate_bytes_per_s": ATOMIC_RATE,
        "merge_floor_bytes": merge_bytes, "merge_achieved_GBps": round(merge_bytes / (t_merge * 1e-3) / 1e9, 1)}
    print(json.dumps(report["stages"]), flush=True)

    # ---- a synthetic scene end to end ------------------------------------------------------------------------------------------------
    lidars, poses = [], []
    for i in range(a.sweeps):
        pose = np.eye(4)
        pose[:3, 3] = (0.5 * i, 0.02 * i, 0.0)                               # 5 m/s at 10 Hz
        box_world = np.array([20.0 + 0.8 * i, 6.0, 0.8])                     # a vehicle ahead, slightly faster
        s = synth_sweep(g, a.points, np.array(voidmap.SENSOR_OFFSET), box_world - pose[:3, 3])      # in the vehicle frame of sweep i
        lidars.append(s)
        poses.append(pose)
    rep = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = voidmap.label_sweeps(lidars, poses, voxel=a.voxel, device=dev, report=rep)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rows = sum(len(o) for o in out)
    box = sum(int(o[-300:].sum()) for o in out)
    report["scene"] = {"sweeps": a.sweeps, "rows": rows, "seconds": round(dt, 3), "ms_per_sweep": round(dt / a.sweeps * 1e3, 3),
                       "dims": rep["dims"], "status": rep["status"], "flagged_fraction": round(sum(int(o.sum()) for o in out) / rows, 6),
                       "flagged_fraction_of_the_box_rows": round(box / (300 * a.sweeps), 4),
                       "flagged_fraction_of_the_static_rows": round((sum(int(o.sum()) for o in out) - box) / (rows - 300 * a.sweeps), 6)}
    print(json.dumps(report["scene"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
