"""What the sweep-to-sweep registration costs on the GPU, measured: usage  python tools/odometry_bench.py [--batch 16] [--points 80000]
[--grid 512] [--reps 20] [--map | --carve | --evict] [--out profiles/odometry_bench.json] [--plane-out profiles/odometry_plane_bench.json] [--parent-lib <libdeflow_amd.so>]

At the configs[2] cloud (80 000 rows per cloud, 512 x 512; ~70 000 rows in range: the compact pc0 / pc1 of a real forward, the clouds
tools/cluster_bench.py times), for B = 1 and B = --batch and stride 4 and 1, with device events after a warm-up (medians of --reps calls):

  * one df_reg_accumulate at T = identity and the first level's gate (max_dist 2.0), next to the yardstick timed on the same grid in the
    same run: df_chamfer_nn pc0 -> pc1 with the same gate -- the same search without the sums (and at every row: stride 1 is the like
    for like comparison);
  * one df_reg_solve;
  * a whole default ``odometry.register`` (two grid builds, 24 accumulate + solve pairs, the final accumulate).

The point-to-plane rows go to a file of their own (--plane-out; the rows and keys above stay as they are), same clouds, same method:

  * one df_normals of pc1 at the default radius, next to ITS yardstick, a DBSCAN core pass (df_dbscan_core, the entry
    tools/cluster_bench.py times) on the same filed cloud at eps = radius -- the same window (nn_search.h: nn_window), once stopping at min_pts rows as the
    clustering does and once walking every row of the window;
  * one df_reg_accumulate_plane, next to df_reg_accumulate of this library and, with --parent-lib, of the PARENT commit's library loaded
    beside it in the same process (the ratio is reported, not fixed in advance);
  * a whole default ``odometry.register`` with residual="point" and residual="plane".

--map [--map-out profiles/localmap_bench.json] measures the local map of the scan-to-map odometry INSTEAD (the files
above are not rewritten): the five stages of one update at the defaults on those clouds (B = 1), their sum, one df_nn_grid_build of the
same capacity + N rows as the yardstick, and a default ``register`` against a map view next to the scan-to-scan one.

--carve [--carve-out profiles/localmap_carve_bench.json] measures the carving of seen-through rows INSTEAD, on the
same clouds and the same map (B = 1, capacity 524 288, the cube and the margins at their defaults): df_map_view, df_depth_cube_build,
df_depth_cube_test and df_map_drop one by one, the four back to back, a whole ``LocalMap.carve`` (which also allocates), and the
yardsticks in the same process -- df_map_view over the same rows (the streaming floor of the test kernel) and the four stages of one
insert update.

--evict [--evict-out profiles/localmap_evict_bench.json] measures nearest-first eviction INSTEAD, in --map's setup
(B = 1, capacity 524 288, the map full, so the timed update overflows): the stages of one update with df_map_compact_near beside
df_map_compact -- the yardstick -- on the same stage tensors, and the update's sum with either policy.

A measuring tool, not a bench.py leg; needs the GPU (no fallback)."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import deflow_amd
from deflow_amd import chamfer, odometry
from deflow_amd import _lib as dflib
from deflow_amd._lib import call, ptr, stream
from deflow_amd.synth import synth_batch


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


def map_bench(a, dev, grid_range, pc0, c0, pc1, c1):
    """--map: the five stages of one local-map update at the defaults (B = 1), their sum, the yardstick -- one df_nn_grid_build of the
    same capacity + N rows -- and a default ``register`` against a map view of steady-state size next to the scan-to-scan one"""
    from deflow_amd.args import workspace
    from deflow_amd.localmap import LocalMap
    md = odometry.MAP_DEFAULTS
    lm = LocalMap(1, md["map_capacity"], voxel=md["map_voxel"], max_per_voxel=md["map_max_per_voxel"],
                  max_range=odometry.SCENE_DEFAULTS["max_range"], device=dev)
    pose = torch.eye(4, dtype=torch.float64, device=dev)[None].clone()
    fill = []
    for k in range(12):                                # the sensor moves 0.5 m per sweep: the window slides, voxels fill up to K
        lm.insert(pc0 if k % 2 == 0 else pc1, c0 if k % 2 == 0 else c1, pose)
        fill.append(int(lm.count))
        pose[0, 0, 3] += 0.5
    cap, N, W, K = lm.capacity, pc1.shape[1], lm.W, lm.max_per_voxel
    n, ncells = cap + N, lm.S * lm.S
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    cand, key, vz, idx, rng, keep = torch.empty(1, n, 3, dtype=torch.float64, device=dev), i32(n), i32(n), i32(n), i32(ncells, 2), i32(n)
    out, cnt, stat, dst = torch.empty_like(lm.points), i32(1), i32(1, 4), torch.empty(1, cap, 3, dtype=torch.float32, device=dev)
    ws, sws = workspace("df_map_ws_bytes", (1, cap, N), dev, "shape"), workspace("df_cell_sort_ws_bytes", (ncells,), dev, "shape")
    stages = {
        "keys": lambda: call("df_map_keys", ptr(lm.points), ptr(lm.count), ptr(pc1), ptr(c1), None, None, ptr(pose), 1, cap, N, lm.voxel, W,
                             ptr(cand), ptr(key), ptr(vz), stream()),
        "cell_sort": lambda: call("df_cell_sort", ptr(key), n, ncells, ptr(idx), ptr(rng), ptr(sws), stream()),
        "select": lambda: call("df_map_select", ptr(key), ptr(idx), ptr(rng), ptr(vz), 1, n, W, K, ptr(keep), stream()),
        "compact": lambda: call("df_map_compact", ptr(cand), ptr(idx), ptr(rng), ptr(keep), 1, cap, N, W, ptr(out), ptr(cnt), ptr(stat),
                                ptr(ws), stream()),
        "view": lambda: call("df_map_view", ptr(lm.points), ptr(lm.count), ptr(pose), 1, cap, ptr(dst), stream()),
    }
    ms = {k: timed(f, a.reps) for k, f in stages.items()}              # in order: each stage reads what the one before wrote
    both = torch.cat((dst, pc1), dim=1).contiguous()                  # the same capacity + N rows, as one fp32 cloud
    grid = chamfer.RowGrid(1, grid_range, odometry.DEFAULTS["cell"], dev)
    t_grid = timed(lambda: grid.file(both, i32(1).fill_(n)), a.reps)
    view, vcount = lm.view(pose)
    t_map = timed(lambda: odometry.register(pc1, c1, view, vcount, xy_range=grid_range), a.reps)
    t_scan = timed(lambda: odometry.register(pc0, c0, pc1, c1, xy_range=grid_range), a.reps)
    total = sum(ms.values())
    rep = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "capacity": cap, "sweep_rows": N, "sweep_valid_rows": int(c1),
           "voxel_m": lm.voxel, "max_per_voxel": K, "window_half_width": W, "map_rows_after_each_insert": fill,
           "map_rows_steady_state": fill[-1], "stat_of_the_timed_update": stat[0].tolist(),
           "stage_ms": {k: round(v, 4) for k, v in ms.items()}, "update_ms": round(total, 4),
           "nn_grid_build_same_rows_ms": round(t_grid, 4), "update_over_grid_build": round(total / t_grid, 3),
           "register_default_scan_ms": round(t_scan, 3), "register_default_map_view_ms": round(t_map, 3),
           "update_over_register_scan": round(total / t_scan, 3)}
    print(json.dumps(rep), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.map_out)), exist_ok=True)
    with open(a.map_out, "w") as f:
        json.dump(rep, f, indent=1)
    print("wrote", a.map_out)


def carve_bench(a, dev, pc0, c0, pc1, c1):
    """--carve: the four stages of one LocalMap.carve at the defaults (B = 1), their sequence, the wrapper, and the yardsticks"""
    from deflow_amd.args import workspace
    from deflow_amd.localmap import LocalMap
    md, cd = odometry.MAP_DEFAULTS, odometry.MAP_CARVE_DEFAULTS
    near = odometry.SCENE_DEFAULTS["min_range"]
    lm = LocalMap(1, md["map_capacity"], voxel=md["map_voxel"], max_per_voxel=md["map_max_per_voxel"],
                  max_range=odometry.SCENE_DEFAULTS["max_range"], device=dev)
    pose = torch.eye(4, dtype=torch.float64, device=dev)[None].clone()
    for k in range(12):                                # as --map: the sensor moves 0.5 m per sweep, the map reaches its steady state
        lm.insert(pc0 if k % 2 == 0 else pc1, c0 if k % 2 == 0 else c1, pose)
        pose[0, 0, 3] += 0.5
    cap, N, W, K, R = lm.capacity, pc1.shape[1], lm.W, lm.max_per_voxel, cd["map_carve_res"]
    n, ncells = cap + N, lm.S * lm.S
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    dst, img, flag = torch.empty(1, cap, 3, dtype=torch.float32, device=dev), i32(1, 6, R, R), i32(1, cap)
    out, cnt, stat, ws = torch.empty_like(lm.points), i32(1), i32(1, 2), workspace("df_map_drop_ws_bytes", (1, cap), dev, "shape")
    halo, margin, rel = cd["map_carve_halo"], cd["map_carve_margin"], cd["map_carve_rel"]
    stages = {
        "view": lambda: call("df_map_view", ptr(lm.points), ptr(lm.count), ptr(pose), 1, cap, ptr(dst), stream()),
        "build": lambda: call("df_depth_cube_build", ptr(pc1), ptr(c1), None, 1, N, R, ptr(img), stream()),
        "test": lambda: call("df_depth_cube_test", ptr(dst), ptr(lm.count), ptr(img), 1, cap, R, halo, margin, rel, near, ptr(flag), None,
                             stream()),
        "drop": lambda: call("df_map_drop", ptr(lm.points), ptr(lm.count), ptr(flag), None, 1, cap, ptr(out), ptr(cnt), ptr(stat), ptr(ws),
                             stream()),
    }
    ms = {k: timed(f, a.reps) for k, f in stages.items()}              # in order: each stage reads what the one before wrote
    t_seq = timed(lambda: [f() for f in stages.values()], a.reps)
    dropped = stat[0].tolist()
    state = (lm.points, lm._spare, lm.count)

    def whole():                                                       # the wrapper, every call from the same map
        lm.points, lm._spare, lm.count = state
        lm.carve(pc1, c1, pose, res=R, halo=halo, margin=margin, rel=rel, near=near)

    t_whole = timed(whole, a.reps)
    lm.points, lm._spare, lm.count = state
    cand, key, vz, idx, rng, keep = torch.empty(1, n, 3, dtype=torch.float64, device=dev), i32(n), i32(n), i32(n), i32(ncells, 2), i32(n)
    cnt4, stat4 = i32(1), i32(1, 4)
    mws, sws = workspace("df_map_ws_bytes", (1, cap, N), dev, "shape"), workspace("df_cell_sort_ws_bytes", (ncells,), dev, "shape")
    update = {
        "keys": lambda: call("df_map_keys", ptr(lm.points), ptr(lm.count), ptr(pc1), ptr(c1), None, None, ptr(pose), 1, cap, N, lm.voxel, W,
                             ptr(cand), ptr(key), ptr(vz), stream()),
        "cell_sort": lambda: call("df_cell_sort", ptr(key), n, ncells, ptr(idx), ptr(rng), ptr(sws), stream()),
        "select": lambda: call("df_map_select", ptr(key), ptr(idx), ptr(rng), ptr(vz), 1, n, W, K, ptr(keep), stream()),
        "compact": lambda: call("df_map_compact", ptr(cand), ptr(idx), ptr(rng), ptr(keep), 1, cap, N, W, ptr(out), ptr(cnt4), ptr(stat4),
                                ptr(mws), stream()),
    }
    ums = {k: timed(f, a.reps) for k, f in update.items()}
    total, utotal = sum(ms.values()), sum(ums.values())
    rep = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "capacity": cap, "map_rows": int(lm.count), "sweep_rows": N,
           "sweep_valid_rows": int(c1), "cube_res": R, "halo": halo, "margin_m": margin, "rel": rel, "near_m": near,
           "rows_tested_dropped": dropped, "stage_ms": {k: round(v, 4) for k, v in ms.items()}, "stages_sum_ms": round(total, 4),
           "stages_back_to_back_ms": round(t_seq, 4), "localmap_carve_call_ms": round(t_whole, 4),
           "map_view_same_rows_ms": round(ms["view"], 4), "test_over_map_view": round(ms["test"] / ms["view"], 3),
           "insert_update_stage_ms": {k: round(v, 4) for k, v in ums.items()}, "insert_update_ms": round(utotal, 4),
           "carve_over_insert_update": round(total / utotal, 3)}
    print(json.dumps(rep), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.carve_out)), exist_ok=True)
    with open(a.carve_out, "w") as f:
        json.dump(rep, f, indent=1)
    print("wrote", a.carve_out)


def evict_bench(a, dev, pc0, c0, pc1, c1):
    """--evict: the stages of one overflowing local-map update at the defaults (B = 1, the map full), with df_map_compact_near beside
    df_map_compact -- the yardstick, on the same stage tensors in the same process -- and the update's sum with either policy"""
    from deflow_amd.args import workspace
    from deflow_amd.localmap import LocalMap
    md = odometry.MAP_DEFAULTS
    lm = LocalMap(1, md["map_capacity"], voxel=md["map_voxel"], max_per_voxel=md["map_max_per_voxel"],
                  max_range=odometry.SCENE_DEFAULTS["max_range"], device=dev)
    pose = torch.eye(4, dtype=torch.float64, device=dev)[None].clone()
    for k in range(12):                                # as --map: the sensor moves 0.5 m per sweep; the map is full after nine sweeps
        lm.insert(pc0 if k % 2 == 0 else pc1, c0 if k % 2 == 0 else c1, pose)
        pose[0, 0, 3] += 0.5
    cap, N, W, K = lm.capacity, pc1.shape[1], lm.W, lm.max_per_voxel
    n, ncells = cap + N, lm.S * lm.S
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    cand, key, vz, idx, rng, keep = torch.empty(1, n, 3, dtype=torch.float64, device=dev), i32(n), i32(n), i32(n), i32(ncells, 2), i32(n)
    out, cnt, stat = torch.empty_like(lm.points), i32(1), i32(1, 4)
    out_n, cnt_n, stat_n, cut = torch.empty_like(lm.points), i32(1), i32(1, 4), i32(1, 2)
    ws, sws = workspace("df_map_ws_bytes", (1, cap, N), dev, "shape"), workspace("df_cell_sort_ws_bytes", (ncells,), dev, "shape")
    nws = workspace("df_map_near_ws_bytes", (1, cap, N, W), dev, "shape")
    stages = {
        "keys": lambda: call("df_map_keys", ptr(lm.points), ptr(lm.count), ptr(pc1), ptr(c1), None, None, ptr(pose), 1, cap, N, lm.voxel, W,
                             ptr(cand), ptr(key), ptr(vz), stream()),
        "cell_sort": lambda: call("df_cell_sort", ptr(key), n, ncells, ptr(idx), ptr(rng), ptr(sws), stream()),
        "select": lambda: call("df_map_select", ptr(key), ptr(idx), ptr(rng), ptr(vz), 1, n, W, K, ptr(keep), stream()),
        "compact": lambda: call("df_map_compact", ptr(cand), ptr(idx), ptr(rng), ptr(keep), 1, cap, N, W, ptr(out), ptr(cnt), ptr(stat),
                                ptr(ws), stream()),
        "compact_near": lambda: call("df_map_compact_near", ptr(cand), ptr(key), ptr(idx), ptr(rng), ptr(keep), 1, cap, N, W, ptr(out_n),
                                     ptr(cnt_n), ptr(stat_n), ptr(cut), ptr(nws), stream()),
    }
    ms = {k: timed(f, a.reps) for k, f in stages.items()}              # in order: each stage reads what the one before wrote
    ms["compact_again"] = timed(stages["compact"], a.reps)            # the yardstick once more, after the new form: the session's spread
    shared = ms["keys"] + ms["cell_sort"] + ms["select"]
    assert stat.tolist() == stat_n.tolist() and cnt.tolist() == cnt_n.tolist() == [cap], "the timed update must overflow"
    differ = int((out.view(torch.int64) != out_n.view(torch.int64)).any(dim=2).sum())
    rep = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "capacity": cap, "sweep_rows": N, "sweep_valid_rows": int(c1),
           "voxel_m": lm.voxel, "max_per_voxel": K, "window_half_width": W, "stat_of_the_timed_update": stat[0].tolist(),
           "cut_of_the_timed_update": cut[0].tolist(), "map_rows_that_differ_between_the_policies": differ,
           "stage_ms": {k: round(v, 4) for k, v in ms.items()}, "near_over_compact": round(ms["compact_near"] / ms["compact"], 3),
           "near_launches": 6, "compact_launches": 3, "update_ms_order": round(shared + ms["compact"], 4),
           "update_ms_near": round(shared + ms["compact_near"], 4), "cell_sort_share_of_update_near": round(ms["cell_sort"] / (shared + ms["compact_near"]), 3),
           "near_ws_bytes": int(call("df_map_near_ws_bytes", 1, cap, N, W)), "compact_ws_bytes": int(call("df_map_ws_bytes", 1, cap, N))}
    print(json.dumps(rep), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.evict_out)), exist_ok=True)
    with open(a.evict_out, "w") as f:
        json.dump(rep, f, indent=1)
    print("wrote", a.evict_out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evict", action="store_true", help="measure nearest-first eviction beside df_map_compact only (DESIGN.md section 6v)")
    ap.add_argument("--evict-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "localmap_evict_bench.json"))
    ap.add_argument("--carve", action="store_true", help="measure the carving of seen-through map rows only (DESIGN.md section 6u)")
    ap.add_argument("--carve-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "localmap_carve_bench.json"))
    ap.add_argument("--map", action="store_true", help="measure the local map of the scan-to-map odometry only (DESIGN.md section 6t)")
    ap.add_argument("--map-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                      "localmap_bench.json"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "odometry_bench.json"))
    ap.add_argument("--plane-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                        "odometry_plane_bench.json"))
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdeflow_amd.so: its df_reg_accumulate is the yardstick")
    a = ap.parse_args()
    parent_acc = None
    if a.parent_lib:
        parent_acc = ctypes.CDLL(os.path.abspath(a.parent_lib)).df_reg_accumulate
        parent_acc.argtypes, parent_acc.restype = dflib._SIGS["df_reg_accumulate"], ctypes.c_int
    assert torch.cuda.is_available(), "tools/odometry_bench.py measures on the GPU"
    dev = torch.device("cuda")
    H = a.grid
    half = 0.1 * H
    rng = [-half, -half, -3, half, half, 3]
    grid_range = (rng[0], rng[1], rng[3], rng[4])
    torch.manual_seed(0)
    m = deflow_amd.DeFlow(voxel_size=[0.2, 0.2, 6], point_cloud_range=rng, grid_feature_size=[H, H]).to(dev).train()
    with torch.no_grad():
        st = m.forward_padded(synth_batch(a.batch, a.points, seed=20240116, grid_hw=(H, H), device=dev))
    all0, all1 = st["p0"].points_c.contiguous(), st["p1"].points_c.contiguous()
    cnt0, cnt1 = st["p0"].counts.contiguous(), st["p1"].counts.contiguous()
    del m, st
    if a.evict:
        evict_bench(a, dev, all0[:1].contiguous(), cnt0[:1].contiguous(), all1[:1].contiguous(), cnt1[:1].contiguous())
        return
    if a.carve:
        carve_bench(a, dev, all0[:1].contiguous(), cnt0[:1].contiguous(), all1[:1].contiguous(), cnt1[:1].contiguous())
        return
    if a.map:
        map_bench(a, dev, grid_range, all0[:1].contiguous(), cnt0[:1].contiguous(), all1[:1].contiguous(), cnt1[:1].contiguous())
        return
    cell, max_dist = odometry.DEFAULTS["cell"], odometry.LEVELS[0]
    report = {"device": torch.cuda.get_device_name(0), "cell_m": cell, "max_dist_m": max_dist, "levels": list(odometry.LEVELS),
              "iters": odometry.DEFAULTS["iters"], "reps": a.reps, "cases": []}
    radius, min_pts, max_curv = (odometry.DEFAULTS[k] for k in ("normal_radius", "normal_min_pts", "normal_max_curv"))
    plane_report = {"device": report["device"], "cell_m": cell, "max_dist_m": max_dist, "levels": list(odometry.LEVELS),
                    "iters": odometry.DEFAULTS["iters"], "reps": a.reps, "normal_radius_m": radius, "normal_min_pts": min_pts,
                    "normal_max_curv": max_curv, "parent_lib": bool(parent_acc), "cases": []}
    for B in sorted({1, a.batch}):
        pc0, pc1, c0, c1 = all0[:B].contiguous(), all1[:B].contiguous(), cnt0[:B].contiguous(), cnt1[:B].contiguous()
        Ns, Nd = pc0.shape[1], pc1.shape[1]
        grid = chamfer.RowGrid(B, grid_range, cell, dev)
        minx, miny, G = grid.minx, grid.miny, grid.G
        (s_rng, s_rows), (d_rng, d_rows) = grid.file(pc0, c0), grid.file(pc1, c1)
        t_search = timed(lambda: grid.nn(pc0, c0, None, (d_rng, d_rows), max_dist ** 2), a.reps)
        nblk = (Ns + 255) // 256
        partial = torch.empty(call("df_reg_ws_bytes", B, Ns) // 8, dtype=torch.float64, device=dev)
        T = torch.eye(4, dtype=torch.float64, device=dev).repeat(B, 1, 1)
        log = torch.empty(B, 4, dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        for stride in (4, 1):
            t_acc = timed(lambda: call("df_reg_accumulate", ptr(s_rng), ptr(s_rows), G, ptr(d_rng), ptr(d_rows), minx, miny, cell, G, B, Ns,
                                       stride, ptr(T), max_dist ** 2, (max_dist / 3) ** 2, ptr(partial), None, None, None, None, stream()),
                          a.reps)
            t_solve = timed(lambda: call("df_reg_solve", ptr(partial), B, nblk, 50, 0, None, ptr(log), None, stream()), a.reps)
            t_reg = timed(lambda: odometry.register(pc0, c0, pc1, c1, xy_range=grid_range, stride=stride), a.reps)
            _, info = odometry.register(pc0, c0, pc1, c1, xy_range=grid_range, stride=stride)
            case = {"batch": B, "rows": Ns, "valid_rows": c0.tolist()[:4], "stride": stride, "chamfer_nn_same_gate_ms": round(t_search, 4),
                    "reg_accumulate_ms": round(t_acc, 4), "accumulate_over_chamfer_nn": round(t_acc / t_search, 3),
                    "reg_solve_ms": round(t_solve, 4), "register_default_ms": round(t_reg, 3), "inliers_at_identity": log[:4, 0].tolist(),
                    "status": info["status"].tolist()[:4], "final_log_sample0": info["log"][0, -1].tolist()}
            report["cases"].append(case)
            print(json.dumps(case), flush=True)
        # ---- point-to-plane --------------------------------------------------------------------------------------------------------
        nrm = torch.empty(B, Nd, 4, dtype=torch.float32, device=dev)
        normals = lambda: call("df_normals", ptr(d_rng), ptr(d_rows), minx, miny, cell, G, B, Nd, radius, min_pts, max_curv, ptr(nrm), None,
                               stream())
        t_normals = timed(normals, a.reps)
        ws = torch.empty(call("df_dbscan_ws_bytes", B, Nd), dtype=torch.uint8, device=dev)
        core = lambda k: call("df_dbscan_core", ptr(d_rng), ptr(d_rows), B, Nd, minx, miny, cell, G, radius, k, ptr(ws), stream())
        t_core, t_core_all = timed(lambda: core(min_pts), a.reps), timed(lambda: core(2 ** 30), a.reps)
        normals()
        valid = (nrm[..., 3] >= 0).sum(dim=1)
        for stride in (4, 1):
            acc_args = (ptr(T), max_dist ** 2, (max_dist / 3) ** 2, ptr(partial), None, None, None, None)
            t_point = timed(lambda: call("df_reg_accumulate", ptr(s_rng), ptr(s_rows), G, ptr(d_rng), ptr(d_rows), minx, miny, cell, G, B,
                                         Ns, stride, *acc_args, stream()), a.reps)
            t_plane = timed(lambda: call("df_reg_accumulate_plane", ptr(s_rng), ptr(s_rows), G, ptr(d_rng), ptr(d_rows), ptr(nrm), minx, miny,
                                         cell, G, B, Ns, Nd, stride, *acc_args, None, stream()), a.reps)
            call("df_reg_solve", ptr(partial), B, nblk, 50, 0, None, ptr(log), None, stream())
            inl = log[:4, 0].tolist()
            t_parent = None
            if parent_acc is not None:
                t_parent = timed(lambda: parent_acc(ptr(s_rng), ptr(s_rows), G, ptr(d_rng), ptr(d_rows), minx, miny, cell, G, B, Ns, stride,
                                                    *acc_args, stream()), a.reps)
            t_reg = {r: timed(lambda: odometry.register(pc0, c0, pc1, c1, xy_range=grid_range, stride=stride, residual=r), a.reps)
                     for r in odometry.RESIDUALS}
            _, info = odometry.register(pc0, c0, pc1, c1, xy_range=grid_range, stride=stride, residual="plane")
            case = {"batch": B, "rows": Ns, "valid_rows": c0.tolist()[:4], "stride": stride, "normals_ms": round(t_normals, 4),
                    "dbscan_core_eps_radius_ms": round(t_core, 4), "dbscan_core_whole_window_ms": round(t_core_all, 4),
                    "normals_over_core_whole_window": round(t_normals / t_core_all, 3), "normals_valid": valid.tolist()[:4],
                    "reg_accumulate_ms": round(t_point, 4), "reg_accumulate_plane_ms": round(t_plane, 4),
                    "plane_over_point": round(t_plane / t_point, 3),
                    "parent_reg_accumulate_ms": None if t_parent is None else round(t_parent, 4),
                    "plane_over_parent_point": None if t_parent is None else round(t_plane / t_parent, 3),
                    "register_point_ms": round(t_reg["point"], 3), "register_plane_ms": round(t_reg["plane"], 3),
                    "plane_inliers_at_identity": inl, "status": info["status"].tolist()[:4],
                    "final_log_sample0": info["log"][0, -1].tolist()}
            plane_report["cases"].append(case)
            print(json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", a.out)
    with open(a.plane_out, "w") as f:
        json.dump(plane_report, f, indent=1)
    print("wrote", a.plane_out)


if __name__ == "__main__":
    main()
