"""What the rigid cluster flow (model=icpflow) costs on the GPU, measured: usage
python tools/rigid_bench.py [--batch 1] [--points 80000] [--objects 100] [--reps 10] [--out profiles/rigid_flow.json]

Synthetic sweeps of --points rows each: --objects L-shaped surfaces of 100-1000 rows that move by up to 2 m along their heading between
the sweeps, four 9000-row walls (over max_cluster_points: status 3), the rest scattered singly (noise for DBSCAN).  Times, with device events after a
warm-up, ``rigid.rigid_cluster_flow`` as a whole and its stages: the joint DBSCAN labels, df_rigid_segments, df_rigid_vote, df_rigid_icp
and df_rigid_apply (each stage alone, on the previous stages' outputs).  A measuring tool, not a bench.py leg; needs the GPU."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from deflow_amd import rigid
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


def surface(rng, n, length, width=1.9, height=1.5):
    on_long = rng.random(n) < length / (length + width)
    u = rng.random(n)
    return np.stack([np.where(on_long, (u - 0.5) * length, -0.5 * length), np.where(on_long, -0.5 * width, (u - 0.5) * width),
                     rng.random(n) * height], axis=1)


def sweeps(rng, points, objects):
    side = int(math.ceil(math.sqrt(objects + 4)))
    step = 96.0 / side
    src, dst = [], []
    for i in range(objects + 4):
        c = np.array([-48.0 + step * (i % side + 0.5), -48.0 + step * (i // side + 0.5), 0.0])
        if i < 4:                                         # a wall: more rows than max_cluster_points
            for out in (src, dst):
                out.append(c + (rng.random((4500, 3)) - 0.5) * [min(step - 1.5, 12.0), 0.3, 3.0])
            continue
        h = rng.uniform(-math.pi, math.pi)
        R = np.array([[math.cos(h), -math.sin(h), 0], [math.sin(h), math.cos(h), 0], [0, 0, 1.0]])
        n0, n1, L = int(rng.integers(100, 1001)), int(rng.integers(100, 1001)), rng.uniform(4.4, min(6.0, step - 3.0))
        src.append(surface(rng, n0, L) @ R.T + c)
        dst.append(surface(rng, n1, L) @ R.T + c + R @ [rng.uniform(0.0, 2.0), 0.0, 0.0] + rng.normal(0, 0.01, (n1, 3)))
    out = []
    for rows in (np.concatenate(src), np.concatenate(dst)):
        rows = rows[:points]
        scatter = (rng.random((points - len(rows), 3)) - 0.5) * [100.0, 100.0, 2.0] + [0, 0, 6.0]      # far above: never in a cluster's reach
        rows = np.concatenate([rows, scatter])
        out.append(rows[rng.permutation(points)].astype(np.float32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--objects", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rigid_flow.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "tools/rigid_bench.py measures on the GPU"
    dev = torch.device("cuda")
    B, N = a.batch, a.points
    rng = np.random.default_rng(0)
    both = [sweeps(rng, N, a.objects) for _ in range(B)]
    pc0s = torch.from_numpy(np.stack([p[0] for p in both])).to(dev)
    pc1 = torch.from_numpy(np.stack([p[1] for p in both])).to(dev)
    cnt = torch.full((B,), N, dtype=torch.int32, device=dev)
    P = rigid.DEFAULTS
    K, R = rigid.kcap(N, N, P["min_cluster_size"]), rigid.vote_radius(P["max_disp"], P["vote_bin"])
    labels_of = lambda: rigid.joint_labels(pc0s, cnt, pc1, cnt, eps=P["eps"], min_points=P["min_points"], min_cluster_size=P["min_cluster_size"])
    labels = labels_of()
    flow, rid, table, vote, status = rigid.rigid_cluster_flow(pc0s, cnt, pc1, cnt, labels=labels)
    st = table[..., 7].long().flatten().bincount(minlength=6).tolist()
    res = {"batch": B, "points_per_sweep": N, "objects": a.objects, "slots": K, "device": torch.cuda.get_device_name(0),
           "status_counts": dict(zip(("empty", "registered", "one_sided", "too_large", "inlier_frac", "bounds"), st)),
           "registered_rows": int((rid > 0).sum()), "status_word": int(status.item())}
    seg_ws = torch.empty(int(call("df_rigid_segments_ws_bytes", B, N, N, K)) // 4 + 1, dtype=torch.int32, device=dev)
    icp_ws = torch.empty(int(call("df_rigid_icp_ws_bytes", B, N, N)) // 4 + 1, dtype=torch.int32, device=dev)
    seg_off = torch.empty(B, 2 * K + 1, dtype=torch.int32, device=dev)
    seg_rows = torch.empty(B, 2 * N, dtype=torch.int32, device=dev)
    sw = torch.zeros(1, dtype=torch.int32, device=dev)
    s = stream()
    stages = {
        "dbscan_joint_labels": labels_of,
        "df_rigid_segments": lambda: call("df_rigid_segments", ptr(labels), B, N, N, K, ptr(seg_off), ptr(seg_rows), ptr(sw), ptr(seg_ws), s),
        "df_rigid_vote": lambda: call("df_rigid_vote", ptr(pc0s), ptr(pc1), ptr(seg_off), ptr(seg_rows), B, N, N, K, P["min_side"],
                                      P["max_cluster_points"], P["vote_cap"], P["vote_bin"], R, ptr(vote), None, s),
        "df_rigid_icp": lambda: call("df_rigid_icp", ptr(pc0s), ptr(pc1), ptr(seg_off), ptr(seg_rows), ptr(vote), B, N, N, K, P["min_side"],
                                     P["max_cluster_points"], P["icp_cap"], P["icp_iters"], P["vote_bin"], P["icp_max_dist"],
                                     P["min_inlier_frac"], P["max_yaw"], P["max_disp"], ptr(table), ptr(icp_ws), s),
        "df_rigid_apply": lambda: call("df_rigid_apply", ptr(pc0s), ptr(cnt), ptr(labels), ptr(seg_off), ptr(seg_rows), ptr(table), B, N, N, K,
                                       ptr(flow), ptr(rid), s),
    }
    res["ms"] = {k: round(timed(fn, a.reps), 4) for k, fn in stages.items()}
    res["ms"]["rigid_cluster_flow"] = round(timed(lambda: rigid.rigid_cluster_flow(pc0s, cnt, pc1, cnt), a.reps), 4)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
