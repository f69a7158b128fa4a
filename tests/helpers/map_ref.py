"""Integer and float64 restatement of the local map of include/deflow_amd.h / DESIGN.md section 6t -- keys, select, compact, view -- one
sample at a time, with Python floats (every operation rounded once), a dict of voxels and Python loops: no code shared with the kernels
and none with ``deflow_amd.localmap``.  ``register_sweeps_map`` is the scan-to-map loop of ``odometry.register_sweeps(target="map")`` on
reg_ref's float64 registration (stride 1), and ``loop_scene`` the closed-loop recording the map tests register."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reg_ref  # noqa: E402

LIMIT = 2 ** 30
NAN64 = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), dtype=np.float64)[0]
NAN32 = np.frombuffer(np.uint32(0x7FC00000).tobytes(), dtype=np.float32)[0]


def voxel_of(w: float, voxel: float):
    """floor(w / voxel) as a Python int, None where w is not finite or the index is not inside (-2^30, 2^30)"""
    if not math.isfinite(w):
        return None
    q = w / voxel
    if not math.isfinite(q):
        return None
    v = math.floor(q)
    return v if abs(v) < LIMIT else None


def keys(map_pts, count, sweep, sweep_count, mask, gate, pose, voxel, W, b=0, B=1):
    """-> cand [n,3] f64, key [n] int64 (B S S: dropped), vz [n] int64 of sample b of B"""
    map_pts, sweep, pose = np.asarray(map_pts, dtype=np.float64), np.asarray(sweep, dtype=np.float32), np.asarray(pose, dtype=np.float64)
    cap, N = map_pts.shape[0], sweep.shape[0]
    S = 2 * W + 1
    drop = B * S * S
    R = [[float(pose[i, j]) for j in range(4)] for i in range(3)]
    voxel = float(voxel)
    anchor = (voxel_of(R[0][3], voxel), voxel_of(R[1][3], voxel))
    cand = np.full((cap + N, 3), NAN64)
    key = np.full(cap + N, drop, dtype=np.int64)
    vz = np.zeros(cap + N, dtype=np.int64)
    for r in range(cap + N):
        if r < cap:
            if not r < int(count):
                continue
            w = [float(v) for v in map_pts[r]]
        else:
            s = r - cap
            if not s < int(sweep_count) or (mask is not None and not int(mask[s]) > 0) or (gate is not None and int(gate) != 0):
                continue
            x, y, z = (float(v) for v in sweep[s])
            if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
                continue
            w = []
            for i in range(3):
                a = R[i][0] * x
                a = a + R[i][1] * y
                a = a + R[i][2] * z
                w.append(a + R[i][3])
        v = [voxel_of(c, voxel) for c in w]
        if None in v or None in anchor:
            continue
        dx, dy = v[0] - anchor[0] + W, v[1] - anchor[1] + W
        if not (0 <= dx <= 2 * W and 0 <= dy <= 2 * W):
            continue
        cand[r], key[r], vz[r] = w, (b * S + dy) * S + dx, v[2]
    return cand, key, vz


def sorted_order(key, drop) -> np.ndarray:
    """the candidates with key < drop by ascending key, equal keys by ascending index: what the stable sort leaves"""
    return np.array(sorted((int(k), c) for c, k in enumerate(key) if k < drop), dtype=np.int64).reshape(-1, 2)[:, 1]


def select(key, vz, drop, K) -> np.ndarray:
    """keep [n] int: a voxel (key, vz) keeps its first K candidates in candidate order -- a dict of voxel -> rows seen so far"""
    seen, keep = {}, np.zeros(len(key), dtype=np.int32)
    for c in range(len(key)):
        if key[c] >= drop:
            continue
        vox = (int(key[c]), int(vz[c]))
        keep[c] = 1 if seen.get(vox, 0) < K else 0
        seen[vox] = seen.get(vox, 0) + 1
    return keep


def compact(cand, key, keep, drop, cap):
    """-> map [cap,3] f64 with a NaN tail, count, stat = (rows in the window, kept, kept rows from the sweep, overflow)"""
    order = sorted_order(key, drop)
    kept = [int(c) for c in order if keep[c]]
    out = np.full((cap, 3), NAN64)
    for at, c in enumerate(kept[:cap]):
        out[at] = cand[c]
    return out, min(len(kept), cap), (len(order), len(kept), sum(1 for c in kept if c >= cap), max(0, len(kept) - cap))


def insert(map_pts, count, sweep, sweep_count, pose, voxel, W, K, mask=None, gate=None):
    """one update of one sample -> (map, count, stat)"""
    cap = map_pts.shape[0]
    cand, key, vz = keys(map_pts, count, sweep, sweep_count, mask, gate, pose, voxel, W)
    drop = (2 * W + 1) ** 2
    return compact(cand, key, select(key, vz, drop, K), drop, cap)


def view(map_pts, count, pose) -> np.ndarray:
    """[cap,3] fp32: R^T (w - t) in float64, each operation rounded once, then to fp32; rows >= count are NaN (0x7FC00000)"""
    m, T = np.asarray(map_pts, dtype=np.float64), np.asarray(pose, dtype=np.float64)
    out = np.full(m.shape, NAN32, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = [m[:, i] - T[i, 3] for i in range(3)]
        for j in range(3):
            o = (T[0, j] * d[0] + T[1, j] * d[1]) + T[2, j] * d[2]
            out[:int(count), j] = o.astype(np.float32)[:int(count)]
    return out


def two_nearest_gap(q, dst, ok) -> float:
    """the smallest difference between the distances of a row of q to its nearest and to its second-nearest participating row of dst"""
    rows = dst[ok].astype(np.float64)
    if rows.shape[0] < 2 or q.shape[0] == 0:
        return math.inf
    d = np.sqrt(((q[:, None, :] - rows[None]) ** 2).sum(axis=2))
    d.partition(1, axis=1)
    return float((d[:, 1] - d[:, 0]).min())


def register_sweeps_map(sweeps, levels, *, voxel, K, cap, W, min_inliers=50, init="previous", gaps=False, stop_below=None):
    """sweeps: fp32 arrays [N_i,3], every row taking part.  -> dict: poses (float64 [4,4] per sweep), M (per later sweep), status,
    maps = (map, count, stat) after every sweep, gap = per later sweep two_nearest_gap at the state of its last iteration (gaps=True)"""
    pose, start = np.eye(4), np.eye(4)
    m, cnt, stat = insert(np.full((cap, 3), NAN64), 0, sweeps[0], len(sweeps[0]), pose, voxel, W, K)
    out = dict(poses=[pose], M=[], status=[], maps=[(m, cnt, stat)], gap=[])
    plan = [d for d, n in levels for _ in range(n)]
    for s in sweeps[1:]:
        dst = view(m, cnt, pose)
        used, dok = reg_ref.used_rows(s, len(s)), reg_ref.participating(dst, cnt)
        T, status = start.copy(), 2
        for it, max_dist in enumerate(plan):
            if gaps and it == len(plan) - 1:
                out["gap"].append(two_nearest_gap(s[used].astype(np.float64) @ T[:3, :3].T + T[:3, 3], dst, dok))
                if stop_below is not None and out["gap"][-1] < stop_below:
                    return None                                        # (a seed search: this scene fails the condition)
            T, status, _ = reg_ref.iterate(T, s, used, dst, dok, max_dist, min_inliers)
        if status != 0:
            T = start.copy()
        pose = pose @ T
        m, cnt, stat = insert(m, cnt, s, len(s), pose, voxel, W, K, gate=status)
        out["poses"].append(pose), out["M"].append(T), out["status"].append(status), out["maps"].append((m, cnt, stat))
        if init == "previous":
            start = T
    return out


def register_sweeps_scan(sweeps, levels, *, min_inliers=50, init="previous"):
    """the scan-to-scan loop of odometry.register_sweeps on reg_ref.register -> poses"""
    start, poses = np.eye(4), [np.eye(4)]
    for a, b in zip(sweeps, sweeps[1:]):
        T, status = reg_ref.register(a, len(a), b, len(b), levels, init=start, min_inliers=min_inliers)
        if status != 0:
            T = start.copy()
        poses.append(poses[-1] @ np.linalg.inv(T))
        if init == "previous":
            start = T
    return poses


# ---- the loop scene ---------------------------------------------------------------------------------------------------------------------
LOOP = dict(sweeps=17, nodes=700, frac=0.7, noise=0.01, radius=0.7, levels=((1.0, 6), (0.5, 6)), voxel=0.5, max_range=51.2)
LOOP_W = math.ceil(LOOP["max_range"] / LOOP["voxel"]) + 1
# the seed the tests take.  Seeds 0 and 1 give the same accuracy figures but fail the tests' condition that, at the last iteration of
# every sweep, the nearest and the second-nearest map row of every used row differ by >= 1e-4 m in distance (K = 1: 4.8e-5 and 1.5e-5
# at worst); seed 2 holds it with 1.35e-4.  With K > 1 no seed can: a voxel then holds several noisy copies of one node, about 1 cm
# apart, and among thousands of rows some are nearly equidistant from two of them.
LOOP_SEED, LOOP_NODES = 2, LOOP["nodes"]


def loop_truth(k: int, n: int = LOOP["sweeps"]) -> np.ndarray:
    """pose of sweep k: on a circle of radius 0.7 m through the origin with a little yaw, back at the identity at k = n - 1"""
    th = 2.0 * math.pi * k / (n - 1)
    T = reg_ref.se3_exp((0.0, 0.0, 0.02 * math.sin(th), 0.0, 0.0, 0.0))
    T[:3, 3] = (LOOP["radius"] * (math.cos(th) - 1.0), LOOP["radius"] * math.sin(th), 0.0) if k != n - 1 else (0.0, 0.0, 0.0)
    return T if k != n - 1 else np.eye(4)


def loop_scene(seed: int = 0, n: int = LOOP["sweeps"], nodes: int = LOOP["nodes"]):
    """-> (sweeps, truth): n fp32 sweeps of reg_ref.lattice(700, seed) seen from loop_truth(k): a random 70 % of the nodes plus 1 cm of
    noise each; the last sweep is a row-permuted copy of sweep 0"""
    world = reg_ref.lattice(nodes, seed).astype(np.float64)
    rng = np.random.default_rng(1000 + seed)
    sweeps, truth = [], []
    for k in range(n - 1):
        T = loop_truth(k, n)
        pick = np.sort(rng.choice(world.shape[0], size=int(LOOP["frac"] * world.shape[0]), replace=False))
        p = (world[pick] - T[:3, 3]) @ T[:3, :3] + rng.normal(0.0, LOOP["noise"], size=(pick.shape[0], 3))
        sweeps.append(p.astype(np.float32))
        truth.append(T)
    sweeps.append(sweeps[0][rng.permutation(sweeps[0].shape[0])].copy())
    truth.append(np.eye(4))
    return sweeps, truth
