"""Integer restatement of the nearest-first eviction of include/deflow_amd.h / DESIGN.md section 6v -- df_map_compact_near -- one sample
at a time, with Python ints and a dict of ring counts: "the rings that fit, then a budget".  No code shared with the kernels and none
with ``deflow_amd.localmap``; keys, select, the sorted order and the view are map_ref's, which this file leaves as it is.
``register_sweeps_map`` is map_ref's scan-to-map loop with ``insert`` swapped for the one below."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_ref  # noqa: E402
import reg_ref  # noqa: E402


def ring_of(key: int, W: int, b: int = 0) -> int:
    """Chebyshev distance of the window column of key = (b S + dy) S + dx from the anchor column (W, W)"""
    S = 2 * W + 1
    local = int(key) - b * S * S
    dy, dx = divmod(local, S)
    assert 0 <= dy < S
    return max(abs(dx - W), abs(dy - W))


def cut_of(rings, cap: int, W: int):
    """rings: the ring of every kept candidate -> (R, budget); (W + 1, 0) when they all fit"""
    h = {}
    for r in rings:
        h[r] = h.get(r, 0) + 1
    if sum(h.values()) <= cap:
        return W + 1, 0
    inside, R = 0, 0
    while R < W and inside + h.get(R, 0) <= cap:          # the largest R in 0 .. W with sum_{r < R} h[r] <= cap
        inside += h.get(R, 0)
        R += 1
    return R, cap - inside


def compact_near(cand, key, keep, drop, cap, W, b=0):
    """-> map [cap,3] f64 with a NaN tail, count, stat (map_ref.compact's four), cut = (R, budget)"""
    order = map_ref.sorted_order(key, drop)
    kept = [int(c) for c in order if keep[c]]
    rings = [ring_of(key[c], W, b) for c in kept]
    R, budget = cut_of(rings, cap, W)
    out = np.full((cap, 3), map_ref.NAN64)
    at = partial = 0
    for c, r in zip(kept, rings):
        if r == R:
            partial += 1
        if r < R or (r == R and partial <= budget):
            out[at] = cand[c]
            at += 1
    assert at == min(len(kept), cap)
    return out, at, (len(order), len(kept), sum(1 for c in kept if c >= cap), max(0, len(kept) - cap)), (R, budget)


def insert(map_pts, count, sweep, sweep_count, pose, voxel, W, K, mask=None, gate=None):
    """one update of one sample under evict="near" -> (map, count, stat, cut)"""
    cap = map_pts.shape[0]
    cand, key, vz = map_ref.keys(map_pts, count, sweep, sweep_count, mask, gate, pose, voxel, W)
    drop = (2 * W + 1) ** 2
    return compact_near(cand, key, map_ref.select(key, vz, drop, K), drop, cap, W)


def register_sweeps_map(sweeps, levels, *, voxel, K, cap, W, evict="near", min_inliers=50, init="previous", gaps=False):
    """map_ref.register_sweeps_map with the update of ``evict``: "near" (the insert above) or "order" (map_ref.insert) -> the same dict,
    plus cuts = (R, budget) after every sweep under "near" """
    def ins(m, cnt, s, pose, gate=None):
        if evict == "near":
            return insert(m, cnt, s, len(s), pose, voxel, W, K, gate=gate)
        return (*map_ref.insert(m, cnt, s, len(s), pose, voxel, W, K, gate=gate), None)

    pose, start = np.eye(4), np.eye(4)
    m, cnt, stat, cut = ins(np.full((cap, 3), map_ref.NAN64), 0, sweeps[0], pose)
    out = dict(poses=[pose], M=[], status=[], maps=[(m, cnt, stat)], gap=[], cuts=[cut])
    plan = [d for d, n in levels for _ in range(n)]
    for s in sweeps[1:]:
        dst = map_ref.view(m, cnt, pose)
        used, dok = reg_ref.used_rows(s, len(s)), reg_ref.participating(dst, cnt)
        T, status = start.copy(), 2
        for it, max_dist in enumerate(plan):
            if gaps and it == len(plan) - 1:
                out["gap"].append(map_ref.two_nearest_gap(s[used].astype(np.float64) @ T[:3, :3].T + T[:3, 3], dst, dok))
            T, status, _ = reg_ref.iterate(T, s, used, dst, dok, max_dist, min_inliers)
        if status != 0:
            T = start.copy()
        pose = pose @ T
        m, cnt, stat, cut = ins(m, cnt, s, pose, gate=status)
        out["poses"].append(pose), out["M"].append(T), out["status"].append(status), out["maps"].append((m, cnt, stat)), out["cuts"].append(cut)
        if init == "previous":
            start = T
    return out


# ---- the loop scene under overflow ------------------------------------------------------------------------------------------------------
# map_ref's loop scene with nodes = 700 (17 sweeps of 489 rows) and a capacity every update overflows.  The GPU's poses are compared with
# this restatement's only where, at the last iteration of every sweep, the nearest and second-nearest map row of every used row differ
# by >= 1e-4 m on the reference alone (map_ref.LOOP_SEED's condition).  Searched on the CPU under evict="near", K = 1: see the figures
# tests/test_localmap_evict_cpu.py prints and asserts for EVICT_SEED, EVICT_CAP.
EVICT_SEED, EVICT_CAP = 3, 450
