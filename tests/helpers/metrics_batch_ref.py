"""numpy float64 restatement of what deflow_amd.metrics_device.DeviceMetrics accumulates from PADDED batches -- TEST INFRASTRUCTURE ONLY.

Per update(): the gather by idx_c (compact row i < counts[b] -> point j = idx_c[b, i]; a j outside [0, N) drops the row and is counted),
est = fp32(pose_flow[j] + flow[i]), the masks (is_valid and eval_mask, each all-true when absent; categories clamped to 0..30, all 0 when
absent), the skip rule (a sample without has_eval_mask is left out iff some sample of the batch has one), the per-frame leaderboard
accumulation -- oracle/ref_metrics.py, frame by frame -- and the range-free summary: deflow_amd.metrics.epe_metrics restated on float64
copies, averaged per batch over the samples that have each key and weighted by the batch size, as eval.py does with evaluate_batch's
return.  Also the seeded batches both the CPU and the GPU test use (make_batch, boundary_batch)."""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

from oracle import ref_metrics as R

V1_KEYS = ("EPE_FD", "EPE_FS", "EPE_BS", "IoU", "EPE", "AccS", "AccR", "Angle")
SUMMARY_KEYS = ("EPE", "AccS", "AccR", "n", "EPE_FD", "EPE_FS", "EPE_BS", "EPE_3way")
META = tuple(R.BUCKETED_METACATEGORIES)
MASK_KEYS = ("is_valid", "eval_mask", "categories", "has_eval_mask")


def epe_summary(est: np.ndarray, gt: np.ndarray, pf: np.ndarray, fg: Optional[np.ndarray]) -> Dict[str, float]:
    """deflow_amd.metrics.epe_metrics, on float64 rows"""
    fin = np.isfinite(est).all(1) & np.isfinite(gt).all(1)
    est, gt, pf = est[fin], gt[fin], pf[fin]
    err = R.compute_end_point_error(est, gt)
    n = int(err.shape[0])
    out = {"EPE": float(err.mean()) if n else float("nan"),
           "AccS": float(R.compute_accuracy(est, gt, 0.05).mean()) if n else float("nan"),
           "AccR": float(R.compute_accuracy(est, gt, 0.10).mean()) if n else float("nan"), "n": n}
    dyn = np.linalg.norm(gt - pf, axis=-1) >= 0.05
    fg = np.ones(n, bool) if fg is None else np.asarray(fg, bool)[fin]
    m = lambda sel: float(err[sel].mean()) if sel.any() else float("nan")
    out.update({"EPE_FD": m(fg & dyn), "EPE_FS": m(fg & ~dyn), "EPE_BS": m(~fg & ~dyn)})
    vals = [v for v in (out["EPE_FD"], out["EPE_FS"], out["EPE_BS"]) if v == v]
    out["EPE_3way"] = sum(vals) / len(vals) if vals else float("nan")
    return out


def frames(batch: dict):
    """-> (dropped rows, [per evaluated sample: est, pose_flow, pc0, gt (float64 [M,3]), ok bool [M], cats int [M], cats given])"""
    flow, pose, pc0, gt = (np.asarray(batch[k], np.float32) for k in ("flow", "pose_flow", "pc0", "gt_flow"))
    idx_c, counts = np.asarray(batch["idx_c"], np.int64), np.asarray(batch["counts"])
    B, N = flow.shape[:2]
    has = batch.get("has_eval_mask")
    skip = ~np.asarray(has, bool) if has is not None and np.asarray(has, bool).any() else np.zeros(B, bool)
    dropped, out = 0, []
    for b in range(B):
        c = int(min(max(int(counts[b]), 0), N))
        j = idx_c[b, :c]
        inr = (j >= 0) & (j < N)
        dropped += int((~inr).sum())
        if skip[b]:
            continue
        j = j[inr]
        with np.errstate(all="ignore"):
            est = (pose[b, j] + flow[b, :c][inr]).astype(np.float32)              # one rounded fp32 add
        ok = np.ones(j.shape[0], bool)
        for k in ("is_valid", "eval_mask"):
            if batch.get(k) is not None:
                ok &= np.asarray(batch[k])[b, j] != 0
        given = batch.get("categories") is not None
        cats = np.clip(np.asarray(batch["categories"]).astype(np.int64)[b, j], 0, 30) if given else np.zeros(j.shape[0], np.int64)
        out.append((est.astype(np.float64), pose[b, j].astype(np.float64), pc0[b, j, :3].astype(np.float64), gt[b, j].astype(np.float64),
                    ok, cats, given))
    return dropped, out


class BatchRef:
    """the accumulator: update(batch) per padded batch (a dict of numpy arrays under DeviceMetrics.update's argument names)"""

    def __init__(self):
        self.om = R.OfficialMetrics()
        self.tot: Dict[str, float] = {}
        self.wsum: Dict[str, int] = {}
        self.dropped = 0
        self.n = 0

    def update(self, batch: dict) -> None:
        dropped, fr = frames(batch)
        self.dropped += dropped
        acc: Dict[str, list] = {}
        for est, pf, pc, gt, ok, cats, given in fr:
            v1 = R.evaluate_leaderboard(est, pf, pc, gt, ok, cats)
            self.om.step(v1, R.evaluate_leaderboard_v2(est, pf, pc, gt, ok, cats))
            self.n += int(v1["n"])
            for k, v in epe_summary(est[ok], gt[ok], pf[ok], (cats != 0)[ok] if given else None).items():
                if v == v:
                    acc.setdefault(k, []).append(v)
        w = int(np.asarray(batch["flow"]).shape[0])
        for k, v in acc.items():
            self.tot[k] = self.tot.get(k, 0.0) + sum(v) / len(v) * w
            self.wsum[k] = self.wsum.get(k, 0) + w

    def result(self, version: int) -> Dict[str, float]:
        return self.om.result(version)

    def summary(self) -> Dict[str, float]:
        return {k: self.tot[k] / self.wsum[k] for k in self.tot}

    def integers(self) -> Dict[str, np.ndarray]:
        """everything DeviceMetrics holds as an integer: n, the 5 x 51 counts, how many frames had each version-1 value, the summary's
        weights"""
        return {"n": np.array([self.n], np.int64), "count": np.stack([self.om.count[c] for c in META]).astype(np.int64),
                "v1_cnt": np.array([len(self.om.v1.get(k, [])) for k in V1_KEYS], np.int64),
                "wsum": np.array([self.wsum.get(k, 0) for k in SUMMARY_KEYS], np.int64)}


def same(want: dict, got: dict, tol: float = 1e-9) -> None:
    """the same keys; NaN where NaN; floats within tol relative and absolute (Angle 1e-7: arccos at 1, tests/test_metrics.py); n exact"""
    assert set(want) == set(got), (sorted(want), sorted(got))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, float) and math.isnan(w):
            assert math.isnan(g), (k, g)
        elif k == "n" and float(w) == int(w):
            assert g == w, (k, g, w)
        else:
            t = max(tol, 1e-7) if k == "Angle" else tol
            assert abs(g - w) <= t * max(1.0, abs(w)), (k, g, w)


# ---- the seeded batches ------------------------------------------------------------------------------------------------------------------
CATS = np.array([0, 0, 0, 0, 1, 19, 19, 6, 17, 3, 30, 21, 2, 23, 14])       # category 0, an unevaluated one (1, 21), all five meta-classes
SEEDS = (101, 102, 103)                                                     # the three batches of the main GPU test


def make_batch(seed: int, rpb: int, *, masks=("is_valid", "eval_mask", "categories"), has="mixed") -> dict:
    """B = 6, N = 2 rpb + 40, counts {0, 1, rpb - 1, rpb, rpb + 1, 2 rpb + 7} in a seeded order; idx_c a random injective map per sample
    (garbage beyond counts, which nobody may read); NaN rows in each of the four inputs; points on both sides of 35 m (box and radius);
    speeds 0 (static), around the 0.05 threshold, across the buckets and beyond 2.0"""
    g = np.random.default_rng(seed)
    B, N = 6, 2 * rpb + 40
    counts = g.permutation(np.array([0, 1, rpb - 1, rpb, rpb + 1, 2 * rpb + 7])).astype(np.int32)
    pc0 = g.normal(0, 22, (B, N, 3)) * [1, 1, 0.1]
    pose = g.normal(0, 0.3, (B, 1, 3)) + 0.01 * pc0[..., [1, 0, 2]] * [-1, 1, 0]
    u = g.random((B, N, 1))
    motion = np.where(u < 0.5, 0.0, np.where(u < 0.65, g.normal(0, 0.03, (B, N, 3)), np.where(u < 0.9, g.normal(0, 0.6, (B, N, 3)),
                                                                                              g.normal(0, 2.5, (B, N, 3)))))
    pose = pose.astype(np.float32)
    gt = (pose + motion.astype(np.float32)).astype(np.float32)               # static rows: gt == pose_flow exactly
    est_flow = (gt - pose) + (g.normal(0, 0.08, (B, N, 3)) * (g.random((B, N, 1)) < 0.7)).astype(np.float32)
    idx_c = np.full((B, N), -7, np.int64)
    flow = np.full((B, N, 3), np.nan, np.float32)
    for b in range(B):
        c = int(counts[b])
        idx_c[b, :c] = g.permutation(N)[:c]
        flow[b, :c] = est_flow[b, idx_c[b, :c]]
    pc0, gt = pc0.astype(np.float32), gt.copy()
    big = int(np.argmax(counts))
    j = idx_c[big, :int(counts[big])]
    flow[big, 5, 1] = np.nan
    pose[big, j[17], 0] = np.nan
    pc0[big, j[29], 2] = np.nan
    pc0[big, j[31], 0] = np.inf
    gt[big, j[43]] = np.nan
    flow[big, 77, 2] = np.inf
    out = {"flow": flow, "pose_flow": pose, "pc0": pc0, "gt_flow": gt, "idx_c": idx_c, "counts": counts}
    if "is_valid" in masks:
        out["is_valid"] = g.random((B, N)) < 0.9
    if "eval_mask" in masks:
        out["eval_mask"] = g.random((B, N)) < 0.8
    if "categories" in masks:
        out["categories"] = CATS[g.integers(0, len(CATS), (B, N))].astype(np.uint8)
    if has is not None:
        out["has_eval_mask"] = {"mixed": np.array([1, 0, 1, 1, 0, 1], bool), "all": np.ones(B, bool), "none": np.zeros(B, bool)}[has]
    return out


def boundary_batch() -> dict:
    """B = 1: fp32 values for which every intermediate is exact, on every threshold the definitions have.  pose_flow = 0, so est = flow."""
    f = np.float32
    below = lambda v: np.nextafter(f(v), f(0))
    rows = [  # pc0 xy, gt, est - gt, category
        ((35, 35), (1.0, 0, 0), (0, 0, 0), 19),                       # box corner (in), radius 49.5 (out); speed 1.0 = edge 25
        ((21, 28), (1.0, 0, 0), (0, 0, 0), 19),                       # radius exactly 35 (in); bucket 25
        ((np.nextafter(f(35), f(36)), 0), (0, 0, 0), (0, 0, 0), 0),   # a hair outside both
        ((0, 35), (0, 0, 0), (0.25, 0, 0), 0),                        # speed 0: bucket 0
        ((1, 1), (0, 2.0, 0), (0, 0, 0), 17),                         # speed 2.0: the open bucket
        ((1, 2), (below(2.0), 0, 0), (0, 0, 0), 3),                   # bucket 49
        ((2, 1), (f(0.05), 0, 0), (0, 0, 0), 6),                      # fp32(0.05) >= 0.05: dynamic, bucket 1
        ((2, 2), (below(0.05), 0, 0), (0, 0, 0), 6),                  # its predecessor: static, bucket 1
        ((3, 1), (3, 4, 0), (0, 0, 0.5), 19),                         # error exactly 0.5, |gt| = 5: relative 0.1 / (1 + 2e-11) < 0.10
        ((3, 2), (0, 0, 0), (0, f(0.05), 0), 0),                      # estimated dynamic, labelled static: a false positive
        ((3, 3), (0, f(0.05), 0), (0, -f(0.05), 0), 30),              # the other way round: a false negative
        ((-35, -35), (0.04 * 0 + 0.5, 0, 0), (0.125, 0, 0), 1),       # an unevaluated category: version 1 only
    ]
    n = len(rows)
    pc0 = np.zeros((1, n, 3), f)
    gt = np.zeros((1, n, 3), f)
    flow = np.zeros((1, n, 3), f)
    cats = np.zeros((1, n), np.uint8)
    for i, (xy, g_, d, c) in enumerate(rows):
        pc0[0, i, :2] = xy
        gt[0, i] = g_
        flow[0, i] = gt[0, i] + np.asarray(d, f)
        cats[0, i] = c
    return {"flow": flow, "pose_flow": np.zeros((1, n, 3), f), "pc0": pc0, "gt_flow": gt, "idx_c": np.arange(n, dtype=np.int64)[None],
            "counts": np.array([n], np.int32), "categories": cats}
