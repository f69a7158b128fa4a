"""Per-pair flow optimised on a GPU distance transform with a per-cluster rigidity term (``model=mbnsf``): ``fastnsf``'s loop -- one small
coordinate MLP per pair of sweeps against a lookup in the distance transform of the second sweep -- plus a penalty on every change of the
distances between rows of one cluster of the first sweep, so that the rows of one body move together.  No weights and no checkpoint.

UNPINNED: the idea is MBNSF's multi-body regulariser (Vidanapathirana et al., 3DV'24), but upstream's source is absent and was not read;
every choice here is this project's own.  The definition is in DESIGN.md section 6m and include/deflow_amd.h; tests/helpers/iso_ref.py
restates it in torch.  The clusters come from ``cluster.dbscan`` once per pair, their ordered row lists from df_rigid_segments, the
neighbour table and the term from csrc/iso.hip; everything else is ``fastnsf.optimize_net``, handed the term, on ``pairopt``'s loop.

CUDA tensors only, like the rest of the library: there is no CPU fallback.  The loop makes no host decision, so one iteration can be
captured as a HIP graph (``graph=True``): a linear chain on one stream."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

from . import fastnsf, pairflow
from ._lib import call, ptr, stream
from .args import integer, merged, nonneg, positive, tensor as _tensor
from .fastnsf import FastNsf, dt_grid, optimize_net
from .pairopt import pair_clouds, rows, sample_sum
from .rigid import segments

P_MAX = 16               # pairs per row (csrc/iso.hip: ISO_PMAX)

# every default of section 6m: fastnsf's ten, then the term's and the clustering's; all of them are arguments of mbnsf_optimize and MbNsf,
# and `mbnsf_<name>=` keys of the commands
DEFAULTS: Dict[str, object] = {**fastnsf.DEFAULTS, "rigid_weight": 10.0, "rigid_pairs": 4, "rigid_delta": 0.2, "eps": 0.7, "min_points": 4,
                               "min_cluster_size": 20, "max_cluster_points": 8192}
COMMAND_KEYS: Dict[str, str] = {"mbnsf_" + k: k for k in DEFAULTS}
# default batch_size of the commands: fastnsf's peak per sample (about 0.9 GB at the defaults and 80 000 rows) plus the neighbour table,
# N x 2 rigid_pairs x 8 bytes (5 MB)
COMMAND_BATCH_SIZE = 4


def params_from_command(given: Dict[str, str]) -> Dict[str, object]:
    return pairflow.params_from_command(pairflow.entry("mbnsf"), given)


def check_params(p: Dict[str, object]) -> Dict[str, object]:
    """validated copy of a parameter dict (ValueError naming the argument); launches nothing"""
    fn = "mbnsf_optimize"
    out = merged(fn, DEFAULTS, p)
    out.update(fastnsf.check_params({k: out[k] for k in fastnsf.DEFAULTS}, fn=fn))
    nonneg(fn, out, "rigid_weight", finite=True)
    positive(fn, out, "rigid_delta", finite=True)
    positive(fn, out, "eps", finite=True)
    for k, hi in (("rigid_pairs", P_MAX), ("min_points", 1 << 30), ("min_cluster_size", 1 << 30), ("max_cluster_points", 1 << 30)):
        integer(fn, out, k, 1, hi, finite=True)
    return out


def kcap(N0: int, min_cluster_size: int) -> int:
    """cluster slots per sample: every cluster has at least min_cluster_size rows, so no more than this many exist"""
    return max(int(N0) // int(min_cluster_size), 1)


def _table(fn: str, name: str, t, dtype, B: int, N: int, device):
    _tensor(fn, name, t, dtype, None, device)
    if t.dim() != 3 or t.shape[0] != B or t.shape[1] != N or t.shape[2] < 2 or t.shape[2] % 2 or t.shape[2] > 2 * P_MAX:
        raise ValueError(f"{fn}: {name} must be {dtype} of shape ({B}, {N}, 2 P) with 1 <= P <= {P_MAX}, got {tuple(t.shape)}")
    if not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError(f"{fn}: {name} must be contiguous and 16-byte aligned")


def iso_plan(x: torch.Tensor, count: torch.Tensor, labels: torch.Tensor, *, pairs: int, max_cluster_points: int,
             kcap: Optional[int] = None, status: Optional[torch.Tensor] = None):
    """x [B,N,3] f32 with count [B] i32 valid leading rows, labels [B,N] i32 (0: no cluster; 1..kcap, default kcap = N)
    -> nbr [B,N,2 pairs] i32 (the rows of every row's forward, then backward partners inside its cluster, -1 without partners),
    r0 [B,N,2 pairs] f32 (their rest distances, 0 at -1), n_pairs [B] i32 (the pair instances M_b).  Labels of rows behind the count are
    ignored.  status: optional i32[1] that is added to for a label outside [0, kcap].  Exact integers; two calls are bit-identical;
    workspaces come from torch's allocator; no host synchronisation."""
    B, N = rows("iso_plan", "x", x)
    dev = x.device
    _tensor("iso_plan", "count", count, torch.int32, (B,), dev)
    _tensor("iso_plan", "labels", labels, torch.int32, (B, N), dev)
    for name, v, hi in (("pairs", pairs, P_MAX), ("max_cluster_points", max_cluster_points, 1 << 30)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
            raise ValueError(f"iso_plan: {name} must be an integer in [1, {hi}], got {v!r}")
    K = N if kcap is None else kcap
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= N + 1:
        raise ValueError(f"iso_plan: kcap must be an integer in [1, {N + 1}], got {kcap!r}")
    if B * N * 2 * pairs >= 2 ** 31 or B * (N + 1) >= 2 ** 31 or B * (2 * K + 1) >= 2 ** 31:
        raise ValueError(f"iso_plan: x: B * N * 2 * pairs < 2^31 expected, got B = {B}, N = {N}, pairs = {pairs}")
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    else:
        _tensor("iso_plan", "status", status, torch.int32, (1,), dev)
    x, count = x.detach().contiguous(), count.contiguous()
    lab, seg_off, seg_rows = segments("iso_plan", "x", labels, count, K, status)
    nbr = torch.empty(B, N, 2 * pairs, dtype=torch.int32, device=dev)
    r0 = torch.empty(B, N, 2 * pairs, dtype=torch.float32, device=dev)
    n_pairs = torch.empty(B, dtype=torch.int32, device=dev)
    call("df_iso_plan", ptr(x), ptr(count), ptr(lab), ptr(seg_off), ptr(seg_rows), B, N, K, pairs, max_cluster_points, ptr(nbr), ptr(r0),
         ptr(n_pairs), stream())
    return nbr, r0, n_pairs


def iso_pairs(w: torch.Tensor, nbr: torch.Tensor, r0: torch.Tensor, *, delta: float):
    """w [B,N,3] f32 (the warped rows), nbr / r0 [B,N,2P] (iso_plan's) -> v [B,N] f32 (the penalty summed over each row's P forward
    instances) and g [B,N,3] f32 (d (sum of the penalties) / d w, not normalised).  Every element is written, 0 at a row without
    partners; no atomics: two calls are bit-identical.  No host synchronisation."""
    B, N = rows("iso_pairs", "w", w)
    _table("iso_pairs", "nbr", nbr, torch.int32, B, N, w.device)
    _table("iso_pairs", "r0", r0, torch.float32, B, N, w.device)
    if r0.shape != nbr.shape:
        raise ValueError(f"iso_pairs: r0 must have the shape of nbr {tuple(nbr.shape)}, got {tuple(r0.shape)}")
    if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not (math.isfinite(delta) and delta > 0):
        raise ValueError(f"iso_pairs: delta must be positive and finite, got {delta!r}")
    P = int(nbr.shape[2]) // 2
    if B * N * 2 * P >= 2 ** 31:
        raise ValueError(f"iso_pairs: w: B * N * 2 P < 2^31 expected, got B = {B}, N = {N}, P = {P}")
    v = torch.empty(B, N, dtype=torch.float32, device=w.device)
    g = torch.empty(B, N, 3, dtype=torch.float32, device=w.device)
    call("df_iso_pairs", ptr(w.detach().contiguous()), ptr(nbr), ptr(r0), B, N, P, float(delta), ptr(v), ptr(g), stream())
    return v, g


def mbnsf_optimize(pc0s: torch.Tensor, count0: torch.Tensor, pc1: torch.Tensor, count1: torch.Tensor, *, grid_range: Sequence[float],
                   init: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, **params):
    """The arguments and the result of ``fastnsf.fastnsf_optimize``, with loss = data + rigid_weight x iso (section 6m).
    labels: the cluster labels [B,N0] i32 of the first sweep when the caller has them (else ``cluster.dbscan`` over the participating
    rows, xy cells over grid_range).  info holds fastnsf's keys and labels [B,N0] i32, n_pairs [B] i32 (the pair instances M_b),
    cluster_status i32[1] (dbscan's and the lists' status word, 0 on a sane input), last_terms [B,2] (data, iso of the last iteration).
    Keywords: DEFAULTS.  Uses no torch autograd.  No host synchronisation unless check_every > 0."""
    fn = "mbnsf_optimize"
    pair = pair_clouds(fn, pc0s, count0, pc1, count1)
    if labels is not None:
        _tensor(fn, "labels", labels, torch.int32, (pair.B, pair.N0), pair.dev)
    p = check_params(params)
    grid = dt_grid(grid_range, p["cell"], p["trunc"], fn=fn)
    x0, n0, m0 = pair.x0, pair.n0, pair.m0
    with torch.no_grad():
        # the clusters, their neighbour table and the number of pair instances: once per pair
        status = torch.zeros(1, dtype=torch.int32, device=pair.dev)
        if labels is None:
            from .cluster import dbscan
            labels, _ = dbscan(x0, n0, mask=m0, eps=p["eps"], min_points=p["min_points"], min_cluster_size=p["min_cluster_size"],
                               grid_range=(grid_range[0], grid_range[1], grid_range[3], grid_range[4]), status=status)
        labels = torch.where(m0, labels, torch.zeros_like(labels)).contiguous()
        nbr, r0, n_pairs = iso_plan(x0, n0, labels, pairs=p["rigid_pairs"], max_cluster_points=p["max_cluster_points"],
                                    kcap=kcap(pair.N0, p["min_cluster_size"]), status=status)
        inv_m = 1.0 / n_pairs.clamp_min(1).to(torch.float32)               # 1 / max(M_b, 1)
        g_scale = (p["rigid_weight"] * inv_m)[:, None, None]

        def iso(W):
            v, gi = iso_pairs(W, nbr, r0, delta=p["rigid_delta"])
            return sample_sum(v) * inv_m, g_scale * gi                      # (gi is 0 outside m0: those rows have no partners)

    flow, info = optimize_net(fn, pair, p, grid, init, term=iso, weight=p["rigid_weight"])
    info.update({"labels": labels, "n_pairs": n_pairs, "cluster_status": status})
    return flow, info


class MbNsf(FastNsf):
    """``model=mbnsf``: ``fastnsf.FastNsf``'s interface -- ``forward_padded`` and ``forward`` with ``DeFlow``'s keys, no weights -- around
    ``mbnsf_optimize``.  Every keyword besides point_cloud_range / voxel_size is one of DEFAULTS; the transform's grid covers
    point_cloud_range."""
    optimize, check_params = staticmethod(mbnsf_optimize), staticmethod(check_params)
    KEEP = ("labels", "n_pairs", "last_terms")
