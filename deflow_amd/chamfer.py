"""Nearest-neighbour search and chamfer distance on the GPU: the counterpart of the reference's chamfer3D extension
([REF README.md:39] ``cd assets/cuda/chamfer3D && python ./setup.py install``), the op behind the self-supervised SeFlow losses.

UNPINNED: the extension's source lives in the absent OpenSceneFlow submodule; the contract restated here is the recalled one --
``ChamferDis.apply(pc0, pc1) -> dist0, dist1, idx0, idx1`` (squared distances, differentiable w.r.t. both clouds) and
``chamfer_distance`` on top of it.  Upstream compares all pairs; here the search walks a uniform xy grid (csrc/chamfer.hip,
DESIGN.md "chamfer nearest neighbour"), and the scatter half of the backward is segmented, not atomic: results are bit-reproducible.

CUDA tensors only, like the rest of the library: there is no CPU fallback."""
from __future__ import annotations

import functools
import math
from typing import Optional, Sequence, Tuple

import torch

from ._lib import call, ptr, stream
from .args import labels, tensor, workspace

# The grid: cells of CELL metres over GRID_RANGE (xmin, ymin, xmax, ymax); rows outside go to the clamped border cells, so the range
# only affects speed, never the result.  CELL: see DESIGN.md (0.5 m: the 3 x 3 cells around a query guarantee a 0.5 m radius, which
# holds the neighbour of ~9 in 10 rows of a 70 000-row cloud, at ~60 candidate rows where the cloud is densest).
CELL = 0.5
GRID_RANGE = (-51.2, -51.2, 51.2, 51.2)


def _grid(B: int, grid_range: Sequence[float], cell: float) -> Tuple[float, float, int]:
    xmin, ymin, xmax, ymax = (float(v) for v in grid_range)
    if not (cell > 0 and xmax > xmin and ymax > ymin):
        raise ValueError(f"chamfer_nn: bad grid (range {tuple(grid_range)}, cell {cell})")
    G = int(math.ceil(max(xmax - xmin, ymax - ymin) / cell - 1e-6))
    G = max(1, min(G, 4096, int(math.isqrt((0x3fffffff - 1) // max(B, 1)))))
    return xmin, ymin, G


_check = functools.partial(tensor, "chamfer_nn")


class RowGrid:
    """The xy search grid of ``B`` samples, sized once: ``file`` puts a cloud's rows under its cells (df_nn_grid_build), ``nn`` searches a
    filed cloud (df_chamfer_nn).  A static cloud is filed once and searched as often as needed.  Checks nothing but the grid: the callers
    have checked their tensors."""

    def __init__(self, B: int, grid_range: Sequence[float], cell: float, device):
        self.minx, self.miny, self.G = _grid(B, grid_range, cell)
        self.B, self.cell, self.dev = int(B), float(cell), device

    def file(self, points: torch.Tensor, count: torch.Tensor, label: Optional[torch.Tensor] = None):
        """points [B,N,3] f32, count [B] i32, label [B,N] i32 or None -> (cell_rng [B G G, 2] i32, rows [B N, 4] f32)"""
        B, N, G = self.B, int(points.shape[1]), self.G
        cell_rng = torch.empty(B * G * G, 2, dtype=torch.int32, device=self.dev)
        rows = torch.empty(B * N, 4, dtype=torch.float32, device=self.dev)
        ws = workspace("df_nn_grid_ws_bytes", (B, N, G), self.dev, f"RowGrid: df_nn_grid_ws_bytes refused B = {B}, N = {N}, G = {G}")
        call("df_nn_grid_build", ptr(points), ptr(count), ptr(label), B, N, self.minx, self.miny, self.cell, G, ptr(cell_rng), ptr(rows),
             ptr(ws), stream())
        return cell_rng, rows

    def nn(self, query: torch.Tensor, qcount: torch.Tensor, qlabel: Optional[torch.Tensor], filed, max_dist2: float,
           far_count: Optional[torch.Tensor] = None):
        """query [B,Nq,3] f32, qcount [B] i32, qlabel [B,Nq] i32 or None, filed: what ``file`` returned -> d2 [B,Nq] f32, idx [B,Nq] i32"""
        B, Nq = self.B, int(query.shape[1])
        d2 = torch.empty(B, Nq, dtype=torch.float32, device=self.dev)
        idx = torch.empty(B, Nq, dtype=torch.int32, device=self.dev)
        call("df_chamfer_nn", ptr(query), ptr(qcount), ptr(qlabel), B, Nq, ptr(filed[0]), ptr(filed[1]), self.minx, self.miny, self.cell,
             self.G, float(max_dist2), ptr(d2), ptr(idx), ptr(far_count), stream())
        return d2, idx


def chamfer_nn(query: torch.Tensor, qcount: torch.Tensor, ref: torch.Tensor, rcount: torch.Tensor,
               qlabel: Optional[torch.Tensor] = None, rlabel: Optional[torch.Tensor] = None, max_dist2: float = math.inf,
               grid_range: Sequence[float] = GRID_RANGE, cell: float = CELL, far_count: Optional[torch.Tensor] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """query [B,Nq,3] f32 with qcount [B] i32 valid leading rows, ref [B,Nr,3] with rcount [B]; optional integer row labels ([B,Nq],
    [B,Nr]): when given only rows with label > 0 take part; non-finite rows never take part.
    -> d2 [B,Nq] f32 = smallest squared distance to a participating ref row of the same sample, idx [B,Nq] i32 = that row (the lowest
    index on equal distances); d2 = +inf, idx = -1 where that distance exceeds max_dist2, no ref row takes part or the query row does
    not.  No host synchronisation, no gradient (ChamferDis / losses.seflow_loss build theirs on top).
    far_count: optional i32[1] the search adds the number of queries to that had to look past the 3 x 3 cells around their own."""
    qs, rs = tuple(getattr(query, "shape", ())), tuple(getattr(ref, "shape", ()))
    if len(qs) != 3 or len(rs) != 3 or qs[2] != 3 or rs[2] != 3 or qs[0] != rs[0]:
        raise ValueError(f"chamfer_nn: query [B,Nq,3] and ref [B,Nr,3] expected, got {qs} and {rs}")
    B, Nq, Nr = qs[0], qs[1], rs[1]
    if B == 0 or Nq == 0 or Nr == 0:
        raise ValueError("chamfer_nn: empty batch or zero padded rows")
    if not (max_dist2 >= 0):
        raise ValueError(f"chamfer_nn: max_dist2 must be >= 0 (inf allowed), got {max_dist2}")
    _check("query", query, torch.float32, (B, Nq, 3))
    _check("ref", ref, torch.float32, (B, Nr, 3))
    _check("qcount", qcount, torch.int32, (B,))
    _check("rcount", rcount, torch.int32, (B,))
    query, ref = query.detach().contiguous(), ref.detach().contiguous()
    ql = labels("chamfer_nn", "qlabel", qlabel, (B, Nq), f"must be an integer CUDA tensor of shape {(B, Nq)}")
    rl = labels("chamfer_nn", "rlabel", rlabel, (B, Nr), f"must be an integer CUDA tensor of shape {(B, Nr)}")
    grid = RowGrid(B, grid_range, cell, query.device)
    return grid.nn(query, qcount, ql, grid.file(ref, rcount, rl), max_dist2, far_count)


def chamfer_bwd(query: torch.Tensor, ref: torch.Tensor, idx: torch.Tensor, g: torch.Tensor, dquery: Optional[torch.Tensor],
                dref: Optional[torch.Tensor]) -> None:
    """accumulate the gradient of d2[b,i] = |query[b,i] - ref[b, idx[b,i]]|^2 weighted by g [B,Nq] into dquery [B,Nq,3] and / or
    dref [B,Nr,3] (rows with idx < 0 are skipped); deterministic: the scatter into dref is segmented by target row"""
    B, Nq, _ = query.shape
    Nr = ref.shape[1]
    ws = None
    if dref is not None:
        ws = torch.empty(call("df_chamfer_bwd_ws_bytes", B, Nq, Nr), dtype=torch.uint8, device=query.device)
    call("df_chamfer_bwd", ptr(query), ptr(ref), ptr(idx), ptr(g), B, Nq, Nr, ptr(dquery), ptr(dref), ptr(ws), stream())


class NNDistFn(torch.autograd.Function):
    """d2 of a finished search as a differentiable function of the two clouds: forward hands the search's own d2 on, backward is
    df_chamfer_bwd.  Rows with idx < 0 (d2 = +inf) get no gradient."""

    @staticmethod
    def forward(ctx, query, ref, d2, idx):
        ctx.save_for_backward(query.detach().contiguous(), ref.detach().contiguous(), idx)
        return d2.clone()

    @staticmethod
    def backward(ctx, g):
        query, ref, idx = ctx.saved_tensors
        g = torch.where(idx >= 0, g, torch.zeros_like(g)).contiguous().float()
        dq = torch.zeros_like(query) if ctx.needs_input_grad[0] else None
        dr = torch.zeros_like(ref) if ctx.needs_input_grad[1] else None
        if dq is not None or dr is not None:
            chamfer_bwd(query, ref, idx, g, dq, dr)
        return dq, dr, None, None


class ChamferDis(torch.autograd.Function):
    """``ChamferDis.apply(pc0 [N,3], pc1 [M,3]) -> dist0 [N], dist1 [M], idx0 [N] i32, idx1 [M] i32``: squared distance from every
    row to its nearest row of the other cloud and that row's index (unbounded, exact); differentiable w.r.t. both clouds.
    Non-finite rows get +inf / -1 and no gradient."""

    @staticmethod
    def forward(ctx, pc0, pc1):
        if pc0.dim() != 2 or pc1.dim() != 2 or pc0.shape[1] != 3 or pc1.shape[1] != 3:
            raise ValueError(f"ChamferDis: [N,3] and [M,3] clouds expected, got {tuple(pc0.shape)} and {tuple(pc1.shape)}")
        a, b = pc0.detach().float().contiguous()[None], pc1.detach().float().contiguous()[None]
        dev = a.device
        na = torch.full((1,), a.shape[1], dtype=torch.int32, device=dev)
        nb = torch.full((1,), b.shape[1], dtype=torch.int32, device=dev)
        d0, i0 = chamfer_nn(a, na, b, nb)
        d1, i1 = chamfer_nn(b, nb, a, na)
        ctx.save_for_backward(a, b, i0, i1)
        ctx.mark_non_differentiable(i0, i1)
        return d0[0], d1[0], i0[0], i1[0]

    @staticmethod
    def backward(ctx, g0, g1, _gi0, _gi1):
        a, b, i0, i1 = ctx.saved_tensors
        da, db = torch.zeros_like(a), torch.zeros_like(b)
        z = lambda g, i: torch.where(i >= 0, g.float()[None], torch.zeros_like(g, dtype=torch.float32)[None]).contiguous()
        chamfer_bwd(a, b, i0, z(g0, i0), da, db)
        chamfer_bwd(b, a, i1, z(g1, i1), db, da)
        return da[0], db[0]


def chamfer_distance(pc0: torch.Tensor, pc1: torch.Tensor, truncate_dist: float = -1) -> torch.Tensor:
    """mean of dist0 + mean of dist1; truncate_dist > 0: each mean only over the rows whose squared distance is <= truncate_dist
    (a mean over no rows is 0).  Rows without a neighbour (non-finite) are left out of both."""
    d0, d1, _, _ = ChamferDis.apply(pc0, pc1)

    def mean(d):
        keep = torch.isfinite(d.detach())
        if truncate_dist > 0:
            keep = keep & (d.detach() <= truncate_dist)
        return torch.where(keep, d, torch.zeros_like(d)).sum() / keep.sum().clamp_min(1)

    return mean(d0) + mean(d1)
