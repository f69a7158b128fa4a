"""DBSCAN on the GPU and, on top of it, the cluster labels of the self-supervised SeFlow mode (``pc0_dynamic`` / ``pc1_dynamic``) from a
per-point dynamic flag alone.

UNPINNED: upstream produces these labels offline on the CPU ([REF assets/slurm/dufolabel_sbatch.py]; process.py: DUFO dynamic flags, then
HDBSCAN, whose source is in the absent submodule).  What runs here is plain DBSCAN with every choice fixed -- the definition is in
include/deflow_amd.h and DESIGN.md section 6b -- so the labels are a pure function of the input and bit-reproducible.  Of the defaults,
``eps = 0.7`` and ``min_cluster_size = 20`` are the recalled arguments of upstream's HDBSCAN call; ``min_points = 4`` and
``min_dynamic_frac = 0.3`` are this project's own choices.  All four are arguments.  The flags themselves: upstream's ``dufo_label`` dataset when the scene files
hold one, otherwise the void map of ``voidmap.py`` (UNPINNED as well).

CUDA tensors only, like the rest of the library: there is no CPU fallback.  Nothing here reads a device value back."""
from __future__ import annotations

import functools
import math
from typing import Optional, Sequence, Tuple

import torch

from ._lib import call, ptr, stream
from .args import tensor, workspace
from .chamfer import GRID_RANGE, RowGrid

# cell = max(CELL_SLACK * eps, extent / 4096).  The kernels are right at any cell >= eps: they scan the cells that a row's clamped position
# +- (eps / cell + 2e-3) covers (csrc/nn_search.h: nn_window), so two rows within eps that fp32 files two cells apart still meet.  The
# slack decides the SPEED only: with it eps / cell + 2e-3 < 1 and that window is the 3 x 3 cells around the row for every row, while at
# cell == eps a row within 2e-3 cell of a cell edge scans a fourth cell (row) and its wave waits for it (core pass + 10.6 %, finish + 5.9 % measured,
# DESIGN.md section 6b).  The range and the cell never change the result.
CELL_SLACK = 1.0025


_check = functools.partial(tensor, "dbscan")


def _flags(name: str, f: Optional[torch.Tensor], shape) -> Optional[torch.Tensor]:
    """a per-row flag (bool or integer, non-zero = set) as the i32 0 / 1 tensor the kernels read"""
    if f is None:
        return None
    _check(name, f)
    if tuple(f.shape) != tuple(shape) or f.dtype.is_floating_point:
        raise ValueError(f"dbscan: {name} must be a bool or integer CUDA tensor of shape {tuple(shape)}")
    return (f != 0).to(torch.int32).contiguous()


def _run(points: torch.Tensor, count: torch.Tensor, mask, dynamic, eps: float, min_points: int, min_cluster_size: int,
         min_dynamic_frac: float, grid_range, status: Optional[torch.Tensor]):
    shape = tuple(getattr(points, "shape", ()))
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"dbscan: points [B,N,3] expected, got {shape}")
    B, N, _ = shape
    if B == 0 or N == 0:
        raise ValueError("dbscan: empty batch or zero padded rows")
    if not (eps > 0 and math.isfinite(eps)):
        raise ValueError(f"dbscan: eps must be a positive finite radius, got {eps}")
    if int(min_points) < 1 or int(min_cluster_size) < 1:
        raise ValueError(f"dbscan: min_points and min_cluster_size must be >= 1, got {min_points} and {min_cluster_size}")
    if not (min_dynamic_frac >= 0 and math.isfinite(min_dynamic_frac)):
        raise ValueError(f"dbscan: min_dynamic_frac must be a finite fraction >= 0, got {min_dynamic_frac}")
    _check("points", points, torch.float32, (B, N, 3))
    _check("count", count, torch.int32, (B,))
    if status is not None:
        _check("status", status, torch.int32, (1,))
    points = points.detach().contiguous()
    m, d = _flags("mask", mask, (B, N)), _flags("dynamic", dynamic, (B, N))
    rg = GRID_RANGE if grid_range is None else grid_range
    xmin, ymin, xmax, ymax = (float(v) for v in rg)
    cell = max(CELL_SLACK * float(eps), max(xmax - xmin, ymax - ymin) / 4096.0)
    dev = points.device
    grid = RowGrid(B, rg, cell, dev)
    minx, miny, G = grid.minx, grid.miny, grid.G
    cell_rng, rows = grid.file(points, count, m)
    ws = workspace("df_dbscan_ws_bytes", (B, N), dev, f"dbscan: df_dbscan_ws_bytes refused B = {B}, N = {N}")
    labels = torch.empty(B, N, dtype=torch.int32, device=dev)
    n_clusters = torch.empty(B, dtype=torch.int32, device=dev)
    s = stream()
    call("df_dbscan_core", ptr(cell_rng), ptr(rows), B, N, minx, miny, cell, G, float(eps), int(min_points), ptr(ws), s)
    call("df_dbscan_link", ptr(cell_rng), B, N, minx, miny, cell, G, float(eps), ptr(status), ptr(ws), s)
    call("df_dbscan_finish", ptr(cell_rng), ptr(d), B, N, minx, miny, cell, G, float(eps), int(min_cluster_size), float(min_dynamic_frac),
         ptr(labels), ptr(n_clusters), ptr(status), ptr(ws), s)
    return labels, n_clusters


def dbscan(points: torch.Tensor, count: torch.Tensor, mask: Optional[torch.Tensor] = None, *, eps: float = 0.7, min_points: int = 4,
           min_cluster_size: int = 1, grid_range: Optional[Sequence[float]] = None, status: Optional[torch.Tensor] = None
           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """points [B,N,3] f32 with count [B] i32 valid leading rows; optional mask [B,N] (bool or integer): only rows with mask != 0 take
    part; non-finite rows never take part.
    -> labels [B,N] i32 (0 = noise or not participating, clusters 1..K per sample in ascending order of their lowest core row),
    n_clusters [B] i32.  A row is core with >= min_points rows within eps (itself included); border rows join the cluster of their
    nearest core row (the lowest row on equal distances); clusters of fewer than min_cluster_size members are dropped to 0.
    grid_range (xmin, ymin, xmax, ymax): where the rows are expected, default the +-51.2 m of the model; it decides only the speed.
    status: optional i32[1] the kernels add to when one of their bounded loops reaches its bound (never, on a sane input).
    No host synchronisation; two calls are bit-identical."""
    return _run(points, count, mask, None, eps, min_points, min_cluster_size, 0.0, grid_range, status)


def dynamic_cluster_labels(points: torch.Tensor, count: torch.Tensor, dynamic: torch.Tensor, *, eps: float = 0.7, min_points: int = 4,
                           min_cluster_size: int = 20, min_dynamic_frac: float = 0.3, grid_range: Optional[Sequence[float]] = None
                           ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The labels seflowLoss wants from a per-point dynamic flag [B,N] (bool or integer, e.g. upstream's DUFO flag): ALL participating
    rows are clustered (dbscan above), and a cluster is kept when it has >= min_cluster_size members of which at least
    min_dynamic_frac are flagged (flagged < min_dynamic_frac * members, in float64, drops it).
    -> labels [B,N] i32, n_clusters [B] i32, status i32[1] (see dbscan; left on the device)."""
    if dynamic is None:
        raise ValueError("dynamic_cluster_labels: the per-row dynamic flag is required (dbscan clusters without one)")
    _check("points", points)
    status = torch.zeros(1, dtype=torch.int32, device=points.device)
    labels, n_clusters = _run(points, count, None, dynamic, eps, min_points, min_cluster_size, min_dynamic_frac, grid_range, status)
    return labels, n_clusters, status
