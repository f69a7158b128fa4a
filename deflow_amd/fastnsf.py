"""Per-pair flow optimised on a GPU distance transform (``model=fastnsf``): ONE small coordinate MLP per pair of sweeps, optimised at test
time against a lookup in the truncated distance transform of the second sweep, with no weights and no checkpoint.

UNPINNED: the recipe is FastNSF's (Li, Zheng & Lucey, ICCV'23) -- the target sweep is turned once into a distance-transform grid, the loss
is a lookup in it, there is no inverse net and no per-iteration search -- but upstream's source is absent, and every choice here is this
project's own.  The definition is in DESIGN.md section 6l and include/deflow_amd.h; tests/helpers/dt_ref.py restates it in torch.  The
transform and its lookup run on csrc/dt.hip, the MLP on csrc/mlp.hip (``deflow_amd.nsfp``'s wrappers), the update on df_adam_step_dev.

CUDA tensors only, like the rest of the library: there is no CPU fallback.  The loop makes no host decision (``nsfp``'s snapshot and
freeze, on the device), so one iteration can be captured as a HIP graph (``graph=True``)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import pairflow
from ._lib import call, ptr, stream
from .nsfp import (BETAS, EPS, MAX_DEPTH, _loop_state, _mean_and_weight, _run, _snapshot_and_freeze, init_params, mlp_backward, mlp_forward,
                   param_stride)
from .pairflow import PairFlowModel, _tensor

R_MAX = 255
LINE_TILE = 256          # x positions per workgroup of the transform's passes (csrc/dt.hip: DT_TILE)

# every default of section 6l; all of them are arguments of fastnsf_optimize and FastNsf, and `fastnsf_<name>=` keys of the commands
DEFAULTS: Dict[str, object] = {"depth": 7, "iters": 1000, "lr": 8e-3, "cell": 0.1, "trunc": 2.0, "patience": 100, "min_delta": 1e-4,
                               "check_every": 50, "seed": 0, "graph": False}
COMMAND_KEYS: Dict[str, str] = {"fastnsf_" + k: k for k in DEFAULTS}
# default batch_size of the commands.  Peak per sample at the defaults and 80 000 rows: the grid (1064 x 1064 x 100 u16, 226 MB), while
# it is built one more copy of it, then the saved activations ((depth + 1) x N x 512 bytes, 328 MB) and the MLP backward's workspace
# of the same size: about 0.9 GB
COMMAND_BATCH_SIZE = 4


def _f32(v: float) -> float:
    return float(torch.tensor(float(v), dtype=torch.float32))


def dt_grid(grid_range: Sequence[float], cell: float, trunc: float):
    """(minx, miny, minz, maxx, maxy, maxz), cell, trunc -> origin (3 floats, as fp32 holds them), dims (GX, GY, GZ), R.
    R = round(trunc / cell) voxels, G_a = ceil((max_a - min_a) / cell) + 2 R, origin_a = min_a - R cell: a position within trunc of an
    in-range point is inside the grid.  ValueError names the argument.  Launches nothing."""
    if len(grid_range) != 6 or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in grid_range):
        raise ValueError(f"dt_grid: grid_range must be 6 finite values (minx, miny, minz, maxx, maxy, maxz), got {grid_range!r}")
    for name, v in (("cell", cell), ("trunc", trunc)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0):
            raise ValueError(f"dt_grid: {name} must be positive and finite, got {v!r}")
    cell, trunc = float(cell), float(trunc)
    R = int(round(trunc / cell))
    if not 1 <= R <= R_MAX or abs(R * cell - trunc) > 1e-6 * trunc:
        raise ValueError(f"dt_grid: trunc must be a whole number of cells, 1 to {R_MAX} of them, got trunc = {trunc}, cell = {cell}")
    r = [float(v) for v in grid_range]
    if not all(r[3 + a] > r[a] for a in range(3)):
        raise ValueError(f"dt_grid: grid_range is empty: {grid_range!r}")
    dims = tuple(int(math.ceil((r[3 + a] - r[a]) / cell - 1e-6)) + 2 * R for a in range(3))      # (102.4 / 0.1 is 1024 + 1e-13)
    if math.prod(dims) >= 2 ** 31:
        raise ValueError(f"dt_grid: grid_range / cell: {dims[0]} x {dims[1]} x {dims[2]} voxels do not fit 31 bits")
    origin = tuple(_f32(r[a] - R * cell) for a in range(3))
    return origin, dims, R


def _rows(fn: str, name: str, t) -> Tuple[int, int]:
    _tensor(fn, name, t, torch.float32)
    if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{fn}: {name} must be torch.float32 of shape (B, N, 3) with B >= 1 and N >= 1, got {tuple(t.shape)}")
    B, N = int(t.shape[0]), int(t.shape[1])
    if B > 65535 or 3 * B * N >= 2 ** 31:
        raise ValueError(f"{fn}: {name}: 1 <= B <= 65535 and 3 * B * N < 2^31 expected, got B = {B}, N = {N}")
    return B, N


def _grid_args(fn: str, origin, cell, dims, radius):
    if len(origin) != 3 or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in origin):
        raise ValueError(f"{fn}: origin must be 3 finite values, got {origin!r}")
    if isinstance(cell, bool) or not isinstance(cell, (int, float)) or not (math.isfinite(cell) and cell > 0):
        raise ValueError(f"{fn}: cell must be positive and finite, got {cell!r}")
    if len(dims) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) and v >= 2 for v in dims) or math.prod(dims) >= 2 ** 31:
        raise ValueError(f"{fn}: dims must be 3 integers (GX, GY, GZ), each >= 2, with a product below 2^31, got {dims!r}")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 1 <= radius <= R_MAX:
        raise ValueError(f"{fn}: radius must be an integer in [1, {R_MAX}], got {radius!r}")


def dt_build(ref: torch.Tensor, count: torch.Tensor, *, origin: Sequence[float], cell: float, dims: Sequence[int], radius: int) -> torch.Tensor:
    """ref [B,N,3] f32 with count [B] i32 valid leading rows -> dt2 [B,GZ,GY,GX] u16: min(R^2, squared distance in voxels to the nearest
    occupied voxel of the sample).  Exact (integers); two calls are bit-identical; no host synchronisation."""
    B, N = _rows("dt_build", "ref", ref)
    _tensor("dt_build", "count", count, torch.int32, (B,), ref.device)
    _grid_args("dt_build", origin, cell, dims, radius)
    GX, GY, GZ = dims
    need = int(call("df_dt_ws_bytes", B, GX, GY, GZ, radius))
    if need < 0:
        raise ValueError(f"dt_build: dims: df_dt_ws_bytes refused B = {B}, dims = {tuple(dims)}, radius = {radius}")
    dt2 = torch.empty(B, GZ, GY, GX, dtype=torch.uint16, device=ref.device)
    ws = torch.empty(need, dtype=torch.uint8, device=ref.device)
    call("df_dt_build", ptr(ref.detach().contiguous()), ptr(count.contiguous()), B, N, origin[0], origin[1], origin[2], cell, GX, GY, GZ,
         radius, ptr(dt2), ptr(ws), stream())
    return dt2


def dt_lookup(query: torch.Tensor, count: torch.Tensor, dt2: torch.Tensor, *, origin: Sequence[float], cell: float, radius: int,
              return_cells: bool = False):
    """query [B,N,3] f32, count [B] i32, dt2 [B,GZ,GY,GX] u16 -> d [B,N] (the trilinear interpolant of cell * sqrt(dt2)), g [B,N,3] (its
    gradient; 0 on an axis whose position was clamped), and with return_cells also cells [B,N,3] i32 (the lower corner used) and clamped
    [B,N] u8 (bit a: axis a was clamped).  Rows behind the count: 0; counted non-finite rows: d = radius * cell, g = 0.  No host
    synchronisation."""
    B, N = _rows("dt_lookup", "query", query)
    _tensor("dt_lookup", "count", count, torch.int32, (B,), query.device)
    _tensor("dt_lookup", "dt2", dt2, torch.uint16, None, query.device)
    if dt2.dim() != 4 or dt2.shape[0] != B or not dt2.is_contiguous():
        raise ValueError(f"dt_lookup: dt2 must be contiguous torch.uint16 of shape ({B}, GZ, GY, GX), got {tuple(dt2.shape)}")
    dims = (int(dt2.shape[3]), int(dt2.shape[2]), int(dt2.shape[1]))
    _grid_args("dt_lookup", origin, cell, dims, radius)
    dev = query.device
    d = torch.empty(B, N, dtype=torch.float32, device=dev)
    g = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    cells = torch.empty(B, N, 3, dtype=torch.int32, device=dev) if return_cells else None
    clamped = torch.empty(B, N, dtype=torch.uint8, device=dev) if return_cells else None
    call("df_dt_lookup", ptr(query.detach().contiguous()), ptr(count.contiguous()), ptr(dt2), B, N, origin[0], origin[1], origin[2], cell,
         dims[0], dims[1], dims[2], radius, ptr(d), ptr(g), ptr(cells), ptr(clamped), stream())
    return (d, g, cells, clamped) if return_cells else (d, g)


def params_from_command(given: Dict[str, str]) -> Dict[str, object]:
    return pairflow.params_from_command(pairflow.entry("fastnsf"), given)


def check_params(p: Dict[str, object]) -> Dict[str, object]:
    """validated copy of a parameter dict (ValueError naming the argument); launches nothing"""
    fn = "fastnsf_optimize"
    out = pairflow.merged(fn, DEFAULTS, p)
    for k, lo, hi in (("depth", 0, MAX_DEPTH), ("iters", 1, 1 << 20), ("patience", 1, 1 << 30), ("check_every", 0, 1 << 30),
                      ("seed", 0, (1 << 63) - 1)):
        pairflow.integer(fn, out, k, lo, hi)
    for k in ("lr", "cell", "trunc"):
        pairflow.positive(fn, out, k)
    pairflow.whole_cells(fn, out, R_MAX)
    pairflow.nonneg(fn, out, "min_delta")
    pairflow.flag(fn, out, "graph")
    return out


def start_params(depth: int, seed: int) -> torch.Tensor:
    """[1, param_stride] f32 on the host: row 0 (the forward net f) of nsfp.init_params, so the same seed starts both estimators from the same f"""
    return init_params(depth, seed)[:1].clone()


def fastnsf_optimize(pc0s: torch.Tensor, count0: torch.Tensor, pc1: torch.Tensor, count1: torch.Tensor, *, grid_range: Sequence[float],
                     init: Optional[torch.Tensor] = None, **params):
    """pc0s [B,N0,3] f32 (first sweep, in the second sweep's frame) with count0 [B] i32 valid leading rows; pc1 [B,N1,3], count1 alike;
    grid_range (minx, miny, minz, maxx, maxy, maxz): the range the transform's grid covers (plus trunc on every side).
    -> flow [B,N0,3] f32 (the best iterate's residual flow; 0 for rows behind count0 and non-finite rows) and info: best_loss [B],
    loss_history [iters,B] (as nsfp_optimize's), stalled [B] i32, frozen [B] bool, params [B,1,stride] (the arena after the last update),
    grads (of the last iteration), cells [B,N0,3] i32 (the last iteration's lookup cells), iters_run (host int).  Keywords: DEFAULTS;
    init: the [1, param_stride] start (else start_params(depth, seed)).  Uses no torch autograd.  No host synchronisation
    unless check_every > 0 (one read of the frozen flags per check_every iterations)."""
    B, N0 = _rows("fastnsf_optimize", "pc0s", pc0s)
    B1, N1 = _rows("fastnsf_optimize", "pc1", pc1)
    dev = pc0s.device
    if B1 != B or pc1.device != dev:
        raise ValueError(f"fastnsf_optimize: pc1 must have the batch size ({B}) and device of pc0s, got {tuple(pc1.shape)} on {pc1.device}")
    for name, c in (("count0", count0), ("count1", count1)):
        _tensor("fastnsf_optimize", name, c, torch.int32, (B,), dev)
    p = check_params(params)
    depth, iters, cell = p["depth"], p["iters"], p["cell"]
    origin, dims, R = dt_grid(grid_range, cell, p["trunc"])
    S = param_stride(depth)
    start = start_params(depth, p["seed"]) if init is None else init
    if not isinstance(start, torch.Tensor) or tuple(start.shape) != (1, S) or start.dtype != torch.float32:
        raise ValueError(f"fastnsf_optimize: init must be a float32 tensor of shape (1, {S})")
    with torch.no_grad():
        pc0s, pc1 = pc0s.detach().contiguous(), pc1.detach().contiguous()
        n0, n1 = count0.contiguous().clamp(0, N0), count1.contiguous().clamp(0, N1)
        # participating rows of the first sweep; everything else is 0 for the net and left out of the loss (the transform leaves
        # non-finite rows of the second sweep out itself)
        m0 = (torch.arange(N0, device=dev)[None] < n0[:, None]) & torch.isfinite(pc0s).all(dim=2)
        x0 = torch.where(m0[..., None], pc0s, torch.zeros_like(pc0s))
        dt2 = dt_build(pc1, n1, origin=origin, cell=cell, dims=dims, radius=R)
        arena = start.to(dev)[None].repeat(B, 1, 1).contiguous()       # [B][1][S]
        grads = torch.zeros_like(arena)
        exp_avg, exp_avg_sq = torch.zeros_like(arena), torch.zeros_like(arena)
        step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        t_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        st = _loop_state(B, iters, x0)
        st["cells"] = None
        fpar = arena[:, 0]
        inf = torch.full((B, N0), math.inf, dtype=torch.float32, device=dev)

        def iteration():
            F, acts = mlp_forward(x0, n0, fpar, depth)
            F = F * m0[..., None]
            W = x0 + F
            d, g, cells, _ = dt_lookup(W, n0, dt2, origin=origin, cell=cell, radius=R, return_cells=True)
            loss, weight = _mean_and_weight(torch.where(m0, d, inf))        # the mean over the participating rows, and 1 / max(n, 1) on them
            mlp_backward(x0, n0, fpar, depth, acts, g * weight[..., None], need_dx=False, dparams=grads[:, 0])
            _snapshot_and_freeze(st, loss, F, t_dev, p)
            step_dev.add_(1)
            call("df_adam_step_dev", ptr(arena), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), arena.numel(), p["lr"], BETAS[0], BETAS[1], EPS,
                 ptr(step_dev), 1.0, stream())
            st["cells"] = cells

        ran = _run(iteration, st, p)
        flow = st["best_flow"] * m0[..., None]
    info = {"best_loss": st["best"], "loss_history": st["history"], "stalled": st["stalled"], "frozen": st["frozen"], "params": arena,
            "grads": grads, "cells": st["cells"], "iters_run": ran}
    return flow, info


class FastNsf(PairFlowModel):
    """``model=fastnsf``: ``nsfp.Nsfp``'s interface -- ``forward_padded`` and ``forward`` with ``DeFlow``'s keys, no weights -- around
    ``fastnsf_optimize``.  Every keyword besides point_cloud_range / voxel_size is one of DEFAULTS; the transform's grid covers
    point_cloud_range."""

    def __init__(self, point_cloud_range=(-51.2, -51.2, -3, 51.2, 51.2, 3), voxel_size=(0.2, 0.2, 6), **params):
        super().__init__(point_cloud_range, voxel_size)
        self.params = check_params(params)
        dt_grid(self.point_cloud_range, self.params["cell"], self.params["trunc"])        # refuse a grid that does not fit here

    def forward_padded(self, batch: Dict[str, torch.Tensor]) -> dict:
        """flow [B,N,3]: row i < counts0[b] is the residual flow of input row idx_c0[b,i] (the decoded rows in ascending order), 0 behind
        them; pose_flow [B,N,3] of every input row.  Reads nothing back when check_every = 0."""
        st = self._pair(batch)
        flow, info = fastnsf_optimize(st["points_c0"], st["counts0"], st["points_c1"], st["counts1"], grid_range=self.point_cloud_range,
                                      **self.params)
        st.update({"flow": flow, "best_loss": info["best_loss"], "loss_history": info["loss_history"], "stalled": info["stalled"],
                   "frozen": info["frozen"]})
        self.last_state = st
        return st
