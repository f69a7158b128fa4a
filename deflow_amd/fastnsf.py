"""Per-pair flow optimised on a GPU distance transform (``model=fastnsf``): ONE small coordinate MLP per pair of sweeps, optimised at test
time against a lookup in the truncated distance transform of the second sweep, with no weights and no checkpoint.

UNPINNED: the recipe is FastNSF's (Li, Zheng & Lucey, ICCV'23) -- the target sweep is turned once into a distance-transform grid, the loss
is a lookup in it, there is no inverse net and no per-iteration search -- but upstream's source is absent, and every choice here is this
project's own.  The definition is in DESIGN.md section 6l and include/deflow_amd.h; tests/helpers/dt_ref.py restates it in torch.  The
transform and its lookup run on csrc/dt.hip, the MLP on csrc/mlp.hip (``deflow_amd.nsfp``'s wrappers); the loop, its snapshot and freeze
and its Adam update are ``deflow_amd.pairopt``'s.  ``DataTerm`` and ``optimize_net`` are shared with ``mbnsf`` and ``floxels``.

CUDA tensors only, like the rest of the library: there is no CPU fallback.  The loop makes no host decision, so one iteration can be
captured as a HIP graph (``graph=True``)."""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional, Sequence

import torch

from . import pairflow
from ._lib import call, ptr, stream
from .args import tensor as _tensor, workspace
from .nsfp import MAX_DEPTH, init_params, mlp_backward, mlp_forward, param_stride
from .pairopt import Loop, OptimisedPairModel, mean_and_weight, pair_clouds, rows

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


def f32(v: float) -> float:
    return float(torch.tensor(float(v), dtype=torch.float32))


def dt_grid(grid_range: Sequence[float], cell: float, trunc: float, fn: str = "dt_grid"):
    """(minx, miny, minz, maxx, maxy, maxz), cell, trunc -> origin (3 floats, as fp32 holds them), dims (GX, GY, GZ), R.
    R = round(trunc / cell) voxels, G_a = ceil((max_a - min_a) / cell) + 2 R, origin_a = min_a - R cell: a position within trunc of an
    in-range point is inside the grid.  ValueError names the argument, against ``fn``.  Launches nothing."""
    if len(grid_range) != 6 or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in grid_range):
        raise ValueError(f"{fn}: grid_range must be 6 finite values (minx, miny, minz, maxx, maxy, maxz), got {grid_range!r}")
    for name, v in (("cell", cell), ("trunc", trunc)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not (math.isfinite(v) and v > 0):
            raise ValueError(f"{fn}: {name} must be positive and finite, got {v!r}")
    cell, trunc = float(cell), float(trunc)
    R = int(round(trunc / cell))
    if not 1 <= R <= R_MAX or abs(R * cell - trunc) > 1e-6 * trunc:
        raise ValueError(f"{fn}: trunc must be a whole number of cells, 1 to {R_MAX} of them, got trunc = {trunc}, cell = {cell}")
    r = [float(v) for v in grid_range]
    if not all(r[3 + a] > r[a] for a in range(3)):
        raise ValueError(f"{fn}: grid_range is empty: {grid_range!r}")
    dims = tuple(int(math.ceil((r[3 + a] - r[a]) / cell - 1e-6)) + 2 * R for a in range(3))      # (102.4 / 0.1 is 1024 + 1e-13)
    if math.prod(dims) >= 2 ** 31:
        raise ValueError(f"{fn}: grid_range / cell: {dims[0]} x {dims[1]} x {dims[2]} voxels do not fit 31 bits")
    origin = tuple(f32(r[a] - R * cell) for a in range(3))
    return origin, dims, R


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
    B, N = rows("dt_build", "ref", ref)
    _tensor("dt_build", "count", count, torch.int32, (B,), ref.device)
    _grid_args("dt_build", origin, cell, dims, radius)
    GX, GY, GZ = dims
    ws = workspace("df_dt_ws_bytes", (B, GX, GY, GZ, radius), ref.device,
                   f"dt_build: dims: df_dt_ws_bytes refused B = {B}, dims = {tuple(dims)}, radius = {radius}")
    dt2 = torch.empty(B, GZ, GY, GX, dtype=torch.uint16, device=ref.device)
    call("df_dt_build", ptr(ref.detach().contiguous()), ptr(count.contiguous()), B, N, origin[0], origin[1], origin[2], cell, GX, GY, GZ,
         radius, ptr(dt2), ptr(ws), stream())
    return dt2


def dt_lookup(query: torch.Tensor, count: torch.Tensor, dt2: torch.Tensor, *, origin: Sequence[float], cell: float, radius: int,
              return_cells: bool = False):
    """query [B,N,3] f32, count [B] i32, dt2 [B,GZ,GY,GX] u16 -> d [B,N] (the trilinear interpolant of cell * sqrt(dt2)), g [B,N,3] (its
    gradient; 0 on an axis whose position was clamped), and with return_cells also cells [B,N,3] i32 (the lower corner used) and clamped
    [B,N] u8 (bit a: axis a was clamped).  Rows behind the count: 0; counted non-finite rows: d = radius * cell, g = 0.  No host
    synchronisation."""
    B, N = rows("dt_lookup", "query", query)
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


def check_params(p: Dict[str, object], fn: str = "fastnsf_optimize") -> Dict[str, object]:
    """validated copy of a parameter dict (ValueError naming the argument, against ``fn``); launches nothing"""
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


class DataTerm:
    """The data term fastnsf, mbnsf and floxels share, built once per pair: the transform of the second sweep (pc1, n1) on ``grid``
    (dt_grid's result, with its cell) and m0, the participating rows of the first sweep (the transform leaves non-finite rows of the
    second sweep out itself)."""

    def __init__(self, pc1: torch.Tensor, n1: torch.Tensor, grid, cell: float, m0: torch.Tensor):
        self.origin, dims, self.R = grid
        self.cell, self.m0 = cell, m0
        self.dt2 = dt_build(pc1, n1, origin=self.origin, cell=cell, dims=dims, radius=self.R)
        self.inf = torch.full(m0.shape, math.inf, dtype=torch.float32, device=m0.device)

    def __call__(self, W: torch.Tensor, n0: torch.Tensor):
        """the warped rows W [B,N0,3] -> data [B] (the mean lookup over m0), d data / d W [B,N0,3] (g / max(n, 1) on m0, 0 elsewhere)
        and the lookup's cells"""
        d, g, cells, _ = dt_lookup(W, n0, self.dt2, origin=self.origin, cell=self.cell, radius=self.R, return_cells=True)
        data, weight = mean_and_weight(torch.where(self.m0, d, self.inf))
        return data, g * weight[..., None], cells


def optimize_net(fn: str, pair, p: Dict[str, object], grid, init: Optional[torch.Tensor], term: Optional[Callable] = None,
                 weight: float = 0.0):
    """fastnsf's loop on pair_clouds' result, validated parameters and dt_grid's result: loss = data, or data + weight x value with
    ``term``: W [B,N0,3] -> (value [B], its gradient [B,N0,3] already scaled by weight and the term's own normalisation).  With a term,
    info gains last_terms [B,2] (data, value of the last iteration).  -> flow, info as fastnsf_optimize's."""
    depth, B = p["depth"], pair.B
    S = param_stride(depth)
    start = start_params(depth, p["seed"]) if init is None else init
    if not isinstance(start, torch.Tensor) or tuple(start.shape) != (1, S) or start.dtype != torch.float32:
        raise ValueError(f"{fn}: init must be a float32 tensor of shape (1, {S})")
    x0, n0, m0 = pair.x0, pair.n0, pair.m0                                 # (rows outside m0 are 0 for the net and left out of the loss)
    with torch.no_grad():
        data_term = DataTerm(pair.pc1, pair.n1, grid, p["cell"], m0)
        arena = start.to(pair.dev)[None].repeat(B, 1, 1).contiguous()       # [B][1][S]
        loop = Loop(arena, x0, p)
        fpar = arena[:, 0]
        last = {"cells": None}
        if term is not None:
            last["last_terms"] = torch.zeros(B, 2, dtype=torch.float32, device=pair.dev)

        def iteration():
            F, acts = mlp_forward(x0, n0, fpar, depth)
            F = F * m0[..., None]
            W = x0 + F
            data, dF, cells = data_term(W, n0)
            loss = data
            if term is not None:
                value, g = term(W)
                loss = data + weight * value
                dF = dF + g
            mlp_backward(x0, n0, fpar, depth, acts, dF, need_dx=False, dparams=loop.grads[:, 0])
            loop.snapshot(loss, F)
            loop.update()
            if term is not None:
                last["last_terms"].copy_(torch.stack([data, value], dim=1))
            last["cells"] = cells

        loop.run(iteration)
        return loop.result(m0, params=arena, **last)


def fastnsf_optimize(pc0s: torch.Tensor, count0: torch.Tensor, pc1: torch.Tensor, count1: torch.Tensor, *, grid_range: Sequence[float],
                     init: Optional[torch.Tensor] = None, **params):
    """pc0s [B,N0,3] f32 (first sweep, in the second sweep's frame) with count0 [B] i32 valid leading rows; pc1 [B,N1,3], count1 alike;
    grid_range (minx, miny, minz, maxx, maxy, maxz): the range the transform's grid covers (plus trunc on every side).
    -> flow [B,N0,3] f32 (the best iterate's residual flow; 0 for rows behind count0 and non-finite rows) and info: best_loss [B],
    loss_history [iters,B] (as nsfp_optimize's), stalled [B] i32, frozen [B] bool, params [B,1,stride] (the arena after the last update),
    grads (of the last iteration), cells [B,N0,3] i32 (the last iteration's lookup cells), iters_run (host int).  Keywords: DEFAULTS;
    init: the [1, param_stride] start (else start_params(depth, seed)).  Uses no torch autograd.  No host synchronisation
    unless check_every > 0 (one read of the frozen flags per check_every iterations)."""
    pair = pair_clouds("fastnsf_optimize", pc0s, count0, pc1, count1)
    p = check_params(params)
    return optimize_net("fastnsf_optimize", pair, p, dt_grid(grid_range, p["cell"], p["trunc"]), init)


class FastNsf(OptimisedPairModel):
    """``model=fastnsf``: ``nsfp.Nsfp``'s interface -- ``forward_padded`` and ``forward`` with ``DeFlow``'s keys, no weights -- around
    ``fastnsf_optimize``.  Every keyword besides point_cloud_range / voxel_size is one of DEFAULTS; the transform's grid covers
    point_cloud_range."""
    optimize, check_params = staticmethod(fastnsf_optimize), staticmethod(check_params)

    def check_grid(self) -> None:
        dt_grid(self.point_cloud_range, self.params["cell"], self.params["trunc"])

