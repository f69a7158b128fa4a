"""Per-pair flow on a voxel grid optimised on a GPU distance transform (``model=floxels``): the flow field is a grid of 3-vectors read
trilinearly, optimised at test time against ``fastnsf``'s lookup in the truncated distance transform of the second sweep, with a
smoothness term that ties neighbouring active nodes together.  There is no net, no weights and no checkpoint.

UNPINNED: the idea is Floxels' (Hoffmann et al., CVPR'25) -- a voxel grid instead of a coordinate MLP -- but upstream's source is absent
and was not read; every choice here is this project's own.  The definition is in DESIGN.md section 6n and include/deflow_amd.h;
tests/helpers/vox_ref.py restates it in numpy and torch.  The plan, the read, its transpose and the stencil run on csrc/voxflow.hip, the
transform and its lookup on csrc/dt.hip (``deflow_amd.fastnsf``'s wrappers and data term); the loop, its snapshot and freeze and its
Adam update are ``deflow_amd.pairopt``'s.

CUDA tensors only, like the rest of the library: there is no CPU fallback.  The loop makes no host decision, so one iteration can be
captured as a HIP graph (``graph=True``): a linear chain on one stream."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import pairflow
from ._lib import call, ptr, stream
from .args import tensor as _tensor, workspace
from .fastnsf import R_MAX, DataTerm, dt_grid, f32
from .pairopt import Loop, OptimisedPairModel, pair_clouds, rows, sample_sum

# every default of section 6n; all of them are arguments of floxels_optimize and Floxels, and `floxels_<name>=` keys of the commands
DEFAULTS: Dict[str, object] = {"voxel": 0.4, "smooth_weight": 10.0, "iters": 1000, "lr": 0.05, "cell": 0.1, "trunc": 2.0, "patience": 100,
                               "min_delta": 1e-4, "check_every": 50, "graph": False}
COMMAND_KEYS: Dict[str, str] = {"floxels_" + k: k for k in DEFAULTS}
# default batch_size of the commands.  Peak per sample at the defaults and 80 000 rows: the transform's grid (1064 x 1064 x 100 u16,
# 226 MB) and one more copy of it while it is built dominate; the field, its gradient, Adam's two moments, the scatter's and the
# stencil's outputs are 12.7 MB each (257 x 257 x 16 nodes), the plan's ranges 7.9 MB
COMMAND_BATCH_SIZE = 4


def vox_grid(grid_range: Sequence[float], voxel: float, fn: str = "vox_grid"):
    """(minx, miny, minz, maxx, maxy, maxz), voxel -> origin (3 floats, as fp32 holds them), dims (VX, VY, VZ): V_a =
    ceil((max_a - min_a) / voxel - 1e-6) + 1 nodes per axis, at least 2; node (i, j, k) sits at origin + voxel (i, j, k).  ValueError
    names the argument, against ``fn``.  Launches nothing."""
    if len(grid_range) != 6 or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in grid_range):
        raise ValueError(f"{fn}: grid_range must be 6 finite values (minx, miny, minz, maxx, maxy, maxz), got {grid_range!r}")
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float)) or not (math.isfinite(voxel) and voxel > 0):
        raise ValueError(f"{fn}: voxel must be positive and finite, got {voxel!r}")
    r = [float(v) for v in grid_range]
    if not all(r[3 + a] > r[a] for a in range(3)):
        raise ValueError(f"{fn}: grid_range is empty: {grid_range!r}")
    steps = [(r[3 + a] - r[a]) / float(voxel) for a in range(3)]
    if max(steps) >= 2 ** 31:
        raise ValueError(f"{fn}: grid_range / voxel: {max(steps):.3g} nodes on one axis do not fit 31 bits")
    dims = tuple(max(int(math.ceil(s - 1e-6)) + 1, 2) for s in steps)                      # (102.4 / 0.4 is 256 + 3e-14)
    if 3 * math.prod(dims) >= 2 ** 31:
        raise ValueError(f"{fn}: grid_range / voxel: 3 x {dims[0]} x {dims[1]} x {dims[2]} node components do not fit 31 bits")
    return tuple(f32(r[a]) for a in range(3)), dims


def _dims(fn: str, dims, B: int, N: int = 1) -> Tuple[int, int, int]:
    if len(dims) != 3 or not all(isinstance(v, int) and not isinstance(v, bool) and v >= 2 for v in dims):
        raise ValueError(f"{fn}: dims must be 3 integers (VX, VY, VZ), each >= 2, got {dims!r}")
    VX, VY, VZ = dims
    if 3 * B * VX * VY * VZ >= 2 ** 31 or B * (VX - 1) * (VY - 1) * (VZ - 1) >= 2 ** 31 or 3 * B * N >= 2 ** 31:
        raise ValueError(f"{fn}: dims: 3 B NV, B NC and 3 B N below 2^31 expected, got B = {B}, N = {N}, dims = {tuple(dims)}")
    return VX, VY, VZ


def _theta(fn: str, name: str, theta, device=None) -> Tuple[int, Tuple[int, int, int]]:
    _tensor(fn, name, theta, torch.float32, None, device)
    if theta.dim() != 5 or theta.shape[4] != 3 or theta.shape[0] < 1 or theta.shape[0] > 65535 or not theta.is_contiguous():
        raise ValueError(f"{fn}: {name} must be contiguous torch.float32 of shape (B, VZ, VY, VX, 3) with 1 <= B <= 65535, got "
                         f"{tuple(theta.shape)}")
    B = int(theta.shape[0])
    dims = (int(theta.shape[3]), int(theta.shape[2]), int(theta.shape[1]))
    try:
        _dims(fn, dims, B)
    except ValueError:
        raise ValueError(f"{fn}: {name}: every grid dimension >= 2 and 3 B NV < 2^31 expected, got {tuple(theta.shape)}") from None
    return B, dims


def vox_plan(x: torch.Tensor, count: torch.Tensor, *, origin: Sequence[float], voxel: float, dims: Sequence[int]) -> Dict[str, object]:
    """x [B,N,3] f32 with count [B] i32 valid leading rows -> the plan of one pair (a dict): cell [B,N] i32 (-1: the row does not take
    part), frac [B,N,3] f32, idx_sorted [B N] i32 (b N + row, grouped by (sample, cell), ascending inside a cell; -1 behind the grouped
    rows), cell_rng [B NC, 2] i32, active [B,NV] u8, pairs [B] i32 (M_b), and dims.  Exact; two calls are bit-identical; workspaces come
    from torch's allocator; no host synchronisation."""
    B, N = rows("vox_plan", "x", x)
    dev = x.device
    _tensor("vox_plan", "count", count, torch.int32, (B,), dev)
    if len(origin) != 3 or not all(isinstance(v, (int, float)) and math.isfinite(v) for v in origin):
        raise ValueError(f"vox_plan: origin must be 3 finite values, got {origin!r}")
    if isinstance(voxel, bool) or not isinstance(voxel, (int, float)) or not (math.isfinite(voxel) and voxel > 0):
        raise ValueError(f"vox_plan: voxel must be positive and finite, got {voxel!r}")
    VX, VY, VZ = _dims("vox_plan", dims, B, N)
    NV, NC = VX * VY * VZ, (VX - 1) * (VY - 1) * (VZ - 1)
    ws = workspace("df_vox_plan_ws_bytes", (B, N, VX, VY, VZ), dev,
                   f"vox_plan: dims: df_vox_plan_ws_bytes refused B = {B}, N = {N}, dims = {tuple(dims)}")
    cell = torch.empty(B, N, dtype=torch.int32, device=dev)
    frac = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
    idx_sorted = torch.empty(B * N, dtype=torch.int32, device=dev)
    cell_rng = torch.empty(B * NC, 2, dtype=torch.int32, device=dev)
    active = torch.empty(B, NV, dtype=torch.uint8, device=dev)
    pairs = torch.empty(B, dtype=torch.int32, device=dev)
    call("df_vox_plan", ptr(x.detach().contiguous()), ptr(count.contiguous()), B, N, origin[0], origin[1], origin[2], float(voxel), VX, VY, VZ,
         ptr(cell), ptr(frac), ptr(idx_sorted), ptr(cell_rng), ptr(active), ptr(pairs), ptr(ws), stream())
    return {"cell": cell, "frac": frac, "idx_sorted": idx_sorted, "cell_rng": cell_rng, "active": active, "pairs": pairs,
            "dims": (VX, VY, VZ)}


def _plan_rows(fn: str, cell, frac, B: int, dev) -> int:
    _tensor(fn, "cell", cell, torch.int32, None, dev)
    if cell.dim() != 2 or cell.shape[0] != B or cell.shape[1] < 1 or not cell.is_contiguous():
        raise ValueError(f"{fn}: cell must be contiguous torch.int32 of shape ({B}, N), got {tuple(cell.shape)}")
    N = int(cell.shape[1])
    _frac(fn, frac, B, N, dev)
    return N


def _frac(fn: str, frac, B: int, N: int, dev) -> None:
    _tensor(fn, "frac", frac, torch.float32, (B, N, 3), dev)
    if not frac.is_contiguous():
        raise ValueError(f"{fn}: frac must be contiguous")


def vox_sample(theta: torch.Tensor, cell: torch.Tensor, frac: torch.Tensor) -> torch.Tensor:
    """theta [B,VZ,VY,VX,3] f32, cell [B,N] i32 and frac [B,N,3] f32 (vox_plan's) -> F [B,N,3] f32: the field read trilinearly at every
    row, 0 where cell = -1.  Every element is written; no host synchronisation."""
    B, dims = _theta("vox_sample", "theta", theta)
    N = _plan_rows("vox_sample", cell, frac, B, theta.device)
    _dims("vox_sample", dims, B, N)
    F = torch.empty(B, N, 3, dtype=torch.float32, device=theta.device)
    call("df_vox_sample", ptr(theta), ptr(cell), ptr(frac), B, N, dims[0], dims[1], dims[2], ptr(F), stream())
    return F


def vox_scatter(dF: torch.Tensor, frac: torch.Tensor, idx_sorted: torch.Tensor, cell_rng: torch.Tensor, *, dims: Sequence[int]) -> torch.Tensor:
    """dF [B,N,3] f32 (rows that do not take part may hold anything), frac, idx_sorted, cell_rng (vox_plan's) -> dtheta [B,NV,3] f32: the
    exact transpose of vox_sample, summed per node in a fixed order.  No atomics: two calls are bit-identical and a sample's result does
    not depend on its batch.  Every node is written, 0 where nothing is incident; no host synchronisation."""
    B, N = rows("vox_scatter", "dF", dF)
    dev = dF.device
    VX, VY, VZ = _dims("vox_scatter", dims, B, N)
    NV, NC = VX * VY * VZ, (VX - 1) * (VY - 1) * (VZ - 1)
    _frac("vox_scatter", frac, B, N, dev)
    _tensor("vox_scatter", "idx_sorted", idx_sorted, torch.int32, (B * N,), dev)
    _tensor("vox_scatter", "cell_rng", cell_rng, torch.int32, (B * NC, 2), dev)
    if not idx_sorted.is_contiguous() or not cell_rng.is_contiguous():
        raise ValueError("vox_scatter: idx_sorted and cell_rng must be contiguous")
    dtheta = torch.empty(B, NV, 3, dtype=torch.float32, device=dev)
    call("df_vox_scatter", ptr(dF.detach().contiguous()), ptr(frac), ptr(idx_sorted), ptr(cell_rng), B, N, VX, VY, VZ, ptr(dtheta), stream())
    return dtheta


def vox_smooth(theta: torch.Tensor, active: torch.Tensor):
    """theta [B,VZ,VY,VX,3] f32, active [B,NV] u8 (vox_plan's) -> v [B,NV] f32 (per node, the squared differences to its forward
    neighbours x+1, y+1, z+1 with both ends active: their sum counts every pair once) and g [B,NV,3] f32 (d (sum of v) / d theta, not
    normalised).  Every element is written, 0 at an inactive node; no atomics; no host synchronisation."""
    B, dims = _theta("vox_smooth", "theta", theta)
    NV = dims[0] * dims[1] * dims[2]
    _tensor("vox_smooth", "active", active, torch.uint8, (B, NV), theta.device)
    if not active.is_contiguous():
        raise ValueError("vox_smooth: active must be contiguous")
    v = torch.empty(B, NV, dtype=torch.float32, device=theta.device)
    g = torch.empty(B, NV, 3, dtype=torch.float32, device=theta.device)
    call("df_vox_smooth", ptr(theta), ptr(active), B, dims[0], dims[1], dims[2], ptr(v), ptr(g), stream())
    return v, g


def params_from_command(given: Dict[str, str]) -> Dict[str, object]:
    return pairflow.params_from_command(pairflow.entry("floxels"), given)


def check_params(p: Dict[str, object]) -> Dict[str, object]:
    """validated copy of a parameter dict (ValueError naming the argument); launches nothing"""
    fn = "floxels_optimize"
    out = pairflow.merged(fn, DEFAULTS, p)
    for k, lo, hi in (("iters", 1, 1 << 20), ("patience", 1, 1 << 30), ("check_every", 0, 1 << 30)):
        pairflow.integer(fn, out, k, lo, hi, finite=True)
    for k in ("voxel", "lr", "cell", "trunc"):
        pairflow.positive(fn, out, k, finite=True)
    for k in ("smooth_weight", "min_delta"):
        pairflow.nonneg(fn, out, k, finite=True)
    pairflow.whole_cells(fn, out, R_MAX)
    pairflow.flag(fn, out, "graph")
    return out


def _grids(fn: str, grid_range, p: Dict[str, object]):
    return dt_grid(grid_range, p["cell"], p["trunc"], fn=fn), vox_grid(grid_range, p["voxel"], fn=fn)


def floxels_optimize(pc0s: torch.Tensor, count0: torch.Tensor, pc1: torch.Tensor, count1: torch.Tensor, *, grid_range: Sequence[float],
                     init: Optional[torch.Tensor] = None, **params):
    """pc0s [B,N0,3] f32 (first sweep, in the second sweep's frame) with count0 [B] i32 valid leading rows; pc1 [B,N1,3], count1 alike;
    grid_range (minx, miny, minz, maxx, maxy, maxz): the range the field's grid covers (the transform's grid covers it plus trunc on
    every side).  loss = data + smooth_weight x smooth (section 6n).
    -> flow [B,N0,3] f32 (the best iterate's residual flow; 0 for rows behind count0 and non-finite rows) and info: best_loss [B],
    loss_history [iters,B], stalled [B] i32, frozen [B] bool (as fastnsf_optimize's), theta [B,VZ,VY,VX,3] (the field after the last
    update, a view into its flat arena), grads [B,NV,3] (of the last iteration), cells [B,N0,3] i32 (the last iteration's lookup cells),
    n_pairs [B] i32 (M_b), last_terms [B,2] (data, smooth of the last iteration), plan (vox_plan's dict), iters_run (host int).
    Keywords: DEFAULTS; init: the [VZ,VY,VX,3] float32 start of every sample (else zero).  The start is deterministic: there is no seed.
    Uses no torch autograd.  No host synchronisation unless check_every > 0 (one read of the frozen flags per check_every iterations)."""
    fn = "floxels_optimize"
    pair = pair_clouds(fn, pc0s, count0, pc1, count1)
    p = check_params(params)
    sw = p["smooth_weight"]
    grid, (vorigin, vdims) = _grids(fn, grid_range, p)
    B, x0, n0 = pair.B, pair.x0, pair.n0                     # (rows outside m0 have cell = -1 (F = 0) and are left out of the loss)
    VX, VY, VZ = _dims(fn, vdims, B, pair.N0)
    NV = VX * VY * VZ
    if init is not None and (not isinstance(init, torch.Tensor) or tuple(init.shape) != (VZ, VY, VX, 3) or init.dtype != torch.float32):
        raise ValueError(f"{fn}: init must be a float32 tensor of shape ({VZ}, {VY}, {VX}, 3)")
    with torch.no_grad():
        # the rows' cells and fractions, their grouping, the active nodes and the number of pairs: once per pair
        plan = vox_plan(pair.pc0s, n0, origin=vorigin, voxel=p["voxel"], dims=vdims)
        inv_m = 1.0 / plan["pairs"].clamp_min(1).to(torch.float32)             # 1 / max(M_b, 1)
        g_scale = (sw * inv_m)[:, None, None]
        data_term = DataTerm(pair.pc1, pair.n1, grid, p["cell"], pair.m0)
        # a flat arena padded to a multiple of 4 (the Adam entry's n % 4 == 0); theta and the gradient are views into theirs
        n_par = 3 * B * NV
        loop = Loop(torch.zeros((n_par + 3) // 4 * 4, dtype=torch.float32, device=pair.dev), x0, p)
        theta = loop.arena[:n_par].view(B, VZ, VY, VX, 3)
        gview = loop.grads[:n_par].view(B, NV, 3)
        if init is not None:
            theta.copy_(init.to(pair.dev)[None].expand(B, VZ, VY, VX, 3))
        last_terms = torch.zeros(B, 2, dtype=torch.float32, device=pair.dev)
        last = {"cells": None}

        def iteration():
            F = vox_sample(theta, plan["cell"], plan["frac"])
            data, dF, cells = data_term(x0 + F, n0)
            v, gs = vox_smooth(theta, plan["active"])
            smooth = sample_sum(v) * inv_m
            loss = data + sw * smooth
            dth = vox_scatter(dF, plan["frac"], plan["idx_sorted"], plan["cell_rng"], dims=vdims)
            torch.addcmul(dth, gs, g_scale, out=gview)                      # (both are 0 at an inactive node: Adam leaves it at 0)
            loop.snapshot(loss, F)
            loop.update()
            last_terms.copy_(torch.stack([data, smooth], dim=1))
            last["cells"] = cells

        loop.run(iteration)
        return loop.result(pair.m0, theta=theta, grads=gview, n_pairs=plan["pairs"], last_terms=last_terms, plan=plan, **last)


class Floxels(OptimisedPairModel):
    """``model=floxels``: ``fastnsf.FastNsf``'s interface -- ``forward_padded`` and ``forward`` with ``DeFlow``'s keys, no weights -- around
    ``floxels_optimize``.  Every keyword besides point_cloud_range / voxel_size is one of DEFAULTS; the field's grid and the transform's
    cover point_cloud_range."""
    optimize, check_params = staticmethod(floxels_optimize), staticmethod(check_params)
    KEEP = ("n_pairs", "last_terms")

    def check_grid(self) -> None:
        _grids("Floxels", self.point_cloud_range, self.params)
