"""Per-pair neural flow prior on the GPU (``model=nsfp``): two small coordinate MLPs per pair of sweeps, optimised at test time against a
truncated two-way chamfer distance, with no weights and no checkpoint.

UNPINNED: the recipe is NSFP's (Li, Pontes & Lucey, NeurIPS'21) -- a forward net f and an inverse net g per pair, the flow read off the
best iterate -- but upstream's source is absent, and every choice here is this project's own.  The definition is in DESIGN.md section 6k
and include/deflow_amd.h; tests/helpers/nsfp_ref.py restates it in torch.  The MLPs run on csrc/mlp.hip (forward, data gradient and
weight gradient on the fp32 MFMA), the searches on csrc/chamfer.hip; the loop and its Adam update are ``deflow_amd.pairopt``'s.

CUDA tensors only, like the rest of the library: there is no CPU fallback.  The loop makes no host decision: the step counter, the
snapshot and the freeze live on the device, so one iteration can be captured as a HIP graph (``graph=True``)."""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import pairflow
from ._lib import call, ptr, stream
from .args import tensor, workspace
from .chamfer import CELL, GRID_RANGE, RowGrid, chamfer_bwd
from .pairopt import BETAS, EPS, Loop, OptimisedPairModel, mean_and_weight, pair_clouds  # noqa: F401  (nsfp.BETAS / EPS stay importable)

WIDTH = 128
ROW_TILE = 64            # rows per workgroup of the forward / data-gradient kernels (csrc/mlp.hip: MT)
WGRAD_SPLIT_ROWS = 1024  # rows per weight-gradient split (csrc/mlp.hip: MSPLIT)
MAX_DEPTH = 15

# every default of section 6k; all of them are arguments of nsfp_optimize and Nsfp, and `nsfp_<name>=` keys of the commands
DEFAULTS: Dict[str, object] = {"depth": 7, "iters": 1000, "lr": 8e-3, "trunc_d2": 4.0, "patience": 100, "min_delta": 1e-4,
                               "check_every": 50, "seed": 0, "graph": False}
COMMAND_KEYS: Dict[str, str] = {"nsfp_" + k: k for k in DEFAULTS}
COMMAND_BATCH_SIZE = 2   # default batch_size of the commands: saved activations are (depth + 1) x N x 512 bytes per net evaluation and sample


def num_params(depth: int) -> int:
    """P: elements of one net's flat parameter vector"""
    return (WIDTH * 3 + WIDTH) + int(depth) * (WIDTH * WIDTH + WIDTH) + (3 * WIDTH + 3)


def param_stride(depth: int) -> int:
    """P rounded up to a multiple of 4: the distance between two nets of an arena (16-byte blocks)"""
    return (num_params(depth) + 3) // 4 * 4


def param_slices(depth: int) -> Dict[str, Tuple[int, Tuple[int, ...]]]:
    """{name: (offset, shape)} of the flat vector: W_in, b_in, W_1, b_1, ..., W_out, b_out"""
    out, o = {}, 0
    for name, shape in ([("W_in", (WIDTH, 3)), ("b_in", (WIDTH,))] +
                        [(f"{k}_{l}", s) for l in range(1, int(depth) + 1) for k, s in (("W", (WIDTH, WIDTH)), ("b", (WIDTH,)))] +
                        [("W_out", (3, WIDTH)), ("b_out", (3,))]):
        out[name] = (o, shape)
        o += math.prod(shape)
    assert o == num_params(depth)
    return out


def init_params(depth: int, seed: int) -> torch.Tensor:
    """[2, param_stride] f32 on the host: f then g; weights U(-a, a) with a = sqrt(6 / (fan_in + fan_out)), biases 0, drawn in layout order
    from torch.Generator().manual_seed(seed)"""
    gen = torch.Generator().manual_seed(int(seed))
    out = torch.zeros(2, param_stride(depth), dtype=torch.float32)
    for n in range(2):
        for name, (o, shape) in param_slices(depth).items():
            if name.startswith("W"):
                a = math.sqrt(6.0 / (shape[0] + shape[1]))
                out[n, o:o + math.prod(shape)] = (torch.rand(shape, generator=gen, dtype=torch.float32) * 2 - 1).mul_(a).reshape(-1)
    return out


def params_from_command(given: Dict[str, str]) -> Dict[str, object]:
    return pairflow.params_from_command(pairflow.entry("nsfp"), given)


def check_params(p: Dict[str, object]) -> Dict[str, object]:
    """validated copy of a parameter dict (ValueError naming the argument); launches nothing"""
    fn = "nsfp_optimize"
    out = pairflow.merged(fn, DEFAULTS, p)
    for k, lo, hi in (("depth", 0, MAX_DEPTH), ("iters", 1, 1 << 20), ("patience", 1, 1 << 30), ("check_every", 0, 1 << 30),
                      ("seed", 0, (1 << 63) - 1)):
        pairflow.integer(fn, out, k, lo, hi)
    pairflow.positive(fn, out, "lr")
    pairflow.positive(fn, out, "trunc_d2")
    pairflow.nonneg(fn, out, "min_delta")
    pairflow.flag(fn, out, "graph")
    return out


# ---- the MLP -------------------------------------------------------------------------------------------------------------------------
_tensor = functools.partial(tensor, other="x is")     # (a device mismatch is reported against x)


def _mlp_args(fn: str, x, count, params, depth) -> Tuple[int, int, int]:
    if isinstance(depth, bool) or not isinstance(depth, int) or not 0 <= depth <= MAX_DEPTH:
        raise ValueError(f"{fn}: depth must be an integer in [0, {MAX_DEPTH}], got {depth!r}")
    _tensor(fn, "x", x, torch.float32)
    if x.dim() != 3 or x.shape[2] != 3 or x.shape[0] < 1 or x.shape[1] < 1 or not x.is_contiguous():
        raise ValueError(f"{fn}: x must be contiguous torch.float32 of shape (B, N, 3) with B >= 1 and N >= 1, got {tuple(x.shape)}")
    B, N = int(x.shape[0]), int(x.shape[1])
    if B > 65535 or 3 * B * N >= 2 ** 31 - 1:
        raise ValueError(f"{fn}: x: 1 <= B <= 65535 and 3 * B * N < 2^31 expected, got B = {B}, N = {N}")
    _tensor(fn, "count", count, torch.int32, (B,), x.device)
    _tensor(fn, "params", params, torch.float32, None, x.device)
    P = num_params(depth)
    if params.dim() != 2 or params.shape[0] != B or params.shape[1] < P or params.stride(1) != 1 or params.stride(0) % 4 or \
            params.stride(0) < P or params.data_ptr() % 16:
        raise ValueError(f"{fn}: params must be (B, >= {P}) float32, rows contiguous, 16-byte aligned with a row stride that is a multiple "
                         f"of 4, got shape {tuple(params.shape)}, stride {tuple(params.stride())}")
    return B, N, int(params.stride(0))


def mlp_forward(x: torch.Tensor, count: torch.Tensor, params: torch.Tensor, depth: int, save: bool = True):
    """x [B,N,3] f32, count [B] i32 valid leading rows, params [B, >= P] f32 (one net per sample; a strided view of an arena is fine)
    -> y [B,N,3] (0 for rows >= count), acts [B,depth+1,N,128] (None with save=False).  No host synchronisation."""
    B, N, stride = _mlp_args("mlp_forward", x, count, params, depth)
    y = torch.empty_like(x)
    acts = torch.empty(B, depth + 1, N, WIDTH, dtype=torch.float32, device=x.device) if save else None
    call("df_mlp_fwd", ptr(x), ptr(count.contiguous()), ptr(params), stride, B, N, depth, ptr(y), ptr(acts), stream())
    return y, acts


def mlp_backward(x: torch.Tensor, count: torch.Tensor, params: torch.Tensor, depth: int, acts: torch.Tensor, dy: torch.Tensor,
                 need_dx: bool = True, dparams: Optional[torch.Tensor] = None):
    """-> dparams [B, param_stride(depth)] (every element written, the padding behind P as 0), dx [B,N,3] or None.  dparams: an output
    view to write into (of that shape, with the strides of params), else a fresh tensor.  Two calls are bit-identical; no host synchronisation."""
    B, N, stride = _mlp_args("mlp_backward", x, count, params, depth)
    _tensor("mlp_backward", "acts", acts, torch.float32, (B, depth + 1, N, WIDTH), x.device)
    _tensor("mlp_backward", "dy", dy, torch.float32, (B, N, 3), x.device)
    if not acts.is_contiguous() or not dy.is_contiguous():
        raise ValueError("mlp_backward: acts and dy must be contiguous")
    P4 = param_stride(depth)
    if dparams is None:
        dparams = torch.empty(B, stride, dtype=torch.float32, device=x.device)[:, :P4]
    else:
        _tensor("mlp_backward", "dparams", dparams, torch.float32, (B, P4), x.device)
        if tuple(dparams.stride()) != tuple(params.stride()) or dparams.data_ptr() % 16:
            raise ValueError(f"mlp_backward: dparams must have the strides of params {tuple(params.stride())} and be 16-byte aligned, got "
                             f"{tuple(dparams.stride())}")
    ws = workspace("df_mlp_ws_bytes", (B, N, depth), x.device, f"mlp_backward: x: df_mlp_ws_bytes refused B = {B}, N = {N}, depth = {depth}")
    dx = torch.empty_like(x) if need_dx else None
    call("df_mlp_bwd", ptr(x), ptr(count.contiguous()), ptr(params), stride, ptr(acts), ptr(dy), B, N, depth, ptr(dparams), ptr(dx),
         ptr(ws), stream())
    return dparams, dx


class FlowMLPFn(torch.autograd.Function):
    """y = mlp(x; params) as a differentiable function of x and params (depth and count are not differentiated)"""

    @staticmethod
    def forward(ctx, x, count, params, depth):
        xd, pd = x.detach().contiguous(), params.detach()
        y, acts = mlp_forward(xd, count, pd, depth, save=True)
        ctx.save_for_backward(xd, count, pd, acts)
        ctx.depth = depth
        return y

    @staticmethod
    def backward(ctx, dy):
        x, count, params, acts = ctx.saved_tensors
        dparams, dx = mlp_backward(x, count, params, ctx.depth, acts, dy.contiguous().float(), need_dx=ctx.needs_input_grad[0])
        return dx, None, (dparams if ctx.needs_input_grad[2] else None), None


def nsfp_optimize(pc0s: torch.Tensor, count0: torch.Tensor, pc1: torch.Tensor, count1: torch.Tensor, *,
                  grid_range: Optional[Sequence[float]] = None, init: Optional[torch.Tensor] = None, **params):
    """pc0s [B,N0,3] f32 (first sweep, in the second sweep's frame) with count0 [B] i32 valid leading rows; pc1 [B,N1,3], count1 alike.
    -> flow [B,N0,3] f32 (the best iterate's residual flow; 0 for rows behind count0 and non-finite rows) and info: best_loss [B],
    loss_history [iters,B] (entries after a sample froze keep its last value; rows of iterations an early stop did not run hold the value
    they would have got: the last one), stalled [B] i32, frozen [B] bool, params [B,2,stride] (the arena after the last update),
    nn (the last iteration's neighbour indices), iters_run (host int).  Keywords: DEFAULTS; init: the [2, param_stride] start (else
    init_params(depth, seed)).  No host synchronisation unless check_every > 0 (one read of the frozen flags per check_every iterations)."""
    pair = pair_clouds("nsfp_optimize", pc0s, count0, pc1, count1, second=True)
    p = check_params(params)
    depth = p["depth"]
    S = param_stride(depth)
    start = init_params(depth, p["seed"]) if init is None else init
    if tuple(start.shape) != (2, S) or start.dtype != torch.float32:
        raise ValueError(f"nsfp_optimize: init must be float32 of shape (2, {S}), got {start.dtype} {tuple(start.shape)}")
    # the participating rows m0 / m1 (as labels: l0 / l1); everything else is 0 for the nets and masked out of the searches
    B, x0, x1, n0, n1, m0, l0, l1 = pair.B, pair.x0, pair.x1, pair.n0, pair.n1, pair.m0, pair.l0, pair.l1
    with torch.no_grad():
        arena = start.to(pair.dev)[None].repeat(B, 1, 1).contiguous()       # [B][2][S]
        loop = Loop(arena, x0, p)
        search, t2 = RowGrid(B, GRID_RANGE if grid_range is None else grid_range, CELL, pair.dev), p["trunc_d2"]
        grid_p1, grid_p0 = search.file(x1, n1, l1), search.file(x0, n0, l0)
        fpar, gpar = arena[:, 0], arena[:, 1]
        last = {"nn": None}

        def iteration():
            F, acts_f = mlp_forward(x0, n0, fpar, depth)
            F = F * m0[..., None]
            W = x0 + F
            G, acts_g = mlp_forward(W, n0, gpar, depth)
            C = W - G
            d_w1, i_w1 = search.nn(W, n0, l0, grid_p1, t2)
            d_1w, i_1w = search.nn(x1, n1, l1, search.file(W, n0, l0), t2)
            d_c0, i_c0 = search.nn(C, n0, l0, grid_p0, t2)
            d_0c, i_0c = search.nn(x0, n0, l0, search.file(C, n0, l0), t2)
            (a, ga), (b, gb), (c, gc), (d, gd) = (mean_and_weight(v) for v in (d_w1, d_1w, d_c0, d_0c))
            loss = (a + b) + (c + d)
            dW, dC = torch.zeros_like(W), torch.zeros_like(C)
            chamfer_bwd(W, x1, i_w1, ga, dW, None)
            chamfer_bwd(x1, W, i_1w, gb, None, dW)
            chamfer_bwd(C, x0, i_c0, gc, dC, None)
            chamfer_bwd(x0, C, i_0c, gd, None, dC)
            _, dxW = mlp_backward(W, n0, gpar, depth, acts_g, -dC, need_dx=True, dparams=loop.grads[:, 1])
            dF = ((dW + dC) + dxW) * m0[..., None]
            mlp_backward(x0, n0, fpar, depth, acts_f, dF, need_dx=False, dparams=loop.grads[:, 0])
            loop.snapshot(loss, F)
            loop.update()
            last["nn"] = (i_w1, i_1w, i_c0, i_0c)

        loop.run(iteration)
        return loop.result(m0, params=arena, **last)


class Nsfp(OptimisedPairModel):
    """``model=nsfp``: the interface of ``rigid.IcpFlow`` -- ``forward_padded`` and ``forward`` with ``DeFlow``'s keys, no weights --
    around ``nsfp_optimize``.  Every keyword besides point_cloud_range / voxel_size is one of DEFAULTS."""
    optimize, check_params = staticmethod(nsfp_optimize), staticmethod(check_params)

    def grid_range(self):
        r = self.point_cloud_range
        return r[0], r[1], r[3], r[4]
