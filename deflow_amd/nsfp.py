"""Per-pair neural flow prior on the GPU (``model=nsfp``): two small coordinate MLPs per pair of sweeps, optimised at test time against a
truncated two-way chamfer distance, with no weights and no checkpoint.

UNPINNED: the recipe is NSFP's (Li, Pontes & Lucey, NeurIPS'21) -- a forward net f and an inverse net g per pair, the flow read off the
best iterate -- but upstream's source is absent, and every choice here is this project's own.  The definition is in DESIGN.md section 6k
and include/deflow_amd.h; tests/helpers/nsfp_ref.py restates it in torch.  The MLPs run on csrc/mlp.hip (forward, data gradient and
weight gradient on the fp32 MFMA), the searches on csrc/chamfer.hip, the update on df_adam_step_dev.

CUDA tensors only, like the rest of the library: there is no CPU fallback.  The loop makes no host decision: the step counter, the
snapshot and the freeze live on the device, so one iteration can be captured as a HIP graph (``graph=True``)."""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import pairflow
from ._lib import call, ptr, stream
from .chamfer import CELL, GRID_RANGE, _grid, chamfer_bwd
from .pairflow import PairFlowModel

WIDTH = 128
ROW_TILE = 64            # rows per workgroup of the forward / data-gradient kernels (csrc/mlp.hip: MT)
WGRAD_SPLIT_ROWS = 1024  # rows per weight-gradient split (csrc/mlp.hip: MSPLIT)
MAX_DEPTH = 15

# every default of section 6k; all of them are arguments of nsfp_optimize and Nsfp, and `nsfp_<name>=` keys of the commands
DEFAULTS: Dict[str, object] = {"depth": 7, "iters": 1000, "lr": 8e-3, "trunc_d2": 4.0, "patience": 100, "min_delta": 1e-4,
                               "check_every": 50, "seed": 0, "graph": False}
COMMAND_KEYS: Dict[str, str] = {"nsfp_" + k: k for k in DEFAULTS}
BETAS, EPS = (0.9, 0.999), 1e-8
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
_tensor = functools.partial(pairflow._tensor, other="x is")     # (a device mismatch is reported against x)


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
    need = int(call("df_mlp_ws_bytes", B, N, depth))
    if need < 0:
        raise ValueError(f"mlp_backward: x: df_mlp_ws_bytes refused B = {B}, N = {N}, depth = {depth}")
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=x.device)
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


# ---- the searches ----------------------------------------------------------------------------------------------------------------------
class _Search:
    """df_nn_grid_build / df_chamfer_nn with the grid of a static cloud kept between iterations"""

    def __init__(self, B: int, grid_range: Sequence[float], cell: float, max_dist2: float, device):
        self.B, self.cell, self.max_dist2, self.dev = B, float(cell), float(max_dist2), device
        self.minx, self.miny, self.G = _grid(B, grid_range, cell)

    def build(self, ref: torch.Tensor, rcount: torch.Tensor, rlabel: torch.Tensor):
        B, Nr = self.B, ref.shape[1]
        cell_rng = torch.empty(B * self.G * self.G, 2, dtype=torch.int32, device=self.dev)
        rows = torch.empty(B * Nr, 4, dtype=torch.float32, device=self.dev)
        ws = torch.empty(call("df_nn_grid_ws_bytes", B, Nr, self.G), dtype=torch.uint8, device=self.dev)
        call("df_nn_grid_build", ptr(ref), ptr(rcount), ptr(rlabel), B, Nr, self.minx, self.miny, self.cell, self.G, ptr(cell_rng),
             ptr(rows), ptr(ws), stream())
        return cell_rng, rows

    def nn(self, query: torch.Tensor, qcount: torch.Tensor, qlabel: torch.Tensor, grid):
        B, Nq = self.B, query.shape[1]
        d2 = torch.empty(B, Nq, dtype=torch.float32, device=self.dev)
        idx = torch.empty(B, Nq, dtype=torch.int32, device=self.dev)
        call("df_chamfer_nn", ptr(query), ptr(qcount), ptr(qlabel), B, Nq, ptr(grid[0]), ptr(grid[1]), self.minx, self.miny, self.cell,
             self.G, self.max_dist2, ptr(d2), ptr(idx), None, stream())
        return d2, idx


def _mean_and_weight(d2: torch.Tensor):
    """per sample: the mean of the finite d2 (0 over no rows) and d mean / d d2 per row.  The sum is taken sample by sample over a fresh
    1-D copy: torch picks a reduction's order from the tensor's shape and alignment, and a pair's loss must not depend on its batch."""
    keep = torch.isfinite(d2)
    n = keep.sum(dim=1).clamp_min(1).to(torch.float32)
    kept = torch.where(keep, d2, torch.zeros_like(d2))
    total = torch.stack([row.clone().sum() for row in kept.unbind(0)])
    return total / n, keep.to(torch.float32) / n[:, None]


def _loop_state(B: int, iters: int, flow_like: torch.Tensor) -> dict:
    """the device-side state of the snapshot / freeze rules (shared with deflow_amd.fastnsf)"""
    dev = flow_like.device
    return {"best": torch.full((B,), math.inf, dtype=torch.float32, device=dev), "best_flow": torch.zeros_like(flow_like),
            "stalled": torch.zeros(B, dtype=torch.int32, device=dev), "frozen": torch.zeros(B, dtype=torch.bool, device=dev),
            "last": torch.zeros(B, dtype=torch.float32, device=dev),
            "history": torch.zeros(iters, B, dtype=torch.float32, device=dev)}


def _snapshot_and_freeze(st: dict, loss: torch.Tensor, F: torch.Tensor, t_dev: torch.Tensor, p: Dict[str, object]) -> None:
    """snapshot and freeze, predicated: the loss is that of the parameters before this iteration's update"""
    active = ~st["frozen"]
    improved = active & (loss < st["best"] - p["min_delta"])
    st["best"].copy_(torch.where(improved, loss, st["best"]))
    st["best_flow"].copy_(torch.where(improved[:, None, None], F, st["best_flow"]))
    st["stalled"].copy_(torch.where(active, torch.where(improved, torch.zeros_like(st["stalled"]), st["stalled"] + 1), st["stalled"]))
    st["last"].copy_(torch.where(active, loss, st["last"]))
    st["history"].index_copy_(0, t_dev, st["last"][None])
    st["frozen"].copy_(st["frozen"] | (st["stalled"] >= p["patience"]))
    t_dev.add_(1)


def _run(iteration, st: dict, p: Dict[str, object]) -> int:
    """run `iteration` p["iters"] times, eagerly or as one captured iteration replayed, with the early stop -> iterations run"""
    iters = p["iters"]
    run = iteration
    ran = 0
    if p["graph"] and iters > 1:
        iteration()                                    # the first iteration eagerly: it also warms the allocator
        ran = 1
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                  # one stream: the graph is a linear chain
            iteration()
        run = graph.replay
        # (capturing launches nothing: the captured iteration first runs at the first replay)
    every = p["check_every"]
    while ran < iters:
        run()
        ran += 1
        if every and ran % every == 0 and ran < iters and bool(st["frozen"].all()):
            break
    if ran < iters:                                    # an early stop changes nothing: the rest of the history is the last value
        st["history"][ran:] = st["last"][None]
    return ran


def _cloud(name: str, t) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"nsfp_optimize: {name} must be a CUDA tensor (deflow_amd has no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"nsfp_optimize: {name} must be torch.float32 of shape (B, N, 3) with B >= 1 and N >= 1, got "
                         f"{t.dtype} {tuple(t.shape)}")
    return int(t.shape[1])


def nsfp_optimize(pc0s: torch.Tensor, count0: torch.Tensor, pc1: torch.Tensor, count1: torch.Tensor, *,
                  grid_range: Optional[Sequence[float]] = None, init: Optional[torch.Tensor] = None, **params):
    """pc0s [B,N0,3] f32 (first sweep, in the second sweep's frame) with count0 [B] i32 valid leading rows; pc1 [B,N1,3], count1 alike.
    -> flow [B,N0,3] f32 (the best iterate's residual flow; 0 for rows behind count0 and non-finite rows) and info: best_loss [B],
    loss_history [iters,B] (entries after a sample froze keep its last value; rows of iterations an early stop did not run hold the value
    they would have got: the last one), stalled [B] i32, frozen [B] bool, params [B,2,stride] (the arena after the last update),
    nn (the last iteration's neighbour indices), iters_run (host int).  Keywords: DEFAULTS; init: the [2, param_stride] start (else
    init_params(depth, seed)).  No host synchronisation unless check_every > 0 (one read of the frozen flags per check_every iterations)."""
    N0, N1 = _cloud("pc0s", pc0s), _cloud("pc1", pc1)
    B, dev = int(pc0s.shape[0]), pc0s.device
    if pc1.shape[0] != B or pc1.device != dev:
        raise ValueError(f"nsfp_optimize: pc1 must have the batch size ({B}) and device of pc0s, got {tuple(pc1.shape)} on {pc1.device}")
    for name, c in (("count0", count0), ("count1", count1)):
        _tensor("nsfp_optimize", name, c, torch.int32, (B,), dev)
    p = check_params(params)
    depth, iters = p["depth"], p["iters"]
    S = param_stride(depth)
    start = init_params(depth, p["seed"]) if init is None else init
    if tuple(start.shape) != (2, S) or start.dtype != torch.float32:
        raise ValueError(f"nsfp_optimize: init must be float32 of shape (2, {S}), got {start.dtype} {tuple(start.shape)}")
    with torch.no_grad():
        pc0s, pc1 = pc0s.detach().contiguous(), pc1.detach().contiguous()
        count0, count1 = count0.contiguous(), count1.contiguous()
        # participating rows; everything else is 0 for the nets and masked out of the searches
        m0 = (torch.arange(N0, device=dev)[None] < count0[:, None]) & torch.isfinite(pc0s).all(dim=2)
        m1 = (torch.arange(N1, device=dev)[None] < count1[:, None]) & torch.isfinite(pc1).all(dim=2)
        x0 = torch.where(m0[..., None], pc0s, torch.zeros_like(pc0s))
        x1 = torch.where(m1[..., None], pc1, torch.zeros_like(pc1))
        l0, l1 = m0.to(torch.int32).contiguous(), m1.to(torch.int32).contiguous()
        n0, n1 = count0.clamp(0, N0), count1.clamp(0, N1)
        arena = start.to(dev)[None].repeat(B, 1, 1).contiguous()       # [B][2][S]
        grads = torch.zeros_like(arena)
        exp_avg, exp_avg_sq = torch.zeros_like(arena), torch.zeros_like(arena)
        step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        t_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        search = _Search(B, GRID_RANGE if grid_range is None else grid_range, CELL, p["trunc_d2"], dev)
        grid_p1, grid_p0 = search.build(x1, n1, l1), search.build(x0, n0, l0)
        st = _loop_state(B, iters, x0)
        st["nn"] = None
        fpar, gpar = arena[:, 0], arena[:, 1]

        def iteration():
            F, acts_f = mlp_forward(x0, n0, fpar, depth)
            F = F * m0[..., None]
            W = x0 + F
            G, acts_g = mlp_forward(W, n0, gpar, depth)
            C = W - G
            d_w1, i_w1 = search.nn(W, n0, l0, grid_p1)
            d_1w, i_1w = search.nn(x1, n1, l1, search.build(W, n0, l0))
            d_c0, i_c0 = search.nn(C, n0, l0, grid_p0)
            d_0c, i_0c = search.nn(x0, n0, l0, search.build(C, n0, l0))
            (a, ga), (b, gb), (c, gc), (d, gd) = (_mean_and_weight(v) for v in (d_w1, d_1w, d_c0, d_0c))
            loss = (a + b) + (c + d)
            dW, dC = torch.zeros_like(W), torch.zeros_like(C)
            chamfer_bwd(W, x1, i_w1, ga, dW, None)
            chamfer_bwd(x1, W, i_1w, gb, None, dW)
            chamfer_bwd(C, x0, i_c0, gc, dC, None)
            chamfer_bwd(x0, C, i_0c, gd, None, dC)
            _, dxW = mlp_backward(W, n0, gpar, depth, acts_g, -dC, need_dx=True, dparams=grads[:, 1])
            dF = ((dW + dC) + dxW) * m0[..., None]
            mlp_backward(x0, n0, fpar, depth, acts_f, dF, need_dx=False, dparams=grads[:, 0])
            _snapshot_and_freeze(st, loss, F, t_dev, p)
            step_dev.add_(1)
            call("df_adam_step_dev", ptr(arena), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), arena.numel(), p["lr"], BETAS[0], BETAS[1], EPS,
                 ptr(step_dev), 1.0, stream())
            st["nn"] = (i_w1, i_1w, i_c0, i_0c)

        ran = _run(iteration, st, p)
        flow = st["best_flow"] * m0[..., None]
    info = {"best_loss": st["best"], "loss_history": st["history"], "stalled": st["stalled"], "frozen": st["frozen"], "params": arena,
            "grads": grads, "nn": st["nn"], "iters_run": ran}
    return flow, info


class Nsfp(PairFlowModel):
    """``model=nsfp``: the interface of ``rigid.IcpFlow`` -- ``forward_padded`` and ``forward`` with ``DeFlow``'s keys, no weights --
    around ``nsfp_optimize``.  Every keyword besides point_cloud_range / voxel_size is one of DEFAULTS."""

    def __init__(self, point_cloud_range=(-51.2, -51.2, -3, 51.2, 51.2, 3), voxel_size=(0.2, 0.2, 6), **params):
        super().__init__(point_cloud_range, voxel_size)
        self.params = check_params(params)

    def forward_padded(self, batch: Dict[str, torch.Tensor]) -> dict:
        """flow [B,N,3]: row i < counts0[b] is the residual flow of input row idx_c0[b,i] (the decoded rows in ascending order), 0 behind
        them; pose_flow [B,N,3] of every input row.  Reads nothing back when check_every = 0."""
        st = self._pair(batch)
        r = self.point_cloud_range
        flow, info = nsfp_optimize(st["points_c0"], st["counts0"], st["points_c1"], st["counts1"], grid_range=(r[0], r[1], r[3], r[4]),
                                   **self.params)
        st.update({"flow": flow, "best_loss": info["best_loss"], "loss_history": info["loss_history"], "stalled": info["stalled"],
                   "frozen": info["frozen"]})
        self.last_state = st
        return st
