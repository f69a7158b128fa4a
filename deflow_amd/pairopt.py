"""What the per-pair test-time optimisers (``model=nsfp|fastnsf|mbnsf|floxels``) share: the checks and masks of a pair of padded clouds,
the per-sample reductions, the optimisation loop -- Adam's state, the device-side snapshot / freeze rule, the eager / graph / early-stop
driver -- and the model class around an optimise function.  The four model modules import from here; this module
imports none of them.  An optimiser is its term(s) and one ``iteration`` closure that ends in ``loop.snapshot(loss, F)``,
``loop.update()``.

Only ``Loop.update`` and the graph capture need the GPU: the snapshot / freeze / early-stop rule is torch ops on whatever device the
arena is on, and tests/test_pairopt_cpu.py runs it on the host."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace
from typing import Callable, Dict, Tuple

import torch

from ._lib import call, ptr, stream
from .args import cloud, tensor as _tensor
from .pairflow import PairFlowModel

BETAS, EPS = (0.9, 0.999), 1e-8


rows = functools.partial(cloud, rows_limit=3)    # (B, N) of a CUDA float32 cloud [B,N,3], or an error of ``fn`` naming the argument


def pair_clouds(fn: str, pc0s, count0, pc1, count1, second: bool = False) -> SimpleNamespace:
    """The arguments every ``*_optimize`` starts with, checked (errors name ``fn`` and the argument) -> pc0s, pc1 (detached, contiguous),
    B, N0, N1, dev, n0, n1 (the counts clamped to the padded widths), m0 [B,N0] bool (the participating rows of the first sweep: counted
    and finite) and x0 (pc0s with 0 in every other row).  second=True: also m1, x1 and the masks as int32 labels l0, l1."""
    B, N0 = rows(fn, "pc0s", pc0s)
    B1, N1 = rows(fn, "pc1", pc1)
    dev = pc0s.device
    if B1 != B or pc1.device != dev:
        raise ValueError(f"{fn}: pc1 must have the batch size ({B}) and device of pc0s, got {tuple(pc1.shape)} on {pc1.device}")
    for name, c in (("count0", count0), ("count1", count1)):
        _tensor(fn, name, c, torch.int32, (B,), dev)
    with torch.no_grad():
        c = SimpleNamespace(pc0s=pc0s.detach().contiguous(), pc1=pc1.detach().contiguous(), B=B, N0=N0, N1=N1, dev=dev,
                            n0=count0.contiguous().clamp(0, N0), n1=count1.contiguous().clamp(0, N1))
        c.m0 = (torch.arange(N0, device=dev)[None] < c.n0[:, None]) & torch.isfinite(c.pc0s).all(dim=2)
        c.x0 = torch.where(c.m0[..., None], c.pc0s, torch.zeros_like(c.pc0s))
        if second:
            c.m1 = (torch.arange(N1, device=dev)[None] < c.n1[:, None]) & torch.isfinite(c.pc1).all(dim=2)
            c.x1 = torch.where(c.m1[..., None], c.pc1, torch.zeros_like(c.pc1))
            c.l0, c.l1 = c.m0.to(torch.int32).contiguous(), c.m1.to(torch.int32).contiguous()
    return c


def sample_sum(v: torch.Tensor) -> torch.Tensor:
    """[B, ...] -> [B]: every sample's sum, taken sample by sample over a fresh 1-D copy: torch picks a reduction's order from the
    tensor's shape and alignment, and a pair's loss must not depend on its batch."""
    return torch.stack([row.clone().sum() for row in v.unbind(0)])


def mean_and_weight(d: torch.Tensor):
    """per sample: the mean of the finite d (0 over no rows) and d mean / d d per row"""
    keep = torch.isfinite(d)
    n = keep.sum(dim=1).clamp_min(1).to(torch.float32)
    return sample_sum(torch.where(keep, d, torch.zeros_like(d))) / n, keep.to(torch.float32) / n[:, None]


class Loop:
    """One optimisation: the flat parameter ``arena`` (updated in place) with its gradient ``grads`` (the iteration writes it) and Adam's
    moments, the step counters, and the state of the snapshot / freeze rule, all on the arena's device.  p: iters, lr, patience,
    min_delta, check_every, graph; flow_like: a tensor [B,N,3] of the flow's shape.  The loop makes no host decision but the read of
    ``check_every``: one iteration is a linear chain on one stream that can be captured as a graph."""

    def __init__(self, arena: torch.Tensor, flow_like: torch.Tensor, p: Dict[str, object]):
        B, dev = int(flow_like.shape[0]), arena.device
        self.arena, self.p = arena, p
        self.grads, self.exp_avg, self.exp_avg_sq = torch.zeros_like(arena), torch.zeros_like(arena), torch.zeros_like(arena)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.t_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.best = torch.full((B,), math.inf, dtype=torch.float32, device=dev)
        self.best_flow = torch.zeros_like(flow_like)
        self.stalled = torch.zeros(B, dtype=torch.int32, device=dev)
        self.frozen = torch.zeros(B, dtype=torch.bool, device=dev)
        self.last = torch.zeros(B, dtype=torch.float32, device=dev)
        self.history = torch.zeros(p["iters"], B, dtype=torch.float32, device=dev)
        self.ran = 0

    def snapshot(self, loss: torch.Tensor, F: torch.Tensor) -> None:
        """snapshot and freeze, predicated: loss [B] and F [B,N,3] are those of the parameters before this iteration's update"""
        active = ~self.frozen
        improved = active & (loss < self.best - self.p["min_delta"])
        self.best.copy_(torch.where(improved, loss, self.best))
        self.best_flow.copy_(torch.where(improved[:, None, None], F, self.best_flow))
        self.stalled.copy_(torch.where(active, torch.where(improved, torch.zeros_like(self.stalled), self.stalled + 1), self.stalled))
        self.last.copy_(torch.where(active, loss, self.last))
        self.history.index_copy_(0, self.t_dev, self.last[None])
        self.frozen.copy_(self.frozen | (self.stalled >= self.p["patience"]))
        self.t_dev.add_(1)

    def update(self) -> None:
        """one Adam step of the whole arena on ``grads``, the step count read on the device"""
        self.step_dev.add_(1)
        call("df_adam_step_dev", ptr(self.arena), ptr(self.grads), ptr(self.exp_avg), ptr(self.exp_avg_sq), self.arena.numel(), self.p["lr"],
             BETAS[0], BETAS[1], EPS, ptr(self.step_dev), 1.0, stream())

    def run(self, iteration: Callable[[], None]) -> int:
        """run ``iteration`` p["iters"] times, eagerly or as one captured iteration replayed, with the early stop -> iterations run"""
        iters, every = self.p["iters"], self.p["check_every"]
        step, ran = iteration, 0
        if self.p["graph"] and iters > 1:
            iteration()                                    # the first iteration eagerly: it also warms the allocator
            ran = 1
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):                  # one stream: the graph is a linear chain
                iteration()
            step = graph.replay
            # (capturing launches nothing: the captured iteration first runs at the first replay)
        while ran < iters:
            step()
            ran += 1
            if every and ran % every == 0 and ran < iters and bool(self.frozen.all()):
                break
        if ran < iters:                                    # an early stop changes nothing: the rest of the history is the last value
            self.history[ran:] = self.last[None]
        self.ran = ran
        return ran

    def result(self, m0: torch.Tensor, **more):
        """-> flow (the best iterate's, 0 outside m0) and info: the keys every optimiser returns, then ``more``"""
        info = {"best_loss": self.best, "loss_history": self.history, "stalled": self.stalled, "frozen": self.frozen, "grads": self.grads,
                "iters_run": self.ran}
        info.update(more)
        return self.best_flow * m0[..., None], info


class OptimisedPairModel(PairFlowModel):
    """A ``model=`` around an optimise function: ``forward_padded`` and ``forward`` with ``DeFlow``'s keys, no weights.  Every keyword
    besides point_cloud_range / voxel_size is one of the module's DEFAULTS.  A subclass names ``optimize`` and ``check_params`` (static),
    the keys of info it keeps besides the common four (``KEEP``), and overrides ``grid_range`` / ``check_grid`` where it has to."""
    KEEP: Tuple[str, ...] = ()

    def __init__(self, point_cloud_range=(-51.2, -51.2, -3, 51.2, 51.2, 3), voxel_size=(0.2, 0.2, 6), **params):
        super().__init__(point_cloud_range, voxel_size)
        self.params = self.check_params(params)
        self.check_grid()

    def check_grid(self) -> None:
        """refuse, at construction, a grid over point_cloud_range that does not fit"""

    def grid_range(self):
        return self.point_cloud_range

    def forward_padded(self, batch: Dict[str, torch.Tensor]) -> dict:
        """flow [B,N,3]: row i < counts0[b] is the residual flow of input row idx_c0[b,i] (the decoded rows in ascending order), 0 behind
        them; pose_flow [B,N,3] of every input row.  Reads nothing back when check_every = 0."""
        st = self._pair(batch)
        flow, info = self.optimize(st["points_c0"], st["counts0"], st["points_c1"], st["counts1"], grid_range=self.grid_range(), **self.params)
        st["flow"] = flow
        st.update({k: info[k] for k in ("best_loss", "loss_history", "stalled", "frozen") + self.KEEP})
        self.last_state = st
        return st
