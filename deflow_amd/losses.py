"""The two ablation losses of the reference's ``loss_fn=`` switch next to deflowLoss ([REF assets/slurm/1_train.sh:58-78]:
``loss_fn = [ff3dLoss (R), zeroflowLoss, deflowLoss]``; [REF README.md:68]: the fastflow3d baseline trains with ff3dLoss).
Their definitions live in the absent OpenSceneFlow submodule (``src/lossfuncs.py``) and are recalled from FastFlow3D / ZeroFlow:

  ff3dLoss      mean over points of |est - gt| * (0.1 for background points (class 0), 1.0 for foreground)
  zeroflowLoss  mean over points of |est - gt| * clamp(1.8 * speed - 0.8, 0.1, 1.0),  speed = |gt| * 10 (m/s at 10 Hz)

each per sample, summed over the batch like deflowLoss in the trainer.  deflowLoss -- the north-star loss -- has its own
HIP kernels (autograd.DeflowLossFn).  Round 5: the Trainer's direct step evaluates these two with HIP kernels as well
(csrc/misc.hip: df_wloss_fwd / _finalize / _bwd, the same definitions); the torch form below serves autograd callers
(Trainer.loss_on_last_forward) and is the kernels' twin in tests/test_gpu_model.py::test_ablation_losses_vs_oracle.

seflowLoss (further down) is the self-supervised loss of the SeFlow mode: sync-free torch reductions over the HIP nearest-neighbour
searches of csrc/chamfer.hip; the Trainer uses it on both of its routes."""
from __future__ import annotations

from typing import Optional

import torch


def _rows(est: torch.Tensor, gt: torch.Tensor, counts: torch.Tensor):
    B, N, _ = est.shape
    valid = torch.arange(N, device=est.device)[None, :] < counts[:, None]
    valid = valid & torch.isfinite(gt).all(-1) & torch.isfinite(est.detach()).all(-1)
    diff = torch.where(valid[..., None], est - gt, torch.zeros_like(est))
    # |d| with a zero (not NaN) gradient at masked rows
    err = torch.where(valid, torch.linalg.vector_norm(torch.where(valid[..., None], diff, torch.ones_like(diff)), dim=-1),
                      torch.zeros_like(diff[..., 0]))
    return err, valid


def _sum_of_sample_means(err: torch.Tensor, weight: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    n = valid.sum(1)
    per = (err * weight * valid).sum(1) / n.clamp_min(1)
    return per[n > 0].sum()


def ff3d_loss(est: torch.Tensor, gt: torch.Tensor, counts: torch.Tensor, classes: Optional[torch.Tensor]) -> torch.Tensor:
    if classes is None:
        raise ValueError("loss_fn=ff3dLoss needs batch['flow_category_indices'] (labelled scene files)")
    err, valid = _rows(est, gt, counts)
    return _sum_of_sample_means(err, (classes > 0).float() * 0.9 + 0.1, valid)


def zeroflow_loss(est: torch.Tensor, gt: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    err, valid = _rows(est, gt, counts)
    speed = torch.linalg.vector_norm(torch.where(valid[..., None], gt, torch.zeros_like(gt)), dim=-1) * 10.0
    return _sum_of_sample_means(err, torch.clamp(1.8 * speed - 0.8, 0.1, 1.0), valid)


# ---- seflowLoss: the self-supervised loss of SeFlow (ECCV'24, Eq. 6-11) the reference merged into the same code base ([REF README.md:16-18]).
# UNPINNED: upstream's src/lossfuncs.py::seflowLoss is in the absent submodule; the form below is the recalled one.
TRUNCATED_DIST = 4.0      # squared metres: upstream's cut-off of the chamfer means


def _nn_dist(nn_fn, query, qcount, ref, rcount, qlabel, rlabel, max_dist2):
    """the search (no gradient) and, on top of it, d2 as a differentiable function of the clouds: csrc/chamfer.hip's deterministic
    backward on the GPU, plain gathers elsewhere (CPU tensors with an injected brute-force search: tests)"""
    d2, idx = nn_fn(query.detach(), qcount, ref.detach(), rcount, qlabel, rlabel, max_dist2)
    if not (query.requires_grad or ref.requires_grad):
        return d2, idx
    if query.is_cuda:
        from .chamfer import NNDistFn
        return NNDistFn.apply(query, ref, d2, idx), idx
    hit = idx >= 0
    near = torch.gather(ref, 1, idx.clamp_min(0).long()[..., None].expand(-1, -1, 3))
    diff = torch.where(hit[..., None], query - near, torch.zeros_like(query))
    return torch.where(hit, (diff * diff).sum(-1), torch.full_like(d2, float("inf"))), idx


def _tmean(d2: torch.Tensor, trunc: float) -> torch.Tensor:
    """per sample: mean of d2 over the rows with d2 <= trunc (rows without a neighbour hold +inf); 0 when there is none"""
    keep = d2.detach() <= trunc
    return torch.where(keep, d2, torch.zeros_like(d2)).sum(1) / keep.sum(1).clamp_min(1)


def _norm_rows(v: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """|v_i| on `rows`, 0 elsewhere, with a zero (not NaN) gradient at masked rows and at v = 0 (as _rows above)"""
    v = torch.where(rows[..., None], v, torch.zeros_like(v))
    return torch.where(rows, torch.linalg.vector_norm(torch.where(rows[..., None], v, torch.ones_like(v)), dim=-1), torch.zeros_like(v[..., 0]))


def seflow_loss(pc0: torch.Tensor, pc1: torch.Tensor, flow: torch.Tensor, counts0: torch.Tensor, counts1: torch.Tensor,
                lab0: torch.Tensor, lab1: torch.Tensor, weights=(1.0, 1.0, 1.0, 1.0), min_dynamic: int = 256, nn_fn=None,
                truncate_dist: float = TRUNCATED_DIST, max_label: Optional[int] = None, stats: Optional[dict] = None):
    """pc0 [B,N,3] the compacted ego-compensated pc0 points, pc1 [B,M,3] the compacted pc1 points, flow [B,N,3] the residual flow,
    counts0 / counts1 [B] valid leading rows, lab0 [B,N] / lab1 [B,M] integer cluster labels (0 = static, > 0 = a dynamic cluster).
    -> (loss, terms [B,4]); loss = sum over samples of the weighted sum of, with p = pc0 + flow, T = truncate_dist and tmean = the mean
    over rows with squared distance <= T:

      0 chamfer_dis          tmean(nn(p -> pc1)) + tmean(nn(pc1 -> p))
      1 dynamic_chamfer_dis  the same between the rows with label > 0 of either cloud; only if the sample has_dynamic = both clouds
                             hold more than min_dynamic such rows, else 0
      2 static_flow_loss     mean of |flow_i| over the rows with label 0
      3 cluster_flow_loss    only if has_dynamic: with (rd, ri) = nn(pc0 -> pc1) on the raw clouds, every cluster c > 0 of lab0 takes,
                             among its rows whose neighbour is dynamic too, the one with the largest rd (lowest row on equal rd), m;
                             its target flow is pc1[ri[m]] - pc0[m] (a constant); clusters without such a row are left out; the term
                             is the mean of |flow_i - target_c| over all rows of the remaining clusters.  No cluster left: the
                             constant tmean(nn(pc0 -> pc1)) + tmean(nn(pc1 -> pc0)).

    A mean over zero rows is 0 here (upstream yields NaN).  Only `flow` receives a gradient; |v| has a zero gradient at v = 0.
    No host read anywhere when max_label is given: the per-label tables have max_label + 1 slots, and rows whose label exceeds it are
    counted into stats["label_overflow"] (they stay dynamic for terms 1-2 and are left out of term 3).  max_label=None reads the
    largest label back (convenience outside the training step).  nn_fn: the search, chamfer.chamfer_nn by default; any function
    of the same signature (tests inject a brute-force one and run this on CPU tensors in float64)."""
    if nn_fn is None:
        from .chamfer import chamfer_nn as nn_fn
    B, N, _ = pc0.shape
    M = pc1.shape[1]
    dev = pc0.device
    if max_label is None:
        max_label = int(lab0.max()) if lab0.numel() else 0
    L = max(int(max_label), 0) + 1
    valid0 = (torch.arange(N, device=dev)[None, :] < counts0[:, None]) & torch.isfinite(pc0).all(-1) & torch.isfinite(flow.detach()).all(-1)
    valid1 = (torch.arange(M, device=dev)[None, :] < counts1[:, None]) & torch.isfinite(pc1).all(-1)
    l0 = torch.where(valid0, lab0.long(), torch.zeros_like(lab0, dtype=torch.long))
    l1 = torch.where(valid1, lab1.long(), torch.zeros_like(lab1, dtype=torch.long))
    dyn0, dyn1 = l0 > 0, l1 > 0
    has_dyn = (dyn0.sum(1) > min_dynamic) & (dyn1.sum(1) > min_dynamic)
    zero = torch.zeros(B, dtype=flow.dtype, device=dev)
    # rows with a non-finite flow (a diverged model) take part in nothing: NaN rows never enter a search
    p = torch.where(valid0[..., None], pc0 + flow, torch.full_like(flow, float("nan")))
    T = float(truncate_dist)

    # 0: chamfer between the moved cloud and pc1
    chamfer = _tmean(_nn_dist(nn_fn, p, counts0, pc1, counts1, None, None, T)[0], T) + \
        _tmean(_nn_dist(nn_fn, pc1, counts1, p, counts0, None, None, T)[0], T)
    # 1: the same between the dynamic rows
    l0i, l1i = l0.to(torch.int32), l1.to(torch.int32)
    dyn_chamfer = _tmean(_nn_dist(nn_fn, p, counts0, pc1, counts1, l0i, l1i, T)[0], T) + \
        _tmean(_nn_dist(nn_fn, pc1, counts1, p, counts0, l1i, l0i, T)[0], T)
    dyn_chamfer = torch.where(has_dyn, dyn_chamfer, zero)
    # 2: static rows should not move
    stat = valid0 & (l0 == 0)
    static = _norm_rows(flow, stat).sum(1) / stat.sum(1).clamp_min(1)
    # 3: one target flow per dynamic cluster -- a segmented arg-max by label through per-sample tables of L slots (slot 0 takes the rest)
    inf = float("inf")
    rd, ri = nn_fn(pc0, counts0, pc1, counts1, None, None, inf)
    rd1, _ = nn_fn(pc1, counts1, pc0, counts0, None, None, inf)
    rd = rd.to(flow.dtype)
    rij = ri.clamp_min(0).long()
    inl = dyn0 & (l0 < L)
    elig = inl & (ri >= 0) & torch.gather(dyn1, 1, rij)
    slot = torch.where(inl, l0, torch.zeros_like(l0))
    best = torch.full((B, L), -inf, dtype=rd.dtype, device=dev).scatter_reduce(
        1, slot, torch.where(elig, rd, torch.full_like(rd, -inf)), "amax", include_self=True)
    is_best = elig & (rd == torch.gather(best, 1, slot))
    rows = torch.arange(N, device=dev)[None, :].expand(B, N)
    m = torch.full((B, L), N, dtype=torch.long, device=dev).scatter_reduce(
        1, slot, torch.where(is_best, rows, torch.full_like(rows, N)), "amin", include_self=True)
    has_target = m < N
    has_target[:, 0] = False
    m = m.clamp_max(N - 1)
    e3 = lambda t: t[..., None].expand(-1, -1, 3)
    target = torch.gather(pc1, 1, e3(torch.gather(rij, 1, m))) - torch.gather(pc0, 1, e3(m))          # [B,L,3], constants
    in_cluster = inl & torch.gather(has_target, 1, slot)
    n_cl = in_cluster.sum(1)
    cluster = _norm_rows(flow - torch.gather(target, 1, e3(slot)).to(flow.dtype), in_cluster).sum(1) / n_cl.clamp_min(1)
    fallback = (_tmean(rd, T) + _tmean(rd1.to(flow.dtype), T)).to(flow.dtype)
    cluster = torch.where(has_dyn, torch.where(n_cl > 0, cluster, fallback), zero)

    terms = torch.stack([chamfer.to(flow.dtype), dyn_chamfer.to(flow.dtype), static, cluster], 1)
    if stats is not None:
        stats["label_overflow"] = (l0 >= L).sum().to(torch.int32).reshape(1)
    w = [float(v) for v in weights]       # (Python floats: no host-to-device copy inside a captured step)
    if len(w) != 4:
        raise ValueError(f"seflow_loss: weights must have 4 entries, got {len(w)}")
    per_term = terms.sum(0)
    return w[0] * per_term[0] + w[1] * per_term[1] + w[2] * per_term[2] + w[3] * per_term[3], terms
