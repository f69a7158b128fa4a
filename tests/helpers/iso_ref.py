"""A naive restatement of DESIGN.md section 6m (model=mbnsf) that shares nothing with csrc/iso.hip: the ordered row lists of the clusters,
the stride rule, the neighbour table and the number of pair instances in numpy; the rigidity term in the dtype it is given, with its
gradient through torch.autograd (not the analytic form); one iteration and the whole loop on dt_ref's lookup and nsfp_ref's MLP and Adam."""
import math

import numpy as np
import torch

from helpers import dt_ref as dr
from helpers import nsfp_ref as nr


def strides(n, P):
    """s_k = 1 + floor((k - 1)(n - 1) / P), k = 1..P, for a list of n >= 2 rows"""
    return [1 + ((k - 1) * (n - 1)) // P for k in range(1, P + 1)]


def lists(labels, count, kcap=None):
    """{label: its rows below `count` in ascending order} for the labels 1..kcap (default: every positive label)"""
    labels = np.asarray(labels)
    head = labels[:max(int(count), 0)]
    return {int(l): np.flatnonzero(head == l) for l in np.unique(head) if l >= 1 and (kcap is None or l <= kcap)}


def table(labels, count, P, max_cluster_points, kcap=None):
    """labels [N] of one sample -> nbr int64 [N, 2P] (forward partners for k = 1..P, then backward ones; -1 without partners), M"""
    N = len(labels)
    nbr = np.full((N, 2 * P), -1, np.int64)
    M = 0
    for L in lists(labels, count, kcap).values():
        n = len(L)
        if not 2 <= n <= max_cluster_points:
            continue
        pos = np.arange(n)
        for k, s in enumerate(strides(n, P)):
            nbr[L, k] = L[(pos + s) % n]
            nbr[L, P + k] = L[(pos - s) % n]
        M += P * n
    return nbr, M


def dist(a, b):
    """|a - b| per row: differences first, then ((dx dx + dy dy) + dz dz) in the dtype given; the slope at 0 is taken as 0"""
    d = a - b
    s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    pos = s > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))


def rest(x, nbr):
    """x [N,3] -> r0 [N,2P] in the dtype of x, 0 at -1"""
    nb = torch.as_tensor(nbr)
    r = dist(x[:, None, :], x[nb.clamp_min(0)])
    return torch.where(nb >= 0, r, torch.zeros_like(r))


def rho(e, delta):
    return torch.where(e <= delta, e * e, delta * (2 * e - delta))


def term(W, nbr, r0, delta):
    """W [N,3] (differentiable) -> v [N] (rho summed over each row's P forward instances), the per-instance e [N,P] of the forward half"""
    nb = torch.as_tensor(nbr)
    P = nb.shape[1] // 2
    fwd = nb[:, :P]
    e = (dist(W[:, None, :], W[fwd.clamp_min(0)]) - r0[:, :P]).abs()
    val = torch.where(fwd >= 0, rho(e, torch.tensor(delta, dtype=W.dtype)), torch.zeros_like(e))
    return val.sum(dim=1), e


def term_and_grad(W, nbr, r0, delta):
    """-> v [N], g [N,3] = d (sum of v) / d W by torch.autograd in the dtype of W, e [N,P]"""
    W = W.detach().clone().requires_grad_(True)
    v, e = term(W, nbr, r0, delta)
    g, = torch.autograd.grad(v.sum(), W)
    return v.detach(), g, e.detach()


def iteration(P0, dt2, origin, cell, R, f_flat, depth, nbr, M, weight, delta, cells=None):
    """one iteration of section 6m on one sample, by torch.autograd over nsfp_ref's forward, dt_ref's lookup and this file's term, in the
    dtype of P0 -> loss, (data, iso), F, d loss / d f, the lookup's cells, W"""
    f_flat = f_flat.detach().clone().requires_grad_(True)
    r0 = rest(P0, nbr)
    F = nr.mlp_forward(P0, f_flat, depth)[0]
    W = P0 + F
    d, _, cells, _ = dr.lookup(W, dt2, origin, cell, R, cells)
    data = d.sum() / max(P0.shape[0], 1)
    iso = term(W, nbr, r0, delta)[0].sum() / max(M, 1)
    loss = data + weight * iso
    df, = torch.autograd.grad(loss, f_flat)
    return loss.detach(), (data.detach(), iso.detach()), F.detach(), df, cells, W.detach()


def optimize(P0, dt2, origin, cell, R, f_flat, depth, iters, nbr, M, weight, delta, lr=8e-3, patience=100, min_delta=1e-4):
    """the whole loop of section 6m on one sample -> best_flow, best_loss, history"""
    m, v = torch.zeros_like(f_flat), torch.zeros_like(f_flat)
    best, best_flow, stalled, hist = math.inf, torch.zeros_like(P0), 0, []
    for t in range(1, iters + 1):
        loss, _, F, df, _, _ = iteration(P0, dt2, origin, cell, R, f_flat, depth, nbr, M, weight, delta)
        hist.append(float(loss))
        if float(loss) < best - min_delta:
            best, best_flow, stalled = float(loss), F, 0
        else:
            stalled += 1
        if stalled >= patience:
            break
        f_flat, m, v = nr.adam_step(f_flat, df, m, v, t, lr)
    return best_flow, best, hist


def same_partition(a, b):
    """True when the label vectors a and b describe the same partition up to renaming (0 stays 0)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or not np.array_equal(a == 0, b == 0):
        return False
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs})
