"""A naive restatement of DESIGN.md section 6n (model=floxels) that shares nothing with csrc/voxflow.hip: the grid, the rows' cells and
fractions (index arithmetic in fp32), their grouping, the active nodes and the pair count in numpy; the trilinear field and the
smoothness term in the dtype they are given, the transpose of the read and the term's gradient through torch.autograd (not the transposed
or analytic forms); one iteration and the whole loop on dt_ref's lookup and nsfp_ref's Adam."""
import math

import numpy as np
import torch

from helpers import dt_ref as dr
from helpers import nsfp_ref as nr


def grid(grid_range, voxel):
    """-> origin (3 floats as fp32 holds them), dims (VX, VY, VZ): ceil((max - min) / voxel - 1e-6) + 1 nodes per axis, at least 2"""
    dims = tuple(max(int(math.ceil((grid_range[3 + a] - grid_range[a]) / voxel - 1e-6)) + 1, 2) for a in range(3))
    return tuple(dr.f32(grid_range[a]) for a in range(3)), dims


def n_cells(dims):
    return (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)


def plan(x, count, origin, voxel, dims):
    """x [N,3] float32 of one sample -> cell int64 [N] (-1: the row does not take part), frac float32 [N,3], idx int64 [N,3] (ix, iy, iz; 0
    at -1).  u = (x - o) / voxel in fp32, clamped to [0, V - 1]; i = min(floor(u), V - 2); t = u - i."""
    x = np.asarray(x, dtype=np.float32)
    N = x.shape[0]
    part = (np.arange(N) < max(int(count), 0)) & np.isfinite(x).all(axis=1)
    xs = np.where(part[:, None], x, np.float32(0))
    V = np.array(dims, dtype=np.int64)
    with np.errstate(all="ignore"):
        u = (xs - np.array(origin, dtype=np.float32)) / np.float32(voxel)
    assert u.dtype == np.float32
    u = np.minimum(np.maximum(u, np.float32(0)), (V - 1).astype(np.float32))
    i = np.minimum(np.floor(u).astype(np.int64), V - 2)
    t = (u - i.astype(np.float32)).astype(np.float32)
    cell = (i[:, 2] * (V[1] - 1) + i[:, 1]) * (V[0] - 1) + i[:, 0]
    cell = np.where(part, cell, -1)
    return cell, np.where(part[:, None], t, np.float32(0)).astype(np.float32), np.where(part[:, None], i, 0)


def grouping(cells, NC):
    """cells: one int64 [N] per sample -> idx_sorted int64 [B N] (b N + row: grouped by (sample, cell), ascending inside a cell; -1
    behind the grouped rows), cell_rng int64 [B NC, 2] (first, end)"""
    B, N = len(cells), len(cells[0])
    key = np.concatenate([np.where(c >= 0, b * NC + c, -1) for b, c in enumerate(cells)])
    rows = np.flatnonzero(key >= 0)
    order = rows[np.argsort(key[rows], kind="stable")]
    idx_sorted = np.full(B * N, -1, np.int64)
    idx_sorted[:len(order)] = order
    cnt = np.bincount(key[rows], minlength=B * NC)
    end = np.cumsum(cnt)
    return idx_sorted, np.stack([end - cnt, end], axis=1)


def active_nodes(cell, dims):
    """cell int64 [N] -> bool [VZ,VY,VX]: the corners of every cell that holds a row; M: the axis-adjacent pairs with both ends active"""
    VX, VY, VZ = dims
    act = np.zeros((VZ, VY, VX), bool)
    c = np.unique(cell[cell >= 0])
    ix, r = c % (VX - 1), c // (VX - 1)
    iy, iz = r % (VY - 1), r // (VY - 1)
    for e in (0, 1):
        for d in (0, 1):
            for a in (0, 1):
                act[iz + e, iy + d, ix + a] = True
    return act, n_pairs(act)


def n_pairs(act):
    return int((act[:, :, 1:] & act[:, :, :-1]).sum() + (act[:, 1:] & act[:, :-1]).sum() + (act[1:] & act[:-1]).sum())


def sample(theta, cell, frac, idx):
    """theta [VZ,VY,VX,3] in the dtype to compute in (differentiable) -> F [N,3]: the 8 corners weighted (wx wy) wz; 0 where cell = -1"""
    dt = theta.dtype
    t = torch.as_tensor(frac).to(dt)
    i = torch.as_tensor(idx)
    F = torch.zeros(t.shape[0], 3, dtype=dt)
    for e in (0, 1):
        for d in (0, 1):
            for a in (0, 1):
                w = ((t[:, 0] if a else 1 - t[:, 0]) * (t[:, 1] if d else 1 - t[:, 1])) * (t[:, 2] if e else 1 - t[:, 2])
                F = F + w[:, None] * theta[i[:, 2] + e, i[:, 1] + d, i[:, 0] + a]
    return torch.where(torch.as_tensor(cell >= 0)[:, None], F, torch.zeros_like(F))


def scatter(dF, cell, frac, idx, dims, dtype):
    """the transpose of `sample` by torch.autograd: d <sample(theta), dF> / d theta -> [VZ,VY,VX,3]; rows with cell = -1 are not read"""
    theta = torch.zeros(dims[2], dims[1], dims[0], 3, dtype=dtype, requires_grad=True)
    keep = torch.as_tensor(cell >= 0)[:, None]
    dFc = torch.where(keep, dF.to(dtype), torch.zeros(1, dtype=dtype))
    g, = torch.autograd.grad((sample(theta, cell, frac, idx) * dFc).sum(), theta)
    return g


def smooth_nodes(theta, act):
    """theta [VZ,VY,VX,3] (differentiable), act bool [VZ,VY,VX] -> v [VZ,VY,VX]: per node the squared differences to its forward
    neighbours x+1, y+1, z+1 with both ends active (differences first, then ((dx dx + dy dy) + dz dz)), added in that order"""
    act = torch.as_tensor(act)
    pad = torch.nn.functional.pad
    v = torch.zeros(act.shape, dtype=theta.dtype)
    for dim, p in ((2, (0, 1)), (1, (0, 0, 0, 1)), (0, (0, 0, 0, 0, 0, 1))):
        n = act.shape[dim] - 1
        d = theta.narrow(dim, 0, n) - theta.narrow(dim, 1, n)
        sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        both = act.narrow(dim, 0, n) & act.narrow(dim, 1, n)
        v = v + pad(torch.where(both, sq, torch.zeros_like(sq)), p)
    return v


def smooth_and_grad(theta, act):
    """-> v [VZ,VY,VX], g [VZ,VY,VX,3] = d (sum of v) / d theta by torch.autograd in the dtype of theta"""
    theta = theta.detach().clone().requires_grad_(True)
    v = smooth_nodes(theta, act)
    g, = torch.autograd.grad(v.sum(), theta)
    return v.detach(), g


def iteration(P0, dt2, origin, cell_size, R, theta, pl, act, M, weight, cells=None):
    """one iteration of section 6n on one sample whose rows all take part, by torch.autograd over this file's field and term and dt_ref's
    lookup, in the dtype of P0; pl = (cell, frac, idx) of `plan` -> loss, (data, smooth), F, d loss / d theta, the two parts of that
    gradient (data, smooth_weight x smooth), the lookup's cells, W"""
    theta = theta.detach().clone().requires_grad_(True)
    F = sample(theta, *pl)
    W = P0 + F
    d, _, cells, _ = dr.lookup(W, dt2, origin, cell_size, R, cells)
    data = d.sum() / max(P0.shape[0], 1)
    smooth = smooth_nodes(theta, act).sum() / max(M, 1)
    loss = data + weight * smooth
    g_data, = torch.autograd.grad(data, theta, retain_graph=True)
    g_smooth, = torch.autograd.grad(weight * smooth, theta, allow_unused=True)
    g_smooth = torch.zeros_like(g_data) if g_smooth is None else g_smooth
    return loss.detach(), (data.detach(), smooth.detach()), F.detach(), g_data + g_smooth, (g_data, g_smooth), cells, W.detach()


def optimize(P0, dt2, origin, cell_size, R, theta, pl, act, M, weight, iters, lr=0.05, patience=100, min_delta=1e-4):
    """the whole loop of section 6n on one sample -> best_flow, best_loss, history"""
    m, v = torch.zeros_like(theta), torch.zeros_like(theta)
    best, best_flow, stalled, hist = math.inf, torch.zeros_like(P0), 0, []
    for t in range(1, iters + 1):
        loss, _, F, dth, _, _, _ = iteration(P0, dt2, origin, cell_size, R, theta, pl, act, M, weight)
        hist.append(float(loss))
        if float(loss) < best - min_delta:
            best, best_flow, stalled = float(loss), F, 0
        else:
            stalled += 1
        if stalled >= patience:
            break
        theta, m, v = nr.adam_step(theta, dth, m, v, t, lr)
    return best_flow, best, hist
