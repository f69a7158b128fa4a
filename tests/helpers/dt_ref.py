"""A naive torch restatement of DESIGN.md section 6l (model=fastnsf) that shares nothing with csrc/dt.hip: the occupancy rule, the
truncated squared distance transform by brute force (and through scipy's exact EDT for grids too large for that; test_fastnsf_cpu.py
holds the two against each other), the trilinear lookup with its analytic gradient, one iteration through torch.autograd on nsfp_ref's
MLP, Adam, the whole loop, and each row's distance to the nearest plane where the lookup's cell changes.

The grid is restated here too (not imported): R = round(trunc / cell), G_a = ceil((max_a - min_a) / cell) + 2 R, origin = min - R cell;
origin and cell are the values fp32 holds."""
import math

import numpy as np
import torch

from helpers import nsfp_ref as nr


def f32(v):
    return float(np.float32(v))


def grid(grid_range, cell, trunc):
    """-> origin (3 floats as fp32 holds them), dims (GX, GY, GZ), R"""
    R = int(round(trunc / cell))
    assert 1 <= R <= 255 and abs(R * cell - trunc) <= 1e-6 * trunc
    dims = tuple(int(math.ceil((grid_range[3 + a] - grid_range[a]) / cell - 1e-6)) + 2 * R for a in range(3))
    return tuple(f32(grid_range[a] - R * cell) for a in range(3)), dims, R


def occupancy(P1, origin, cell, dims):
    """P1 [n,3] float32 -> bool [GZ,GY,GX]: voxel floor((p - o) / cell) per axis in fp32; non-finite rows and rows outside occupy nothing"""
    P1 = torch.as_tensor(P1, dtype=torch.float32)
    occ = torch.zeros(dims[2], dims[1], dims[0], dtype=torch.bool)
    f = torch.floor((P1 - torch.tensor(origin, dtype=torch.float32)) / torch.tensor(cell, dtype=torch.float32))
    ok = torch.isfinite(P1).all(dim=1)
    for a in range(3):
        ok &= (f[:, a] >= 0) & (f[:, a] < dims[a])
    v = f[ok].long()
    occ[v[:, 2], v[:, 1], v[:, 0]] = True
    return occ


def brute_dt2(occ, R):
    """int64 [GZ,GY,GX]: min(R*R, min over occupied v' of |v - v'|^2), every voxel centre against every occupied voxel (small grids)"""
    GZ, GY, GX = occ.shape
    z, y, x = torch.meshgrid(torch.arange(GZ), torch.arange(GY), torch.arange(GX), indexing="ij")
    vox = torch.stack([z, y, x], dim=-1).reshape(-1, 3)
    src = vox[occ.reshape(-1)]
    out = torch.full((vox.shape[0],), R * R, dtype=torch.int64)
    if src.shape[0]:
        step = max(1, (1 << 24) // src.shape[0])
        for s in range(0, vox.shape[0], step):
            d = ((vox[s:s + step, None, :] - src[None, :, :]) ** 2).sum(-1).min(dim=1).values
            out[s:s + step] = torch.minimum(d, out[s:s + step])
    return out.reshape(GZ, GY, GX)


def edt_dt2(occ, R):
    """the same through scipy's exact Euclidean distance transform (squared distances between voxel centres are integers)"""
    from scipy import ndimage
    if not bool(occ.any()):
        return torch.full(occ.shape, R * R, dtype=torch.int64)
    d = ndimage.distance_transform_edt(~occ.numpy())
    return torch.from_numpy(np.minimum(np.rint(d * d), R * R).astype(np.int64))


def lookup(q, dt2, origin, cell, R, cells=None):
    """q [n,3] in the dtype to compute in, dt2 integer [GZ,GY,GX] -> d [n], g [n,3] (analytic), cells [n,3] int64 (ix, iy, iz), clamped
    [n,3] bool.  cells GIVEN: the interpolant of that cell is evaluated at the (clamped) query even if t leaves [0, 1] slightly.
    Non-finite rows: d = R cell, g = 0.  Differentiable in q through torch.autograd as well (d only)."""
    dt = q.dtype
    GZ, GY, GX = dt2.shape
    G = torch.tensor([GX, GY, GZ], dtype=dt)
    c = torch.tensor(cell, dtype=dt)
    fin = torch.isfinite(q).all(dim=1)
    qq = torch.where(fin[:, None], q, torch.zeros_like(q))
    u_raw = (qq - torch.tensor(origin, dtype=dt)) / c - 0.5
    clamped = (u_raw < 0) | (u_raw > G - 1)
    u = torch.minimum(torch.maximum(u_raw, torch.zeros_like(u_raw)), (G - 1).expand_as(u_raw))
    if cells is None:
        cells = torch.minimum(torch.floor(u.detach()), (G - 2).expand_as(u)).long()
    t = u - cells.to(dt)
    V = c * torch.sqrt(dt2.to(dt))
    ix, iy, iz = cells[:, 0], cells[:, 1], cells[:, 2]
    v = {(a, b, e): V[iz + e, iy + b, ix + a] for a in (0, 1) for b in (0, 1) for e in (0, 1)}
    tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
    ex = {(b, e): v[0, b, e] * (1 - tx) + v[1, b, e] * tx for b in (0, 1) for e in (0, 1)}
    fy = {e: ex[0, e] * (1 - ty) + ex[1, e] * ty for e in (0, 1)}
    d = fy[0] * (1 - tz) + fy[1] * tz
    gx = sum((v[1, b, e] - v[0, b, e]) * (ty if b else 1 - ty) * (tz if e else 1 - tz) for b in (0, 1) for e in (0, 1))
    gy = sum((ex[1, e] - ex[0, e]) * (tz if e else 1 - tz) for e in (0, 1))
    gz = fy[1] - fy[0]
    g = torch.stack([gx, gy, gz], dim=1) / c
    g = torch.where(clamped | ~fin[:, None], torch.zeros_like(g), g)
    d = torch.where(fin, d, (R * c).expand_as(d))
    return d, g.detach(), cells, clamped


def plane_distance(q, origin, cell, dims):
    """per row, in voxels: the distance of u = (q - o) / cell - 0.5 (float64) to the nearest plane where the cell index changes or the
    clamp begins (the integers 0 .. G - 1 of every axis), minimised over the axes"""
    u = (q.double() - torch.tensor(origin, dtype=torch.float64)) / cell - 0.5
    G = torch.tensor(dims, dtype=torch.float64)
    inside = (u >= 0) & (u <= G - 1)
    dist = torch.where(inside, (u - torch.round(u)).abs(), torch.maximum(-u, u - (G - 1)))
    return dist.min(dim=1).values


def iteration(P0, dt2, origin, cell, R, f_flat, depth, cells=None):
    """one iteration on one sample, by torch.autograd over nsfp_ref's forward and this file's lookup, in the dtype of P0 ->
    loss, F, d loss / d f, the lookup's cells, W"""
    f_flat = f_flat.detach().clone().requires_grad_(True)
    F = nr.mlp_forward(P0, f_flat, depth)[0]
    W = P0 + F
    d, _, cells, _ = lookup(W, dt2, origin, cell, R, cells)
    loss = d.sum() / max(P0.shape[0], 1)
    df, = torch.autograd.grad(loss, f_flat)
    return loss.detach(), F.detach(), df, cells, W.detach()


def optimize(P0, dt2, origin, cell, R, f_flat, depth, iters, lr=8e-3, patience=100, min_delta=1e-4):
    """the whole loop of section 6l on one sample -> best_flow, best_loss, history"""
    m, v = torch.zeros_like(f_flat), torch.zeros_like(f_flat)
    best, best_flow, stalled, hist = math.inf, torch.zeros_like(P0), 0, []
    for t in range(1, iters + 1):
        loss, F, df, _, _ = iteration(P0, dt2, origin, cell, R, f_flat, depth)
        hist.append(float(loss))
        if float(loss) < best - min_delta:
            best, best_flow, stalled = float(loss), F, 0
        else:
            stalled += 1
        if stalled >= patience:
            break
        f_flat, m, v = nr.adam_step(f_flat, df, m, v, t, lr)
    return best_flow, best, hist
