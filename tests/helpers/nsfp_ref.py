"""A naive torch restatement of DESIGN.md section 6k (model=nsfp) that shares nothing with csrc/mlp.hip: the MLP and its gradients written
out by hand, the all-pairs truncated chamfer distance, one iteration of the optimisation, and Adam -- all in the dtype they are given.

The parameter layout is restated here too (not imported): W_in[128][3], b_in, per hidden layer W_l[out][in], b_l, W_out[3][128], b_out."""
import math

import numpy as np
import torch

H = 128


def num_params(depth):
    return (H * 3 + H) + depth * (H * H + H) + (3 * H + 3)


def unpack(flat, depth):
    """flat [>= P] -> list of (W, b) per layer: input, hidden 1..depth, output"""
    out, o = [], 0
    for rows, cols in [(H, 3)] + [(H, H)] * depth + [(3, H)]:
        W = flat[o:o + rows * cols].reshape(rows, cols)
        o += rows * cols
        out.append((W, flat[o:o + rows]))
        o += rows
    assert o == num_params(depth)
    return out


def pack(layers, stride=None):
    flat = torch.cat([torch.cat([W.reshape(-1), b.reshape(-1)]) for W, b in layers])
    if stride is not None and stride > flat.numel():
        flat = torch.cat([flat, flat.new_zeros(stride - flat.numel())])
    return flat


def mlp_forward(x, flat, depth):
    """x [n,3] -> y [n,3], pre-activations z_0..z_depth, activations a_0..a_depth"""
    layers = unpack(flat, depth)
    zs, acts, a = [], [], x
    for W, b in layers[:-1]:
        z = a @ W.T + b
        a = torch.where(z > 0, z, torch.zeros_like(z))
        zs.append(z)
        acts.append(a)
    W, b = layers[-1]
    return a @ W.T + b, zs, acts


def mlp_backward(x, flat, depth, dy, masks):
    """hand-written backward with the given ReLU masks (list of bool [n,128] per layer 0..depth) -> dflat [P], dx [n,3]"""
    layers = unpack(flat, depth)
    a = x
    acts = [x]
    for (W, b), m in zip(layers[:-1], masks):
        z = a @ W.T + b
        a = torch.where(m, z, torch.zeros_like(z))
        acts.append(a)
    grads = [None] * len(layers)
    W, b = layers[-1]
    grads[-1] = (dy.T @ acts[-1], dy.sum(0))
    da = dy @ W
    for l in range(depth, -1, -1):
        dz = torch.where(masks[l], da, torch.zeros_like(da))
        grads[l] = (dz.T @ acts[l], dz.sum(0))
        da = dz @ layers[l][0]
    return pack(grads), da


def nn_all_pairs(A, Bc, trunc_d2):
    """squared nearest-neighbour distance of every row of A to Bc (differences formed first, then squared), the row (lowest index on
    ties), and the well-posedness figures: min gap best / second best, min |d2 - trunc_d2|"""
    if A.shape[0] == 0 or Bc.shape[0] == 0:
        return A.new_full((A.shape[0],), math.inf), torch.full((A.shape[0],), -1, dtype=torch.int64), math.inf, math.inf
    d = ((A[:, None, :] - Bc[None, :, :]) ** 2).sum(-1)
    s, _ = torch.sort(d, dim=1)
    d2, idx = d.min(dim=1)
    gap = float((s[:, 1] - s[:, 0]).min()) if Bc.shape[0] > 1 else math.inf
    edge = float((d2 - trunc_d2).abs().min())
    return d2, idx, gap, edge


def tc_with_idx(A, Bc, idx_ab, idx_ba, trunc_d2):
    """the truncated two-way chamfer term with GIVEN neighbour rows (-1: the row is left out), differentiable in A and Bc"""
    def half(Q, R, idx):
        keep = idx >= 0
        d2 = ((Q - R[idx.clamp_min(0)]) ** 2).sum(-1)
        return torch.where(keep, d2, torch.zeros_like(d2)).sum() / keep.sum().clamp_min(1)
    return half(A, Bc, idx_ab) + half(Bc, A, idx_ba)


def tc(A, Bc, trunc_d2, report=None):
    """tc(A, Bc) of section 6k by all pairs; report (a dict) collects the well-posedness figures"""
    da, ia, g1, e1 = nn_all_pairs(A.detach(), Bc.detach(), trunc_d2)
    db, ib, g2, e2 = nn_all_pairs(Bc.detach(), A.detach(), trunc_d2)
    ia = torch.where(da <= trunc_d2, ia, torch.full_like(ia, -1))
    ib = torch.where(db <= trunc_d2, ib, torch.full_like(ib, -1))
    if report is not None:
        report["min_gap"] = min(report.get("min_gap", math.inf), g1, g2)
        report["min_trunc_edge"] = min(report.get("min_trunc_edge", math.inf), e1, e2)
    return tc_with_idx(A, Bc, ia, ib, trunc_d2), (ia, ib)


def iteration(P0, P1, f_flat, g_flat, depth, trunc_d2, nn=None, report=None):
    """one iteration's loss, F and the gradients of both nets, by torch.autograd over this file's forward.  nn: the four index vectors
    (W->P1, P1->W, C->P0, P0->C) to use instead of the all-pairs search."""
    f_flat = f_flat.detach().clone().requires_grad_(True)
    g_flat = g_flat.detach().clone().requires_grad_(True)
    F, zf, _ = mlp_forward(P0, f_flat, depth)
    W = P0 + F
    G, zg, _ = mlp_forward(W, g_flat, depth)
    C = W - G
    if nn is None:
        L1, (i_w1, i_1w) = tc(W, P1, trunc_d2, report)
        L2, (i_c0, i_0c) = tc(C, P0, trunc_d2, report)
    else:
        i_w1, i_1w, i_c0, i_0c = nn
        L1, L2 = tc_with_idx(W, P1, i_w1, i_1w, trunc_d2), tc_with_idx(C, P0, i_c0, i_0c, trunc_d2)
    loss = L1 + L2
    df, dg = torch.autograd.grad(loss, (f_flat, g_flat))
    if report is not None:
        report["z"] = [z.detach() for z in zf + zg]
    return loss.detach(), F.detach(), df, dg, (i_w1, i_1w, i_c0, i_0c)


def small_preactivations(zs, bound):
    return int(sum(int((z.abs() < bound).sum()) for z in zs))


def adam_step(p, g, m, v, t, lr=8e-3, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update (no amsgrad, no weight decay), step number t >= 1, in the dtype of p"""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    mh = m / (1 - b1 ** t)
    vh = v / (1 - b2 ** t)
    return p - lr * mh / (vh.sqrt() + eps), m, v


def optimize(P0, P1, f_flat, g_flat, depth, iters, trunc_d2=4.0, lr=8e-3, patience=100, min_delta=1e-4):
    """the whole loop of section 6k on one sample -> best_flow, best_loss, history"""
    mf, vf, mg, vg = (torch.zeros_like(f_flat) for _ in range(4))
    best, best_flow, stalled, hist = math.inf, torch.zeros_like(P0), 0, []
    for t in range(1, iters + 1):
        loss, F, df, dg, _ = iteration(P0, P1, f_flat, g_flat, depth, trunc_d2)
        hist.append(float(loss))
        if float(loss) < best - min_delta:
            best, best_flow, stalled = float(loss), F, 0
        else:
            stalled += 1
        if stalled >= patience:
            break
        f_flat, mf, vf = adam_step(f_flat, df, mf, vf, t, lr)
        g_flat, mg, vg = adam_step(g_flat, dg, mg, vg, t, lr)
    return best_flow, best, hist


def replay(history, patience, min_delta):
    """best_loss, stalled, frozen, argmin of ONE sample from its fp32 loss history, in fp32 arithmetic as the device does it"""
    best, stalled, frozen, arg = np.float32(np.inf), 0, False, -1
    for t, l in enumerate(np.asarray(history, dtype=np.float32)):
        if frozen:
            break
        if l < np.float32(best - np.float32(min_delta)):
            best, stalled, arg = l, 0, t
        else:
            stalled += 1
        frozen = stalled >= patience
    return best, stalled, frozen, arg


def xavier_params(depth, gen, dtype=torch.float32, scale=1.0, bias=0.0):
    """one net: weights U(-a, a), a = scale * sqrt(6 / (fan_in + fan_out)); biases U(-bias, bias)"""
    layers = []
    for rows, cols in [(H, 3)] + [(H, H)] * depth + [(3, H)]:
        a = scale * math.sqrt(6.0 / (rows + cols))
        W = (torch.rand(rows, cols, generator=gen, dtype=torch.float64) * 2 - 1) * a
        b = (torch.rand(rows, generator=gen, dtype=torch.float64) * 2 - 1) * bias
        layers.append((W, b))
    return pack(layers).to(dtype)


def planted_blobs(seed, blobs=4, per_blob=60, shift=0.6, spacing=8.0, size=(2.0, 1.0, 0.8)):
    """a few rigid blobs; the second sweep independently re-sampled from the same shapes and moved by under 1 m -> P0, P1, true flow of P0"""
    rng = np.random.default_rng(seed)
    P0, P1, flow = [], [], []
    for k in range(blobs):
        centre = np.array([spacing * (k - 0.5 * (blobs - 1)), 0.75 * spacing * (((k * 7) % 3) - 1), 0.5])
        t = np.array([shift * math.cos(1.3 * k + seed), shift * math.sin(1.3 * k + seed), 0.0])
        a = centre + (rng.random((per_blob, 3)) - 0.5) * np.array(size)
        b = centre + (rng.random((per_blob, 3)) - 0.5) * np.array(size) + t
        P0.append(a), P1.append(b), flow.append(np.broadcast_to(t, a.shape))
    return (np.concatenate(P0).astype(np.float32), np.concatenate(P1).astype(np.float32), np.concatenate(flow).astype(np.float32))


def wellposed(P0, P1, f_flat, g_flat, depth, trunc_d2):
    """the well-posedness of one iteration's case: min gap between the best and second-best d2, min |d2 - trunc_d2| (both over the four
    searches, in float64), and the number of pre-activations whose |z| (float64) is below the forward bound of their layer,
    max(1e-4 max |z|, 4 x the fp32 helper's difference from float64)"""
    r64, r32 = {}, {}
    iteration(P0.double(), P1.double(), f_flat.double(), g_flat.double(), depth, trunc_d2, report=r64)
    iteration(P0.float(), P1.float(), f_flat.float(), g_flat.float(), depth, trunc_d2, report=r32)
    small = 0
    for z64, z32 in zip(r64["z"], r32["z"]):
        bound = max(1e-4 * float(z64.abs().max()), 4 * float((z32.double() - z64).abs().max()))
        small += int((z64.abs() < bound).sum())
    return {"min_gap": r64["min_gap"], "min_trunc_edge": r64["min_trunc_edge"], "small_z": small}


def decided_params(depth, gen, x_scale=30.0):
    """one net whose ReLUs are decided far from 0 on coordinates of up to x_scale metres: small weights, biases of +-(0.7 .. 1.0)"""
    layers = []
    for rows, cols in [(H, 3)] + [(H, H)] * depth + [(3, H)]:
        a = 0.1 * math.sqrt(6.0 / (rows + cols)) if cols == H else 0.1 / x_scale
        W = (torch.rand(rows, cols, generator=gen, dtype=torch.float64) * 2 - 1) * a
        if rows == 3:
            W, b = W * 3, torch.zeros(3, dtype=torch.float64)
        else:
            sign = torch.where(torch.rand(rows, generator=gen) < 0.7, 1.0, -1.0).double()
            b = sign * (0.7 + 0.3 * torch.rand(rows, generator=gen, dtype=torch.float64))
        layers.append((W, b))
    return pack(layers)
