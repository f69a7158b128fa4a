"""The naive restatement of the chamfer nearest-neighbour op and of seflowLoss that the tests compare the engine with: per sample,
boolean masks, a Python loop over torch.unique(labels), an all-pairs chunked search.  Written independently of
deflow_amd.losses.seflow_loss and deflow_amd/csrc/chamfer.hip; runs in whatever dtype its inputs have (fp32 and float64 in the tests).

UNPINNED, like the engine's side: upstream's chamfer3D extension and src/lossfuncs.py::seflowLoss are in the absent submodule; this is
the recalled form (SeFlow, ECCV'24, Eq. 6-11)."""
import math

import torch

INF = float("inf")


def nn_all_pairs(q: torch.Tensor, r: torch.Tensor, chunk: int = 0, second: bool = False):
    """q [n,3], r [m,3] (all rows take part) -> d2 [n] smallest squared distance (differences first, then squares), idx [n] int64 the
    lowest row of r at that distance; (+inf, -1) when m == 0.  second=True: also the second-smallest distance (+inf when m < 2)."""
    n, m = q.shape[0], r.shape[0]
    d2 = torch.full((n,), INF, dtype=q.dtype, device=q.device)
    idx = torch.full((n,), -1, dtype=torch.long, device=q.device)
    d2nd = torch.full((n,), INF, dtype=q.dtype, device=q.device)
    if m == 0 or n == 0:
        return (d2, idx, d2nd) if second else (d2, idx)
    chunk = chunk or max(16, (1 << 23) // m)          # ~8 M pairs at a time
    for s in range(0, n, chunk):
        diff = q[s:s + chunk, None, :] - r[None, :, :]
        d = (diff * diff).sum(-1)                                   # [c, m]
        best = d.min(1).values
        # lowest index among the rows at the smallest distance
        first = torch.where(d == best[:, None], torch.arange(m, device=q.device)[None, :], m).min(1).values
        d2[s:s + chunk], idx[s:s + chunk] = best, first
        if second and m >= 2:
            d2nd[s:s + chunk] = d.scatter(1, first[:, None], INF).min(1).values
    return (d2, idx, d2nd) if second else (d2, idx)


def nn_padded(query, qcount, ref, rcount, qlabel=None, rlabel=None, max_dist2=INF, second=False):
    """the engine's chamfer_nn contract on padded batches, by all pairs: rows take part if they are valid leading rows, finite and
    (when labels are given) have label > 0; a neighbour farther than max_dist2 is no neighbour.  -> d2 [B,Nq], idx [B,Nq] int32"""
    B, Nq, _ = query.shape
    d2 = torch.full((B, Nq), INF, dtype=query.dtype, device=query.device)
    idx = torch.full((B, Nq), -1, dtype=torch.int32, device=query.device)
    d2nd = torch.full((B, Nq), INF, dtype=query.dtype, device=query.device)
    for b in range(B):
        qm = torch.zeros(Nq, dtype=torch.bool, device=query.device)
        qm[: int(qcount[b])] = True
        qm &= torch.isfinite(query[b]).all(-1)
        rm = torch.zeros(ref.shape[1], dtype=torch.bool, device=query.device)
        rm[: int(rcount[b])] = True
        rm &= torch.isfinite(ref[b]).all(-1)
        if qlabel is not None:
            qm &= qlabel[b] > 0
        if rlabel is not None:
            rm &= rlabel[b] > 0
        rows = torch.nonzero(rm)[:, 0]
        out = nn_all_pairs(query[b][qm], ref[b][rm], second=second)
        d, i = out[0], out[1]
        keep = d <= max_dist2
        d2[b, qm] = torch.where(keep, d, torch.full_like(d, INF))
        idx[b, qm] = torch.where(keep & (i >= 0), rows[i.clamp_min(0)] if rows.numel() else i, torch.full_like(i, -1)).to(torch.int32)
        if second:
            d2nd[b, qm] = out[2]
    return (d2, idx, d2nd) if second else (d2, idx)


def _tmean(d, T):
    keep = d <= T
    return d[keep].mean() if bool(keep.any()) else d.new_zeros(())


def _chamfer(a, b, T):
    """tmean of the squared distances a -> b plus b -> a, differentiable through the gathered neighbours"""
    if a.shape[0] == 0 or b.shape[0] == 0:
        return a.new_zeros(())
    with torch.no_grad():
        _, ia = nn_all_pairs(a, b)
        _, ib = nn_all_pairs(b, a)
    da = ((a - b[ia]) ** 2).sum(-1)
    db = ((b - a[ib]) ** 2).sum(-1)
    return _tmean(da, T) + _tmean(db, T)


def _norm(v):
    """|v| per row with a zero gradient at v = 0"""
    sq = (v * v).sum(-1)
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def seflow_ref(pc0, pc1, flow, counts0, counts1, lab0, lab1, weights=(1.0, 1.0, 1.0, 1.0), min_dynamic=256, truncate_dist=4.0,
               report=None):
    """-> loss, terms [B,4] (rows: chamfer_dis, dynamic_chamfer_dis, static_flow_loss, cluster_flow_loss).  report (a dict): collects
    what a test needs to judge whether the inputs are well-posed -- the kept / dropped distances nearest to the truncation threshold
    and, per cluster, the relative gap between its two largest eligible raw distances."""
    B = pc0.shape[0]
    T = truncate_dist
    terms = []
    trunc_gap, cluster_gap = INF, INF
    for b in range(B):
        n0, n1 = int(counts0[b]), int(counts1[b])
        a, c, f = pc0[b, :n0], pc1[b, :n1], flow[b, :n0]
        la, lc = lab0[b, :n0], lab1[b, :n1]
        p = a + f
        t0 = _chamfer(p, c, T)
        da, dc = la > 0, lc > 0
        has_dyn = int(da.sum()) > min_dynamic and int(dc.sum()) > min_dynamic
        t1 = _chamfer(p[da], c[dc], T) if has_dyn else p.new_zeros(())
        st = la == 0
        t2 = _norm(f[st]).mean() if bool(st.any()) else p.new_zeros(())
        t3 = p.new_zeros(())
        if report is not None and n0 and n1:
            with torch.no_grad():
                pairs = [(p, c), (c, p)] + ([(p[da], c[dc]), (c[dc], p[da])] if has_dyn else [])
                for x, y in pairs:
                    d, _ = nn_all_pairs(x, y)
                    if d.numel():
                        trunc_gap = min(trunc_gap, float((d - T).abs().min()))
        if has_dyn:
            with torch.no_grad():
                rd, ri = nn_all_pairs(a, c)
            errs = []
            for lab in torch.unique(la).tolist():
                if lab <= 0:
                    continue
                rows = torch.nonzero((la == lab) & dc[ri])[:, 0]          # rows of the cluster whose neighbour is dynamic too
                if rows.numel() == 0:
                    continue
                d = rd[rows]
                top = d.max()
                m = rows[torch.nonzero(d == top)[0, 0]]                   # lowest row at the largest distance
                if report is not None and rows.numel() > 1:
                    two = torch.sort(d, descending=True).values[:2]
                    cluster_gap = min(cluster_gap, float((two[0] - two[1]) / two[0].clamp_min(1e-300)))
                target = (c[ri[m]] - a[m]).detach()
                errs.append(_norm(f[la == lab] - target))
            if errs:
                t3 = torch.cat(errs).mean()
            else:
                with torch.no_grad():
                    t3 = _tmean(rd, T) + _tmean(nn_all_pairs(c, a)[0], T)
                if report is not None:
                    for d in (rd, nn_all_pairs(c, a)[0]):
                        trunc_gap = min(trunc_gap, float((d - T).abs().min()))
        terms.append(torch.stack([t0, t1, t2, t3]))
    terms = torch.stack(terms)
    if report is not None:
        report["trunc_gap"] = min(report.get("trunc_gap", INF), trunc_gap)
        report["cluster_gap"] = min(report.get("cluster_gap", INF), cluster_gap)
    w = torch.as_tensor(weights, dtype=terms.dtype, device=terms.device)
    return (terms * w).sum(), terms


def brute_nn_fn(query, qcount, ref, rcount, qlabel=None, rlabel=None, max_dist2=math.inf):
    """nn_fn for deflow_amd.losses.seflow_loss on CPU tensors: the padded all-pairs search above"""
    return nn_padded(query, qcount, ref, rcount, qlabel, rlabel, max_dist2)
