"""Naive float64 restatement of the DBSCAN definition in include/deflow_amd.h / DESIGN.md section 6b: all pairs, connected components by a
breadth-first walk, and the border, filter and numbering rules.  No grid, no union-find: nothing shared with csrc/cluster.hip.

Besides the labels it reports what makes an input well-posed for an exact comparison with the fp32 kernels:
  band_pairs    pairs of participating rows with d^2 inside eps^2 (1 +- 1e-5).  fp32 differences of coordinates below 100 m put the kernel's
                d^2 within a few 1e-7 relative of the float64 value, so a case with no pair in the band has one right set of neighbourhoods
                in both precisions;
  border_ties   border rows whose nearest core row is less than 1e-5 relative closer than a core row of ANOTHER component without the two
                distances being equal in float64 (an exact tie is decided by the row index in both precisions).
Comparison cases assert that both are 0: conditions on the input, not tolerances on the result."""
import torch

BAND = 1e-5


def dbscan_ref(points, count=None, mask=None, dynamic=None, eps=0.7, min_points=4, min_cluster_size=1, min_dynamic_frac=0.3,
               strict=False, allowed=None):
    """one cloud: points [N,3], count = valid leading rows (default N), mask / dynamic [N] or None.  strict / allowed: the deliberately
    WRONG variants of tests/helpers/grid_cases.py (d2 < eps2; neighbours only where the bool [N,N] ``allowed`` says), never the definition.
    -> dict: labels [N] int64, n_clusters, core [N] bool, root [N] int64 (lowest core row of the row's component, -1 = none, BEFORE the
    filters), border [N] bool, band_pairs, border_ties, exact_pairs (the band pairs with d2 == eps2 exactly)"""
    p = points.detach().double().cpu()
    N = p.shape[0]
    count = N if count is None else int(count)
    part = (torch.arange(N) < count) & torch.isfinite(p).all(-1)
    if mask is not None:
        part &= mask.cpu() != 0
    q = torch.where(part[:, None], p, torch.zeros_like(p))
    d2 = sum((q[:, None, c] - q[None, :, c]) ** 2 for c in range(3))      # differences first, then squares
    both = part[:, None] & part[None, :]
    eps2 = float(eps) ** 2
    near = both & ((d2 < eps2) if strict else (d2 <= eps2))    # N(i): the row itself included
    if allowed is not None:
        near &= torch.as_tensor(allowed, dtype=torch.bool)
    off_diag = ~torch.eye(N, dtype=torch.bool)
    band = both & off_diag & (d2 > eps2 * (1 - BAND)) & (d2 < eps2 * (1 + BAND))
    core = part & (near.sum(1) >= int(min_points))
    link = near & core[:, None] & core[None, :]
    root = torch.full((N,), -1, dtype=torch.int64)
    for i in torch.nonzero(core)[:, 0].tolist():              # ascending: a component is named after its lowest core row
        if root[i] >= 0:
            continue
        root[i] = i
        frontier = torch.tensor([i])
        while frontier.numel():
            reach = link[frontier].any(0) & (root < 0)
            root[reach] = i
            frontier = torch.nonzero(reach)[:, 0]
    # border rows: nearest core row within eps, the lowest row on equal distances
    border = torch.zeros(N, dtype=torch.bool)
    ties = 0
    cand = near & core[None, :] & (part & ~core)[:, None]
    dc = torch.where(cand, d2, torch.full_like(d2, float("inf")))
    for i in torch.nonzero(cand.any(1))[:, 0].tolist():
        row = dc[i]
        best = float(row.min())
        j = int(torch.nonzero(row == best)[0, 0])              # lowest index among the equal ones
        border[i] = True
        root[i] = root[j]
        other = row[(root != root[j]) & core]
        if other.numel():
            o = float(other.min())
            if o != best and o - best <= BAND * max(best, 1e-30):
                ties += 1
    # filters, then numbering in ascending order of the lowest core row
    labels = torch.zeros(N, dtype=torch.int64)
    k = 0
    for r in torch.unique(root[root >= 0]).tolist():           # sorted ascending
        members = root == r
        m = int(members.sum())
        if m < int(min_cluster_size):
            continue
        if dynamic is not None:
            flagged = int((members & (dynamic.cpu() != 0)).sum())
            if flagged < float(min_dynamic_frac) * m:          # float64, as the definition states
                continue
        k += 1
        labels[members] = k
    return {"labels": labels, "n_clusters": k, "core": core, "root": root, "border": border, "band_pairs": int(band.sum()) // 2,
            "border_ties": ties, "exact_pairs": int((band & (d2 == eps2)).sum()) // 2}    # (exact_pairs: the band pairs AT eps2)


def dbscan_ref_padded(points, count, mask=None, dynamic=None, **kw):
    """padded batch [B,N,3] with count [B]: -> labels [B,N] int64, n_clusters [B] int64, and the summed well-posedness counts plus the
    per-sample dicts"""
    B = points.shape[0]
    out = [dbscan_ref(points[b], int(count[b]), None if mask is None else mask[b], None if dynamic is None else dynamic[b], **kw)
           for b in range(B)]
    return (torch.stack([o["labels"] for o in out]), torch.tensor([o["n_clusters"] for o in out], dtype=torch.int64),
            {"band_pairs": sum(o["band_pairs"] for o in out), "border_ties": sum(o["border_ties"] for o in out), "samples": out})


def blob_scatter(n_blob=3000, n_scatter=1500, seed=0, extent=51.0, blobs=60):
    """the comparison cloud: `blobs` Gaussian blobs (sigma 0.5 / 0.5 / 0.3 m) of n_blob points in all plus n_scatter points spread
    uniformly over +-extent, shuffled; fp32"""
    g = torch.Generator().manual_seed(seed)
    centres = (torch.rand(blobs, 3, generator=g) * 2 - 1) * torch.tensor([extent - 3, extent - 3, 1.5])
    which = torch.randint(0, blobs, (n_blob,), generator=g)
    pts = centres[which] + torch.randn(n_blob, 3, generator=g) * torch.tensor([0.5, 0.5, 0.3])
    sc = (torch.rand(n_scatter, 3, generator=g) * 2 - 1) * torch.tensor([extent, extent, 2.0])
    allp = torch.cat([pts, sc]).float()
    return allp[torch.randperm(allp.shape[0], generator=g)].contiguous()
