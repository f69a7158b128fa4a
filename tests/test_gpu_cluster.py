"""GPU: the DBSCAN op (csrc/cluster.hip, deflow_amd/cluster.py) against the naive float64 restatement in tests/helpers/dbscan_ref.py, and
the Trainer's online cluster labels.  Labels and counts are integers: every comparison with the helper is exact equality.  Each
comparison case first asserts that its INPUT is well-posed (no pair within 1e-5 relative of eps^2, no border row nearly equidistant from two
clusters; see the helper) -- a condition on the input, not a tolerance on the result."""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from dbscan_ref import blob_scatter, dbscan_ref_padded  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], grid_feature_size=[64, 64])
EPS = 0.7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def check(name, dev, points, count, mask=None, dynamic=None, grid_range=None, **kw):
    """the op on `dev` against the helper on the same fp32 inputs: the input is well-posed, labels and n_clusters are equal, a second call
    is bit-identical, the status word is 0"""
    from deflow_amd.cluster import dbscan, dynamic_cluster_labels
    want, wantk, rep = dbscan_ref_padded(points, count, mask, dynamic, **kw)
    assert rep["band_pairs"] == 0 and rep["border_ties"] == 0, f"{name}: ill-posed input {rep['band_pairs']} / {rep['border_ties']}"
    p, c = points.to(dev), i32(list(count), dev)
    m = None if mask is None else mask.to(dev)
    gk = {} if grid_range is None else {"grid_range": grid_range}

    def run():
        if dynamic is not None:
            assert mask is None
            return dynamic_cluster_labels(p, c, dynamic.to(dev), **kw, **gk)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lab, k = dbscan(p, c, m, status=status, **kw, **gk)
        return lab, k, status

    lab, k, status = run()
    lab2, k2, _ = run()
    assert lab.dtype == torch.int32 and k.dtype == torch.int32 and lab.shape == points.shape[:2] and k.shape == (points.shape[0],)
    assert torch.equal(lab, lab2) and torch.equal(k, k2), f"{name}: a repeated call differs"
    n_border = sum(int(s["border"].sum()) for s in rep["samples"])
    n_core = sum(int(s["core"].sum()) for s in rep["samples"])
    print(f"[cluster] {name}: clusters {wantk.tolist()} (op {k.tolist()}), {n_core} core rows, {n_border} border rows, "
          f"{int((lab.cpu().long() != want).sum())} rows differ, status {int(status)}")
    assert int(status) == 0, f"{name}: a bounded loop hit its bound"
    assert torch.equal(k.cpu().long(), wantk), f"{name}: n_clusters {k.tolist()} vs {wantk.tolist()}"
    assert torch.equal(lab.cpu().long(), want), f"{name}: {int((lab.cpu().long() != want).sum())} labels differ"
    return lab, k, rep


def batch_case():
    """B = 3: different counts, NaN / inf rows inside the counted part, a mask, one empty sample"""
    a, b = blob_scatter(seed=1), blob_scatter(seed=3)
    pts = torch.stack([a, b, blob_scatter(seed=5)])
    pts[1, 100:140] = float("nan")
    pts[1, 200, 1] = float("inf")
    pts[0, 7, 2] = float("-inf")
    count = [4500, 3100, 0]
    g = torch.Generator().manual_seed(17)
    mask = torch.randint(1, 4, (3, 4500), generator=g)
    mask[torch.rand(3, 4500, generator=g) < 0.05] = -1         # non-zero: takes part
    mask[torch.rand(3, 4500, generator=g) < 0.12] = 0
    return pts, count, mask


def test_batch_counts_nan_rows_mask_and_an_empty_sample(dev):
    pts, count, mask = batch_case()
    lab, k, rep = check("batch, no mask", dev, pts, count, eps=EPS, min_points=4)
    assert int(k[2]) == 0 and bool((lab[2] == 0).all()) and int(k[0]) > 20 and int(k[1]) > 10
    bad = ~torch.isfinite(pts).all(-1)
    assert bool((lab.cpu()[bad] == 0).all()) and bool((lab[1, 3100:] == 0).all())
    lab_m, _, _ = check("batch, mask", dev, pts, count, mask=mask, eps=EPS, min_points=4)
    assert bool((lab_m.cpu()[mask == 0] == 0).all())
    check("batch, mask, min_cluster_size 20", dev, pts, count, mask=mask, eps=EPS, min_points=4, min_cluster_size=20)
    check("batch, bool mask, min_points 6, eps 0.5", dev, pts, count, mask=mask != 0, eps=0.5, min_points=6)
    check("B = 1", dev, pts[:1].contiguous(), count[:1], eps=EPS, min_points=4)


def outside_case():
    """a cloud whose clusters straddle and lie beyond the grid range on several sides -- pairs of neighbours that are BOTH outside included"""
    base = blob_scatter(n_blob=1500, n_scatter=300, seed=2, extent=12.0, blobs=25)
    far = []
    g = torch.Generator().manual_seed(23)
    for cx, cy in ((14.0, 0.0), (-13.0, -15.0), (0.5, 19.0), (30.0, 30.0), (-40.0, 2.0), (9.9, -10.1), (-10.0, 10.0)):
        far.append(torch.tensor([cx, cy, 0.0]) + torch.randn(40, 3, generator=g) * torch.tensor([0.4, 0.4, 0.2]))
    pts = torch.cat([base] + far)
    return pts[torch.randperm(pts.shape[0], generator=g)].float()[None].contiguous()


def test_rows_outside_the_grid_range(dev):
    pts = outside_case()
    n = [pts.shape[1]]
    rng = (-10.0, -10.0, 10.0, 10.0)
    out = ((pts[0, :, :2].abs() > 10.0).any(-1))
    assert int(out.sum()) > 250
    lab, k, rep = check("outside the range", dev, pts, n, grid_range=rng, eps=EPS, min_points=4)
    assert len(torch.unique(lab.cpu()[0][out])) > 6                # whole clusters out there
    wide, _, _ = check("the same, default range", dev, pts, n, eps=EPS, min_points=4)
    assert torch.equal(lab, wide)                                  # the range decides only the speed
    tiny, _, _ = check("the same, a 2 m range", dev, pts, n, grid_range=(-1.0, -1.0, 1.0, 1.0), eps=EPS, min_points=4)
    assert torch.equal(lab, tiny)


def test_long_chain_in_shuffled_order(dev):
    """4000 rows spaced 0.85 eps along x, min_points = 2, given in shuffled order: one cluster; the union-find sees deep trees and every
    loop stays inside its bound (status 0).  A correctness case with bounded loops, run once."""
    n = 4000
    g = torch.Generator().manual_seed(31)
    x = torch.arange(n, dtype=torch.float64) * (0.85 * EPS) - 0.5 * n * 0.85 * EPS
    pts = torch.stack([x, torch.full_like(x, 0.3), torch.zeros_like(x)], 1).float()
    pts = pts[torch.randperm(n, generator=g)][None].contiguous()
    lab, k, rep = check("chain", dev, pts, [n], eps=EPS, min_points=2)
    assert int(k[0]) == 1 and bool((lab == 1).all())
    lab, k, rep = check("chain, min_points 4", dev, pts, [n], eps=EPS, min_points=4)      # 3 rows within eps: no core row at all
    assert int(k[0]) == 0 and bool((lab == 0).all())


def test_all_rows_identical(dev):
    pts = torch.tensor([[3.25, -7.5, 0.75]]).repeat(2500, 1)[None].contiguous()
    lab, k, _ = check("identical rows", dev, pts, [2500], eps=EPS, min_points=4)
    assert int(k[0]) == 1 and bool((lab == 1).all())
    lab, k, _ = check("identical rows, 3 of them", dev, pts, [3], eps=EPS, min_points=4)
    assert int(k[0]) == 0 and bool((lab == 0).all())


def equidistant_case():
    """two tight groups of four core rows 1.2 m apart and one row exactly between them: its nearest core rows of the two clusters are at the
    same distance bit for bit, and it goes to the cluster of the lower ROW (the right-hand group here, listed first)"""
    right = torch.tensor([[0.6, 0.0, 0.0], [0.9, 0.0, 0.0], [0.9, 0.25, 0.0], [1.1, 0.0, 0.25]])
    left = right * torch.tensor([-1.0, 1.0, 1.0])
    mid = torch.tensor([[0.0, 0.0, 0.0]])
    return torch.cat([right[1:], left[1:], mid, right[:1], left[:1]])[None].contiguous()       # the two nearest: rows 7 (right), 8 (left)


def test_equidistant_border_row(dev):
    pts = equidistant_case()
    lab, k, rep = check("equidistant border row", dev, pts, [9], eps=EPS, min_points=4)
    s = rep["samples"][0]
    assert bool(s["border"][6]) and int(s["border"].sum()) == 1 and int(k[0]) == 2
    assert int(lab[0, 6]) == int(lab[0, 7]) == 1 and int(lab[0, 8]) == 2
    # the mirror image: now the left-hand row is the lower one
    sw = pts.clone()
    sw[0, [7, 8]] = pts[0, [8, 7]]
    lab, k, _ = check("equidistant border row, swapped", dev, sw, [9], eps=EPS, min_points=4)
    assert int(lab[0, 6]) == int(lab[0, 7]) and bool((sw[0, 7, 0] < 0))


def dynamic_case():
    pts = blob_scatter(seed=1)
    g = torch.Generator().manual_seed(41)
    dyn = (pts[:, 0] > 5.0) & (torch.rand(pts.shape[0], generator=g) < 0.6)       # clusters on the left: none flagged; on the right: ~60 %
    dyn |= (pts[:, 0] < -30.0) & (torch.rand(pts.shape[0], generator=g) < 0.15)   # far left: ~15 %, below the 30 %
    return torch.stack([pts, blob_scatter(seed=3)]), [4500, 4000], torch.stack([dyn, torch.zeros_like(dyn)])


def test_dynamic_cluster_labels_with_both_filters_biting(dev):
    pts, count, dyn = dynamic_case()
    kw = dict(eps=EPS, min_points=4)
    _, k_all, _ = check("dynamic: no filter", dev, pts, count, **kw)
    _, k_size, _ = check("dynamic: size filter only", dev, pts, count, dynamic=torch.ones_like(dyn), min_cluster_size=40, min_dynamic_frac=0.3, **kw)
    lab, k, rep = check("dynamic: both filters", dev, pts, count, dynamic=dyn, min_cluster_size=40, min_dynamic_frac=0.3, **kw)
    _, k_frac, _ = check("dynamic: flag filter only", dev, pts, count, dynamic=dyn.long() * 5, min_cluster_size=1, min_dynamic_frac=0.3, **kw)
    print(f"[cluster] clusters: all {k_all.tolist()}, size filter {k_size.tolist()}, flag filter {k_frac.tolist()}, both {k.tolist()}")
    assert int(k_all[0]) > int(k_size[0]) > int(k[0]) > 0 and int(k_all[0]) > int(k_frac[0]) >= int(k[0])
    assert int(k[1]) == 0 and bool((lab[1] == 0).all())                  # nothing flagged in sample 1
    check("dynamic: frac 0 keeps what the size filter keeps", dev, pts, count, dynamic=dyn, min_cluster_size=20, min_dynamic_frac=0.0, **kw)
    check("dynamic: frac 1", dev, pts, count, dynamic=dyn, min_cluster_size=2, min_dynamic_frac=1.0, **kw)


def test_side_stream_beside_other_kernels(dev):
    """a call on a side stream while the default stream runs other library kernels: the same labels"""
    from deflow_amd.chamfer import chamfer_nn
    from deflow_amd.cluster import dbscan
    pts, count, mask = batch_case()
    p, c, m = pts.to(dev), i32(count, dev), mask.to(dev)
    want, wk = dbscan(p, c, m, eps=EPS)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    q = p + 0.1
    for _ in range(6):
        chamfer_nn(q, c, p, c)                         # keeps the default stream busy
    with torch.cuda.stream(side):
        got, gk = dbscan(p, c, m, eps=EPS)
    for _ in range(6):
        chamfer_nn(q, c, p, c)
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(gk, wk)


def test_arguments(dev):
    from deflow_amd.cluster import dbscan, dynamic_cluster_labels
    p = torch.zeros(1, 8, 3, device=dev)
    c = i32([8], dev)
    with pytest.raises(TypeError, match="CUDA"):
        dbscan(p.cpu(), c.cpu())
    with pytest.raises(ValueError):
        dbscan(p, c, eps=0.0)
    with pytest.raises(ValueError):
        dbscan(p, c, min_points=0)
    with pytest.raises(ValueError):
        dbscan(p, c.long())
    with pytest.raises(ValueError):
        dbscan(p, c, torch.zeros(1, 8, device=dev))                      # a float mask
    with pytest.raises(ValueError):
        dynamic_cluster_labels(p, c, torch.zeros(1, 7, dtype=torch.bool, device=dev))
    lab, k, status = dynamic_cluster_labels(p, c, torch.ones(1, 8, dtype=torch.bool, device=dev), min_cluster_size=8)
    assert lab.tolist() == [[1] * 8] and k.tolist() == [1] and int(status) == 0


# ---- the training step ------------------------------------------------------------------------------------------------------------------
N_PTS = 6000
# eps 0.3: the small synthetic clouds hold ~5 200 rows in 12.8 m x 12.8 m -- at 0.7 they are one component
CL = dict(eps=0.3, min_points=4, min_cluster_size=6, min_dynamic_frac=0.2)


def flag_batch(B, seed, dev, n=N_PTS):
    """a synthetic batch with the dynamic FLAG only (tile labels > 0), as train.py's cluster_labels=online builds it"""
    from deflow_amd.synth import synth_batch, synth_cluster_labels
    b = synth_batch(B, n, seed=seed, grid_hw=(64, 64), device=dev)
    l0, l1 = synth_cluster_labels(b)
    b["pc0_dufo"], b["pc1_dufo"] = l0 > 0, l1 > 0
    return b, (l0, l1)


def fresh(dev, seed=78, **kw):
    import deflow_amd
    from deflow_amd.optim import Trainer
    torch.manual_seed(seed)
    m = deflow_amd.DeFlow(**SMALL, num_iters=2).to(dev).train()
    return m, Trainer(m, lr=1e-3, loss_fn="seflowLoss", loss_args=dict(min_dynamic=4), **kw)


def scattered_labels(batch, st):
    """dynamic_cluster_labels on the step's own compact clouds, scattered back to input rows: what a file of labels would hold"""
    from deflow_amd.cluster import dynamic_cluster_labels
    out = []
    rg = SMALL["point_cloud_range"]
    for p, key in ((st["p0"], "pc0_dufo"), (st["p1"], "pc1_dufo")):
        f = batch[key]
        fc = torch.gather(f.long(), 1, p.idx_c.clamp(0, f.shape[1] - 1))
        lab, k, status = dynamic_cluster_labels(p.points_c, p.counts, fc, grid_range=(rg[0], rg[1], rg[3], rg[4]), **CL)
        assert int(status) == 0
        valid = torch.arange(lab.shape[1], device=lab.device)[None, :] < p.counts[:, None]
        full = torch.zeros(f.shape, dtype=torch.int64, device=lab.device)
        b_ix = torch.arange(lab.shape[0], device=lab.device)[:, None].expand_as(lab)
        full[b_ix[valid], p.idx_c[valid]] = lab.long()[valid]
        out.append((full, k))
    return out


def test_trainer_online_labels_equal_supplied_labels(dev):
    """a seflowLoss step with cluster_labels and flags in the batch == a step of an identical trainer whose batch carries the labels
    dynamic_cluster_labels gives for the same compact clouds, scattered back to input rows: loss, terms and parameters bit for bit"""
    m1, t1 = fresh(dev, cluster_labels=CL)
    batch, _ = flag_batch(2, 400, dev)
    loss1 = t1.step(batch)
    assert int(t1.last_cluster_status) == 0 and int(t1.last_label_overflow) == 0
    (lab0, k0), (lab1, k1) = scattered_labels(batch, m1.last_state)
    print(f"[cluster] trainer: clusters per sample pc0 {k0.tolist()} pc1 {k1.tolist()}, labelled rows {int((lab0 > 0).sum())} / {int((lab1 > 0).sum())}, "
          f"terms {t1.last_loss_terms.mean(0).tolist()}")
    assert int(k0.min()) > 0 and int(k1.min()) > 0 and bool((t1.last_loss_terms[:, [0, 2]] > 0).all())
    assert bool((t1.last_loss_terms[:, 1] > 0).any()) and bool((t1.last_loss_terms[:, 3] > 0).any())      # the labels reach terms 1 and 3
    m2, t2 = fresh(dev)
    supplied = {k: v for k, v in batch.items() if k not in ("pc0_dufo", "pc1_dufo")}
    supplied["pc0_dynamic"], supplied["pc1_dynamic"] = lab0, lab1
    loss2 = t2.step(supplied)
    assert t2.last_cluster_status is None
    assert float(loss1) == float(loss2) and torch.equal(t1.last_loss_terms, t2.last_loss_terms)
    assert torch.equal(t1.flat.param, t2.flat.param) and torch.equal(t1.opt.exp_avg_sq, t2.opt.exp_avg_sq)
    # labels in the batch win over flags, and the keyword changes nothing then
    m3, t3 = fresh(dev, cluster_labels=CL)
    both = dict(supplied)
    both["pc0_dufo"], both["pc1_dufo"] = torch.ones_like(batch["pc0_dufo"]), torch.ones_like(batch["pc1_dufo"])
    loss3 = t3.step(both)
    assert float(loss3) == float(loss2) and torch.equal(t3.flat.param, t2.flat.param) and t3.last_cluster_status is None


def test_trainer_without_keyword_or_flags_raises(dev):
    m, t = fresh(dev)
    batch, _ = flag_batch(2, 400, dev)
    with pytest.raises(ValueError, match="pc0_dynamic"):
        t.step(batch)                                  # flags, but the keyword is not set
    m, t = fresh(dev, cluster_labels={})
    del batch["pc1_dufo"]
    with pytest.raises(ValueError, match="pc0_dynamic"):
        t.step(batch)


def test_captured_online_step_equals_eager(dev):
    bs = [flag_batch(2, 420 + i, dev)[0] for i in range(2)]
    seq = [bs[1], bs[0], bs[1]]
    m1, t1 = fresh(dev, cluster_labels=CL)
    want = [(float(t1.step(b)), t1.last_loss_terms.clone()) for b in seq]
    m2, t2 = fresh(dev, cluster_labels=CL)
    t2.capture(bs[0])
    got = []
    for b in seq:
        l = t2.step_captured(b)
        got.append((float(l), t2.last_loss_terms.clone()))
    torch.cuda.synchronize()
    assert [g[0] for g in got] == [w[0] for w in want], (got, want)
    assert all(torch.equal(g[1], w[1]) for g, w in zip(got, want))
    assert torch.equal(t2.flat.param, t1.flat.param) and torch.equal(t2.opt.exp_avg_sq, t1.opt.exp_avg_sq)
    assert int(t2.last_cluster_status) == 0


def test_train_cli_runs_online_labels(dev, capsys):
    import deflow_amd.train as T
    T.main(["model=deflow", "lr=2e-4", "epochs=1", "batch_size=2", "loss_fn=seflowLoss", "cluster_labels=online", "cluster_min_size=10", "cluster_eps=0.3",
            "train_data=synthetic", "model.target.num_iters=2", "voxel_size=[0.2, 0.2, 6]", "point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3]",
            "pairs_per_epoch=6", "points_per_cloud=6000", "log_every=1"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "trainer/loss" in l]
    assert len(steps) == 3
    for l in steps:
        for k in ("chamfer_dis", "dynamic_chamfer_dis", "static_flow_loss", "cluster_flow_loss"):
            assert math.isfinite(l["trainer/" + k]), l
        assert l["trainer/chamfer_dis"] > 0 and l["trainer/static_flow_loss"] > 0
