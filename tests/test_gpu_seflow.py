"""GPU: the chamfer nearest-neighbour op (csrc/chamfer.hip), ChamferDis and the seflowLoss training step against the naive float64
restatement in tests/helpers/seflow_ref.py."""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import parity  # noqa: E402
from seflow_ref import nn_all_pairs, nn_padded, seflow_ref  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], grid_feature_size=[64, 64])
SMALL_RANGE = (-6.4, -6.4, 6.4, 6.4)
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def check_nn(name, query, qcount, ref, rcount, ql=None, rl=None, max_dist2=INF, exact_idx=False, **kw):
    """chamfer_nn against the float64 all-pairs helper on the same fp32 inputs: d2 within 1e-6 relative, +inf / -1 exactly where the
    rule says; idx equal to the helper's wherever its best and second-best distance differ by more than 1e-5 relative, elsewhere a
    participating row at the reported distance -- and at most 1 % of the rows under that exemption"""
    from deflow_amd.chamfer import chamfer_nn
    d2, idx = chamfer_nn(query, qcount, ref, rcount, ql, rl, max_dist2, **kw)
    d2b, idxb = chamfer_nn(query, qcount, ref, rcount, ql, rl, max_dist2, **kw)
    assert torch.equal(d2, d2b) and torch.equal(idx, idxb), f"{name}: a repeated call differs"
    w2, widx, w2nd = nn_padded(query.double(), qcount, ref.double(), rcount, ql, rl, max_dist2, second=True)
    assert d2.shape == w2.shape and idx.shape == widx.shape and idx.dtype == torch.int32
    none = torch.isinf(w2)
    assert torch.equal(torch.isinf(d2), none), f"{name}: +inf rows differ ({int(torch.isinf(d2).sum())} vs {int(none.sum())})"
    assert torch.equal(idx < 0, none) and bool((idx[none] == -1).all()), f"{name}: idx = -1 rows differ"
    hit = ~none
    n_hit = int(hit.sum())
    if n_hit == 0:
        print(f"[seflow] {name}: no neighbour anywhere ({d2.numel()} rows)")
        return d2, idx
    rel = ((d2.double() - w2).abs() / w2.clamp_min(1e-30))[hit]
    rel = torch.where(w2[hit] == 0, d2.double()[hit], rel)          # exact duplicates: 0 must be 0
    clear = hit & ((w2nd - w2) > 1e-5 * w2)
    exempt = hit & ~clear
    share = int(exempt.sum()) / n_hit
    print(f"[seflow] {name}: {n_hit} neighbours of {d2.numel()} rows, max rel d2 error {float(rel.max()):.2e}, "
          f"{int(exempt.sum())} rows with a near-tie ({100 * share:.3f} %)")
    assert float(rel.max()) <= 1e-6, f"{name}: d2 off by {float(rel.max()):.3e} relative"
    assert torch.equal(idx[clear], widx[clear]), f"{name}: {int((idx[clear] != widx[clear]).sum())} wrong neighbours"
    if not exact_idx:
        assert share <= 0.01, f"{name}: {100 * share:.2f} % of the rows are near-ties"
    # near-ties: whatever row is named must take part and lie at the reported distance
    B, Nr = ref.shape[0], ref.shape[1]
    part = (torch.arange(Nr, device=ref.device)[None, :] < rcount[:, None]) & torch.isfinite(ref).all(-1)
    if rl is not None:
        part &= rl > 0
    j = idx.clamp_min(0).long()
    named = torch.gather(ref.double(), 1, j[..., None].expand(-1, -1, 3))
    dn = ((query.double() - named) ** 2).sum(-1)
    assert bool(torch.gather(part, 1, j)[exempt].all()), f"{name}: a named row does not take part"
    assert bool(((dn - d2.double()).abs() <= 1e-6 * dn)[exempt].all()), f"{name}: a named row is not at the reported distance"
    if exact_idx:
        assert torch.equal(idx[hit], widx[hit]), f"{name}: the lowest row must win an exact tie"
    return d2, idx


def pair_clouds(seed, n, grid_hw, dev):
    """one synthetic pair, NaN padding removed: pc0 [1,n',3], pc1 [1,n',3], counts"""
    from deflow_amd.synth import synth_pair
    pc0, pc1, _, _ = synth_pair(seed, n, grid_hw)
    ok = torch.isfinite(pc0).all(-1) & torch.isfinite(pc1).all(-1)
    pc0, pc1 = pc0[ok][None].to(dev).contiguous(), pc1[ok][None].to(dev).contiguous()
    return pc0, pc1, i32([pc0.shape[1]], dev)


@pytest.mark.parametrize("n,grid_hw,rng", [(6000, (64, 64), SMALL_RANGE), (20000, (512, 512), None)])
def test_nn_synthetic_pair_both_directions(dev, n, grid_hw, rng):
    pc0, pc1, cnt = pair_clouds(41, n, grid_hw, dev)
    kw = {} if rng is None else {"grid_range": rng}
    for max_d2 in (INF, 4.0, 0.01):      # unbounded, the loss's truncation, a radius that rejects most rows
        check_nn(f"pair {n} pc0->pc1 max_dist2={max_d2}", pc0, cnt, pc1, cnt, max_dist2=max_d2, **kw)
        check_nn(f"pair {n} pc1->pc0 max_dist2={max_d2}", pc1, cnt, pc0, cnt, max_dist2=max_d2, **kw)


def blobs(dev, seed=3):
    """two blobs 60 m apart, a few isolated rows, rows outside the +-51.2 m range (clamped border cells) and non-finite rows"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(1500, 3, generator=g) * torch.tensor([1.5, 1.5, 0.8]) + torch.tensor([-30.0, 5.0, 0.0])
    b = torch.randn(1500, 3, generator=g) * torch.tensor([1.5, 1.5, 0.8]) + torch.tensor([30.0, -5.0, 0.0])
    lone = torch.tensor([[0.0, 0.0, 0.0], [0.0, 45.0, 1.0], [-50.9, -50.9, -2.0], [51.19, 51.19, 2.0], [10.0, -40.0, 0.5]])
    out = torch.tensor([[80.0, 3.0, 0.0], [-75.0, -90.0, 1.0], [51.3, 0.0, 0.0], [0.0, -1.0e6, 0.0], [-3.0e4, 2.0, 0.0],
                        [120.0, 120.0, 0.0]])
    bad = torch.tensor([[float("nan"), 0.0, 0.0], [0.0, INF, 0.0], [1.0, 2.0, -INF], [float("nan")] * 3])
    pts = torch.cat([a, b, lone, out, bad])
    return pts[torch.randperm(pts.shape[0], generator=g)].to(dev)


def test_nn_far_search_border_cells_and_bad_rows(dev):
    """far searches (the neighbour of a row of one blob lies 60 m away when only the other blob is the ref), rows outside the range on
    both sides, and non-finite query / ref rows: those end in +inf / -1 and never in a cell index"""
    pts = blobs(dev)
    q = (pts + torch.tensor([0.3, -0.2, 0.1], device=dev))[None].contiguous()
    r = pts[None].contiguous()
    n = i32([pts.shape[0]], dev)
    d2, idx = check_nn("blobs all", q, n, r, n)
    bad_q = ~torch.isfinite(q[0]).all(-1)
    assert int(bad_q.sum()) == 4 and bool(torch.isinf(d2[0][bad_q]).all()) and bool((idx[0][bad_q] == -1).all())
    bad_r = torch.nonzero(~torch.isfinite(r[0]).all(-1))[:, 0]
    assert not bool(torch.isin(idx[0].long(), bad_r).any())
    check_nn("blobs max_dist2=4", q, n, r, n, max_dist2=4.0)
    # ref = the rows with x > 0 only (labels): every query of the other blob searches ~60 m
    lab_r = (r[0, :, 0] > 0).long()[None]
    check_nn("blobs far", q, n, r, n, rl=lab_r)
    check_nn("blobs far, short of it", q, n, r, n, rl=lab_r, max_dist2=100.0)
    # a coarse and a fine grid give the same answer (the grid only decides the speed)
    a = check_nn("blobs cell 0.25", q, n, r, n, cell=0.25)
    b = check_nn("blobs cell 3.0, small range", q, n, r, n, cell=3.0, grid_range=(-10.0, -10.0, 10.0, 10.0))
    assert torch.equal(a[0], b[0])


def test_nn_labels_counts_batches_and_ties(dev):
    from deflow_amd.synth import synth_pair
    g = torch.Generator().manual_seed(11)
    clouds = [synth_pair(50 + b, 3000, (64, 64), nan_frac=0.0) for b in range(3)]
    pc0 = torch.stack([c[0] for c in clouds]).to(dev)
    pc1 = torch.stack([c[1] for c in clouds]).to(dev)
    c0, c1 = i32([3000, 1700, 2500], dev), i32([2100, 3000, 40], dev)
    l0 = (torch.rand(3, 3000, generator=g) < 0.3).long().to(dev) * 7
    l1 = ((torch.rand(3, 3000, generator=g) < 0.3).long() * torch.randint(1, 90, (3, 3000), generator=g)).to(dev)
    l1[0, :5] = -3                                   # a negative label is no label
    kw = {"grid_range": SMALL_RANGE}
    check_nn("B=3 unequal counts", pc0, c0, pc1, c1, **kw)
    check_nn("B=3 max_dist2=4", pc1, c1, pc0, c0, max_dist2=4.0, **kw)
    check_nn("labels on the query side", pc0, c0, pc1, c1, ql=l0, **kw)
    check_nn("labels on the ref side", pc0, c0, pc1, c1, rl=l1, **kw)
    check_nn("labels on both sides", pc0, c0, pc1, c1, ql=l0, rl=l1, max_dist2=4.0, **kw)
    d2, idx = check_nn("all-zero ref labels", pc0, c0, pc1, c1, rl=torch.zeros_like(l1), **kw)
    assert bool(torch.isinf(d2).all()) and bool((idx == -1).all())
    d2, idx = check_nn("all-zero query labels", pc0, c0, pc1, c1, ql=torch.zeros_like(l0), **kw)
    assert bool(torch.isinf(d2).all())
    d2, idx = check_nn("count = 0 on the ref side", pc0, c0, pc1, i32([0, 3000, 0], dev), **kw)
    assert bool(torch.isinf(d2[0]).all()) and bool(torch.isinf(d2[2]).all()) and bool(torch.isfinite(d2[1, :1700]).all())
    d2, idx = check_nn("count = 0 on the query side", pc0, i32([0, 0, 0], dev), pc1, c1, **kw)
    assert bool((idx == -1).all())
    check_nn("B=1", pc0[:1].contiguous(), c0[:1], pc1[:1].contiguous(), c1[:1], **kw)
    # duplicates: every ref point four times over (shuffled); queries = some of the very same points (distance 0 to four rows) and
    # points beside them (the same non-zero distance, bit for bit, to four rows): the lowest row must win
    base = pc1[0, :600]
    perm = torch.randperm(2400, generator=g).to(dev)
    ref = base.repeat(4, 1)[perm][None].contiguous()
    beside = base[:300] + (torch.randn(300, 3, generator=g) * 0.05).to(dev)
    qry = torch.cat([base[:500], beside])[None].contiguous()
    d2, idx = check_nn("duplicates", qry, i32([800], dev), ref, i32([2400], dev), exact_idx=True, **kw)
    assert bool((d2[0, :500] == 0).all())


def test_nn_full_size(dev):
    """the configs[2] cloud size once: B = 2, 80 000 rows per cloud, the 512 x 512 range"""
    from deflow_amd.synth import synth_batch
    b = synth_batch(2, 80000, seed=9, grid_hw=(512, 512), device=dev)
    n = 80000 - int(80000 * 0.02)
    pc0, pc1 = b["pc0"][:, :n].contiguous(), b["pc1"][:, :n].contiguous()
    cnt = i32([n, n - 5000], dev)
    far = torch.zeros(1, dtype=torch.int32, device=dev)
    check_nn("full size pc0->pc1", pc0, cnt, pc1, cnt, far_count=far)
    check_nn("full size pc1->pc0 max_dist2=4", pc1, cnt, pc0, cnt, max_dist2=4.0)
    print(f"[seflow] full size: {int(far) / 2 / int(cnt.sum()):.3f} of the queries looked past their 3 x 3 cells")


def _chamfer_by_helper(a, b, w0, w1):
    """sum w0 dist0 + sum w1 dist1 through the helper's search and plain autograd (any dtype)"""
    with torch.no_grad():
        _, ia = nn_all_pairs(a, b)
        _, ib = nn_all_pairs(b, a)
    return (w0.to(a.dtype) * ((a - b[ia]) ** 2).sum(-1)).sum() + (w1.to(a.dtype) * ((b - a[ib]) ** 2).sum(-1)).sum()


def test_chamfer_dis_gradients(dev):
    """ChamferDis.apply: distances / indices as the helper's, gradients w.r.t. BOTH clouds against float64 autograd through the helper
    under parity.three_way's rule -- including a target row that is the neighbour of hundreds of rows (the segmented scatter) -- and
    two calls bit-identical"""
    from deflow_amd.chamfer import ChamferDis, chamfer_distance
    pc0, pc1, _ = pair_clouds(77, 5000, (64, 64), dev)
    a, b = pc0[0].clone(), pc1[0].clone()
    g = torch.Generator().manual_seed(5)
    # 400 rows of a crowd around one lone row of b, far from everything else
    lone = torch.tensor([[40.0, 40.0, 0.0]])
    crowd = lone + torch.randn(400, 3, generator=g) * 0.3
    a = torch.cat([a, crowd.to(dev)])
    b = torch.cat([b, lone.to(dev)])
    w0 = (torch.rand(a.shape[0], generator=g) + 0.5).to(dev)
    w1 = (torch.rand(b.shape[0], generator=g) + 0.5).to(dev)

    def run():
        x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        d0, d1, i0, i1 = ChamferDis.apply(x, y)
        ((w0 * d0).sum() + (w1 * d1).sum()).backward()
        return d0.detach(), d1.detach(), i0, i1, x.grad, y.grad

    got, again = run(), run()
    for u, v in zip(got, again):
        assert torch.equal(u, v), "two ChamferDis calls differ"
    d0, d1, i0, i1, ga, gb = got
    assert int((i0 == b.shape[0] - 1).sum()) >= 400          # the lone row collects the crowd
    refs = {}
    for dt in (torch.float32, torch.float64):
        x, y = a.detach().clone().to(dt).requires_grad_(True), b.detach().clone().to(dt).requires_grad_(True)
        _chamfer_by_helper(x, y, w0, w1).backward()
        refs[dt] = (x.grad, y.grad)
    w0d, w0i, w0s = nn_all_pairs(a.double(), b.double(), second=True)
    clear = (w0s - w0d) > 1e-5 * w0d
    assert torch.equal(i0.long()[clear], w0i[clear]) and float(((d0.double() - w0d).abs() / w0d.clamp_min(1e-30)).max()) <= 1e-6
    parity.three_way("test_chamfer_dis_gradients", "d/d pc0", ga, refs[torch.float32][0], refs[torch.float64][0])
    parity.three_way("test_chamfer_dis_gradients", "d/d pc1", gb, refs[torch.float32][1], refs[torch.float64][1])
    # chamfer_distance on top: plain and truncated means
    for trunc in (-1, 4.0):
        got_cd = chamfer_distance(a, b, truncate_dist=trunc)
        dd0, dd1 = nn_all_pairs(a.double(), b.double())[0], nn_all_pairs(b.double(), a.double())[0]
        want = sum((d[d <= trunc].mean() if trunc > 0 else d.mean()) for d in (dd0, dd1))
        assert abs(float(got_cd) - float(want)) <= 1e-5 * float(want), (trunc, float(got_cd), float(want))
    with pytest.raises(TypeError):
        ChamferDis.apply(a.cpu(), b.cpu())


# ---- the training step ------------------------------------------------------------------------------------------------------------------
N_PTS = 6000


def seflow_batch(B, seed, dev, n=N_PTS, with_flow=True):
    from deflow_amd.synth import synth_batch, synth_cluster_labels
    b = synth_batch(B, n, seed=seed, grid_hw=(64, 64), device=dev)
    b["pc0_dynamic"], b["pc1_dynamic"] = synth_cluster_labels(b)
    if not with_flow:
        del b["flow"]
    return b


def fresh(dev, seed=78, dtype="fp32", lr=1e-3, **kw):
    import deflow_amd
    from deflow_amd.optim import Trainer
    torch.manual_seed(seed)
    m = deflow_amd.DeFlow(**SMALL, num_iters=2).to(dev).train()
    return m, Trainer(m, lr=lr, loss_fn="seflowLoss", dtype=dtype, **kw)


def compact_labels(batch, st):
    p0, p1 = st["p0"], st["p1"]
    g = lambda l, ix: torch.gather(l.long(), 1, ix.clamp(0, l.shape[1] - 1))
    return g(batch["pc0_dynamic"], p0.idx_c), g(batch["pc1_dynamic"], p1.idx_c)


@pytest.mark.parametrize("seed,min_dynamic", [(400, 256), (401, 256), (400, 100000)])
def test_trainer_step_matches_the_helper(dev, monkeypatch, seed, min_dynamic):
    """Trainer(loss_fn='seflowLoss').step: the loss, last_loss_terms and the d(flow) handed to the backward against the helper in fp32
    and float64 (parity.three_way's rule), fed with the step's own points_c / flow.  The float64 side first asserts that the inputs
    are well-posed: no distance within 1e-3 of the truncation threshold, and per cluster the two largest eligible raw distances more
    than 1e-5 relative apart.  min_dynamic = 100000: the batch on the other side of the threshold (terms 1 and 3 exactly 0)."""
    seen = {}

    def spy_backward(model, engine, dflow, params, sink):
        seen["dflow"] = dflow.clone()
        return real_backward(model, engine, dflow, params, sink)

    import deflow_amd.autograd as ag
    real_backward = ag.deflow_backward
    monkeypatch.setattr(ag, "deflow_backward", spy_backward)
    m, t = fresh(dev, loss_args=dict(min_dynamic=min_dynamic))
    batch = seflow_batch(2, seed, dev)
    loss = t.step(batch)
    st = m.last_state
    flow, p0, p1 = st["flow"].detach(), st["p0"], st["p1"]
    lab0, lab1 = compact_labels(batch, st)
    assert int(t.last_label_overflow) == 0
    dyn_rows = [int((lab0[b, : int(p0.counts[b])] > 0).sum()) for b in range(2)]
    print(f"[seflow] seed {seed}: counts {p0.counts.tolist()} / {p1.counts.tolist()}, dynamic pc0 rows {dyn_rows}")
    assert min(dyn_rows) > 256
    out = {}
    for dt in (torch.float32, torch.float64):
        f = flow.to(dt).requires_grad_(True)
        rep = {}
        l, terms = seflow_ref(p0.points_c.to(dt), p1.points_c.to(dt), f, p0.counts, p1.counts, lab0, lab1, min_dynamic=min_dynamic,
                              report=rep if dt == torch.float64 else None)
        out[dt] = (l.detach(), terms.detach(), torch.autograd.grad(l, f)[0])
        if dt == torch.float64:
            print(f"[seflow] seed {seed}: nearest distance to the truncation threshold {rep['trunc_gap']:.2e}, smallest relative gap "
                  f"of a cluster's two largest raw distances {rep['cluster_gap']:.2e}")
            assert rep["trunc_gap"] > 1e-3 and rep["cluster_gap"] > 1e-5, rep
    name = f"test_trainer_step_matches_the_helper[{seed}-{min_dynamic}]"
    parity.three_way(name, "loss", loss.reshape(1), out[torch.float32][0].reshape(1), out[torch.float64][0].reshape(1))
    parity.three_way(name, "terms", t.last_loss_terms, out[torch.float32][1], out[torch.float64][1])
    parity.three_way(name, "dflow", seen["dflow"], out[torch.float32][2], out[torch.float64][2])
    if min_dynamic > 256:
        assert bool((t.last_loss_terms[:, 1] == 0).all()) and bool((t.last_loss_terms[:, 3] == 0).all())
    else:
        assert bool((t.last_loss_terms > 0).all())


def test_label_overflow_is_counted(dev):
    m, t = fresh(dev, loss_args=dict(max_label=2))
    batch = seflow_batch(2, 400, dev)
    t.step(batch)
    st = m.last_state
    lab0, _ = compact_labels(batch, st)
    valid = torch.arange(lab0.shape[1], device=dev)[None, :] < st["p0"].counts[:, None]
    want = int(((lab0 > 2) & valid).sum())
    assert want > 0 and int(t.last_label_overflow) == want
    batch["max_label"] = 64                      # the batch's own statement wins
    t.step(batch)
    assert int(t.last_label_overflow) == 0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_direct_step_equals_autograd_step_and_repeats(dev, monkeypatch, dtype):
    """three steps: the direct route bit-identical to DF_TRAINER_AUTOGRAD=1, and a repeated run from the same state bit-identical"""
    out = []
    for env in (None, None, "1"):
        if env:
            monkeypatch.setenv("DF_TRAINER_AUTOGRAD", env)
        m, t = fresh(dev, dtype=dtype, gradient_clip_val=5.0)
        losses = [float(t.step(seflow_batch(2, 410 + i, dev))) for i in range(3)]
        out.append((losses, t.flat.param.clone(), t.opt.exp_avg_sq.clone(), t.last_loss_terms.clone()))
    for other in out[1:]:
        assert out[0][0] == other[0], (out[0][0], other[0])
        assert all(torch.equal(u, v) for u, v in zip(out[0][1:], other[1:]))
    assert all(math.isfinite(v) for v in out[0][0])


def test_captured_step_equals_eager(dev):
    """capture + step_captured on changing batches equals the eager trainer bit for bit -- which also shows the step reads nothing back"""
    bs = [seflow_batch(2, 420 + i, dev) for i in range(2)]
    seq = [bs[1], bs[0], bs[1]]
    m1, t1 = fresh(dev)
    want = [(float(t1.step(b)), t1.last_loss_terms.clone()) for b in seq]
    m2, t2 = fresh(dev)
    t2.capture(bs[0])
    got = []
    for b in seq:
        l = t2.step_captured(b)
        got.append((float(l), t2.last_loss_terms.clone()))
    torch.cuda.synchronize()
    assert [g[0] for g in got] == [w[0] for w in want], (got, want)
    assert all(torch.equal(g[1], w[1]) for g, w in zip(got, want))
    assert torch.equal(t2.flat.param, t1.flat.param) and torch.equal(t2.opt.exp_avg_sq, t1.opt.exp_avg_sq)


def test_batch_without_labels_raises_and_without_flow_trains(dev):
    m, t = fresh(dev)
    b = seflow_batch(2, 430, dev)
    del b["pc1_dynamic"]
    with pytest.raises(ValueError, match="pc0_dynamic"):
        t.step(b)
    b = seflow_batch(2, 430, dev, with_flow=False)
    before = t.flat.param.clone()
    loss = t.step(b)
    assert math.isfinite(float(loss)) and not torch.equal(before, t.flat.param)


def test_it_learns(dev):
    """30 steps of seflowLoss on synthetic pairs lower the seflowLoss of a held-out synthetic batch (the float64 helper on the model's
    eval-mode flow) below the untrained model's.  The held-out EPE before / after is printed, not asserted.
    lr = 2e-4, the reference's and this trainer's default [REF README.md:66].  (Measured once at five times that, the 1e-3 the other
    tests of this file step with: the third step's loss jumps from 3.0 to 10.4, and after 30 steps the eval-mode loss -- BatchNorm
    running statistics -- is 4.10 against 3.13 untrained, while the same parameters score 2.68 in train mode.)"""
    from deflow_amd.metrics import evaluate_batch
    m, t = fresh(dev, seed=123, lr=2e-4)
    held = seflow_batch(2, 9000, dev)

    def held_out():
        m.eval()
        with torch.no_grad():
            res = m(held)
            st = m.forward_padded(held)
            p0, p1 = st["p0"], st["p1"]
            lab0, lab1 = compact_labels(held, st)
            l, terms = seflow_ref(p0.points_c.double(), p1.points_c.double(), st["flow"].double(), p0.counts, p1.counts, lab0, lab1)
            epe = evaluate_batch(res, held).get("EPE", float("nan"))
        m.train()
        return float(l), terms.sum(0).tolist(), float(epe)

    l0, t0, e0 = held_out()
    for i in range(30):
        t.step(seflow_batch(2, 500 + 2 * i, dev))
    l1, t1, e1 = held_out()
    print(f"[seflow] held-out seflowLoss {l0:.4f} -> {l1:.4f} (terms {[round(v, 4) for v in t0]} -> {[round(v, 4) for v in t1]}); "
          f"held-out EPE {e0:.4f} -> {e1:.4f} (not asserted)")
    assert l1 < l0


def test_train_cli_runs_seflow(dev, capsys):
    import deflow_amd.train as T
    T.main(["model=deflow", "lr=2e-4", "epochs=1", "batch_size=2", "loss_fn=seflowLoss", "train_data=synthetic", "model.target.num_iters=2",
            "voxel_size=[0.2, 0.2, 6]", "point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3]", "pairs_per_epoch=4", "points_per_cloud=6000",
            "log_every=1"])
    lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    steps = [l for l in lines if "trainer/loss" in l]
    assert len(steps) == 2
    for l in steps:
        for k in ("chamfer_dis", "dynamic_chamfer_dis", "static_flow_loss", "cluster_flow_loss"):
            assert math.isfinite(l["trainer/" + k]), l
        assert l["trainer/chamfer_dis"] > 0 and l["trainer/static_flow_loss"] > 0
    assert any("val" in l and "EPE" in l["val"] for l in lines)
