"""GPU: the loss and optimiser entry points no other kernel test calls directly -- df_wloss_fwd / _finalize / _bwd (ff3dLoss,
zeroflowLoss), the df_deflow_loss_* trio through the C ABI, df_gather_gt and df_adam_step_dev -- each against a float64 restatement
of its definition (csrc/misc.hip, deflow_amd/losses.py) written here.

Inputs: counts per sample 0, 1, 255, 256, 257, 1000 with N = 1000 (the 256-thread block edge and a full sample); rows that are NaN /
inf in est, others NaN in gt (skipped); rows with est == gt exactly (gradient 0); |gt| on both sides of the deflowLoss bin edges
(speed = |gt| / 0.1 at 0.4 and 1.0), none within 1e-4 of an edge.  nblk = 2 (the grid-stride loop runs) and 64.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 255, 256, 257, 1000]
B, N, NCLS = len(COUNTS), 1000, 1100
GSCALE, GSCALE_DEV = 0.75, 1.7      # host factor x device scalar (!= 1)
SENTINEL = -777.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(31)
    d = torch.randn(B, N, 3, generator=g)
    mag = torch.rand(B, N, 1, generator=g) * 0.2                  # |gt| in [0, 0.2): speeds 0 .. 2 across both bin edges
    gt = d / d.norm(dim=-1, keepdim=True) * mag
    for edge in (0.4, 1.0):                                       # keep 1e-3 clear of the edges (the checks need 1e-4)
        near = ((gt.double().norm(dim=-1) / 0.1 - edge).abs() < 1e-3)
        gt[near] = gt[near] * 1.01
    est = gt + torch.randn(B, N, 3, generator=g) * 0.05
    est[:, 3::17] = gt[:, 3::17]                                  # exact hits: err = 0, gradient 0
    est[:, 5::29] = float("nan")
    est[:, 7::31] = float("inf")
    gt[:, 11::23] = float("nan")
    speed = gt.double().norm(dim=-1) / 0.1
    ok = torch.isfinite(speed)
    assert float((speed[ok] - 0.4).abs().min()) > 1e-4 and float((speed[ok] - 1.0).abs().min()) > 1e-4
    inside = torch.arange(N)[None, :] < torch.tensor(COUNTS)[:, None]
    for lo, hi in ((-1, 0.4), (0.4, 1.0), (1.0, 9)):
        assert int(((speed > lo) & (speed < hi) & inside)[2:].sum(1).min()) > 0   # every sample from 255 rows up fills all three bins
    idx_c = torch.stack([torch.randperm(NCLS, generator=g)[:N] for _ in range(B)])     # compact row -> original point
    idx_c[:, 1::13] = -5                                          # below 0 and at / above Ncls: the kernel clamps
    idx_c[:, 2::19] = NCLS
    idx_c[:, 4::37] = NCLS + 1000
    cls = torch.randint(0, 3, (B, NCLS), generator=g)             # class 0 = background
    counts = torch.tensor(COUNTS, dtype=torch.int32)
    return dict(est=est, gt=gt, idx_c=idx_c.to(torch.int64), cls=cls.to(torch.int64), counts=counts)


def _valid(data):
    rows = torch.arange(N)[None, :] < data["counts"][:, None].long()
    return rows & torch.isfinite(data["est"]).all(-1) & torch.isfinite(data["gt"]).all(-1)


def _weights64(data, kind):
    """float64 [B,N] weight of every row: kind 0 ff3dLoss (0.1 for class 0 of the clamped original index, else 1), kind 1 zeroflowLoss"""
    if kind == 0:
        j = data["idx_c"].clamp(0, NCLS - 1)
        return torch.where(torch.gather(data["cls"], 1, j) > 0, 1.0, 0.1).double()
    speed = torch.nan_to_num(data["gt"].double().norm(dim=-1)) * 10.0
    return torch.clamp(1.8 * speed - 0.8, 0.1, 1.0)


def _grad64(diff, err, scale):
    """d/d est of scale * |est - gt|: scale * diff / err, 0 where err == 0 (the kernels' convention) or the row is not counted"""
    g = diff * (scale / err.clamp_min(1e-300))[..., None]
    return torch.where((err > 0)[..., None] & torch.isfinite(g), g, torch.zeros_like(g))


def _rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


def _dest(dev):
    return torch.full((B, N, 3), SENTINEL, dtype=torch.float32, device=dev)


def _check_rows(dest, want_grad, data, tol, what):
    dest = dest.cpu()
    inside = torch.arange(N)[None, :] < data["counts"][:, None].long()
    assert torch.isfinite(dest).all(), what
    assert bool((dest[~inside] == SENTINEL).all()), f"{what}: rows past the count were written"
    e = _rel(dest[inside], want_grad[inside])
    print(f"[parity] {what}: gradient err / max = {e:.3e} (tol {tol:.0e})")
    assert e <= tol, f"{what}: {e:.3e}"
    assert bool((dest[inside & ~_valid(data)] == 0).all()), f"{what}: a skipped row has a gradient"


@pytest.mark.parametrize("nblk", [2, 64])
@pytest.mark.parametrize("kind", [0, 1])
def test_wloss_kernels_vs_float64(dev, data, kind, nblk):
    """sum over samples of mean over valid rows of w |est - gt|: loss and bins within 1e-6 relative, gradient within 1e-5 of its max"""
    from deflow_amd._lib import call, ptr, stream
    valid = _valid(data)
    diff = torch.nan_to_num(data["est"].double() - data["gt"].double(), nan=0.0, posinf=0.0, neginf=0.0)
    err = diff.norm(dim=-1)
    w = _weights64(data, kind)
    sm = torch.where(valid, w * err, torch.zeros_like(err)).sum(1)
    cn = valid.sum(1).double()
    loss64 = (sm[cn > 0] / cn[cn > 0]).sum()
    gs = GSCALE * GSCALE_DEV
    grad64 = _grad64(diff, err, torch.where(valid, gs * w / cn.clamp_min(1)[:, None], torch.zeros_like(w)))
    if kind == 0:   # the restatement against the oracle's own definition, sample by sample
        from oracle import ref_torch as O
        j = data["idx_c"].clamp(0, NCLS - 1)
        want = sum(O.ff3d_loss(data["est"][b, :n].double(), data["gt"][b, :n].double(), torch.gather(data["cls"], 1, j)[b, :n])
                   for b, n in enumerate(COUNTS) if n and valid[b].any())
        assert abs(float(want) - float(loss64)) <= 1e-7 * float(loss64)       # (the oracle forms its 0.1 / 1.0 weights in fp32)
    else:
        from oracle import ref_torch as O
        want = sum(O.zeroflow_loss(data["est"][b, :n].double(), data["gt"][b, :n].double()) for b, n in enumerate(COUNTS) if n and valid[b].any())
        assert abs(float(want) - float(loss64)) <= 1e-12 * float(loss64)

    d = {k: v.to(dev) for k, v in data.items()}
    cls, idx = (d["cls"], d["idx_c"]) if kind == 0 else (None, None)     # kind 1 reads neither
    partial = torch.full((B, nblk, 2), float("nan"), dtype=torch.float32, device=dev)
    bins = torch.full((B, 2), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    call("df_wloss_fwd", ptr(d["est"]), ptr(d["gt"]), ptr(d["counts"]), B, N, kind, ptr(cls), ptr(idx), NCLS if kind == 0 else 0,
         ptr(partial), nblk, stream())
    call("df_wloss_finalize", ptr(partial), B, nblk, ptr(bins), ptr(loss), stream())
    dest = _dest(dev)
    gdev = torch.tensor([GSCALE_DEV], dtype=torch.float32, device=dev)
    call("df_wloss_bwd", ptr(d["est"]), ptr(d["gt"]), ptr(d["counts"]), B, N, kind, ptr(cls), ptr(idx), NCLS if kind == 0 else 0,
         ptr(bins), ptr(gdev), GSCALE, ptr(dest), nblk, stream())
    torch.cuda.synchronize()
    e_loss = abs(float(loss) - float(loss64)) / float(loss64)
    e_bins = _rel(bins, torch.stack([sm, cn], 1))
    e_cnt = float((bins[:, 1].double().cpu() - cn).abs().max())
    print(f"[parity] wloss kind {kind} nblk {nblk}: loss err {e_loss:.3e}, bins err {e_bins:.3e} (tol 1e-06)")
    assert e_loss <= 1e-6 and e_bins <= 1e-6 and e_cnt == 0
    for b in range(B):      # per sample too: a small sample's sum must not hide behind the 1000-row one
        if cn[b] > 0:
            assert abs(float(bins[b, 0]) - float(sm[b])) <= 1e-6 * float(sm[b]), b
    _check_rows(dest, grad64, data, 1e-5, f"wloss kind {kind} nblk {nblk}")
    # gscale_dev = NULL: the host factor alone
    dest2 = _dest(dev)
    call("df_wloss_bwd", ptr(d["est"]), ptr(d["gt"]), ptr(d["counts"]), B, N, kind, ptr(cls), ptr(idx), NCLS if kind == 0 else 0,
         ptr(bins), None, GSCALE, ptr(dest2), nblk, stream())
    torch.cuda.synchronize()
    _check_rows(dest2, grad64 / GSCALE_DEV, data, 1e-5, f"wloss kind {kind} nblk {nblk} host scale")


@pytest.mark.parametrize("nblk", [2, 64])
def test_deflow_loss_kernels_vs_float64(dev, data, nblk):
    """three speed bins per sample, sum of the per-bin mean errors: the figures of test_ego_transform_loss_adam (loss 1e-5, gradient 1e-4)"""
    from deflow_amd._lib import call, ptr, stream
    from oracle import ref_torch as O
    valid = _valid(data)
    diff = torch.nan_to_num(data["est"].double() - data["gt"].double(), nan=0.0, posinf=0.0, neginf=0.0)
    err = diff.norm(dim=-1)
    speed = torch.nan_to_num(data["gt"].double().norm(dim=-1)) / 0.1
    which = torch.where(speed < 0.4, 0, torch.where(speed <= 1.0, 1, 2))
    bins64 = torch.zeros(B, 6, dtype=torch.float64)
    scale = torch.zeros(B, N, dtype=torch.float64)
    loss64 = 0.0
    gs = GSCALE * GSCALE_DEV
    for k in range(3):
        sel = valid & (which == k)
        bins64[:, 2 * k] = torch.where(sel, err, torch.zeros_like(err)).sum(1)
        bins64[:, 2 * k + 1] = sel.sum(1)
        cn = bins64[:, 2 * k + 1]
        loss64 = loss64 + float((bins64[:, 2 * k][cn > 0] / cn[cn > 0]).sum())
        scale = torch.where(sel, gs / cn.clamp_min(1)[:, None], scale)
    grad64 = _grad64(diff, err, scale)
    want = sum(float(O.deflow_loss(data["est"][b, :n].double(), data["gt"][b, :n].double())) for b, n in enumerate(COUNTS) if n and valid[b].any())
    assert abs(want - loss64) <= 1e-12 * loss64       # the restatement is the oracle's definition

    d = {k: v.to(dev) for k, v in data.items()}
    partial = torch.full((B, nblk, 6), float("nan"), dtype=torch.float32, device=dev)
    bins = torch.full((B, 6), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    call("df_deflow_loss_fwd", ptr(d["est"]), ptr(d["gt"]), ptr(d["counts"]), B, N, ptr(partial), nblk, stream())
    call("df_deflow_loss_finalize", ptr(partial), B, nblk, ptr(bins), ptr(loss), stream())
    dest = _dest(dev)
    gdev = torch.tensor([GSCALE_DEV], dtype=torch.float32, device=dev)
    call("df_deflow_loss_bwd", ptr(d["est"]), ptr(d["gt"]), ptr(d["counts"]), B, N, ptr(bins), ptr(gdev), GSCALE, ptr(dest), nblk, stream())
    torch.cuda.synchronize()
    e_loss = abs(float(loss) - loss64) / loss64
    e_bins = _rel(bins, bins64)
    print(f"[parity] deflow loss nblk {nblk}: loss err {e_loss:.3e}, bins err {e_bins:.3e} (tol 1e-05)")
    assert e_loss <= 1e-5 and e_bins <= 1e-5
    assert bool(((bins.double().cpu() - bins64).abs() <= 1e-5 * bins64).all())        # per sample and bin: a small sample does not hide
    assert torch.equal(bins[:, 1::2].double().cpu(), bins64[:, 1::2])       # the bin populations: no row on the wrong side of an edge
    _check_rows(dest, grad64, data, 1e-4, f"deflow loss nblk {nblk}")


@pytest.mark.parametrize("nblk", [2, 64])
def test_gather_gt_exact(dev, data, nblk):
    """gt[b, i] = flow[b, idx_c[b, i]] - pose_flow[b, idx_c[b, i]] in fp32, exactly; rows past the count untouched"""
    from deflow_amd._lib import call, ptr, stream
    g = torch.Generator().manual_seed(5)
    flow, pose = torch.randn(B, N, 3, generator=g), torch.randn(B, N, 3, generator=g) * 0.3
    idx = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(torch.int64)
    want = torch.gather(flow, 1, idx[..., None].expand(-1, -1, 3)) - torch.gather(pose, 1, idx[..., None].expand(-1, -1, 3))
    out = _dest(dev)
    fd, pd, idd, cd = flow.to(dev), pose.to(dev), idx.to(dev), data["counts"].to(dev)
    call("df_gather_gt", ptr(fd), ptr(pd), ptr(idd), ptr(cd), B, N, ptr(out), nblk, stream())
    torch.cuda.synchronize()
    out = out.cpu()
    inside = torch.arange(N)[None, :] < data["counts"][:, None].long()
    assert torch.equal(out[inside], want[inside])
    assert bool((out[~inside] == SENTINEL).all())


def _adam64(p, grads, lr, b1, b2, eps, gscale):
    p, m, v = p.double().clone(), torch.zeros_like(p, dtype=torch.float64), torch.zeros_like(p, dtype=torch.float64)
    for t, g in enumerate(grads, 1):
        g = g.double() * gscale
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    return p


@pytest.mark.parametrize("n", [4, 4 * (4096 * 256 + 3)])      # one vector; one vector-of-four past 4096 workgroups x 256 threads + a ragged tail
def test_adam_step_dev_matches_host_step_form(dev, n):
    """df_adam_step_dev (step number read from device memory: the form a captured graph replays) is bit-identical to df_adam_step at
    steps 1, 2 and 1000 with grad_scale = 0.37, and three steps of it are within 1e-6 of a float64 Adam"""
    from deflow_amd._lib import call, ptr, stream
    g = torch.Generator().manual_seed(n % 1000 + 3)
    lr, b1, b2, eps, gscale = 2e-4, 0.9, 0.999, 1e-8, 0.37
    p0 = torch.randn(n, generator=g)
    for step in (1, 2, 1000):
        gr = torch.randn(n, generator=g).to(dev)
        m0, v0 = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01
        state = []
        for form in ("host", "dev"):
            p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
            if form == "host":
                call("df_adam_step", ptr(p), ptr(gr), ptr(m), ptr(v), n, lr, b1, b2, eps, step, gscale, stream())
            else:
                sd = torch.tensor([step], dtype=torch.int32, device=dev)
                call("df_adam_step_dev", ptr(p), ptr(gr), ptr(m), ptr(v), n, lr, b1, b2, eps, ptr(sd), gscale, stream())
            torch.cuda.synchronize()
            state.append((p, m, v))
        for a, b, what in zip(state[0], state[1], ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(a, b), f"step {step} {what}: {int((a != b).sum())} of {n} elements differ, max {float((a - b).abs().max()):.3e}"
        assert not torch.equal(state[1][0], p0.to(dev))
    grads = [torch.randn(n, generator=g) for _ in range(3)]
    p, m, v = p0.to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    sd = torch.zeros(1, dtype=torch.int32, device=dev)
    for gr in grads:
        sd += 1
        gd = gr.to(dev)
        call("df_adam_step_dev", ptr(p), ptr(gd), ptr(m), ptr(v), n, lr, b1, b2, eps, ptr(sd), gscale, stream())
    torch.cuda.synchronize()
    e = _rel(p, _adam64(p0, grads, lr, b1, b2, eps, gscale))
    print(f"[parity] adam_step_dev n={n}: 3 steps vs float64 Adam {e:.3e} (tol 1e-06)")
    assert e <= 1e-6
