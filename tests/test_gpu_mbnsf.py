"""GPU: the per-cluster rigidity term and the per-pair flow optimised with it (csrc/iso.hip, deflow_amd/mbnsf.py)
against tests/helpers/iso_ref.py.

The neighbour table and the pair counts are integers and are compared exactly.  Bound of every floating-point comparison: max(1e-4 of the
compared tensor's largest magnitude, 4 x the fp32 helper's own difference from the float64 helper on that case).  Conditions that make a
case well-posed are asserted on the INPUT."""
import numpy as np
import pytest
import torch

from helpers import dt_ref as dr
from helpers import iso_ref as ir
from helpers import nsfp_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANGE = (-6.4, -6.4, -1.6, 6.4, 6.4, 1.6)


def _bound(ref64, ref32):
    return max(1e-4 * float(ref64.abs().max()), 4 * float((ref32.double() - ref64).abs().max()))


def _close(got, ref64, ref32, what):
    err, tol = float((got.double().cpu() - ref64).abs().max()), _bound(ref64, ref32)
    print(f"{what}: err {err:.3e} bound {tol:.3e} (max |ref| {float(ref64.abs().max()):.3e})")
    assert err <= tol, (what, err, tol)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dirty(value):
    """leave `value` in freed blocks of the caching allocator, so that an output element the kernels skip shows it"""
    junk = [torch.full((n,), value, dtype=torch.int16, device=DEV) for n in (1 << 22, 1 << 20, 1 << 18, 1 << 16, 4096, 512)]
    torch.cuda.synchronize()
    del junk


# ---- 1. the plan, exact ---------------------------------------------------------------------------------------------------------------
N, COUNTS = 700, (700, 350, 0)


def _plan_case(P, lattice):
    """B = 3 with counts {N, N / 2, 0}; per sample clusters of 1, 2, 3, P, P + 1, 64, 257 and 300 rows scattered over the rows (they
    interleave in row order; 257 and 300: lists longer than a workgroup), the rest label 0; labelled rows lie behind the counts of
    samples 1 and 2.  x: uniform in a 4 m box, or on a 1/64 m lattice."""
    sizes = [1, 2, 3, P, P + 1, 64, 257, 300]
    assert sum(sizes) <= N - 38
    labels = np.stack([_scatter(N, sizes, 10 * P + b) for b in range(3)])
    gen = torch.Generator().manual_seed(P)
    x = torch.randint(-128, 129, (3, N, 3), generator=gen).float() / 64 if lattice else torch.rand(3, N, 3, generator=gen) * 4 - 2
    return sizes, labels, x


def _scatter(n, sizes, seed):
    rng = np.random.default_rng(seed)
    labels = np.zeros(n, np.int32)
    rows = rng.permutation(n)[:sum(sizes)]
    o = 0
    for l, s in enumerate(sizes, start=1):
        labels[rows[o:o + s]] = l
        o += s
    return labels


@pytest.mark.parametrize("P", [1, 4, 16])
@pytest.mark.parametrize("cap", [64, 8192])
def test_plan_is_exact(P, cap):
    """max_cluster_points = 64: the clusters of 257 and 300 rows are too large and get no partners, the one of 64 rows is the largest
    eligible one; 8192: every cluster of two or more rows is eligible"""
    from deflow_amd import mbnsf
    sizes, labels, x = _plan_case(P, lattice=False)
    for b in (1, 2):
        assert int((labels[b, COUNTS[b]:] > 0).sum()) > 100, "labelled rows behind the count"
    assert all(np.diff(np.flatnonzero(labels[0] == l)).max() > 1 for l in (6, 7, 8)) and int((labels[0] == 0).sum()) >= 38, "interleaved; label-0 rows"
    want = [ir.table(labels[b], COUNTS[b], P, cap) for b in range(3)]
    want_nbr = torch.from_numpy(np.stack([w[0] for w in want]))
    want_m = torch.tensor([w[1] for w in want])
    assert want[0][1] == P * sum(s for s in sizes if 2 <= s <= cap) and 0 < want[1][1] < want[0][1] and want[2][1] == 0
    lab, cnt = torch.from_numpy(labels).to(DEV), torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    outs = []
    for fill in (0x7777, 0x0101):
        _dirty(fill)
        outs.append(mbnsf.iso_plan(x.to(DEV), cnt, lab, pairs=P, max_cluster_points=cap))
    nbr, r0, m = outs[0]
    assert nbr.shape == (3, N, 2 * P) and nbr.dtype == torch.int32 and r0.shape == (3, N, 2 * P) and m.shape == (3,) and m.dtype == torch.int32
    assert torch.equal(nbr.cpu().long(), want_nbr), "the neighbour table (every element written)"
    assert torch.equal(m.cpu().long(), want_m), "the pair instances"
    for a, b2 in zip(outs[0], outs[1]):
        assert torch.equal(_bits(a), _bits(b2)), "two calls are bit-identical"
    # the rest distances: 0 at -1 (every element written), within the bound elsewhere
    r0c = r0.cpu()
    assert not r0c[want_nbr < 0].any()
    for b in range(2):
        r64, r32 = ir.rest(x[b].double(), want[b][0]), ir.rest(x[b], want[b][0])
        _close(r0c[b], r64, r32, f"r0[{b}]")
        assert float(r64.max()) > 2.0
    for b in range(3):
        one = mbnsf.iso_plan(x[b:b + 1].to(DEV), cnt[b:b + 1], lab[b:b + 1].contiguous(), pairs=P, max_cluster_points=cap)
        assert all(torch.equal(_bits(o[0]), _bits(t[b])) for o, t in zip(one, outs[0])), "a sample alone equals the sample inside the batch"
    # a smaller kcap: labels above it are in no list, and the status word says so
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    nbr5, _, m5 = mbnsf.iso_plan(x.to(DEV), cnt, lab, pairs=P, max_cluster_points=cap, kcap=5, status=status)
    w5 = [ir.table(labels[b], COUNTS[b], P, cap, kcap=5) for b in range(3)]
    assert torch.equal(nbr5.cpu().long(), torch.from_numpy(np.stack([w[0] for w in w5]))) and m5.tolist() == [w[1] for w in w5]
    assert int(status) == sum(int((labels[b, :COUNTS[b]] > 5).sum()) for b in range(3))


def test_plan_rest_distances_are_bit_equal_on_a_lattice():
    """x on a 1/64 m lattice inside +-2 m: every difference, square and sum is exact in fp32, the square root is correctly rounded"""
    from deflow_amd import mbnsf
    _, labels, x = _plan_case(4, lattice=True)
    cnt = torch.tensor(COUNTS, dtype=torch.int32, device=DEV)
    nbr, r0, _ = mbnsf.iso_plan(x.to(DEV), cnt, torch.from_numpy(labels).to(DEV), pairs=4, max_cluster_points=8192)
    for b in range(3):
        want = ir.rest(x[b].double(), ir.table(labels[b], COUNTS[b], 4, 8192)[0]).float()
        assert torch.equal(_bits(r0[b].cpu()), _bits(want))
    assert len(torch.unique(r0.cpu())) > 500


# ---- 2. the pairs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 4, 16])
def test_pairs_against_float64(P):
    """the tables of test 1 (every cluster eligible), w = x + F with F = 0.25 m x N(0, 1): chosen on the CPU so that, by the float64
    helper, between 10 % and 90 % of the instances lie beyond delta = 0.2 m (asserted).  The two rows of sample 0's 2-row cluster are
    warped onto one point (r1 = 0: the value counts, the gradient is 0).  NaN behind the counts: those rows are written as 0."""
    from deflow_amd import mbnsf
    delta = 0.2
    _, labels, x = _plan_case(P, lattice=False)
    gen = torch.Generator().manual_seed(100 + P)
    w = x + 0.25 * torch.randn(3, N, 3, generator=gen)
    two = np.flatnonzero(labels[0] == 2)
    w[0, two[1]] = w[0, two[0]]
    tables = [ir.table(labels[b], COUNTS[b], P, 8192) for b in range(3)]
    for b in range(3):
        w[b, COUNTS[b]:] = float("nan")
    cnt, lab = torch.tensor(COUNTS, dtype=torch.int32, device=DEV), torch.from_numpy(labels).to(DEV)
    nbr, r0, m = mbnsf.iso_plan(x.to(DEV), cnt, lab, pairs=P, max_cluster_points=8192)
    assert torch.equal(nbr.cpu().long(), torch.from_numpy(np.stack([t[0] for t in tables])))
    outs = []
    for fill in (0x7f7f, 0x0101):
        _dirty(fill)
        outs.append(mbnsf.iso_pairs(w.to(DEV), nbr, r0, delta=delta))
    v, g = outs[0]
    assert v.shape == (3, N) and g.shape == (3, N, 3)
    assert torch.equal(_bits(v), _bits(outs[1][0])) and torch.equal(_bits(g), _bits(outs[1][1])), "two calls are bit-identical"
    iso = torch.stack([row.clone().sum() for row in v.unbind(0)]) / m.clamp_min(1).float()
    v, g, iso = v.cpu(), g.cpu(), iso.cpu()
    assert not v[2].any() and not g[2].any() and float(iso[2]) == 0.0, "a sample without rows"
    for b in range(2):
        tb, M = tables[b]
        c = COUNTS[b]
        res = {}
        for dt in (torch.float64, torch.float32):
            xb, wb = x[b, :c].to(dt), w[b, :c].to(dt)
            vv, gg, e = ir.term_and_grad(wb, tb[:c], ir.rest(xb, tb[:c]), delta)
            res[dt] = (vv, gg, (vv.sum() / max(M, 1)).reshape(1), e)
        r64, r32 = res[torch.float64], res[torch.float32]
        has = torch.from_numpy(tb[:c, :P] >= 0)
        frac = float((r64[3][has] > delta).double().mean())
        print(b, "instances beyond delta:", frac)
        assert 0.1 <= frac <= 0.9 and int(has.sum()) == M
        _close(v[b, :c], r64[0], r32[0], f"v[{b}]")
        _close(g[b, :c], r64[1], r32[1], f"g[{b}]")
        _close(iso[b].reshape(1), r64[2], r32[2], f"iso[{b}]")
        assert not v[b, c:].any() and not g[b, c:].any(), "behind the count"
        none = torch.from_numpy((tb[:c] < 0).all(axis=1))
        assert not v[b, :c][none].any() and not g[b, :c][none].any() and int(none.sum()) >= 5, "rows without partners"
        assert float(r64[1].abs().max()) > 0.5
    # r1 = 0: the value of the instance is rho(r0) on both rows (P forward instances each), the gradient 0
    rest = float(r0[0, two[0], 0])
    rho = np.float32(rest) ** 2 if rest <= delta else np.float32(delta) * (2 * np.float32(rest) - np.float32(delta))
    assert rest > 0 and not g[0, two].any() and abs(float(v[0, two[0]]) - P * float(rho)) <= 1e-6 * P * float(rho) and float(v[0, two[0]]) == float(v[0, two[1]])


def test_pairs_antisymmetry_and_closed_form():
    from deflow_amd import mbnsf
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    lab = torch.ones(1, 2, dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(8)
    for P in (1, 3, 4, 16):
        # a 2-row cluster: both rows see the same instances from either end, so their gradients are exact negatives
        for _ in range(4):
            x = torch.randn(1, 2, 3, generator=gen).to(DEV)
            w = (x.cpu() + 0.3 * torch.randn(1, 2, 3, generator=gen)).to(DEV)
            nbr, r0, m = mbnsf.iso_plan(x, 2 * one, lab, pairs=P, max_cluster_points=8192)
            assert nbr[0].tolist() == [[1] * (2 * P), [0] * (2 * P)] and int(m) == 2 * P and len(torch.unique(_bits(r0))) == 1
            v, g = mbnsf.iso_pairs(w, nbr, r0, delta=0.05)
            assert torch.equal(_bits(g[0, 0]), _bits(-g[0, 1])) and float(g.abs().max()) > 0 and torch.equal(_bits(v[0, 0]), _bits(v[0, 1]))
        # closed form: 1 m apart at rest, 2 m apart warped along x, delta = 0.25 -> rho = 0.25 (2 - 0.25), rho' = 2 x 0.25 on 2P instances
        x = torch.tensor([[[0.0, 0, 0], [1.0, 0, 0]]], device=DEV)
        nbr, r0, m = mbnsf.iso_plan(x, 2 * one, lab, pairs=P, max_cluster_points=8192)
        assert bool((r0 == 1.0).all())
        v, g = mbnsf.iso_pairs(2 * x, nbr, r0, delta=0.25)
        assert v[0].tolist() == [P * 0.25 * 1.75] * 2 and g[0].tolist() == [[-P * 2 * 2 * 0.25, 0.0, 0.0], [P * 2 * 2 * 0.25, 0.0, 0.0]]
        # at rest the term and its gradient vanish
        v, g = mbnsf.iso_pairs(x, nbr, r0, delta=0.25)
        assert not v.any() and not g.any()


# ---- 3. contract ----------------------------------------------------------------------------------------------------------------------
def test_contract():
    from deflow_amd import mbnsf
    from deflow_amd._lib import load
    x = torch.zeros(2, 8, 3, device=DEV)
    cnt = torch.full((2,), 8, dtype=torch.int32, device=DEV)
    lab = torch.ones(2, 8, dtype=torch.int32, device=DEV)
    kw = dict(pairs=4, max_cluster_points=64)
    nbr, r0, m = mbnsf.iso_plan(x, cnt, lab, **kw)
    assert m.tolist() == [32, 32] and int(nbr.min()) >= 0
    for call, what, exc in ((lambda: mbnsf.iso_plan(x.cpu(), cnt, lab, **kw), "x", TypeError),
                            (lambda: mbnsf.iso_plan(x[:, :, :2], cnt, lab, **kw), "x", ValueError),
                            (lambda: mbnsf.iso_plan(x.double(), cnt, lab, **kw), "x", ValueError),
                            (lambda: mbnsf.iso_plan(x, cnt.long(), lab, **kw), "count", ValueError),
                            (lambda: mbnsf.iso_plan(x, cnt, lab.long(), **kw), "labels", ValueError),
                            (lambda: mbnsf.iso_plan(x, cnt, lab[:, :7], **kw), "labels", ValueError),
                            (lambda: mbnsf.iso_plan(x, cnt, lab.cpu(), **kw), "labels", TypeError),
                            (lambda: mbnsf.iso_plan(x, cnt, lab, pairs=0, max_cluster_points=64), "pairs", ValueError),
                            (lambda: mbnsf.iso_plan(x, cnt, lab, pairs=17, max_cluster_points=64), "pairs", ValueError),
                            (lambda: mbnsf.iso_plan(x, cnt, lab, pairs=4, max_cluster_points=0), "max_cluster_points", ValueError),
                            (lambda: mbnsf.iso_plan(x, cnt, lab, kcap=0, **kw), "kcap", ValueError),
                            (lambda: mbnsf.iso_plan(x, cnt, lab, status=torch.zeros(2, dtype=torch.int32, device=DEV), **kw), "status", ValueError),
                            (lambda: mbnsf.iso_pairs(x.cpu(), nbr, r0, delta=0.2), "w", TypeError),
                            (lambda: mbnsf.iso_pairs(x, nbr.float(), r0, delta=0.2), "nbr", ValueError),
                            (lambda: mbnsf.iso_pairs(x, nbr[:1], r0, delta=0.2), "nbr", ValueError),
                            (lambda: mbnsf.iso_pairs(x, nbr[:, :, :7], r0, delta=0.2), "nbr", ValueError),
                            (lambda: mbnsf.iso_pairs(x, nbr, r0[:, :, :4].contiguous(), delta=0.2), "r0", ValueError),
                            (lambda: mbnsf.iso_pairs(x, nbr, r0.double(), delta=0.2), "r0", ValueError),
                            (lambda: mbnsf.iso_pairs(x, nbr, r0, delta=0.0), "delta", ValueError),
                            (lambda: mbnsf.iso_pairs(x, nbr, r0, delta=float("inf")), "delta", ValueError),
                            (lambda: mbnsf.mbnsf_optimize(x, cnt, x[:1], cnt, grid_range=RANGE), "pc1", ValueError),
                            (lambda: mbnsf.mbnsf_optimize(x, cnt, x, cnt.long(), grid_range=RANGE), "count1", ValueError),
                            (lambda: mbnsf.mbnsf_optimize(x, cnt, x, cnt, grid_range=RANGE, labels=lab.long()), "labels", ValueError),
                            (lambda: mbnsf.mbnsf_optimize(x, cnt, x, cnt, grid_range=RANGE, cell=0.3), "trunc", ValueError),
                            (lambda: mbnsf.mbnsf_optimize(x, cnt, x, cnt, grid_range=RANGE[:4]), "grid_range", ValueError),
                            (lambda: mbnsf.mbnsf_optimize(x, cnt, x, cnt, grid_range=RANGE, init=torch.zeros(2, 8)), "init", ValueError),
                            (lambda: mbnsf.mbnsf_optimize(x, cnt, x, cnt, grid_range=RANGE, rigid_pairs=17), "rigid_pairs", ValueError),
                            (lambda: mbnsf.mbnsf_optimize(x, cnt, x, cnt, grid_range=RANGE, rigid_weight=-1.0), "rigid_weight", ValueError)):
        with pytest.raises(exc, match=what):
            call()
    # the C entries return their codes without launching
    lib = load()
    SHAPE, ALIGN, ARG = -1, -2, -3
    p, q, h = 0x10000, 0x10004, 0x10002
    plan = lambda x=p, count=p, labels=p, off=p, rows=p, B=1, N=8, K=8, P=4, cap=64, nbr=p, r0=p, pairs=p: lib.df_iso_plan(
        x, count, labels, off, rows, B, N, K, P, cap, nbr, r0, pairs, None)
    assert plan(P=0) == SHAPE and plan(P=17) == SHAPE and plan(B=0) == SHAPE and plan(B=65536) == SHAPE and plan(N=0) == SHAPE and plan(K=0) == SHAPE
    assert plan(B=4096, N=1 << 16, P=4) == SHAPE and plan(B=1, N=1 << 26, P=16) == SHAPE              # B N 2P = 2^31
    for k in ("x", "count", "labels", "off", "rows", "nbr", "r0", "pairs"):
        assert plan(**{k: None}) == ARG, k
    assert plan(cap=0) == ARG
    assert plan(nbr=q) == ALIGN and plan(r0=q) == ALIGN and plan(x=h) == ALIGN and plan(pairs=h) == ALIGN and plan(rows=h) == ALIGN
    pairs = lambda w=p, nbr=p, r0=p, B=1, N=8, P=4, delta=0.2, v=p, g=p: lib.df_iso_pairs(w, nbr, r0, B, N, P, delta, v, g, None)
    assert pairs(P=0) == SHAPE and pairs(P=17) == SHAPE and pairs(B=0) == SHAPE and pairs(B=65536) == SHAPE and pairs(N=-1) == SHAPE
    assert pairs(B=4096, N=1 << 16, P=4) == SHAPE
    for k in ("w", "nbr", "r0", "v", "g"):
        assert pairs(**{k: None}) == ARG, k
    assert pairs(delta=0.0) == ARG and pairs(delta=-0.2) == ARG and pairs(delta=float("inf")) == ARG and pairs(delta=float("nan")) == ARG
    assert pairs(nbr=q) == ALIGN and pairs(r0=q) == ALIGN and pairs(w=h) == ALIGN and pairs(v=h) == ALIGN and pairs(g=h) == ALIGN
    torch.cuda.synchronize()


# ---- 4. weight 0 ----------------------------------------------------------------------------------------------------------------------
def _pad_pair(samples, pad0=5, pad1=9):
    """[(P0, P1)] -> pc0s, count0, pc1, count1 on the device, NaN rows behind the counts"""
    n0, n1 = max(len(s[0]) for s in samples) + pad0, max(len(s[1]) for s in samples) + pad1
    a = np.full((len(samples), n0, 3), np.nan, np.float32)
    b = np.full((len(samples), n1, 3), np.nan, np.float32)
    for i, (P0, P1) in enumerate(samples):
        a[i, :len(P0)], b[i, :len(P1)] = P0, P1
    c0 = torch.tensor([len(s[0]) for s in samples], dtype=torch.int32, device=DEV)
    c1 = torch.tensor([len(s[1]) for s in samples], dtype=torch.int32, device=DEV)
    return torch.from_numpy(a).to(DEV), c0, torch.from_numpy(b).to(DEV), c1


def _loop_case():
    """the case of section 6l(5)"""
    samples = [nr.planted_blobs(2, blobs=3, per_blob=40, spacing=2.5, size=(1.2, 0.8, 0.6))[:2],
               nr.planted_blobs(3, blobs=2, per_blob=50, spacing=2.5, size=(1.2, 0.8, 0.6))[:2]]
    return _pad_pair(samples), dict(grid_range=RANGE, depth=1, iters=40, patience=4, min_delta=3e-3, seed=3)


def test_weight_zero_is_fastnsf():
    from deflow_amd import fastnsf, mbnsf
    (pc0s, c0, pc1, c1), kw = _loop_case()
    f0, i0 = fastnsf.fastnsf_optimize(pc0s, c0, pc1, c1, check_every=0, **kw)
    f1, i1 = mbnsf.mbnsf_optimize(pc0s, c0, pc1, c1, check_every=0, rigid_weight=0, **kw)
    assert torch.equal(f1, f0) and f0.any()
    for k in ("loss_history", "best_loss", "params"):
        assert torch.equal(i1[k], i0[k]), k
    assert int(i1["n_pairs"].min()) > 0 and float(i1["last_terms"][:, 1].min()) > 0, "the term was there, with weight 0"
    f2, i2 = mbnsf.mbnsf_optimize(pc0s, c0, pc1, c1, check_every=0, **kw)
    assert not torch.equal(f2, f0) and not torch.equal(i2["loss_history"], i0["loss_history"]), "the default weight changes the result"


# ---- 5. one iteration -----------------------------------------------------------------------------------------------------------------
FACTOR = 32768.0


def test_one_iteration_against_float64():
    """The case of section 6l(4): iters = 1, B = 2 (210 + 150 rows), depth 2, helpers.decided_params (seed 42), the defaults' grid over
    +-6.4 / +-1.6 m.  At that start, as it is, the term is 1e-11: the decided net is nearly constant over a blob.  So the start's
    output-layer weights are multiplied by 32768, chosen on the CPU; pre-activations and ReLU decisions do not change.  The factor alone
    would move every row by the same 6 km (the net's constant part), out of the grid and of fp32's resolution, so the output bias is set
    to minus the mean output over both samples' rows: the warped rows stay inside the grid.  With that start, by the float64 helper on
    the planted partition, the largest entry of d iso / d F is 3.5e-3 and 4.9e-3 and 11.7 % and 10.5 % of the instances lie beyond delta
    (asserted: at least 1e-3, and both branches of rho occur).  Loss, last_terms, F, the gradient and the net after the Adam step against
    the float64 helper fed the op's own cells and labels; the labels equal the planted partition up to renaming."""
    from deflow_amd import mbnsf, nsfp
    depth, cell = 2, dr.f32(0.1)
    P, S = nsfp.num_params(depth), nsfp.param_stride(depth)
    samples = [nr.planted_blobs(2, blobs=3, per_blob=70, spacing=2.5, size=(1.2, 0.8, 0.6))[:2],
               nr.planted_blobs(7, blobs=3, per_blob=50, spacing=2.5, size=(1.2, 0.8, 0.6))[:2]]
    f = nr.decided_params(depth, torch.Generator().manual_seed(42))
    n_out = 3 * nr.H + 3
    f[P - n_out:P - 3] *= FACTOR
    f[P - 3:P] = -nr.mlp_forward(torch.from_numpy(np.concatenate([s[0] for s in samples])).double(), f, depth)[0].mean(0)
    init = torch.zeros(1, S)
    init[0, :P] = f.float()
    pc0s, c0, pc1, c1 = _pad_pair(samples)
    flow, info = mbnsf.mbnsf_optimize(pc0s, c0, pc1, c1, grid_range=RANGE, init=init, depth=depth, iters=1)
    origin, dims, R = dr.grid(RANGE, 0.1, 2.0)
    torch.cuda.synchronize()
    assert info["iters_run"] == 1 and info["loss_history"].shape == (1, 2) and info["params"].shape == (2, 1, S) and int(info["cluster_status"]) == 0
    assert info["last_terms"].shape == (2, 2) and info["labels"].shape == pc0s.shape[:2] and info["labels"].dtype == torch.int32
    w, delta, Pr = mbnsf.DEFAULTS["rigid_weight"], mbnsf.DEFAULTS["rigid_delta"], mbnsf.DEFAULTS["rigid_pairs"]
    for b, (P0, P1) in enumerate(samples):
        P0t, n0 = torch.from_numpy(P0), len(P0)
        labels = info["labels"][b].cpu().numpy()
        assert not labels[n0:].any() and ir.same_partition(labels[:n0], np.repeat([1, 2, 3], n0 // 3)), "the op's labels are the planted blobs"
        nbr, M = ir.table(labels[:n0], n0, Pr, mbnsf.DEFAULTS["max_cluster_points"])
        assert M == Pr * n0 == int(info["n_pairs"][b])
        dt2 = dr.edt_dt2(dr.occupancy(P1, origin, cell, dims), R)
        cells = info["cells"][b].cpu().long()
        res = {}
        for dt in (torch.float64, torch.float32):
            fd = init[0, :P].to(dt)
            loss, terms, F, df, _, W = ir.iteration(P0t.to(dt), dt2, origin, cell, R, fd, depth, nbr, M, w, delta, cells=cells[:n0])
            z = torch.zeros_like(fd)
            res[dt] = (loss.reshape(1), torch.stack(terms), F, df, nr.adam_step(fd, df, z, z, 1)[0], W)
        r64, r32 = res[torch.float64], res[torch.float32]
        # well-posed, on the input: decided ReLUs, a term that matters, both branches of rho, warped rows inside the range
        z64, z32 = nr.mlp_forward(P0t.double(), init[0, :P].double(), depth)[1], nr.mlp_forward(P0t, init[0, :P], depth)[1]
        assert sum(int((a.abs() < _bound(a, c)).sum()) for a, c in zip(z64, z32)) == 0
        _, g_iso, e = ir.term_and_grad(r64[5], nbr, ir.rest(P0t.double(), nbr), delta)
        beyond = float((e > delta).double().mean())
        print(b, "largest entry of d iso / d F:", float(g_iso.abs().max()) / M, "instances beyond delta:", beyond)
        assert float(g_iso.abs().max()) / M >= 1e-3 and 0 < beyond < 1
        lo, hi = torch.tensor(RANGE[:3], dtype=torch.float64), torch.tensor(RANGE[3:], dtype=torch.float64)
        assert bool(((r64[5] > lo) & (r64[5] < hi)).all())
        _close(info["loss_history"][0, b].reshape(1), r64[0], r32[0], f"loss[{b}]")
        _close(info["best_loss"][b].reshape(1), r64[0], r32[0], f"best_loss[{b}]")
        _close(info["last_terms"][b], r64[1], r32[1], f"last_terms[{b}]")
        assert abs(float(info["last_terms"][b, 0] + w * info["last_terms"][b, 1]) - float(info["loss_history"][0, b])) <= 1e-6 * float(r64[0])
        _close(flow[b, :n0], r64[2], r32[2], f"flow[{b}] (the start's F: the only iterate)")
        assert not flow[b, n0:].any()
        _close(info["grads"][b, 0, :P], r64[3], r32[3], f"df[{b}]")
        _close(info["params"][b, 0, :P], r64[4], r32[4], f"f after the step [{b}]")
        assert float(r64[3].abs().max()) > 1e-3


# ---- 6. loop logic --------------------------------------------------------------------------------------------------------------------
def test_loop_logic_is_exact():
    """as section 6l(5), at this model's defaults: snapshot / freeze replayed from the op's own history of the TOTAL loss; check_every
    and the graph change no bit; a sample alone equals itself inside the batch"""
    from deflow_amd import mbnsf
    (pc0s, c0, pc1, c1), kw = _loop_case()
    flow, info = mbnsf.mbnsf_optimize(pc0s, c0, pc1, c1, check_every=0, **kw)
    hist = info["loss_history"].cpu().numpy()
    assert info["iters_run"] == 40 and hist.shape == (40, 2) and np.isfinite(hist).all()
    args = []
    for b in range(2):
        best, stalled, frozen, arg = nr.replay(hist[:, b], kw["patience"], kw["min_delta"])
        print(b, "best", best, "stalled", stalled, "frozen", frozen, "argmin", arg)
        assert np.float32(info["best_loss"][b].item()) == best and int(info["stalled"][b]) == stalled and bool(info["frozen"][b]) == frozen
        args.append(arg)
        if frozen:                       # entries after the freeze keep the last value
            t = arg + kw["patience"]
            assert (hist[t:, b] == hist[t, b]).all()
    assert min(args) >= 1, "the best iterate is not the start"
    for b in range(2):
        f2, i2 = mbnsf.mbnsf_optimize(pc0s, c0, pc1, c1, check_every=0, **dict(kw, iters=args[b] + 1))
        assert torch.equal(_bits(f2[b]), _bits(flow[b])), "the flow is the best iterate's"
        assert torch.equal(_bits(i2["loss_history"][:, b]), _bits(info["loss_history"][:args[b] + 1, b]))
    f1, i1 = mbnsf.mbnsf_optimize(pc0s[1:], c0[1:], pc1[1:], c1[1:], check_every=0, **kw)
    assert torch.equal(_bits(f1[0]), _bits(flow[1])) and torch.equal(_bits(i1["loss_history"][:, 0]), _bits(info["loss_history"][:, 1]))
    assert torch.equal(i1["labels"][0], info["labels"][1]) and int(i1["n_pairs"][0]) == int(info["n_pairs"][1])
    for other in (dict(check_every=5), dict(check_every=0, graph=True), dict(check_every=5, graph=True)):
        f3, i3 = mbnsf.mbnsf_optimize(pc0s, c0, pc1, c1, **dict(kw, **other))
        assert torch.equal(_bits(f3), _bits(flow)), other
        for k in ("best_loss", "loss_history", "stalled", "last_terms"):
            if k == "last_terms" and i3["iters_run"] < 40:
                continue
            assert torch.equal(_bits(i3[k].float() if k == "stalled" else i3[k]), _bits(info[k].float() if k == "stalled" else info[k])), (other, k)
        assert torch.equal(i3["frozen"], info["frozen"])
        if other.get("check_every") and bool(info["frozen"].all()):
            assert i3["iters_run"] < 40


# ---- 7. planted motion ----------------------------------------------------------------------------------------------------------------
def test_planted_motion():
    """section 6l(6)'s case at the defaults of this model: four rigid blobs of 200 rows (1.2 x 0.8 x 0.6 m, 2.5 m apart), the second sweep
    independently re-sampled and moved by 0.6 m each; depth 2, 200 iterations, seed 0, range +-6.4 / +-1.6 m.  Computed on the CPU with
    the committed helper on the planted partition: zero-flow EPE 0.600 m, float64 helper 0.0701 m (at most half of the zero-flow EPE;
    model=fastnsf's helper: 0.1998 m), float32 helper 0.0658 m (within a factor 1.5 of float64's).  The op's labels must be the four
    blobs and its EPE at most twice the float64 helper's: 0.1402 m."""
    from deflow_amd import mbnsf
    P0, P1, truth = nr.planted_blobs(2, blobs=4, per_blob=200, shift=0.6, spacing=2.5, size=(1.2, 0.8, 0.6))
    ref64, ref32 = 0.0700947939184352, 0.06577217688909
    assert abs(float(np.linalg.norm(truth, axis=1).mean()) - 0.6) < 1e-6 and ref64 <= 0.6 / 2 and max(ref64, ref32) <= 1.5 * min(ref64, ref32)
    pc0s, c0, pc1, c1 = _pad_pair([(P0, P1)])
    flow, info = mbnsf.mbnsf_optimize(pc0s, c0, pc1, c1, grid_range=RANGE, depth=2, iters=200, seed=0)
    labels = info["labels"][0].cpu().numpy()
    assert ir.same_partition(labels[:800], np.repeat([1, 2, 3, 4], 200)) and not labels[800:].any() and int(info["n_pairs"][0]) == 4 * 800
    epe = float(np.linalg.norm(flow[0, :len(P0)].cpu().numpy() - truth, axis=1).mean())
    print("EPE", epe, "best_loss", float(info["best_loss"][0]), "last terms", info["last_terms"][0].tolist(), "helper float64", ref64)
    assert epe <= 2 * ref64


# ---- 8. through the stack -------------------------------------------------------------------------------------------------------------
def test_mbnsf_inside_sweepflow_and_metrics():
    from helpers import rigid_ref as rr
    from helpers import sweep_flow_ref as SR
    from deflow_amd import mbnsf, metrics, sweeps
    from deflow_amd.deflow import batch_transform
    rng = np.random.default_rng(9)
    host = {}
    scenes = [rr.planted_sample(4, n_vehicles=2, n_static=1, n_one=0, pad0=0, pad1=0), rr.planted_sample(5, n_vehicles=2, n_static=1, n_one=0, pad0=0, pad1=0)]
    for g, key in (("0", "pc0s"), ("1", "pc1")):
        raws, drops = [], []
        for s in scenes:
            ground = np.stack([rng.uniform(-45, 45, 60), rng.uniform(-45, 45, 60), rng.normal(-1.6, 0.02, 60)], axis=1).astype(np.float32)
            far = np.stack([rng.uniform(52, 60, 20), rng.uniform(-10, 10, 20), rng.uniform(0, 1, 20)], axis=1).astype(np.float32)
            raw = np.concatenate([s[key], ground, far, np.full((1, 3), np.nan, np.float32)])
            drop = np.concatenate([np.zeros(len(s[key])), np.ones(60), np.zeros(21)]).astype(np.uint8)
            p = rng.permutation(len(raw))
            raws.append(raw[p]), drops.append(drop[p])
        n = max(len(r) for r in raws) + 3
        host["raw" + g] = np.full((2, n, 3), np.nan, np.float32)
        host["drop" + g] = np.zeros((2, n), np.uint8)
        for b in range(2):
            host["raw" + g][b, :len(raws[b])], host["drop" + g][b, :len(raws[b])] = raws[b], drops[b]
        host["n" + g] = np.array([len(r) for r in raws], dtype=np.int32)
    pose0 = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    pose1 = pose0.copy()
    pose1[:, :3, 3] = (0.3, -0.02, 0.004)
    d = lambda a: torch.from_numpy(a).to(DEV)
    model = mbnsf.MbNsf(depth=1, iters=3, cell=0.4, trunc=2.0, check_every=0)
    sf = sweeps.SweepFlow(model)
    args = (d(host["raw0"]), d(host["n0"]), d(host["drop0"]), d(host["raw1"]), d(host["n1"]), d(host["drop1"]), d(pose0), d(pose1))
    with torch.no_grad():
        est, dyn = sf.infer(*args)
        st = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in model.last_state.items()}
        est2, dyn2 = sf.infer(*args)
    assert torch.equal(est.view(torch.int32), est2.view(torch.int32)) and torch.equal(dyn, dyn2)
    est, dyn = est.cpu().numpy(), dyn.cpu().numpy()
    T = batch_transform({"pose0": d(pose0), "pose1": d(pose1)}, DEV).cpu().numpy()
    _, _, pos_of, kept = SR.compact_batch(host["raw0"], host["n0"], host["drop0"])
    want, want_dyn = SR.compose_batch(host["raw0"], host["n0"], T, pos_of, st["flow"], st["idx_c0"], st["counts0"])
    assert np.array_equal(est.view(np.int32), want.view(np.int32)) and np.array_equal(dyn, want_dyn)
    for b in range(2):
        c0 = int(st["counts0"][b])
        assert c0 == int(kept[b]) - 21 and np.isfinite(st["flow"][b]).all() and st["flow"][b][:c0].any() and not st["flow"][b][c0:].any()
        assert st["labels"][b][:c0].max() >= 2 and not st["labels"][b][c0:].any() and int(st["n_pairs"][b]) > 0, "the vehicles were clustered"
    assert st["loss_history"].shape == (3, 2) and np.isfinite(st["best_loss"]).all() and (st["last_terms"][:, 1] > 0).all()
    # forward()'s dict of lists into evaluate_batch, host and device
    keep0 = [(np.arange(host["raw0"].shape[1]) < host["n0"][b]) & (host["drop0"][b] == 0) for b in range(2)]
    batch = {"pc0": d(np.stack([np.concatenate([host["raw0"][b][keep0[b]], np.full((st["pc0s"].shape[1] - keep0[b].sum(), 3), np.nan, np.float32)])
                                for b in range(2)])),
             "pc1": d(st["points_c1"]), "pose0": d(pose0), "pose1": d(pose1)}
    batch["flow"] = torch.zeros_like(batch["pc0"])
    batch["flow_is_valid"] = torch.ones(batch["pc0"].shape[:2], dtype=torch.bool, device=DEV)
    batch["flow_category_indices"] = torch.ones(batch["pc0"].shape[:2], dtype=torch.uint8, device=DEV)
    with torch.no_grad():
        res = model(batch)
    assert sorted(res) == ["flow", "pc0_points_lst", "pc0_valid_point_idxes", "pc1_points_lst", "pc1_valid_point_idxes", "pose_flow"]
    assert [int(f.shape[0]) for f in res["flow"]] == st["counts0"].tolist()
    m = metrics.evaluate_batch(res, batch)
    assert {"EPE", "AccS", "AccR"} <= set(m) and all(np.isfinite(v) for v in m.values())
    from deflow_amd.metrics_device import DeviceMetrics, evaluate_batch_device
    dm = DeviceMetrics(torch.device(DEV))
    with torch.no_grad():
        evaluate_batch_device(model, batch, dm)
    assert abs(dm.summary()["EPE"] - m["EPE"]) < 1e-4


def test_save_vis_and_eval_commands(tmp_path, golden_dir, capsys):
    import json
    import os
    import shutil
    from deflow_amd import mbnsf, save, vis
    from deflow_amd.h5scene import H5File
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "scene_val.h5"), tmp_path / "scene_val.h5")      # never written under tests/golden
    small = ["mbnsf_cell=0.4", "mbnsf_trunc=2.0", "mbnsf_iters=3", "mbnsf_depth=1", "mbnsf_rigid_pairs=2"]
    argv = ["model=mbnsf", f"dataset_path={tmp_path}", *small, "mbnsf_check_every=0", "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"]
    assert save.main(argv) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert [x["scene"] for x in lines] == ["scene_val"] and lines[0]["sweeps"] >= 2
    path = save.flow_path(str(tmp_path), "scene_val", "mbnsf")
    assert os.path.basename(path) == "scene_val.mbnsf.flow.npz"
    got, meta = save.read_flow(path), save.read_meta(path)
    assert meta == {"res_name": "mbnsf", "checkpoint": None, "model": "mbnsf", "voxel_size": [0.2, 0.2, 6.0],
                    "point_cloud_range": [-6.4, -6.4, -3.0, 6.4, 6.4, 3.0], "ground_source": "auto", "half": False,
                    "params": dict(mbnsf.DEFAULTS, iters=3, depth=1, check_every=0, cell=0.4, trunc=2.0, rigid_pairs=2),
                    "definition": "DESIGN.md 6f, 6m (UNPINNED)"}
    with H5File(str(tmp_path / "scene_val.h5")) as f:
        ts = sorted(f.keys(), key=int)
        rows = {t: int(f[t]["lidar"].read().shape[0]) for t in ts}
    assert list(got) == ts[:-1]
    for t in ts[:-1]:
        assert got[t][0].dtype == np.float32 and got[t][0].shape == (rows[t], 3) and np.isfinite(got[t][0]).all()
    assert any(got[t][0].any() for t in ts[:-1])
    out_dir = tmp_path / "png"
    assert vis.main([f"dataset_path={tmp_path}", "res_name=mbnsf", "scenes=scene_val", f"out_dir={out_dir}", "range=6.4", "res=0.2",
                     "panels=est"]) == 0
    line = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")][0]
    assert line["scene"] == "scene_val" and line["images"] >= 2 and len(os.listdir(out_dir / "scene_val")) == line["images"]
    from deflow_amd import eval as ev
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "index_total.pkl"), tmp_path / "index_total.pkl")
    out = ev.main(["model=mbnsf", f"val_data={tmp_path}", *small, "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"])
    result = json.loads([x for x in capsys.readouterr().out.splitlines() if x.startswith("{")][-1])
    assert result["model"] == "mbnsf" and result["checkpoint"] is None and "EPE" in result["metrics"] and "leaderboard" in out
