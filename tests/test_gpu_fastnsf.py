"""GPU: the distance transform, its lookup and the per-pair flow optimised on it (csrc/dt.hip, deflow_amd/fastnsf.py)
against tests/helpers/dt_ref.py.

The transform is integer arithmetic and is compared exactly.  Bound of every floating-point comparison: max(1e-4 of the compared tensor's
largest magnitude, 4 x the fp32 helper's own difference from the float64 helper on that case).  Conditions that make a case well-posed are
asserted on the INPUT."""
import numpy as np
import pytest
import torch

from helpers import dt_ref as dr
from helpers import nsfp_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 256        # fastnsf.LINE_TILE (asserted below)
RANGE = (-6.4, -6.4, -1.6, 6.4, 6.4, 1.6)


def _bound(ref64, ref32):
    return max(1e-4 * float(ref64.abs().max()), 4 * float((ref32.double() - ref64).abs().max()))


def _close(got, ref64, ref32, what):
    err, tol = float((got.double().cpu() - ref64).abs().max()), _bound(ref64, ref32)
    print(f"{what}: err {err:.3e} bound {tol:.3e} (max |ref| {float(ref64.abs().max()):.3e})")
    assert err <= tol, (what, err, tol)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _u16(t):
    """a uint16 device tensor -> int64 on the host"""
    return torch.from_numpy(t.cpu().numpy().astype(np.int64))


def _dirty(value):
    """leave `value` in freed blocks of the caching allocator, so that an output element the kernels skip shows it"""
    junk = [torch.full((n,), value, dtype=torch.int16, device=DEV) for n in (1 << 22, 1 << 20, 1 << 18, 1 << 16, 4096, 512)]
    torch.cuda.synchronize()
    del junk


# ---- 1. the transform, exact ----------------------------------------------------------------------------------------------------------
CELL, ORIGIN = 0.25, (-1.75, 0.5, -3.0)      # dyadic: every voxel boundary is an exact fp32 value


def _build_case(dims, R, seed, N=40):
    """B = 3 with counts {N, N // 2, 0}: rows inside the grid, NaN rows, rows outside it, rows on its faces (the low face belongs to
    voxel 0, the high face is outside), more NaN behind the counts"""
    gen = torch.Generator().manual_seed(seed)
    o, ext = torch.tensor(ORIGIN), torch.tensor(dims, dtype=torch.float32) * CELL
    x = o + torch.rand(3, N, 3, generator=gen) * ext
    x[:, 3] = float("nan")
    x[:, 4, 0] = float("inf")
    x[:, 5] = o - 0.3                                   # outside, below
    x[:, 6] = o + ext + 0.01                            # outside, above
    x[:, 7] = o                                         # the low corner: voxel (0, 0, 0)
    x[:, 8] = o + ext                                   # the high corner: outside
    x[:, 9, 0] = (o + ext)[0]                           # on the high x face: outside
    x[:, 10, 1] = o[1]                                  # on the low y face: inside
    x[:, 11] = o + ext - 0.001                          # the last voxel
    x[:, 12] = 1.0e30
    counts = [N, N // 2, 0]
    want = torch.stack([dr.brute_dt2(dr.occupancy(x[b, :c], ORIGIN, CELL, dims), R) for b, c in enumerate(counts)])
    for b, c in enumerate(counts):
        x[b, c:] = float("nan") if b != 1 else 0.0      # behind the count: never read (sample 1: rows that WOULD occupy voxels)
    return x, counts, want


BUILD_CASES = [((2, 2, 2), 1), ((2, 2, 2), 20), ((5, 3, 2), 3), ((70, 33, 17), 1), ((70, 33, 17), 3), ((70, 33, 17), 20),
               ((TILE + 2 * 3 + 1 + 37, 5, 4), 3), ((2 * TILE, 3, 2), 20)]


@pytest.mark.parametrize("dims,R", BUILD_CASES)
def test_transform_is_exact(dims, R):
    """grids (2,2,2), (5,3,2), (70,33,17); an x axis longer than the line tile plus 2R + 1 (300) and one of exactly two tiles; axes shorter
    than R (every axis of (2,2,2) and (5,3,2) at R = 20, z = 17 at R = 20); R in {1, 3, 20}"""
    from deflow_amd import fastnsf
    assert fastnsf.LINE_TILE == TILE
    x, counts, want = _build_case(dims, R, 1000 * R + sum(dims))
    assert int((want[0] == 0).sum()) >= 3 and bool((want[2] == R * R).all())
    xg, cnt = x.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)
    kw = dict(origin=ORIGIN, cell=CELL, dims=dims, radius=R)
    outs = []
    for fill in (0x7777, 0x0101):
        _dirty(fill)
        outs.append(_u16(fastnsf.dt_build(xg, cnt, **kw)))
    assert outs[0].shape == (3, dims[2], dims[1], dims[0])
    assert torch.equal(outs[0], want), "the exact truncated squared distance transform (every element written)"
    assert torch.equal(outs[0], outs[1]), "two calls are bit-identical"
    for b in range(3):
        one = _u16(fastnsf.dt_build(xg[b:b + 1].contiguous(), cnt[b:b + 1], **kw))
        assert torch.equal(one[0], want[b]), "a sample alone equals the sample inside the batch"


def test_transform_of_a_single_point_in_closed_form():
    from deflow_amd import fastnsf
    dims, R = (70, 33, 17), 20
    p = torch.tensor([[[ORIGIN[0] + 41.5 * CELL, ORIGIN[1] + 30.2 * CELL, ORIGIN[2] + 0.9 * CELL]]])
    got = _u16(fastnsf.dt_build(p.to(DEV), torch.ones(1, dtype=torch.int32, device=DEV), origin=ORIGIN, cell=CELL, dims=dims, radius=R))
    z, y, x = torch.meshgrid(torch.arange(17), torch.arange(33), torch.arange(70), indexing="ij")
    assert torch.equal(got[0], ((x - 41) ** 2 + (y - 30) ** 2 + z ** 2).clamp_max(R * R))


# ---- 2. the lookup --------------------------------------------------------------------------------------------------------------------
def _random_dt2(dims, R, n, seed):
    gen = torch.Generator().manual_seed(seed)
    occ = torch.zeros(dims[2], dims[1], dims[0], dtype=torch.bool)
    for _ in range(n):
        occ[int(torch.randint(dims[2], (1,), generator=gen)), int(torch.randint(dims[1], (1,), generator=gen)),
            int(torch.randint(dims[0], (1,), generator=gen))] = True
    return dr.brute_dt2(occ, R)


def _to_dev_u16(dt2):
    return torch.from_numpy(dt2.numpy().astype(np.uint16)).to(DEV)


def test_lookup_against_float64():
    """B = 2 grids of (9, 7, 2) voxels (a G = 2 axis), R = 3, cell 0.2, 700 rows (three blocks): queries with t uniform in [0.05, 0.95] in
    every cell, then queries beyond each of the six faces, a NaN row and rows behind the count"""
    from deflow_amd import fastnsf
    dims, R, cell, origin = (9, 7, 2), 3, dr.f32(0.2), (dr.f32(-0.9), dr.f32(0.3), dr.f32(-0.2))
    N, counts = 700, [700, 333]
    dts = torch.stack([_random_dt2(dims, R, 5, 1), _random_dt2(dims, R, 3, 2)])
    gen = torch.Generator().manual_seed(7)
    G = torch.tensor(dims, dtype=torch.float64)
    i = torch.floor(torch.rand(2, N, 3, generator=gen, dtype=torch.float64) * (G - 1)).clamp_max_(G - 2)
    t = 0.05 + 0.9 * torch.rand(2, N, 3, generator=gen, dtype=torch.float64)
    o64 = torch.tensor(origin, dtype=torch.float64)
    q = o64 + (i + t + 0.5) * cell
    face = {}
    for k in range(6):                                   # rows 100 + k: beyond face k (axis k % 3, low or high), inside on the other axes
        a = k % 3
        q[:, 100 + k, a] = (o64[a] - 0.37) if k < 3 else (o64[a] + dims[a] * cell + 0.41)
        face[100 + k] = a
    q = q.float()
    q[:, 50] = float("nan")
    qg, cnt = q.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV)
    _dirty(0x7f7f)
    d, g, cells, clamped = fastnsf.dt_lookup(qg, cnt, _to_dev_u16(dts), origin=origin, cell=cell, radius=R, return_cells=True)
    d2, g2 = fastnsf.dt_lookup(qg, cnt, _to_dev_u16(dts), origin=origin, cell=cell, radius=R)
    assert torch.equal(_bits(d), _bits(d2)) and torch.equal(_bits(g), _bits(g2))
    d, g, cells, clamped = d.cpu(), g.cpu(), cells.cpu().long(), clamped.cpu()
    for b, c in enumerate(counts):
        assert not d[b, c:].any() and not g[b, c:].any() and not cells[b, c:].any() and not clamped[b, c:].any(), "behind the count"
        assert float(d[b, 50]) == np.float32(R) * np.float32(cell) and not g[b, 50].any() and not cells[b, 50].any(), "a NaN row"
        keep = torch.ones(c, dtype=torch.bool)
        keep[50] = False
        qb = q[b, :c][keep]
        assert float(dr.plane_distance(qb, origin, cell, dims).min()) > 0.04
        d64, g64, c64, k64 = dr.lookup(qb.double(), dts[b], origin, cell, R)
        d32, g32, _, _ = dr.lookup(qb, dts[b], origin, cell, R)
        assert torch.equal(cells[b, :c][keep], c64), "the cells are float64's (every row is at least 0.04 voxel from a plane)"
        assert torch.equal(clamped[b, :c][keep].long(), (k64.long() * torch.tensor([1, 2, 4])).sum(dim=1))
        _close(d[b, :c][keep], d64, d32, f"d[{b}]")
        _close(g[b, :c][keep], g64, g32, f"g[{b}]")
        assert float(g64.abs().max()) > 0.5
        for r, a in face.items():
            assert int(clamped[b, r]) == 1 << a and float(g[b, r, a]) == 0.0
            on = q[b, r].clone().double()                # the clamped position: the centre of the outermost voxel of that axis
            on[a] = o64[a] + (0.5 if r < 103 else dims[a] - 0.5) * cell
            d_on, g_on, _, _ = dr.lookup(on[None], dts[b], origin, cell, R)
            assert abs(float(d[b, r]) - float(d_on)) <= _bound(d64, d32)
            others = [x for x in range(3) if x != a]
            assert float((g[b, r, others].double() - g_on[0, others]).abs().max()) <= _bound(g64, g32)
        assert any(float(g[b, r].abs().max()) > 0 for r in face), "the other axes keep their gradient"


def test_lookup_layout_is_exact():
    """a hand-made dt2 of perfect squares, cell 0.25, a dyadic origin, t in multiples of 1/4: every corner value, weight, product and sum
    is a small dyadic number, so fp32 is exact in any order and d and g must EQUAL float64's.  A swapped axis or corner cannot pass."""
    from deflow_amd import fastnsf
    dims, R, cell, origin = (6, 5, 4), 5, 0.25, (-1.0, 2.5, -0.5)
    gen = torch.Generator().manual_seed(11)
    dts = torch.randint(0, R + 1, (2, dims[2], dims[1], dims[0]), generator=gen) ** 2
    N = 300
    G = torch.tensor(dims, dtype=torch.float64)
    u = torch.floor(torch.rand(2, N, 3, generator=gen, dtype=torch.float64) * (G - 1) * 4) / 4         # 0 .. G - 1 in quarters, planes included
    u[0, 0], u[0, 1] = torch.zeros(3, dtype=torch.float64), G - 1                                     # the corners of the clamp range
    q = (torch.tensor(origin, dtype=torch.float64) + (u + 0.5) * cell).float()
    assert torch.equal(((q.double() - torch.tensor(origin, dtype=torch.float64)) / cell - 0.5), u), "the queries are exact in fp32"
    cnt = torch.tensor([N, N - 7], dtype=torch.int32, device=DEV)
    d, g, cells, clamped = fastnsf.dt_lookup(q.to(DEV), cnt, _to_dev_u16(dts), origin=origin, cell=cell, radius=R, return_cells=True)
    for b, c in enumerate((N, N - 7)):
        d64, g64, c64, k64 = dr.lookup(q[b, :c].double(), dts[b], origin, cell, R)
        assert torch.equal(d[b, :c].cpu().double(), d64) and torch.equal(g[b, :c].cpu().double(), g64)
        assert torch.equal(cells[b, :c].cpu().long(), c64) and not clamped[b].any() and not k64.any()
        assert float(d64.max()) > 0.9 and float(g64.abs().max()) >= 2.0 and len(torch.unique(d64)) > 50          # not a degenerate case


# ---- 3. contract ----------------------------------------------------------------------------------------------------------------------
def test_contract():
    from deflow_amd import fastnsf
    from deflow_amd._lib import load
    x = torch.zeros(2, 8, 3, device=DEV)
    cnt = torch.full((2,), 8, dtype=torch.int32, device=DEV)
    kw = dict(origin=(0.0, 0.0, 0.0), cell=0.5, dims=(4, 4, 4), radius=2)
    dt2 = fastnsf.dt_build(x, cnt, **kw)
    assert dt2.dtype == torch.uint16 and dt2.shape == (2, 4, 4, 4)
    lk = dict(origin=(0.0, 0.0, 0.0), cell=0.5, radius=2)
    for call, what, exc in ((lambda: fastnsf.dt_build(x.cpu(), cnt, **kw), "ref", TypeError),
                            (lambda: fastnsf.dt_build(x[:, :, :2], cnt, **kw), "ref", ValueError),
                            (lambda: fastnsf.dt_build(x.double(), cnt, **kw), "ref", ValueError),
                            (lambda: fastnsf.dt_build(x, cnt.long(), **kw), "count", ValueError),
                            (lambda: fastnsf.dt_build(x, cnt[:1], **kw), "count", ValueError),
                            (lambda: fastnsf.dt_build(x, cnt, **dict(kw, dims=(4, 1, 4))), "dims", ValueError),
                            (lambda: fastnsf.dt_build(x, cnt, **dict(kw, dims=(2048, 2048, 512))), "dims", ValueError),
                            (lambda: fastnsf.dt_build(x, cnt, **dict(kw, radius=256)), "radius", ValueError),
                            (lambda: fastnsf.dt_build(x, cnt, **dict(kw, radius=0)), "radius", ValueError),
                            (lambda: fastnsf.dt_build(x, cnt, **dict(kw, cell=0.0)), "cell", ValueError),
                            (lambda: fastnsf.dt_build(x, cnt, **dict(kw, origin=(0.0, float("nan"), 0.0))), "origin", ValueError),
                            (lambda: fastnsf.dt_lookup(x.cpu(), cnt, dt2, **lk), "query", TypeError),
                            (lambda: fastnsf.dt_lookup(x, cnt.long(), dt2, **lk), "count", ValueError),
                            (lambda: fastnsf.dt_lookup(x, cnt, dt2.view(torch.int16), **lk), "dt2", ValueError),
                            (lambda: fastnsf.dt_lookup(x, cnt, dt2[:1], **lk), "dt2", ValueError),
                            (lambda: fastnsf.dt_lookup(x, cnt, dt2[:, :, :1].contiguous(), **lk), "dims", ValueError),
                            (lambda: fastnsf.dt_lookup(x, cnt, dt2, **dict(lk, radius=300)), "radius", ValueError),
                            (lambda: fastnsf.fastnsf_optimize(x, cnt, x[:1], cnt, grid_range=RANGE), "pc1", ValueError),
                            (lambda: fastnsf.fastnsf_optimize(x, cnt, x, cnt.long(), grid_range=RANGE), "count1", ValueError),
                            (lambda: fastnsf.fastnsf_optimize(x, cnt, x, cnt, grid_range=RANGE, cell=0.3), "trunc", ValueError),
                            (lambda: fastnsf.fastnsf_optimize(x, cnt, x, cnt, grid_range=RANGE[:4]), "grid_range", ValueError),
                            (lambda: fastnsf.fastnsf_optimize(x, cnt, x, cnt, grid_range=RANGE, init=torch.zeros(2, 8)), "init", ValueError),
                            (lambda: fastnsf.fastnsf_optimize(x, cnt, x, cnt, grid_range=RANGE, trunc_d2=4.0), "trunc_d2", ValueError)):
        with pytest.raises(exc, match=what):
            call()
    # the C entries return their codes without launching
    lib = load()
    SHAPE, ALIGN, ARG = -1, -2, -3
    assert lib.df_dt_ws_bytes(2, 4, 4, 4, 2) == 2 * 64 * 2 and lib.df_dt_ws_bytes(1, 3, 3, 3, 1) == 64          # rounded up to 16 bytes
    for bad in ((1, 4, 4, 4, 0), (1, 4, 4, 4, 256), (1, 1, 4, 4, 2), (1, 4, 4, 1, 2), (1, 2048, 2048, 512, 2), (0, 4, 4, 4, 2), (65536, 4, 4, 4, 2)):
        assert lib.df_dt_ws_bytes(*bad) == SHAPE, bad
    p, q = 0x10000, 0x10002
    build = lambda ref=p, count=p, B=1, N=8, cell=0.5, G=(4, 4, 4), R=2, out=p, ws=p, ox=0.0: lib.df_dt_build(ref, count, B, N, ox, 0.0, 0.0, cell, *G, R, out, ws, None)
    assert build(N=0) == SHAPE and build(R=0) == SHAPE and build(R=256) == SHAPE and build(G=(4, 1, 4)) == SHAPE and build(G=(2048, 2048, 512)) == SHAPE
    assert build(ref=None) == ARG and build(count=None) == ARG and build(out=None) == ARG and build(ws=None) == ARG
    assert build(cell=0.0) == ARG and build(cell=float("inf")) == ARG and build(ox=float("nan")) == ARG
    assert build(out=q) == ALIGN and build(ws=p + 8) == ALIGN and build(ref=q) == ALIGN
    look = lambda query=p, count=p, dt=p, B=1, N=8, cell=0.5, G=(4, 4, 4), R=2, d=p, g=p, cells=None, cl=None: lib.df_dt_lookup(
        query, count, dt, B, N, 0.0, 0.0, 0.0, cell, *G, R, d, g, cells, cl, None)
    assert look(N=-1) == SHAPE and look(R=0) == SHAPE and look(G=(4, 4, 1)) == SHAPE and look(B=0) == SHAPE
    assert look(query=None) == ARG and look(dt=None) == ARG and look(d=None) == ARG and look(g=None) == ARG and look(cell=-1.0) == ARG
    assert look(dt=q) == ALIGN and look(d=q) == ALIGN and look(cells=q) == ALIGN
    torch.cuda.synchronize()


# ---- 4. one iteration -----------------------------------------------------------------------------------------------------------------
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


def _ref_dt2(P1, cell=0.1, trunc=2.0):
    origin, dims, R = dr.grid(RANGE, cell, trunc)
    return dr.edt_dt2(dr.occupancy(P1, origin, dr.f32(cell), dims), R), origin, dims, R


def test_one_iteration_against_float64():
    """iters = 1, B = 2 (210 + 150 rows), depth 2, a start whose ReLUs are decided (helpers.decided_params, seed 42), the defaults' grid
    over +-6.4 / +-1.6 m (168 x 168 x 72 voxels): the loss of the start, F, the gradient and the net after the Adam step against the
    float64 helper fed the op's own cells.  Separately the op's cells must be float64's for every row farther than 1e-3 voxel from a
    plane where the cell changes or the clamp begins; chosen on the CPU so that the helper alone puts 99 % and 100 % of the two samples'
    rows that far (asserted: at least 90 %).  The op's grid equals the helper's (scipy's exact transform), exactly."""
    from deflow_amd import fastnsf, nsfp
    depth, cell = 2, dr.f32(0.1)
    P, S = nsfp.num_params(depth), nsfp.param_stride(depth)
    init = torch.zeros(1, S)
    init[0, :P] = nr.decided_params(depth, torch.Generator().manual_seed(42)).float()
    samples = [nr.planted_blobs(2, blobs=3, per_blob=70, spacing=2.5, size=(1.2, 0.8, 0.6))[:2],
               nr.planted_blobs(7, blobs=3, per_blob=50, spacing=2.5, size=(1.2, 0.8, 0.6))[:2]]
    pc0s, c0, pc1, c1 = _pad_pair(samples)
    flow, info = fastnsf.fastnsf_optimize(pc0s, c0, pc1, c1, grid_range=RANGE, init=init, depth=depth, iters=1)
    origin, dims, R = fastnsf.dt_grid(RANGE, 0.1, 2.0)
    assert (origin, dims, R) == dr.grid(RANGE, 0.1, 2.0) and dims == (168, 168, 72)
    grids = _u16(fastnsf.dt_build(pc1, c1, origin=origin, cell=0.1, dims=dims, radius=R))
    torch.cuda.synchronize()
    assert info["iters_run"] == 1 and info["loss_history"].shape == (1, 2) and info["params"].shape == (2, 1, S)
    for b, (P0, P1) in enumerate(samples):
        P0t, n0 = torch.from_numpy(P0), len(P0)
        dt2 = _ref_dt2(P1)[0]
        assert torch.equal(grids[b], dt2), "the op's grid is the exact transform"
        cells = info["cells"][b].cpu().long()
        assert not cells[n0:].any()
        res = {}
        for dt in (torch.float64, torch.float32):
            f = init[0, :P].to(dt)
            loss, F, df, _, _ = dr.iteration(P0t.to(dt), dt2, origin, cell, R, f, depth, cells=cells[:n0])
            z = torch.zeros_like(f)
            res[dt] = (loss, F, df, nr.adam_step(f, df, z, z, 1)[0])
        r64, r32 = res[torch.float64], res[torch.float32]
        # well-posed: no pre-activation inside the forward bound, most rows away from the planes
        z64, z32 = nr.mlp_forward(P0t.double(), init[0, :P].double(), depth)[1], nr.mlp_forward(P0t, init[0, :P], depth)[1]
        assert sum(int((a.abs() < _bound(a, c)).sum()) for a, c in zip(z64, z32)) == 0
        _, _, _, free_cells, W64 = dr.iteration(P0t.double(), dt2, origin, cell, R, init[0, :P].double(), depth)
        far = dr.plane_distance(W64, origin, cell, dims) > 1e-3
        print(b, "rows farther than 1e-3 voxel from a plane:", float(far.float().mean()))
        assert float(far.float().mean()) >= 0.9
        assert torch.equal(cells[:n0][far], free_cells[far]), "the op's cells are float64's away from the planes"
        _close(info["loss_history"][0, b].reshape(1), r64[0].reshape(1), r32[0].reshape(1), f"loss[{b}]")
        _close(info["best_loss"][b].reshape(1), r64[0].reshape(1), r32[0].reshape(1), f"best_loss[{b}]")
        _close(flow[b, :n0], r64[1], r32[1], f"flow[{b}] (the start's F: the only iterate)")
        assert not flow[b, n0:].any()
        _close(info["grads"][b, 0, :P], r64[2], r32[2], f"df[{b}]")
        _close(info["params"][b, 0, :P], r64[3], r32[3], f"f after the step [{b}]")
        assert float(r64[2].abs().max()) > 1e-3


# ---- 5. loop logic --------------------------------------------------------------------------------------------------------------------
def test_loop_logic_is_exact():
    """snapshot / freeze from the op's own loss history, in a pure-Python replay; early stop, check_every and the graph change nothing.
    patience 4 and min_delta 3e-3 were chosen on the CPU: the fp32 helper's histories have their best iterates at 26 and 21 of the 40 iterations and freeze 4 later."""
    from deflow_amd import fastnsf
    samples = [nr.planted_blobs(2, blobs=3, per_blob=40, spacing=2.5, size=(1.2, 0.8, 0.6))[:2],
               nr.planted_blobs(3, blobs=2, per_blob=50, spacing=2.5, size=(1.2, 0.8, 0.6))[:2]]
    pc0s, c0, pc1, c1 = _pad_pair(samples)
    kw = dict(grid_range=RANGE, depth=1, iters=40, patience=4, min_delta=3e-3, seed=3)
    flow, info = fastnsf.fastnsf_optimize(pc0s, c0, pc1, c1, check_every=0, **kw)
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
    assert bool(info["frozen"].any()), "the case freezes at least one sample inside the budget"
    assert min(args) >= 1, "the best iterate is not the start"
    for b in range(2):
        f2, i2 = fastnsf.fastnsf_optimize(pc0s, c0, pc1, c1, check_every=0, **dict(kw, iters=args[b] + 1))
        assert torch.equal(_bits(f2[b]), _bits(flow[b])), "the flow is the best iterate's"
        assert torch.equal(_bits(i2["loss_history"][:, b]), _bits(info["loss_history"][:args[b] + 1, b]))
    # a sample alone: the same result as inside the batch (equal padded N)
    f1, i1 = fastnsf.fastnsf_optimize(pc0s[1:], c0[1:], pc1[1:], c1[1:], check_every=0, **kw)
    assert torch.equal(_bits(f1[0]), _bits(flow[1])) and torch.equal(_bits(i1["loss_history"][:, 0]), _bits(info["loss_history"][:, 1]))
    for other in (dict(check_every=5), dict(check_every=0, graph=True), dict(check_every=5, graph=True)):
        f3, i3 = fastnsf.fastnsf_optimize(pc0s, c0, pc1, c1, **dict(kw, **other))
        assert torch.equal(_bits(f3), _bits(flow)), other
        for k in ("best_loss", "loss_history", "stalled"):
            assert torch.equal(_bits(i3[k].float() if k == "stalled" else i3[k]), _bits(info[k].float() if k == "stalled" else info[k])), (other, k)
        assert torch.equal(i3["frozen"], info["frozen"])
        if other.get("check_every") and bool(info["frozen"].all()):
            assert i3["iters_run"] < 40


# ---- 6. planted motion ----------------------------------------------------------------------------------------------------------------
def test_planted_motion():
    """four rigid blobs of 200 rows (1.2 x 0.8 x 0.6 m, 2.5 m apart), the second sweep independently re-sampled and moved by 0.6 m each;
    depth 2, 200 iterations, seed 0, range +-6.4 / +-1.6 m, every other parameter at its default.  Chosen on the CPU with the helper:
    zero-flow EPE 0.600 m, float64 helper 0.1998 m (at most half of the zero-flow EPE), float32 helper 0.1989 m (within a factor 1.5 of
    float64's).  The op must reach at most twice the float64 helper's EPE."""
    from deflow_amd import fastnsf
    P0, P1, truth = nr.planted_blobs(2, blobs=4, per_blob=200, shift=0.6, spacing=2.5, size=(1.2, 0.8, 0.6))
    ref64, ref32 = 0.19976479230996724, 0.198946421744676
    assert abs(float(np.linalg.norm(truth, axis=1).mean()) - 0.6) < 1e-6 and ref64 <= 0.6 / 2 and max(ref64, ref32) <= 1.5 * min(ref64, ref32)
    pc0s, c0, pc1, c1 = _pad_pair([(P0, P1)])
    flow, info = fastnsf.fastnsf_optimize(pc0s, c0, pc1, c1, grid_range=RANGE, depth=2, iters=200, seed=0)
    epe = float(np.linalg.norm(flow[0, :len(P0)].cpu().numpy() - truth, axis=1).mean())
    print("EPE", epe, "best_loss", float(info["best_loss"][0]), "helper float64", ref64)
    assert epe <= 2 * ref64


# ---- 7. through the stack -------------------------------------------------------------------------------------------------------------
def test_fastnsf_inside_sweepflow_and_metrics():
    from helpers import rigid_ref as rr
    from helpers import sweep_flow_ref as SR
    from deflow_amd import fastnsf, metrics, sweeps
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
    model = fastnsf.FastNsf(depth=1, iters=3, cell=0.4, trunc=2.0, check_every=0)
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
    assert st["loss_history"].shape == (3, 2) and np.isfinite(st["best_loss"]).all()
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
    from deflow_amd import fastnsf, save, vis
    from deflow_amd.h5scene import H5File
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "scene_val.h5"), tmp_path / "scene_val.h5")      # never written under tests/golden
    small = ["fastnsf_cell=0.4", "fastnsf_trunc=2.0", "fastnsf_iters=3", "fastnsf_depth=1"]
    argv = ["model=fastnsf", f"dataset_path={tmp_path}", *small, "fastnsf_check_every=0", "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"]
    assert save.main(argv) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert [x["scene"] for x in lines] == ["scene_val"] and lines[0]["sweeps"] >= 2
    path = save.flow_path(str(tmp_path), "scene_val", "fastnsf")
    assert os.path.basename(path) == "scene_val.fastnsf.flow.npz"
    got, meta = save.read_flow(path), save.read_meta(path)
    assert meta == {"res_name": "fastnsf", "checkpoint": None, "model": "fastnsf", "voxel_size": [0.2, 0.2, 6.0],
                    "point_cloud_range": [-6.4, -6.4, -3.0, 6.4, 6.4, 3.0], "ground_source": "auto", "half": False,
                    "params": dict(fastnsf.DEFAULTS, iters=3, depth=1, check_every=0, cell=0.4, trunc=2.0),
                    "definition": "DESIGN.md 6f, 6l (UNPINNED)"}
    with H5File(str(tmp_path / "scene_val.h5")) as f:
        ts = sorted(f.keys(), key=int)
        rows = {t: int(f[t]["lidar"].read().shape[0]) for t in ts}
    assert list(got) == ts[:-1]
    for t in ts[:-1]:
        assert got[t][0].dtype == np.float32 and got[t][0].shape == (rows[t], 3) and np.isfinite(got[t][0]).all()
    assert any(got[t][0].any() for t in ts[:-1])
    out_dir = tmp_path / "png"
    assert vis.main([f"dataset_path={tmp_path}", "res_name=fastnsf", "scenes=scene_val", f"out_dir={out_dir}", "range=6.4", "res=0.2",
                     "panels=est"]) == 0
    line = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")][0]
    assert line["scene"] == "scene_val" and line["images"] >= 2 and len(os.listdir(out_dir / "scene_val")) == line["images"]
    from deflow_amd import eval as ev
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "index_total.pkl"), tmp_path / "index_total.pkl")
    out = ev.main(["model=fastnsf", f"val_data={tmp_path}", *small, "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"])
    result = json.loads([x for x in capsys.readouterr().out.splitlines() if x.startswith("{")][-1])
    assert result["model"] == "fastnsf" and result["checkpoint"] is None and "EPE" in result["metrics"] and "leaderboard" in out
