"""GPU: the flow field on a voxel grid and the per-pair flow optimised on it (csrc/voxflow.hip, deflow_amd/floxels.py; DESIGN.md section
6n) against tests/helpers/vox_ref.py.

The plan's integers are compared exactly.  Bound of every floating-point comparison: max(1e-4 of the compared tensor's largest magnitude,
4 x the fp32 helper's own difference from the float64 helper on that case).  Conditions that make a case well-posed are asserted on the
INPUT."""
import numpy as np
import pytest
import torch

from helpers import dt_ref as dr
from helpers import nsfp_ref as nr
from helpers import vox_ref as vr

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
DIMS, VOXEL, ORIGIN = (9, 7, 5), 0.5, (-2.0, -1.5, -1.0)
N, COUNTS = 700, (700, 350, 0)
NV, NC = 9 * 7 * 5, 8 * 6 * 4
LONG, MID = (1, 1, 1), (5, 4, 2)           # the cells with 300 and with 65 rows


def _in_cell(rng, c, n):
    """n rows strictly inside cell c = (ix, iy, iz), t in [0.01, 0.99]"""
    return (np.array(ORIGIN) + VOXEL * (np.array(c) + rng.uniform(0.01, 0.99, (n, 3)))).astype(np.float32)


def _plan_rows(seed):
    """one sample's N rows, in a random order (the cells' rows interleave), and the kind of every row: 0 strictly inside a cell, 1 on
    the 1/64 m lattice (some of them on node planes), 2 on the upper faces, 3 outside the range, 4 NaN"""
    rng = np.random.default_rng(seed)
    hi = np.array(ORIGIN) + VOXEL * (np.array(DIMS) - 1)
    parts, kinds = [_in_cell(rng, LONG, 300), _in_cell(rng, MID, 65)], [0] * 365
    cells = [(ix, iy, iz) for ix in (0, 2, 3, 6, 7) for iy in (0, 2, 5) for iz in (0, 3)]        # empty cells between occupied ones
    for k in rng.integers(0, len(cells), 165):
        parts.append(_in_cell(rng, cells[k], 1)), kinds.append(0)
    lat = np.array(ORIGIN) + rng.integers(0, (np.array(DIMS) - 1) * 32 + 1, (100, 3)) / 64.0
    lat[:30] = np.array(ORIGIN) + VOXEL * rng.integers(0, np.array(DIMS), (30, 3))              # on node planes of all three axes
    lat[30:45, 0] = ORIGIN[0] + VOXEL * rng.integers(0, DIMS[0], 15)                             # on an x plane only
    parts.append(lat.astype(np.float32)), kinds.extend([1] * 100)
    up = np.array(ORIGIN) + rng.integers(0, (np.array(DIMS) - 1) * 32 + 1, (30, 3)) / 64.0
    up[:10, 0], up[10:20, 1], up[20:28, 2], up[28:] = hi[0], hi[1], hi[2], hi                     # i = V - 2, t = 1
    parts.append(up.astype(np.float32)), kinds.extend([2] * 30)
    out = rng.uniform(-1, 1, (30, 3)) * 2
    out[:10, 0], out[10:20, 1], out[20:, 2] = hi[0] + rng.uniform(0.1, 3, 10), ORIGIN[1] - rng.uniform(0.1, 3, 10), hi[2] + 1e4
    parts.append(out.astype(np.float32)), kinds.extend([3] * 30)
    bad = _in_cell(rng, MID, 10)
    bad[:4, 0], bad[4:7, 1], bad[7:, 2] = np.nan, np.inf, -np.inf
    parts.append(bad), kinds.extend([4] * 10)
    x, kinds = np.concatenate(parts), np.array(kinds)
    assert len(x) == N
    p = rng.permutation(N)
    return x[p], kinds[p]


_PLAN = {}


def _plan_case():
    """B = 3 with counts {700, 350, 0}, NaN behind the counts; the helper's plan of every sample, computed once and shared"""
    if not _PLAN:
        rows = [_plan_rows(20 + b) for b in range(3)]
        x = np.stack([r[0] for r in rows])
        kinds = np.stack([r[1] for r in rows])
        for b in range(3):
            x[b, COUNTS[b]:] = np.nan
        plans = [vr.plan(x[b], COUNTS[b], ORIGIN, VOXEL, DIMS) for b in range(3)]
        idx_sorted, rng = vr.grouping([p[0] for p in plans], NC)
        acts = [vr.active_nodes(p[0], DIMS) for p in plans]
        _PLAN.update(x=x, kinds=kinds, plans=plans, idx_sorted=idx_sorted, rng=rng, acts=acts)
    return _PLAN


def _gpu_plan(x, counts):
    from deflow_amd import floxels
    return floxels.vox_plan(torch.from_numpy(x).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), origin=ORIGIN, voxel=VOXEL, dims=DIMS)


def test_plan_is_exact():
    c = _plan_case()
    x, kinds, plans = c["x"], c["kinds"], c["plans"]
    # the input: clearances, the long cells, empty cells between occupied ones, NaN inside a count
    for b in range(2):
        head = np.arange(N) < COUNTS[b]
        u = (x[b].astype(np.float64) - np.array(ORIGIN)) / VOXEL
        inside = head & (kinds[b] == 0)
        assert np.abs(u[inside] - np.round(u[inside])).min() >= 1e-3, "strictly inside: at least 1e-3 voxel clear of every plane"
        cell = plans[b][0]
        per = np.bincount(cell[cell >= 0], minlength=NC)
        long_c, mid_c = (LONG[2] * 6 + LONG[1]) * 8 + LONG[0], (MID[2] * 6 + MID[1]) * 8 + MID[0]
        if b == 0:
            assert per[long_c] >= 300 and per[mid_c] >= 65 and per.max() == per[long_c], "a cell longer than a workgroup, one of 65 rows"
        occ = per > 0
        assert 20 <= occ.sum() < NC and (occ[2:] & ~occ[1:-1] & occ[:-2]).any(), "empty cells between occupied ones"
        assert int((head & (kinds[b] == 4)).sum()) >= 2 and (cell[head & (kinds[b] == 4)] == -1).all() and (cell[~head] == -1).all()
        up = head & (kinds[b] == 2)
        assert (plans[b][1][up] == 1).any() and (plans[b][1][head & (kinds[b] == 1)] == 0).any()
        assert (cell[head & (kinds[b] == 3)] >= 0).all(), "rows outside the range are clamped, not dropped"
    want_cell = torch.from_numpy(np.stack([p[0] for p in plans]))
    want_act = torch.from_numpy(np.stack([a[0].reshape(-1) for a in c["acts"]]))
    want_m = torch.tensor([a[1] for a in c["acts"]])
    assert want_m[0] > want_m[1] > 0 and want_m[2] == 0 and 0 < int(want_act[0].sum()) < NV
    outs = []
    for fill in (0x7777, 0x0101):
        _dirty(fill)
        outs.append(_gpu_plan(x, COUNTS))
    p = outs[0]
    assert p["cell"].shape == (3, N) and p["frac"].shape == (3, N, 3) and p["idx_sorted"].shape == (3 * N,) and p["cell_rng"].shape == (3 * NC, 2)
    assert p["active"].shape == (3, NV) and p["active"].dtype == torch.uint8 and p["pairs"].shape == (3,) and p["dims"] == DIMS
    assert torch.equal(p["cell"].cpu().long(), want_cell), "the cells (every element written)"
    assert torch.equal(p["active"].cpu().bool(), want_act), "the active nodes"
    assert torch.equal(p["pairs"].cpu().long(), want_m), "the pairs"
    assert torch.equal(p["idx_sorted"].cpu().long(), torch.from_numpy(c["idx_sorted"])), "the grouping: rows (-1 behind the grouped rows)"
    assert torch.equal(p["cell_rng"].cpu().long(), torch.from_numpy(c["rng"])), "the grouping: ranges"
    for k in ("cell", "frac", "idx_sorted", "cell_rng", "pairs"):
        assert torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), ("two calls are bit-identical", k)
    assert torch.equal(outs[0]["active"], outs[1]["active"])
    # the fractions: within the bound of the float64 value at the helper's cell, 0 where the row does not take part, bit-equal on the lattice
    frac = p["frac"].cpu()
    for b in range(3):
        cell, f32, idx = plans[b]
        part = cell >= 0
        assert not frac[b][torch.from_numpy(~part)].any()
        if not part.any():
            continue
        u = np.clip((x[b][part].astype(np.float64) - np.array(ORIGIN, np.float32).astype(np.float64)) / np.float64(np.float32(VOXEL)), 0,
                    np.array(DIMS) - 1)
        f64 = torch.from_numpy(u - idx[part])
        _close(frac[b][torch.from_numpy(part)], f64, torch.from_numpy(f32[part]), f"frac[{b}]")
        lattice = part & np.isin(kinds[b], (1, 2))
        assert lattice.sum() > 50 and torch.equal(_bits(frac[b][torch.from_numpy(lattice)]), _bits(torch.from_numpy(f32[lattice])))
        print(b, "all fractions bit-equal to the fp32 helper:", torch.equal(_bits(frac[b]), _bits(torch.from_numpy(f32))))
    # a sample alone equals the sample inside the batch (the grouping up to the slots and rows of the samples before it)
    for b in range(3):
        one = _gpu_plan(x[b:b + 1], COUNTS[b:b + 1])
        for k in ("cell", "frac", "active", "pairs"):
            assert torch.equal(one[k][0], p[k][b]), (b, k)
        base = int(p["cell_rng"][b * NC, 0])
        kept = int((plans[b][0] >= 0).sum())
        assert torch.equal(one["cell_rng"], p["cell_rng"][b * NC:(b + 1) * NC] - base)
        assert torch.equal(one["idx_sorted"][:kept], p["idx_sorted"][base:base + kept] - b * N) and bool((one["idx_sorted"][kept:] == -1).all())


# ---- 2. the read and its transpose ----------------------------------------------------------------------------------------------------
def test_sample_and_scatter_against_float64():
    """item 1's plan; theta = N(0, 1) on every node, dF = N(0, 1) on every row with NaN behind the counts"""
    from deflow_amd import floxels
    c = _plan_case()
    gen = torch.Generator().manual_seed(5)
    theta = torch.randn(3, DIMS[2], DIMS[1], DIMS[0], 3, generator=gen)
    dF = torch.randn(3, N, 3, generator=gen)
    for b in range(3):
        dF[b, COUNTS[b]:] = float("nan")
    p = _gpu_plan(c["x"], COUNTS)
    outs = []
    for fill in (0x7f7f, 0x0101):
        _dirty(fill)
        outs.append((floxels.vox_sample(theta.to(DEV), p["cell"], p["frac"]),
                     floxels.vox_scatter(dF.to(DEV), p["frac"], p["idx_sorted"], p["cell_rng"], dims=DIMS)))
    F, dth = outs[0]
    assert F.shape == (3, N, 3) and dth.shape == (3, NV, 3)
    assert torch.equal(_bits(F), _bits(outs[1][0])) and torch.equal(_bits(dth), _bits(outs[1][1])), "two calls are bit-identical"
    F, dth = F.cpu(), dth.cpu()
    assert not F[2].any() and not dth[2].any(), "a sample without rows"
    for b in range(2):
        pl, act = c["plans"][b], torch.from_numpy(c["acts"][b][0].reshape(-1))
        part = torch.from_numpy(pl[0] >= 0)
        res = {}
        for dt in (torch.float64, torch.float32):
            res[dt] = (vr.sample(theta[b].to(dt), *pl), vr.scatter(dF[b].to(dt), *pl, DIMS, dt).reshape(NV, 3))
        (F64, d64), (F32, d32) = res[torch.float64], res[torch.float32]
        _close(F[b], F64, F32, f"F[{b}]")
        _close(dth[b], d64, d32, f"dtheta[{b}]")
        assert not F[b][~part].any() and int((~part).sum()) > 0, "0 at cell = -1"
        assert not dth[b][~act].any() and 0 < int(act.sum()) < NV, "a node with nothing incident gets exactly 0"
        assert float(d64.abs().max()) > 3, "the long cell's corners sum hundreds of rows"
        # the transpose identity, in float64 sums of the op's outputs
        dFc = torch.where(part[:, None], dF[b], torch.zeros(1)).double()
        I64, I32 = float((F64 * dFc).sum()), float((F32.double() * dFc).sum())
        tol = max(1e-4 * abs(I64), 4 * abs(I32 - I64))
        lhs, rhs = float((F[b].double() * dFc).sum()), float((theta[b].reshape(NV, 3).double() * dth[b].double()).sum())
        print(b, "<sample(theta), dF>", lhs, "<theta, scatter(dF)>", rhs, "float64 helper", I64, "bound", tol)
        assert abs(I64) > 1 and abs(lhs - I64) <= tol and abs(rhs - I64) <= tol and abs(lhs - rhs) <= tol
    # a sample alone equals the sample inside the batch, bit for bit
    one = _gpu_plan(c["x"][1:2], COUNTS[1:2])
    d1 = floxels.vox_scatter(dF[1:2].to(DEV), one["frac"], one["idx_sorted"], one["cell_rng"], dims=DIMS)
    assert torch.equal(_bits(d1[0].cpu()), _bits(dth[1]))


def test_scatter_at_the_long_cell_threshold():
    """df_vox_scatter sums a cell of more than 128 rows with the node's whole wave and a shorter one with the node's own thread: cells of
    exactly 128, 129, 1000 (16 rows per lane) and 64 rows in a 4 x 3 x 3 grid, their rows interleaved; sample 1 counts the first 900 rows
    only, so its cells are shorter.  Against float64; two calls bit-identical; a sample alone equals itself inside the batch."""
    from deflow_amd import floxels
    dims, voxel, origin = (4, 3, 3), 0.5, (0.0, 0.0, 0.0)
    rng = np.random.default_rng(31)
    sizes = {(0, 0, 0): 128, (1, 0, 0): 129, (2, 1, 1): 1000, (0, 1, 1): 64}
    n = sum(sizes.values()) + 5
    xs = []
    for b in range(2):
        x = np.concatenate([voxel * (np.array(c) + rng.uniform(0.01, 0.99, (k, 3))) for c, k in sizes.items()] + [np.full((5, 3), np.nan)])
        xs.append(x[rng.permutation(n)].astype(np.float32))
    x, counts = np.stack(xs), (n, 900)
    plans = [vr.plan(x[b], counts[b], origin, voxel, dims) for b in range(2)]
    per = [np.bincount(p[0][p[0] >= 0], minlength=12) for p in plans]
    assert sorted(per[0][per[0] > 0]) == [64, 128, 129, 1000] and 129 < per[1].max() < 1000 and (per[1] > 0).sum() == 4
    gen = torch.Generator().manual_seed(32)
    dF = torch.randn(2, n, 3, generator=gen)
    dF[1, 900:] = float("nan")
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    p = floxels.vox_plan(torch.from_numpy(x).to(DEV), cnt, origin=origin, voxel=voxel, dims=dims)
    assert torch.equal(p["cell"].cpu().long(), torch.from_numpy(np.stack([q[0] for q in plans])))
    _dirty(0x7f7f)
    dth = floxels.vox_scatter(dF.to(DEV), p["frac"], p["idx_sorted"], p["cell_rng"], dims=dims)
    again = floxels.vox_scatter(dF.to(DEV), p["frac"], p["idx_sorted"], p["cell_rng"], dims=dims)
    assert torch.equal(_bits(dth), _bits(again)), "two calls are bit-identical"
    for b in range(2):
        d64, d32 = vr.scatter(dF[b].double(), *plans[b], dims, torch.float64), vr.scatter(dF[b], *plans[b], dims, torch.float32)
        _close(dth[b], d64.reshape(-1, 3), d32.reshape(-1, 3), f"dtheta[{b}]")
        act = torch.from_numpy(vr.active_nodes(plans[b][0], dims)[0].reshape(-1))
        assert not dth[b].cpu()[~act].any() and 0 < int(act.sum()) < 36
        one = floxels.vox_plan(torch.from_numpy(x[b:b + 1]).to(DEV), cnt[b:b + 1], origin=origin, voxel=voxel, dims=dims)
        d1 = floxels.vox_scatter(dF[b:b + 1].to(DEV), one["frac"], one["idx_sorted"], one["cell_rng"], dims=dims)
        assert torch.equal(_bits(d1[0]), _bits(dth[b])), "a sample alone equals the sample inside the batch"


# ---- 3. the smoothness term -----------------------------------------------------------------------------------------------------------
def _smooth_check(theta, act, what):
    """theta [B,VZ,VY,VX,3], act bool [B,VZ,VY,VX] (host) against the helper in float64"""
    from deflow_amd import floxels
    B = theta.shape[0]
    _dirty(0x7f7f)
    v, g = floxels.vox_smooth(theta.to(DEV), torch.from_numpy(act.reshape(B, -1).astype(np.uint8)).to(DEV))
    v2, g2 = floxels.vox_smooth(theta.to(DEV), torch.from_numpy(act.reshape(B, -1).astype(np.uint8)).to(DEV))
    assert torch.equal(_bits(v), _bits(v2)) and torch.equal(_bits(g), _bits(g2))
    v, g = v.cpu(), g.cpu()
    for b in range(B):
        a = torch.from_numpy(act[b].reshape(-1))
        v64, g64 = vr.smooth_and_grad(theta[b].double(), act[b])
        v32, g32 = vr.smooth_and_grad(theta[b], act[b])
        assert not v[b][~a].any() and not g[b][~a].any(), "0 at an inactive node"
        if vr.n_pairs(act[b]) == 0:
            assert not v[b].any() and not g[b].any(), (what, b, "no pairs: every output is 0")
            continue
        _close(v[b], v64.reshape(-1), v32.reshape(-1), f"{what} v[{b}]")
        _close(g[b], g64.reshape(-1, 3), g32.reshape(-1, 3), f"{what} g[{b}]")
    return v, g


def test_smooth_against_float64():
    c = _plan_case()
    gen = torch.Generator().manual_seed(6)
    # item 1's active nodes
    act = np.stack([a[0] for a in c["acts"]])
    v, g = _smooth_check(torch.randn(3, DIMS[2], DIMS[1], DIMS[0], 3, generator=gen), act, "plan")
    assert float(v[0].sum()) > 100 and not v[2].any()
    # given patterns on a 5 x 4 x 3 grid: an isolated node, a full line along each axis, a fully active grid, all inactive
    pat = np.zeros((6, 3, 4, 5), bool)
    pat[0, 1, 2, 3] = True
    pat[1, 1, 2, :] = True
    pat[2, 2, :, 0] = True
    pat[3, :, 3, 4] = True
    pat[4] = True
    assert [vr.n_pairs(a) for a in pat] == [0, 4, 3, 2, 3 * 4 * 4 + 3 * 3 * 5 + 2 * 4 * 5, 0]
    v, g = _smooth_check(torch.randn(6, 3, 4, 5, 3, generator=gen), pat, "patterns")
    assert not v[0].any() and not g[0].any() and not v[5].any() and not g[5].any()
    assert int((v[1] != 0).sum()) == 4 and int((v[2] != 0).sum()) == 3 and int((v[3] != 0).sum()) == 2, "one value per pair, at its lower end"
    assert int((v[4] == 0).sum()) == 1, "a fully active grid: only the last corner has no forward neighbour"
    # closed form: two active x-neighbours with theta = (0,0,0) and (1,2,2); an inactive node's theta is ignored
    a2 = np.zeros((1, 2, 2, 2), bool)
    a2[0, 0, 0, :] = True
    t2 = torch.zeros(1, 2, 2, 2, 3)
    t2[0, 0, 0, 1] = torch.tensor([1.0, 2.0, 2.0])
    t2[0, 1, 1, 1] = 7.0
    v, g = _smooth_check(t2, a2, "closed form")
    assert v[0].tolist() == [9.0, 0, 0, 0, 0, 0, 0, 0] and g[0, 0].tolist() == [-2.0, -4.0, -4.0] and g[0, 1].tolist() == [2.0, 4.0, 4.0]
    assert not g[0, 2:].any()


# ---- 4. contract ----------------------------------------------------------------------------------------------------------------------
def test_contract():
    from deflow_amd import floxels
    from deflow_amd._lib import load
    x = torch.tensor([[[a, b, c] for c in (0.25, 0.75) for b in (0.25, 0.75) for a in (0.25, 0.75)]] * 2, device=DEV)      # a row in every cell
    cnt = torch.full((2,), 8, dtype=torch.int32, device=DEV)
    kw = dict(origin=(0.0, 0.0, 0.0), voxel=0.5, dims=(3, 3, 3))
    p = floxels.vox_plan(x, cnt, **kw)
    th = torch.zeros(2, 3, 3, 3, 3, device=DEV)
    assert p["pairs"].tolist() == [54, 54] and int(p["cell"].min()) >= 0
    sc = lambda dF=x, frac=p["frac"], idx=p["idx_sorted"], rng=p["cell_rng"], dims=(3, 3, 3): floxels.vox_scatter(dF, frac, idx, rng, dims=dims)
    opt = lambda *a, **k: floxels.floxels_optimize(*a, **k)
    for call, what, exc in ((lambda: floxels.vox_plan(x.cpu(), cnt, **kw), "x", TypeError),
                            (lambda: floxels.vox_plan(x[:, :, :2], cnt, **kw), "x", ValueError),
                            (lambda: floxels.vox_plan(x.double(), cnt, **kw), "x", ValueError),
                            (lambda: floxels.vox_plan(x, cnt.long(), **kw), "count", ValueError),
                            (lambda: floxels.vox_plan(x, cnt.cpu(), **kw), "count", TypeError),
                            (lambda: floxels.vox_plan(x, cnt, origin=(0.0, 0.0), voxel=0.5, dims=(3, 3, 3)), "origin", ValueError),
                            (lambda: floxels.vox_plan(x, cnt, origin=(0.0, 0.0, float("nan")), voxel=0.5, dims=(3, 3, 3)), "origin", ValueError),
                            (lambda: floxels.vox_plan(x, cnt, origin=(0.0, 0.0, 0.0), voxel=0.0, dims=(3, 3, 3)), "voxel", ValueError),
                            (lambda: floxels.vox_plan(x, cnt, origin=(0.0, 0.0, 0.0), voxel=float("inf"), dims=(3, 3, 3)), "voxel", ValueError),
                            (lambda: floxels.vox_plan(x, cnt, origin=(0.0, 0.0, 0.0), voxel=0.5, dims=(3, 3, 1)), "dims", ValueError),
                            (lambda: floxels.vox_plan(x, cnt, origin=(0.0, 0.0, 0.0), voxel=0.5, dims=(2048, 2048, 512)), "dims", ValueError),
                            (lambda: floxels.vox_sample(th.cpu(), p["cell"], p["frac"]), "theta", TypeError),
                            (lambda: floxels.vox_sample(th[..., :2], p["cell"], p["frac"]), "theta", ValueError),
                            (lambda: floxels.vox_sample(th[:, :1], p["cell"], p["frac"]), "theta", ValueError),
                            (lambda: floxels.vox_sample(th, p["cell"].long(), p["frac"]), "cell", ValueError),
                            (lambda: floxels.vox_sample(th, p["cell"][:1], p["frac"]), "cell", ValueError),
                            (lambda: floxels.vox_sample(th, p["cell"], p["frac"][:, :7]), "frac", ValueError),
                            (lambda: floxels.vox_sample(th, p["cell"], p["frac"].cpu()), "frac", TypeError),
                            (lambda: sc(dF=x.cpu()), "dF", TypeError), (lambda: sc(dF=x.double()), "dF", ValueError),
                            (lambda: sc(frac=p["frac"][:1]), "frac", ValueError), (lambda: sc(idx=p["idx_sorted"][:15]), "idx_sorted", ValueError),
                            (lambda: sc(idx=p["idx_sorted"].long()), "idx_sorted", ValueError), (lambda: sc(rng=p["cell_rng"][:15]), "cell_rng", ValueError),
                            (lambda: sc(dims=(3, 3)), "dims", ValueError), (lambda: sc(dims=(3, 3, 4)), "cell_rng", ValueError),
                            (lambda: floxels.vox_smooth(th, p["active"].int()), "active", ValueError),
                            (lambda: floxels.vox_smooth(th, p["active"][:, :26]), "active", ValueError),
                            (lambda: floxels.vox_smooth(th.double(), p["active"]), "theta", ValueError),
                            (lambda: opt(x, cnt, x[:1], cnt, grid_range=RANGE), "pc1", ValueError),
                            (lambda: opt(x, cnt, x, cnt.long(), grid_range=RANGE), "count1", ValueError),
                            (lambda: opt(x, cnt, x, cnt, grid_range=RANGE, cell=0.3), "trunc", ValueError),
                            (lambda: opt(x, cnt, x, cnt, grid_range=RANGE[:4]), "grid_range", ValueError),
                            (lambda: opt(x, cnt, x, cnt, grid_range=RANGE, init=torch.zeros(9, 33, 33)), "init", ValueError),
                            (lambda: opt(x, cnt, x, cnt, grid_range=RANGE, voxel=-0.4), "voxel", ValueError),
                            (lambda: opt(x, cnt, x, cnt, grid_range=RANGE, smooth_weight=-1.0), "smooth_weight", ValueError),
                            (lambda: opt(x, cnt, x, cnt, grid_range=RANGE, depth=2), "depth", ValueError),
                            (lambda: opt(x, cnt, x, cnt, grid_range=RANGE, seed=1), "seed", ValueError)):
        with pytest.raises(exc, match=what):
            call()
    # the C entries return their codes without launching
    lib = load()
    SHAPE, ALIGN, ARG = -1, -2, -3
    a, q, h = 0x10000, 0x10004, 0x10002
    nan, inf = float("nan"), float("inf")
    plan = lambda x=a, count=a, B=1, N=8, o=(0.0, 0.0, 0.0), voxel=0.5, V=(3, 3, 3), cell=a, frac=a, idx=a, rng=a, active=a, pairs=a, ws=a: \
        lib.df_vox_plan(x, count, B, N, o[0], o[1], o[2], voxel, V[0], V[1], V[2], cell, frac, idx, rng, active, pairs, ws, None)
    sample = lambda theta=a, cell=a, frac=a, B=1, N=8, V=(3, 3, 3), F=a: lib.df_vox_sample(theta, cell, frac, B, N, V[0], V[1], V[2], F, None)
    scatter = lambda dF=a, frac=a, idx=a, rng=a, B=1, N=8, V=(3, 3, 3), dth=a: lib.df_vox_scatter(dF, frac, idx, rng, B, N, V[0], V[1], V[2], dth, None)
    smooth = lambda theta=a, active=a, B=1, V=(3, 3, 3), v=a, g=a: lib.df_vox_smooth(theta, active, B, V[0], V[1], V[2], v, g, None)
    big_n = dict(B=1, N=(1 << 31) // 3 + 1)                     # 3 B N >= 2^31
    big_v = dict(B=8, V=(1024, 1024, 128))                      # 3 B NV >= 2^31
    big_c = dict(B=17, V=(513, 513, 513))                       # B NC >= 2^31 (3 B NV too)
    for f in (plan, sample, scatter):
        assert f(B=0) == SHAPE and f(B=65536) == SHAPE and f(N=0) == SHAPE and f(**big_n) == SHAPE, f
    for f in (plan, sample, scatter, smooth):
        assert f(B=0) == SHAPE and f(B=65536) == SHAPE and f(**big_v) == SHAPE and f(**big_c) == SHAPE, f
        for V in ((1, 3, 3), (3, 1, 3), (3, 3, 1), (3, 3, -2)):
            assert f(V=V) == SHAPE, (f, V)
    assert lib.df_vox_plan_ws_bytes(1, 8, 3, 3, 3) >= 32 and lib.df_vox_plan_ws_bytes(0, 8, 3, 3, 3) == -1 and lib.df_vox_plan_ws_bytes(1, 8, 3, 1, 3) == -1
    for k in ("x", "count", "cell", "frac", "idx", "rng", "active", "pairs", "ws"):
        assert plan(**{k: None}) == ARG, k
    assert plan(voxel=0.0) == ARG and plan(voxel=-0.5) == ARG and plan(voxel=inf) == ARG and plan(voxel=nan) == ARG
    assert plan(o=(nan, 0.0, 0.0)) == ARG and plan(o=(0.0, nan, 0.0)) == ARG and plan(o=(0.0, 0.0, nan)) == ARG
    assert plan(ws=q) == ALIGN and plan(x=h) == ALIGN and plan(count=h) == ALIGN and plan(cell=h) == ALIGN and plan(frac=h) == ALIGN
    assert plan(idx=h) == ALIGN and plan(rng=h) == ALIGN and plan(pairs=h) == ALIGN
    for k in ("theta", "cell", "frac", "F"):
        assert sample(**{k: None}) == ARG and sample(**{k: h}) == ALIGN, k
    for k in ("dF", "frac", "idx", "rng", "dth"):
        assert scatter(**{k: None}) == ARG and scatter(**{k: h}) == ALIGN, k
    for k in ("theta", "active", "v", "g"):
        assert smooth(**{k: None}) == ARG, k
    assert smooth(theta=h) == ALIGN and smooth(v=h) == ALIGN and smooth(g=h) == ALIGN
    torch.cuda.synchronize()


# ---- 5. one iteration -----------------------------------------------------------------------------------------------------------------
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


def _smooth_init(dims, origin, voxel, seed=11, amp=0.12):
    """a smooth random field [VZ,VY,VX,3]: per component three sine waves of random direction, wavelength of a few metres"""
    VX, VY, VZ = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(VZ), np.arange(VY), np.arange(VX), indexing="ij")
    pos = np.stack([x, y, z], axis=-1) * voxel + np.array(origin)
    out = np.zeros((VZ, VY, VX, 3))
    for c in range(3):
        for _ in range(3):
            k = rng.normal(size=3) * np.array([1.2, 1.2, 2.0])
            out[..., c] += amp * np.sin(pos @ k + rng.uniform(0, 2 * np.pi))
    return torch.from_numpy(out.astype(np.float32))


def test_one_iteration_against_float64():
    """The case of section 6l(4): iters = 1, B = 2 (210 + 150 rows), the defaults' grids over +-6.4 / +-1.6 m, from a smooth random init
    chosen on the CPU so that, by the float64 helper, both terms are at least 1e-3 of the loss and both parts of d theta at least 1e-3 of
    the whole (asserted; they are 0.32 + 0.16 and 0.34 + 0.16, and 0.027 / 0.027 of 0.034 and 0.046).  Loss, last_terms, F, the gradient
    and the field after the Adam step against the float64 helper fed the op's own lookup cells."""
    from deflow_amd import floxels
    D = floxels.DEFAULTS
    cell, voxel, w = dr.f32(D["cell"]), dr.f32(D["voxel"]), D["smooth_weight"]
    samples = [nr.planted_blobs(2, blobs=3, per_blob=70, spacing=2.5, size=(1.2, 0.8, 0.6))[:2],
               nr.planted_blobs(7, blobs=3, per_blob=50, spacing=2.5, size=(1.2, 0.8, 0.6))[:2]]
    origin, dims, R = dr.grid(RANGE, D["cell"], D["trunc"])
    vo, vd = vr.grid(RANGE, D["voxel"])
    init = _smooth_init(vd, vo, D["voxel"])
    pc0s, c0, pc1, c1 = _pad_pair(samples)
    flow, info = floxels.floxels_optimize(pc0s, c0, pc1, c1, grid_range=RANGE, init=init, iters=1)
    torch.cuda.synchronize()
    nv = vd[0] * vd[1] * vd[2]
    assert info["iters_run"] == 1 and info["loss_history"].shape == (1, 2) and info["theta"].shape == (2, vd[2], vd[1], vd[0], 3)
    assert info["last_terms"].shape == (2, 2) and info["grads"].shape == (2, nv, 3) and info["n_pairs"].shape == (2,)
    for b, (P0, P1) in enumerate(samples):
        P0t, n0 = torch.from_numpy(P0), len(P0)
        pl = vr.plan(P0, n0, vo, voxel, vd)
        act, M = vr.active_nodes(pl[0], vd)
        a = torch.from_numpy(act.reshape(-1))
        assert M == int(info["n_pairs"][b]) and torch.equal(info["plan"]["active"][b].cpu().bool(), a)
        assert torch.equal(info["plan"]["cell"][b, :n0].cpu().long(), torch.from_numpy(pl[0])) and bool((info["plan"]["cell"][b, n0:] == -1).all())
        dt2 = dr.edt_dt2(dr.occupancy(P1, origin, cell, dims), R)
        cells = info["cells"][b].cpu().long()
        res = {}
        for dt in (torch.float64, torch.float32):
            th = init.to(dt)
            loss, terms, F, dth, parts, _, W = vr.iteration(P0t.to(dt), dt2, origin, cell, R, th, pl, act, M, w, cells=cells[:n0])
            z = torch.zeros_like(th)
            res[dt] = (loss.reshape(1), torch.stack(terms), F, dth.reshape(nv, 3), nr.adam_step(th, dth, z, z, 1, D["lr"])[0], W, parts)
        r64, r32 = res[torch.float64], res[torch.float32]
        # well-posed, on the input: both terms and both parts of the gradient matter, the warped rows stay inside the range
        data, sm = float(r64[1][0]), w * float(r64[1][1])
        gd, gs, gall = float(r64[6][0].abs().max()), float(r64[6][1].abs().max()), float(r64[3].abs().max())
        print(b, "data", data, "smooth_weight x smooth", sm, "max |d data|", gd, "max |d smooth|", gs, "max |d theta|", gall, "M", M)
        assert min(data, sm) >= 1e-3 * (data + sm) and min(gd, gs) >= 1e-3 * gall and gall > 1e-3
        lo, hi = torch.tensor(RANGE[:3], dtype=torch.float64), torch.tensor(RANGE[3:], dtype=torch.float64)
        assert bool(((r64[5] > lo) & (r64[5] < hi)).all())
        _close(info["loss_history"][0, b].reshape(1), r64[0], r32[0], f"loss[{b}]")
        _close(info["best_loss"][b].reshape(1), r64[0], r32[0], f"best_loss[{b}]")
        _close(info["last_terms"][b], r64[1], r32[1], f"last_terms[{b}]")
        assert abs(float(info["last_terms"][b, 0] + w * info["last_terms"][b, 1]) - float(info["loss_history"][0, b])) <= 1e-6 * float(r64[0])
        _close(flow[b, :n0], r64[2], r32[2], f"flow[{b}] (the start's F: the only iterate)")
        assert not flow[b, n0:].any()
        _close(info["grads"][b], r64[3], r32[3], f"dtheta[{b}]")
        _close(info["theta"][b], r64[4], r32[4], f"theta after the step [{b}]")
        assert not info["grads"][b].cpu()[~a].any(), "inactive nodes get exactly 0"
        assert torch.equal(_bits(info["theta"][b].reshape(nv, 3).cpu()[~a]), _bits(init.reshape(nv, 3)[~a])), "and Adam leaves them where they were"


# ---- 6. loop logic --------------------------------------------------------------------------------------------------------------------
def _loop_case():
    """the case of section 6l(5)"""
    samples = [nr.planted_blobs(2, blobs=3, per_blob=40, spacing=2.5, size=(1.2, 0.8, 0.6))[:2],
               nr.planted_blobs(3, blobs=2, per_blob=50, spacing=2.5, size=(1.2, 0.8, 0.6))[:2]]
    return _pad_pair(samples), dict(grid_range=RANGE, iters=40, patience=4, min_delta=3e-3)


def test_loop_logic_is_exact():
    """as section 6l(5), at this model's defaults: snapshot / freeze replayed from the op's own history of the TOTAL loss; check_every
    and the graph change no bit; a sample alone equals itself inside the batch"""
    from deflow_amd import floxels
    (pc0s, c0, pc1, c1), kw = _loop_case()
    flow, info = floxels.floxels_optimize(pc0s, c0, pc1, c1, check_every=0, **kw)
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
    assert float(info["last_terms"][:, 1].min()) > 0, "the history is the total loss: the smoothness term is in it"
    for b in range(2):
        f2, i2 = floxels.floxels_optimize(pc0s, c0, pc1, c1, check_every=0, **dict(kw, iters=args[b] + 1))
        assert torch.equal(_bits(f2[b]), _bits(flow[b])), "the flow is the best iterate's"
        assert torch.equal(_bits(i2["loss_history"][:, b]), _bits(info["loss_history"][:args[b] + 1, b]))
    f1, i1 = floxels.floxels_optimize(pc0s[1:], c0[1:], pc1[1:], c1[1:], check_every=0, **kw)
    assert torch.equal(_bits(f1[0]), _bits(flow[1])) and torch.equal(_bits(i1["loss_history"][:, 0]), _bits(info["loss_history"][:, 1]))
    assert torch.equal(_bits(i1["theta"][0]), _bits(info["theta"][1])) and int(i1["n_pairs"][0]) == int(info["n_pairs"][1])
    for other in (dict(check_every=5), dict(check_every=0, graph=True), dict(check_every=5, graph=True)):
        f3, i3 = floxels.floxels_optimize(pc0s, c0, pc1, c1, **dict(kw, **other))
        assert torch.equal(_bits(f3), _bits(flow)), other
        for k in ("best_loss", "loss_history", "stalled", "last_terms", "theta"):
            if k in ("last_terms", "theta") and i3["iters_run"] < 40:
                continue
            assert torch.equal(_bits(i3[k].float() if k == "stalled" else i3[k]), _bits(info[k].float() if k == "stalled" else info[k])), (other, k)
        assert torch.equal(i3["frozen"], info["frozen"])
        if other.get("check_every") and bool(info["frozen"].all()):
            assert i3["iters_run"] < 40


# ---- 7. planted motion ----------------------------------------------------------------------------------------------------------------
def test_planted_motion():
    """section 6l(6)'s case at the defaults of this model: four rigid blobs of 200 rows (1.2 x 0.8 x 0.6 m, 2.5 m apart), the second sweep
    independently re-sampled and moved by 0.6 m each; 200 iterations, range +-6.4 / +-1.6 m.  Computed on the CPU with the committed
    helper (tests/test_floxels_cpu.py recomputes both): zero-flow EPE 0.600 m, float64 helper 0.0689 m (at most half of the zero-flow
    EPE), float32 helper 0.0689 m (within a factor 1.5 of float64's); both stop early after 183 iterations.  The op's EPE must be at most
    twice the float64 helper's, 0.1378 m, and that is below model=fastnsf's 0.1998 m."""
    from deflow_amd import floxels
    P0, P1, truth = nr.planted_blobs(2, blobs=4, per_blob=200, shift=0.6, spacing=2.5, size=(1.2, 0.8, 0.6))
    ref64, ref32 = 0.06888271436466897, 0.06892478529339785
    assert abs(float(np.linalg.norm(truth, axis=1).mean()) - 0.6) < 1e-6 and ref64 <= 0.6 / 2 and max(ref64, ref32) <= 1.5 * min(ref64, ref32)
    assert 2 * ref64 < 0.1998
    pc0s, c0, pc1, c1 = _pad_pair([(P0, P1)])
    flow, info = floxels.floxels_optimize(pc0s, c0, pc1, c1, grid_range=RANGE, iters=200)
    epe = float(np.linalg.norm(flow[0, :len(P0)].cpu().numpy() - truth, axis=1).mean())
    print("EPE", epe, "best_loss", float(info["best_loss"][0]), "last terms", info["last_terms"][0].tolist(), "iterations", info["iters_run"],
          "helper float64", ref64)
    assert int(info["n_pairs"][0]) == 481 and not flow[0, len(P0):].any()
    assert epe <= 2 * ref64


# ---- 8. through the stack -------------------------------------------------------------------------------------------------------------
def test_floxels_inside_sweepflow_and_metrics():
    from helpers import rigid_ref as rr
    from helpers import sweep_flow_ref as SR
    from deflow_amd import floxels, metrics, sweeps
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
    model = floxels.Floxels(iters=3, cell=0.4, trunc=2.0, check_every=0)
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
        assert int(st["n_pairs"][b]) > 0
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
    from deflow_amd import floxels, save, vis
    from deflow_amd.h5scene import H5File
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "scene_val.h5"), tmp_path / "scene_val.h5")      # never written under tests/golden
    small = ["floxels_cell=0.4", "floxels_trunc=2.0", "floxels_iters=3", "floxels_voxel=0.8"]
    argv = ["model=floxels", f"dataset_path={tmp_path}", *small, "floxels_check_every=0", "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"]
    assert save.main(argv) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert [x["scene"] for x in lines] == ["scene_val"] and lines[0]["sweeps"] >= 2
    path = save.flow_path(str(tmp_path), "scene_val", "floxels")
    assert os.path.basename(path) == "scene_val.floxels.flow.npz"
    got, meta = save.read_flow(path), save.read_meta(path)
    assert meta == {"res_name": "floxels", "checkpoint": None, "model": "floxels", "voxel_size": [0.2, 0.2, 6.0],
                    "point_cloud_range": [-6.4, -6.4, -3.0, 6.4, 6.4, 3.0], "ground_source": "auto", "half": False,
                    "params": dict(floxels.DEFAULTS, iters=3, check_every=0, cell=0.4, trunc=2.0, voxel=0.8),
                    "definition": "DESIGN.md 6f, 6n (UNPINNED)"}
    with H5File(str(tmp_path / "scene_val.h5")) as f:
        ts = sorted(f.keys(), key=int)
        rows = {t: int(f[t]["lidar"].read().shape[0]) for t in ts}
    assert list(got) == ts[:-1]
    for t in ts[:-1]:
        assert got[t][0].dtype == np.float32 and got[t][0].shape == (rows[t], 3) and np.isfinite(got[t][0]).all()
    assert any(got[t][0].any() for t in ts[:-1])
    out_dir = tmp_path / "png"
    assert vis.main([f"dataset_path={tmp_path}", "res_name=floxels", "scenes=scene_val", f"out_dir={out_dir}", "range=6.4", "res=0.2",
                     "panels=est"]) == 0
    line = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")][0]
    assert line["scene"] == "scene_val" and line["images"] >= 2 and len(os.listdir(out_dir / "scene_val")) == line["images"]
    from deflow_amd import eval as ev
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "index_total.pkl"), tmp_path / "index_total.pkl")
    out = ev.main(["model=floxels", f"val_data={tmp_path}", *small, "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"])
    result = json.loads([x for x in capsys.readouterr().out.splitlines() if x.startswith("{")][-1])
    assert result["model"] == "floxels" and result["checkpoint"] is None and "EPE" in result["metrics"] and "leaderboard" in out
