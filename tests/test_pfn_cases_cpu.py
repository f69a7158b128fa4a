"""CPU: the conditions that make tests/test_gpu_pfn_cases.py meaningful, decided without a GPU.

  * the fp32 and the float64 oracle voxelise every case identically (the comparison is between the same pillars), and the float64
    restatement the faults are injected into (pfn_cases.pfn_backward64) equals the float64 oracle's autograd to 1e-12;
  * the oracle's own fp32-vs-float64 error stays under a quarter of the bound in the three norms of parity.py, on the canvas and the
    three parameter gradients, so parity.three_way(floor=2e-5, factor=4) is the 2e-5 floor and nothing wider.  The figure depends on
    how many threads the CPU sums with: worst 1.0e-6 with eight (dW, degenerate max), 3.6e-6 with one (dbeta, degenerate avg: 5000
    equal terms added one after the other), 3.7e-6 seen on a 16-thread host (dW, rect_far avg) -- against the limit of 5e-6;
  * each fault a kernel could plausibly have, injected into the float64 computation, pushes at least one of dW / dgamma / dbeta over
    that bound at the case built for it;
  * the clouds really reach the launch paths they were built for (nbs, a sorted position past 8192, a run across it, an empty sample
    in the middle, the tie pillars of `pair`).

Fault (e), the maximum going to the last attaining point: a tie between different points at the ReLU's zero carries no gradient under
either rule (the ReLU masks it), so it cannot be seen in any gradient; `pair` therefore also has a tie at a POSITIVE value between two
different points (helpers/pfn_cases.py, TIE_CH), where the rule decides which point's features enter dW.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pfn_cases as PC  # noqa: E402
import parity  # noqa: E402

IDS = [f"{n}-{m}-{'train' if t else 'eval'}" for n, m, t in PC.PARAMS]


def _errs(got, want):
    return parity.rel_err(got, want), parity.rms_rel(got, want), parity.one_minus_cos(got, want)


def _bounds(r32, r64):
    """the three bounds parity.three_way(floor=FLOOR, factor=FACTOR) would apply to a tensor"""
    e, r, c = _errs(r32, r64)
    return max(PC.FLOOR, PC.FACTOR * e), max(PC.FLOOR, PC.FACTOR * r), max(PC.FLOOR ** 2, PC.FACTOR ** 2 * c)


def _breach(got, r32, r64):
    """-> (name, norm, error / bound) of the worst violation among dW / dgamma / dbeta, or None"""
    worst = None
    for k in PC.GRADS:
        for norm, e, b in zip(("max", "rms", "1-cos"), _errs(got[k], r64["grads"][k]), _bounds(r32["grads"][k], r64["grads"][k])):
            if e > b and (worst is None or e / b > worst[2]):
                worst = (k, norm, e / b)
    return worst


@pytest.mark.parametrize("name,mode,train", PC.PARAMS, ids=IDS)
def test_same_pillars_and_restatement(name, mode, train):
    c = PC.case(name, mode, train)
    r32, r64 = PC.reference(name, mode, train)
    for ci in range(len(c.clouds)):
        for a, b in zip(r32["coords"][ci], r64["coords"][ci]):
            assert torch.equal(a, b)
    m = PC.pfn_backward64(c)
    for k in PC.GRADS:
        assert parity.rel_err(m[k], r64["grads"][k]) <= 1e-12, k
    assert _breach(m, r32, r64) is None


@pytest.mark.parametrize("name,mode,train", PC.PARAMS, ids=IDS)
def test_oracle_fp32_error_is_a_quarter_of_the_bound(name, mode, train):
    r32, r64 = PC.reference(name, mode, train)
    tens = {k: (r32["grads"][k], r64["grads"][k]) for k in PC.GRADS}
    tens.update({f"canvas{i}": (a, b) for i, (a, b) in enumerate(zip(r32["canvas"], r64["canvas"]))})
    for k, (a, b) in tens.items():
        e, r, c = _errs(a, b)
        print(f"[pfn cases] {name} {mode} train={train} {k}: oracle fp32 vs float64 max {e:.2e} rms {r:.2e} 1-cos {c:.1e}")
        assert e <= PC.FLOOR / 4 and r <= PC.FLOOR / 4 and c <= (PC.FLOOR / 4) ** 2, (k, e, r, c)


def _last_sample(c):
    return max(b for b, vc in enumerate(PC.reference(c.name, c.mode, c.train)[1]["coords"][0]) if vc.shape[0])


def _fault(name, mode, train, fault, **fk):
    c = PC.case(name, mode, train)
    r32, r64 = PC.reference(name, mode, train)
    w = _breach(PC.pfn_backward64(c, fault, **fk), r32, r64)
    print(f"[pfn cases] {name} {mode} train={train} fault {fault} {fk}: {w}")
    assert w is not None, f"{fault} stays inside the bound at {name} {mode}"
    return w


@pytest.mark.parametrize("mode", PC.MODES)
@pytest.mark.parametrize("name", PC.NAMES)
def test_fault_a_last_pillar_of_a_sample_dropped(name, mode):
    """the last pillar of the last non-empty sample (degenerate: one of the two points of sample 3)"""
    _fault(name, mode, True, "drop_last_pillar", sample=_last_sample(PC.case(name, mode, True)))


@pytest.mark.parametrize("mode", PC.MODES)
def test_fault_b_one_block_of_the_second_pass_dropped(mode):
    _fault("stride", mode, True, "drop_block", sample=0, start=8192)


@pytest.mark.parametrize("mode", PC.MODES)
def test_fault_c_coefficients_of_the_previous_sample(mode):
    _fault("degenerate", mode, True, "coef_prev")


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("mode", PC.MODES)
def test_fault_d_second_cloud_overwrites(mode, train):
    _fault("pair", mode, train, "overwrite")


@pytest.mark.parametrize("train", [True, False])
def test_fault_e_max_goes_to_the_last_attaining_point(train):
    _fault("pair", "max", train, "last_max")


@pytest.mark.parametrize("mode", PC.MODES)
def test_fault_f_centre_with_gx_and_gy_swapped(mode):
    _fault("rect_far", mode, True, "swap_gxgy")


@pytest.mark.parametrize("name,sample,pillar_len", [("tiny", 0, 3), ("stride", 0, 5), ("degenerate", 0, 5000), ("pair", 0, 5)])
def test_fault_g_mean_without_its_division(name, sample, pillar_len):
    """for the first pillar of at least `pillar_len` points (tiny: the three-point pillar; degenerate: the 5000-point cell)"""
    c = PC.case(name, "avg", True)
    _, cell = PC.sorted_sample(c, 0, sample)
    n = torch.unique_consecutive(cell, return_counts=True)[1]
    k = int((n >= pillar_len).nonzero()[0])
    _fault(name, "avg", True, "no_inv", sample=sample, pillar=k)


# ---- the clouds reach what they were built for --------------------------------------------------------------------------------------
def _counts(c, cloud=0):
    return [int(vc.shape[0]) for vc in PC.reference(c.name, c.mode, c.train)[1]["coords"][cloud]]


def test_structure_tiny():
    c = PC.case("tiny", "avg", True)
    assert c.nbs == 1 and (c.B, c.N) == (2, 20) and min(_counts(c)) >= 2


def test_structure_stride():
    c = PC.case("stride", "avg", True)
    assert c.nbs == 256 > 32 and (c.B, c.N) == (3, 9000)
    cnt = _counts(c)
    assert cnt[0] >= 8192 + 32 and min(cnt) > 256 * 32, cnt         # a whole block of the second pass in sample 0
    _, cell = PC.sorted_sample(c, 0, 0)
    heads0 = (cell[8192:8224] != cell[8191:8223]).sum()
    assert int(heads0) >= 16                                        # fault (b) drops that many pillars
    _, cell = PC.sorted_sample(c, 0, 1)
    uc, n = torch.unique_consecutive(cell, return_counts=True)
    start = torch.cumsum(n, 0) - n
    k = int(((start < 8192) & (start + n > 8192)).nonzero()[0])
    assert int(n[k]) >= PC.STRADDLE and int(start[k]) <= 8192 - 8 and int(start[k] + n[k]) >= 8192 + 8, (int(start[k]), int(n[k]))


@pytest.mark.parametrize("train", [True, False])
def test_structure_degenerate(train):
    c = PC.case("degenerate", "avg", train)
    assert _counts(c) == [5600, 3000, 0, 2 if train else 1]
    _, cell = PC.sorted_sample(c, 0, 0)
    assert int(torch.unique_consecutive(cell, return_counts=True)[1].max()) >= 5000
    _, cell = PC.sorted_sample(c, 0, 1)
    assert int(cell.min() // 64) == int(cell.max() // 64)           # one row of cells


def test_structure_rect_far():
    c = PC.case("rect_far", "avg", True)
    H, W = c.dims
    assert (H, W) == (40, 72) and W & (W - 1) != 0 and (c.B, c.N) == (3, 5000)
    pts = c.clouds[0]
    assert float(pts[~pts.isnan()].abs().max()) > 51.0
    vc = torch.cat(PC.reference("rect_far", "avg", True)[1]["coords"][0])
    assert int(vc[:, 1].max()) == H - 1 and int(vc[:, 2].max()) == W - 1 and int(vc[:, 1:].min()) == 0


@pytest.mark.parametrize("train", [True, False])
def test_structure_pair(train):
    """the duplicates and the two tie pillars of cloud 0 are what the module docstring of pfn_cases says"""
    from oracle import ref_torch as O
    c = PC.case("pair", "max", train)
    assert len(c.clouds) == 2 and (c.B, c.N) == (2, 700) and not torch.equal(c.clouds[0], c.clouds[1])
    m = PC.oracle(c, double=True)
    a = c.clouds[0]
    # (i) three exact copies and one different point, alone in their pillar
    b, d0, other = PC.DUP_POINTS
    assert torch.equal(a[b, d0], a[b, d0 + 1]) and torch.equal(a[b, d0], a[b, d0 + 2]) and not torch.equal(a[b, d0], a[b, other])
    info = m.voxelizer(a[b:b + 1])[0]
    row = {int(i): k for k, i in enumerate(info["point_idxes"])}
    same = (info["voxel_coords"] == info["voxel_coords"][row[d0]]).all(1)
    assert int(same.sum()) == 4 and all(bool(same[row[i]]) for i in (d0, d0 + 1, d0 + 2, other))
    # (ii) two different points of one pillar: equal and positive in TIE_CH, zero in some channels for both, positive elsewhere
    b, p, q = PC.TIE_POINTS
    info = m.voxelizer(a[b:b + 1])[0]
    row = {int(i): k for k, i in enumerate(info["point_idxes"])}
    same = (info["voxel_coords"] == info["voxel_coords"][row[p]]).all(1)
    assert int(same.sum()) == 2 and bool(same[row[q]]) and not torch.equal(a[b, p], a[b, q])
    assert tuple(info["voxel_coords"][row[p]][1:].tolist()) == PC.TIE_CELL
    assert float(c.gout[0][b, PC.TIE_CH, PC.TIE_CELL[0], PC.TIE_CELL[1]]) == PC.TIE_GRAD
    for mod in (m, PC.oracle(c, double=False)):
        dt = next(mod.parameters()).dtype
        fn = mod.feature_net
        pts, coors = info["points"].to(dt), info["voxel_coords"]
        # the per-point features (the module's forward up to the scatter)
        vm, _, inv = O._scatter_mean(pts, coors)
        ctr = torch.stack([coors[:, 2].to(dt) * fn.vx + fn.x_offset, coors[:, 1].to(dt) * fn.vy + fn.y_offset,
                           coors[:, 0].to(dt) * fn.vz + fn.z_offset], 1)
        with torch.no_grad():
            y = fn.pfn_layers[0](torch.cat([pts, pts - vm[inv], pts - ctr], 1))
        yp, yq = y[row[p]], y[row[q]]
        assert float(yp[PC.TIE_CH]) == float(yq[PC.TIE_CH]) > 0.0
        both_zero = (yp == 0) & (yq == 0)
        assert int(both_zero.sum()) >= 1 and int(((yp > 0) & (yq > 0)).sum()) >= 2
        pos = (yp > 0) & (yq > 0)
        assert int(((yp != yq) & pos).sum()) == int(pos.sum()) - 1      # different points: every other live channel differs
