"""GPU: the pillar feature net's backward kernels (pfn_bwd_stats_kernel<MODE>, pfn_bwd_finalize_kernel, pfn_bwd_weights_kernel<MODE>
and the df_colsum_finalize that ends them) against float64 at the cases of tests/helpers/pfn_cases.py, through
DynamicEmbedder.pillarize / pillarize_bwd as deflow_amd/autograd.py calls them.

Per case x mode (avg, max) x train / eval: the canvas and the valid-point counts of the forward, then dW [32,9], dgamma, dbeta under
parity.three_way(floor=2e-5, factor=4) -- the layer census' figure for a BatchNorm backward; tests/test_pfn_cases_cpu.py shows that the
oracle's own fp32 error never lifts it and that the faults these cases were built for breach it.  `pair` runs the trainer's form: the
two clouds' gradients are the 32-channel halves of one [B,H,W,64] buffer whose cells outside the reading cloud hold NaN (one read of a
dead cell would show), the second call accumulating into the first's result; in training mode its result must repeat to the bit.
Every case also checks the accumulate branch alone: grads pre-filled with random values come back as those values plus the
grads=None result, to the fp32 rounding of one addition.

Measured on an MI355X (worst over the 16 parameter sets; max-relative / rms-relative / 1 - cos against float64, bounds 2e-5 / 2e-5 /
4e-10; in brackets the oracle's own fp32 max-relative error in the same run, which depends on the CPU's thread count):
  canvas  4.2e-6 / 1.7e-6 / 1.4e-12  (degenerate, training)   [5.2e-7]
  dW      2.5e-6 / 2.2e-6 / 2.4e-12  (degenerate max train)   [3.7e-6, rect_far avg]
  dgamma  1.9e-6 / 1.3e-6 / 6.9e-13  (degenerate max train)   [7.7e-7]
  dbeta   3.5e-6 / 1.9e-6 / 1.8e-12  (degenerate avg train)   [5.5e-7]
Every other case stays under 1e-6 in all three tensors.  The worst figures are those of the 5000-point cell: the kernels add its points
one after the other in fp32 (pfn_mean, and the 5000 equal terms g / 5000 of a channel's sum), a random walk of about sqrt(5000) 2^-24.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import pfn_cases as PC  # noqa: E402
import parity  # noqa: E402

pytestmark = pytest.mark.gpu
IDS = [f"{n}-{m}-{'train' if t else 'eval'}" for n, m, t in PC.PARAMS]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _three_way(tag, name, got, r32, r64):
    return parity.three_way(tag, name, got, r32, r64, floor=PC.FLOOR, factor=PC.FACTOR)


@pytest.mark.parametrize("name,mode,train", PC.PARAMS, ids=IDS)
def test_pfn_case_vs_float64(dev, name, mode, train):
    from deflow_amd.encoder import DynamicEmbedder
    from deflow_amd._lib import img
    c = PC.case(name, mode, train)
    r32, r64 = PC.reference(name, mode, train)
    H, W = c.dims
    tag = f"pfn_case {name} {mode} {'train' if train else 'eval'}"
    mine = DynamicEmbedder(c.vs, c.dims, c.rng, 32, mode=mode)
    mine.load_state_dict(c.state)
    mine = mine.to(dev).train(train)
    nc = len(c.clouds)
    # forward: one canvas per cloud -- the 32-channel halves of one 64-channel buffer when there are two (deflow.py)
    canvas = torch.full((c.B, H, W, 32 * nc), float("nan"), device=dev)
    # upstream gradient, kept alive to the end (img() holds raw pointers); two clouds: NaN wherever the reading cloud has no pillar
    if nc == 1:
        gbuf = nhwc(c.gout[0]).to(dev)
    else:
        gbuf = torch.full((c.B, H, W, 64), float("nan"))
        for ci in range(nc):
            occ = PC.occupied(c, ci)
            gbuf[..., 32 * ci:32 * ci + 32][occ] = nhwc(c.gout[ci])[occ]
        gbuf = gbuf.to(dev)
    states = []
    with torch.no_grad():
        for ci, pts in enumerate(c.clouds):
            states.append(mine.pillarize(pts.to(dev), img(canvas, 32, 32 * ci), train))
    for ci, st in enumerate(states):
        assert st.counts.cpu().tolist() == [int(vc.shape[0]) for vc in r64["coords"][ci]]
        _three_way(tag, f"canvas{ci}", canvas[..., 32 * ci:32 * ci + 32].permute(0, 3, 1, 2), r32["canvas"][ci], r64["canvas"][ci])

    def backward(first=None):
        g = first
        for ci, st in enumerate(states):
            g = mine.pillarize_bwd(st, img(gbuf, 32, 32 * ci), g)
        return dict(zip(PC.GRADS, g))

    got = backward()
    for k in PC.GRADS:        # every figure before the first assertion
        assert torch.isfinite(got[k]).all(), f"{tag} {k}: non-finite (a read of a dead cell?)"
        print(f"[pfn cases] {tag} {k}: max {parity.rel_err(got[k], r64['grads'][k]):.2e} rms {parity.rms_rel(got[k], r64['grads'][k]):.2e}")
    for k in PC.GRADS:
        _three_way(tag, k, got[k], r32["grads"][k], r64["grads"][k])
    if nc == 2 and train:     # "every sum has one fixed order" (csrc/pillarize.hip)
        again = backward()
        for k in PC.GRADS:
            assert torch.equal(again[k], got[k]), f"{tag} {k}: the repeated backward differs"
    # the accumulate branch alone: the first cloud's call into pre-filled gradients
    base = dict(zip(PC.GRADS, mine.pillarize_bwd(states[0], img(gbuf, 32, 0), None)))
    g = torch.Generator().manual_seed(7)
    fill = {k: (torch.randn(v.shape, generator=g) * 10.0).to(dev) for k, v in base.items()}
    acc = dict(zip(PC.GRADS, mine.pillarize_bwd(states[0], img(gbuf, 32, 0), tuple(fill[k].clone() for k in PC.GRADS))))
    for k in PC.GRADS:
        # acc = fl(fill + S), base = fl(S) with S the kernels' float64 sum: |acc - (fill + base)| <= 2^-24 (|S| + |fill + S|)
        want = fill[k].double() + base[k].double()
        lim = 2.0 ** -24 * (base[k].double().abs() + want.abs()) * 1.0001
        over = ((acc[k].double() - want).abs() - lim).max()
        assert float(over) <= 0.0, f"{tag} {k}: accumulate is off by more than one rounding ({float(over):.3e} over)"
    del gbuf, canvas
