"""GPU: LinearDecoder on the `edges` case of tests/helpers/decoder_cases.py (every row-tile tail, empty first / middle / last samples, a
70-row cell, 943 cells) against the oracle in float64 -- its only other test is one golden shape."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import decoder_cases as DC  # noqa: E402
import parity  # noqa: E402

pytestmark = pytest.mark.gpu


def _weights():
    g = np.load(os.path.join(DC.ROOT, "tests", "golden", "g3_lineardecoder.npz"))
    return {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}


def _oracle(c, double):
    from oracle import ref_torch as O
    m = O.LinearDecoder()
    m.load_state_dict(_weights())
    dt = torch.float64 if double else torch.float32
    m = m.to(dt)
    before, after = c.before.to(dt).clone().requires_grad_(True), c.after.to(dt).clone().requires_grad_(True)
    flows = m(before, after, [{"voxel_coords": vc, "point_offsets": o.to(dt)} for vc, o in zip(c.coords, c.offs)])
    sum((f * ct.to(dt)).sum() for f, ct in zip(flows, c.cot)).backward()
    return [f.detach() for f in flows], before.grad, after.grad, {k: p.grad for k, p in m.named_parameters()}


def test_linear_decoder_edges_vs_float64():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from deflow_amd.decoder import LinearDecoder
    dev = torch.device("cuda")
    c = DC.case("edges")
    f32, gb32, ga32, gw32 = _oracle(c, False)
    f64, gb64, ga64, gw64 = _oracle(c, True)
    m = LinearDecoder()
    m.load_state_dict(_weights())
    m = m.to(dev)
    before, after = c.before.to(dev).requires_grad_(True), c.after.to(dev).requires_grad_(True)
    flows = m(before, after, c.infos())
    sum((f * ct.to(dev)).sum() for f, ct in zip(flows, c.cot)).backward()
    torch.cuda.synchronize()
    bad = []

    def chk(what, got, w32, w64):
        try:
            parity.three_way("linear_case_edges", what, got, w32, w64)
        except AssertionError as e:
            bad.append(str(e))

    for b, n in enumerate(c.counts):
        assert tuple(flows[b].shape) == (n, 3)
        if n:
            chk(f"flow[{b}]", flows[b], f32[b], f64[b])
    chk("d(before)", before.grad, gb32, gb64)
    chk("d(after)", after.grad, ga32, ga64)
    for k, p in m.named_parameters():
        chk("grad " + k, p.grad, gw32[k], gw64[k])
    assert not bad, "\n".join(bad)
