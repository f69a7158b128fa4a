"""GPU: the GRU decoder's row tiles, split-K walks, two-stage column sum and segmented gather backward against float64, on the cases of
tests/helpers/decoder_cases.py (what each case reaches is decided on the CPU by tests/test_decoder_cases_cpu.py).

Everything goes through the decoder's module and engine boundary (ConvGRUDecoder.__call__, .run, .run_backward); nothing inside is
intercepted.  Every test records the df_* entry points it invoked (a recording proxy over _lib.load) and asserts the set it was built
to reach.
"""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import decoder_cases as DC  # noqa: E402
import parity  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = {"lean": {"DF_GRU_LEAN": "1", "DF_GRU_X2": "1"},         # the default: lean kernels, bf16x2 products
         "lean_fp32": {"DF_GRU_LEAN": "1", "DF_GRU_X2": "0"},    # lean kernels, fp32 MFMA
         "full": {"DF_GRU_LEAN": "0", "DF_GRU_X2": "1"}}         # the kernels that save every plane
LEAN_ENTRIES = {"df_gru_lean_fwd", "df_gru_lean_bwd", "df_gru_lean_wgrad", "df_gru_lean_head_wgrad", "df_gru_lean_finalize", "df_gru_xtab",
                "df_gather_bwd_m", "df_colsum_finalize", "df_conv2d_wgrad_reduce"}
FULL_ENTRIES = {"df_gru_decoder_fwd_mp", "df_gru_decoder_bwd_mp", "df_gru_wgrad_mp", "df_gru_head_wgrad", "df_gather_bwd",
                "df_colsum_finalize", "df_conv2d_wgrad_reduce"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the decoder case tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _record(monkeypatch):
    """-> the set that collects every df_* entry point looked up on the library from here on"""
    from deflow_amd import _lib
    lib, seen = _lib.load(), set()

    class Proxy:
        def __getattr__(self, name):
            if name.startswith("df_"):
                seen.add(name)
            return getattr(lib, name)

    proxy = Proxy()
    monkeypatch.setattr(_lib, "load", lambda: proxy)
    return seen


def _head(c, dev):
    from deflow_amd.decoder import ConvGRUDecoder
    m = ConvGRUDecoder(num_iters=c.iters)
    m.load_state_dict(DC.weights())
    return m.to(dev)


def _module_step(c, dev):
    """the module as test_gru_decoder_golden calls it, then backward with the case's cotangent
    -> dict(flow=[...], gbefore, gafter, gw) shaped like DC.reference's"""
    m = _head(c, dev)
    before = c.before.to(dev).requires_grad_(True)
    after = c.after.to(dev).requires_grad_(True)
    flows = m(before, after, c.infos())
    sum((f * ct.to(dev)).sum() for f, ct in zip(flows, c.cot)).backward()
    torch.cuda.synchronize()
    return dict(flow=[f.detach() for f in flows], gbefore=before.grad, gafter=after.grad, gw={k: p.grad for k, p in m.named_parameters()})


def _pairs(c, got, ref):
    """(name, got, reference tensor ...) over flow per non-empty sample, d(before), d(after) and every parameter gradient"""
    for b, n in enumerate(c.counts):
        assert tuple(got["flow"][b].shape) == (n, 3), (b, got["flow"][b].shape)
        if n:
            yield f"flow[{b}]", got["flow"][b], [r["flow"][b] for r in ref]
    yield "d(before)", got["gbefore"], [r["gbefore"] for r in ref]
    yield "d(after)", got["gafter"], [r["gafter"] for r in ref]
    for k, g in got["gw"].items():
        yield "grad " + k, g, [r["gw"][k] for r in ref]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["edges", "walk", "blocks"])
def test_decoder_case_vs_float64(dev, monkeypatch, name, form):
    """flow per sample, d(before), d(after) and every parameter gradient: err(HIP, fp64) <= max(1e-4, 4 x err(oracle fp32, fp64)) in the
    three norms of parity.three_way (floor and factor unchanged); empty samples return [0, 3]"""
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    c = DC.case(name)
    t0 = time.perf_counter()
    r32, r64 = DC.reference(name)
    t1 = time.perf_counter()
    seen = _record(monkeypatch)
    got = _module_step(c, dev)
    t2 = time.perf_counter()
    tag = f"gru_case_{name}_{form}"
    bad, worst = [], 0.0
    for what, g, (w32, w64) in _pairs(c, got, (r32, r64)):
        try:
            worst = max(worst, parity.three_way(tag, what, g, w32, w64))
        except AssertionError as e:      # every tensor's figures are printed and recorded before the test fails
            bad.append(str(e))
    print(f"[decoder cases] {tag}: worst max-norm error vs fp64 {worst:.3e}; reference {t1 - t0:.1f} s, GPU step {t2 - t1:.1f} s; "
          f"entries: {' '.join(sorted(seen))}")
    assert not bad, "\n".join(bad)
    want = set(FULL_ENTRIES if form == "full" else LEAN_ENTRIES)
    if name == "blocks":
        want.add("df_colsum_stage")
    else:
        assert "df_colsum_stage" not in seen
    if form == "lean_fp32":
        assert "df_split_bf16x2_rows" not in seen        # DF_GRU_X2=0 really selected the fp32-MFMA kernels
    assert want <= seen, f"not reached: {sorted(want - seen)}"
    assert not (seen & (LEAN_ENTRIES ^ FULL_ENTRIES)) - want, f"the other form's kernels ran: {sorted(seen)}"


@pytest.mark.parametrize("name", ["edges", "walk"])
def test_decoder_case_bf16_operand_mode(dev, monkeypatch, name):
    """ops.mfma_bf16(True): the rule of test_gru_decoder_bf16_operand_mode -- flow and every gradient within 2e-2 of the largest element
    of the fp32 reference"""
    from deflow_amd import ops
    c = DC.case(name)
    r32, _ = DC.reference(name)
    seen = _record(monkeypatch)
    with ops.mfma_bf16(True):
        got = _module_step(c, dev)
    bad = []
    for what, g, (w32,) in _pairs(c, got, (r32,)):
        e = parity.rel_err(g, w32)
        parity.record(f"gru_case_{name}_bf16", what, err_vs_oracle32=e, bound=2e-2, ok=e <= 2e-2)
        print(f"[parity] gru_case_{name}_bf16 {what}: rel_err={e:.3e} (tol 2e-02)")
        if e > 2e-2:
            bad.append(f"{what}: {e:.3e}")
    assert not bad, bad
    assert {"df_gru_lean_fwd", "df_gru_lean_bwd", "df_gru_lean_wgrad", "df_gru_lean_head_wgrad", "df_gather_bwd"} <= seen, sorted(seen)
    assert "df_split_bf16x2_rows" not in seen and "df_gather_bwd_m" not in seen


# ---- engine level: the segmented gather backward ---------------------------------------------------------------------------------
def _engine(c, dev, both, prefill=None):
    """ConvGRUDecoder.run + .run_backward on whole 64-channel NHWC tensors.  both: d(before) into an image of its own (the 32-lane
    kernel form), else dbefore=None (the trainer's sparse case: the 16-lane form).  prefill = (before image, after image): accumulate
    onto them.  -> (d(before) NHWC or None, d(after) NHWC, dh0 [B,N,128])"""
    from deflow_amd._lib import img
    from deflow_amd.autograd import GradDict
    from deflow_amd.decoder import pack_infos
    m = _head(c, dev)
    bh = c.before.permute(0, 2, 3, 1).contiguous().to(dev)
    ah = c.after.permute(0, 2, 3, 1).contiguous().to(dev)
    ps = pack_infos(c.infos(), c.H, c.W, dev, True)
    flow, sv = m.run(img(bh), img(ah), ps, True)
    dflow = torch.zeros(c.B, c.N, 3, device=dev)
    for b, n in enumerate(c.counts):
        dflow[b, :n] = c.cot[b].to(dev)
    acc = prefill is not None
    db = (prefill[0].to(dev).clone() if acc else torch.empty(c.B, c.H, c.W, 64, device=dev)) if both else None
    da = prefill[1].to(dev).clone() if acc else torch.empty(c.B, c.H, c.W, 64, device=dev)
    dh0 = m.run_backward(dflow, ps, sv, img(db) if both else None, img(da), acc and both, acc, GradDict())
    torch.cuda.synchronize()
    return db, da, dh0.view(c.B, c.N, 128)


def _segsum(c, dh0, lo):
    """CPU: per cell, the rows' channels [lo, lo + 64) of dh0 added in ascending row order in fp32 -> [B,H,W,64]"""
    dh0 = dh0.cpu()
    out = [DC.segsum_ascending(dh0[b, :n, lo:lo + 64].contiguous(), c.cells(b), c.H * c.W) for b, n in enumerate(c.counts)]
    return torch.stack(out).view(c.B, c.H, c.W, 64)


@pytest.mark.parametrize("name", ["edges", "walk"])
def test_gather_backward_forms_bit_exact(dev, monkeypatch, name):
    """the batched gather backward (csrc/decoder_bwd.hip) promises: a cell's rows are added in ascending index order, bit-identically to
    the one-cell kernel.  (a) the 16-lane form (dbefore=None) and the 32-lane form give the module path's images to the bit, and both
    equal the sequential fp32 sum of the returned dh0 rows on the CPU;  (b) accumulate: image = (that sum) + prefill, ONE fp32 add per
    element after the segmented sum, as the kernel orders it -- asserted to the bit, not to 1 ulp;  (c) the maximum df_gather_bwd_m
    leaves on the written tensor equals max |d(after)| exactly."""
    from deflow_amd._lib import ver
    c = DC.case(name)
    seen = _record(monkeypatch)
    mod = _module_step(c, dev)
    mod_a, mod_b = mod["gafter"].permute(0, 2, 3, 1), mod["gbefore"].permute(0, 2, 3, 1)
    # (a) 16-lane form
    seen.clear()
    _, da1, dh1 = _engine(c, dev, both=False)
    assert "df_gather_bwd_m" in seen and "df_gather_bwd" not in seen
    assert torch.equal(da1, mod_a), "d(after): the one-image form differs from the module path"
    sum_a = _segsum(c, dh1, 64)
    assert torch.equal(da1.cpu(), sum_a), "d(after) is not the ascending-order fp32 sum of the dh0 rows"
    # (c) the measured maximum, both forms
    rec = getattr(da1, "_df_amax", None)       # the record the kernel's caller leaves on the tensor it wrote
    assert rec is not None and rec[1] == ver(da1)
    assert float(rec[0]) == float(da1.abs().max()) > 0
    # (a) 32-lane form
    db2, da2, dh2 = _engine(c, dev, both=True)
    assert all(torch.equal(dh2[b, :n], dh1[b, :n]) for b, n in enumerate(c.counts))
    assert torch.equal(da2, mod_a) and torch.equal(db2, mod_b)
    sum_b = _segsum(c, dh2, 0)
    assert torch.equal(db2.cpu(), sum_b), "d(before) is not the ascending-order fp32 sum of the dh0 rows"
    assert torch.equal(da2.cpu(), sum_a)
    rec = getattr(da2, "_df_amax", None)
    assert rec is not None and float(rec[0]) == float(da2.abs().max())
    # (b) accumulate onto random images, both forms (df_gather_bwd: the measuring entry does not accumulate)
    g = torch.Generator().manual_seed(7)
    pre_b, pre_a = torch.randn(c.B, c.H, c.W, 64, generator=g), torch.randn(c.B, c.H, c.W, 64, generator=g)
    seen.clear()
    db3, da3, _ = _engine(c, dev, both=True, prefill=(pre_b, pre_a))
    assert "df_gather_bwd" in seen and "df_gather_bwd_m" not in seen
    assert torch.equal(da3.cpu(), sum_a + pre_a) and torch.equal(db3.cpu(), sum_b + pre_b)
    _, da4, _ = _engine(c, dev, both=False, prefill=(pre_b, pre_a))
    assert torch.equal(da4.cpu(), sum_a + pre_a)
    # the heavy cell really took more than one wavefront's worth of rows through the four-cell loop
    b, cell = next(iter(c.heavy.items()))
    assert int((c.cells(b) == cell).sum()) >= 70 and float(da1[b].view(-1, 64)[cell].abs().max()) > 0


def test_walk_under_poisoned_memory(dev, monkeypatch):
    """`walk` leaves most of the 1024 head splits without a stage: their partial tiles (a torch.empty workspace) must be written as
    zeros.  After every free block of the allocator was filled with NaN the gradients are finite and equal the first run's to the bit."""
    c = DC.case("walk")
    seen = _record(monkeypatch)
    g0 = _module_step(c, dev)
    assert "df_gru_lean_head_wgrad" in seen
    torch.cuda.empty_cache()
    junk = torch.full((1 << 28,), float("nan"), device=dev)     # 1 GiB of NaN back into the allocator's free lists ...
    small = [torch.full((1 << 17,), float("nan"), device=dev) for _ in range(64)]     # ... and into its pool of blocks below 1 MB
    del junk, small
    g1 = _module_step(c, dev)
    for what, a, (b,) in _pairs(c, g1, (g0,)):
        assert torch.isfinite(a).all(), f"{what}: a kernel read memory it never wrote"
        assert torch.equal(a, b), f"{what}: not bit-identical after the allocator was poisoned"
