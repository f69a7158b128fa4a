"""GPU: the GRU decoder's bf16 forms against float64 AT THEIR OWN ROUNDING, on the `edges` and `walk` cases of
tests/helpers/decoder_cases.py (plus `edges` with one iteration: the first iteration is the last, and the q GEMM prefetches W_1
instead of W_z).

The reference is tests/helpers/decoder_bf16_ref.py: the decoder restated in float64 with every operand rounded to bfloat16 where the
kernel rounds it (its docstring is the list under test; tests/test_decoder_bf16_ref_cpu.py proves it against the oracle and shows
that each misplaced rounding fails the bound used here).  The bound is parity.three_way with floor and factor untouched,

    err(HIP, emulation float64)  <=  max(1e-4, 4 x err(emulation fp32, emulation float64))      in max, rms and 1 - cos,

the fp32 emulation measuring how strongly these inputs amplify fp32 noise into bf16 rounding flips.  A flip is a per-row event, so
the norms run over the case's flows concatenated to [sum n, 3], over d(before) and d(after) whole, and per parameter gradient; the 2e-2
tests (test_gru_decoder_bf16_operand_mode, test_decoder_case_bf16_operand_mode) stay beside these, and the full form's bf16 BACKWARD
(csrc/decoder3_bwd.hip, DF_GRU_LEAN=0 under bf16) remains on them alone.

Every test records the df_* entry points it reached (the proxy of tests/test_gpu_decoder_cases.py) and asserts the set.
"""
import dataclasses
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import decoder_bf16_ref as E  # noqa: E402
import decoder_cases as DC  # noqa: E402
import parity  # noqa: E402
from test_gpu_decoder_cases import FULL_ENTRIES, LEAN_ENTRIES, _head, _module_step, _record  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEAN_BF16 = {"df_gru_lean_fwd", "df_gru_lean_bwd", "df_gru_lean_wgrad", "df_gru_lean_head_wgrad", "df_gru_lean_finalize", "df_gru_xtab",
             "df_gather_bwd", "df_colsum_finalize", "df_conv2d_wgrad_reduce"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the decoder bf16 case tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _case(tag):
    """-> (Case, name of the decoder case, iteration override): `edges_t1` is `edges` run for one iteration"""
    if tag == "edges_t1":
        return dataclasses.replace(DC.case("edges"), name="edges_t1", iters=1), "edges", 1
    return DC.case(tag), tag, None


def _gru(seen):
    return {e for e in seen if e.startswith("df_gru_")}


def _check(tag, c, got, refs):
    """three_way per tensor of E.pairs; every tensor's figures are printed and recorded before the test fails, then per-sample figures
    of the flow.  -> {tensor: max-norm error vs the float64 emulation}"""
    for b, n in enumerate(c.counts):
        assert tuple(got["flow"][b].shape) == (n, 3), (b, got["flow"][b].shape)
    bad, errs = [], {}
    for what, g, (a32, a64) in E.pairs(got, refs):
        try:
            errs[what] = parity.three_way(tag, what, g, a32, a64)
        except AssertionError as e:
            bad.append(str(e))
    if bad:
        for b, n in enumerate(c.counts):
            if n:
                f, a32, a64 = got["flow"][b], refs[0]["flow"][b], refs[1]["flow"][b]
                print(f"[decoder bf16] {tag} flow[{b}] ({n} rows): HIP max {parity.rel_err(f, a64):.2e} rms {parity.rms_rel(f, a64):.2e} | "
                      f"emulation fp32 max {parity.rel_err(a32, a64):.2e} rms {parity.rms_rel(a32, a64):.2e}")
    assert not bad, "\n".join(bad)
    print(f"[decoder bf16] {tag}: worst max-norm error vs the float64 emulation {max(errs.values()):.3e} ({max(errs, key=errs.get)}), "
          f"flow {errs['flow']:.3e}")
    return errs


def _nhwc(c, dev):
    return c.before.permute(0, 2, 3, 1).contiguous().to(dev), c.after.permute(0, 2, 3, 1).contiguous().to(dev)


@pytest.mark.parametrize("tag", ["edges", "walk", "edges_t1"])
def test_inference_kernel_vs_float64(dev, monkeypatch, tag):
    """df_gru_decoder_fwd_bf16 alone, through ConvGRUDecoder.run_bf16 at the engine boundary (NHWC images).  Measured on an MI355X,
    flow, max / rms / 1 - cos against the float64 emulation (in brackets the fp32 emulation's own max / rms; the rms bound is 1e-4):
        edges     3.11e-4 / 2.53e-5 / 3.2e-10   (3.11e-4 / 2.34e-5)
        walk      3.12e-4 / 1.69e-5 / 1.4e-10   (6.19e-4 / 1.70e-5)
        edges_t1  4.65e-4 / 3.54e-5 / 6.3e-10   (2.78e-4 / 2.24e-5)
    (rows gru_bf16_inference_* of the parity report)"""
    from deflow_amd._lib import img
    from deflow_amd.decoder import pack_infos
    c, name, it = _case(tag)
    t0 = time.perf_counter()
    refs = E.reference(name, "inference", iters=it)
    t1 = time.perf_counter()
    m = _head(c, dev)
    bh, ah = _nhwc(c, dev)
    ps = pack_infos(c.infos(), c.H, c.W, dev, False)
    seen = _record(monkeypatch)
    flow, _ = m.run_bf16(img(bh), img(ah), ps)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    got = dict(flow=[flow[b, :n] for b, n in enumerate(c.counts)])
    _check(f"gru_bf16_inference_{tag}", c, got, refs)
    print(f"[decoder bf16] inference {tag}: reference {t1 - t0:.1f} s, GPU {t2 - t1:.1f} s; entries: {' '.join(sorted(seen))}")
    assert _gru(seen) == {"df_gru_decoder_fwd_bf16"}, sorted(seen)


@pytest.mark.parametrize("name", ["edges", "walk"])
@pytest.mark.parametrize("form", ["lean"])
def test_bf16_mode_step_vs_float64(dev, monkeypatch, form, name):
    """ops.mfma_bf16(True), the mode Trainer(dtype="bf16") runs the decoder in (mfma_bf16 = 2): flow, d(before), d(after) and every
    parameter gradient of the module step against the `lean` emulation and its manual backward.  Measured on an MI355X, max / rms
    against the float64 emulation (in brackets the fp32 emulation's own):
        edges  flow 1.99e-4 / 1.39e-5 (1.56e-4 / 1.37e-5)   d(before) 7.7e-5 / 3.5e-5 (1.1e-4 / 5.8e-5)   d(after) 7.0e-5 / 3.9e-5 (1.4e-4 / 7.3e-5)
               worst gradient: gru.convr.weight 2.67e-4 / 1.05e-4 (1.17e-4 / 1.14e-4; bounds 4.7e-4 / 4.5e-4)
        walk   flow 4.16e-4 / 1.63e-5 (4.18e-4 / 1.53e-5)   d(before) 3.0e-4 / 9.2e-5 (1.6e-4 / 5.6e-5)   d(after) 3.8e-4 / 8.8e-5 (2.5e-4 / 6.0e-5)
               worst gradient: gru.convr.weight 1.86e-4 / 1.88e-4 (1.63e-4 / 1.23e-4; bounds 6.5e-4 / 4.9e-4)
    Every tensor's rms error is within 2 x the fp32 emulation's; no tensor needed the kernels' gate formulas in the companion."""
    from deflow_amd import ops
    monkeypatch.setenv("DF_GRU_LEAN", "1")
    c = DC.case(name)
    t0 = time.perf_counter()
    refs = E.reference(name, "lean", backward=True)
    t1 = time.perf_counter()
    seen = _record(monkeypatch)
    with ops.mfma_bf16(True):
        got = _module_step(c, dev)
    t2 = time.perf_counter()
    _check(f"gru_bf16_step_{name}_{form}", c, got, refs)
    print(f"[decoder bf16] step {name}: reference {t1 - t0:.1f} s, GPU step {t2 - t1:.1f} s; entries: {' '.join(sorted(seen))}")
    assert LEAN_BF16 <= seen, f"not reached: {sorted(LEAN_BF16 - seen)}"
    assert "df_split_bf16x2_rows" not in seen and "df_gather_bwd_m" not in seen
    assert not seen & (FULL_ENTRIES - LEAN_ENTRIES - {"df_gather_bwd"}), f"the full form's kernels ran: {sorted(seen)}"


@pytest.mark.parametrize("tag", ["edges", "walk", "edges_t1"])
@pytest.mark.parametrize("form", ["full"])
def test_bf16_mode_forward_vs_float64(dev, monkeypatch, form, tag):
    """DF_GRU_LEAN=0 under ops.mfma_bf16(True): the full form's forward (gru_fwd3_kernel<.., BF, W16>), flow only, in both of its
    instantiations -- the one that saves the planes (a forward that will be differentiated) and the one that does not (no_grad); the
    two must agree to the bit.  Measured on an MI355X: the figures of test_inference_kernel_vs_float64 to the printed digit (edges
    3.11e-4 / 2.53e-5, walk 3.12e-4 / 1.69e-5, edges_t1 4.65e-4 / 3.54e-5): the two kernels round the same values"""
    from deflow_amd import ops
    monkeypatch.setenv("DF_GRU_LEAN", "0")
    c, name, it = _case(tag)
    refs = E.reference(name, "full", iters=it)
    seen = _record(monkeypatch)
    m = _head(c, dev)
    with ops.mfma_bf16(True):
        saving = m(c.before.to(dev).requires_grad_(True), c.after.to(dev).requires_grad_(True), c.infos())
        with torch.no_grad():
            plain = m(c.before.to(dev), c.after.to(dev), c.infos())
    torch.cuda.synchronize()
    got = dict(flow=[f.detach() for f in saving])
    _check(f"gru_bf16_fwd_{tag}_{form}", c, got, refs)
    assert all(torch.equal(a.detach(), b) for a, b in zip(saving, plain)), "the saving and the plain forward differ"
    assert _gru(seen) == {"df_gru_decoder_fwd_mp"}, sorted(seen)


def _rows(t, c, width):
    """[B * N, width] padded rows -> the valid rows of every sample, concatenated"""
    t = t.view(c.B, c.N, width)
    return torch.cat([t[b, :n] for b, n in enumerate(c.counts)])


def test_mode1_equals_mode2(dev, monkeypatch):
    """mfma_bf16 = 1 (fp32 weights, rounded in the kernel) has no Python caller: df_gru_lean_fwd and df_gru_lean_bwd called directly on
    `edges`, with the fp32 weights and transposes of the module's own helpers (_weights, _weights_bwd(False, False)).

    Mode 1 and mode 2 round the same values with the same RNE cast (gemm_dma.h pack_bf16 / torch's .to(bfloat16)) but do NOT feed the
    same MFMA sequence: in mode 1 lane group lq of a 32-deep chunk holds k = 4 lq .. 4 lq + 3 and 16 + 4 lq .. 16 + 4 lq + 3 (a_lane =
    row + 4 lq, second group at +16; the B fragment from the swizzled slots lq and 4 + lq of the fp32 tile), in mode 2 it holds
    k = 8 lq .. 8 lq + 7 (a_lane = row + 8 lq, second group at +4; one b128 of the bf16 tile).  The 32 products of one
    v_mfma_f32_16x16x32_bf16 are the same set in another order of k slots, so bit-identity is not promised by the code; mode 1 is
    therefore held to the float64 bound of mode 2 (flow, h_T, dh0, dpre1 against the `lean` emulation), and whether the two modes came
    out identical is printed and recorded, not asserted.  Measured on an MI355X: NOT identical, forward or backward; max / rms against the
    float64 emulation, mode 1 | mode 2 (fp32 emulation): flow 1.99e-4 / 2.03e-5 | 1.99e-4 / 1.39e-5 (1.56e-4 / 1.37e-5), h_T 5.2e-5 /
    4.3e-6 | 2.5e-6 / 2.4e-7 (2.2e-5 / 1.9e-6), dh0 4.2e-4 / 5.1e-5 | 3.5e-4 / 3.8e-5 (6.8e-4 / 6.7e-5), dpre1 6.6e-5 / 9.5e-6 | 6.6e-5 /
    8.1e-6 (4.8e-5 / 5.0e-6)."""
    from deflow_amd._lib import call, img, ptr, stream
    from deflow_amd.decoder import pack_infos
    c = DC.case("edges")
    e32, e64 = E.reference("edges", "lean", backward=True)
    m = _head(c, dev)
    B, N, T = c.B, c.N, c.iters
    BN = B * N
    bh, ah = _nhwc(c, dev)
    ps = pack_infos(c.infos(), c.H, c.W, dev, True)
    dflow = torch.zeros(B, N, 3, device=dev)
    for b, n in enumerate(c.counts):
        dflow[b, :n] = c.cot[b].to(dev)
    seen = _record(monkeypatch)
    W, keep = m._weights()
    xtab = m._xtab(W)
    W16, keep16 = m._weights16(W, keep)
    z = dict(dtype=torch.float32, device=dev)          # zero-filled outputs: what a kernel does not write compares equal

    def fwd(Wm, mode):
        flow, hs = torch.zeros(B, N, 3, **z), torch.zeros((T + 1) * BN * 128, **z)
        call("df_gru_lean_fwd", img(bh), img(ah), ptr(ps.coords), ptr(ps.offs), ptr(ps.counts), B, N, T, Wm, ptr(xtab), ptr(flow),
             ptr(hs), mode, stream())
        return flow, hs

    def bwd(bf, hs, mode):
        _, Wm, WT, keepb = m._weights_bwd(bf, False)
        gpl, dh0, dpre1 = torch.zeros(4 * T * BN * 128, **z), torch.zeros(BN, 128, **z), torch.zeros(BN, 32, **z)
        partial = torch.zeros(B * ((N + 63) // 64), call("df_gru_lean_partial_width"), **z)
        call("df_gru_lean_bwd", ptr(dflow), ptr(ps.offs), ptr(ps.counts), B, N, T, Wm, WT, ptr(xtab), ptr(hs), ptr(gpl), ptr(dh0),
             ptr(dpre1), ptr(partial), mode, stream())
        torch.cuda.synchronize()
        return gpl, dh0, dpre1, partial

    flow1, hs1 = fwd(W, 1)
    flow2, hs2 = fwd(W16, 2)
    torch.cuda.synchronize()
    b1, b2 = bwd(False, hs1, 1), bwd(True, hs2, 2)
    del keep, keep16
    same_f = torch.equal(flow1, flow2) and torch.equal(hs1, hs2)
    same_b = all(torch.equal(x, y) for x, y in zip(b1, b2))
    parity.record("gru_bf16_mode1_edges", "mode 1 == mode 2 to the bit", forward=same_f, backward=same_b)
    print(f"[decoder bf16] mode 1 vs mode 2 on edges: forward (flow, saved planes) bit-identical: {same_f}; backward (planes, dh0, dpre1, "
          f"partial sums) bit-identical: {same_b}")
    for mode, flow, hs, (_, dh0, dpre1, _) in ((1, flow1, hs1, b1), (2, flow2, hs2, b2)):
        tag = f"gru_bf16_mode{mode}_edges"
        _check(tag, c, dict(flow=[flow[b, :n] for b, n in enumerate(c.counts)]), (e32, e64))
        hT = _rows(hs[T * BN * 128:], c, 128)
        parity.three_way(tag, "h_T", hT, e32["hT"], e64["hT"])
        parity.three_way(tag, "dh0", _rows(dh0, c, 128), e32["dh0"], e64["dh0"])
        parity.three_way(tag, "dpre1", _rows(dpre1, c, 32), e32["dpre1"], e64["dpre1"])
    assert _gru(seen) == {"df_gru_lean_fwd", "df_gru_lean_bwd", "df_gru_xtab", "df_gru_lean_partial_width"}, sorted(seen)


# the tensors behind which the backward kernel's per-workgroup partial sums stand (the [416][4] sums S, dW_2, d b_2): whole tensors, and
# the x columns (128 ..) of the four GEMM weights
S_TENSORS = ("grad gru.convz.bias", "grad gru.convr.bias", "grad gru.convq.bias", "grad decoder.0.bias", "grad decoder.2.weight",
             "grad decoder.2.bias", "grad offset_encoder.weight", "grad offset_encoder.bias")
S_COLUMNS = ("grad gru.convz.weight", "grad gru.convr.weight", "grad gru.convq.weight", "grad decoder.0.weight")
WAVE_ENVS = {"default": {}, "waves4": {"DF_GRU_WAVES": "4", "DF_GRU_FWD_WAVES": "4"}, "fwd8": {"DF_GRU_FWD_WAVES": "8"}}


def test_wave_forms_bit_identical(dev, tmp_path):
    """DF_GRU_WAVES / DF_GRU_FWD_WAVES (csrc/decoder4.hip: 4, 8 or 12 waves per workgroup; read once per process -> one fresh child per
    form, one alive at a time): the module step on `edges` in fp32 (bf16x2) mode and under ops.mfma_bf16(True).

    From the code: a wave owns 16 rows and does the same arithmetic on them in every form, so flow, the saved planes, the gate-gradient
    planes, dh0 and with them d(before), d(after) and the h columns (:128) of the four GEMM weight gradients are bit-identical.  The
    backward's partial sums are NOT the same sum in the 4-wave form: a workgroup adds its waves' partials (4 or 8 of them) and the
    column sum then adds the workgroups', so DF_GRU_WAVES=4 groups the same terms differently in fp32 -- ((w0 + w1 + w2 + w3) + (w4 + ..
    + w7)) per 128 rows against two separate rows of 64.  Everything fed by those sums (the biases, the offset encoder, the head's
    second layer and the x columns of the GEMM weights) is therefore held to the float64 bound of its mode in that form, and asserted
    bit-identical only where the backward's form is unchanged (DF_GRU_FWD_WAVES=8).  Measured on an MI355X: DF_GRU_FWD_WAVES=8: 30 of 30
    tensors identical; DF_GRU_WAVES=4 DF_GRU_FWD_WAVES=4: flow, d(before), d(after), grad decoder.2.bias and the h columns identical in
    both modes, the other eleven gradients differ in the last bits and meet their bounds (fp32 mode: at most 5.5e-6 max / 6.7e-6 rms
    against the float64 oracle; bf16 mode: the figures of test_bf16_mode_step_vs_float64)."""
    c = DC.case("edges")
    runs = {}
    for tag, env in WAVE_ENVS.items():
        out = str(tmp_path / f"{tag}.npz")
        e = {k: v for k, v in os.environ.items() if k not in ("DF_GRU_WAVES", "DF_GRU_FWD_WAVES", "DF_GRU_LEAN", "DF_GRU_X2")}
        t0 = time.perf_counter()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "decoder_wave_child.py"), out], cwd=ROOT,
                           env=dict(e, **env), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, f"{tag}: exit {r.returncode}\n" + r.stdout[-1500:] + r.stderr[-3000:]
        runs[tag] = {k: torch.from_numpy(v) for k, v in np.load(out).items()}
        print(f"[decoder bf16] wave form {tag}: child took {time.perf_counter() - t0:.1f} s")
    base = runs["default"]
    assert len(base) == 2 * 15
    refs = {"fp32": DC.reference("edges"), "bf16": E.reference("edges", "lean", backward=True)}
    bad = []
    for tag in ("waves4", "fwd8"):
        differ = sorted(k for k in base if not torch.equal(runs[tag][k], base[k]))
        parity.record("gru_wave_forms_edges", tag, tensors_that_differ=differ)
        print(f"[decoder bf16] wave form {tag}: {len(base) - len(differ)} of {len(base)} tensors bit-identical to the default; differ: {differ}")
        for k in base:
            mode, what = k.split("/", 1)
            got, ref = runs[tag][k], base[k]
            if tag == "waves4" and (what in S_TENSORS or what in S_COLUMNS):
                if what in S_COLUMNS and not torch.equal(got.view(got.shape[0], 192)[:, :128], ref.view(ref.shape[0], 192)[:, :128]):
                    bad.append(f"{tag} {k}: the h columns differ")
                r32, r64 = refs[mode]
                try:
                    parity.three_way(f"gru_wave_{tag}_{mode}_edges", what, got, r32["gw"][what[5:]], r64["gw"][what[5:]])
                except AssertionError as ex:
                    bad.append(str(ex))
            elif not torch.equal(got, ref):
                bad.append(f"{tag} {k}: not bit-identical to the default form (max |diff| {float((got - ref).abs().max()):.3e})")
    assert not bad, "\n".join(bad)
