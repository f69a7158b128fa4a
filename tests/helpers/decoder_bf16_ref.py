"""The GRU decoder's bf16 forms restated on the CPU in plain torch, rounding to bfloat16 exactly where the kernels round: the reference
of tests/test_gpu_decoder_bf16_cases.py, itself proved by tests/test_decoder_bf16_ref_cpu.py (rounding off: equal to the float64 oracle
to 1e-10; mutations: each wrong rounding point fails parity.three_way).

emulate(case, form, dtype, rounding=True, backward=False, mut=(), gates="exact", iters=None) runs on a Case of
tests/helpers/decoder_cases.py with the `w.*` weights of tests/golden/g2_grudecoder_it4.npz and returns a dict shaped like
decoder_cases.reference's: flow (list per sample), and with backward=True gbefore, gafter, gw (a MANUAL backward: the kernels do not
differentiate through their roundings, so autograd through the emulation would be another function).  Arithmetic is in `dtype`
(float64: the reference; float32: its companion, which measures how strongly the inputs amplify fp32 noise into bf16 flips), with exact
sigmoid, tanh and erf-GELU (gates="kernel": the kernels' own formulas, csrc/common.h df_sigmoid_fast / df_tanh_fast).  R(v) below is RNE
to bfloat16 (ref64.bf16_rne); rounding=False makes R the identity, and every form is then the oracle's function.

Where the kernels round -- the specification under test.  W_g = the [128,192] weight of gate g (z, r, q), W_1 the head's [32,192]; columns
:128 multiply h, columns 128: multiply x = W_off o + b_off.

form "lean": forward gru_fwd4_kernel<.., MODE 1 | 2, ..> (csrc/decoder4.hip), weights in the form decoder.py:166-172 (_weights16) casts
  weights   R(W_z[:, :128]), R(W_r[:, :128]), R(W_q[:, :128]), R(W_1[:, :128])     decoder.py:170; mode 1: gemm_dma.h:200 (pack_bf16 of the
                                                                                   fp32 tile); the x columns are never read
  x part    P o + c, P = W[:, 128:] W_off, c = W[:, 128:] b_off + b, from the fp32 parameters in float64, stored fp32, applied as three
            fp32 FMAs: NOT rounded                                                 decoder4.hip:72-89 (table), :182-196 (xinit)
  A operand R(h) for z and r (decoder4.hip:223, :229), R(r * h) for q (:234 writes r * h with the fp32 h, :238), R(h_T) for the head
            (:263); the rounding itself is gemm_dma.h:185 / :197 (pack_bf16)
  state     h stays fp32 across iterations; the blend (1 - z) h + z q uses it     decoder4.hip:201-205, :245
  head      hidden layer gelu(pre1) fp32, W_2 and b_2 fp32                         decoder4.hip:267-274
  saved     planes 0 .. T-1 = R(h_t) (h entering iteration t), plane T = h_T fp32  decoder4.hip:207-217

form "inference": gru_fwd_bf16_kernel (csrc/decoder_bf16.hip); form "full": gru_fwd3_kernel<.., BF, W16> (csrc/decoder3.hip).  As lean but
  x         R(W_off o + b_off)              decoder_bf16.hip:117-119 (stored as bf16);  decoder3.hip:82-89 + gemm_dma.h:185 (x stays fp32 in
                                            registers and is rounded as the A operand of each GEMM: the same value)
  weights   all 192 columns rounded         decoder.py:283-284 (run_bf16), decoder.py:170; biases fp32 (decoder_bf16.hip:150-164,
                                            decoder3.hip:111-125)
  A operand R(h), R(r * h) (fp32 h), R(h_T) decoder_bf16.hip:143, :181, :194;  decoder3.hip:168, :186, :213
  saved (full only, decoder3.hip:133-155): R(h_t), R(z), R(r), R(q), R(r * h) per iteration, h_T fp32 -- returned as "planes" for
            completeness; the backward that reads them (decoder3_bwd.hip) is NOT emulated

form "lean", backward: gru_bwd4_kernel<MODE 1 | 2, ..> (csrc/decoder4.hip) + gru_wgrad4_kernel<1> / gru_head_wgrad4_kernel
(csrc/decoder_wgrad.hip) + gru_lean_finalize_kernel
  head      pre1 = x part + R(h_T) R(W_1[:, :128])^T (decoder4.hip:375, :455); hv = gelu(pre1), dpre1 = (dflow W_2) gelu'(pre1) fp32 (:479-482);
            dW_2 = dflow^T hv, db_2 fp32 (:484); dh = R(dpre1) R(W_1[:, :128]) (:488, :521)
  per iteration, reversed: hb = the saved bf16 plane R(h_t) (:531) is the ONLY h the backward has: it enters r * hb (:544), (q - hb) in
            dz_pre (:558) and hb in dr_pre (:580) -- the forward used the fp32 h there
  gates     z, r from hb, q from R(r * hb), rounded weights (:534-549)
  data      dh <- dh (1 - z) + R(dz_pre) R(W_z[:, :128]) + (R(dq_pre) R(W_q[:, :128])) r + R(dr_pre) R(W_r[:, :128])
            (:556-588; the transposed weights are bf16 casts of the fp32 transposes, decoder.py:231: the same values)
  planes    R(dz_pre) | R(dr_pre) | R(dq_pre) | R(r * hb) (lds_to_plane, :342-348); dW_g[:, :128] = fp32 sum of products of those planes
            with the R(h_t) planes (z, r) or the R(r * hb) plane (q)              decoder_wgrad.hip:393, :467-482
  S sums    S_g = sum dg_pre (x) (o, 1) from the UNROUNDED fp32 dg_pre (colsum reads the A region, decoder4.hip:414-427, after c_to_lds of the
            fp32 values); dW_g[:, 128:], d b_g, dW_off, d b_off from S and the fp32 parameters (decoder4.hip:631-656)
  head dW_1[:, :128] = dpre1^T h_T on bf16x2 products of the fp32 values (decoder_wgrad.hip:605-618): not rounded here

Read from the code and NOT as the list in the issue has it: nothing -- every point above was confirmed.  Two details the list leaves open:
the mode-1 kernels round the fp32 weight tile element by element with the same RNE cast as the host's .to(bfloat16) (same values as
mode 2, but another k-to-lane assignment inside an MFMA: see test_mode1_equals_mode2), and the backward's q is recomputed from R(r * hb),
not from the forward's R(r * h), so even z, r, q of the two passes differ by flips.

mut: the deliberate mistakes of tests/test_decoder_bf16_ref_cpu.py
  "state_bf16"      h <- R(h) after every blend          "rh_rounded_h"   r * R(h) in the forward
  "blend_rounded_h" (1 - z) R(h) + z q                    "hid_rounded"    R(gelu(pre1)) before W_2
  "x_flip"          lean: x rounded as the inference form has it; inference / full: x not rounded
  "bwd_q_minus_h"   backward: (q - h) with the unrounded h  "bwd_dz_plane"   the dz_pre plane of the weight gradient left unrounded
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_cases as DC  # noqa: E402
import ref64 as R  # noqa: E402

FORMS = ("lean", "inference", "full")
MUTATIONS = ("state_bf16", "rh_rounded_h", "blend_rounded_h", "hid_rounded", "x_flip", "bwd_q_minus_h", "bwd_dz_plane")
LOG2E = 1.4426950408889634


def _gate_fns(kind: str):
    if kind == "exact":
        return torch.sigmoid, torch.tanh
    assert kind == "kernel"
    return (lambda v: 1.0 / (1.0 + torch.exp2(-LOG2E * v))), (lambda v: 1.0 - 2.0 / (1.0 + torch.exp2(2.0 * LOG2E * v)))


def emulate(c, form: str, dtype=torch.float64, rounding: bool = True, backward: bool = False, mut=(), gates: str = "exact",
            iters: int = None):
    assert form in FORMS and set(mut) <= set(MUTATIONS), (form, mut)
    assert not backward or form == "lean", "only the lean form's backward is emulated"
    T = c.iters if iters is None else iters
    rnd = (lambda t: R.bf16_rne(t).to(dtype)) if rounding else (lambda t: t)
    sig, tanh = _gate_fns(gates)
    w = {k: v.to(dtype) for k, v in DC.weights().items()}
    w64 = {k: v.double() for k, v in DC.weights().items()}
    W = {g: w[f"gru.conv{g}.weight"].view(128, 192) for g in "zrq"}
    W["1"] = w["decoder.0.weight"]
    bias = {"z": w["gru.convz.bias"], "r": w["gru.convr.bias"], "q": w["gru.convq.bias"], "1": w["decoder.0.bias"]}
    W_off, b_off, W_2, b_2 = w["offset_encoder.weight"], w["offset_encoder.bias"], w["decoder.2.weight"], w["decoder.2.bias"]
    Wh = {g: rnd(W[g][:, :128]) for g in W}

    # rows of every sample, concatenated
    offs = torch.cat(c.offs).to(dtype)
    h0 = torch.cat([torch.cat([c.before[b].to(dtype)[:, vc[:, 1].long(), vc[:, 2].long()].T,
                               c.after[b].to(dtype)[:, vc[:, 1].long(), vc[:, 2].long()].T], 1) for b, vc in enumerate(c.coords)])
    if form == "lean" and "x_flip" not in mut:
        # the [416,4] table (df_gru_xtab): float64 products of the fp32 parameters, stored in the run's dtype
        P = {g: (w64[_wkey(g)].view(-1, 192)[:, 128:] @ w64["offset_encoder.weight"]).to(dtype) for g in W}
        cc = {g: (w64[_wkey(g)].view(-1, 192)[:, 128:] @ w64["offset_encoder.bias"] + w64[_bkey(g)]).to(dtype) for g in W}
        xc = {g: offs @ P[g].T + cc[g] for g in W}
    else:   # x as an operand of GEMMs on all 192 (rounded) weight columns; x_flip on these forms leaves x itself unrounded
        x = offs @ W_off.T + b_off
        if form == "lean" or "x_flip" not in mut:
            x = rnd(x)
        xc = {g: x @ rnd(W[g][:, 128:]).T + bias[g] for g in W}

    h, hs, planes = h0, [], []
    for _ in range(T):
        hs.append(h)
        hA = rnd(h)
        z = sig(xc["z"] + hA @ Wh["z"].T)
        r = sig(xc["r"] + hA @ Wh["r"].T)
        rh = rnd(r * (hA if "rh_rounded_h" in mut else h))
        q = tanh(xc["q"] + rh @ Wh["q"].T)
        planes.append(dict(h_in=hA, z=rnd(z), r=rnd(r), q=rnd(q), rh=rh))
        h = (1.0 - z) * (hA if "blend_rounded_h" in mut else h) + z * q
        if "state_bf16" in mut:
            h = rnd(h)
    hT = h
    pre1 = xc["1"] + rnd(hT) @ Wh["1"].T
    hid = R.gelu(pre1)
    if "hid_rounded" in mut:
        hid = rnd(hid)
    flow = hid @ W_2.T + b_2
    out = dict(flow=list(flow.split(c.counts)), planes=planes, hT=hT)
    if not backward:
        return out

    o1 = torch.cat([offs, torch.ones_like(offs[:, :1])], 1)          # (o, 1): S_g = dg_pre^T o1, [rows of g, 4]
    dflow = torch.cat(c.cot).to(dtype)
    gw = {"decoder.2.weight": dflow.T @ hid, "decoder.2.bias": dflow.sum(0)}
    dpre1 = (dflow @ W_2) * R.gelu_grad(pre1)
    S = {"1": dpre1.T @ o1}
    dWh = {"1": dpre1.T @ hT}
    dh = rnd(dpre1) @ Wh["1"]
    for g in "zrq":
        S[g], dWh[g] = torch.zeros(128, 4, dtype=dtype), torch.zeros(128, 128, dtype=dtype)
    for t in reversed(range(T)):
        hb = rnd(hs[t])
        z = sig(xc["z"] + hb @ Wh["z"].T)
        r = sig(xc["r"] + hb @ Wh["r"].T)
        rh = rnd(r * hb)
        q = tanh(xc["q"] + rh @ Wh["q"].T)
        d = dh
        dq_pre = d * z * (1.0 - q * q)
        dz_pre = d * (q - (hs[t] if "bwd_q_minus_h" in mut else hb)) * z * (1.0 - z)
        drh = rnd(dq_pre) @ Wh["q"]
        dr_pre = drh * hb * r * (1.0 - r)
        dh = d * (1.0 - z) + rnd(dz_pre) @ Wh["z"] + drh * r + rnd(dr_pre) @ Wh["r"]
        for g, dg, hp in (("z", dz_pre, hb), ("r", dr_pre, hb), ("q", dq_pre, rh)):
            S[g] = S[g] + dg.T @ o1
            dWh[g] = dWh[g] + (dg if (g == "z" and "bwd_dz_plane" in mut) else rnd(dg)).T @ hp
    # the small gradients from the S sums (gru_lean_finalize_kernel): fp32 parameters
    dW_off, db_off = torch.zeros(64, 3, dtype=dtype), torch.zeros(64, dtype=dtype)
    for g in ("z", "r", "q", "1"):
        gw[_wkey(g)] = torch.cat([dWh[g], S[g][:, :3] @ W_off.T + S[g][:, 3:4] * b_off], 1).view(w[_wkey(g)].shape)
        gw[_bkey(g)] = S[g][:, 3]
        dW_off = dW_off + W[g][:, 128:].T @ S[g][:, :3]
        db_off = db_off + W[g][:, 128:].T @ S[g][:, 3]
    gw["offset_encoder.weight"], gw["offset_encoder.bias"] = dW_off, db_off
    # the gather's backward: a cell's rows summed
    gb, ga = torch.zeros(c.B, c.H * c.W, 64, dtype=dtype), torch.zeros(c.B, c.H * c.W, 64, dtype=dtype)
    for b, d in enumerate(dh.split(c.counts)):
        gb[b].index_add_(0, c.cells(b), d[:, :64])
        ga[b].index_add_(0, c.cells(b), d[:, 64:])
    out.update(dh0=dh, dpre1=dpre1)          # rows of all samples: the backward kernel's own outputs, before the gather's sums
    out.update(gbefore=gb.view(c.B, c.H, c.W, 64).permute(0, 3, 1, 2), gafter=ga.view(c.B, c.H, c.W, 64).permute(0, 3, 1, 2), gw=gw)
    return out


def _wkey(g: str) -> str:
    return "decoder.0.weight" if g == "1" else f"gru.conv{g}.weight"


def _bkey(g: str) -> str:
    return "decoder.0.bias" if g == "1" else f"gru.conv{g}.bias"


_EMU = {}


def reference(name: str, form: str, backward: bool = False, iters: int = None, gates: str = "exact"):
    """-> (fp32 emulation, float64 emulation) of a case; computed once per process and never modified by its readers"""
    key = (name, form, backward, iters, gates)
    if key not in _EMU:
        c = DC.case(name)
        _EMU[key] = tuple(emulate(c, form, dt, backward=backward, iters=iters, gates=gates if dt == torch.float32 else "exact")
                          for dt in (torch.float32, torch.float64))
    return _EMU[key]


def cat_flow(res) -> torch.Tensor:
    """the case's flows as one [sum n, 3] tensor: a bf16 flip is a per-row event and a one-row sample has no average"""
    return torch.cat([f.detach().cpu() for f in res["flow"]])


def pairs(res, refs):
    """(name, got, [reference tensors]) over the concatenated flow and, where both sides carry them, d(before), d(after) and every
    parameter gradient"""
    yield "flow", cat_flow(res), [cat_flow(r) for r in refs]
    if "gw" in res and "gw" in refs[0]:
        yield "d(before)", res["gbefore"], [r["gbefore"] for r in refs]
        yield "d(after)", res["gafter"], [r["gafter"] for r in refs]
        for k in sorted(refs[0]["gw"]):
            yield "grad " + k, res["gw"][k], [r["gw"][k] for r in refs]
