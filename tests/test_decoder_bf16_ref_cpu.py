"""CPU: the emulating reference of the GRU decoder's bf16 forms (tests/helpers/decoder_bf16_ref.py) is right and sharp, decided without
a GPU.  tests/test_gpu_decoder_bf16_cases.py holds the kernels to parity.three_way(got, emulation fp32, emulation float64); this file
shows what that bound can and cannot see.

  * rounding switched off, the emulation -- its hand-written backward included -- is the float64 oracle to 1e-10 (measured <= 2e-15);
  * the floor: the emulation in fp32 against the emulation in float64 (bf16 rounding flips seeded by fp32 noise).  Measured, flow over
    the concatenated rows, max-norm / rms / 1 - cos:
        edges  lean 1.6e-4 / 1.4e-5 / 9e-11     inference = full 3.1e-4 / 2.3e-5 / 3e-10
        walk   lean 4.2e-4 / 1.5e-5 / 1e-10     inference = full 6.2e-4 / 1.7e-5 / 1e-10
    asserted inside twice the prototype's worst figures (max 6.2e-4, rms 3.2e-5); the gradients' rms floors are 5e-6 .. 1.2e-4, so
    three_way's rms bound on the GPU is 1e-4 for flow and at most 5e-4 for a gradient -- against 6e-4 .. 1.7e-3 for the whole effect
    of bf16 operands on flow;
  * every mutation of decoder_bf16_ref.MUTATIONS fails three_way at the default floor and factor in the rms AND the cosine norm, on
    both cases and every form it applies to (measured rms 4e-4 .. 1.4e-3 against bounds of 1e-4 .. 3.2e-4): none is left uncovered.
    The forward mutations are judged on flow; "bwd_q_minus_h" on d(before) and d(after); "bwd_dz_plane" shows in grad gru.convz.weight
    alone (it touches nothing else), 9.7e-4 .. 1.2e-3 rms against a bound of 3e-4.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import decoder_bf16_ref as E  # noqa: E402
import decoder_cases as DC  # noqa: E402
import parity  # noqa: E402

CASES = ["edges", "walk"]
FLOOR_MAX, FLOOR_RMS = 2 * 6.2e-4, 2 * 3.2e-5      # twice the worst fp32-vs-float64 figures of the prototype the bound was designed on
FORWARD_MUT = ["state_bf16", "rh_rounded_h", "blend_rounded_h", "hid_rounded", "x_flip"]
BACKWARD_MUT = {"bwd_q_minus_h": ["d(before)", "d(after)"], "bwd_dz_plane": ["grad gru.convz.weight"]}


@pytest.mark.parametrize("name", CASES)
def test_rounding_off_is_the_float64_oracle(name):
    c = DC.case(name)
    _, r64 = DC.reference(name)
    got = E.emulate(c, "lean", torch.float64, rounding=False, backward=True)
    worst = 0.0
    for b, n in enumerate(c.counts):
        assert tuple(got["flow"][b].shape) == (n, 3)
    for what, g, (w,) in E.pairs(got, (r64,)):
        e = parity.rel_err(g, w)
        worst = max(worst, e)
        assert e <= 1e-10, f"{name} {what}: emulation without rounding vs float64 oracle {e:.3e}"
    for form in ("inference", "full"):
        for gates in ("exact", "kernel"):      # the kernels' gate formulas are the same functions
            f = E.emulate(c, form, torch.float64, rounding=False, gates=gates)
            e = parity.rel_err(E.cat_flow(f), E.cat_flow(r64))
            worst = max(worst, e)
            assert e <= 1e-10, f"{name} {form} {gates}: {e:.3e}"
    print(f"[decoder bf16 ref] {name}: rounding off, worst error vs the float64 oracle {worst:.2e}")


@pytest.mark.parametrize("form", E.FORMS)
@pytest.mark.parametrize("name", CASES)
def test_fp32_noise_floor(name, form):
    e32, e64 = E.reference(name, form, backward=form == "lean")
    for what, g, (w,) in E.pairs(e32, (e64,)):
        m, r, c = parity.rel_err(g, w), parity.rms_rel(g, w), parity.one_minus_cos(g, w)
        parity.record(f"gru_bf16_floor_{name}_{form}", what, max=m, rms=r, one_minus_cos=c)
        print(f"[decoder bf16 ref] floor {name} {form} {what}: max {m:.2e} rms {r:.2e} 1-cos {c:.1e}")
        if what == "flow":
            assert m <= FLOOR_MAX and r <= FLOOR_RMS and c <= FLOOR_RMS ** 2, f"{name} {form}: floor max {m:.3e} rms {r:.3e} 1-cos {c:.3e}"


def _rms_and_cos_out(got, a32, a64):
    """the rms and cosine verdicts of parity.three_way, each alone"""
    rb = max(parity.FLOOR, parity.FACTOR * parity.rms_rel(a32, a64))
    cb = max(parity.FLOOR ** 2, parity.FACTOR ** 2 * parity.one_minus_cos(a32, a64))
    return parity.rms_rel(got, a64) > rb, parity.one_minus_cos(got, a64) > cb


@pytest.mark.parametrize("mut", FORWARD_MUT + list(BACKWARD_MUT))
@pytest.mark.parametrize("name", CASES)
def test_mutation_fails_three_way(name, mut):
    c = DC.case(name)
    bwd = mut in BACKWARD_MUT
    for form in (("lean",) if bwd else E.FORMS):
        e32, e64 = E.reference(name, form, backward=form == "lean")
        mt = E.emulate(c, form, torch.float64, backward=bwd, mut=(mut,))
        tensors = {what: (g, refs) for what, g, refs in E.pairs(mt, (e32, e64))}
        for what in (BACKWARD_MUT[mut] if bwd else ["flow"]):
            g, (a32, a64) = tensors[what]
            rms_out, cos_out = _rms_and_cos_out(g, a32, a64)
            assert rms_out or cos_out, f"{name} {form} {mut}: {what} passes the rms and the cosine bound -- the GPU test cannot see it"
            with pytest.raises(AssertionError):
                parity.three_way(f"gru_bf16_mut_{name}_{form}_{mut}", what, g, a32, a64)
