"""GPU: the engine on rectangular, non-power-of-two BEV grids against the CPU oracle (cases and what each reaches:
tests/helpers/rect_cases.py, decided on the CPU by tests/test_rect_cases_cpu.py).

Everything the square model tests check, on grids where H and W can be told apart, where h, w and h*w of every UNet level are no
powers of two (the elementwise kernels' real-division index decode), and where the clouds overfill one axis only: eval forward
(index lists equal, flow 1e-4, pose_flow 1e-5), a training step through the nn.Module path and through the Trainer's direct path
(parity.check_step: every parameter gradient against the float64 oracle), the bf16 training mode against the same float64
gradients, and the training tile rule as an error that leaves the model untouched.  No bound is restated here: parity's floor and
factor, and test_gpu_model's BF16_GRAD_RMS.
"""
import functools
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import parity  # noqa: E402
import rect_cases as RC  # noqa: E402
from test_gpu_model import BF16_GRAD_RMS, check, to_dev  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the rectangular-grid tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _mine(c, state, dev, **kw):
    import deflow_amd
    m = deflow_amd.DeFlow(**c.cfg, **kw)
    m.load_state_dict(state)
    return m.to(dev)


def _record(monkeypatch):
    """-> the set that collects every df_* entry point looked up on the library from here on (test_gpu_decoder_cases.py's proxy)"""
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


# ---- eval forward ----------------------------------------------------------------------------------------------------------------
def _eval_vs_oracle(c, ref, mine, dev, tag):
    """test_gpu_model.py::test_forward_eval_vs_oracle's checks"""
    ref.eval(); mine.eval()
    batch = RC.make_batch(c)
    with torch.no_grad():
        want = ref(batch)
        got = mine(to_dev(batch, dev))
    for b in range(c.B):
        assert torch.equal(got["pc0_valid_point_idxes"][b].cpu(), want["pc0_valid_point_idxes"][b])
        assert torch.equal(got["pc1_valid_point_idxes"][b].cpu(), want["pc1_valid_point_idxes"][b])
        assert torch.equal(got["pc1_points_lst"][b].cpu(), want["pc1_points_lst"][b])
        e = parity.rel_err(got["flow"][b], want["flow"][b])
        parity.record(f"rect_eval_{tag}", f"flow[{b}]", err_vs_oracle32=e, bound=1e-4, ok=e <= 1e-4)
        check(f"rect eval {tag} flow b{b}", got["flow"][b], want["flow"][b], 1e-4)
        m = ~torch.isnan(want["pose_flow"][b])
        check(f"rect eval {tag} pose_flow b{b}", got["pose_flow"][b].cpu()[m], want["pose_flow"][b][m], 1e-5)


EVAL = [("64x96", dict(decoder_option="gru", num_iters=2)), ("96x64", dict(decoder_option="gru", num_iters=2)),
        ("40x72", dict(decoder_option="gru", num_iters=2)), ("64x96", dict(decoder_option="linear")),
        ("64x96", dict(decoder_option="gru", num_iters=2, align_corners=True))]


@pytest.mark.parametrize("name,opt", EVAL, ids=[f"{n}-{o['decoder_option']}{'-ac' if o.get('align_corners') else ''}" for n, o in EVAL])
def test_forward_eval_vs_oracle(dev, name, opt):
    c = RC.case(name)
    ref = RC.oracle(c, 1, **opt)
    _eval_vs_oracle(c, ref, _mine(c, ref.state_dict(), dev, **opt), dev, f"{name}_{opt['decoder_option']}{'_ac' if opt.get('align_corners') else ''}")


# ---- training step, nn.Module path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["64x96", "96x64"])
def test_train_step_vs_oracle(dev, monkeypatch, name):
    """mine(bd) -> O.training_loss -> backward, as test_gpu_model.py::test_train_step_vs_oracle: flow, loss and every parameter gradient
    three-way against the float64 oracle, BatchNorm-shadowed biases against sum |dy|, the buffers after the step"""
    from oracle import ref_torch as O
    c = RC.case(name)
    ref = RC.oracle(c, 2, decoder_option="gru", num_iters=2)
    mine = _mine(c, ref.state_dict(), dev, decoder_option="gru", num_iters=2)
    ref.train(); mine.train()
    ref, ref64 = parity.oracle_pair(ref)
    batch = RC.make_batch(c)
    o32, o64 = parity.oracle_step(ref, batch), parity.oracle_step(ref64, batch)
    bd = to_dev(batch, dev)
    sums = parity.DyAbsSums(monkeypatch)
    res_m = mine(bd)
    loss_m = O.training_loss(res_m, bd)
    loss_m.backward()
    parity.check_step(f"rect_train_{name}", mine, res_m, loss_m.detach(), o32, o64, dy_sums=sums)
    br = dict(ref.named_buffers())
    for k, v in mine.named_buffers():
        if v.dtype.is_floating_point:
            check(f"rect {name} buffer {k}", v, br[k], 1e-4)
        else:
            assert int(v) == int(br[k]), k


# ---- the Trainer's direct path ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trainer_reference(name):
    """the oracle pair of one grid, stepped once: (initial state, batch, fp32 step, float64 step)"""
    c = RC.case(name)
    ref = RC.oracle(c, 13, decoder_option="gru", num_iters=2).train()
    state = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    ref, ref64 = parity.oracle_pair(ref)
    batch = RC.make_batch(c)
    t0 = time.perf_counter()
    o32, o64 = parity.oracle_step(ref, batch), parity.oracle_step(ref64, batch)
    print(f"[rect] oracle fp32 + float64 step on {name}: {time.perf_counter() - t0:.1f} s")
    return state, batch, o32, o64


@pytest.fixture(scope="module")
def ref_96x256():
    return _trainer_reference("96x256")


def _trainer_step(c, state, batch, dev, dtype):
    from deflow_amd import ops
    from deflow_amd.optim import Trainer
    mine = _mine(c, state, dev, decoder_option="gru", num_iters=2).train()
    tr = Trainer(mine, lr=0.0, dtype=dtype)
    bd = to_dev(batch, dev)
    with ops.mfma_bf16(dtype == "bf16", dtype == "bf16"), torch.no_grad():
        tr.flat.zero_grad(); tr.sink.begin()
        loss = tr._forward_backward(bd)
    torch.cuda.synchronize()
    st = mine.last_state
    m0 = st["counts0"].tolist()
    return mine, tr, {"flow": [st["flow"][b, :m0[b]] for b in range(len(m0))]}, loss.detach()


def _fp32_trainer_case(dev, monkeypatch, name, reference):
    c = RC.case(name)
    state, batch, o32, o64 = reference
    seen = _record(monkeypatch)
    mine, _, res_m, loss_m = _trainer_step(c, state, batch, dev, "fp32")
    parity.check_step(f"rect_trainer_{name}", mine, res_m, loss_m, o32, o64)
    print(f"[rect] trainer {name} conv entries: {' '.join(sorted(k for k in seen if 'conv2d' in k and not k.endswith('_ok')))}")
    assert {"df_deflow_loss_fwd", "df_deflow_loss_bwd"} <= seen
    return seen


def test_trainer_step_96x256_vs_oracle(dev, monkeypatch, ref_96x256):
    """tr.flat.zero_grad(); tr.sink.begin(); tr._forward_backward(bd): the hand-sequenced step on [96, 256] -- the fp16x2 halo form
    at W = 128, the row-pair form at W = 64, the generic form at W = 32"""
    seen = _fp32_trainer_case(dev, monkeypatch, "96x256", ref_96x256)
    assert seen & {"df_conv2d_h2", "df_conv2d_x3"}, sorted(seen)      # the shape reached the forms it was chosen for


def test_trainer_step_256x96_vs_oracle(dev, monkeypatch):
    """the transposed grid: W = 48 / 24 / 12, the same pixel counts per level"""
    _fp32_trainer_case(dev, monkeypatch, "256x96", _trainer_reference("256x96"))


def test_bf16_training_mode_96x256_vs_float64(dev, monkeypatch, ref_96x256):
    """Trainer(dtype="bf16") under ops.mfma_bf16(True, True) against the float64 oracle step of the fixture; the rule of
    test_gpu_model.py::_bf16_step_vs_digest applied to the full tensors instead of projections: per non-shadowed parameter
    rms-relative error and gradient-norm error <= BF16_GRAD_RMS, loss within 2e-3, per-sample flow within 2e-2 of ||flow||."""
    c = RC.case("96x256")
    state, batch, _, (res64, loss64, g64) = ref_96x256
    seen = _record(monkeypatch)
    mine, tr, res_m, loss16 = _trainer_step(c, state, batch, dev, "bf16")
    assert tr.bf16_store
    le = abs(float(loss16) - float(loss64)) / abs(float(loss64))
    print(f"[parity] rect_bf16_96x256 loss {float(loss16):.6f} / {float(loss64):.6f}: rel err {le:.3e} (bound 2e-3)")
    bad = []
    if le > 2e-3:
        bad.append(f"loss: {le:.3e} > 2e-3")
    for b in range(c.B):
        fe = parity.rms_rel(res_m["flow"][b], res64["flow"][b])
        parity.record("rect_bf16_96x256", f"flow[{b}]", rms_vs_fp64=fe, bound=2e-2, ok=fe <= 2e-2)
        print(f"[parity] rect_bf16_96x256 flow[{b}]: ||d|| / ||flow|| = {fe:.3e} (bound 2e-2)")
        if fe > 2e-2:
            bad.append(f"flow[{b}]: {fe:.3e} > 2e-2")
    worst = (0.0, 0.0, "")
    for k, p in mine.named_parameters():
        if parity.is_bn_shadowed_bias(k):
            continue
        r = parity.rms_rel(p.grad, g64[k])
        l2 = float(g64[k].double().norm())
        dn = abs(float(p.grad.double().norm()) - l2) / l2
        ok = r <= BF16_GRAD_RMS and dn <= BF16_GRAD_RMS
        parity.record("rect_bf16_96x256", "grad " + k, rms_vs_fp64=r, norm_err=dn, rms_bound=BF16_GRAD_RMS, ok=ok)
        worst = max(worst, (r, dn, k))
        if not ok:
            bad.append(f"grad {k}: rms {r:.3e} norm {dn:.3e} > {BF16_GRAD_RMS}")
    parity.record("rect_bf16_96x256", "worst grad " + worst[2], rms_vs_fp64=worst[0], norm_err=worst[1], rms_bound=BF16_GRAD_RMS,
                  ok=worst[0] <= BF16_GRAD_RMS)
    print(f"[parity] rect_bf16_96x256 bf16 mode vs float64 oracle: worst gradient rms-relative error {worst[0]:.3e} (norm error {worst[1]:.3e}) "
          f"on {worst[2]} -- bound {BF16_GRAD_RMS}")
    assert not bad, "\n".join(bad)
    assert {"df_conv2d_w16", "df_conv2d_wgrad_bf16"} <= seen, sorted(k for k in seen if "conv2d" in k)


# ---- the training tile rule -------------------------------------------------------------------------------------------------------
def test_training_tile_rule_is_an_error_that_touches_nothing(dev):
    """[40, 72] at B = 2: 90 rows per statistic group at stride 8, no multiple of the 64-row tile.  The training forward refuses with a
    ValueError naming B, H, W and the rule BEFORE any launch (state_dict() bit-equal afterwards); eval on the same model then passes"""
    c = RC.case("40x72")
    opt = dict(decoder_option="gru", num_iters=2)
    ref = RC.oracle(c, 1, **opt)
    mine = _mine(c, ref.state_dict(), dev, **opt).train()
    before = {k: v.detach().clone() for k, v in mine.state_dict().items()}
    bd = to_dev(RC.make_batch(c), dev)
    rule = r"B = 2, H = 40, W = 72.*B\*\(H/2\^k\)\*\(W/2\^k\) must be a multiple of df_conv2d_tile_m for k = 1, 2, 3"
    with pytest.raises(ValueError, match=rule):
        mine(bd)
    with pytest.raises(ValueError, match=rule), torch.no_grad():      # the tape-less training forward (batch statistics) as well
        mine(bd)
    with pytest.raises(ValueError, match=rule), torch.no_grad():      # and the backbone called on its own
        mine.backbone.run(torch.zeros(c.B, c.H, c.W, 64, device=dev), True, None)
    torch.cuda.synchronize()
    after = mine.state_dict()
    assert list(after) == list(before)
    for k, v in after.items():
        assert torch.equal(v, before[k]), f"{k} moved in a refused forward"
    _eval_vs_oracle(c, ref, mine, dev, "40x72_after_refusal")
