"""GPU: an UpsampleSkip block's last 3x3 convolution composed with the next block's 1x1 (its only reader, nothing in between) into ONE
3x3 layer -- ops.WeightPrep(compose=...), unet._upsample_skip / run_backward, DF_FUSE_U5U1.

  * the compose launch inside df_weight_prep and df_u5u1_decompose against float64 at the two real size triples and a ragged one:
    We, be, dW5, db5, dW1, db1 within the suite's CONV32 rule (2e-6 of max |ref|), the composed planes within the fp16x2 rule with a
    scale >= max |We|, two runs bit-equal
  * df_upsample2x_bwd_h2: the planes df_h2_pack makes of df_upsample2x_bwd's output with the same bound, bit for bit
  * one model and batch, composed against not: the kernel tags, every parameter gradient and the flow against the float64 oracle
    (the three-way rule of tests/parity.py in the digest form of test_gpu_model.py::_bs16_case), the composed path's error within a
    factor 2 of the other's per tensor, and the switch
"""
import os
import struct
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

CONV32_MAX = 2e-6       # tests/test_gpu_layer_census.py CONV32: of max |ref|


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _h2_scale(amax: float) -> float:
    """df_h2_scale: the power of two that puts amax into [2^14, 2^15)"""
    e = (struct.unpack("<I", struct.pack("<f", amax))[0] >> 23) & 255
    return 2.0 ** (min(max(268 - e, 1), 254) - 127)


def _unpack_planes(planes: torch.Tensor, shape, amax: float) -> torch.Tensor:
    n = planes.numel() // 2
    hi, lo = planes[:n].double(), planes[n:].double()
    return ((hi + lo / 2048.0) / _h2_scale(amax)).view(shape)


def _max_err(got, ref) -> float:
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _pair(O, C, I, dev, seed):
    g = torch.Generator().manual_seed(seed)
    c5 = torch.nn.Conv2d(I, C, 3, 1, 1)
    c1 = torch.nn.Conv2d(C, O, 1, 1, 0)
    with torch.no_grad():
        for p in (*c5.parameters(), *c1.parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() == 1 else 0.05))
    c5, c1 = c5.to(dev), c1.to(dev)
    for m in (c5, c1):
        m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
    return c5, c1


@pytest.mark.parametrize("O,C,I", [(128, 256, 256), (64, 128, 128), (64, 128, 64)])
def test_compose_and_decompose_vs_float64(dev, O, C, I):
    from deflow_amd import ops
    from deflow_amd._lib import call, ptr, stream
    c5, c1 = _pair(O, C, I, dev, 1000 + O + C + I)
    w5, w1 = ops.ohwi(c5.weight).double(), c1.weight.detach().double().view(O, C)          # [C,3,3,I], [O,C]
    b5, b1 = c5.bias.detach().double(), c1.bias.detach().double()
    we_ref = torch.einsum("oc,cyxi->oyxi", w1, w5)
    be_ref = w1 @ b5 + b1
    wa = torch.zeros(1, device=dev)
    wa.copy_(torch.cat([p.detach().reshape(-1) for p in (*c5.parameters(), *c1.parameters())]).abs().max().reshape(1))
    runs = []
    for _ in range(2):
        wp = ops.WeightPrep([], wa, compose=[(c5, c1)])
        wp.run(wa)
        we, be = wp.composed(c5, c1)
        assert we.shape == (O, 3, 3, I) and be.shape == (O,)
        wt = wp.wt(we)
        (p_w, a_w), (p_t, a_t) = wp.h2(we), wp.h2(wt)
        l1 = wp.l1(we, be)
        torch.cuda.synchronize()
        runs.append([t.clone() for t in (we, be, wt, p_w, p_t, a_w, l1[0], l1[1])])
    we, be, wt, p_w, p_t, a_w, l1w, bmax = runs[0]
    e_we, e_be = _max_err(we, we_ref), _max_err(be, be_ref)
    print(f"[fuse] compose {O},{C},{I}: We {e_we:.2e} be {e_be:.2e} of max |ref| (bound {CONV32_MAX:.0e})")
    assert e_we <= CONV32_MAX and e_be <= CONV32_MAX
    # the composed layer is an ordinary layer of the table: transpose, planes of both with ITS scale, row L1 norm, max |bias|
    assert torch.equal(wt, we.permute(3, 1, 2, 0))
    amax = float(a_w)
    assert amax >= float(we.abs().max()) and amax <= 2.0 * float(we.abs().max())
    for planes, src in ((p_w, we), (p_t, wt.contiguous())):
        back = _unpack_planes(planes, src.shape, amax)
        err = (back - src.double()).abs()
        assert bool((err <= src.double().abs() * 2.0 ** -21 + amax * 2.0 ** -36).all()), float(err.max())
    assert abs(float(l1w) - float(we.abs().sum((1, 2, 3)).max())) <= 1e-5 * float(l1w) and float(bmax) == float(be.abs().max())
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # decompose: the four parameter gradients from the composed layer's weight gradient and bias sum
    g = torch.Generator().manual_seed(7)
    dwe = torch.randn(O, 3, 3, I, generator=g).to(dev)
    dbe = torch.randn(O, generator=g).to(dev)
    outs = []
    for _ in range(2):
        dw5, db5 = torch.full((C, 3, 3, I), 7.0, device=dev), torch.full((C,), 7.0, device=dev)
        dw1, db1 = torch.full((O, C), 7.0, device=dev), torch.full((O,), 7.0, device=dev)
        call("df_u5u1_decompose", ptr(ops.ohwi(c1.weight)), ptr(ops.ohwi(c5.weight)), ptr(c5.bias.detach()), ptr(dwe), ptr(dbe), O, C, 9, I,
             ptr(dw5), ptr(db5), ptr(dw1), ptr(db1), stream())
        torch.cuda.synchronize()
        outs.append((dw5, db5, dw1, db1))
    dw5, db5, dw1, db1 = outs[0]
    refs = dict(dW5=torch.einsum("oc,oyxi->cyxi", w1, dwe.double()), db5=w1.t() @ dbe.double(),
                dW1=torch.einsum("oyxi,cyxi->oc", dwe.double(), w5) + torch.outer(dbe.double(), b5), db1=dbe.double())
    for (name, ref), got in zip(refs.items(), (dw5, db5, dw1, db1)):
        e = _max_err(got, ref)
        print(f"[fuse] decompose {O},{C},{I}: {name} {e:.2e} of max |ref| (bound {CONV32_MAX:.0e})")
        assert e <= CONV32_MAX, (name, e)
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("n,h,w", [(2, 8, 8), (2, 6, 10)])
def test_upsample2x_bwd_h2_equals_pack_of_the_fp32_form(dev, n, h, w, ac):
    from deflow_amd import ops
    from deflow_amd._lib import call, img, ptr, stream
    lat = 64
    g = torch.Generator().manual_seed(n * 100 + h * 10 + w + int(ac))
    dcat = torch.randn(n, 2 * h, 2 * w, 2 * lat, generator=g).to(dev)        # the engine's dy: the first half of a concatenation's gradient
    bound = torch.full((1,), 4.5 * float(dcat.abs().max()), device=dev)
    dt = torch.full((n, h, w, lat), 7.0, device=dev)
    call("df_upsample2x_bwd", img(dcat, lat, 0), img(dt), int(ac), stream())
    ref = ops.h2_pack(dt, bound)
    got = ops.h2_empty((n, h, w, lat), dev, bound)
    got.fill_(7.0)
    ops.upsample2x_bwd(img(dcat, lat, 0), img(got), ac)
    torch.cuda.synchronize()
    assert float(dt.abs().max()) <= float(bound)
    assert torch.equal(got, ref), float((ops.h2_unpack(got) - ops.h2_unpack(ref)).abs().max())
    assert float((ops.h2_unpack(got) - dt).abs().max()) <= 2.0 ** -21 * float(dt.abs().max()) + 2.0 ** -36 * float(bound)


# ---- one model and batch, composed against not ----------------------------------------------------------------------------------
# The shape.  bs16_256 (B = 16, 256 x 256, 20 000 points) has no pre-split FORWARD form for the composed layers: 64 x 64 x 16 pixels of
# 128 output channels are 256 of the 512 tiles the 256 x 128 form asks for, and 128-pixel rows have no 512 x 64 form (df_conv2d_h2p_ok;
# asserted below).  The smallest case of tests/helpers/rect_cases.py that takes both layers is 320x512 at B = 16, which has no float64
# reference a test can afford: the oracle is a CPU program (its voxeliser indexes with CPU tensors) and 16 such pairs cost it minutes
# in float64 (Case.oracle = False).  The shape used is therefore the one that takes the layers AND has float64 digests committed:
# bs16_512 = BASELINE configs[2] itself (tests/golden/bs16_512_digest.npz, oracle/gen_digest_bs16.py: per tensor ||g||_2, 16 random-sign
# projections of the float64 gradient and the fp32 oracle's own rms error).
# The rule.  A projection of an error vector e is N(0, ||e||_2^2): per tensor, est = sqrt(mean of the 16 squared projection errors) is
# the estimate of ||e||_2 both paths are measured with.  Each path:  every projection within 4.5 x max(1e-4, 4 x oracle fp32 rms) x
# ||g||_2 (_bs16_case's form of the three-way rule).  Composed against not:  est_fused <= 2 x est_unfused per tensor.
GRID, N_PTS = 512, 80000
# (with the resolution: 3x3 256 -> 128 / 128 -> 64 are also the first 3x3 of decoder_step2 / 3, one level up)
FUSED_TAGS = ("fwd 3x3 s1 256->128 @128x128", "fwd 3x3 s1 128->64 @256x256", "dgrad 3x3 s1 128->256 @128x128", "dgrad 3x3 s1 64->128 @256x256",
              "wgrad 3x3 s1 256->128 @128x128", "wgrad 3x3 s1 128->64 @256x256")
UNFUSED_TAGS = ("fwd 1x1 s1 256->128", "fwd 1x1 s1 128->64", "dgrad 1x1 s1 128->256", "dgrad 1x1 s1 64->128", "wgrad 1x1 s1 256->128", "wgrad 1x1 s1 128->64")
SIG = 4.5


def test_bs16_256_has_no_forward_form_for_the_composed_layers():
    """why the model-level tests do not run at the bs16_256 shape (and do at bs16_512): the library's own answer"""
    from deflow_amd import ops
    from deflow_amd._lib import DfImg, call

    def ok(n, h, w, cin, cout):
        def d(c, elt):
            return DfImg(0x10000, n, h, w, c, c, n, h * w * c, 0, elt, 0)
        return (call("df_conv2d_h2p_ok", d(cin, 2), d(cout, 0), 3, 1, ops.CONV_FWD, ops.EPI_BIAS),
                call("df_conv2d_h2p_ok", d(cout, 2), d(cin, 2), 3, 1, ops.CONV_DGRAD, ops.EPI_BIAS),
                call("df_conv2d_wgrad_h2p_ok", d(cin, 2), d(cout, 2), 3, 1))
    assert ok(16, 64, 64, 256, 128)[0] == 0 and ok(16, 128, 128, 128, 64)[0] == 0          # bs16_256
    assert ok(16, 128, 128, 256, 128) == (1, 1, 1) and ok(16, 256, 256, 128, 64) == (1, 1, 1)    # bs16_512
    assert ok(16, 80, 128, 256, 128) == (1, 1, 1) and ok(16, 160, 256, 128, 64) == (1, 1, 1)     # 320x512


def _trainer_step(dev, cfg, state, bd, fuse: str, wprep: str = "1"):
    import deflow_amd
    from deflow_amd import ops
    from deflow_amd.optim import Trainer
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DF_FUSE_U5U1", fuse)
        mp.setenv("DF_WPREP", wprep)
        mine = deflow_amd.DeFlow(**cfg)
        mine.load_state_dict(state)
        mine = mine.to(dev).train()
        tr = Trainer(mine, lr=0.0)
        prof = ops.KernelProfiler()
        mp.setattr(ops, "PROFILER", prof)
        tr.flat.zero_grad(); tr.sink.begin()
        loss = tr._forward_backward(bd)
        torch.cuda.synchronize()
    st = mine.last_state
    m0 = st["counts0"].tolist()
    return dict(loss=loss.detach().clone(), counts=m0, flow=[st["flow"][b, :m0[b]].clone() for b in range(len(m0))],
                arena=tr.flat.grad.clone(), grads={k: p.grad.clone() for k, p in mine.named_parameters()},
                tags=[r[4] for r in prof.records])


@pytest.fixture(scope="module")
def steps(dev):
    """the bs16_512 step of test_gpu_model.py::_bs16_case through the Trainer's own path (the one that holds a WeightPrep): composed,
    not composed, and not composed without the weight prep; + the float64 digests"""
    import numpy as np
    from oracle import ref_torch as O
    from deflow_amd.synth import synth_batch
    dg = dict(np.load(os.path.join(ROOT, "tests", "golden", f"bs16_{GRID}_digest.npz")))
    assert int(dg["grid"]) == GRID and int(dg["n_pts"]) == N_PTS
    B = int(dg["batch"]) if "batch" in dg else 16
    voxel = float(dg["voxel"]) if "voxel" in dg else 0.2
    half = 0.5 * voxel * GRID
    cfg = dict(voxel_size=[voxel, voxel, 6], point_cloud_range=[-half, -half, -3, half, half, 3], grid_feature_size=[GRID, GRID],
               num_iters=int(dg["iters"]) if "iters" in dg else 4)
    torch.manual_seed(int(dg["init_seed"]) if "init_seed" in dg else 16)
    state = O.DeFlow(**cfg).state_dict()          # (only the seeded initial weights: the oracle does not run here)
    batch = synth_batch(B, N_PTS, seed=int(dg["seed"]) if "seed" in dg else 4242, grid_hw=(int(round(GRID * voxel / 0.2)),) * 2,
                        exact=bool(int(dg["exact_synth"])) if "exact_synth" in dg else False)
    bd = {k: v.to(dev) for k, v in batch.items()}
    t0 = time.perf_counter()
    out = dict(dg=dg, on=_trainer_step(dev, cfg, state, bd, "1"), off=_trainer_step(dev, cfg, state, bd, "0"),
               off_nowp=_trainer_step(dev, cfg, state, bd, "0", wprep="0"))
    print(f"[fuse] three bs16_{GRID} steps: {time.perf_counter() - t0:.1f} s")
    return out


def test_composed_layers_run_and_the_1x1_layers_do_not(steps):
    on, off = steps["on"]["tags"], steps["off"]["tags"]
    for t in FUSED_TAGS:
        assert sum(x.startswith(t) for x in on) == 1, (t, [x for x in on if " s1 " in x][:40])
        assert not any(x.startswith(t) for x in off), t
    for t in UNFUSED_TAGS:
        assert not any(x.startswith(t) for x in on), t
        assert sum(x.startswith(t) for x in off) == 1, t
    assert sum(x.startswith("decompose") for x in on) == 2 and not any(x.startswith("decompose") for x in off)


def test_switch_off_is_the_unfused_step_to_the_bit(steps):
    """DF_FUSE_U5U1=0 holds no composed layer anywhere: the gradient arena, the loss and the flow equal those of the step without the
    weight prep (DF_WPREP=0: every form from the per-call kernels), which tests/test_gpu_h2p.py ties to the prep bit for bit"""
    off, ref = steps["off"], steps["off_nowp"]
    assert torch.equal(off["arena"], ref["arena"]) and torch.equal(off["loss"], ref["loss"])
    assert all(torch.equal(a, b) for a, b in zip(off["flow"], ref["flow"]))
    assert not torch.equal(off["arena"], steps["on"]["arena"])          # (and the composed step is another computation)


def test_composed_step_vs_float64_digests_and_vs_the_unfused_step(steps):
    """flow, loss and every parameter gradient of both paths against the float64 oracle's digests; per tensor the composed path's
    error estimate is at most twice the unfused path's (both paths round the same quantities once more or once less).  Both figures
    of every tensor go to the parity report (`fuse_u5u1`); the largest of each path = that path's model_error_budget figure."""
    import numpy as np
    import parity
    from oracle.gen_digest_bs16 import project
    dg = steps["dg"]
    l64, l32 = float(dg["loss64"]), float(dg["loss32"])
    est = {"on": {}, "off": {}}
    for path in ("off", "on"):
        s = steps[path]
        assert abs(float(s["loss"]) - l64) <= max(1e-4, 4 * abs(l32 - l64) / abs(l64)) * abs(l64), path
        for b, n in enumerate(s["counts"]):
            assert n == int(dg[f"flow.{b}.count"]), (path, b)
            if n:
                l2 = float(dg[f"flow.{b}.l2"])
                dp = project(f"flow.{b}", s["flow"][b]).numpy() - dg[f"flow.{b}.proj"]
                assert np.abs(dp).max() <= SIG * max(1e-4, 4 * float(dg[f"flow.{b}.e32_rms"])) * l2, (path, b)
                est[path][f"flow[{b}]"] = float(np.sqrt(np.mean(dp ** 2))) / l2
        for k, g in s["grads"].items():
            if parity.is_bn_shadowed_bias(k):
                continue
            l2 = float(dg[f"grad.{k}.l2"])
            rel = max(1e-4, 4 * float(dg[f"grad.{k}.e32_rms"]))
            dp = project("grad." + k, g).numpy() - dg[f"grad.{k}.proj"]
            dn = abs(float(g.double().norm()) - l2)
            assert np.abs(dp).max() <= SIG * rel * l2 and dn <= SIG * rel * l2, (path, k, float(np.abs(dp).max()) / l2, dn / l2, rel)
            est[path]["grad " + k] = float(np.sqrt(np.mean(dp ** 2))) / l2
    worst, bad = (0.0, ""), []
    for name, e_on in est["on"].items():
        e_off = est["off"][name]
        ratio = e_on / e_off if e_off > 0 else (0.0 if e_on == 0 else float("inf"))
        parity.record("fuse_u5u1", name, est_rms_fused_vs_fp64=e_on, est_rms_unfused_vs_fp64=e_off, ratio=ratio, bound_ratio=2.0, ok=ratio <= 2.0)
        worst = max(worst, (ratio, name))
        if ratio > 2.0:
            bad.append((name, e_on, e_off))
    print(f"[fuse] worst est(fused) / est(unfused) = {worst[0]:.2f} ({worst[1]}); largest estimated rms error vs float64: fused "
          f"{max(est['on'].values()):.2e}, unfused {max(est['off'].values()):.2e} (bound 1e-4)")
    assert not bad, bad[:8]
