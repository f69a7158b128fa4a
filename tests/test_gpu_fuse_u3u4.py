"""An UpsampleSkip block's 1x1 skip convolution u3 folded into the block's first 3x3 u4 (zero padding 1), its only reader --
ops.WeightPrep(compose_skip=...), unet._upsample_skip / run_backward, DF_FUSE_U3U4.

  * CPU, float64: the two-layer tail (u3, concatenation, zero-padded u4) against the composed form with its single bias and the border
    correction, and the five decomposed parameter gradients (+ d(b)) against autograd, on images where every one of the nine tap classes
    and both corner cases occur -- to float64 rounding
  * GPU kernels against float64 at the three channel pairs of the network on 6 x 10 and 8 x 8 images: the compose launch inside
    df_weight_prep (We, be, beta, the planes, the bias bound), df_u3u4_border_fix, df_u3u4_border_sums, df_u3u4_decompose within the bounds
    tests/test_gpu_fuse_u5u1.py holds its compose / decompose kernels to (2e-6 of max |ref|; the fp16x2 plane rule), two runs bit-equal;
    df_cat_pack_up's halves bit-identical to df_upsample2x_h2 and df_h2_pack with the same scale
  * one model and batch (bs16_512, the shape with committed float64 digests; the first two blocks take the composed layer there),
    composed against not (DF_FUSE_U3U4=0): the launch tags, every parameter gradient and the flow against the float64 digests by the
    rule of test_gpu_fuse_u5u1.py, the composed path's error estimate within a factor 2 of the other's per tensor
  * the switches: DF_FUSE_U3U4=0 runs the skip convolutions as layers again; DF_FUSE_U5U1=0 ("no composed layers") gives the same step to
    the bit whatever DF_FUSE_U3U4 says
"""
import os
import struct
import time

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONV32_MAX = 2e-6       # tests/test_gpu_fuse_u5u1.py (= tests/test_gpu_layer_census.py CONV32): of max |ref|
PAIRS = [(256, 256), (128, 128), (64, 64)]          # (outc, lat): 512 -> 256, 256 -> 128, 128 -> 64
IMAGES = [(6, 10), (8, 8)]


# ---- the algebra, in whatever dtype the operands have (float64 in every use below); weights in [O,3,3,I] memory order -----------
def outside(H: int, W: int) -> torch.Tensor:
    """[9,H,W] bool: tap (ky, kx) of a zero-padded 3x3 at pixel (y, x) falls on the padding"""
    ys, xs = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    ky, kx = (torch.arange(9) // 3).view(9, 1, 1), (torch.arange(9) % 3).view(9, 1, 1)
    yy, xx = ys + ky - 1, xs + kx - 1
    return (yy < 0) | (yy >= H) | (xx < 0) | (xx >= W)


def compose(w3, b3, w4, b4):
    lat, O = w3.shape[0], w4.shape[0]
    we = torch.cat([w4[..., :lat], torch.einsum("oyxc,ci->oyxi", w4[..., lat:], w3)], -1)
    beta = torch.einsum("oyxc,c->oyx", w4[..., lat:], b3).reshape(O, 9)
    return we, b4 + beta.sum(1), beta


def border_sub(beta, H, W):
    """[H,W,O]: what the single bias over-counts at each pixel = the sum of beta over the taps on the padding"""
    return torch.einsum("tyx,ot->yxo", outside(H, W).to(beta), beta)


def tapsums(dy):
    """dy [N,H,W,O] -> T [O,9] = sum of dy over the pixels whose tap lands inside the image"""
    return torch.einsum("tyx,nyxo->ot", (~outside(dy.shape[1], dy.shape[2])).to(dy), dy)


def decompose(w3, b3, w4, dwe, T):
    lat, O = w3.shape[0], w4.shape[0]
    dw4 = torch.cat([dwe[..., :lat], torch.einsum("ci,oyxi->oyxc", w3, dwe[..., lat:]) + b3.view(1, 1, 1, lat) * T.view(O, 3, 3, 1)], -1)
    dw3 = torch.einsum("oyxc,oyxi->ci", w4[..., lat:], dwe[..., lat:])
    db3 = torch.einsum("oyxc,oyx->c", w4[..., lat:], T.view(O, 3, 3))
    return dw4, T[:, 4].clone(), dw3, db3


@pytest.mark.parametrize("outc,lat", [(64, 64), (24, 40)])
@pytest.mark.parametrize("H,W", [(6, 10), (2, 3)])
def test_algebra_float64(outc, lat, H, W):
    g = torch.Generator().manual_seed(outc * 1000 + lat * 10 + H)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    B = 2
    w3, b3 = (0.1 * rnd(lat, lat)).requires_grad_(), rnd(lat).requires_grad_()
    w4, b4 = (0.1 * rnd(outc, 3, 3, 2 * lat)).requires_grad_(), rnd(outc).requires_grad_()
    up, b = rnd(B, lat, H, W), rnd(B, lat, H, W).requires_grad_()
    dy = rnd(B, outc, H, W)
    # the two layers: u3, concatenation, zero-padded u4
    y = F.conv2d(torch.cat([up, F.conv2d(b, w3.view(lat, lat, 1, 1), b3)], 1), w4.permute(0, 3, 1, 2), b4, padding=1)
    ref = torch.autograd.grad(y, (w4, b4, w3, b3, b), dy)
    # the composed form
    we, be, beta = compose(w3.detach(), b3.detach(), w4.detach(), b4.detach())
    we.requires_grad_()
    b2 = b.detach().clone().requires_grad_()
    y2 = F.conv2d(torch.cat([up, b2], 1), we.permute(0, 3, 1, 2), be, padding=1) - border_sub(beta, H, W).permute(2, 0, 1)
    tol = lambda r: 1e-12 * float(r.abs().max())
    assert float((y2 - y).detach().abs().max()) <= tol(y.detach())
    dwe, db = torch.autograd.grad(y2, (we, b2), dy)
    got = decompose(w3.detach(), b3.detach(), w4.detach(), dwe, tapsums(dy.permute(0, 2, 3, 1))) + (db,)
    for name, a, r in zip(("dW4", "db4", "dW3", "db3", "d(b)"), got, ref):
        assert a.shape == r.shape and float((a - r).abs().max()) <= tol(r), name
    # every tap class occurs: the nine subsets of taps on the padding at 6 x 10; at 2 x 3 also pixels that touch two opposite borders
    classes = {tuple(outside(H, W)[:, yy, xx].tolist()) for yy in range(H) for xx in range(W)}
    assert len(classes) == (9 if (H, W) == (6, 10) else 6)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _h2_scale(amax: float) -> float:
    e = (struct.unpack("<I", struct.pack("<f", amax))[0] >> 23) & 255
    return 2.0 ** (min(max(268 - e, 1), 254) - 127)


def _unpack_planes(planes, shape, amax):
    n = planes.numel() // 2
    return ((planes[:n].double() + planes[n:].double() / 2048.0) / _h2_scale(amax)).view(shape)


def _max_err(got, ref) -> float:
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _pair(outc, lat, dev, seed):
    g = torch.Generator().manual_seed(seed)
    c3, c4 = torch.nn.Conv2d(lat, lat, 1, 1, 0), torch.nn.Conv2d(2 * lat, outc, 3, 1, 1)
    with torch.no_grad():
        for p in (*c3.parameters(), *c4.parameters()):
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() == 1 else 0.05))
    c3, c4 = c3.to(dev), c4.to(dev)
    for m in (c3, c4):
        m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
    return c3, c4


def _f64(c3, c4):
    from deflow_amd import ops
    lat = c3.weight.shape[0]
    return (c3.weight.detach().double().view(lat, lat), c3.bias.detach().double(), ops.ohwi(c4.weight).double(), c4.bias.detach().double())


@pytest.mark.gpu
@pytest.mark.parametrize("outc,lat", PAIRS)
def test_compose_vs_float64(dev, outc, lat):
    from deflow_amd import ops
    c3, c4 = _pair(outc, lat, dev, 3000 + outc + lat)
    we_ref, be_ref, beta_ref = compose(*_f64(c3, c4))
    wa = torch.zeros(1, device=dev)
    wa.copy_(torch.cat([p.detach().reshape(-1) for p in (*c3.parameters(), *c4.parameters())]).abs().max().reshape(1))
    runs = []
    for _ in range(2):
        wp = ops.WeightPrep([], wa, compose_skip=[(c3, c4)])
        wp.run(wa)
        we, be, beta = wp.composed_skip(c3, c4)
        assert we.shape == (outc, 3, 3, 2 * lat) and be.shape == (outc,) and beta.shape == (outc, 9)
        wt = wp.wt(we)
        (p_w, a_w), (p_t, _) = wp.h2(we), wp.h2(wt)
        l1 = wp.l1(we, be)
        torch.cuda.synchronize()
        runs.append([t.clone() for t in (we, be, beta, wt, p_w, p_t, a_w, l1[0], l1[1])])
    we, be, beta, wt, p_w, p_t, a_w, l1w, bmax = runs[0]
    errs = dict(We=_max_err(we, we_ref), be=_max_err(be, be_ref), beta=_max_err(beta, beta_ref))
    print(f"[u3u4] compose {outc},{lat}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" of max |ref| (bound {CONV32_MAX:.0e})")
    assert all(v <= CONV32_MAX for v in errs.values()), errs
    assert torch.equal(we[..., :lat], ops.ohwi(c4.weight)[..., :lat])          # the first half: W4a itself
    # an ordinary layer of the table: transpose, planes of both with ITS scale, row L1 norm; the bias bound covers |b4| + sum |beta|
    assert torch.equal(wt, we.permute(3, 1, 2, 0))
    amax = float(a_w)
    assert amax >= float(we.abs().max()) and amax <= 2.0 * float(we.abs().max())
    for planes, src in ((p_w, we), (p_t, wt.contiguous())):
        err = (_unpack_planes(planes, src.shape, amax) - src.double()).abs()
        assert bool((err <= src.double().abs() * 2.0 ** -21 + amax * 2.0 ** -36).all()), float(err.max())
    assert abs(float(l1w) - float(we.abs().sum((1, 2, 3)).max())) <= 1e-5 * float(l1w)
    need = float((c4.bias.detach().double().abs() + beta_ref.abs().sum(1)).max())
    assert need <= float(bmax) <= need * (1 + 1e-5) and float(bmax) >= float(be.abs().max())
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", IMAGES)
@pytest.mark.parametrize("outc,lat", PAIRS)
def test_border_kernels_and_decompose_vs_float64(dev, outc, lat, H, W):
    from deflow_amd import ops
    from deflow_amd._lib import call, img, ptr, stream
    c3, c4 = _pair(outc, lat, dev, 4000 + outc + lat + H)
    w3, b3, w4, b4 = _f64(c3, c4)
    beta_ref = compose(w3, b3, w4, b4)[2]
    g = torch.Generator().manual_seed(H * 100 + W + outc)
    N = 2
    # -- border fix: the border pixels of a pre-split image lose the beta of the taps on the padding; the interior is not touched
    y = (3.0 * torch.randn(N, H, W, outc, generator=g)).to(dev)
    beta = beta_ref.float().contiguous()
    bound = torch.full((1,), float(y.abs().max()) + float(beta_ref.abs().sum(1).max()), device=dev)
    outs = []
    for _ in range(2):
        yh = ops.h2_pack(y, bound)
        before = ops.h2_unpack(yh)
        call("df_u3u4_border_fix", img(yh), ptr(bound), ptr(beta), stream())
        after = ops.h2_unpack(yh)
        torch.cuda.synchronize()
        outs.append((yh.clone(), after))
    ref = before.double() - border_sub(beta.double(), H, W).to(dev)
    e = _max_err(after, ref)
    print(f"[u3u4] border fix {outc} ch {H}x{W}: {e:.2e} of max |ref| (bound {CONV32_MAX:.0e})")
    assert e <= CONV32_MAX and float(after.abs().max()) <= float(bound)
    assert torch.equal(after[:, 1:-1, 1:-1], before[:, 1:-1, 1:-1]) and not torch.equal(after[:, 0], before[:, 0])
    assert torch.equal(outs[0][0], outs[1][0])
    # -- border sums and the decomposition
    dyf = torch.randn(N, H, W, outc, generator=g).to(dev)
    dbound = torch.full((1,), 1.5 * float(dyf.abs().max()), device=dev)
    dyh = ops.h2_pack(dyf, dbound)
    dy = ops.h2_unpack(dyh).double()          # the values the kernels read
    dbe = dy.sum((0, 1, 2)).float()
    dwe = torch.randn(outc, 3, 3, 2 * lat, generator=g).to(dev)
    w3t = ops.weight_transpose(ops.ohwi(c3.weight))
    assert torch.equal(w3t.view(lat, lat), c3.weight.detach().view(lat, lat).t())
    outs = []
    for _ in range(2):
        part = torch.full((8, N, outc), 7.0, dtype=torch.float64, device=dev)
        T = torch.full((outc, 9), 7.0, dtype=torch.float64, device=dev)
        call("df_u3u4_border_sums", img(dyh), ptr(dbound), ptr(dbe), ptr(part), ptr(T), stream())
        dw4, db4 = torch.full((outc, 3, 3, 2 * lat), 7.0, device=dev), torch.full((outc,), 7.0, device=dev)
        dw3, db3 = torch.full((lat, lat), 7.0, device=dev), torch.full((lat,), 7.0, device=dev)
        call("df_u3u4_decompose", ptr(w3t), ptr(ops.ohwi(c4.weight)), ptr(c3.bias.detach()), ptr(dwe), ptr(T), outc, lat,
             ptr(dw4), ptr(db4), ptr(dw3), ptr(db3), stream())
        torch.cuda.synchronize()
        outs.append((part, T, dw4, db4, dw3, db3))
    part, T, dw4, db4, dw3, db3 = outs[0]
    part_ref = torch.stack([dy[:, 0].sum(1), dy[:, -1].sum(1), dy[:, :, 0].sum(1), dy[:, :, -1].sum(1),
                            dy[:, 0, 0], dy[:, 0, -1], dy[:, -1, 0], dy[:, -1, -1]])
    T_ref = tapsums(dy.cpu()).to(dev)
    refs = dict(part=part_ref, T=T_ref, **dict(zip(("dW4", "db4", "dW3", "db3"), decompose(w3.to(dev), b3.to(dev), w4.to(dev), dwe.double(), T_ref))))
    for (name, r), got in zip(refs.items(), (part, T, dw4, db4, dw3, db3)):
        e = _max_err(got, r)
        print(f"[u3u4] decompose {outc},{lat} {H}x{W}: {name} {e:.2e} of max |ref| (bound {CONV32_MAX:.0e})")
        assert e <= CONV32_MAX, (name, e)
    assert torch.equal(dw4[..., :lat], dwe[..., :lat])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("H,W", IMAGES)
@pytest.mark.parametrize("lat", [256, 128, 64])
def test_pack_kernel_halves_bit_identical(dev, lat, H, W, ac):
    from deflow_amd import ops
    from deflow_amd._lib import call, img, ptr, stream
    g = torch.Generator().manual_seed(lat + H * 10 + W + int(ac))
    N = 2
    t = torch.randn(N, H // 2, W // 2, lat, generator=g).to(dev)
    b = (2.0 * torch.randn(N, H, W, lat, generator=g)).to(dev)
    bound = torch.full((1,), max(float(t.abs().max()), float(b.abs().max())), device=dev)
    ref = ops.h2_empty((N, H, W, 2 * lat), dev, bound)
    ref.fill_(7.0)
    ops.upsample2x(img(t), img(ref, lat, 0), ac)                                   # df_upsample2x_h2 into the first half's planes
    call("df_h2_pack", img(b), ptr(bound), img(ref, lat, lat), stream())          # df_h2_pack into the second half's
    got = ops.h2_empty((N, H, W, 2 * lat), dev, bound)
    got.fill_(7.0)
    ops.upsample2x(img(t), img(got, lat, 0), ac, pack=img(b))
    torch.cuda.synchronize()
    assert torch.equal(got, ref), float((ops.h2_unpack(got) - ops.h2_unpack(ref)).abs().max())
    assert torch.equal(ops.h2_unpack(got)[..., lat:], ops.h2_unpack(ops.h2_pack(b, bound)))


# ---- one model and batch, composed against not: the bs16_512 step (tests/test_gpu_fuse_u5u1.py explains the shape and the rule) ---
GRID, N_PTS = 512, 80000
ON_TAGS = ("pack + bilinear x2 512 ch @128x128", "pack + bilinear x2 256 ch @256x256", "border fix 256 ch @128x128", "border fix 128 ch @256x256",
           "border sums 256 ch @128x128", "border sums 128 ch @256x256", "u3u4 decompose 1x1 256->256", "u3u4 decompose 1x1 128->128")
OFF_TAGS = ("fwd 1x1 s1 256->256", "fwd 1x1 s1 128->128", "dgrad 1x1 s1 256->256", "dgrad 1x1 s1 128->128", "wgrad 1x1 s1 256->256",
            "wgrad 1x1 s1 128->128")
BOTH_TAGS = ("fwd 3x3 s1 512->256 @128x128", "fwd 3x3 s1 256->128 @256x256", "dgrad 3x3 s1 256->512 @128x128", "dgrad 3x3 s1 128->256 @256x256",
             "wgrad 3x3 s1 512->256 @128x128", "wgrad 3x3 s1 256->128 @256x256", "fwd 1x1 s1 64->64", "wgrad 1x1 s1 64->64")
SIG = 4.5


def _trainer_step(dev, cfg, state, bd, env):
    import deflow_amd
    from deflow_amd import ops
    from deflow_amd.optim import Trainer
    with pytest.MonkeyPatch.context() as mp:
        for k in ("DF_FUSE_U3U4", "DF_FUSE_U5U1"):
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
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
    out = dict(dg=dg, on=_trainer_step(dev, cfg, state, bd, {}), off=_trainer_step(dev, cfg, state, bd, {"DF_FUSE_U3U4": "0"}),
               none=_trainer_step(dev, cfg, state, bd, {"DF_FUSE_U5U1": "0"}),
               none_both=_trainer_step(dev, cfg, state, bd, {"DF_FUSE_U5U1": "0", "DF_FUSE_U3U4": "0"}))
    print(f"[u3u4] four bs16_{GRID} steps: {time.perf_counter() - t0:.1f} s")
    return out


@pytest.mark.gpu
def test_composed_layers_run_and_the_skip_convolutions_do_not(steps):
    on, off = steps["on"]["tags"], steps["off"]["tags"]
    for t in ON_TAGS:
        assert sum(x.startswith(t) for x in on) == 1, (t, [x for x in on if "u3u4" in x or "border" in x or "pack" in x])
        assert not any(x.startswith(t) for x in off), t
    for t in OFF_TAGS:
        assert not any(x.startswith(t) for x in on), t
        assert sum(x.startswith(t) for x in off) == 1, t
    for t in BOTH_TAGS:         # the 3x3 layers keep their shapes; the last block keeps its skip convolution
        assert sum(x.startswith(t) for x in on) == 1 and sum(x.startswith(t) for x in off) == 1, t


@pytest.mark.gpu
def test_switches(steps):
    """DF_FUSE_U3U4=0 is another computation than the composed step; under DF_FUSE_U5U1=0 (no composed layers: the step
    tests/test_gpu_fuse_u5u1.py ties to the one without a weight prep, bit for bit) DF_FUSE_U3U4 changes nothing"""
    on, off, a, b = (steps[k] for k in ("on", "off", "none", "none_both"))
    assert not torch.equal(on["arena"], off["arena"])
    assert torch.equal(a["arena"], b["arena"]) and torch.equal(a["loss"], b["loss"])
    assert all(torch.equal(x, y) for x, y in zip(a["flow"], b["flow"]))
    assert a["tags"] == b["tags"] and not any("u3u4" in x or x.startswith("pack") for x in a["tags"])


@pytest.mark.gpu
def test_composed_step_vs_float64_digests_and_vs_the_uncomposed_step(steps):
    """flow, loss and every parameter gradient of both paths against the float64 oracle's digests (test_gpu_fuse_u5u1.py's rule); per
    tensor the composed path's error estimate is at most twice the other's"""
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
            print(f"[u3u4] {path} {k}: max proj err {float(np.abs(dp).max()) / l2:.2e} norm err {dn / l2:.2e} (bound {SIG * rel:.2e})")
            assert np.abs(dp).max() <= SIG * rel * l2 and dn <= SIG * rel * l2, (path, k, float(np.abs(dp).max()) / l2, dn / l2, rel)
            est[path]["grad " + k] = float(np.sqrt(np.mean(dp ** 2))) / l2
    worst, bad = (0.0, ""), []
    for name, e_on in est["on"].items():
        e_off = est["off"][name]
        ratio = e_on / e_off if e_off > 0 else (0.0 if e_on == 0 else float("inf"))
        parity.record("fuse_u3u4", name, est_rms_fused_vs_fp64=e_on, est_rms_unfused_vs_fp64=e_off, ratio=ratio, bound_ratio=2.0, ok=ratio <= 2.0)
        worst = max(worst, (ratio, name))
        if ratio > 2.0:
            bad.append((name, e_on, e_off))
    print(f"[u3u4] worst est(composed) / est(not) = {worst[0]:.2f} ({worst[1]}); largest estimated rms error vs float64: composed "
          f"{max(est['on'].values()):.2e}, not {max(est['off'].values()):.2e} (bound 1e-4)")
    assert not bad, bad[:8]
