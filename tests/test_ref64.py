"""CPU: the float64 layer references of the census (tests/helpers/ref64.py) against torch autograd in float64 at small odd shapes,
and negative tests of the census' comparison on synthetic tensors -- it must flag the errors one wrong layer makes."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref64 as R  # noqa: E402

D = torch.float64


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


def close(got, want, tol=1e-12):
    got, want = got.detach(), want.detach()
    assert got.shape == want.shape, (got.shape, want.shape)
    e = float((got - want).abs().max() / want.abs().max().clamp_min(1e-300))
    assert e <= tol, e


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# cin, cout, k, stride, n, h, w: 1x1 and 3x3, stride 1 and 2, odd and even extents
# (the last two: the stride-2 geometries of tests/helpers/conv_cases.py -- the last window starts on the last row and column of a 9 x 13
# image; 9 x 67 -> 5 x 34)
CONV = [(5, 7, 3, 1, 2, 9, 11), (6, 4, 3, 2, 3, 9, 7), (6, 4, 3, 2, 1, 10, 8), (8, 3, 1, 1, 2, 5, 7), (3, 5, 1, 2, 2, 7, 5),
        (4, 6, 3, 2, 2, 9, 13), (3, 4, 3, 2, 2, 9, 67)]


@pytest.mark.parametrize("ci,co,k,s,n,h,w", CONV)
def test_conv_forward_and_gradients_vs_autograd(ci, co, k, s, n, h, w):
    g = _gen(ci * 31 + co + k * 7 + s + h)
    x = torch.randn(n, h, w, ci, generator=g, dtype=D)
    wt = torch.randn(co, ci, k, k, generator=g, dtype=D, requires_grad=True)
    b = torch.randn(co, generator=g, dtype=D, requires_grad=True)
    xr = nchw(x).clone().requires_grad_(True)
    y = F.conv2d(xr, wt, b, stride=s, padding=k // 2)
    close(R.conv2d(x, wt, b, s), nhwc(y))
    dy = torch.randn(y.shape, generator=g, dtype=D)
    y.backward(dy)
    close(R.conv2d_dgrad(nhwc(dy), wt, (h, w), s), nhwc(xr.grad))
    dw, db = R.conv2d_wgrad(x, nhwc(dy), k, s)
    close(dw, wt.grad)
    close(db, b.grad)


def test_conv_dtype_argument():
    """dtype = float32: the same functions evaluated in float32 (the yardstick of the case tables' bounds), operands and bias included"""
    g = _gen(9)
    x, wt, b = torch.randn(2, 9, 13, 8, generator=g), torch.randn(6, 8, 3, 3, generator=g), torch.randn(6, generator=g)
    dy = torch.randn(2, 5, 7, 6, generator=g)
    for f32, f64 in ((R.conv2d(x, wt, b, 2, dtype=torch.float32), R.conv2d(x, wt, b, 2)),
                     (R.conv2d_dgrad(dy, wt, (9, 13), 2, dtype=torch.float32), R.conv2d_dgrad(dy, wt, (9, 13), 2)),
                     (R.conv2d_wgrad(x, dy, 3, 2, dtype=torch.float32)[0], R.conv2d_wgrad(x, dy, 3, 2)[0])):
        assert f32.dtype == torch.float32 and f64.dtype == D
        e = float((f32.double() - f64).abs().max() / f64.abs().max())
        assert 0.0 < e <= 1e-5, e
    close(R.conv2d(x, wt, b, 2, rnd=R.bf16_rne, dtype=torch.float32).double(), R.conv2d(x, wt, b, 2, rnd=R.bf16_rne), 1e-5)


def test_conv_chunking_by_image(monkeypatch):
    """the image chunks (bounded temporaries) change nothing"""
    g = _gen(3)
    x, wt, dy = torch.randn(5, 6, 7, 4, generator=g, dtype=D), torch.randn(3, 4, 3, 3, generator=g, dtype=D), torch.randn(5, 3, 4, 3, generator=g, dtype=D)
    whole = (R.conv2d(x, wt, None, 2), R.conv2d_dgrad(dy, wt, (6, 7), 2), R.conv2d_wgrad(x, dy, 3, 2)[0])
    monkeypatch.setattr(R, "_CHUNK", 1)        # one image per chunk
    close(R.conv2d(x, wt, None, 2), whole[0])
    close(R.conv2d_dgrad(dy, wt, (6, 7), 2), whole[1])
    close(R.conv2d_wgrad(x, dy, 3, 2)[0], whole[2])


def test_conv_reads_channel_slices_and_pair_views():
    """operands as the census hands them over: a channel slice of a concatenation, and the two clouds' halves stacked as 2B images"""
    g = _gen(5)
    cat = torch.randn(2, 7, 9, 10, generator=g, dtype=D)
    wt = torch.randn(3, 4, 3, 3, generator=g, dtype=D)
    close(R.conv2d(cat[..., 6:], wt), nhwc(F.conv2d(nchw(cat[..., 6:].contiguous()), wt, padding=1)))
    pair = torch.cat([cat[..., :5], cat[..., 5:]], 0)             # image (cloud, b) = cloud * B + b
    w5 = torch.randn(3, 5, 3, 3, generator=g, dtype=D)
    close(R.conv2d(pair, w5, None, 2), nhwc(F.conv2d(nchw(pair), w5, stride=2, padding=1)))


def test_bf16_operand_hook():
    """rnd = bf16_rne: both operands rounded RNE to bfloat16, then float64 arithmetic; the bias is not rounded"""
    g = _gen(7)
    x, wt, b = torch.randn(2, 5, 6, 8, generator=g), torch.randn(4, 8, 3, 3, generator=g), torch.randn(4, generator=g)
    want = nhwc(F.conv2d(nchw(x).to(torch.bfloat16).double(), wt.to(torch.bfloat16).double(), b.double(), padding=1))
    close(R.conv2d(x, wt, b, rnd=R.bf16_rne), want)
    assert float((R.conv2d(x, wt, b) - want).abs().max()) > 1e-4      # (the hook does something)
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8)])      # ties: to even
    assert R.bf16_rne(v).double().tolist() == [1.0, 1.0 + 2 * 2.0 ** -7, -1.0]


def _bn_gelu_autograd(y, gamma, beta, groups, eps, train, rmean=None, rvar=None, momentum=0.1):
    """the reference module: BatchNorm2d (one call per group, as the two clouds' encoder calls) + exact GELU, in float64 autograd"""
    outs = []
    for yg in nchw(y).chunk(groups, 0):
        outs.append(F.gelu(F.batch_norm(yg, rmean, rvar, gamma, beta, train, momentum, eps), approximate="none"))
    return nhwc(torch.cat(outs, 0))


@pytest.mark.parametrize("groups", [1, 2])
def test_bn_gelu_train_vs_autograd(groups):
    g = _gen(11 + groups)
    n, h, w, C, eps, mom = 2 * groups, 5, 3, 6, 1e-5, 0.1
    y = (torch.randn(n, h, w, C, generator=g, dtype=D) * 2 + 0.5).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=D) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=D).requires_grad_(True)
    rm0, rv0 = torch.randn(C, generator=g, dtype=D), torch.rand(C, generator=g, dtype=D) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    z = _bn_gelu_autograd(y, gamma, beta, groups, eps, True, rm, rv, mom)
    mean, var = R.bn_stats(y, groups)
    scale, shift, invstd = R.bn_fold_train(mean, var, gamma, beta, eps)
    close(R.bn_gelu(y, scale, shift, groups), z)
    rm_r, rv_r = R.bn_running_update(rm0, rv0, mean, var, n // groups * h * w, mom)
    close(rm_r, rm)
    close(rv_r, rv)
    dz = torch.randn(z.shape, generator=g, dtype=D)
    z.backward(dz)
    dy, dgamma, dbeta = R.bn_gelu_bwd(dz, y, scale, shift, mean, invstd, groups)
    close(dy, y.grad, 1e-11)
    close(dgamma, gamma.grad)
    close(dbeta, beta.grad)


def test_bn_gelu_eval_and_frozen_backward_vs_autograd():
    g = _gen(13)
    n, h, w, C, eps = 3, 4, 5, 7, 1e-5
    y = torch.randn(n, h, w, C, generator=g, dtype=D).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=D) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=D).requires_grad_(True)
    rm, rv = torch.randn(C, generator=g, dtype=D), torch.rand(C, generator=g, dtype=D) + 0.5
    z = _bn_gelu_autograd(y, gamma, beta, 1, eps, False, rm, rv)
    scale, shift = R.bn_fold_eval(gamma, beta, rm, rv, eps)
    close(R.bn_gelu(y, scale, shift), z)
    dz = torch.randn(z.shape, generator=g, dtype=D)
    z.backward(dz)
    dy, dgamma, dbeta = R.bn_gelu_bwd(dz, y, scale, shift, rm, torch.rsqrt(rv + eps), 1, frozen=True)
    close(dy, y.grad)
    close(dgamma, gamma.grad)
    close(dbeta, beta.grad)


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("h,w", [(3, 5), (1, 4), (4, 4)])
def test_upsample2x_vs_interpolate(ac, h, w):
    """forward into / backward out of a channel slice of a concatenation, both align_corners values"""
    g = _gen(17 + h * w + ac)
    t = torch.randn(2, h, w, 4, generator=g, dtype=D, requires_grad=True)
    cat = torch.randn(2, 2 * h, 2 * w, 9, generator=g, dtype=D)
    up = nhwc(F.interpolate(nchw(t), scale_factor=2, mode="bilinear", align_corners=ac))
    cat_view = cat[..., 3:7]                       # the slice the upsampled half occupies
    close(R.upsample2x(t, ac), up)
    d = torch.randn(up.shape, generator=g, dtype=D)
    cat[..., 3:7] = d
    up.backward(d)
    close(R.upsample2x_bwd(cat_view, ac), t.grad)


def _keys(n, h, w, count, seed):
    g = _gen(seed)
    return torch.sort(torch.randperm(n * h * w, generator=g)[:count])[0].to(torch.int32)


def test_sparse_references_are_the_dense_layers_at_the_cells():
    g = _gen(19)
    n, h, w = 2, 6, 10
    keys = _keys(n, h, w, 37, 1)
    b, r, c = R.cells(keys, h, w)
    x = torch.randn(n, h, w, 5, generator=g, dtype=D)
    wt = torch.randn(4, 5, 3, 3, generator=g, dtype=D, requires_grad=True)
    bias = torch.randn(4, generator=g, dtype=D, requires_grad=True)
    y = nhwc(F.conv2d(nchw(x), wt, bias, padding=1))
    close(R.sparse_conv3x3(x, wt, bias, keys), y[b, r, c])
    occ = R.occupancy(keys, n, h, w)
    dy = torch.randn(y.shape, generator=g, dtype=D) * occ          # the gather backward: non-zero at the cells only
    y.backward(dy)
    dw, db = R.sparse_wgrad3x3(x, dy, keys)
    close(dw, wt.grad)
    close(db, bias.grad)


def test_canvas_gradient_references_vs_autograd():
    """the first encoder conv (3x3 stride 2, 32 -> 64 channels here 4 -> 6) and the skip conv (1x1) both read one cloud's canvas:
    weight gradient over the occupied cells, input gradient at the occupied cells"""
    g = _gen(23)
    n, h, w, ci = 2, 8, 6, 4
    keys = _keys(n, h, w, 21, 2)
    occ = R.occupancy(keys, n, h, w)
    canvas = (torch.randn(n, h, w, ci, generator=g, dtype=D) * occ).requires_grad_(True)
    w1 = torch.randn(6, ci, 3, 3, generator=g, dtype=D, requires_grad=True)
    w3 = torch.randn(5, ci, 1, 1, generator=g, dtype=D)
    y1 = F.conv2d(nchw(canvas), w1, stride=2, padding=1)
    ys = F.conv2d(nchw(canvas), w3)
    dy1, dskip = torch.randn(y1.shape, generator=g, dtype=D), torch.randn(ys.shape, generator=g, dtype=D)
    (y1 * dy1).sum().add((ys * dskip).sum()).backward()
    noisy = canvas.detach() + (1 - occ) * 7.0          # values outside the cells must not count
    close(R.sparse_in_wgrad(noisy, nhwc(dy1), keys), w1.grad)
    b, r, c = R.cells(keys, h, w)
    close(R.pillar_input_grad(nhwc(dy1), w1, nhwc(dskip), w3, keys), canvas.grad[b, r, c])


# ------------------------------------------------------------------------------------ the comparison flags a wrong layer ----
FP32 = R.Bounds(max=2e-6, rms=2e-6, ch=2e-5)      # the census' bounds of the fp16x2 / x3 convolutions (test_gpu_layer_census.py)


def _noisy(ref, rel, seed):
    """ref + fp32-product-sized noise: what a correct kernel returns"""
    g = _gen(seed)
    return ref + torch.randn(ref.shape, generator=g, dtype=D) * rel * ref.abs().max() / 4


def test_comparison_passes_a_correct_output():
    g = _gen(29)
    ref = torch.randn(4, 16, 16, 64, generator=g, dtype=D)
    e = R.errors(_noisy(ref, 1e-7, 1), ref)
    assert FP32.ok(e), e


def test_comparison_flags_one_shifted_tile():
    """one 64-row tile of the [rows, C] output off by 1e-5 of max |y|"""
    g = _gen(31)
    ref = torch.randn(4, 16, 16, 64, generator=g, dtype=D)
    got = _noisy(ref, 1e-7, 2).reshape(-1, 64)
    got[5 * 64:6 * 64] += 1e-5 * float(ref.abs().max())
    e = R.errors(got.reshape(ref.shape), ref)
    assert not FP32.ok(e) and e["max"] > FP32.max, e


def test_comparison_flags_one_scaled_weight_gradient_channel():
    """one output channel of a weight gradient [O,I,kh,kw] scaled by (1 + 1e-4); the channel is one of the smaller ones"""
    g = _gen(37)
    ref = torch.randn(64, 64, 3, 3, generator=g, dtype=D) * torch.logspace(0, -3, 64, dtype=D).view(64, 1, 1, 1)
    got = _noisy(ref, 1e-7, 3)
    got[50] *= 1 + 1e-4
    e = R.errors(got, ref, ch_dim=0)
    assert e["max"] <= FP32.max                       # (the max-norm alone would not see it)
    assert not FP32.ok(e) and e["ch_idx"] == 50, e


def test_comparison_flags_a_missing_image():
    """a weight gradient that left one of the 2B images out of its sum"""
    g = _gen(41)
    x, dy = torch.randn(8, 9, 9, 6, generator=g, dtype=D), torch.randn(8, 9, 9, 5, generator=g, dtype=D)
    want, _ = R.conv2d_wgrad(x, dy, 3)
    got, _ = R.conv2d_wgrad(x[1:], dy[1:], 3)
    e = R.errors(got, want, ch_dim=0)
    assert not FP32.ok(e), e


def test_comparison_flags_a_small_wholly_wrong_channel():
    """a channel holding 1e-3 of the tensor's norm whose every value is wrong (here: another channel's values at its scale)"""
    g = _gen(43)
    ref = torch.randn(2, 8, 8, 64, generator=g, dtype=D)
    ref[..., 9] *= 1.001e-3 * float(ref.norm()) / float(ref[..., 9].norm())
    got = _noisy(ref, 1e-7, 4)
    got[..., 9] = ref[..., 10] * float(ref[..., 9].norm() / ref[..., 10].norm())
    e = R.errors(got, ref)
    assert e["rms"] < 2e-3 and not FP32.ok(e) and e["ch_idx"] == 9 and e["ch"] > 0.5, e


def test_comparison_flags_non_finite_values():
    ref = torch.ones(2, 3, 3, 4, dtype=D)
    got = ref.clone()
    got[1, 2, 0, 3] = float("nan")
    assert not FP32.ok(R.errors(got, ref))


def test_bf16_rule():
    """within one bf16 ulp of the reference: the RNE-rounded reference passes, two ulps off does not"""
    g = _gen(47)
    ref = torch.randn(1000, generator=g, dtype=D)
    assert R.bf16_excess(ref.float().to(torch.bfloat16), ref, 2.0 ** -8) <= 0.5 + 1e-9
    off = (ref.float().to(torch.bfloat16).double() + 2 * R.bf16_ulp(ref)).float()
    assert R.bf16_excess(off, ref, 2.0 ** -8) > 1.0
