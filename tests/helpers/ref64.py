"""Float64 restatements of what each UNet layer computes: the references of the layer census (tests/test_gpu_layer_census.py),
themselves checked against torch autograd by tests/test_ref64.py.

Plain torch, NHWC tensors in and out, on whatever device the operands live on (the GPU computes them in float64): a k x k
convolution is k * k shifted GEMMs, chunked by image so that no temporary exceeds ~2^25 elements.  Weights are LOGICAL [O, I, kh, kw]
tensors (any memory format).  `rnd` is the operand-rounding hook: None = the fp32 values as stored; `bf16_rne` = each operand
rounded to bfloat16 round-to-nearest-even exactly as the bf16-operand kernels read it (biases, BatchNorm scales and shifts stay
fp32: the kernels apply them in fp32 registers); the arithmetic after the hook is float64 either way.

The comparison at the end (`errors` / `Bounds.ok`) is what the census asserts with; tests/test_ref64.py shows on synthetic tensors
that it flags the errors one wrong layer makes (a shifted tile, a scaled channel, a missing image, a small channel that is wholly
wrong)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Optional

import torch
import torch.nn.functional as F

_CHUNK = 1 << 25


def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """the value a bf16-operand kernel reads: RNE to bfloat16 (torch's cast rounds to nearest even)"""
    return t.detach().float().to(torch.bfloat16)


def operand(t: torch.Tensor, rnd: Optional[Callable] = None, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    t = t.detach()
    return (t if rnd is None else rnd(t)).to(dtype)


def _imgs_per_chunk(n: int, pixels: int, width: int) -> int:
    return max(1, min(n, _CHUNK // max(1, pixels * width)))


def _out_hw(h: int, w: int, k: int, stride: int):
    p = k // 2
    return (h + 2 * p - k) // stride + 1, (w + 2 * p - k) // stride + 1


def _tap(t: torch.Tensor, ky: int, kx: int, ho: int, wo: int, stride: int) -> torch.Tensor:
    """the [n, ho, wo, C] window of a padded NHWC tensor that tap (ky, kx) of a stride-`stride` convolution reads"""
    return t[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride, :]


def _pad(x: torch.Tensor, p: int) -> torch.Tensor:
    return F.pad(x, (0, 0, p, p, p, p)) if p else x


# ---------------------------------------------------------------------------------------------------------- convolutions ----
def conv2d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1, rnd=None,
           dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """y = conv(x; w) + bias, padding k // 2 (the UNet's 1x1 and 3x3 layers, stride 1 or 2).  x [n,h,w,ci] -> [n,ho,wo,co]"""
    x, w = operand(x, rnd, dtype), operand(w, rnd, dtype)
    n, h, wd, ci = x.shape
    co, _, k, _ = w.shape
    ho, wo = _out_hw(h, wd, k, stride)
    xp = _pad(x, k // 2)
    y = x.new_zeros(n, ho, wo, co)
    step = _imgs_per_chunk(n, ho * wo, max(ci, co))
    for i in range(0, n, step):
        for ky in range(k):
            for kx in range(k):
                y[i:i + step] += _tap(xp[i:i + step], ky, kx, ho, wo, stride) @ w[:, :, ky, kx].T
    if bias is not None:
        y += bias.detach().to(dtype)
    return y


def conv2d_dgrad(dy: torch.Tensor, w: torch.Tensor, hw, stride: int = 1, rnd=None, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """data gradient of conv2d: dx [n,h,w,ci] for the output gradient dy [n,ho,wo,co]; hw = (h, w) of the input (stride 2 with an
    odd size: the last row / column receives no tap of the window that would start past the end)"""
    dy, w = operand(dy, rnd, dtype), operand(w, rnd, dtype)
    n, ho, wo, co = dy.shape
    _, ci, k, _ = w.shape
    h, wd = hw
    p = k // 2
    assert _out_hw(h, wd, k, stride) == (ho, wo)
    dxp = dy.new_zeros(n, h + 2 * p, wd + 2 * p, ci)
    step = _imgs_per_chunk(n, ho * wo, max(ci, co))
    for i in range(0, n, step):
        for ky in range(k):
            for kx in range(k):
                _tap(dxp[i:i + step], ky, kx, ho, wo, stride).add_(dy[i:i + step] @ w[:, :, ky, kx])
    return dxp[:, p:p + h, p:p + wd, :]


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, k: int, stride: int = 1, rnd=None, dtype: torch.dtype = torch.float64):
    """-> (dw [co,ci,k,k], db [co]) = the weight and bias gradients of conv2d for input x and output gradient dy"""
    x, dy = operand(x, rnd, dtype), operand(dy, rnd, dtype)
    n, h, wd, ci = x.shape
    _, ho, wo, co = dy.shape
    assert _out_hw(h, wd, k, stride) == (ho, wo)
    xp = _pad(x, k // 2)
    dw = x.new_zeros(co, ci, k, k)
    step = _imgs_per_chunk(n, ho * wo, max(ci, co))
    for i in range(0, n, step):
        d2 = dy[i:i + step].reshape(-1, co).T
        for ky in range(k):
            for kx in range(k):
                dw[:, :, ky, kx] += d2 @ _tap(xp[i:i + step], ky, kx, ho, wo, stride).reshape(-1, ci)
    return dw, dy.sum((0, 1, 2))


# ------------------------------------------------------------------------------------------------------ BatchNorm + GELU ----
def gelu(u: torch.Tensor) -> torch.Tensor:
    """exact (erf) GELU, as nn.GELU() and the kernels' df_gelu"""
    return 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))


def gelu_grad(u: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _groups(t: torch.Tensor, groups: int) -> torch.Tensor:
    """[n,h,w,C] -> [groups, rows per group, C]: statistic group g = images g * n / groups ... (g + 1) * n / groups - 1 (the two
    clouds' images of the shared encoder, unet._cwn_forward)"""
    return t.reshape(groups, -1, t.shape[-1])


def bn_stats(y: torch.Tensor, groups: int = 1):
    """-> (mean, biased variance), each [groups, C]: two passes in float64 over the values as stored"""
    yg = _groups(y.detach().double(), groups)
    mean = yg.mean(1)
    return mean, ((yg - mean[:, None]) ** 2).mean(1)


def bn_running_update(rmean: torch.Tensor, rvar: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, count: int, momentum: float):
    """running statistics after a training forward whose groups were successive calls of the module (unbiased variance)"""
    rm, rv = rmean.detach().double().clone(), rvar.detach().double().clone()
    for g in range(mean.shape[0]):
        rm = (1.0 - momentum) * rm + momentum * mean[g]
        rv = (1.0 - momentum) * rv + momentum * var[g] * (count / (count - 1.0))
    return rm, rv


def bn_fold_train(mean, var, gamma, beta, eps: float):
    """batch statistics -> (scale, shift, invstd), each [groups, C]"""
    invstd = torch.rsqrt(var + eps)
    scale = gamma.detach().double() * invstd
    return scale, beta.detach().double() - mean * scale, invstd


def bn_fold_eval(gamma, beta, rmean, rvar, eps: float):
    """eval mode: the running statistics folded into one scale and shift per channel"""
    invstd = torch.rsqrt(rvar.detach().double() + eps)
    scale = gamma.detach().double() * invstd
    return scale, beta.detach().double() - rmean.detach().double() * scale


def _per_group(v: torch.Tensor, groups: int) -> torch.Tensor:
    v = v.detach().double()
    return (v.reshape(1, -1) if v.dim() == 1 else v).expand(groups, -1)[:, None, :]


def bn_gelu(y: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, groups: int = 1, rnd=None) -> torch.Tensor:
    """z = gelu(y * scale + shift) with per-group [groups, C] (or shared [C]) scale and shift"""
    yg = _groups(operand(y, rnd), groups)
    return gelu(yg * _per_group(scale, groups) + _per_group(shift, groups)).reshape(y.shape)


def bn_gelu_bwd(dz: torch.Tensor, y: torch.Tensor, scale, shift, mean, invstd, groups: int = 1, frozen: bool = False):
    """backward of z = gelu(bn(y)) with the statistics the forward normalised with ([groups, C] each; `frozen`: eval-mode BatchNorm,
    whose statistics are constants).  -> (dy, dgamma, dbeta): dgamma = sum g * xhat, dbeta = sum g, g = dz * gelu'(y * scale + shift),
    dy = scale * (g - mean_group(g) - xhat * mean_group(g * xhat)) (train) or scale * g (frozen)"""
    yg, dzg = _groups(y.detach().double(), groups), _groups(dz.detach().double(), groups)
    sc, sh = _per_group(scale, groups), _per_group(shift, groups)
    xhat = (yg - _per_group(mean, groups)) * _per_group(invstd, groups)
    g = dzg * gelu_grad(yg * sc + sh)
    gx = g * xhat
    dy = g if frozen else g - g.mean(1, keepdim=True) - xhat * gx.mean(1, keepdim=True)
    return (sc * dy).reshape(y.shape), gx.sum((0, 1)), g.sum((0, 1))


# ----------------------------------------------------------------------------------------------------------- bilinear x2 ----
def interp_matrix(n: int, align_corners: bool, device=None) -> torch.Tensor:
    """[2n, n] float64 matrix of the 1-D linear x2 upsampling (torch's source-index rule)"""
    a = torch.zeros(2 * n, n, dtype=torch.float64)
    for o in range(2 * n):
        if align_corners:
            src = o * (n - 1) / (2 * n - 1) if n > 1 else 0.0
        else:
            src = max(0.5 * (o + 0.5) - 0.5, 0.0)
        i0 = min(int(math.floor(src)), n - 1)
        i1 = min(i0 + 1, n - 1)
        lam = src - i0
        a[o, i0] += 1.0 - lam
        a[o, i1] += lam
    return a.to(device)


def upsample2x(x: torch.Tensor, align_corners: bool) -> torch.Tensor:
    """bilinear x2 of an NHWC tensor (any strides: a channel slice of a concatenation reads as it is)"""
    x = x.detach().double()
    ah, aw = interp_matrix(x.shape[1], align_corners, x.device), interp_matrix(x.shape[2], align_corners, x.device)
    return torch.einsum("ph,nhwc,qw->npqc", ah, x, aw)


def upsample2x_bwd(dy: torch.Tensor, align_corners: bool) -> torch.Tensor:
    """gradient of upsample2x: dy [n,2h,2w,c] -> dx [n,h,w,c]"""
    dy = dy.detach().double()
    ah = interp_matrix(dy.shape[1] // 2, align_corners, dy.device)
    aw = interp_matrix(dy.shape[2] // 2, align_corners, dy.device)
    return torch.einsum("ph,npqc,qw->nhwc", ah, dy, aw)


# ---------------------------------------------------------------------------------------------------- sparse edge kernels ----
# (dtype: the arithmetic, float64 unless a test asks for the reference's own fp32 error on the CPU -- tests/helpers/sparse_cases.py)
def cells(keys: torch.Tensor, h: int, w: int):
    """sorted cell keys (b * h * w + row * w + col) -> (b, row, col) index tensors"""
    k = keys.long()
    return k // (h * w), (k % (h * w)) // w, k % w


def sparse_conv3x3(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], keys: torch.Tensor, rnd=None,
                   dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """df_sparse_conv3x3 / _h2 / _bf16: the 3x3 stride-1 convolution evaluated at the listed cells only -> [ncells, co] (row j = cell
    keys[j]); the dense convolution restricted to those cells"""
    x, w = operand(x, rnd, dtype), operand(w, rnd, dtype)
    n, h, wd, _ = x.shape
    b, r, c = cells(keys, h, wd)
    xp = _pad(x, 1)
    y = x.new_zeros(b.numel(), w.shape[0])
    for ky in range(3):
        for kx in range(3):
            y += xp[b, r + ky, c + kx] @ w[:, :, ky, kx].T
    return y if bias is None else y + bias.detach().to(dtype)


def sparse_wgrad3x3(x: torch.Tensor, dy: torch.Tensor, keys: torch.Tensor, dtype: torch.dtype = torch.float64):
    """df_sparse_wgrad3x3 / _x2: weight and bias gradients of the 3x3 stride-1 convolution whose output gradient is non-zero at the
    listed cells only -> (dw [co,ci,3,3], db [co])"""
    x, dy = operand(x, None, dtype), operand(dy, None, dtype)
    n, h, wd, ci = x.shape
    b, r, c = cells(keys, h, wd)
    d = dy[b, r, c]                                  # [ncells, co]
    xp = _pad(x, 1)
    dw = x.new_zeros(dy.shape[-1], ci, 3, 3)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = d.T @ xp[b, r + ky, c + kx]
    return dw, d.sum(0)


def occupancy(keys: torch.Tensor, n: int, h: int, w: int, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """[n,h,w,1] float64 mask of the listed cells"""
    m = torch.zeros(n * h * w, dtype=dtype, device=keys.device)
    m[keys.long()] = 1.0
    return m.view(n, h, w, 1)


def sparse_in_wgrad(x: torch.Tensor, dy: torch.Tensor, keys: torch.Tensor, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """df_sparse_in_wgrad: weight gradient of the first encoder conv (3x3 stride 2) of one cloud, summed over the occupied input
    cells only (x = that cloud's [B,H,W,32] canvas view, dy its [B,H/2,W/2,64] output gradient) -> dw [co,ci,3,3]"""
    n, h, w, _ = x.shape
    return conv2d_wgrad(operand(x, None, dtype) * occupancy(keys, n, h, w, dtype), dy, 3, 2, dtype=dtype)[0]


def pillar_input_grad(dy1: torch.Tensor, w1: torch.Tensor, dskip: torch.Tensor, w3: torch.Tensor, keys: torch.Tensor,
                      dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """df_pillar_input_grad: d(canvas) of one cloud at the occupied cells = data gradient of the first encoder conv (3x3 stride 2, w1)
    + data gradient of the skip conv on the canvas (1x1, w3 [lat, 64, 1, 1], this cloud's 32 input channels) -> [ncells, 32]"""
    n, h, w, _ = dskip.shape
    d = conv2d_dgrad(dy1, w1, (h, w), 2, dtype=dtype) + conv2d_dgrad(dskip, w3, (h, w), 1, dtype=dtype)
    b, r, c = cells(keys, h, w)
    return d[b, r, c]


# ------------------------------------------------------------------------------------------------------------ comparison ----
def errors(got: torch.Tensor, ref: torch.Tensor, ch_dim: int = -1, ch_floor: float = 1e-3) -> dict:
    """max |got - ref| / max |ref|, ||got - ref|| / ||ref||, and the worst per-channel rms-relative error among the channels (along
    ch_dim) that hold at least ch_floor of the tensor's norm; non-finite values in got make every figure inf"""
    got, ref = got.detach().double().to(ref.device), ref.detach().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return {"max": math.inf, "rms": math.inf, "ch": math.inf, "ch_idx": -1, "finite": False}
    d = got - ref
    rn = float(ref.norm())
    out = {"max": float(d.abs().max() / ref.abs().max().clamp_min(1e-300)), "rms": float(d.norm()) / max(rn, 1e-300),
           "ch": 0.0, "ch_idx": -1, "finite": True}
    if ref.dim() > 1:
        rc = ref.movedim(ch_dim, 0).reshape(ref.shape[ch_dim], -1).norm(dim=1)
        dc = d.movedim(ch_dim, 0).reshape(ref.shape[ch_dim], -1).norm(dim=1)
        sel = rc >= ch_floor * rn
        if bool(sel.any()):
            rel = torch.where(sel, dc / rc.clamp_min(1e-300), torch.zeros_like(dc))
            out["ch"], out["ch_idx"] = float(rel.max()), int(rel.argmax())
    return out


@dataclass(frozen=True)
class Bounds:
    """what a layer's output must meet: max-abs / max|ref|, rms-relative, per-channel rms-relative"""
    max: float
    rms: float
    ch: float

    def ok(self, e: dict) -> bool:
        return e["finite"] and e["max"] <= self.max and e["rms"] <= self.rms and e["ch"] <= self.ch


def bf16_ulp(v: torch.Tensor) -> torch.Tensor:
    """one bf16 ulp at |v| (8 significant bits): 2^(floor(log2 |v|) - 7)"""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(1e-300))) - 7.0)


def bf16_excess(got: torch.Tensor, ref: torch.Tensor, floor: float) -> float:
    """the bf16-storage rule (tests/test_gpu_kernels.py::test_conv_w16_bf16_storage): a bf16 output lies within one bf16 ulp of the
    reference -> max over elements of |got - ref| / ulp(max(|ref|, floor * max|ref|)) (<= 1 passes); the floor covers results that are
    cancellations, whose fp32 accumulation noise is not small against the result itself"""
    got, ref = got.detach().double().to(ref.device), ref.detach().double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    scale = ref.abs().clamp_min(floor * float(ref.abs().max()))
    return float(((got - ref).abs() / bf16_ulp(scale)).max())
