"""The elementwise kernels' cases that are computed twice: by tests/test_gpu_elementwise_cases.py in its own process (the default,
eight-channel forms) and by this file run as a script in ONE fresh child process with DF_UP8=0 DF_BN_X8=0 (the four-channel forms,
documented as bit-identical; the library reads both switches once per process).  The script saves every output under the path it is
given; the parent asserts torch.equal.

Inputs are drawn on the device from seeded generators, so both processes hold the same values.  Outputs of pre-split ("h2") tensors
are returned as the int32 view of their storage (fp16 planes read as float32 may be NaN bit patterns, which never compare equal).
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import ref64 as R  # noqa: E402

SENTINEL = -512.0               # exact in float32 and bfloat16
SENTINEL_BITS = 0x7FC1A5A5      # for pre-split storage, compared as int32
EPS = 1e-5

# name -> (n, h, w, C, groups, channel offset of z inside its buffer, buffer width)
PRESPLIT_APPLY = {
    "c32": (3, 5, 7, 32, 3, 32, 64),            # h*w = 35, C/8 = 4; written into the upper half of a 64-wide pre-split buffer
    "c96": (3, 5, 7, 96, 3, 0, 96),             # C/8 = 12
    # 1 048 576 < n*h*w*C/8 = 1 593 000 < 2 097 152: the capped grid (4096 blocks x 256 threads) loops, and the second unrolled element
    # group holds a real element for the first 544 424 threads and the clamped repeat for the others
    "big": (3, 250, 177, 96, 3, 0, 96),
}
BILINEAR_SHAPES = [(1, 1, 1, 8), (2, 1, 9, 8), (2, 7, 1, 16), (3, 5, 9, 12), (2, 6, 10, 40)]
BILINEAR_H2 = {"h2c32": (2, 5, 9, 32, 0, 64), "h2c96": (2, 3, 7, 96, 96, 192)}       # n, h, w, C, channel offset, buffer width


def gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def randn(shape, g, dev):
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)


def bn_inputs(n, h, w, C, groups, dev, seed, dtype=torch.float32):
    """-> y [n,h,w,C] (dtype), gamma, beta, bn_ss [groups,4,C] float32 = (scale, shift, mean, invstd) of the float64 batch statistics
    of the values as stored"""
    g = gen(dev, seed)
    y = (randn((n, h, w, C), g, dev) * (0.5 + 2.0 * torch.rand(C, generator=g, device=dev)) + randn((C,), g, dev)).to(dtype)
    gamma, beta = torch.rand(C, generator=g, device=dev) + 0.5, randn((C,), g, dev) * 0.3
    mean, var = R.bn_stats(y, groups)
    scale, shift, invstd = R.bn_fold_train(mean, var, gamma, beta, EPS)
    bn_ss = torch.stack([scale, shift, mean, invstd], 1).float().contiguous()
    return y, gamma, beta, bn_ss


def h2_buffer(shape, dev, bound):
    """a pre-split buffer whose storage holds SENTINEL_BITS everywhere"""
    from deflow_amd import ops
    t = ops.h2_empty(shape, dev, bound)
    t.view(torch.int32).fill_(SENTINEL_BITS)
    return t


def presplit_apply(name, dev):
    """-> dict(y, bn_ss, ipg, bound, buf = the pre-split buffer, c_off, C)"""
    from deflow_amd import ops
    from deflow_amd._lib import img
    n, h, w, C, groups, c_off, width = PRESPLIT_APPLY[name]
    y, _, _, bn_ss = bn_inputs(n, h, w, C, groups, dev, 1000 + C + h)
    # the bound df_bn_finalize2 derives: max_c |scale_c| max|y| + |shift_c|
    bound = (bn_ss[:, 0].abs() * y.abs().max() + bn_ss[:, 1].abs()).max().reshape(1).contiguous()
    buf = h2_buffer((n, h, w, width), dev, bound)
    ops.bn_gelu_apply(y, bn_ss, n // groups, img(buf, C, c_off))
    torch.cuda.synchronize()
    return dict(y=y, bn_ss=bn_ss, ipg=n // groups, groups=groups, bound=bound, buf=buf, c_off=c_off, C=C)


def bilinear_input(shape, dev):
    n, h, w, C = shape
    return randn(shape, gen(dev, 7 + n + 10 * h + 100 * w + 1000 * C), dev)


def bilinear_plain(shape, ac, dev):
    """contiguous fp32 forward and backward -> (x, y, dy, dx)"""
    from deflow_amd import ops
    from deflow_amd._lib import img
    n, h, w, C = shape
    x = bilinear_input(shape, dev)
    y = torch.full((n, 2 * h, 2 * w, C), SENTINEL, device=dev)
    ops.upsample2x(img(x), img(y), ac)
    dy = randn((n, 2 * h, 2 * w, C), gen(dev, 99 + C + h), dev)
    dx = torch.full((n, h, w, C), SENTINEL, device=dev)
    ops.upsample2x_bwd(img(dy), img(dx), ac)
    torch.cuda.synchronize()
    return x, y, dy, dx


def bilinear_ld20(ac, dev):
    """8 channels at offset 12 of 20-wide buffers (rows 4-aligned, not 8-aligned): forward into the view; backward from a view into a view
    -> (x, ycat, dycat, dxcat)"""
    from deflow_amd import ops
    from deflow_amd._lib import img
    n, h, w, C = 2, 5, 9, 8
    x = bilinear_input((n, h, w, C), dev)
    ycat = torch.full((n, 2 * h, 2 * w, 20), SENTINEL, device=dev)
    ops.upsample2x(img(x), img(ycat, C, 12), ac)
    dycat = randn((n, 2 * h, 2 * w, 20), gen(dev, 5), dev)
    dxcat = torch.full((n, h, w, 20), SENTINEL, device=dev)
    ops.upsample2x_bwd(img(dycat, C, 12), img(dxcat, C, 12), ac)
    torch.cuda.synchronize()
    return x, ycat, dycat, dxcat


def bilinear_bf16_out(ac, dev):
    """fp32 input, bfloat16 output (the bf16-storage mode's concatenation): 40 channels at offset 8 of a 48-wide buffer -> (x, ycat)"""
    from deflow_amd import ops
    from deflow_amd._lib import img
    shape = (2, 6, 10, 40)
    x = bilinear_input(shape, dev)
    ycat = torch.full((2, 12, 20, 48), SENTINEL, dtype=torch.bfloat16, device=dev)
    ops.upsample2x(img(x), img(ycat, 40, 8), ac)
    torch.cuda.synchronize()
    return x, ycat


def bilinear_h2(name, ac, dev):
    """pre-split output into a channel slice of a pre-split concatenation whose bound is 1.7 max |x| -> (x, buf, c_off, C)"""
    from deflow_amd import ops
    from deflow_amd._lib import img
    n, h, w, C, c_off, width = BILINEAR_H2[name]
    x = bilinear_input((n, h, w, C), dev)
    bound = (x.abs().max() * 1.7).reshape(1).contiguous()
    buf = h2_buffer((n, 2 * h, 2 * w, width), dev, bound)
    ops.upsample2x(img(x), img(buf, C, c_off), ac)
    torch.cuda.synchronize()
    return x, buf, c_off, C


def shape_key(shape):
    return "x".join(str(v) for v in shape)


def apply_outputs(dev):
    return {f"apply_{name}": presplit_apply(name, dev)["buf"].view(torch.int32).cpu() for name in PRESPLIT_APPLY}


def bilinear_outputs(dev):
    """every bilinear output the four-channel and the eight-channel forms must agree on to the bit: {name: cpu tensor}"""
    out = {}
    for ac in (False, True):
        for shape in BILINEAR_SHAPES:
            _, y, _, dx = bilinear_plain(shape, ac, dev)
            out[f"up_{shape_key(shape)}_ac{int(ac)}"] = y.cpu()
            out[f"upbwd_{shape_key(shape)}_ac{int(ac)}"] = dx.cpu()
        _, ycat, _, dxcat = bilinear_ld20(ac, dev)
        out[f"up_ld20_ac{int(ac)}"], out[f"upbwd_ld20_ac{int(ac)}"] = ycat.cpu(), dxcat.cpu()
        out[f"up_bf16_ac{int(ac)}"] = bilinear_bf16_out(ac, dev)[1].cpu()
        for name in BILINEAR_H2:
            out[f"up_{name}_ac{int(ac)}"] = bilinear_h2(name, ac, dev)[1].view(torch.int32).cpu()
    return out


if __name__ == "__main__":
    assert os.environ.get("DF_UP8") == "0" and os.environ.get("DF_BN_X8") == "0", "run with DF_UP8=0 DF_BN_X8=0 (the four-channel forms)"
    assert torch.cuda.is_available()
    torch.save({**apply_outputs(torch.device("cuda")), **bilinear_outputs(torch.device("cuda"))}, sys.argv[1])
    print("saved", sys.argv[1])
