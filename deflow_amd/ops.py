"""Thin tensor-level wrappers over the C ABI (include/deflow_amd.h).  Every function launches HIP kernels on
torch's current stream with raw device pointers; nothing here computes with torch ops."""
from __future__ import annotations

import ctypes
import os

from typing import Optional, Tuple

import torch

from ._lib import DfImg, call, img, ptr, stream, ver

CONV_FWD, CONV_DGRAD = 0, 1
EPI_BIAS, EPI_STATS, EPI_BN_GELU = 0, 1, 2


def _f32(*shape, device) -> torch.Tensor:
    return torch.empty(shape, dtype=torch.float32, device=device)


def ohwi(w: torch.Tensor) -> torch.Tensor:
    """Conv weight [O,I,kh,kw] -> contiguous [O,kh,kw,I] memory (free when the parameter is channels_last)."""
    v = w.detach().permute(0, 2, 3, 1)
    if v.is_contiguous():
        v._df_keep = True       # a VIEW of the parameter: stable address, shared version counter -- the per-tensor caches may key on it
        return v
    # a parameter that is NOT channels_last (a plain nn.Module nobody converted): the contiguous copy is kept while the parameter is
    # unchanged, so that its transposes / fp16 planes are too (one copy per parameter, replaced when an optimizer writes it)
    try:
        key, epoch = (w.data_ptr(), tuple(w.shape)), (w._version, WEIGHT_GEN[0])
    except RuntimeError:
        return v.contiguous()
    hit = _OHWI_CACHE.get(key)
    if hit is not None and hit[1] == epoch:
        return hit[0]
    c = v.contiguous()
    c._df_keep = True
    if hit is not None:         # the superseded copy's transpose and planes go with it
        ck = (hit[0].data_ptr(), tuple(hit[0].shape))
        old_t = _WT_CACHE.pop(ck, None)
        if old_t is not None:
            _PLANE_CACHE.pop((old_t[0].data_ptr(), tuple(old_t[0].shape)), None)
        _PLANE_CACHE.pop(ck, None)
    if len(_OHWI_CACHE) > 256:
        _OHWI_CACHE.clear()
    _OHWI_CACHE[key] = (c, epoch, w)
    return c


_OHWI_CACHE: dict = {}


class KernelProfiler:
    """Optional per-launch HIP-event timing of the hot kernels (bench.py's live roofline figures).  Events are
    recorded on the stream the kernels are launched on (torch's current stream)."""

    def __init__(self):
        self.records = []  # (kernel / stage name, algorithmic flops, start event, end event, layer tag[, algorithmic bytes[, moved bytes]])

    def summary(self):
        out = {}
        for name, flops, e0, e1, _tag, *rest in self.records:
            d = out.setdefault(name, {"launches": 0, "flops": 0.0, "ms": 0.0, "bytes": 0.0, "moved": 0.0})
            d["launches"] += 1
            d["flops"] += flops
            d["bytes"] += rest[0] if rest else 0.0
            d["moved"] += rest[1] if len(rest) > 1 else 0.0
            d["ms"] += e0.elapsed_time(e1)
        return out


PROFILER: Optional[KernelProfiler] = None

# BatchNorm's num_batches_tracked counters: 18 one-element `add_` launches per training forward when done layer by layer.  Inside
# `deferred_tracked()` (DeFlow._run) the increments are collected and applied by ONE multi-tensor launch at the end of the forward.
_TRACKED: Optional[list] = None


def bump_tracked(t: torch.Tensor, k: int) -> None:
    if _TRACKED is None:
        t.add_(k)
    else:
        _TRACKED.append((t, int(k)))


class deferred_tracked:
    def __enter__(self):
        global _TRACKED
        self.prev = _TRACKED
        _TRACKED = []
        return self

    def __exit__(self, *exc):
        global _TRACKED
        pend, _TRACKED = _TRACKED, self.prev
        if pend:
            acc: dict = {}          # (a tensor may come twice -- the feature net's counter, once per cloud: one entry each for the launch)
            for t, k in pend:
                e = acc.setdefault(id(t), [t, 0])
                e[1] += k
            torch._foreach_add_([e[0] for e in acc.values()], [e[1] for e in acc.values()])
        return False

# Mixed-precision switch of the convolution kernels (forward, data gradient, weight gradient): True = MFMA operands rounded
# to bf16 as they leave LDS, fp32 accumulation, all tensors still fp32 (df_conv2d_mp / df_conv2d_wgrad_mp).  Set by
# optim.Trainer(dtype="bf16") around its forward + backward (BASELINE configs[4]: "bf16 MFMA" training); False everywhere else.
MFMA_BF16 = False


# bf16 STORAGE on top of the bf16-operand mode (round 3; on with Trainer(dtype="bf16") unless DF_BF16_STORE=0): inside the UNet
# encoder the conv outputs y, the activations z, and the gradients dz / dy of every 3x3 stride-1 ConvWithNorms layer live in
# HBM as bfloat16 (BatchNorm statistics from the fp32 accumulators' rounded values, normalisation / GELU / their backward in
# fp32 registers) -- the BatchNorm + GELU passes and the conv I/O move half the bytes, and the weight gradient reads bf16 tiles
# with transposing LDS reads (csrc/conv_wgrad.hip wgrad3_tr_kernel).  Stage inputs / outputs (the skip tensors) stay fp32.
BF16_STORE = False


class mfma_bf16:
    """with ops.mfma_bf16(True[, store=True]): ...  -- scoped form of the switches above"""

    def __init__(self, on: bool, store: bool = False):
        self.on, self.store = bool(on), bool(on) and bool(store)

    def __enter__(self):
        global MFMA_BF16, BF16_STORE
        self.prev, MFMA_BF16 = MFMA_BF16, self.on
        self.prev_store, BF16_STORE = BF16_STORE, self.store
        return self

    def __exit__(self, *exc):
        global MFMA_BF16, BF16_STORE
        MFMA_BF16 = self.prev
        BF16_STORE = self.prev_store
        return False


class timed:
    """with ops.timed("stage", bytes=..., flops=...): HIP events around a launch (or a short chain of launches) on the current
    stream when a KernelProfiler is installed; free otherwise.  `bytes` / `flops` are the ALGORITHMIC figures of DESIGN.md
    section 4 (what the stage has to move / compute), not what the implementation happens to do; `moved` (optional) = the bytes the
    implementation is KNOWN to stream through HBM by construction (e.g. the GRU kernels' saved planes), reported beside them."""

    def __init__(self, name: str, bytes: float = 0.0, flops: float = 0.0, tag: str = "", moved: float = 0.0):
        self.name, self.bytes, self.flops, self.tag, self.moved = name, float(bytes), float(flops), tag, float(moved)
        self.prof = PROFILER

    def __enter__(self):
        if self.prof is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.prof is not None and exc[0] is None:
            self.e1.record()
            self.prof.records.append((self.name, self.flops, self.e0, self.e1, self.tag, self.bytes, self.moved))
        return False


class SideStream:
    """Second HIP stream for the weight-gradient GEMMs of the backward pass.  They depend only on a layer's input and
    output gradient, nothing on the critical path (data gradients -> next layer) depends on them until the optimizer, so
    they run concurrently with the HBM-bound normalisation / activation backward kernels and fill the MFMA pipe while
    those stream.  `keep` pins every tensor a side-stream kernel reads until the main stream has joined (the caching
    allocator would otherwise hand the blocks to later main-stream allocations)."""

    def __init__(self, device):
        self.stream = torch.cuda.Stream(device=device)
        self.keep: list = []

    def fork(self):
        """context manager: work enqueued inside runs on the side stream, after everything enqueued so far on main"""
        ev = torch.cuda.Event()
        ev.record()
        self.stream.wait_event(ev)
        return torch.cuda.stream(self.stream)

    def join(self):
        torch.cuda.current_stream().wait_stream(self.stream)
        self.keep.clear()


SIDE: Optional[SideStream] = None
_SIDE_CACHE: dict = {}


class side_stream:
    """with ops.side_stream(on, device): ...  -- the backward inside puts its weight-gradient GEMMs on the second stream (on =
    True), keeps them on the main stream (False), or leaves the process-wide setting alone (None).  optim.Trainer turns it on
    for dtype="bf16" on one GPU: in that mode no kernel saturates the matrix pipe, so two streams overlap (52.2 -> 49.2 ms per
    step); the fp32 step, MFMA-bound end to end, loses 1 % to it and keeps one stream."""

    def __init__(self, on: Optional[bool], device=None):
        self.on, self.device = on, device

    def __enter__(self):
        global SIDE
        self.prev = SIDE
        if self.on is True:
            key = str(self.device)
            if key not in _SIDE_CACHE:
                _SIDE_CACHE[key] = SideStream(self.device)
            SIDE = _SIDE_CACHE[key]
        elif self.on is False:
            SIDE = None
        return self

    def __exit__(self, *exc):
        global SIDE
        SIDE = self.prev
        return False


W_F32, W_B16, W_X3, W_H2, W_WP, W_F32_H2 = range(6)                               # DF_CONV_W_*: the kind of weights a conv entry point takes
FAM_REG, FAM_DMA, FAM_HALO, FAM_HALO_W16, FAM_HALO_X3, FAM_HALO_X3P = range(6)      # DF_CONV_FAM_*
PLAN_XP, PLAN_X16, PLAN_BWS, PLAN_DMA, PLAN_CLS = 1, 2, 4, 8, 16                    # DF_CONV_PLAN_*: bits of the plan's flags word


def conv_plan(x: DfImg, y: DfImg, ks: int, stride: int, mode: int, epi: int, weights: int) -> tuple:
    """what the library's dispatch decides for the call (df_conv2d_plan; host side, nothing is launched): -> (family, BM, BN, WM, WN, SEG,
    DB, planes, flags, stats_mul); raises where the launch would be refused"""
    out = (ctypes.c_int32 * 10)()
    call("df_conv2d_plan", x, y, ks, stride, mode, epi, weights, ctypes.addressof(out))
    return tuple(out)


def _conv_label(x: DfImg, y: DfImg, ks: int, stride: int, mode: int, epi: int, form: str, h2f: bool) -> str:
    """profiler label of the launch conv2d made in `form`, formatted from the library's plan -- bench.py's roofline and the layer census
    match on these strings.  The DMA-tile forms carry the fp32 instance's name, `/h2` marking fp16x2 products on the 128-row tiles; the
    persistent plane kernels carry conv_halo_x3_kernel's"""
    weights = {"w16": W_B16, "x3": W_X3, "h2": W_H2, "h2p": W_H2, "dgrad_bn": W_H2}.get(form, W_F32)
    fam, bm, bn, wm, wn, seg, db, planes, flags, _ = conv_plan(x, y, ks, stride, mode, 3 if form == "dgrad_bn" else epi, weights)
    if fam in (FAM_HALO_X3, FAM_HALO_X3P):
        np = {3: "", 2: ",2", 1: f",1,{'true' if flags & PLAN_X16 else 'false'}"}[planes]
        return f"conv_halo_x3_kernel<{bm},{bn},{wm},{wn},{seg},{db}{np}{',xp' if flags & PLAN_XP else ''}>"
    if fam == FAM_HALO_W16:
        return f"conv_halo_w16_kernel<{bn},{wm},{wn},{seg}>"
    if fam == FAM_HALO:
        return f"conv_halo_kernel<{bn},{wm},{wn}>"
    if fam == FAM_DMA:
        return f"conv_dma_kernel<{bm},{bn},{wm},{wn}>" + ("/h2" if h2f and bm == 128 else "")
    return f"conv_kernel<{bm},{bn},{wm},{wn}>"


# ---- max |x| bookkeeping of the fp16x2 convolution kernels (df_conv2d_h2 / df_conv2d_wgrad_h2) -------------------------------
# The kernels scale each operand by a power of two taken from an UPPER BOUND of its absolute maximum (a device scalar, so nothing
# here synchronises); any bound within a factor of ~2^10 serves.  Where the bound comes from:
#   activations / gradients  written by the BatchNorm + GELU passes: measured by those kernels as they write (bn_gelu_apply,
#                            bn_gelu_bwd); everything else: one df_absmax pass the first time a convolution reads the tensor,
#                            remembered on the descriptor / tensor object (the tape keeps it for the weight gradient)
#   weights                  ops.W_AMAX when a Trainer set it (one df_absmax over the whole parameter arena per step), else
#                            per call
# Slots come zero-filled from a small pool (one fill per _AMAX_POOL_N slots; amax_pool_reset() starts a fresh pool -- the Trainer
# does so at the top of every step, inside a captured step too, so that a replay re-zeroes what it accumulates into).
_AMAX_POOL_N = 256
_amax_pool = [None, 0]
W_AMAX: Optional[torch.Tensor] = None


def amax_pool_reset():
    _amax_pool[0] = None


def amax_slot(device) -> torch.Tensor:
    if _amax_pool[0] is None or _amax_pool[1] >= _AMAX_POOL_N or _amax_pool[0].device != torch.device(device):
        _amax_pool[0] = torch.zeros(_AMAX_POOL_N, dtype=torch.float32, device=device)
        _amax_pool[1] = 0
    i = _amax_pool[1]
    _amax_pool[1] = i + 1
    return _amax_pool[0][i:i + 1]


def amax_of(d: DfImg, device) -> torch.Tensor:
    """device scalar >= max |x| of the image view: the producer's measurement if it left one, else one df_absmax pass"""
    a = getattr(d, "_amax", None)
    if a is None:
        a = amax_slot(device)
        call("df_absmax", d, ptr(a), stream())
        d._amax = a
        src = getattr(d, "_src", None)
        if src is not None:               # whole-tensor view: the next descriptor made of the tensor finds the measurement (_lib.img)
            src._df_amax = (a, ver(src))
    return a


def wrote(t: torch.Tensor) -> None:
    """a kernel wrote (accumulated into) t through a raw pointer, without measuring: whatever bound t carried is no longer one
    (the kernels leave torch's version counter alone, so the record would otherwise stay 'valid' -- ADVICE r3)"""
    if getattr(t, "_df_amax", None) is not None:
        t._df_amax = None


def _h2_on() -> bool:
    return os.environ.get("DF_CONV_H2", "1") != "0"


# ---- PRE-SPLIT ("h2") tensors, round 4 (include/deflow_amd.h "PRE-SPLIT tensors"; csrc/elementwise.hip) -------------------------
# An activation / gradient whose only consumers are the fp16x2 3x3 convolution and weight-gradient kernels is stored by its PRODUCER as
# two scaled fp16 planes (the bytes of the fp32 tensor), with the scale taken from a bound of max |x| that is known before the producer
# writes: BatchNorm + GELU outputs from the statistics (df_bn_finalize2 / df_bn_bwd_finalize2), plain convolution outputs from
# max |input| x the largest L1 norm of a weight row (+ max |bias|).  The consumers then fetch their operands by LDS-DMA with no
# in-kernel split (conv_halo_x3_kernel<.., XP>, wgrad3_h2p_kernel).  DF_H2P=0 keeps every tensor fp32 (round 3's data flow).
def h2p_on() -> bool:
    return h2_active() and os.environ.get("DF_H2P", "1") != "0"


def h2_empty(shape, device, bound: torch.Tensor) -> torch.Tensor:
    """storage of an h2 image [N,H,W,C] (C % 32 == 0): float32-typed memory holding per pixel and 32-channel chunk [32 fp16 hi | 32
    fp16 lo]; `bound` = the device scalar that defines its power-of-two scale (every producer and consumer takes THIS tensor)."""
    assert shape[-1] % 32 == 0
    t = torch.empty(shape, dtype=torch.float32, device=device)
    t._df_h2 = bound
    return t


def h2_unpack(t: torch.Tensor) -> torch.Tensor:
    """fp32 copy of an h2 tensor (tests / debugging)"""
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    call("df_h2_unpack", img(t), ptr(t._df_h2), img(out), stream())
    return out


def h2_pack(x: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    t = h2_empty(x.shape, x.device, bound)
    call("df_h2_pack", img(x), ptr(bound), img(t), stream())
    return t


def fuse_u5u1_on() -> bool:
    """DF_FUSE_U5U1=0: no composed layers -- every UpsampleSkip block runs its last 3x3 and the next block its 1x1 (unet._upsample_skip)"""
    return os.environ.get("DF_FUSE_U5U1", "1") != "0"


def fuse_u3u4_on() -> bool:
    """DF_FUSE_U3U4=0 (or DF_FUSE_U5U1=0: no composed layers at all): every UpsampleSkip block runs its 1x1 skip convolution as a layer
    instead of folded into the block's first 3x3 (unet._upsample_skip)"""
    return fuse_u5u1_on() and os.environ.get("DF_FUSE_U3U4", "1") != "0"


class WeightPrep:
    """Every convolution layer's per-step weight forms from ONE launch (df_weight_prep; round 4): transposed weights, [hi | lo] fp16
    planes of the weights and of their transpose (every layer: the 3x3 stride-1 kernels and, since the round's second session, the
    1x1 / stride-2 kernel read them), row L1 norms and max |bias| (a-priori bounds of pre-split outputs).  optim.Trainer builds one at the top of every step (the parameters change once per step) and installs it as
    ops.WPREP; ops.weight_transpose / _split_h2 / rows_l1max answer from it when the tensor they are asked about is one of its
    layers, and fall back to their own launches otherwise (plain autograd users, the decoder head's GEMM weights)."""

    def __init__(self, convs, w_amax: torch.Tensor, compose=(), compose_skip=()):
        """compose: (conv5, conv1) pairs -- a 3x3 layer and the 1x1 layer that is its only reader, with nothing in between (an UpsampleSkip
        block's last convolution and the next block's first): the prep then also holds the ONE 3x3 layer  conv1 o conv5  as an ordinary
        layer (weights We [O,kh,kw,I] and bias be in its own storage: self.composed), made by the compose launch inside df_weight_prep.
        DF_FUSE_U5U1=0: none.
        compose_skip: (conv3, conv4) pairs -- an UpsampleSkip block's 1x1 skip convolution and the block's first 3x3, whose second half of
        input channels is its only reader: the prep then also holds the ONE 3x3 layer of conv4's shape that reads [up(t) | b] instead of
        [up(t) | conv3(b)] (self.composed_skip: We, be and the per-tap bias terms beta the border correction needs).  DF_FUSE_U3U4=0: none."""
        import numpy as np
        self.convs = [m for m in convs if m.weight.dim() == 4]
        self.compose = [(m5, m1) for m5, m1 in compose] if fuse_u5u1_on() else []
        self.compose_skip = [(m3, m4) for m3, m4 in compose_skip] if fuse_u3u4_on() else []
        srcs = [m for pair in self.compose + self.compose_skip for m in pair]
        assert all(m.bias is not None for m in srcs)
        dev = (self.convs + srcs)[0].weight.device
        ws = [ohwi(m.weight) for m in self.convs]
        assert all(w.data_ptr() == m.weight.data_ptr() for w, m in zip(ws, self.convs)), "conv weights must be channels_last (OHWI memory)"
        assert all(ohwi(m.weight).data_ptr() == m.weight.data_ptr() for m in srcs), "conv weights must be channels_last (OHWI memory)"
        ptrs = [w.data_ptr() for w in ws] + [m.bias.data_ptr() for m in self.convs if m.bias is not None]
        ptrs += [m.weight.data_ptr() for m in srcs] + [m.bias.data_ptr() for m in srcs]
        self.base = min(ptrs)
        nc, ns = len(self.compose), len(self.compose_skip)
        nl = len(ws) + nc + ns      # ordinary records (the composed layers among them); their source records follow
        rec = np.zeros(nl + nc + ns, dtype=[("w_off", "<i8"), ("b_off", "<i8"), ("wt_off", "<i8"), ("w2_off", "<i8"), ("wt2_off", "<i8"),
                                       ("cout", "<i4"), ("taps", "<i4"), ("cin", "<i4"), ("split", "<i4"), ("blk0", "<i4"), ("pad", "<i4")])
        off, blk = 0, 0
        self.layer = {}
        for i, (w, m) in enumerate(zip(ws, self.convs)):
            co, kh, kw, ci = w.shape
            n = w.numel()
            split = 1      # (round 4, second session: the 1x1 / stride-2 layers read pre-split weights too: conv_dma_kernel<.., H2, BP>)
            rec[i] = ((w.data_ptr() - self.base) // 4, (m.bias.data_ptr() - self.base) // 4 if m.bias is not None else -1,
                      off, off + n, off + 2 * n, co, kh * kw, ci, split, blk, 0)
            self.layer[w.data_ptr()] = (i, off, n, (co, kh, kw, ci), split)
            off += 3 * n if split else n
            blk += co + ci
        comp = []
        for k, (m5, m1) in enumerate(self.compose):
            i = len(ws) + k
            c5, kh, kw, ci = ohwi(m5.weight).shape
            co = m1.weight.shape[0]
            assert tuple(m1.weight.shape) == (co, c5, 1, 1) and co % 8 == 0 and m5.stride == (1, 1) and m1.stride == (1, 1)
            n = co * kh * kw * ci
            we_off, be_off = off, off + n
            off += n + (co + 63) // 64 * 64
            rec[i] = (we_off, be_off, off, off + n, off + 2 * n, co, kh * kw, ci, 1, blk, nl + k)
            rec[nl + k] = ((m5.weight.data_ptr() - self.base) // 4, (m5.bias.data_ptr() - self.base) // 4, (m1.weight.data_ptr() - self.base) // 4,
                           (m1.bias.data_ptr() - self.base) // 4, 3 * nl + k, c5, kh * kw, ci, co, 2 ** 31 - 1, 0)
            comp.append((i, we_off, be_off, off, n, (co, kh, kw, ci)))
            off += 3 * n
            blk += co + ci
        for k, (m3, m4) in enumerate(self.compose_skip):
            i = len(ws) + nc + k
            co, kh, kw, ci = ohwi(m4.weight).shape
            lat = m3.weight.shape[0]
            assert (tuple(m3.weight.shape) == (lat, lat, 1, 1) and ci == 2 * lat and (kh, kw) == (3, 3) and co % 16 == 0 and lat % 16 == 0
                    and m4.stride == (1, 1) and m4.padding == (1, 1) and m3.stride == (1, 1))
            n = co * kh * kw * ci
            we_off, be_off = off, off + n
            off += n + (co + 63) // 64 * 64 + (co * 9 + 63) // 64 * 64          # We, be, beta [O][9]
            rec[i] = (we_off, be_off, off, off + n, off + 2 * n, co, 9, ci, 1, blk, nl + nc + k)
            rec[nl + nc + k] = ((m4.weight.data_ptr() - self.base) // 4, (m4.bias.data_ptr() - self.base) // 4, (m3.weight.data_ptr() - self.base) // 4,
                                (m3.bias.data_ptr() - self.base) // 4, 3 * nl + nc + k, co, 9, ci, lat, 2 ** 31 - 1, 1)
            comp.append((i, we_off, be_off, off, n, (co, kh, kw, ci)))
            off += 3 * n
            blk += co + ci
        self.total_blocks, self.nl = blk, nl
        self.table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        self.out = torch.empty(off, dtype=torch.float32, device=dev)
        self._norms = torch.zeros(3 * nl + nc + ns, dtype=torch.float32, device=dev)     # [nl][3], then the composed layers' max |We|
        self.norms = self._norms[:3 * nl].view(nl, 3)
        self.w_amax = w_amax
        self.by_wt = {}                 # data_ptr of a transposed view -> (layer, plane offset) for _split_h2 of the transpose
        self.bias_of = {m.bias.data_ptr(): self.layer[w.data_ptr()][0] for w, m in zip(ws, self.convs) if m.bias is not None}
        self.comp_of, self.comp_amax = {}, {}
        for k, ((ma, mb), (i, we_off, be_off, foff, n, shape)) in enumerate(zip(self.compose + self.compose_skip, comp)):
            we, be = self.out[we_off:we_off + n].view(shape), self.out[be_off:be_off + shape[0]]
            self.layer[we.data_ptr()] = (i, foff, n, shape, 1)
            self.bias_of[be.data_ptr()] = i
            if k < nc:
                self.comp_of[(id(ma), id(mb))] = (we, be)
            else:
                b0 = be_off + (shape[0] + 63) // 64 * 64
                self.comp_of[(id(ma), id(mb))] = (we, be, self.out[b0:b0 + shape[0] * 9].view(shape[0], 9))
            self.comp_amax[i] = self._norms[3 * nl + k:3 * nl + k + 1]
        self._src_ptrs = [(m, m.weight.data_ptr(), m.bias.data_ptr(), tuple(m.weight.shape)) for m in srcs]
        self._anchor = torch.empty(0, dtype=torch.float32, device=dev)

    def composed(self, m5, m1):
        """(We [O,kh,kw,I], be [O]) of the layer composed of conv5 and conv1 (views of this prep's storage, valid after run()), or None"""
        return self.comp_of.get((id(m5), id(m1)))

    def composed_skip(self, m3, m4):
        """(We [O,3,3,2 lat], be [O], beta [O,9]) of the layer composed of the skip convolution conv3 and conv4 (views, valid after run()), or None"""
        return self.comp_of.get((id(m3), id(m4)))

    def stale(self) -> bool:
        """True when a conv parameter no longer lives where the table says (model.to(), load_state_dict(assign=True), p.data = ...):
        the table holds raw addresses, so the caller must rebuild the WeightPrep before running it"""
        for m in self.convs:
            e = self.layer.get(m.weight.data_ptr())          # (the OHWI view of a channels_last weight starts at the same address)
            co, ci, kh, kw = m.weight.shape
            if e is None or e[3] != (co, kh, kw, ci):
                return True
            if m.bias is not None and m.bias.data_ptr() not in self.bias_of:
                return True
        for m, wp, bp, shape in self._src_ptrs:
            if m.weight.data_ptr() != wp or m.bias is None or m.bias.data_ptr() != bp or tuple(m.weight.shape) != shape:
                return True
        return False

    def run(self, w_amax: torch.Tensor):
        """(re)compute every form for the current parameter values"""
        import ctypes
        assert not self.stale(), "WeightPrep: a conv parameter moved since the table was built -- rebuild it (Trainer does: _wprep)"
        self.w_amax = w_amax
        self._norms.zero_()
        call("df_weight_prep", ctypes.c_void_p(self.base), ptr(self.table), self.nl, self.total_blocks, ptr(w_amax), ptr(self.out), ptr(self.norms),
             stream())

    def wt(self, w_ohwi: torch.Tensor) -> Optional[torch.Tensor]:
        e = self.layer.get(w_ohwi.data_ptr())
        if e is None:
            return None
        i, off, n, (co, kh, kw, ci), split = e
        t = self.out[off:off + n].view(ci, kh, kw, co)
        self.by_wt[t.data_ptr()] = (i, off + 2 * n, n, split)
        return t

    def h2(self, w: torch.Tensor):
        """[hi | lo] planes (a float16 view of 2 x numel) of a layer's weights, or of its transpose as self.wt() returned it"""
        e = self.layer.get(w.data_ptr())
        if e is not None and e[4]:
            i, off, n, _, _ = e
            return self.out[off + n:off + 2 * n].view(torch.float16), self.comp_amax.get(i, self.w_amax)    # (a composed layer: its own scale)
        e = self.by_wt.get(w.data_ptr())
        if e is not None and e[3]:
            i, o2, n, _ = e
            return self.out[o2:o2 + n].view(torch.float16), self.comp_amax.get(i, self.w_amax)
        return None

    def l1(self, w: torch.Tensor, bias: Optional[torch.Tensor]):
        """(max row L1 norm, max |bias| or None) device scalars for a layer's weights or their transpose; None if not one of ours"""
        e = self.layer.get(w.data_ptr())
        col = 0
        if e is None:
            e2 = self.by_wt.get(w.data_ptr())
            if e2 is None:
                return None
            i, col = e2[0], 1
        else:
            i = e[0]
        bm = None
        if bias is not None:
            j = self.bias_of.get(bias.data_ptr())
            if j is None:
                return None
            bm = self.norms[j, 2:3]
        return self.norms[i, col:col + 1], bm


WPREP: Optional[WeightPrep] = None


def rows_l1max(w2d_rows: int, row_len: int, w: torch.Tensor, bias: Optional[torch.Tensor] = None):
    """-> (max_row sum |w[row, :]|, max |bias| or None) as device scalars: the weight side of a conv output's a-priori bound"""
    if WPREP is not None:
        hit = WPREP.l1(w, bias)
        if hit is not None:
            return hit
    l1 = amax_slot(w.device)
    bm = amax_slot(w.device) if bias is not None else None
    call("df_rows_l1max", ptr(w), w2d_rows, row_len, ptr(bias), 0 if bias is None else bias.numel(), ptr(l1), ptr(bm), stream())
    return l1, bm


def h2_bound(a: torch.Tensor, l1: Optional[torch.Tensor] = None, b: Optional[torch.Tensor] = None,
             other: Optional[torch.Tensor] = None, slack: float = 1.001) -> torch.Tensor:
    """device scalar max(other, a * l1 * slack + b)"""
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    call("df_h2_bound", ptr(out), ptr(a), ptr(l1), ptr(b), ptr(other), float(slack), stream())
    return out


def conv_out_bound(x: DfImg, w_rows: torch.Tensor, bias: Optional[torch.Tensor], device, other: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bound of max |conv(x; w) + bias| for the kernel operand `w_rows` ([rows = output channels][taps x input channels] memory:
    the OHWI weights of a forward conv, the transposed ones of a data gradient):  max|x| x max_row ||w_row||_1 + max |bias|"""
    rows = w_rows.shape[0]
    l1, bm = rows_l1max(rows, w_rows.numel() // rows, w_rows, bias)
    return h2_bound(amax_of(x, device), l1, bm, other)


def h2_active() -> bool:
    """are the fp32-mode 3x3 stride-1 convolutions on the fp16x2 kernels (so that producers should measure max |x|)?"""
    return (not MFMA_BF16) and _h2_on() and os.environ.get("DF_CONV_X3", "1") != "0"


_UP_FUSED_NO: set = set()     # (shape keys for which df_conv2d_h2f_wp_up answered DF_E_SHAPE: the two launches are used)


def conv1x1_up_fused(x: DfImg, w_ohwi: torch.Tensor, bias: torch.Tensor, y: DfImg, t: DfImg, align_corners: bool) -> bool:
    """The 1x1 skip convolution of an UpsampleSkip block into the SECOND half `y` of a pre-split concatenation, its workgroups also
    writing the first half = bilinear x2 of `t` (df_conv2d_h2f_wp_up, round 6): -> True if that one launch was issued, False if the
    call is not covered (no WeightPrep planes / no bound on x / shape outside the 8-wave DMA kernels) -- the caller then issues
    ops.upsample2x + ops.conv2d.  DF_UP_FUSED=0: never."""
    if (os.environ.get("DF_UP_FUSED", "1") == "0" or not h2_active() or MFMA_BF16 or y.elt != 2 or x.elt != 0 or t.elt != 0
            or getattr(x, "_amax", None) is None or getattr(y, "_amax", None) is None):
        return False
    wp = _wprep_planes(w_ohwi)
    if wp is None:
        return False
    key = (x.n, x.h, x.w, x.c, y.c, y.ld)
    if key in _UP_FUSED_NO:
        return False
    prof = PROFILER
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    try:
        call("df_conv2d_h2f_wp_up", x, ptr(w_ohwi), ptr(wp[0]), ptr(x._amax), ptr(wp[1]), ptr(bias), y, ptr(y._amax), t, int(align_corners), stream())
    except RuntimeError as e:
        if "DF_E_SHAPE" not in str(e):
            raise
        _UP_FUSED_NO.add(key)
        return False
    if prof is not None:
        e1.record()
        prof.records.append(("conv_dma_kernel<up>/h2", 2.0 * y.n * y.h * y.w * x.c * y.c, e0, e1,
                             f"fwd 1x1 s1 {x.c}->{y.c} @{y.h}x{y.w} x{y.n} fh + bilinear x2", float(x.n * x.h * x.w * x.c * 4 + 2 * y.n * y.h * y.w * y.c * 4)))
    return True


def _split_h2(w_ohwi: torch.Tensor):
    """weights -> (two fp16 planes, their amax): per call (they change every optimizer step; each conv uses them once per direction)
    -- or from the step's WeightPrep when the tensor is one of its layers (or a transpose it handed out)"""
    if WPREP is not None:
        hit = WPREP.h2(w_ohwi)
        if hit is not None:
            return hit
    wa = W_AMAX
    if wa is None:
        # outside a trainer step (inference, plain autograd): planes are kept per weight tensor until it changes -- an eval-mode forward
        # split every 3x3 layer's weights on every call (round 5: 14 df_split_h2 + 21 df_absmax launches of the 95 of a B = 1 forward)
        # ONE entry per weight tensor (keyed by address and shape, validated by its write epoch): a changed tensor replaces its entry,
        # so plain-autograd training does not pile up a triple per layer and step until a clear
        key, epoch = _cache_key(w_ohwi)
        hit = _PLANE_CACHE.get(key) if key is not None else None
        if hit is not None and hit[3] == epoch:
            return hit[0], hit[1]
        # (a bound of its own tensor, NOT a pooled slot: amax_pool_reset() recycles those between steps)
        wa = torch.zeros(1, dtype=torch.float32, device=w_ohwi.device)
        call("df_absmax", img(w_ohwi.reshape(1, 1, -1, w_ohwi.shape[-1])), ptr(wa), stream())
        w2 = torch.empty(2 * w_ohwi.numel(), dtype=torch.float16, device=w_ohwi.device)
        call("df_split_h2", ptr(w_ohwi), ptr(wa), ptr(w2), w_ohwi.numel(), stream())
        if key is not None:
            if len(_PLANE_CACHE) > 256:
                _PLANE_CACHE.clear()
            _PLANE_CACHE[key] = (w2, wa, w_ohwi, epoch)     # (the tensor is kept: its address cannot be reused while cached)
        return w2, wa
    w2 = torch.empty(2 * w_ohwi.numel(), dtype=torch.float16, device=w_ohwi.device)
    call("df_split_h2", ptr(w_ohwi), ptr(wa), ptr(w2), w_ohwi.numel(), stream())
    return w2, wa


_PLANE_CACHE: dict = {}
_WT_CACHE: dict = {}


def _cache_key(t: torch.Tensor):
    """-> ((address, shape), write epoch) of a weight tensor for the per-tensor caches of non-trainer callers; (None, None) for
    tensors that do not track versions (inference mode)"""
    # only tensors MARKED as having a stable identity (`_df_keep`): ops.ohwi's view of a channels_last parameter and the transposes
    # weight_transpose keeps for those.  Anything else -- a per-call contiguous copy, the decoder's packed gate matrices, a gradient
    # passed through weight_transpose -- is a fresh tensor whose address may repeat with version 0: never cached
    if not getattr(t, "_df_keep", False):
        return None, None
    try:
        return (t.data_ptr(), tuple(t.shape)), (t._version, WEIGHT_GEN[0])
    except RuntimeError:
        return None, None


def _wprep_planes(w_ohwi: torch.Tensor):
    """(planes, their amax) of a 1x1 / stride-2 layer's weights (or of the transpose ops.weight_transpose handed out) if the step's
    WeightPrep made them, else from a split of its own (kept while the tensor is unchanged) -- conv_dma_kernel<.., H2, BP> fetches the
    weights pre-split.  DF_CONV_H2F_WP=0: None (the kernel splits its weight fragments itself)."""
    if os.environ.get("DF_CONV_H2F_WP", "1") == "0":
        return None
    if WPREP is not None:
        hit = WPREP.h2(w_ohwi)
        if hit is not None:
            return hit
    if W_AMAX is not None:      # inside a trainer step without the weight prep (DF_WPREP=0): the same kernel, planes from a per-call split
        return _split_h2(w_ohwi)
    # plain autograd / inference callers: the same kernel again (one form of the convolution whoever calls it: the captured trainer
    # program and a hand-driven eager step agree bit for bit, tests/helpers/rccl_world1.py); planes are kept per weight tensor until it
    # changes (inference: split once; a transposed copy made per call misses and is split per call)
    return _split_h2(w_ohwi)     # (W_AMAX is None here: _split_h2 keeps the planes in _PLANE_CACHE)


def _w_amax(w_ohwi: torch.Tensor) -> torch.Tensor:
    """bound of the weights for the in-kernel split (DF_CONV_H2F_WP=0: no prepared planes): the trainer's, else one df_absmax pass"""
    if W_AMAX is not None:
        return W_AMAX
    wa = amax_slot(w_ohwi.device)
    call("df_absmax", img(w_ohwi.reshape(1, 1, -1, w_ohwi.shape[-1])), ptr(wa), stream())
    return wa


def _conv_form(x: DfImg, y: DfImg, ks: int, stride: int, mode: int, epi: int, bias, accumulate: bool, bwd_bn) -> Tuple[str, bool]:
    """The form that takes the call, decided in ONE place (queries only: nothing is allocated or launched) -> (form, h2f):
      dgrad_bn  the fp16x2 3x3 data gradient whose epilogue leaves the BatchNorm-backward partials (df_conv2d_h2p_dgrad_bn)
      h2p / h2  fp32-accurate 3x3 stride-1 products from TWO fp16 planes per operand with per-tensor power-of-two scales (conv_halo_x3_kernel
                <NP = 2>: three MFMAs per operand pair instead of six), with / without a pre-split input or output
      x3        ... from three bf16 planes (DF_CONV_H2=0)
      yh2       a 1x1 / stride-2 convolution with a pre-split OUTPUT: the fp32-input kernels
      h2f       a convolution without a haloed fp16x2 form whose input carries a bound: fp16x2 on the fragments of the DMA-tile kernel
      w16       bf16 mode: bf16 tiles in LDS (conv_halo_w16_kernel)
      mp        the fp32 / bf16-operand MFMA kernels (conv2d makes it `amax` where the output's max |y| is wanted)
    h2f: the fragments of a `yh2` / `h2f` call are split (x has a bound); conv2d then looks for the layer's prepared weight planes."""
    s1 = ks == 3 and stride == 1
    geom = (x, y, ks, stride, mode)
    if MFMA_BF16:
        assert x.elt != 2 and y.elt != 2
        w16 = s1 and os.environ.get("DF_CONV_W16", "1") != "0" and call("df_conv2d_w16_ok", *geom, epi) == 1
        return ("w16" if w16 else "mp"), False
    pre = x.elt == 2 or y.elt == 2     # pre-split input and / or output (h2 images; their bounds ride on the descriptors)
    if pre:
        assert _h2_on() and not accumulate
        assert s1 or x.elt == 0, "1x1 / stride-2 convolutions read fp32"
    if s1 and (pre or (x.elt == 0 and y.elt == 0 and call("df_conv2d_x3_ok", *geom, epi) == 1)):
        if not _h2_on():
            return "x3", False
        if (bwd_bn is not None and mode == CONV_DGRAD and y.elt == 0 and not accumulate and bias is None and y.ld == y.c
                and os.environ.get("DF_FUSE_BN_BWD", "1") != "0" and call("df_conv2d_h2p_ok", *geom, 3) == 1):
            return "dgrad_bn", False
        if pre:
            assert call("df_conv2d_h2p_ok", *geom, epi) == 1, "no pre-split tile form for this shape (ask df_conv2d_h2p_ok first)"
        return ("h2p" if pre else "h2"), False
    # (round 5: also the 3x3 stride-1 layers that have NO haloed fp16x2 tile form -- too few pixels: the 64 x 64 layers of a B = 1
    # forward ran on the fp32 MFMA, 5 x 94 us of a 2.2 ms forward)
    h2f = (h2_active() and x.elt == 0 and y.elt in (0, 2)
           and x.c % (64 if os.environ.get("DF_CONV_H2F_C32", "1") == "0" else 32) == 0     # (32: the first encoder conv on the canvas: its bound comes from the pillar feature net's statistics)
           and getattr(x, "_amax", None) is not None and os.environ.get("DF_CONV_H2F", "1") != "0")
    return ("yh2" if pre else "h2f" if h2f else "mp"), h2f


def conv2d(x: DfImg, w_ohwi: torch.Tensor, bias: Optional[torch.Tensor], y: DfImg, ks: int, stride: int = 1,
           mode: int = CONV_FWD, epi: int = EPI_BIAS, scale=None, shift=None, stats=None, accumulate: bool = False,
           amax_out: Optional[torch.Tensor] = None, bwd_bn=None, x_border: Optional[torch.Tensor] = None):
    """amax_out: the slot the output's max |y| is accumulated into (fp16x2 mode; default: a fresh one) -- several producers of one
    buffer (the two halves of a concatenation) share a slot.
    x_border = beta [C][9]: x (pre-split) is the raw output of a layer composed of a skip convolution and a zero-padded 3x3
    (WeightPrep.composed_skip), whose single bias over-counts the folded bias at the border pixels: this call, x's first reader, takes
    the excess off in place before it reads (df_u3u4_border_fix) -- the composed layer's own launch stays a plain convolution.
    bwd_bn = (y_prev, bn_ss_prev, partial): a 3x3 stride-1 DATA gradient whose output is the gradient of a BatchNorm + GELU layer's
    output -- the fp16x2 kernel's epilogue then also leaves that layer's backward partial sums in `partial` (df_conv2d_h2p_dgrad_bn).
    -> True if it did (the caller then skips ops.bn_gelu_bwd's reduce pass); ignored (False) on any other kernel."""
    if x_border is not None:
        assert x.elt == 2
        with timed("u3u4_border_fix", bytes=16.0 * x.n * (x.h + x.w - 2) * x.c, tag=f"border fix {x.c} ch @{x.h}x{x.w} x{x.n}"):
            call("df_u3u4_border_fix", x, ptr(x._amax), ptr(x_border), stream())
    prof = PROFILER
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    form, h2f = _conv_form(x, y, ks, stride, mode, epi, bias, accumulate, bwd_bn)
    # fp32 mode with the fp16x2 kernels on: every fp32 conv output carries its max |y| for a possible fp16x2 consumer (measured by
    # the epilogue; outputs that go through BatchNorm + GELU first get theirs from that pass instead)
    ya = None
    if h2_active() and y.elt == 0 and epi == EPI_STATS and amax_out is not None:
        ya = amax_out          # max |y| of a conv output that BatchNorm + GELU follow: the bounds of the pre-split z / dy come from it
    elif h2_active() and y.elt == 0 and epi != EPI_STATS:
        ya = amax_out if amax_out is not None else amax_slot(w_ohwi.device)
        y._amax = ya
        src = getattr(y, "_src", None)      # the descriptor covers a whole tensor: descriptors made of it later inherit the bound
        if src is not None:
            src._df_amax = (ya, ver(src))
    if ya is None and getattr(y, "_src", None) is not None:
        wrote(y._src)          # (an unmeasured write into a tensor that carried a bound)
    if form == "mp" and ya is not None:
        form = "amax"          # the same kernels, measuring
    # what the form reads besides x and y: the weights in its layout (they change every optimizer step: split / cast once per call unless
    # the step's WeightPrep holds them), bounds
    dev, acc = w_ohwi.device, int(accumulate)
    tail = (ks, stride, ks // 2, mode, epi, ptr(scale), ptr(shift), ptr(stats))
    if form in ("dgrad_bn", "h2p", "h2"):
        w2, wa = _split_h2(w_ohwi)
    elif form in ("yh2", "h2f"):
        wp = _wprep_planes(w_ohwi) if h2f else None
        if wp is not None:      # this layer's planes: no weight split in the kernel (conv_dma_kernel<.., H2, BP>)
            form = "h2f_wp"
        wa = _w_amax(w_ohwi) if (h2f and wp is None) else None
    elif form == "x3":
        wx = torch.empty(3 * w_ohwi.numel(), dtype=torch.bfloat16, device=dev)
        call("df_split_bf16x3", ptr(w_ohwi), ptr(wx), w_ohwi.numel(), stream())
    elif form == "w16":         # (the activations stay fp32 in memory unless the descriptors say bf16)
        wx = torch.empty(w_ohwi.numel(), dtype=torch.bfloat16, device=dev)
        call("df_cast_bf16", ptr(w_ohwi), ptr(wx), w_ohwi.numel() // x.c, x.c, x.c, x.c, stream())
    if form == "dgrad_bn":
        call("df_conv2d_h2p_dgrad_bn", x, ptr(w2), ptr(amax_of(x, dev)), ptr(wa), y, *map(ptr, bwd_bn), ptr(ya), stream())
    elif form == "h2p":
        call("df_conv2d_h2p", x, ptr(w2), ptr(amax_of(x, dev)), ptr(wa), ptr(bias), y, ptr(y._amax) if y.elt == 2 else None, *tail, 0, ptr(ya), stream())
    elif form == "h2":
        call("df_conv2d_h2", x, ptr(w2), ptr(amax_of(x, dev)), ptr(wa), ptr(bias), y, *tail, acc, ptr(ya), stream())
    elif form == "h2f_wp":      # (y pre-split: its bound, no measurement -- ya is None then)
        call("df_conv2d_h2f_wp", x, ptr(w_ohwi), ptr(wp[0]), ptr(x._amax), ptr(wp[1]), ptr(bias), y, ptr(y._amax) if y.elt == 2 else None, *tail, acc, ptr(ya), stream())
    elif form == "yh2":
        call("df_conv2d_yh2", x, ptr(w_ohwi), ptr(x._amax) if h2f else None, ptr(wa), ptr(bias), y, ptr(y._amax), *tail, 0, stream())
    elif form == "h2f":
        call("df_conv2d_h2f", x, ptr(w_ohwi), ptr(x._amax), ptr(wa), ptr(bias), y, *tail, acc, ptr(ya), stream())
    elif form == "amax":
        call("df_conv2d_amax", x, ptr(w_ohwi), ptr(bias), y, *tail, acc, ptr(ya), stream())
    elif form == "x3":
        call("df_conv2d_x3", x, ptr(wx), ptr(bias), y, *tail, acc, stream())
    elif form == "w16":
        call("df_conv2d_w16", x, ptr(wx), ptr(bias), y, *tail, acc, stream())
    else:
        call("df_conv2d_mp", x, ptr(w_ohwi), ptr(bias), y, *tail, acc, int(MFMA_BF16), stream())
    if prof is not None:
        e1.record()
        small = y if mode == CONV_FWD else x  # the conv-output-sized grid
        flops = 2.0 * small.n * small.h * small.w * ks * ks * x.c * y.c
        tag = f"{'fwd' if mode == CONV_FWD else 'dgrad'} {ks}x{ks} s{stride} {x.c}->{y.c} @{small.h}x{small.w} x{small.n} {'fbh'[x.elt]}{'fbh'[y.elt]}"
        # operand bytes of the call (input + output images once, the weights once): what an HBM-bound small-K layer is priced against
        esz = lambda d: (4, 2, 4)[d.elt]
        obytes = float(x.n * x.h * x.w * x.c * esz(x) + y.n * y.h * y.w * y.c * esz(y) * (2 if accumulate else 1) + w_ohwi.numel() * 4)
        prof.records.append((_conv_label(x, y, ks, stride, mode, epi, form, h2f) + ("/bf16" if MFMA_BF16 else ""), flops, e0, e1, tag, obytes))
    return form == "dgrad_bn"


def conv_tile_m(rows_per_group: int, cout: int) -> int:
    return call("df_conv2d_tile_m", rows_per_group, cout)


# Folded eval-mode BatchNorm (scale, shift, mean, invstd) is cached per module: five tiny torch launches per layer and
# forward otherwise -- 90 of the 175 launches of a B=1 inference.  The cache key carries the tensors' version counters
# plus PARAM_GEN, which every HIP-side writer that bypasses autograd's counters bumps (Adam on the flat arena, the
# running-statistics update of a training forward).
PARAM_GEN = [0]
# ... and WEIGHT_GEN, bumped only where WEIGHTS are written that way (the arena's Adam kernel, a captured step's replay): the epoch of the
# per-tensor weight caches (ohwi copies, transposes, fp16 planes) -- the running-statistics updates of a training forward bump
# PARAM_GEN eighteen times per step and would void them for nothing
WEIGHT_GEN = [0]


def invalidate_weight_caches() -> None:
    """Void every per-tensor weight cache (fp16 planes, transposes, OHWI copies) and every folded BatchNorm.  The caches are validated by
    (tensor._version, WEIGHT_GEN): writers that go through autograd's version counters -- optimizer.step() in eager PyTorch,
    load_state_dict, parameter.copy_() -- need nothing.  Writers that BYPASS the counters must call this (or bump the generations) after
    they write: a user-captured CUDA-graph replay of a torch optimizer step, raw-pointer writes into the parameter arena, another
    library updating the weights in place.  FlatAdam.step / step_captured and the trainer's graph replay do it themselves;
    load_from_checkpoint calls it for good measure."""
    WEIGHT_GEN[0] += 1
    PARAM_GEN[0] += 1


def folded_bn(bn) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    key = (PARAM_GEN[0], bn.weight._version, bn.bias._version, bn.running_mean._version, bn.running_var._version,
           bn.weight.data_ptr(), bn.running_var.data_ptr(), bn.eps)
    c = getattr(bn, "_df_fold", None)
    if c is None or c[0] != key:
        invstd = torch.rsqrt(bn.running_var + bn.eps)
        scale = (bn.weight.detach() * invstd).contiguous()
        shift = (bn.bias.detach() - bn.running_mean * scale).contiguous()
        c = (key, scale, shift, bn.running_mean, invstd)
        bn._df_fold = c
    return c[1], c[2], c[3], c[4]


class SyncBN:
    """sync_bn (Lightning's sync_batchnorm / torch SyncBatchNorm) for the data-parallel ranks: the per-channel sums behind a
    BatchNorm's batch statistics -- forward (sum, sum of squares, count) and backward (sum of g, sum of g * xhat) -- are
    all-reduced between the partial-sum kernels and the finalisation, which then runs as a few fp64 torch ops on [C]-sized
    tensors instead of the fused finalize kernels.  Parameter gradients (dgamma, dbeta) stay rank-local sums: the
    gradient all-reduce averages them like every other parameter (as torch's SyncBatchNorm + DDP do)."""

    def __init__(self, dist, group, world: int):
        self.dist, self.group, self.world = dist, group, world

    def sum(self, t: torch.Tensor) -> torch.Tensor:
        self.dist.all_reduce(t, group=self.group)
        return t


SYNC: Optional[SyncBN] = None   # set by optim.Trainer(sync_bn=True) on a multi-rank process group


def bn_finalize(partial, tiles_per_group, groups, C, count, gamma, beta, eps, momentum, rmean, rvar, bn_ss, y_amax=None, z_bound=None):
    """y_amax / z_bound (both or neither): max |y| as the conv epilogue measured it, and the zero-initialised slot that receives the
    bound of max |gelu(bn(y))| -- the scale of the pre-split z the apply pass writes next"""
    PARAM_GEN[0] += 1  # running statistics change under any cached eval-mode fold
    if SYNC is not None:
        red = SYNC.sum(partial.view(groups, tiles_per_group, C, 2).to(torch.float64).sum(1))      # [groups, C, 2], all ranks
        cnt = float(count) * SYNC.world
        ga = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64, device=partial.device)
        be = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64, device=partial.device)
        out = bn_ss.view(groups, 4, C)
        for g in range(groups):                    # groups = successive calls of the module: running statistics in call order
            mean = red[g, :, 0] / cnt
            var = (red[g, :, 1] / cnt - mean * mean).clamp_min(0.0)
            invstd = torch.rsqrt(var + eps)
            out[g] = torch.stack([ga * invstd, be - mean * ga * invstd, mean, invstd]).float()
            if rmean is not None:
                unb = var * (cnt / (cnt - 1.0)) if cnt > 1 else var
                rmean.mul_(1.0 - momentum).add_((momentum * mean).float())
                rvar.mul_(1.0 - momentum).add_((momentum * unb).float())
        if z_bound is not None:
            z_bound.copy_((out[:, 0].abs() * y_amax + out[:, 1].abs()).max().reshape(1))
        return
    splits = min(64, tiles_per_group // 64)  # two-stage reduction once a group has thousands of tile partials
    scratch = torch.empty(groups * splits * 2 * C, dtype=torch.float64, device=partial.device) if splits > 1 else None
    call("df_bn_finalize2", ptr(partial), tiles_per_group, groups, C, count, ptr(gamma), ptr(beta), eps, momentum,
         ptr(rmean), ptr(rvar), ptr(bn_ss), ptr(scratch), splits, ptr(y_amax), ptr(z_bound), stream())


def _elt(t: torch.Tensor) -> int:
    return 1 if t.dtype == torch.bfloat16 else 0


def bn_gelu_apply(y: torch.Tensor, bn_ss: torch.Tensor, imgs_per_group: int, z: DfImg):
    with timed("bn_gelu_apply", bytes=(y.element_size() + (2.0 if z.elt == 1 else 4.0)) * y.numel()):          # read y, write z
        if z.elt == 2:      # pre-split z: its bound (df_bn_finalize2) is an INPUT here
            call("df_bn_gelu_apply_t", ptr(y), _elt(y), ptr(bn_ss), imgs_per_group, z, ptr(z._amax), stream())
            return
        a = amax_slot(y.device) if (h2_active() and z.elt == 0) else None     # max |z| for the fp16x2 convolution that reads z
        call("df_bn_gelu_apply_t", ptr(y), _elt(y), ptr(bn_ss), imgs_per_group, z, ptr(a), stream())
        if a is not None:
            z._amax = a


def _pow2_blocks(rows_per_group: int, cap: int = 512) -> int:
    """largest power of two <= cap dividing rows_per_group with >= 16 rows per block"""
    n = 1
    while n * 2 <= cap and rows_per_group % (n * 2) == 0 and rows_per_group // (n * 2) >= 16:
        n *= 2
    return n


def bn_gelu_bwd(dz: DfImg, y: torch.Tensor, bn_ss: torch.Tensor, imgs_per_group: int, groups: int, gamma_grad: bool = True,
                frozen: bool = False, dy_dtype: torch.dtype = torch.float32, dy_h2: bool = False,
                y_amax: Optional[torch.Tensor] = None, partial_pre=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> dy [n,h,w,C] (dy_dtype: float32, or bfloat16 in the bf16-storage mode), dgamma [C], dbeta [C], dbias [C].
    dy_h2 (with y_amax = max |y| from the forward's conv epilogue): dy is written pre-split (ops.h2_empty) with the scale of the
    bound the finalisation derives from max |dz|, max |y| and the statistics.
    frozen: eval-mode BatchNorm (running statistics are constants): the batch-statistic terms of the data gradient
    vanish (coef = 0), dgamma / dbeta keep their form, and the conv bias gradient is no longer cancelled."""
    dev = y.device
    C = dz.c
    rows_per_group = imgs_per_group * dz.h * dz.w
    nbg = _pow2_blocks(rows_per_group)
    nblk = nbg * groups
    gb = 2.0 if dz.elt else 4.0
    if partial_pre is not None:
        # the partial sums came out of the epilogue of the data gradient that produced dz (ops.conv2d bwd_bn): [groups * nbp][C][2]
        partial, nbp = partial_pre
        nbg_fin = nbp
    else:
        partial = _f32(nblk, C, 2, device=dev)
        nbg_fin = nbg
        with timed("bn_gelu_bwd_reduce", bytes=(gb + y.element_size()) * y.numel()):     # read dz, y
            call("df_bn_gelu_bwd_reduce_t", dz, ptr(y), _elt(y), ptr(bn_ss), imgs_per_group, ptr(partial), nblk, stream())
    dy_bound = None
    if dy_h2:
        assert y_amax is not None and dy_dtype == torch.float32 and dz.elt == 0 and y.dtype == torch.float32
        dy_bound = amax_slot(dev)
        dz_amax = amax_of(dz, dev)
    if SYNC is not None and not frozen:
        red = partial.view(groups, nbg_fin, C, 2).to(torch.float64).sum(1)          # [groups, C, (sum g, sum g * xhat)], this rank
        dbeta, dgamma = red[:, :, 0].sum(0).float(), red[:, :, 1].sum(0).float()
        glob = SYNC.sum(red.clone()) / (float(rows_per_group) * SYNC.world)
        coef = glob.permute(0, 2, 1).contiguous().float()                        # [groups, 2, C]
        if dy_h2:
            ss = bn_ss.view(groups, 4, C)
            xh = (y_amax + ss[:, 2].abs()) * ss[:, 3]
            dy_bound.copy_((ss[:, 0].abs() * (1.13 * dz_amax + coef[:, 0].abs() + xh * coef[:, 1].abs())).max().reshape(1))
    else:
        dgamma, dbeta = _f32(C, device=dev), _f32(C, device=dev)
        coef = _f32(groups, 2, C, device=dev)
        if dy_h2:
            call("df_bn_bwd_finalize2", ptr(partial), nbg_fin, groups, C, rows_per_group, ptr(dgamma), ptr(dbeta), ptr(coef), ptr(bn_ss),
                 ptr(dz_amax), ptr(y_amax), ptr(dy_bound), stream())
        else:
            call("df_bn_bwd_finalize", ptr(partial), nbg_fin, groups, C, rows_per_group, ptr(dgamma), ptr(dbeta), ptr(coef), stream())
        if frozen:
            coef.zero_()
    dy = h2_empty(y.shape, dev, dy_bound) if dy_h2 else torch.empty(y.shape, dtype=dy_dtype, device=dev)
    dbp = _f32(nblk, C, device=dev)
    with timed("bn_gelu_bwd_apply", bytes=(gb + y.element_size() + dy.element_size()) * y.numel()):     # read dz, y; write dy
        a = dy_bound if dy_h2 else amax_slot(dev) if (h2_active() and dy_dtype == torch.float32) else None     # max |dy| for the fp16x2 dgrad / wgrad
        call("df_bn_gelu_bwd_apply_t", dz, ptr(y), _elt(y), ptr(bn_ss), ptr(coef), imgs_per_group, ptr(dy), 2 if dy_h2 else _elt(dy), ptr(dbp), nblk,
             ptr(a), stream())
        if a is not None and not dy_h2:
            dy._df_amax = (a, ver(dy))          # _lib.img() hands it on to the descriptors made of this tensor
    dbias = _f32(C, device=dev)
    call("df_colsum_finalize", ptr(dbp), nblk, C, 1, ptr(dbias), 0, stream())
    return dy, dgamma, dbeta, dbias


def colsum(x: DfImg, device) -> torch.Tensor:
    rows = x.n * x.h * x.w
    nblk = max(1, min(1024, rows // 64))
    partial = _f32(nblk, x.c, device=device)
    call("df_colsum_partial", x, ptr(partial), nblk, stream())
    out = _f32(x.c, device=device)
    call("df_colsum_finalize", ptr(partial), nblk, x.c, 1, ptr(out), 0, stream())
    return out


def weight_transpose(w_ohwi: torch.Tensor) -> torch.Tensor:
    """[Cout,kh,kw,Cin] -> [Cin,kh,kw,Cout]"""
    if WPREP is not None:
        hit = WPREP.wt(w_ohwi)
        if hit is not None:
            return hit
    key = epoch = None
    if W_AMAX is None:      # outside a trainer step: the transpose of an unchanged weight tensor is kept (and with it the fp16 planes
        key, epoch = _cache_key(w_ohwi)      # _split_h2 keeps for THAT tensor) -- a backward made ~30 fresh copies that never hit
        hit = _WT_CACHE.get(key) if key is not None else None
        if hit is not None and hit[2] == epoch:
            return hit[0]
    co, kh, kw, ci = w_ohwi.shape
    wt = torch.empty((ci, kh, kw, co), dtype=torch.float32, device=w_ohwi.device)
    call("df_weight_transpose", ptr(w_ohwi), ptr(wt), co, kh * kw, ci, stream())
    if key is not None:
        old = _WT_CACHE.get(key)
        if old is not None:      # the superseded transpose's planes go with it
            _PLANE_CACHE.pop(_cache_key(old[0])[0], None)
        if len(_WT_CACHE) > 256:
            _WT_CACHE.clear()
        wt._df_keep = True
        _WT_CACHE[key] = (wt, w_ohwi, epoch)
    return wt


def _wgrad_mp_label(x: DfImg, dy: DfImg, ks: int, stride: int) -> str:      # mirrors df_conv2d_wgrad_mp's dispatch (DF_WGRAD_RING / _RING_S2)
    if ks == 1:
        return f"wgrad1x1_kernel<{128 if x.c >= 128 else 64}>" if dy.c % 128 == 0 else "wgrad_kernel<1,1,32>"
    if stride == 2:
        return "wgrad3_ring_kernel<16,2,2>" if os.environ.get("DF_WGRAD_RING_S2", "1") != "0" else "wgrad_kernel<3,2,32>"
    ring = int(os.environ.get("DF_WGRAD_RING", "2"))
    return f"wgrad3_ring_kernel<32,{ring},1>" if ring in (2, 3) else "wgrad_dma_kernel<3,1,32>"


def _wgrad_form(x: DfImg, dy: DfImg, ks: int, stride: int, row_counts: Optional[torch.Tensor]) -> tuple:
    """The weight-gradient form that takes the layer and, in ONE place per form, what goes with it: -> (form, its _splits query (None:
    df_conv2d_wgrad_splits), its entry point, dev -> that call's arguments between (x, dy) and (ws, splits, ..), its profiler label --
    bench.py's roofline and the layer census match on these strings)"""
    geom = (ks, stride, ks // 2)
    amax = lambda dev: (None, None) if MFMA_BF16 else (ptr(amax_of(x, dev)), ptr(amax_of(dy, dev)))     # (bf16 mode: the one-plane forms)
    if x.elt == 2 and dy.elt == 2:       # both operands pre-split (h2 images); their bounds are the ones that defined the planes' scales
        assert ks == 3 and stride == 1 and row_counts is None and call("df_conv2d_wgrad_h2p_ok", x, dy, ks, stride) == 1
        return "h2p", "df_conv2d_wgrad_h2p_splits", "df_conv2d_wgrad_h2p", lambda dev: (ptr(x._amax), ptr(dy._amax), *geom), "wgrad3_h2p_kernel<4>"
    assert x.elt != 2 and dy.elt != 2, "a pre-split tensor meets an fp32 one in a weight gradient: unpack it (ops.h2_unpack) or keep both split"
    if x.elt == 1 and dy.elt == 1:       # bf16-storage mode: both tensors bfloat16 in memory (transposing-read kernel, 3x3 stride 1 only)
        return "bf16", None, "df_conv2d_wgrad_bf16", lambda dev: geom, "wgrad3_tr_kernel<4>"
    # round 5: the 1x1 and stride-2 layers' fp32 tensors split in flight -- fp16x2 products instead of the fp32 MFMA (row lists: _mp only)
    fly = row_counts is None and ((h2_active() and _h2_on()) or (MFMA_BF16 and os.environ.get("DF_WGRAD_BF_FLY", "1") != "0"))
    if fly and ks == 1 and stride == 1 and call("df_conv2d_wgrad1_h2_ok", x, dy) == 1:
        return ("w1h2", "df_conv2d_wgrad1_h2_splits", "df_conv2d_wgrad1_h2", amax,
                f"wgrad1_h2_kernel<{128 if dy.c % 128 == 0 else 64},{128 if x.c >= 128 else 64}>")
    if fly and ks == 3 and stride == 2 and call("df_conv2d_wgrad_s2_h2_ok", x, dy) == 1:
        return "s2h2", "df_conv2d_wgrad_s2_h2_splits", "df_conv2d_wgrad_s2_h2", amax, "wgrad3s2_h2_kernel"
    if row_counts is None and not MFMA_BF16 and ks == 3 and stride == 1 and call("df_conv2d_wgrad_x3_ok", x, dy, ks, stride) == 1:
        if _h2_on():     # fp32 mode, fp32-accurate products: two scaled fp16 planes per operand, else three bf16 planes
            return "h2", None, "df_conv2d_wgrad_h2", lambda dev: (*amax(dev), *geom), "wgrad3_x3_kernel<2>"
        return "x3", None, "df_conv2d_wgrad_x3", lambda dev: geom, "wgrad3_x3_kernel<3>"
    return "mp", None, "df_conv2d_wgrad_mp", lambda dev: geom, _wgrad_mp_label(x, dy, ks, stride)


def conv2d_wgrad(x: DfImg, dy: DfImg, ks: int, stride: int, dw: torch.Tensor, ld_co: Optional[int] = None,
                 accumulate: bool = False, row_counts: Optional[torch.Tensor] = None, rows_per_seg: int = 0, dw_off: int = 0,
                 want_bias: bool = False, decompose: Optional[tuple] = None) -> Optional[torch.Tensor]:
    """dw (float memory [Cout][taps][Cin] with row pitch ld_co, starting dw_off elements in) (+)= dy^T x.
    want_bias: also return the bias gradient sum_p dy[p, :] (fused: the kernel already stages every dy tile).
    decompose = (w1, w5, b5, dw5, db5, dw1, db1): the layer is one composed of w5 [C,kh,kw,I], b5 and the 1x1 layer w1 [O,1,1,C]
    (WeightPrep.composed); dw and the bias sum are then taken apart into the four parameter gradients (df_u5u1_decompose).
    decompose = ("skip", w3t, w4, b3, dw4, db4, dw3, db3): the layer is one composed of the 1x1 skip convolution w3 (w3t = its transpose
    [I,1,1,C]), b3 and the zero-padded 3x3 w4 [O,3,3,2 lat] (WeightPrep.composed_skip); dw, the bias sum and the border sums of dy are
    then taken apart into those parameters' gradients (df_u3u4_border_sums, df_u3u4_decompose)."""
    dev = dw.device
    assert decompose is None or (want_bias and ld_co is None and not accumulate and not dw_off)
    form, query, entry, mid, name = _wgrad_form(x, dy, ks, stride, row_counts)
    splits = call(query, x, dy) if query else call("df_conv2d_wgrad_splits", x, dy, ks, stride)
    taps = ks * ks
    ws = _f32(splits * dy.c * taps * x.c, device=dev)
    prof = PROFILER
    if prof is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    bias_ws = _f32(splits, dy.c, device=dev) if want_bias else None
    tail = (ptr(row_counts), rows_per_seg, ptr(bias_ws), int(MFMA_BF16)) if form == "mp" else (ptr(bias_ws),)
    call(entry, x, dy, *mid(dev), ptr(ws), splits, *tail, stream())
    if prof is not None:
        e1.record()
        tag = f"wgrad {ks}x{ks} s{stride} {x.c}->{dy.c} @{dy.h}x{dy.w} x{dy.n} {'fbh'[x.elt]}{'fbh'[dy.elt]}"
        esz = lambda d: (4, 2, 4)[d.elt]
        prof.records.append((name + ("/bf16" if MFMA_BF16 else ""), 2.0 * dy.n * dy.h * dy.w * taps * x.c * dy.c, e0, e1, tag,
                             float(x.n * x.h * x.w * x.c * esz(x) + dy.n * dy.h * dy.w * dy.c * esz(dy))))
    if want_bias and os.environ.get("DF_FUSE_REDUCE", "1") != "0":   # weight + bias partials in one launch
        db = _f32(dy.c, device=dev)
        call("df_conv2d_wgrad_reduce_bias", ptr(ws), splits, dy.c, taps, x.c, dw.data_ptr() + 4 * dw_off,
             taps * x.c if ld_co is None else ld_co, int(accumulate), ptr(bias_ws), ptr(db), stream())
        _decompose(decompose, dw, db, taps, dy)
        return db
    call("df_conv2d_wgrad_reduce", ptr(ws), splits, dy.c, taps, x.c, dw.data_ptr() + 4 * dw_off,
         taps * x.c if ld_co is None else ld_co, int(accumulate), stream())
    if want_bias:
        db = _f32(dy.c, device=dev)
        call("df_colsum_finalize", ptr(bias_ws), splits, dy.c, 1, ptr(db), 0, stream())
        _decompose(decompose, dw, db, taps, dy)
        return db
    return None


def _decompose(d: Optional[tuple], dwe: torch.Tensor, dbe: torch.Tensor, taps: int, dy: DfImg) -> None:
    if d is None:
        return
    if d[0] == "skip":
        _, w3t, w4, b3, dw4, db4, dw3, db3 = d
        O, lat = w4.shape[0], w3t.shape[0]
        assert taps == 9 and dy.elt == 2 and dy.c == O and w4.shape[-1] == 2 * lat
        part = torch.empty(8 * dy.n * O + 9 * O, dtype=torch.float64, device=dwe.device)       # border sums per image, then T [O][9]
        T = part[8 * dy.n * O:]
        with timed("u3u4_border_sums", bytes=8.0 * dy.n * (dy.h + dy.w) * O, tag=f"border sums {O} ch @{dy.h}x{dy.w} x{dy.n}"):
            call("df_u3u4_border_sums", dy, ptr(dy._amax), ptr(dbe), ptr(part), ptr(T), stream())
        with timed("u3u4_decompose", flops=4.0 * O * taps * lat * lat, tag=f"u3u4 decompose 1x1 {lat}->{lat} of 3x3 {2 * lat}->{O}"):
            call("df_u3u4_decompose", ptr(w3t), ptr(w4), ptr(b3), ptr(dwe), ptr(T), O, lat, ptr(dw4), ptr(db4), ptr(dw3), ptr(db3), stream())
        return
    w1, w5, b5, dw5, db5, dw1, db1 = d
    O, C, I = w1.shape[0], w5.shape[0], w5.shape[-1]
    with timed("u5u1_decompose", flops=4.0 * O * C * taps * I, tag=f"decompose {C}->{O} of 3x3 {I}->{C}"):
        call("df_u5u1_decompose", ptr(w1), ptr(w5), ptr(b5), ptr(dwe), ptr(dbe), O, C, taps, I, ptr(dw5), ptr(db5), ptr(dw1), ptr(db1), stream())


def upsample2x(x: DfImg, y: DfImg, align_corners: bool, pack: Optional[DfImg] = None):
    """pack = b (fp32 [N,2h,2w,C]): y is the FIRST half of a pre-split concatenation of 2 C channels whose second half is b itself (the
    skip convolution runs folded into the 3x3 that reads the concatenation: WeightPrep.composed_skip) -- one kernel writes whole pixels,
    the bilinear half exactly as df_upsample2x_h2 does and b split with the concatenation's scale (df_cat_pack_up)"""
    if pack is not None:
        assert y.elt == 2 and y.ld == 2 * y.c and pack.elt == 0
        cat = DfImg(y.ptr, y.n, y.h, y.w, 2 * y.c, y.ld, y.grp_size, y.img_stride, y.grp_off, 2, 0)
        with timed("cat_pack_up", bytes=4.0 * (x.n * x.h * x.w * x.c + 3 * y.n * y.h * y.w * y.c), tag=f"pack + bilinear x2 {2 * y.c} ch @{y.h}x{y.w} x{y.n}"):
            call("df_cat_pack_up", x, pack, cat, int(align_corners), ptr(y._amax), stream())
        return
    if y.elt == 2:      # the upsampled half of a pre-split concatenation: scale from the concatenation's bound (>= max |x|)
        call("df_upsample2x_h2", x, y, int(align_corners), ptr(y._amax), stream())
        return
    call("df_upsample2x", x, y, int(align_corners), stream())


def upsample2x_bwd(dy: DfImg, dx: DfImg, align_corners: bool):
    if dx.elt == 2:     # dx is the output gradient of a composed 3x3 layer: written pre-split, scaled by its bound (>= 4.5 max |dy|)
        call("df_upsample2x_bwd_h2", dy, dx, int(align_corners), ptr(dx._amax), stream())
        return
    call("df_upsample2x_bwd", dy, dx, int(align_corners), stream())


def small_outer(a: torch.Tensor, lda: int, na: int, b: Optional[torch.Tensor], ldb: int, nb: int, counts: torch.Tensor,
                rows_per_seg: int, nseg: int, rows: int) -> torch.Tensor:
    nblk = max(1, min(1024, rows // 256))
    partial = _f32(nblk, na * nb, device=a.device)
    call("df_small_outer", ptr(a), lda, na, ptr(b), ldb, nb, ptr(counts), rows_per_seg, nseg, rows, ptr(partial), nblk,
         stream())
    out = _f32(na, nb, device=a.device)
    call("df_colsum_finalize", ptr(partial), nblk, na * nb, 1, ptr(out), 0, stream())
    return out
