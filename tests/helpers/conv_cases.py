"""Cases for the dense convolution kernels (csrc/conv.hip, conv_common.h, conv_wgrad.hip: forward, data gradient, weight gradient and the
split-K reductions): shapes built to reach one piece of a kernel's walk each -- a ragged last row tile, the 128 x 32 tile, stride 2 on odd
images, the haloed forms on thin images, a split that starts mid-row or crosses an image -- the tensors the kernels read, the memory
layouts they are addressed through, and a restatement of the walks in plain Python.

Forward / data gradient (Prob; `legs`: fwd_bias, fwd_gelu = DF_EPI_BN_GELU, fwd_stats = DF_EPI_STATS, dgrad, dgrad_acc = accumulate)
  case            layer and image x [n, h, w]                                what it reaches
  tail64          3x3 s1, 64->64 and 64->128, [3, 5, 9]                      M = 135 = 2 * 64 + 7: 64-row tiles straddle the 45-pixel images, the last
                                                                             tile has 7 rows (m < m_end in the loaders, the not-FULL epilogue, ROW_BAD)
  tail128         3x3 s1, 64->64 and 64->128, [1, 65, 65]                    4225 rows > 4096: 128-row tiles without a halo form (conv_dma_kernel
                                                                             <128,64,..>, <128,128,..>); 33 full tiles, then a tile of ONE row
  n32             1x1, 64->96 and 64->32, [2, 7, 11]                         variant 128032 (cout % 64 != 0); M = 154 = 128 + 26
  s2_odd          3x3 s2, 32->64, [2, 9, 13] -> [2, 5, 7]                    forward: the last window starts on the last row and column; data
                                                                             gradient: odd dx, so the generic register path
  s2_even_ragged  3x3 s2, 32->64, [1, 10, 14] -> [1, 5, 7]                   data gradient: dx is even, but the 35 rows of a parity class are no
                                                                             tile multiple: class mode is refused, the generic path runs
  s2_class        3x3 s2, 64->64, [2, 16, 16] and [1, 16, 16]                data gradient in class mode, 2 tiles and 1 tile per parity class
  thin            3x3 s1, 64->64, [1, 1, 1], [2, 1, 40], [2, 40, 1]          every tap but the centre / a whole tap row / a whole tap column is
                                                                             outside the image
  halo_thin       3x3 s1, 64->64 and 128->128, fwd_stats, [2, 1, 128] and    the haloed forms at H = 1 (no row above or below), the W == 64 row-pair
                  [2, 2, 64] (two groups of one image), [1, 3, 256]          form on an image that is one pair, the 256-pixel row tile at 64
                                                                             channels (statistics rows per tile: stats_mul = 2)
  halo_odd        3x3 s1, 64->64 and 128->128, [1, 33, 128]                  4224 rows = 33 full 128-row tiles on the haloed forms, odd H
  views           tail64 (64->64) and s2_odd with n = 4                      both tensors channel slices of wider buffers, two groups of two images,
                                                                             grp_off != 2 img_stride; NaN around the input, sentinel around the output

Forms (test ids): mp, mpbf16 = df_conv2d_mp with mfma_bf16 0 / 1; amax = df_conv2d_amax; h2f = df_conv2d_h2f; h2fwp = df_conv2d_h2f_wp;
x3, h2, w16 = df_conv2d_x3 / _h2 / _w16 (halo_* only: the library's _ok queries say 1 there and 0 for tail*); yh2 = df_conv2d_yh2 with a
pre-split output, ybf16 = df_conv2d_mp with a bf16 output (tail64, tail128 only).  yh2 refuses accumulation (DF_E_ARG).

Weight gradient (WProb; every split count with and without bias_ws, ending in df_conv2d_wgrad_reduce_bias / _reduce)
  case        layer and image                                   what it reaches
  w_ragged    3x3 s1, 64->64, [3, 5, 9]                         one 32-pixel chunk per row, 9 pixels valid; 15 chunks; splits 1, 2 (starts mid-image,
                                                                crosses an image), 15, 9 (two chunks each: the eighth has one, the ninth is EMPTY)
  w_two_seg   3x3 s1, 64->64, [2, 15, 40]                       two chunks per row (32 + 8), 60 chunks; splits 1, 7, 9 (a split begins on the second
                                                                chunk of a row), 60, 16 (the last one empty), and the library's own count
  w_x3        3x3 s1, 64->64 and 32->64, [2, 3, 64]             the x3 / fp16x2 / bf16-storage forms (W % 32 == 0); 12 chunks; splits 1, 5, 12
                                                                (fewer stages than the ring is deep), 8 (two empty)
  w_s2_odd    3x3 s2, 32->64, [2, 9, 67] -> [2, 5, 34]          16-pixel chunks 16 + 16 + 2; the 33-pixel input patch runs over the right border of
                                                                an odd-width image; cin = 32 leaves half a ci tile idle; splits 1, 4, 7 (one empty)
  w_k96       3x3 s1, 96->192, [1, 4, 32]                       one and a half ci tiles, three co tiles; 4 chunks; splits 1, 4, 3 (the third empty)
  w_1x1       1x1, 64->64, 128->128, 96->128, [2, 7, 11]        wgrad_kernel<1,1,32>, wgrad1x1_kernel<64> / <128> (and their DMA forms), wgrad1_h2_kernel
                                                                <64,64> / <128,128> / <128,64> with 11 of 32 pixels valid per chunk
  w_rows      1x1, 64->64, [1, 1, 240], rows_per_seg = 40,      wg_row_ok on both sides of a chunk boundary, an empty segment
              row_counts [0, 1, 31, 32, 33, 40]
  w_views     w_ragged and w_s2_odd with n = 4                  groups and channel slices as `views`; dw written at an offset with ld_co wider than a row,
                                                                accumulate 0 and 1
Forms: mp, mpbf16 = df_conv2d_wgrad_mp; x3, h2 = df_conv2d_wgrad_x3 / _h2; w1h2, w1bf16 = df_conv2d_wgrad1_h2 with bounds / both NULL;
s2h2, s2bf16 = df_conv2d_wgrad_s2_h2 likewise; bf16 = df_conv2d_wgrad_bf16 on df_cast_bf16 copies.

Tensors are seeded fp32, finite, NHWC; weights LOGICAL [O, I, kh, kw].  reference(p) / wreference(p) hold the ref64 result in float64 and the
same function evaluated in float32 on the CPU (and both again on bf16-rounded operands), cached per process and never modified by their
readers.  bounds(floor, r32, r64) is max(floor, 4 x that fp32 error) per norm of ref64.errors; the floors are the layer census' figures.

tiling / restate (rows -> tiles) and wchunks / split_ranges / partials64 (chunks -> splits -> reduce) restate the kernels' walks; with
fault=None they equal ref64, and they take the faults tests/test_conv_cases_cpu.py injects (never into a kernel)."""
import os
import sys
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

import ref64 as R
from sparse_cases import FACTOR, bounds, excess  # noqa: F401  (one rule for every case table)

if os.path.dirname(os.path.dirname(os.path.abspath(__file__))) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from test_gpu_layer_census import BF16_FLOOR, BIAS32, CONV32  # noqa: E402,F401  (the project's floors: one figure, one place)

SENTINEL = -512.0            # exact in every format the kernels store
GUARD_ROWS = 128             # sentinel rows before the first and after the last image row of an output buffer: one 128-row tile
STATS_TOL = 2e-5             # the statistics partials, per table (test_conv_x3_fp32_accurate's figure)
FWD, DGRAD = 0, 1            # DF_CONV_FWD / DF_CONV_DGRAD
EPI = {"bias": 0, "stats": 1, "gelu": 2}
E_SHAPE, E_ARG = -1, -3

F_GEN = ("mp", "mpbf16", "amax", "h2f", "h2fwp")
F_TAIL = F_GEN + ("yh2", "ybf16")
F_HALO = F_GEN + ("x3", "h2", "w16")
BF16_OPERAND_FORMS = ("mpbf16", "w16")           # bound against the reference on bf16-rounded operands
# forms whose bound takes the sequential fp32 chain over taps x cin (chain32) instead of ref64's blocked fp32 evaluation: none needed it
CHAIN_FORMS: Tuple[str, ...] = ()

L4 = (("fwd", "bias", False), ("fwd", "gelu", False), ("dgrad", "bias", False), ("dgrad", "bias", True))


# ---- forward / data gradient ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Prob:
    case: str
    cin: int
    cout: int
    k: int
    stride: int
    n: int
    h: int
    w: int
    mode: str                 # fwd / dgrad
    epi: str                  # bias / gelu / stats
    acc: bool = False
    grp: int = 0              # images per group (0: one group of n)
    views: bool = False
    seed: int = 0

    @property
    def ho(self):
        return R._out_hw(self.h, self.w, self.k, self.stride)[0]

    @property
    def wo(self):
        return R._out_hw(self.h, self.w, self.k, self.stride)[1]

    @property
    def in_shape(self):       # the tensor the kernel reads
        return (self.n, self.h, self.w, self.cin) if self.mode == "fwd" else (self.n, self.ho, self.wo, self.cout)

    @property
    def out_shape(self):      # the tensor the kernel writes
        return (self.n, self.ho, self.wo, self.cout) if self.mode == "fwd" else (self.n, self.h, self.w, self.cin)

    @property
    def M(self):
        return self.out_shape[0] * self.out_shape[1] * self.out_shape[2]

    @property
    def leg(self):
        return (f"fwd_{self.epi}" if self.mode == "fwd" else "dgrad") + ("_acc" if self.acc else "")

    @property
    def pid(self):
        return f"{self.case} {self.cin}->{self.cout} k{self.k}s{self.stride} @{self.n}x{self.h}x{self.w} {self.leg}"


CASES: Dict[str, dict] = {
    "tail64": dict(seed=51, forms=F_TAIL, why="M = 135 = 2 * 64 + 7: 64-row tiles straddle images of 45 pixels; the last tile has 7 rows"),
    "tail128": dict(seed=52, forms=F_TAIL, why="M = 4225 > 4096: 128-row tiles without a halo form; 33 full tiles and a tile of one row"),
    "n32": dict(seed=53, forms=F_GEN, why="cout % 64 != 0: variant 128032; M = 154 = 128 + 26"),
    "s2_odd": dict(seed=54, forms=F_GEN, why="stride 2 on a 9 x 13 image: the last window starts on the last row and column; odd dx: the generic path"),
    "s2_even_ragged": dict(seed=55, forms=F_GEN, why="stride-2 data gradient, dx even, 35 rows per parity class: class mode refused"),
    "s2_class": dict(seed=56, forms=F_GEN, why="stride-2 data gradient in class mode: 2 tiles and 1 tile per parity class"),
    "thin": dict(seed=57, forms=F_GEN, why="1 x 1, 1 x 40 and 40 x 1 images: whole tap rows and columns outside the image"),
    "halo_thin": dict(seed=58, forms=F_HALO, why="the haloed forms at H = 1, the W == 64 row-pair form on one pair, the 256-pixel row tile; statistics per tile"),
    "halo_odd": dict(seed=59, forms=F_HALO, why="33 full 128-row tiles on the haloed forms, odd H"),
    "views": dict(seed=60, forms=F_GEN, why="channel slices of wider buffers, two groups of two images, grp_off != 2 img_stride"),
}


def _mk(case, layers, shapes, legs, **kw) -> List[Prob]:
    out = []
    for (ci, co, k, s) in layers:
        for sh in shapes:
            n, h, w = sh[:3]
            for (mode, epi, acc) in legs:
                out.append(Prob(case, ci, co, k, s, n, h, w, mode, epi, acc, grp=(sh[3] if len(sh) > 3 else 0), **kw))
    return out


def _all_probs() -> Dict[str, List[Prob]]:
    c33 = [(64, 64, 3, 1), (64, 128, 3, 1)]
    halo = [(64, 64, 3, 1), (128, 128, 3, 1)]
    t = {
        "tail64": _mk("tail64", c33, [(3, 5, 9)], L4),
        "tail128": _mk("tail128", c33, [(1, 65, 65)], L4),
        "n32": _mk("n32", [(64, 96, 1, 1), (64, 32, 1, 1)], [(2, 7, 11)], (("fwd", "bias", False), ("fwd", "gelu", False), ("fwd", "bias", True))),
        "s2_odd": _mk("s2_odd", [(32, 64, 3, 2)], [(2, 9, 13)], L4),
        "s2_even_ragged": _mk("s2_even_ragged", [(32, 64, 3, 2)], [(1, 10, 14)], (("fwd", "bias", False),) + L4[2:]),
        "s2_class": _mk("s2_class", [(64, 64, 3, 2)], [(2, 16, 16), (1, 16, 16)], L4[2:]),
        "thin": _mk("thin", [(64, 64, 3, 1)], [(1, 1, 1), (2, 1, 40), (2, 40, 1)], (L4[0], L4[2])),
        "halo_thin": _mk("halo_thin", halo, [(2, 1, 128, 1), (2, 2, 64, 1), (1, 3, 256)], (("fwd", "stats", False),)),
        "halo_odd": _mk("halo_odd", halo, [(1, 33, 128)], (L4[0],) + L4[2:]),
        "views": _mk("views", [(64, 64, 3, 1)], [(4, 5, 9, 2)], L4, views=True) + _mk("views", [(32, 64, 3, 2)], [(4, 9, 13, 2)], L4, views=True),
    }
    out = {}
    for name, ps in t.items():
        out[name] = [replace(p, seed=CASES[name]["seed"] * 100 + i) for i, p in enumerate(ps)]
    return out


PROBS = _all_probs()
NAMES = list(PROBS)


def forms(case: str) -> Tuple[str, ...]:
    return CASES[case]["forms"]


def refused(p: Prob, form: str) -> Optional[int]:
    """the error code the entry point documents for this problem in this form (None: it runs)"""
    if form == "yh2" and p.acc:
        return E_ARG                      # the planes of two scales do not add
    return None


_T: Dict[str, dict] = {}


def tensors(p: Prob) -> dict:
    """x = what the kernel reads (fwd: the input, dgrad: the output gradient), w [O,I,k,k], bias (fwd), scale / shift (gelu), old (acc)"""
    if p.pid not in _T:
        g = torch.Generator().manual_seed(p.seed)
        t = dict(x=torch.randn(*p.in_shape, generator=g),
                 w=torch.randn(p.cout, p.cin, p.k, p.k, generator=g) * (2.0 / (p.k * p.k * p.cin)) ** 0.5,
                 bias=torch.randn(p.cout, generator=g) * 0.1 if p.mode == "fwd" else None,
                 scale=torch.rand(p.cout, generator=g) * 0.8 + 0.6, shift=torch.randn(p.cout, generator=g) * 0.2,
                 old=torch.randn(*p.out_shape, generator=g))
        _T[p.pid] = t
    return _T[p.pid]


def kernel_weights(p: Prob) -> torch.Tensor:
    """the weight memory the entry points take: [Cout,kh,kw,Cin] forward, its transpose [Cin,kh,kw,Cout] for the data gradient"""
    w = tensors(p)["w"]
    return (w.permute(0, 2, 3, 1) if p.mode == "fwd" else w.permute(1, 2, 3, 0)).contiguous()


def _ref(p: Prob, dtype, rnd):
    t = tensors(p)
    if p.mode == "fwd":
        y = R.conv2d(t["x"], t["w"], t["bias"], p.stride, rnd=rnd, dtype=dtype)
        if p.epi == "gelu":
            y = R.gelu(y * t["scale"].to(dtype) + t["shift"].to(dtype))
    else:
        y = R.conv2d_dgrad(t["x"], t["w"], (p.h, p.w), p.stride, rnd=rnd, dtype=dtype)
    return y + t["old"].to(dtype) if p.acc else y


_REFS: Dict[str, dict] = {}


def reference(p: Prob) -> dict:
    """-> {"plain": (fp32 result, float64 result), "bf16": the same on bf16-rounded operands}, each [n, ho, wo, C] of the written tensor"""
    if p.pid not in _REFS:
        _REFS[p.pid] = {"plain": (_ref(p, torch.float32, None), _ref(p, torch.float64, None)),
                        "bf16": (_ref(p, torch.float32, R.bf16_rne), _ref(p, torch.float64, R.bf16_rne))}
    return _REFS[p.pid]


# ---- memory layouts -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Lay:
    ld: int             # floats per pixel of the buffer
    off: int            # channel offset of the slice
    grp_size: int
    img_stride: int
    grp_off: int
    lead: int           # elements before pixel 0 of image 0 (the guard)
    total: int          # elements of the whole buffer


def layout(shape, grp: int, views: bool, side: str) -> Lay:
    """side: x (what the kernel reads) or y (what it writes).  plain: contiguous images; views: the slice [off, off + c) of a wider
    buffer, a gap of 8 rows after every image and 12 more between the groups"""
    n, h, w, c = shape
    g = grp or n
    if views:
        ld, off = (c + 64, 36) if side == "x" else (c + 96, 60)
        gap, ggap = 8 * ld, 12 * ld
    else:
        ld, off, gap, ggap = c, 0, 0, 0
    img_stride = h * w * ld + gap
    grp_off = g * img_stride + ggap
    guard = max(GUARD_ROWS, 2 * w + 4) * ld
    extent = (g - 1) * img_stride + (n // g - 1) * grp_off + h * w * ld
    return Lay(ld, off, g, img_stride, grp_off, guard, guard + extent + guard)


def index(lay: Lay, shape) -> torch.Tensor:
    """[n,h,w,c] int64: the buffer position of every element of the tensor"""
    n, h, w, c = shape
    i = torch.arange(n)
    base = (i % lay.grp_size) * lay.img_stride + (i // lay.grp_size) * lay.grp_off
    pix = torch.arange(h * w) * lay.ld
    return (lay.lead + lay.off + base[:, None, None] + pix[None, :, None] + torch.arange(c)[None, None, :]).view(n, h, w, c)


# ---- the row walk ----------------------------------------------------------------------------------------------------------------
def _variant(rows, rpg, cout, epi):
    from deflow_amd._lib import call
    return call("df_conv2d_variant", rows, rpg, cout, epi)


def class_mode_asked(p: Prob) -> bool:
    """conv_plan's `cls` (csrc/conv.hip): a 3x3 stride-2 data gradient with the bias epilogue onto an image with even sides"""
    return p.mode == "dgrad" and p.stride == 2 and p.k == 3 and p.epi == "bias" and p.h % 2 == 0 and p.w % 2 == 0


def tiling(p: Prob) -> dict:
    """conv_plan's tile choice restated (the variant itself is asked from the library): -> var, bm, bn, cls (class mode taken),
    tiles [(class or None, m0, m_end)] in launch order of the row tiles"""
    _, oh, ow, C = p.out_shape
    M = p.M
    rpg = (p.grp or p.n) * oh * ow
    cls = class_mode_asked(p)
    rows = M // 4 if cls else M
    var = _variant(rows, rpg, C, EPI[p.epi])
    bm = var // 1000
    if cls and rows % bm == 0:
        tiles = [(c, t * bm, (t + 1) * bm) for c in range(4) for t in range(rows // bm)]
        return dict(var=var, bm=bm, bn=var % 1000, cls=True, tiles=tiles, m_end=rows)
    if cls:
        var = _variant(M, rpg, C, EPI[p.epi])
        bm = var // 1000
    tiles = [(None, m0, m0 + bm) for m0 in range(0, M, bm)]
    return dict(var=var, bm=bm, bn=var % 1000, cls=False, tiles=tiles, m_end=M)


def decode(p: Prob, m: torch.Tensor, cls: Optional[int], swap: bool = False):
    """RowDecode: GEMM row -> (image, output row, output column); swap: the fault that divides by H where W belongs"""
    _, oh, ow, _ = p.out_shape
    if cls is None:
        n = m // (oh * ow)
        rem = m - n * oh * ow
        d = oh if swap else ow
        oy = rem // d
        return n, oy, rem - oy * d
    hh, wh, py, px = oh // 2, ow // 2, cls >> 1, cls & 1
    n = m // (hh * wh)
    rem = m - n * hh * wh
    yy = rem // wh
    return n, 2 * yy + py, 2 * (rem - yy * wh) + px


def rows64(p: Prob, n, oy, ox, fault: Optional[str] = None, dtype=torch.float64, chain: bool = False) -> torch.Tensor:
    """the output rows at (n, oy, ox), tap by tap over the flattened input as the kernels address it: pixel (qy Ws + qx) of image n, zero
    where (qy, qx) is outside the image.  faults: `tap_wrap` -- a tap left or right of the image reads the address it computes, the end of
    the neighbouring row; `cross_image` -- a tap above or below reads the neighbouring image.  chain: one sequential sum over taps x
    channels in `dtype` (the worst order a correct kernel may use).  The epilogue (bias, BatchNorm + GELU) is applied; `old` is not"""
    t = tensors(p)
    N, Hs, Ws, Cs = p.in_shape
    src = t["x"].to(dtype).reshape(N * Hs * Ws, Cs)
    w = t["w"].to(dtype)
    pad = p.k // 2
    out = torch.zeros(n.numel(), p.out_shape[3], dtype=dtype)
    for ky in range(p.k):
        for kx in range(p.k):
            if p.mode == "fwd":
                qy, qx = oy * p.stride + ky - pad, ox * p.stride + kx - pad
                ok = torch.ones_like(qy, dtype=torch.bool)
                wt = w[:, :, ky, kx].T                     # [cin, cout]
            else:
                ty, tx = oy + pad - ky, ox + pad - kx
                ok = (ty % p.stride == 0) & (tx % p.stride == 0)
                qy, qx = ty // p.stride, tx // p.stride
                wt = w[:, :, ky, kx]                       # [cout, cin]
            iny, inx = (qy >= 0) & (qy < Hs), (qx >= 0) & (qx < Ws)
            flat = qy * Ws + qx
            if fault == "tap_wrap":
                inx = (flat >= 0) & (flat < Hs * Ws)
            if fault == "cross_image":
                g = n * Hs * Ws + flat
                iny = (g >= 0) & (g < N * Hs * Ws)
            ok = ok & iny & inx
            rows = src[(n * Hs * Ws + flat).clamp(0, N * Hs * Ws - 1)] * ok[:, None]
            if chain:
                for c in range(Cs):
                    out += rows[:, c:c + 1] * wt[c][None, :]
            else:
                out += rows @ wt
    if t["bias"] is not None:
        out = out + t["bias"].to(dtype)
    if p.epi == "gelu":
        out = R.gelu(out * t["scale"].to(dtype) + t["shift"].to(dtype))
    return out


def restate(p: Prob, fault: Optional[str] = None) -> torch.Tensor:
    """the written tensor, tile by tile in float64: a buffer of SENTINEL (accumulate: the old values) into which every tile stores the rows
    m0 <= m < min(m0 + bm, m_end).  faults: `drop_ragged` / `dup_ragged` -- the last, ragged tile is not stored / is applied twice;
    `swap_hw` -- the loaders decode rows with H and W swapped; `tap_wrap`, `cross_image` -- rows64's"""
    tl = tiling(p)
    out = tensors(p)["old"].double().clone() if p.acc else torch.full(p.out_shape, SENTINEL, dtype=torch.float64)
    last = len(tl["tiles"]) - 1
    for j, (cls, m0, m1) in enumerate(tl["tiles"]):
        ragged = m1 > tl["m_end"]
        if ragged and j == last and fault == "drop_ragged":
            continue
        m = torch.arange(m0, min(m1, tl["m_end"]))
        n, oy, ox = decode(p, m, cls)
        ln, ly, lx = decode(p, m, cls, swap=True) if fault == "swap_hw" else (n, oy, ox)
        rows = rows64(p, ln, ly, lx, fault if fault in ("tap_wrap", "cross_image") else None)
        for _ in range(2 if (ragged and j == last and fault == "dup_ragged") else 1):
            out[n, oy, ox] = (out[n, oy, ox] if p.acc else 0.0) + rows
    return out


def chain32(p: Prob) -> torch.Tensor:
    """the reference as ONE sequential float32 chain over taps x channels per output element (then the epilogue and the old value)"""
    _, oh, ow, _ = p.out_shape
    n, oy, ox = decode(p, torch.arange(p.M), None)
    y = rows64(p, n, oy, ox, dtype=torch.float32, chain=True).view(p.out_shape)
    return y + tensors(p)["old"] if p.acc else y


def stats_layout(p: Prob, form: str) -> Tuple[int, int]:
    """(rows of y per statistics tile, table rows per tile): df_conv2d_tile_m rows and one table row, except the 256-pixel row tile of the
    x3 / h2 forms at 64 output channels, which fills two table rows (sums, then zeros: stats_mul)"""
    from deflow_amd._lib import call
    _, oh, ow, C = p.out_shape
    rpg = (p.grp or p.n) * oh * ow
    tm = call("df_conv2d_tile_m", rpg, C)
    two = ow == 64 and oh % 2 == 0
    wide = form in ("x3", "h2") and not two and C % 128 != 0 and ow % 256 == 0 and p.M % 256 == 0 and rpg % 256 == 0
    return (256, 2) if wide else (tm, 1)


def stats64(p: Prob, y64: torch.Tensor, form: str) -> torch.Tensor:
    """the partial table [M / tile_m, C, 2] (sum, sum of squares per tile and channel) of the float64 result"""
    rows, mul = stats_layout(p, form)
    C = y64.shape[-1]
    yt = y64.reshape(-1, rows, C)
    tab = torch.zeros(yt.shape[0], mul, C, 2, dtype=torch.float64)
    tab[:, 0, :, 0] = yt.sum(1)
    tab[:, 0, :, 1] = (yt * yt).sum(1)
    return tab.reshape(-1, C, 2)


# ---- weight gradient --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class WProb:
    case: str
    cin: int
    cout: int
    k: int
    stride: int
    n: int
    h: int
    w: int
    splits: Tuple[int, ...]            # 0 = the count the library's own *_splits function returns
    grp: int = 0
    views: bool = False
    row_counts: Optional[Tuple[int, ...]] = None
    rows_per_seg: int = 0
    seed: int = 0

    @property
    def ho(self):
        return R._out_hw(self.h, self.w, self.k, self.stride)[0]

    @property
    def wo(self):
        return R._out_hw(self.h, self.w, self.k, self.stride)[1]

    @property
    def pid(self):
        return f"{self.case} {self.cin}->{self.cout} k{self.k}s{self.stride} @{self.n}x{self.h}x{self.w}"


W_MP = ("mp", "mpbf16")
WCASES: Dict[str, dict] = {
    "w_ragged": dict(seed=71, forms=W_MP, why="one chunk per row, 9 of 32 pixels valid; a split starts mid-image and crosses an image; an empty ninth split"),
    "w_two_seg": dict(seed=72, forms=W_MP, why="chunks of 32 + 8 pixels; a split begins on the second chunk of a row; an empty sixteenth split"),
    "w_x3": dict(seed=73, forms=W_MP + ("x3", "h2", "bf16"), why="W % 32 == 0: the x3 / fp16x2 / bf16-storage forms; fewer stages than the ring is deep"),
    "w_s2_odd": dict(seed=74, forms=W_MP + ("s2h2", "s2bf16"), why="16-pixel chunks 16 + 16 + 2, the input patch runs over the right border, half a ci tile idle"),
    "w_k96": dict(seed=75, forms=W_MP + ("x3", "h2", "bf16"), why="cin = 96: one and a half ci tiles; three co tiles"),
    "w_1x1": dict(seed=76, forms=W_MP + ("w1h2", "w1bf16"), why="the 1x1 tile forms with 11 of 32 pixels valid per chunk"),
    "w_rows": dict(seed=77, forms=W_MP, why="row_counts on both sides of a chunk boundary, an empty segment; 8 chunks in 5 splits: the fifth empty"),
    "w_views": dict(seed=78, forms=W_MP + ("s2h2", "s2bf16"), why="groups, channel slices, dw at an offset with ld_co wider than a row, accumulate"),
}


def _all_wprobs() -> Dict[str, List[WProb]]:
    t = {
        "w_ragged": [WProb("w_ragged", 64, 64, 3, 1, 3, 5, 9, (1, 2, 15, 9))],
        "w_two_seg": [WProb("w_two_seg", 64, 64, 3, 1, 2, 15, 40, (1, 7, 9, 60, 16, 0))],
        "w_x3": [WProb("w_x3", ci, 64, 3, 1, 2, 3, 64, (1, 5, 12, 8)) for ci in (64, 32)],
        "w_s2_odd": [WProb("w_s2_odd", 32, 64, 3, 2, 2, 9, 67, (1, 4, 7, 0))],
        "w_k96": [WProb("w_k96", 96, 192, 3, 1, 1, 4, 32, (1, 4, 3, 0))],
        "w_1x1": [WProb("w_1x1", ci, co, 1, 1, 2, 7, 11, (1, 3, 8, 0)) for ci, co in ((64, 64), (128, 128), (96, 128))],
        "w_rows": [WProb("w_rows", 64, 64, 1, 1, 1, 1, 240, (1, 3, 5, 0), row_counts=(0, 1, 31, 32, 33, 40), rows_per_seg=40)],
        "w_views": [WProb("w_views", 64, 64, 3, 1, 4, 5, 9, (2, 0), grp=2, views=True),
                    WProb("w_views", 32, 64, 3, 2, 4, 9, 67, (7, 0), grp=2, views=True)],
    }
    out = {}
    for name, ps in t.items():
        out[name] = [replace(p, seed=WCASES[name]["seed"] * 100 + i) for i, p in enumerate(ps)]
    return out


WPROBS = _all_wprobs()
WNAMES = list(WPROBS)


def wforms(case: str, p: Optional[WProb] = None) -> Tuple[str, ...]:
    f = WCASES[case]["forms"]
    if p is not None and p.k == 3 and p.stride == 1:
        f = tuple(x for x in f if not x.startswith("s2"))        # (w_views: the stride-2 forms take its stride-2 layer only)
    return f


def wtensors(p: WProb) -> dict:
    if p.pid not in _T:
        g = torch.Generator().manual_seed(p.seed)
        _T[p.pid] = dict(x=torch.randn(p.n, p.h, p.w, p.cin, generator=g), dy=torch.randn(p.n, p.ho, p.wo, p.cout, generator=g),
                         old=torch.randn(p.cout, p.cin, p.k, p.k, generator=g))
    return _T[p.pid]


def chunk_pixels(p: WProb) -> int:
    """output pixels per chunk: wgrad_chunk() of csrc/conv_wgrad.hip with the default switches"""
    return 16 if (p.k == 3 and p.stride == 2) else 32


def wchunks(p: WProb):
    """-> (P, chunks per row, [(image, output row, first column)] in the kernels' order): wg_chunk restated"""
    P = chunk_pixels(p)
    cpr = (p.wo + P - 1) // P
    return P, cpr, [(ch // cpr // p.ho, ch // cpr % p.ho, ch % cpr * P) for ch in range(p.n * p.ho * cpr)]


def split_ranges(total: int, splits: int) -> List[Tuple[int, int]]:
    """chunks_per_split, c_begin, c_end: [(first chunk, one past the last)] per split (an empty range where the count overshoots)"""
    cps = (total + splits - 1) // splits
    return [(min(s * cps, total), min(s * cps + cps, total)) for s in range(splits)]


def row_ok(p: WProb) -> torch.Tensor:
    """wg_row_ok over the pixels of an image row: [wo] bool"""
    if p.row_counts is None:
        return torch.ones(p.wo, dtype=torch.bool)
    px = torch.arange(p.wo)
    return (px % p.rows_per_seg) < torch.tensor(p.row_counts)[px // p.rows_per_seg]


def split_mask(p: WProb, lo: int, hi: int, fault: Optional[str] = None) -> torch.Tensor:
    """[n, ho, wo] bool: the output-gradient pixels the chunks lo .. hi - 1 multiply.  faults: `skip_last_chunk` -- the last chunk of every
    row is left out; `ignore_row_counts`"""
    P, cpr, chunks = wchunks(p)
    ok = torch.ones(p.wo, dtype=torch.bool) if fault == "ignore_row_counts" else row_ok(p)
    m = torch.zeros(p.n, p.ho, p.wo, dtype=torch.bool)
    for ch in range(lo, hi):
        n, oy, ox0 = chunks[ch]
        if fault == "skip_last_chunk" and ox0 // P == cpr - 1:
            continue
        m[n, oy, ox0:min(ox0 + P, p.wo)] = ok[ox0:min(ox0 + P, p.wo)]
    return m


def _wgrad(p: WProb, mask: torch.Tensor, dtype, rnd=None):
    t = wtensors(p)
    return R.conv2d_wgrad(t["x"], t["dy"] * mask[..., None], p.k, p.stride, rnd=rnd, dtype=dtype)


def phantom64(p: WProb) -> torch.Tensor:
    """the fault `count_invalid`: what a ragged chunk adds if its pixels past the end of the row are multiplied too, at the addresses they
    compute -- the output gradient of the next row's first pixels against the input pixels behind the row's end (float64 dw)"""
    t = wtensors(p)
    P, cpr, _ = wchunks(p)
    x, dy = t["x"].double().reshape(p.n, p.h * p.w, p.cin), t["dy"].double().reshape(p.n, p.ho * p.wo, p.cout)
    dw = torch.zeros(p.cout, p.cin, p.k, p.k, dtype=torch.float64)
    pad = p.k // 2
    for n in range(p.n):
        for oy in range(p.ho):
            for ox in range(p.wo, cpr * P):
                fy = oy * p.wo + ox
                if fy >= p.ho * p.wo:
                    continue
                for ky in range(p.k):
                    iy = oy * p.stride + ky - pad
                    if not 0 <= iy < p.h:
                        continue
                    for kx in range(p.k):
                        fx = iy * p.w + ox * p.stride + kx - pad
                        if 0 <= fx < p.h * p.w:
                            dw[:, :, ky, kx] += torch.outer(dy[n, fy], x[n, fx])
    return dw


def partials64(p: WProb, splits: int, fault: Optional[str] = None):
    """the split-K workspaces [splits, O, I, k, k] and [splits, O] over NaN, in float64: split s writes the sums of its chunks, zeros if it
    has none.  faults: split_mask's, and `count_invalid` (phantom64, booked on the first split)"""
    _, _, chunks = wchunks(p)
    ws = torch.full((splits, p.cout, p.cin, p.k, p.k), float("nan"), dtype=torch.float64)
    bws = torch.full((splits, p.cout), float("nan"), dtype=torch.float64)
    for s, (lo, hi) in enumerate(split_ranges(len(chunks), splits)):
        ws[s], bws[s] = _wgrad(p, split_mask(p, lo, hi, fault), torch.float64)
    if fault == "count_invalid":
        ws[0] += phantom64(p)
    return ws, bws


def reduce64(ws: torch.Tensor, fault: Optional[str] = None) -> torch.Tensor:
    """df_conv2d_wgrad_reduce: the sum over the splits.  fault `lose_split`: the middle split is left out"""
    if fault == "lose_split":
        keep = [s for s in range(ws.shape[0]) if s != ws.shape[0] // 2]
        return ws[keep].sum(0)
    return ws.sum(0)


_WREFS: Dict[str, dict] = {}


def wreference(p: WProb) -> dict:
    """-> {"plain": ((dw32, db32), (dw64, db64)), "bf16": the same on bf16-rounded operands}: dw [O,I,k,k], db [O]"""
    if p.pid not in _WREFS:
        m = split_mask(p, 0, len(wchunks(p)[2]))
        _WREFS[p.pid] = {"plain": (_wgrad(p, m, torch.float32), _wgrad(p, m, torch.float64)),
                         "bf16": (_wgrad(p, m, torch.float32, R.bf16_rne), _wgrad(p, m, torch.float64, R.bf16_rne))}
    return _WREFS[p.pid]


def wsplits(p: WProb, form: str, x, dy) -> List[int]:
    """the problem's split counts, 0 replaced by what the form's own *_splits function returns for the descriptors x, dy"""
    from deflow_amd._lib import call
    own = (call("df_conv2d_wgrad1_h2_splits", x, dy) if form.startswith("w1") else call("df_conv2d_wgrad_s2_h2_splits", x, dy)
           if form.startswith("s2") else call("df_conv2d_wgrad_splits", x, dy, p.k, p.stride))
    out = []
    for s in p.splits:
        s = s or own
        if s not in out:
            out.append(s)
    return out


# ---- the reductions on their own ---------------------------------------------------------------------------------------------------
REDUCE_SPLITS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 57)
REDUCE_SHAPE = dict(taps=9, cin=36, pad=20)                # rows of 324 floats, ld_co = 324 + 20
REDUCE_COUTS = (64, 65)      # 64 x 324 = 81 whole blocks of 256 threads; 65 x 324 leaves the last block 68, and the bias part a column alone


def reduce_case(splits: int, cout: int):
    """-> ws [splits, cout, 324], bias_ws [splits, cout], old [cout, 324] (fp32, seeded)"""
    g = torch.Generator().manual_seed(900 + splits + 1000 * cout)
    c, r = cout, REDUCE_SHAPE["taps"] * REDUCE_SHAPE["cin"]
    return torch.randn(splits, c, r, generator=g), torch.randn(splits, c, generator=g), torch.randn(c, r, generator=g)


def reduce_refs(ws: torch.Tensor, old: Optional[torch.Tensor]):
    """-> (the sum over the splits as one sequential float32 chain (+ old), the float64 sum (+ old))"""
    s32 = torch.zeros_like(ws[0])
    for k in range(ws.shape[0]):
        s32 = s32 + ws[k]
    s64 = ws.double().sum(0)
    return (s32, s64) if old is None else (s32 + old, s64 + old.double())


def ulp32(v: torch.Tensor) -> torch.Tensor:
    """one float32 ulp at |v| (float64 in and out)"""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23.0)
