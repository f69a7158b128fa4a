"""Bird's-eye-view flow images rasterised on the GPU (csrc/render.hip; definition: include/deflow_amd.h and DESIGN.md section 6i,
UNPINNED): what ``python -m deflow_amd.vis`` draws with.

* ``render_rows``: rows + a vector and a class per row -> PNG scanlines ``[B, H, 1 + 3W]`` u8 (``png.write_png`` frames them).  A 64-bit
  atomic maximum per covered pixel decides what is seen, so the image does not depend on the execution order;
* ``flow_vectors``: a flow of raw rows minus their pose flow (``df_ego_transform``'s), the vector the colour shows.

CUDA tensors only: there is no CPU fallback (tests/helpers/render_ref.py restates the definition in numpy).  Nothing is read back."""
from __future__ import annotations

import functools
import math
from typing import Sequence, Tuple

import torch

from ._lib import call, ptr, stream
from .args import cloud, tensor

MAX_SIDE = 4096
MAX_RADIUS = 4


_check = functools.partial(tensor, "render", other="points is")
_rows = functools.partial(cloud, "render", rows_limit=1)


def _number(name: str, v, positive: bool) -> float:
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"render: {name} must be a number, got {v!r}") from None
    if not math.isfinite(v) or (positive and not v > 0):
        raise ValueError(f"render: {name} must be {'positive and ' if positive else ''}finite, got {v!r}")
    return v


def check_image(B: int, size: Sequence[int], radius: int = 0, bg: Sequence[int] = (24, 24, 24), legend: int = 0) -> Tuple[int, int, int]:
    """the image's guards (the entry points' own, restated so that the error names the argument) -> W, H, bg as 0xRRGGBB"""
    if not isinstance(size, (tuple, list)) or len(size) != 2 or not all(isinstance(v, int) and not isinstance(v, bool) for v in size):
        raise ValueError(f"render: size must be (W, H), two integers, got {size!r}")
    W, H = size
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f"render: size: 1 <= W, H <= {MAX_SIDE} expected, got {W} x {H}")
    if B * H * (1 + 3 * W) >= 2 ** 31:
        raise ValueError(f"render: size: B * H * (1 + 3 W) < 2^31 expected, got B = {B}, {W} x {H}")
    if not isinstance(radius, int) or isinstance(radius, bool) or not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"render: radius must be an integer in 0 .. {MAX_RADIUS}, got {radius!r}")
    if not isinstance(bg, (tuple, list)) or len(bg) != 3 or not all(isinstance(v, int) and 0 <= v <= 255 for v in bg):
        raise ValueError(f"render: bg must be (R, G, B) with integers in 0 .. 255, got {bg!r}")
    if not isinstance(legend, int) or isinstance(legend, bool) or legend < 0 or (legend > 0 and 2 * legend + 5 > min(W, H)):
        raise ValueError(f"render: legend must be 0 or a radius L with 2 L + 5 <= min(W, H) = {min(W, H)}, got {legend!r}")
    return W, H, (bg[0] << 16) | (bg[1] << 8) | bg[2]


def render_rows(points: torch.Tensor, count: torch.Tensor, vec: torch.Tensor, cls: torch.Tensor, *, view: Sequence[float],
                size: Sequence[int], vmax: float, radius: int = 1, bg: Sequence[int] = (24, 24, 24), legend: int = 0) -> torch.Tensor:
    """points, vec [B,N,3] f32, count [B] i32 valid leading rows, cls [B,N] u8 (0 = not drawn, 1 = the colour of ``vec``, 2 = grey);
    view = (xmin, ymin, inv_res), size = (W, H) -> scanlines [B, H, 1 + 3W] u8: per line a 0 filter byte and W RGB pixels, x to the right,
    y up.  ``legend`` = L > 0 puts a colour-wheel disc of radius L into the top right corner.  The intermediate image comes from torch's
    allocator and is zeroed on the current stream: the op can be captured in a graph.  Two calls are bit-identical."""
    B, N = _rows("points", points)
    dev = points.device
    _check("vec", vec, torch.float32, (B, N, 3), dev)
    _check("cls", cls, torch.uint8, (B, N), dev)
    _check("count", count, torch.int32, (B,), dev)
    if not isinstance(view, (tuple, list)) or len(view) != 3:
        raise ValueError(f"render: view must be (xmin, ymin, inv_res), got {view!r}")
    xmin, ymin = _number("view[0] (xmin)", view[0], False), _number("view[1] (ymin)", view[1], False)
    inv_res = _number("view[2] (inv_res)", view[2], True)
    vmax = _number("vmax", vmax, True)
    W, H, bg_rgb = check_image(B, size, radius, bg, legend)
    points, vec, cls, count = points.detach().contiguous(), vec.detach().contiguous(), cls.contiguous(), count.contiguous()
    image = torch.zeros(B, H, W, dtype=torch.int64, device=dev)
    out = torch.empty(B, H, 1 + 3 * W, dtype=torch.uint8, device=dev)
    call("df_render_splat", ptr(points), ptr(vec), ptr(cls), ptr(count), B, N, xmin, ymin, inv_res, W, H, vmax, radius, ptr(image), stream())
    call("df_render_resolve", ptr(image), B, W, H, bg_rgb, legend, ptr(out), stream())
    return out


def flow_vectors(raw: torch.Tensor, count_raw: torch.Tensor, flow: torch.Tensor, T: torch.Tensor) -> torch.Tensor:
    """raw [B,N,3] f32, flow [B,N,3] f32 (an estimate such as ``SweepFlow.infer``'s ``flow_est``, or the ground truth), T [B,4,4] f32 ->
    fp32(flow - pose_flow) per raw row, the pose flow being ``df_ego_transform``'s: a row that ``compose_flow`` gave
    its pose flow comes out exactly 0.  Rows behind ``count_raw`` and non-finite rows hold whatever the arithmetic gives (NaN for NaN
    padding); ``render_rows`` skips them."""
    B, N = _rows("raw", raw)
    dev = raw.device
    _check("count_raw", count_raw, torch.int32, (B,), dev)
    _check("flow", flow, torch.float32, (B, N, 3), dev)
    _check("T", T, torch.float32, (B, 4, 4), dev)
    raw, T = raw.detach().contiguous(), T.contiguous()
    moved = torch.empty_like(raw)
    pose_flow = torch.empty_like(raw)
    call("df_ego_transform", ptr(raw), ptr(T), B, N, ptr(moved), ptr(pose_flow), stream())
    return torch.sub(flow.detach(), pose_flow)          # one IEEE subtraction per element
