"""A depth cube about the sensor: the range-image visibility test that tells which rows of a cloud the current sweep sees through.

UNPINNED: this project's own definition -- include/deflow_amd.h and DESIGN.md section 6u.  A direction from the origin is filed on one of
the six faces of a cube with ``res`` x ``res`` bins each; a bin holds the smallest depth (absolute major coordinate) of the sweep's rows
filed there.  A query row is SEEN THROUGH when the sweep has a return well behind it in its own bin's neighbourhood.  No transcendental
function and every fp32 operation rounded once, so numpy float32 reproduces every value bit for bit.

CUDA tensors only: there is no CPU fallback.  ``build`` is df_depth_cube_build (a fill and one integer atomicMin per row), ``seen_through``
is df_depth_cube_test; nothing reads a device value back and no grid dimension comes from one."""
from __future__ import annotations

import functools
from typing import Dict, Optional

import torch

from ._lib import call, ptr, stream
from .args import cloud, integer, labels, nonneg, tensor

_tensor = functools.partial(tensor, other="the cube is")
RES_MAX, HALO_MAX = 2048, 4


def check_params(fn: str, p: Dict[str, object]) -> Dict[str, object]:
    """(res, halo, margin, rel, near) of ``p``, those present, held to the entries' limits under the names ``fn`` knows them by"""
    if "res" in p:
        integer(fn, p, "res", 2, RES_MAX)
        if p["res"] % 2:
            raise ValueError(f"{fn}: res must be even, got {p['res']!r}")
    if "halo" in p:
        integer(fn, p, "halo", 0, HALO_MAX)
    for k in ("margin", "rel", "near"):
        if k in p:
            nonneg(fn, p, k)
    return p


class DepthCube:
    """img [B,6,res,res] u32 held as int32: the bit pattern of the smallest depth per bin, 0x7F800000 (+inf) where there is none"""

    def __init__(self, B: int, res: int, device):
        p = check_params("DepthCube", {"B": B, "res": res})
        integer("DepthCube", p, "B", 1, 65535)
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError("DepthCube: device must be a CUDA device (deflow_amd has no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.B, self.res, self.dev = p["B"], p["res"], device
        if self.B * 6 * self.res * self.res >= 2 ** 30:
            raise ValueError(f"DepthCube: B = {self.B} cubes of 6 x {self.res} x {self.res} bins are beyond the entries' limit (6 B res^2 < 2^30)")
        self.img = torch.empty(self.B, 6, self.res, self.res, dtype=torch.int32, device=device)

    def _cloud(self, fn: str, points, count):
        B, N = cloud(fn, "points", points)
        if B != self.B or points.device != self.dev:
            raise ValueError(f"{fn}: points must hold {self.B} samples on {self.dev}, got {B} on {points.device}")
        if B * N >= 2 ** 30:
            raise ValueError(f"{fn}: B = {B} samples of {N} rows are beyond the entries' limit (B N < 2^30)")
        _tensor(fn, "count", count, torch.int32, (B,), self.dev)
        return B, N, points.detach().contiguous(), count.contiguous()

    def build(self, points: torch.Tensor, count: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """file points [B,N,3] f32 (count [B] i32 valid leading rows, optional integer / bool mask [B,N]: rows with mask > 0 take part)
        -> .img, replaced in place"""
        fn = "DepthCube.build"
        B, N, points, count = self._cloud(fn, points, count)
        lab = labels(fn, "mask", mask, (B, N), f"must be an integer or bool CUDA tensor of shape {(B, N)} on {self.dev}", self.dev)
        call("df_depth_cube_build", ptr(points), ptr(count), ptr(lab), B, N, self.res, ptr(self.img), stream())
        return self.img

    def seen_through(self, points: torch.Tensor, count: torch.Tensor, *, halo: int, margin: float, rel: float, near: float,
                     depth: bool = False):
        """flag [B,M] i32 of points [B,M,3] f32 (count [B] i32) against the cube as built: 1 where (depth * fp32(1 + rel)) + margin is
        smaller than the smallest depth in the (2 halo + 1)^2 bins about the row's own (include/deflow_amd.h).  depth=True: (flag, dmin
        [B,M] f32)"""
        fn = "DepthCube.seen_through"
        p = check_params(fn, {"halo": halo, "margin": margin, "rel": rel, "near": near})
        B, M, points, count = self._cloud(fn, points, count)
        flag = torch.empty(B, M, dtype=torch.int32, device=self.dev)
        dmin = torch.empty(B, M, dtype=torch.float32, device=self.dev) if depth else None
        call("df_depth_cube_test", ptr(points), ptr(count), ptr(self.img), B, M, self.res, p["halo"], p["margin"], p["rel"], p["near"],
             ptr(flag), ptr(dmin), stream())
        return (flag, dmin) if depth else flag
