"""Rectangular, non-power-of-two BEV grids: the one table behind tests/test_gpu_rect_grids.py, the census runs D / E of
tests/test_gpu_layer_census.py, and tests/test_rect_cases_cpu.py (which decides on the CPU that each case is what it claims).

Order of a grid: grid_feature_size = [H, W] = [ny, nx] (train.grid_from): H counts the y extent of point_cloud_range, W the x
extent.  Every range below is the grid at 0.2 m voxels, centred on the origin.

Clouds come from synth_pair(seed + b, N, grid_hw=(max(H, W),) * 2): the square of the LONG side, so the cloud overfills the short
axis only -- rows leave through the range on one axis, and an engine that swapped H and W would drop (and keep) different rows.

SELECTION is the kernel-form table of the issue this file answers: per (grid, B, stage) what the library's host-side queries return
for a stage's 3x3 stride-1 layers, asked with descriptors of 2B images as unet._h2p_ok / unet._stage_store16_ok ask (selection()
below).  tests/test_rect_cases_cpu.py asserts the library still answers this way."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Tuple

import torch

VOXEL = 0.2
STAGE_C = (64, 128, 256)      # output channels of encoder stages 1, 2, 3 (strides 2, 4, 8)


@dataclass(frozen=True)
class Case:
    name: str
    H: int
    W: int
    B: int
    N: int
    seed: int
    why: str
    oracle: bool = True       # small enough for the CPU oracle (the census shapes are checked on the GPU in float64 instead)

    @property
    def grid(self):
        return [self.H, self.W]

    @property
    def point_cloud_range(self):
        hx, hy = round(self.W * VOXEL / 2, 6), round(self.H * VOXEL / 2, 6)
        return [-hx, -hy, -3, hx, hy, 3]

    @property
    def cfg(self) -> dict:
        return dict(voxel_size=[VOXEL, VOXEL, 6], point_cloud_range=self.point_cloud_range, grid_feature_size=self.grid)

    def stage_hw(self, k: int) -> Tuple[int, int]:
        return self.H >> k, self.W >> k

    def rows_pg(self, k: int) -> int:
        """rows of one BatchNorm statistic group (one cloud's B images) at encoder stage k"""
        h, w = self.stage_hw(k)
        return self.B * h * w


CASES: Dict[str, Case] = {c.name: c for c in (
    Case("64x96", 64, 96, 2, 1500, 100, "generic conv forms; 64-row statistic tiles over 96-pixel images at stage 3 (tiles straddle images)"),
    Case("96x64", 96, 64, 2, 1500, 110, "the transpose of 64x96: an H / W swap anywhere in the engine shows against the oracle"),
    Case("40x72", 40, 72, 2, 1500, 120, "5 x 9 at stride 8 (odd on both axes); legal in eval, violates the training tile rule (90 rows per group)"),
    Case("96x256", 96, 256, 2, 6000, 130, "fp16x2 halo form (W = 128), row-pair form (W = 64), generic form (W = 32); bf16-tile forms at stages 1-2"),
    Case("256x96", 256, 96, 2, 6000, 140, "the transpose of 96x256: generic forms at W = 48 / 24 / 12 with the same pixel counts"),
    Case("320x512", 320, 512, 16, 50000, 20240116, "census run D: the smallest rectangular shape on which every benchmarked fp32 form is selected; "
         "h = 160 / 80 / 40 and every h*w are no powers of two", oracle=False),
    Case("320x512_b8", 320, 512, 8, 50000, 20240116, "selection only: at B = 8 stage 3 falls below the pre-split forms' tile count", oracle=False),
    Case("192x256", 192, 256, 16, 20000, 4242, "census run E (bf16 mode): bf16-tile forms at stages 1-2, generic at stage 3; h = 96 / 48 / 24", oracle=False),
)}

# (case, stage) -> tile_m, h2p (forward, data gradient, weight gradient), w16 (forward with stats, data gradient), x3
SELECTION = {
    ("320x512", 1): (128, (1, 1, 1), (1, 1), 1),
    ("320x512", 2): (128, (1, 1, 1), (1, 1), 1),
    ("320x512", 3): (128, (1, 1, 1), (1, 1), 1),
    ("320x512_b8", 3): (128, (0, 0, 1), (1, 1), 1),
    ("192x256", 1): (128, (0, 0, 1), (1, 1), 1),
    ("192x256", 2): (128, (0, 0, 1), (1, 1), 1),
    ("192x256", 3): (128, (0, 0, 1), (0, 0), 0),
    ("96x256", 1): (128, (0, 0, 1), (1, 1), 1),
    ("96x256", 2): (128, (0, 0, 1), (1, 1), 1),
    ("96x256", 3): (128, (0, 0, 1), (0, 0), 0),
    ("64x96", 1): (128, (0, 0, 0), (0, 0), 0),
    ("64x96", 2): (128, (0, 0, 0), (0, 0), 0),
    ("64x96", 3): (64, (0, 0, 0), (0, 0), 0),
}


def case(name: str) -> Case:
    return CASES[name]


def selection(c: Case, k: int):
    """what the library answers for the 3x3 stride-1 layers of encoder stage k of case c, in SELECTION's layout.  Host-side queries on
    descriptors of that shape (2B images, one group): nothing is launched and no GPU is needed."""
    from deflow_amd import ops
    from deflow_amd._lib import DfImg, call
    n, (h, w), C = 2 * c.B, c.stage_hw(k), STAGE_C[k - 1]
    probe = torch.empty(64, dtype=torch.float32)
    base = (probe.data_ptr() + 127) // 128 * 128

    def d(elt):
        return DfImg(base, n, h, w, C, C, n, h * w * C, 0, elt, 0)
    f32, b16, h2 = d(0), d(1), d(2)
    h2p = (call("df_conv2d_h2p_ok", h2, f32, 3, 1, ops.CONV_FWD, ops.EPI_BIAS), call("df_conv2d_h2p_ok", h2, f32, 3, 1, ops.CONV_DGRAD, ops.EPI_BIAS),
           call("df_conv2d_wgrad_h2p_ok", h2, h2, 3, 1))
    w16 = (call("df_conv2d_w16_ok", b16, b16, 3, 1, ops.CONV_FWD, ops.EPI_STATS), call("df_conv2d_w16_ok", b16, b16, 3, 1, ops.CONV_DGRAD, ops.EPI_BIAS))
    x3 = call("df_conv2d_x3_ok", f32, f32, 3, 1, ops.CONV_FWD, ops.EPI_STATS)
    return ops.conv_tile_m(c.rows_pg(k), C), h2p, w16, x3


def make_batch(c: Case) -> Dict[str, torch.Tensor]:
    """tests/test_gpu_model.py's make_batch on the square of the case's long side"""
    from deflow_amd.synth import synth_pair
    side = max(c.H, c.W)
    pairs = [synth_pair(c.seed + b, c.N, grid_hw=(side, side)) for b in range(c.B)]
    return {"pc0": torch.stack([p[0] for p in pairs]), "pc1": torch.stack([p[1] for p in pairs]),
            "pose0": torch.stack([torch.eye(4) for _ in pairs]),
            "pose1": torch.stack([torch.linalg.inv(p[2]) for p in pairs]),
            "flow": torch.stack([p[3] for p in pairs])}


def oracle(c: Case, seed: int, **kw):
    """the CPU oracle on the case's grid with scattered BatchNorm affine parameters and running statistics (test_gpu_model.build_pair)"""
    from oracle import ref_torch as O
    torch.manual_seed(seed)
    ref = O.DeFlow(**c.cfg, **kw)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.uniform_(0.6, 1.4); m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.3, 0.3); m.running_var.uniform_(0.6, 1.5)
    return ref
