"""A voxel-capped local map kept on the GPU: the target of the scan-to-map odometry (``odometry.register_sweeps(target="map")``).

UNPINNED: this project's own definition -- include/deflow_amd.h and DESIGN.md section 6t.  World-frame points (the world is the first
sweep's frame) in float64, at most ``max_per_voxel`` per cubic voxel, inside a window of (2 W + 1)^2 voxel columns about the sensor,
W = ceil(max_range / voxel) + 1.  Older points win: a full voxel refuses every new point, and a point that leaves the window is gone.

CUDA tensors only: there is no CPU fallback.  ``insert`` is df_map_keys, df_cell_sort, df_map_select, df_map_compact and ``view`` is
df_map_view; nothing reads a device value back, so a recording can be queued whole before its one read-back.  ``carve`` (opt-in,
DESIGN.md section 6u) is the one way a row inside the window leaves: df_map_view, the depth cube of ``visibility`` built on the current
sweep and tested on the view, then df_map_drop.  ``evict="near"`` (opt-in, UNPINNED) makes the last call of
``insert`` df_map_compact_near: on overflow the rows of the outermost window rings go, not the end of the sorted order."""
from __future__ import annotations

import functools
import math
from typing import Optional, Tuple

import torch

from ._lib import call, ptr, stream
from .args import cloud, integer, labels, positive, tensor, workspace

_tensor = functools.partial(tensor, other="the map is")
W_MAX = 2047
EVICT = ("order", "near")


class LocalMap:
    """points [B,capacity,3] f64 (rows >= count are NaN), count [B] i32, stat [B,4] i32 of the last insert = (rows in the window, rows
    kept, kept rows that came from the sweep, overflow = kept rows that did not fit into capacity).  evict: which rows an overflow loses --
    "order": the end of the sorted order (df_map_compact); "near": the outermost rings of the window (df_map_compact_near), and then cut
    [B,2] i32 of the last insert = (R, budget), (W + 1, 0) for a sample without overflow.  Under "order" cut is None."""

    def __init__(self, B: int, capacity: int, *, voxel: float, max_per_voxel: int, max_range: float, device, evict: str = "order"):
        if evict not in EVICT:
            raise ValueError(f"LocalMap: evict must be 'order' or 'near', got {evict!r}")
        p = {"B": B, "capacity": capacity, "voxel": voxel, "max_per_voxel": max_per_voxel, "max_range": max_range}
        integer("LocalMap", p, "B", 1, 65535)
        integer("LocalMap", p, "capacity", 1, 2 ** 30 - 1)
        integer("LocalMap", p, "max_per_voxel", 1, 2 ** 31 - 1)
        positive("LocalMap", p, "voxel")
        positive("LocalMap", p, "max_range")
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError("LocalMap: device must be a CUDA device (deflow_amd has no CPU fallback)")
        if device.index is None:                                       # "cuda": the current device, under the name its tensors carry
            device = torch.device("cuda", torch.cuda.current_device())
        self.B, self.capacity, self.voxel, self.max_per_voxel = p["B"], p["capacity"], p["voxel"], p["max_per_voxel"]
        W = math.ceil(p["max_range"] / self.voxel) + 1
        S = 2 * W + 1
        if W > W_MAX or self.B * S * S >= 2 ** 30:
            raise ValueError(f"LocalMap: max_range / voxel = {p['max_range']} / {self.voxel} gives a window of {S} x {S} columns: the "
                             f"half-width must be <= {W_MAX} and B x columns < 2^30")
        self.W, self.S, self.dev = W, S, device
        self.points = torch.full((self.B, self.capacity, 3), float("nan"), dtype=torch.float64, device=device)
        self._spare = torch.empty_like(self.points)
        self.count = torch.zeros(self.B, dtype=torch.int32, device=device)
        self.stat = torch.zeros(self.B, 4, dtype=torch.int32, device=device)
        self.evict, self.cut = evict, None

    def _pose(self, fn: str, pose) -> torch.Tensor:
        _tensor(fn, "pose", pose, torch.float64, (self.B, 4, 4), self.dev)
        return pose.detach().contiguous()

    def insert(self, points: torch.Tensor, count: torch.Tensor, pose: torch.Tensor, *, mask: Optional[torch.Tensor] = None,
               gate: Optional[torch.Tensor] = None) -> None:
        """points [B,N,3] f32 in the sensor's frame with count [B] i32 valid leading rows, pose [B,4,4] f64 (world = R s + t); optional
        integer / bool mask [B,N] (rows with mask > 0 take part) and gate [B] i32 (a sample with gate != 0 inserts nothing: the
        ``status`` of the registration that made the pose).  Replaces .points, .count and .stat, and .cut under evict="near"."""
        fn = "LocalMap.insert"
        B, N = cloud(fn, "points", points)
        if B != self.B or points.device != self.dev:
            raise ValueError(f"{fn}: points must hold {self.B} samples on {self.dev}, got {B} on {points.device}")
        _tensor(fn, "count", count, torch.int32, (B,), self.dev)
        pose = self._pose(fn, pose)
        lab = labels(fn, "mask", mask, (B, N), f"must be an integer or bool CUDA tensor of shape {(B, N)} on {self.dev}", self.dev)
        if gate is not None:
            gate = _tensor(fn, "gate", gate, torch.int32, (B,), self.dev).contiguous()
        cap, W, dev = self.capacity, self.W, self.dev
        n, ncells = cap + N, B * self.S * self.S
        refused = f"{fn}: B = {B} samples of capacity + N = {n} candidate rows are beyond the entries' limits (B (capacity + N) < 2^30)"
        near = self.evict == "near"
        ws = workspace("df_map_near_ws_bytes", (B, cap, N, W), dev, refused) if near else workspace("df_map_ws_bytes", (B, cap, N), dev, refused)
        points, count = points.detach().contiguous(), count.contiguous()
        cand = torch.empty(B, n, 3, dtype=torch.float64, device=dev)
        key = torch.empty(B * n, dtype=torch.int32, device=dev)
        vz = torch.empty(B * n, dtype=torch.int32, device=dev)
        idx = torch.empty(B * n, dtype=torch.int32, device=dev)
        rng = torch.empty(ncells, 2, dtype=torch.int32, device=dev)
        keep = torch.empty(B * n, dtype=torch.int32, device=dev)
        sort_ws = workspace("df_cell_sort_ws_bytes", (ncells,), dev, refused)
        count_out = torch.empty(B, dtype=torch.int32, device=dev)
        stat = torch.empty(B, 4, dtype=torch.int32, device=dev)
        out = self._spare
        s = stream()
        call("df_map_keys", ptr(self.points), ptr(self.count), ptr(points), ptr(count), ptr(lab), ptr(gate), ptr(pose), B, cap, N,
             self.voxel, W, ptr(cand), ptr(key), ptr(vz), s)
        call("df_cell_sort", ptr(key), B * n, ncells, ptr(idx), ptr(rng), ptr(sort_ws), s)
        call("df_map_select", ptr(key), ptr(idx), ptr(rng), ptr(vz), B, n, W, self.max_per_voxel, ptr(keep), s)
        if near:
            cut = torch.empty(B, 2, dtype=torch.int32, device=dev)
            call("df_map_compact_near", ptr(cand), ptr(key), ptr(idx), ptr(rng), ptr(keep), B, cap, N, W, ptr(out), ptr(count_out),
                 ptr(stat), ptr(cut), ptr(ws), s)
            self.cut = cut
        else:
            call("df_map_compact", ptr(cand), ptr(idx), ptr(rng), ptr(keep), B, cap, N, W, ptr(out), ptr(count_out), ptr(stat), ptr(ws), s)
        self._spare, self.points, self.count, self.stat = self.points, out, count_out, stat
        self.last = {"cand": cand, "key": key, "vz": vz, "idx_sorted": idx, "cell_rng": rng, "keep": keep}     # the stages, for tests
        if near:
            self.last["cut"] = cut

    def carve(self, points: torch.Tensor, count: torch.Tensor, pose: torch.Tensor, *, mask: Optional[torch.Tensor] = None,
              gate: Optional[torch.Tensor] = None, res: int, halo: int, margin: float, rel: float, near: float) -> None:
        """drop the map rows that the sweep points [B,N,3] f32 (count, mask as in ``insert``), taken at pose [B,4,4] f64, sees through
        (UNPINNED: DESIGN.md section 6u): ``view(pose)``, a ``visibility.DepthCube`` of ``res`` bins built on the sweep, its test on the
        view (halo, margin, rel, near) and df_map_drop into the spare buffer.  A sample with gate != 0 drops nothing.  Replaces .points
        and .count, sets .carve_stat [B,2] i32 = (rows tested, rows dropped) and keeps the stages in .last_carve."""
        from .visibility import DepthCube
        fn = "LocalMap.carve"
        if gate is not None:
            gate = _tensor(fn, "gate", gate, torch.int32, (self.B,), self.dev).contiguous()
        cube = DepthCube(self.B, res, self.dev)
        B, cap, dev = self.B, self.capacity, self.dev
        ws = workspace("df_map_drop_ws_bytes", (B, cap), dev, f"{fn}: B = {B} samples of {cap} rows are beyond the entries' limits")
        dst, _ = self.view(pose)
        img = cube.build(points, count, mask)
        flag = cube.seen_through(dst, self.count, halo=halo, margin=margin, rel=rel, near=near)
        count_out = torch.empty(B, dtype=torch.int32, device=dev)
        stat = torch.empty(B, 2, dtype=torch.int32, device=dev)
        out = self._spare
        call("df_map_drop", ptr(self.points), ptr(self.count), ptr(flag), ptr(gate), B, cap, ptr(out), ptr(count_out), ptr(stat), ptr(ws),
             stream())
        self.last_carve = {"view": dst, "count": self.count, "img": img, "flag": flag}     # the stages (count: before the drop), for tests
        self._spare, self.points, self.count, self.carve_stat = self.points, out, count_out, stat

    def view(self, pose: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """the map in the frame of pose [B,4,4] f64 -> (dst [B,capacity,3] f32 with NaN rows past the count, count [B] i32): the
        ``dst`` and ``count_d`` of ``odometry.register``"""
        pose = self._pose("LocalMap.view", pose)
        dst = torch.empty(self.B, self.capacity, 3, dtype=torch.float32, device=self.dev)
        call("df_map_view", ptr(self.points), ptr(self.count), ptr(pose), self.B, self.capacity, ptr(dst), stream())
        return dst, self.count
