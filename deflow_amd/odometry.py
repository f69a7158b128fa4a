"""Sweep-to-sweep odometry on the GPU: the per-sweep ``pose`` of a raw recording, the last per-sweep input of the self-supervised chain
that nothing in the tree produced (``HDF5Dataset`` reads it for ``pose0`` / ``pose1``, ``voidmap.sweep_frames`` puts every sweep in one
frame with it).

UNPINNED: people with their own recordings are normally sent to an external LiDAR odometry for this.  What runs here is this project's own
definition -- include/deflow_amd.h and DESIGN.md section 6r -- a scan-to-scan, point-to-point ICP with Geman-McClure weights in 6 degrees
of freedom (``residual="point"``, the default) or, with ``residual="plane"``, a point-to-plane ICP against normals of the target that
``normals`` estimates on the GPU: no map by default (``target="map"`` registers every sweep against a voxel-capped local map of the sweeps
so far instead of its predecessor: ``localmap.LocalMap``; ``map_carve=True`` drops the map rows each sweep sees
through before it is inserted: DESIGN.md section 6u; ``map_evict="near"`` makes an overflowing map lose its outermost rows instead of the
end of its sorted order: DESIGN.md section 6v), no loop closure, no motion un-distortion, and nothing
about its accuracy on real sweeps has been measured.  Scene flow
needs only the relative transform of consecutive sweeps (the reference's ``ego_motion``), which is what it estimates; the poses are those
transforms chained.

``register`` is the op (CUDA tensors only: there is no CPU fallback, every iteration is two launches and nothing in it reads a device
value back); ``register_sweeps`` / ``scene_poses`` run it over the consecutive sweeps of a recording, and
``python -m deflow_amd.odometry data_dir=<dir>`` writes ``<scene_id>.pose.npz`` beside every scene, which ``HDF5Dataset`` and the void map
pick up (``pose_source``) when the file has no ``pose``."""
from __future__ import annotations

import functools
import json
import math
import os
import sys
import time
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, ptr, stream
from .args import cloud, flag, integer, labels, nonneg, positive, tensor
from .chamfer import GRID_RANGE, RowGrid

SIDECAR_SUFFIX = ".pose.npz"
POSE_SOURCES = ("auto", "file", "sidecar")
# this project's own choices, unmeasured: gate distances of the levels (kernel = max_dist / 3), iterations per level, the grids' cell
LEVELS = (2.0, 1.0, 0.5)
RESIDUALS = ("point", "plane")
# residual: which default is better on real sweeps is unmeasured, so the point residual stays.  normal_*: choices, not measurements --
# the neighbourhood's radius (<= cell), the fewest rows a normal is fitted to, the largest curvature lambda0 / trace of a valid normal
DEFAULTS: Dict[str, Any] = {"xy_range": GRID_RANGE, "cell": 1.0, "stride": 4, "levels": LEVELS, "iters": 8, "min_inliers": 50,
                            "planar": False, "residual": "point", "normal_radius": 1.0, "normal_min_pts": 5, "normal_max_curv": 0.05}
SCENE_DEFAULTS: Dict[str, Any] = {"min_range": 3.0, "max_range": 51.2}
TARGETS = ("scan", "map")
# target: what a sweep is registered against -- its predecessor ("scan", the default: which is better on real sweeps is unmeasured) or a
# local map of the sweeps so far (localmap.LocalMap).  map_*: this project's own choices, unmeasured -- the map's
# voxel, the rows a voxel keeps, the rows the map holds
MAP_DEFAULTS: Dict[str, Any] = {"target": "scan", "map_voxel": 0.5, "map_max_per_voxel": 4, "map_capacity": 524288}
# map_carve: before a sweep is inserted, drop the map rows it sees through (localmap.LocalMap.carve; UNPINNED, off
# by default).  Choices, not measurements: the depth cube's bins per face edge, the window of bins about a row's own, the absolute and the
# relative margin by which a return must lie behind a row.  The test's ``near`` is the scene's min_range.  (Beside MAP_DEFAULTS, not in
# it: the keys of 6t stay what they were.)
MAP_CARVE_DEFAULTS: Dict[str, Any] = {"map_carve": False, "map_carve_res": 256, "map_carve_halo": 1, "map_carve_margin": 0.5,
                                      "map_carve_rel": 0.02}
# map_evict: which rows the map loses when an update overflows map_capacity (localmap.LocalMap(evict=...); UNPINNED).
# "order": the end of the sorted order, what it always was; "near": the outermost rings of the window, so that what goes is what is
# farthest from the sensor.  Whether "near" helps on real sweeps is unmeasured.  (A dict of its own, for the reason given above.)
MAP_EVICT_DEFAULTS: Dict[str, Any] = {"map_evict": "order"}
MAP_EVICTS = ("order", "near")


_tensor = functools.partial(tensor, "register", other="src")


def schedule(levels, iters) -> List[Tuple[float, int]]:
    """levels: gate distances (each then runs ``iters`` iterations) or (max_dist, iters) pairs -> [(max_dist, iters), ...]"""
    out = []
    try:
        for lv in levels:
            d, n = (lv if isinstance(lv, (tuple, list)) else (lv, iters))
            d, n = float(d), int(n)
            if not (math.isfinite(d) and d > 0) or not 0 <= n <= 1024:
                raise ValueError
            out.append((d, n))
    except (TypeError, ValueError):
        raise ValueError(f"register: levels must be positive finite distances or (distance, iterations 0..1024) pairs, got {levels!r} "
                         f"with iters={iters!r}") from None
    if not out:
        raise ValueError("register: levels must name at least one level")
    return out


def _normal_params(fn: str, names: Tuple[str, str, str], radius, min_pts, max_curv) -> Tuple[float, int, float]:
    """df_normals' limits on (radius, min_pts, max_curv), under the names ``fn`` knows them by (the radius is held against the grid's
    cell by _radius_fits, once the grid is known)"""
    kr, km, kc = names
    p = {kr: radius, km: min_pts, kc: max_curv}
    positive(fn, p, kr)
    integer(fn, p, km, 3, 2 ** 31 - 1)
    positive(fn, p, kc)
    if p[kc] > 1.0 / 3.0:
        raise ValueError(f"{fn}: {kc} must lie in (0, 1/3], got {p[kc]!r}")
    return p[kr], p[km], p[kc]


def _radius_fits(fn: str, name: str, radius: float, cell: float) -> None:
    if radius > cell:
        raise ValueError(f"{fn}: {name} = {radius!r} is larger than the grid's cell = {cell!r}: the neighbours of a row are looked for in "
                         "the cells within one cell of its position only")


def _filed_normals(grid: RowGrid, filed, N: int, radius: float, min_pts: int, max_curv: float, want_m: bool):
    """df_normals on a cloud that ``grid.file`` filed -> (normals [B,N,4] f32, m [B,N] i32 or None)"""
    out = torch.empty(grid.B, N, 4, dtype=torch.float32, device=grid.dev)
    m = torch.empty(grid.B, N, dtype=torch.int32, device=grid.dev) if want_m else None
    call("df_normals", ptr(filed[0]), ptr(filed[1]), grid.minx, grid.miny, grid.cell, grid.G, grid.B, N, radius, min_pts, max_curv,
         ptr(out), ptr(m), stream())
    return out, m


def normals(points: torch.Tensor, count: torch.Tensor, *, mask: Optional[torch.Tensor] = None, xy_range: Sequence[float], cell: float,
            radius: float, min_pts: int, max_curv: float):
    """Surface normals of points [B,N,3] f32 with count [B] i32 valid leading rows and an optional integer / bool mask [B,N] (rows take
    part as in ``register``): for every row the plane through the rows within ``radius`` (<= cell) of it, itself included.
    -> (n [B,N,3] f32, curv [B,N] f32, m [B,N] i32): the unit normal pointing towards the frame's origin, lambda0 / (lambda0 + lambda1 +
    lambda2) of the neighbourhood's covariance and the number of neighbours.  A row is VALID with m >= min_pts, a covariance that is not 0
    and curv <= max_curv; every other row has n = 0, curv = -1 (and m = 0 where the row does not take part).  CUDA tensors only: there is
    no CPU fallback.  Two launches after the grid build, no host synchronisation (include/deflow_amd.h)."""
    B, N = cloud("normals", "points", points, rows_limit=1)
    dev = points.device
    tensor("normals", "count", count, torch.int32, (B,), dev, other="points")
    radius, min_pts, max_curv = _normal_params("normals", ("radius", "min_pts", "max_curv"), radius, min_pts, max_curv)
    try:
        grid = RowGrid(B, xy_range, cell, dev)
    except (TypeError, ValueError):
        raise ValueError(f"normals: bad grid (xy_range {tuple(xy_range)}, cell {cell})") from None
    _radius_fits("normals", "radius", radius, grid.cell)
    lab = labels("normals", "mask", mask, (B, N), f"must be an integer or bool CUDA tensor of shape {(B, N)} on {dev}", dev)
    out, m = _filed_normals(grid, grid.file(points.detach().contiguous(), count.contiguous(), lab), N, radius, min_pts, max_curv, True)
    return out[..., :3], out[..., 3], m


def register(src: torch.Tensor, count_s: torch.Tensor, dst: torch.Tensor, count_d: torch.Tensor, *, init: Optional[torch.Tensor] = None,
             mask_s: Optional[torch.Tensor] = None, mask_d: Optional[torch.Tensor] = None, xy_range: Sequence[float] = DEFAULTS["xy_range"],
             cell: float = DEFAULTS["cell"], stride: int = DEFAULTS["stride"], levels=DEFAULTS["levels"], iters: int = DEFAULTS["iters"],
             min_inliers: int = DEFAULTS["min_inliers"], planar: bool = DEFAULTS["planar"], rows: bool = False,
             residual: str = DEFAULTS["residual"], normal_radius: float = DEFAULTS["normal_radius"],
             normal_min_pts: int = DEFAULTS["normal_min_pts"], normal_max_curv: float = DEFAULTS["normal_max_curv"]):
    """src [B,Ns,3] f32 with count_s [B] i32 valid leading rows, dst [B,Nd,3] with count_d [B]; optional integer / bool masks [B,Ns], [B,Nd]
    (only rows with mask > 0 take part; non-finite rows never do).  init: [B,4,4] floating CUDA tensor, identity when None.
    -> (T [B,4,4] float64 with dst ~ R src + t, info).  info: ``status`` [B] i32 of the last iteration (0 updated, 2 fewer than min_inliers
    inliers, 3 singular: T was left alone in that iteration), ``log`` [B, total iterations + 1, 4] f32 = (inliers, weighted mean squared
    residual, |omega|, |v|) of every iteration and, last, of the final T; rows=True adds the final per-row ``q`` [B,Ns,3], ``idx`` [B,Ns],
    ``d2`` [B,Ns], ``w`` [B,Ns].  levels: gate distances, each run for ``iters`` iterations with kernel = distance / 3,
    or (distance, iterations) pairs.  A fixed number of launches, no early stop, no host synchronisation.
    residual="plane": the residual of a row is its distance to the plane of its nearest target row, n . (q - d), with the target's normals
    estimated once (``normals`` with normal_radius <= cell, normal_min_pts, normal_max_curv); a row whose partner has no valid normal is
    no inlier.  rows=True then adds ``e`` [B,Ns], and info has ``normals_valid`` [B] i64, the number of valid target normals.  The
    normal_* parameters are not looked at with residual="point"."""
    if not isinstance(src, torch.Tensor) or not isinstance(dst, torch.Tensor) or src.dim() != 3 or dst.dim() != 3 or src.shape[2] != 3 or \
            dst.shape[2] != 3 or src.shape[0] != dst.shape[0]:
        raise ValueError("register: src [B,Ns,3] and dst [B,Nd,3] expected, got "
                         f"{tuple(getattr(src, 'shape', ()))} and {tuple(getattr(dst, 'shape', ()))}")
    B, Ns, _ = src.shape
    Nd = dst.shape[1]
    if B == 0 or Ns == 0 or Nd == 0:
        raise ValueError("register: empty batch or zero padded rows")
    _tensor("src", src, torch.float32, (B, Ns, 3))
    dev = src.device
    _tensor("dst", dst, torch.float32, (B, Nd, 3), dev)
    _tensor("count_s", count_s, torch.int32, (B,), dev)
    _tensor("count_d", count_d, torch.int32, (B,), dev)
    if int(stride) != stride or not 1 <= int(stride) <= 1024:
        raise ValueError(f"register: stride must be an integer in 1..1024, got {stride!r}")
    if int(min_inliers) != min_inliers or int(min_inliers) < 0:
        raise ValueError(f"register: min_inliers must be an integer >= 0, got {min_inliers!r}")
    plan = schedule(levels, iters)
    if residual not in RESIDUALS:
        raise ValueError(f"register: residual must be 'point' or 'plane', got {residual!r}")
    plane = residual == "plane"
    if plane:
        normal_radius, normal_min_pts, normal_max_curv = _normal_params(
            "register", ("normal_radius", "normal_min_pts", "normal_max_curv"), normal_radius, normal_min_pts, normal_max_curv)
    try:
        grid = RowGrid(B, xy_range, cell, dev)
    except (TypeError, ValueError):
        raise ValueError(f"register: bad grid (xy_range {tuple(xy_range)}, cell {cell})") from None
    if plane:
        _radius_fits("register", "normal_radius", normal_radius, grid.cell)
    if init is None:
        T = torch.eye(4, dtype=torch.float64, device=dev).repeat(B, 1, 1)
    else:
        if not isinstance(init, torch.Tensor) or not init.is_cuda or init.device != dev or tuple(init.shape) != (B, 4, 4) or \
                not init.dtype.is_floating_point:
            raise ValueError(f"register: init must be a floating CUDA tensor of shape {(B, 4, 4)} on {dev}")
        T = init.detach().to(torch.float64).contiguous().clone()
    src, dst = src.detach().contiguous(), dst.detach().contiguous()
    count_s, count_d = count_s.contiguous(), count_d.contiguous()
    ms = labels("register", "mask_s", mask_s, (B, Ns), f"must be an integer or bool CUDA tensor of shape {(B, Ns)} on {dev}", dev)
    md = labels("register", "mask_d", mask_d, (B, Nd), f"must be an integer or bool CUDA tensor of shape {(B, Nd)} on {dev}", dev)

    (s_rng, s_rows), (d_rng, d_rows) = grid.file(src, count_s, ms), grid.file(dst, count_d, md)
    minx, miny, G = grid.minx, grid.miny, grid.G
    nblk = (Ns + 255) // 256
    slab = call("df_reg_ws_bytes", B, Ns)
    if slab <= 0:
        raise ValueError(f"register: B = {B} samples of Ns = {Ns} rows are beyond the entries' limits (B <= 65535, B Ns < 2^30)")
    partial = torch.empty(slab // 8, dtype=torch.float64, device=dev)
    total = sum(n for _, n in plan)
    log = torch.zeros(total + 1, B, 4, dtype=torch.float32, device=dev)
    status = torch.full((B,), 2, dtype=torch.int32, device=dev)      # (no iteration at all: nothing was updated)
    s = stream()

    info: Dict[str, torch.Tensor] = {"status": status}
    if plane:                                                          # the target is fixed over all iterations: its normals, once
        nrm, _ = _filed_normals(grid, (d_rng, d_rows), Nd, normal_radius, normal_min_pts, normal_max_curv, False)
        info["normals_valid"] = (nrm[..., 3] >= 0).sum(dim=1)
    nouts = 5 if plane else 4

    def accumulate(max_dist, outs=(None,) * nouts):
        if plane:
            call("df_reg_accumulate_plane", ptr(s_rng), ptr(s_rows), G, ptr(d_rng), ptr(d_rows), ptr(nrm), minx, miny, float(cell), G, B,
                 Ns, Nd, int(stride), ptr(T), float(max_dist) ** 2, (float(max_dist) / 3.0) ** 2, ptr(partial), *(ptr(o) for o in outs), s)
            return
        call("df_reg_accumulate", ptr(s_rng), ptr(s_rows), G, ptr(d_rng), ptr(d_rows), minx, miny, float(cell), G, B, Ns, int(stride), ptr(T),
             float(max_dist) ** 2, (float(max_dist) / 3.0) ** 2, ptr(partial), *(ptr(o) for o in outs), s)

    it = 0
    for max_dist, n in plan:
        for _ in range(n):
            accumulate(max_dist)
            call("df_reg_solve", ptr(partial), B, nblk, int(min_inliers), int(bool(planar)), ptr(T), ptr(log[it]), ptr(status), s)
            it += 1
    outs = (None,) * nouts
    if rows:
        outs = (torch.empty(B, Ns, 3, dtype=torch.float32, device=dev), torch.empty(B, Ns, dtype=torch.int32, device=dev),
                torch.empty(B, Ns, dtype=torch.float32, device=dev), torch.empty(B, Ns, dtype=torch.float32, device=dev))
        if plane:
            outs += (torch.empty(B, Ns, dtype=torch.float32, device=dev),)
        info.update(zip(("q", "idx", "d2", "w", "e"), outs))
    accumulate(plan[-1][0], outs)                                      # the final T's rows and log: nothing is solved
    call("df_reg_solve", ptr(partial), B, nblk, int(min_inliers), int(bool(planar)), None, ptr(log[total]), None, s)
    info["log"] = log.permute(1, 0, 2)
    return T, info


# ---- recordings -------------------------------------------------------------------------------------------------------------------------
def chain_poses(rel: Sequence[np.ndarray]) -> List[np.ndarray]:
    """rel[k] maps sweep k into sweep k + 1's frame -> the poses: pose_0 = I, pose_{k+1} = pose_k @ inv(rel[k]), float64"""
    poses = [np.eye(4, dtype=np.float64)]
    for T in rel:
        poses.append(poses[-1] @ np.linalg.inv(np.asarray(T, dtype=np.float64)))
    return poses


def register_sweeps(lidars: Sequence[np.ndarray], ground: Optional[Sequence[Optional[np.ndarray]]] = None, *, init: str = "previous",
                    min_range: float = SCENE_DEFAULTS["min_range"], max_range: float = SCENE_DEFAULTS["max_range"], device="cuda",
                    report: Optional[dict] = None, target: str = MAP_DEFAULTS["target"], map_voxel: float = MAP_DEFAULTS["map_voxel"],
                    map_max_per_voxel: int = MAP_DEFAULTS["map_max_per_voxel"], map_capacity: int = MAP_DEFAULTS["map_capacity"],
                    map_carve: bool = MAP_CARVE_DEFAULTS["map_carve"], map_carve_res: int = MAP_CARVE_DEFAULTS["map_carve_res"],
                    map_carve_halo: int = MAP_CARVE_DEFAULTS["map_carve_halo"],
                    map_carve_margin: float = MAP_CARVE_DEFAULTS["map_carve_margin"],
                    map_carve_rel: float = MAP_CARVE_DEFAULTS["map_carve_rel"],
                    map_evict: str = MAP_EVICT_DEFAULTS["map_evict"], **params) -> List[np.ndarray]:
    """Relative transforms of consecutive sweeps given as arrays [N_i, >= 3], each in its own vehicle frame, in time order:
    -> rel[k] float64 [4,4] mapping sweep k into sweep k + 1's frame, one B = 1 ``register`` per pair.  target="scan": sweep k + 1 is the
    target of sweep k.  target="map": sweep k + 1 is registered against a local map of the sweeps 0 .. k seen from pose_k (at most
    map_max_per_voxel rows per voxel of map_voxel metres, map_capacity rows, a window of max_range about the sensor; DESIGN.md section
    6t), the map is kept on the device and a failed sweep inserts nothing; rel[k] is then the inverse of that registration's result.  ground: per sweep None or a 0 / 1
    map_carve=True (target="map" only; UNPINNED): between the pose of sweep k + 1 and its insertion the map rows
    that the sweep sees through are dropped -- a depth cube of map_carve_res bins per face edge built on the sweep's participating rows,
    a map row flagged when a return lies more than map_carve_margin + map_carve_rel x its depth behind it in the (2 map_carve_halo + 1)^2
    bins about its own, rows nearer than min_range left alone; a failed sweep carves nothing.
    map_evict="near" (target="map" only; UNPINNED): an update that overflows map_capacity loses the rows of the
    outermost rings of the window about the sensor instead of the end of the sorted order ("order", the default).  ground: per sweep None or a 0 / 1
    array [N_i]; ground rows do not take part.  Rows take part only at a horizontal distance from the frame's origin in
    [min_range, max_range].  The first pair starts from identity; init="previous": each later pair from the previous pair's result
    (constant velocity), "identity": every pair from identity.  A pair whose status is not 0 keeps its initial transform.
    report: a dict that receives the parameters, the failed pairs and the final inliers / residual of every pair (target="map": also
    map_count and map_overflow after every sweep, with map_carve map_carved, the rows every later sweep dropped, and with
    map_evict="near" map_cut, the pair (R, budget) of every sweep's update)."""
    if init not in ("previous", "identity"):
        raise ValueError(f"register_sweeps: init must be 'previous' or 'identity', got {init!r}")
    if target not in TARGETS:
        raise ValueError(f"register_sweeps: target must be 'scan' or 'map', got {target!r}")
    mp = {"map_voxel": map_voxel, "map_max_per_voxel": map_max_per_voxel, "map_capacity": map_capacity}
    positive("register_sweeps", mp, "map_voxel")
    integer("register_sweeps", mp, "map_max_per_voxel", 1, 2 ** 31 - 1)
    integer("register_sweeps", mp, "map_capacity", 1, 2 ** 30 - 1)
    cp = {"map_carve": map_carve, "map_carve_res": map_carve_res, "map_carve_halo": map_carve_halo, "map_carve_margin": map_carve_margin,
          "map_carve_rel": map_carve_rel}
    flag("register_sweeps", cp, "map_carve")
    if cp["map_carve"]:
        if target != "map":
            raise ValueError("register_sweeps: map_carve=True needs target='map': there is no map to carve with target='scan'")
        from .visibility import HALO_MAX, RES_MAX
        integer("register_sweeps", cp, "map_carve_res", 2, RES_MAX)
        if cp["map_carve_res"] % 2:
            raise ValueError(f"register_sweeps: map_carve_res must be even, got {map_carve_res!r}")
        integer("register_sweeps", cp, "map_carve_halo", 0, HALO_MAX)
        nonneg("register_sweeps", cp, "map_carve_margin")
        nonneg("register_sweeps", cp, "map_carve_rel")
    if map_evict not in MAP_EVICTS:
        raise ValueError(f"register_sweeps: map_evict must be 'order' or 'near', got {map_evict!r}")
    if map_evict == "near" and target != "map":
        raise ValueError("register_sweeps: map_evict='near' needs target='map': there is no map to evict from with target='scan'")
    near = map_evict == "near"
    if not (0 <= float(min_range) < float(max_range)):
        raise ValueError(f"register_sweeps: 0 <= min_range < max_range expected, got {min_range}, {max_range}")
    unknown = sorted(set(params) - set(DEFAULTS))
    if unknown:
        raise TypeError(f"register_sweeps: unknown parameters {unknown}")
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError("register_sweeps: device must be a CUDA device (deflow_amd has no CPU fallback)")
    clouds = []
    for k, lidar in enumerate(lidars):
        p = np.ascontiguousarray(np.asarray(lidar)[:, :3], dtype=np.float32)
        with np.errstate(invalid="ignore"):
            rng = np.hypot(p[:, 0].astype(np.float64), p[:, 1].astype(np.float64))
            keep = (rng >= min_range) & (rng <= max_range)
        if ground is not None and ground[k] is not None:
            g = np.asarray(ground[k]).reshape(-1)
            if g.shape[0] != p.shape[0]:
                raise ValueError(f"register_sweeps: {g.shape[0]} ground flags for sweep {k}, which has {p.shape[0]} rows")
            keep &= g == 0
        if p.shape[0] == 0:
            p, keep = np.full((1, 3), np.nan, dtype=np.float32), np.zeros(1, dtype=bool)
        clouds.append((torch.from_numpy(p).to(device)[None], torch.full((1,), p.shape[0], dtype=torch.int32, device=device),
                       torch.from_numpy(keep.astype(np.int32)).to(device)[None]))
    start = torch.eye(4, dtype=torch.float64, device=device)[None]
    Ts, stats, fill, carved, cuts = [], [], [], [], []
    if target == "map" and clouds:
        from .localmap import LocalMap
        lmap = LocalMap(1, mp["map_capacity"], voxel=mp["map_voxel"], max_per_voxel=mp["map_max_per_voxel"], max_range=float(max_range),
                        device=device, **({"evict": "near"} if near else {}))
        pose = start.clone()
        lmap.insert(*clouds[0][:2], pose, mask=clouds[0][2])
        fill.append(torch.cat((lmap.count, lmap.stat[0, 3:])))
        if near:
            cuts.append(lmap.cut)
        for ps, cs, ms in clouds[1:]:
            dst, cd = lmap.view(pose)
            T, info = register(ps, cs, dst, cd, init=start, mask_s=ms, **params)
            ok = (info["status"] == 0).reshape(1, 1, 1)
            T = torch.where(ok, T, start)                              # a failed sweep keeps its initial transform ...
            pose = pose @ T
            if cp["map_carve"]:                                        # ... carves nothing ...
                lmap.carve(ps, cs, pose, mask=ms, gate=info["status"], res=cp["map_carve_res"], halo=cp["map_carve_halo"],
                           margin=cp["map_carve_margin"], rel=cp["map_carve_rel"], near=float(min_range))
                carved.append(lmap.carve_stat[0, 1:])
            lmap.insert(ps, cs, pose, mask=ms, gate=info["status"])    # ... and inserts nothing
            Ts.append(T)
            stats.append(torch.cat((info["status"].to(torch.float32), info["log"][0, -1, :2])))
            fill.append(torch.cat((lmap.count, lmap.stat[0, 3:])))
            if near:
                cuts.append(lmap.cut)
            if init == "previous":
                start = T
    for k in range(len(clouds) - 1 if target == "scan" else 0):
        (ps, cs, ms), (pd, cd, md) = clouds[k], clouds[k + 1]
        T, info = register(ps, cs, pd, cd, init=start, mask_s=ms, mask_d=md, **params)
        ok = (info["status"] == 0).reshape(1, 1, 1)
        T = torch.where(ok, T, start)                                  # a failed pair keeps its initial transform
        Ts.append(T)
        stats.append(torch.cat((info["status"].to(torch.float32), info["log"][0, -1, :2])))
        if init == "previous":
            start = T
    if not Ts:
        rel, st = [], np.zeros((0, 3), dtype=np.float32)
    else:
        rel = list(torch.cat(Ts).cpu().numpy())                        # the one read-back, after every pair was queued
        st = torch.stack(stats).cpu().numpy()
        if target == "map":                                            # the registration maps sweep k + 1 into sweep k's frame
            rel = [np.linalg.inv(T) for T in rel]
    if report is not None:
        if target == "map":
            mf = torch.stack(fill).cpu().numpy() if fill else np.zeros((0, 2), dtype=np.int32)
            report.update(map_count=[int(c) for c in mf[:, 0]], map_overflow=[int(c) for c in mf[:, 1]])
            if cp["map_carve"]:
                report.update(map_carved=[int(c) for c in torch.cat(carved).cpu().numpy()] if carved else [])
            if near:
                report.update(map_cut=[(int(c[0]), int(c[1])) for c in torch.cat(cuts).cpu().numpy()] if cuts else [])
        report.update(params={**DEFAULTS, **params, "min_range": float(min_range), "max_range": float(max_range), "init": init,
                              "target": target, **mp, **cp, "map_evict": map_evict},
                      failed=[{"pair": int(k), "status": int(s[0])} for k, s in enumerate(st) if int(s[0]) != 0],
                      inliers=[float(s[1]) for s in st], residual=[float(s[2]) for s in st])
    return rel


def scene_poses(h5_path: str, *, ground_source: str = "auto", init: str = "previous", device="cuda", report: Optional[dict] = None,
                **params) -> Dict[str, np.ndarray]:
    """Poses of every sweep of a preprocessed scene file, sweeps taken in timestamp order: {timestamp: float64 [4,4]}, the first sweep's
    frame as the world (pose_0 = I, pose_{k+1} = pose_k @ inv(T_k)).  ground_source="auto": ground rows are left out where the group holds
    a ``ground_mask`` or ``<scene_id>.ground.npz`` (python -m deflow_amd.ground) has the sweep; "none": every row is used."""
    from .ground import SIDECAR_SUFFIX as GROUND_SUFFIX
    from .h5scene import H5File
    if ground_source not in ("auto", "none"):
        raise ValueError(f"scene_poses: ground_source must be 'auto' or 'none', got {ground_source!r}")
    side = None
    gpath = h5_path[:-3] + GROUND_SUFFIX if h5_path.endswith(".h5") else None
    if ground_source == "auto" and gpath and os.path.exists(gpath):
        with np.load(gpath, allow_pickle=False) as z:
            side = {k: z[k] for k in z.files if k != "meta"}
    with H5File(h5_path) as f:
        keys = sorted(f.keys(), key=int)
        lidars = [f[k]["lidar"].read() for k in keys]
        ground: List[Optional[np.ndarray]] = [None] * len(keys)
        if ground_source == "auto":
            for i, k in enumerate(keys):
                if "ground_mask" in f[k]:
                    ground[i] = f[k]["ground_mask"].read()
                elif side is not None and k in side:
                    ground[i] = side[k]
    rel = register_sweeps(lidars, ground, init=init, device=device, report=report, **params)
    if report is not None:
        report["params"]["ground_source"] = ground_source
        report["ground_masks"] = sum(g is not None for g in ground)
    return dict(zip(keys, chain_poses(rel)))


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    return v


def write_sidecar(path: str, poses: Dict[str, np.ndarray], meta: Dict[str, Any]) -> None:
    """<scene_id>.pose.npz: one float64 [4,4] per timestamp and the parameters as a JSON string under ``meta``; written atomically"""
    tmp = path + ".tmp.npz"
    np.savez(tmp, meta=np.array(json.dumps({k: _plain(v) for k, v in meta.items()}, sort_keys=True)),
             **{str(k): np.asarray(v, dtype=np.float64).reshape(4, 4) for k, v in poses.items()})
    os.replace(tmp, path)


def read_sidecar(path: str) -> Dict[str, np.ndarray]:
    """the per-timestamp poses of a sidecar (without ``meta``)"""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files if k != "meta"}


# ---- the readers' side: where a sweep's pose comes from ---------------------------------------------------------------------------------
def check_pose_source(pose_source: str, pose_sidecar: Optional[str]) -> None:
    if pose_source not in POSE_SOURCES:
        raise ValueError(f"pose_source must be 'auto', 'file' or 'sidecar', got {pose_source!r}")
    if pose_source == "sidecar" and not pose_sidecar:
        raise ValueError("pose_source='sidecar' needs a pose_sidecar suffix")


def load_pose_sidecar(directory: str, scene_id: str, pose_sidecar: Optional[str] = SIDECAR_SUFFIX) -> Optional[Dict[str, np.ndarray]]:
    """the poses of ``<directory>/<scene_id><pose_sidecar>``, None when there is no such file (or no suffix)"""
    if not pose_sidecar:
        return None
    path = os.path.join(directory, f"{scene_id}{pose_sidecar}")
    return read_sidecar(path) if os.path.exists(path) else None


def sweep_pose(group, side: Optional[Dict[str, np.ndarray]], *, scene_id: str, ts: str, pose_source: str = "auto",
               pose_sidecar: Optional[str] = SIDECAR_SUFFIX, directory: str = ".") -> np.ndarray:
    """The pose of one sweep, by ``pose_source``: "auto": the group's own ``pose`` dataset wins, a group without one takes the sidecar's;
    "file": the dataset only; "sidecar": the sidecar (``side``: what load_pose_sidecar returned) only.  A sidecar that is missing or lacks
    the timestamp is a ValueError naming the command that writes it."""
    if pose_source == "file" or (pose_source == "auto" and "pose" in group):
        return group["pose"].read()
    if side is None or ts not in side:
        what = "does not exist" if side is None else f"has no entry for sweep {ts}"
        raise ValueError(f"{scene_id}: no pose for sweep {ts} (pose_source={pose_source!r}): {scene_id}{pose_sidecar} {what}; write it with  "
                         f"python -m deflow_amd.odometry data_dir={directory}")
    pose = np.asarray(side[ts])
    if pose.shape != (4, 4):
        raise ValueError(f"{scene_id}{pose_sidecar}: pose of shape {pose.shape} for sweep {ts}, [4,4] expected")
    return pose


# ---- command line -----------------------------------------------------------------------------------------------------------------------
CLI_DEFAULTS: Dict[str, Any] = {"data_dir": None, "scenes": None, "overwrite": False, "ground_source": "auto", "init": "previous",
                                **SCENE_DEFAULTS, **MAP_DEFAULTS, **MAP_CARVE_DEFAULTS, **MAP_EVICT_DEFAULTS,
                                **{k: (list(v) if isinstance(v, tuple) else v) for k, v in DEFAULTS.items()}}
USAGE = ("usage: python -m deflow_amd.odometry data_dir=<dir> [scenes=a,b] [overwrite=false] [stride=4] [levels=2,1,0.5] [iters=8] "
         "[planar=false] [min_inliers=50] [residual=point|plane] [normal_radius=1] [normal_min_pts=5] [normal_max_curv=0.05] "
         "[ground_source=auto|none] [init=previous|identity] [min_range=3] [max_range=51.2] [cell=1] "
         "[xy_range=-51.2,-51.2,51.2,51.2] [target=scan|map] [map_voxel=0.5] [map_max_per_voxel=4] [map_capacity=524288] "
         "[map_carve=false] [map_carve_res=256] [map_carve_halo=1] [map_carve_margin=0.5] [map_carve_rel=0.02] "
         "[map_evict=order|near]")


def _bool(v: str) -> bool:
    if v.lower() not in ("true", "false", "1", "0"):
        raise ValueError(v)
    return v.lower() in ("true", "1")


def parse_args(argv: List[str]) -> Dict[str, Any]:
    """key=value arguments in the style of deflow_amd.train"""
    cfg = dict(CLI_DEFAULTS)
    for a in argv:
        if "=" not in a:
            raise SystemExit(f"expected key=value, got {a!r}")
        k, v = a.split("=", 1)
        k = k.lstrip("+")
        if k not in CLI_DEFAULTS:
            raise SystemExit(f"unknown key {k!r}; known: {', '.join(sorted(CLI_DEFAULTS))}")
        try:
            if k == "data_dir":
                cfg[k] = v
            elif k == "scenes":
                cfg[k] = [s for s in v.split(",") if s]
            elif k in ("overwrite", "planar", "map_carve"):
                cfg[k] = _bool(v)
            elif k == "ground_source":
                if v not in ("auto", "none"):
                    raise ValueError(v)
                cfg[k] = v
            elif k == "residual":
                if v not in RESIDUALS:
                    raise ValueError(v)
                cfg[k] = v
            elif k == "target":
                if v not in TARGETS:
                    raise ValueError(v)
                cfg[k] = v
            elif k == "map_evict":
                if v not in MAP_EVICTS:
                    raise ValueError(v)
                cfg[k] = v
            elif k == "init":
                if v not in ("previous", "identity"):
                    raise ValueError(v)
                cfg[k] = v
            elif k in ("levels", "xy_range"):
                cfg[k] = [float(x) for x in v.strip("[]()").split(",")]
                if (k == "xy_range" and len(cfg[k]) != 4) or not cfg[k] or not all(math.isfinite(x) for x in cfg[k]) or \
                        (k == "levels" and not all(x > 0 for x in cfg[k])):
                    raise ValueError(v)
            elif k in ("stride", "iters", "min_inliers", "normal_min_pts", "map_max_per_voxel", "map_capacity", "map_carve_res",
                       "map_carve_halo"):
                cfg[k] = int(v)
                lo, hi = {"stride": (1, 1024), "iters": (0, 1024), "min_inliers": (0, 2 ** 31 - 1), "normal_min_pts": (3, 2 ** 31 - 1),
                          "map_max_per_voxel": (1, 2 ** 31 - 1), "map_capacity": (1, 2 ** 30 - 1), "map_carve_res": (2, 2048),
                          "map_carve_halo": (0, 4)}[k]
                if not lo <= cfg[k] <= hi or (k == "map_carve_res" and cfg[k] % 2):
                    raise ValueError(v)
            else:
                cfg[k] = float(v)
                if not math.isfinite(cfg[k]) or cfg[k] < 0 or (k in ("cell", "normal_radius", "normal_max_curv", "map_voxel") and cfg[k] == 0) or \
                        (k == "normal_max_curv" and cfg[k] > 1.0 / 3.0):
                    raise ValueError(v)
        except ValueError:
            raise SystemExit(f"bad value for {k}: {v!r}")
    if not cfg["data_dir"]:
        raise SystemExit(USAGE)
    if not cfg["min_range"] < cfg["max_range"]:
        raise SystemExit(f"bad value for min_range / max_range: {cfg['min_range']} .. {cfg['max_range']}")
    if cfg["map_carve"] and cfg["target"] != "map":
        raise SystemExit("bad value for map_carve / target: map_carve=true needs target=map")
    if cfg["map_evict"] == "near" and cfg["target"] != "map":
        raise SystemExit("bad value for map_evict / target: map_evict=near needs target=map")
    if cfg["residual"] == "plane" and cfg["normal_radius"] > cfg["cell"]:
        raise SystemExit(f"bad value for normal_radius / cell: the radius {cfg['normal_radius']} is larger than the cell {cfg['cell']}")
    return cfg


def main(argv=None) -> int:
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    assert torch.cuda.is_available(), "the odometry runs on the HIP engine only"
    d = cfg["data_dir"]
    scenes = cfg["scenes"] or sorted(n[:-3] for n in os.listdir(d) if n.endswith(".h5"))
    params = {k: (tuple(cfg[k]) if isinstance(cfg[k], list) else cfg[k]) for k in (*DEFAULTS, *SCENE_DEFAULTS, *MAP_DEFAULTS, *MAP_CARVE_DEFAULTS, *MAP_EVICT_DEFAULTS)}
    for sid in scenes:
        out = os.path.join(d, sid + SIDECAR_SUFFIX)
        if os.path.exists(out) and not cfg["overwrite"]:
            print(json.dumps({"scene": sid, "skipped": "sidecar exists (overwrite=true replaces it)"}), flush=True)
            continue
        rep: Dict[str, Any] = {}
        t0 = time.perf_counter()
        poses = scene_poses(os.path.join(d, sid + ".h5"), ground_source=cfg["ground_source"], init=cfg["init"], report=rep, **params)
        sections = ["6r"] + (["6t"] if cfg["target"] == "map" else []) + (["6u"] if cfg["map_carve"] else []) + \
            (["6v"] if cfg["map_evict"] == "near" else [])
        write_sidecar(out, poses, {**rep["params"], "failed": rep["failed"], "definition": f"DESIGN.md {', '.join(sections)} (UNPINNED)"})
        ps = list(poses.values())
        path = sum(float(np.linalg.norm(b[:3, 3] - a[:3, 3])) for a, b in zip(ps, ps[1:]))
        n = max(len(rep["inliers"]), 1)
        print(json.dumps({"scene": sid, "sweeps": len(poses), "failed_pairs": rep["failed"],
                          "mean_inliers": round(sum(rep["inliers"]) / n, 3), "mean_residual": round(sum(rep["residual"]) / n, 9),
                          "path_length": round(path, 6), "seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
