"""A void map on the GPU: per-point dynamic flags from ray casting, the one input the online cluster labels (``cluster.py``,
``Trainer(cluster_labels=...)``) could not get from plain preprocessed scene files.

UNPINNED: upstream writes the ``dufo_label`` dataset offline on the CPU with DUFOMap ([REF assets/slurm/dufolabel_sbatch.py] -> process.py;
Duberg et al., RA-L 2024; the code is in the absent submodule).  What runs here is a DUFOMap-style void map with every choice fixed -- the
definition is in include/deflow_amd.h and DESIGN.md section 6c -- so the map and the flags are a pure integer function of the input and
bit-reproducible.  Parity with upstream's flags is not claimed and was not measured.  Space that some sweep has seen through is void; a
return that lies in void space is dynamic.

``VoidMap`` is the op (CUDA tensors only: there is no CPU fallback, and nothing in it reads a device value back); ``label_scene`` labels a
scene file with it, and ``python -m deflow_amd.voidmap data_dir=<dir>`` writes ``<scene_id>.dufo.npz`` beside every scene, which
``HDF5Dataset`` picks up."""
from __future__ import annotations

import functools
import json
import math
import os
import sys
import time
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import call, ptr, stream
from .args import tensor

SUB = 256                          # sub-voxel units per voxel
SIDECAR_SUFFIX = ".dufo.npz"
MAX_BITS = 1 << 31
# the recalled mount of the AV2 up lidar in the vehicle frame -- UNPINNED, hence an argument everywhere
SENSOR_OFFSET = (1.35, 0.0, 1.64)


def ray_limit(max_range: float, voxel: float) -> int:
    """R of the definition: the Chebyshev range cut in sub-voxel units"""
    return int(round(float(max_range) / float(voxel) * SUB))


_check = functools.partial(tensor, "VoidMap", other="the map is")


class VoidMap:
    """The void map V of ``batch`` samples over one grid, and the free / occupied bits of the last sweep.

    grid_min: three coordinates (rounded to fp32); dims (Gx, Gy, Gz) with Gx % 32 == 0 and Gx * Gy * Gz < 2^31; voxel: the voxel size.
    hit_margin: a ray frees the voxels further than this many voxels (Chebyshev) from its end; erode: radius r in {0, 1, 2} of the erosion
    of a sweep's free space before it joins the map; max_range: rays longer than this (largest axis) are cut there and free all of
    their voxels.  ``integrate`` adds a sweep, ``query`` flags points, ``clear`` empties the map."""

    def __init__(self, batch: int, grid_min: Sequence[float], dims: Sequence[int], voxel: float = 0.1, *, hit_margin: int = 2,
                 erode: int = 1, max_range: float = 80.0, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError("VoidMap: device must be a CUDA device (deflow_amd has no CPU fallback)")
        if device.index is None:               # "cuda" -> the current device, so that tensors' devices compare equal to the map's
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else device
        if int(batch) < 1 or int(batch) > 65535:
            raise ValueError(f"VoidMap: batch must be in 1..65535, got {batch}")
        if len(tuple(grid_min)) != 3 or len(tuple(dims)) != 3:
            raise ValueError("VoidMap: grid_min and dims have three entries each")
        gmin = tuple(float(np.float32(v)) for v in grid_min)
        Gx, Gy, Gz = (int(v) for v in dims)
        if not all(math.isfinite(v) for v in gmin):
            raise ValueError(f"VoidMap: grid_min must be finite, got {grid_min}")
        if min(Gx, Gy, Gz) < 1 or Gx % 32 != 0:
            raise ValueError(f"VoidMap: dims must be positive with Gx a multiple of 32, got {(Gx, Gy, Gz)}")
        if Gx * Gy * Gz >= MAX_BITS:
            raise ValueError(f"VoidMap: the grid {(Gx, Gy, Gz)} has {Gx * Gy * Gz} voxels, the limit is 2^31 - 1: coarsen voxel")
        if not (voxel > 0 and math.isfinite(voxel)):
            raise ValueError(f"VoidMap: voxel must be a positive finite size, got {voxel}")
        if int(hit_margin) != hit_margin or int(hit_margin) < 0:
            raise ValueError(f"VoidMap: hit_margin must be an integer >= 0, got {hit_margin}")
        if erode not in (0, 1, 2):
            raise ValueError(f"VoidMap: erode must be 0, 1 or 2, got {erode}")
        R = ray_limit(max_range, voxel) if math.isfinite(max_range) else 0
        if not 1 <= R <= 1 << 24:
            raise ValueError(f"VoidMap: max_range / voxel * 256 must round into 1..2^24, got max_range {max_range}, voxel {voxel}")
        self.batch, self.grid_min, self.dims, self.voxel = int(batch), gmin, (Gx, Gy, Gz), float(voxel)
        self.hit_margin, self.erode, self.max_range, self.R, self.device = int(hit_margin), int(erode), float(max_range), R, device
        self.k = float(np.float32(SUB / float(voxel)))                 # fp32(256 / voxel), computed on the host
        W = Gx * Gy * Gz // 32
        z = lambda: torch.zeros(self.batch, W, dtype=torch.int32, device=device)
        self._v, self._f, self._o = z(), z(), z()

    # the u32 words (bit = (z * Gy + y) * Gx + x, word bit >> 5, bit bit & 31), [batch, Gx*Gy*Gz/32]
    @property
    def words(self) -> torch.Tensor:
        return self._v.view(torch.uint32)

    @property
    def last_free(self) -> torch.Tensor:
        return self._f.view(torch.uint32)

    @property
    def last_occ(self) -> torch.Tensor:
        return self._o.view(torch.uint32)

    def _grid_args(self):
        return (*self.grid_min, self.k, *self.dims)

    def _points(self, points, count):
        _check("points", points)
        if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] != self.batch or points.shape[1] < 1:
            raise ValueError(f"VoidMap: points [{self.batch},N,3] with N >= 1 expected, got {tuple(points.shape)}")
        B, N, _ = points.shape
        _check("points", points, torch.float32, (B, N, 3), self.device)
        _check("count", count, torch.int32, (B,), self.device)
        return points.detach().contiguous(), count.contiguous(), B, N

    def integrate(self, points: torch.Tensor, count: torch.Tensor, origin: torch.Tensor, status: Optional[torch.Tensor] = None,
                  *, attempts: Optional[torch.Tensor] = None, always_atomic: bool = False) -> None:
        """One sweep per sample: points [B,N,3] f32 with count [B] i32 valid leading rows, origin [B,3] f32 the sensor position.
        Builds the sweep's free and occupied bits (``last_free`` / ``last_occ``) and ORs the eroded free space into the map.
        status: optional i32[1], increased when a ray reaches the walk's bound (never, on a valid map); attempts: optional i64[1],
        increased by the number of free-bit sets the rays asked for; always_atomic drops the test before the atomic (measuring only)."""
        points, count, B, N = self._points(points, count)
        _check("origin", origin, torch.float32, (B, 3), self.device)
        if status is not None:
            _check("status", status, torch.int32, (1,), self.device)
        if attempts is not None:
            _check("attempts", attempts, torch.int64, (1,), self.device)
        s = stream()
        args = (ptr(points), ptr(count), ptr(origin.contiguous()), B, N, *self._grid_args(), self.hit_margin, self.R, ptr(self._f),
                ptr(self._o), ptr(status))
        if attempts is None and not always_atomic:
            call("df_void_cast", *args, s)
        else:                                  # the measuring form of the same kernel
            call("df_void_cast_probe", *args, ptr(attempts), int(bool(always_atomic)), s)
        call("df_void_merge", ptr(self._f), ptr(self._o), ptr(self._v), B, *self.dims, self.erode, s)

    def query(self, points: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
        """-> bool [B,N]: the row takes part, its voxel is inside the grid and void"""
        points, count, B, N = self._points(points, count)
        flags = torch.empty(B, N, dtype=torch.int32, device=points.device)
        call("df_void_query", ptr(points), ptr(count), B, N, *self._grid_args(), ptr(self._v), ptr(flags), stream())
        return flags != 0

    def clear(self) -> None:
        self._v.zero_()
        self._f.zero_()
        self._o.zero_()


# ---- scene labeller ---------------------------------------------------------------------------------------------------------------------
def scene_grid(origins, voxel: float, range_xy: float, z_half: float) -> Tuple[Tuple[float, float, float], Tuple[int, int, int]]:
    """The grid of a scene, a pure function of its sensor origins [K,3]: the bounding box of the origins widened by range_xy in x and y
    and by z_half in z.  grid_min = fp32(lower corner); dims = ceil((upper corner - grid_min) / voxel), at least 1, with Gx rounded up
    to a multiple of 32.  Raises when the grid would hold 2^31 voxels or more."""
    o = np.asarray(origins, dtype=np.float64).reshape(-1, 3)
    if o.shape[0] == 0 or not np.isfinite(o).all():
        raise ValueError("scene_grid: at least one finite origin is needed")
    pad = np.array([range_xy, range_xy, z_half], dtype=np.float64)
    gmin = (o.min(0) - pad).astype(np.float32)
    n = np.ceil((o.max(0) + pad - gmin.astype(np.float64)) / float(voxel)).astype(np.int64)
    n = np.maximum(n, 1)
    dims = (int((n[0] + 31) // 32 * 32), int(n[1]), int(n[2]))
    bits = dims[0] * dims[1] * dims[2]
    if bits >= MAX_BITS:
        raise ValueError(f"scene_grid: {dims[0]} x {dims[1]} x {dims[2]} = {bits} voxels at voxel {voxel}, the limit is 2^31 - 1: "
                         "coarsen voxel (or narrow range_xy / z_half)")
    return tuple(float(v) for v in gmin), dims


def sweep_frames(lidars: Sequence[np.ndarray], poses: Sequence[np.ndarray], sensor_offset=SENSOR_OFFSET):
    """every sweep in the frame of the first one: T_i = inv(pose_0) @ pose_i in float64; ALL rows (ground included) transformed in
    float64 and rounded to fp32; origin_i = T_i @ (sensor_offset, 1).  -> (points fp32 [N_i,3] per sweep, origins float64 [K,3])"""
    inv0 = np.linalg.inv(np.asarray(poses[0], dtype=np.float64))
    off = np.array([*sensor_offset, 1.0], dtype=np.float64)
    pts, org = [], []
    for lidar, pose in zip(lidars, poses):
        T = inv0 @ np.asarray(pose, dtype=np.float64)
        p = np.asarray(lidar)[:, :3].astype(np.float64)
        pts.append((p @ T[:3, :3].T + T[:3, 3]).astype(np.float32))
        org.append((T @ off)[:3])
    return pts, np.stack(org)


def label_sweeps(lidars: Sequence[np.ndarray], poses: Sequence[np.ndarray], *, voxel: float = 0.1, range_xy: float = 51.2,
                 z_half: float = 4.0, sensor_offset=SENSOR_OFFSET, hit_margin: int = 2, erode: int = 1, max_range: float = 80.0,
                 device="cuda", grid=None, report: Optional[dict] = None) -> List[np.ndarray]:
    """Flags of a scene given as sweeps in time order: every sweep is integrated into one map (B = 1), then every sweep is queried.
    -> uint8 [N_i] per sweep.  grid: (grid_min, dims) instead of scene_grid's; report: a dict that receives the grid and the status word."""
    pts, org = sweep_frames(lidars, poses, sensor_offset)
    gmin, dims = scene_grid(org, voxel, range_xy, z_half) if grid is None else grid
    vm = VoidMap(1, gmin, dims, voxel, hit_margin=hit_margin, erode=erode, max_range=max_range, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=vm.device)
    dev_pts = []
    for p, o in zip(pts, org):
        if p.shape[0] == 0:
            dev_pts.append(None)
            continue
        dp = torch.from_numpy(p).to(vm.device)[None]
        dc = torch.full((1,), p.shape[0], dtype=torch.int32, device=vm.device)
        vm.integrate(dp, dc, torch.from_numpy(o.astype(np.float32)).to(vm.device)[None], status)
        dev_pts.append((dp, dc))
    out = []
    for p, d in zip(pts, dev_pts):
        out.append(np.zeros(0, dtype=np.uint8) if d is None else vm.query(*d)[0].to(torch.uint8).cpu().numpy())
    if report is not None:
        report.update(grid_min=list(gmin), dims=list(dims), status=int(status))
    return out


def label_scene(h5_path: str, *, voxel: float = 0.1, range_xy: float = 51.2, z_half: float = 4.0, sensor_offset=SENSOR_OFFSET,
                hit_margin: int = 2, erode: int = 1, max_range: float = 80.0, device="cuda", grid=None,
                report: Optional[dict] = None, pose_source: str = "auto", pose_sidecar: Optional[str] = ".pose.npz") -> Dict[str, np.ndarray]:
    """Flags of every sweep of a preprocessed scene file, sweeps taken in time order: {timestamp: uint8 [N]}, N the rows of that sweep's
    ``lidar`` (ground rows included: they are cast like every other return).  pose_source / pose_sidecar: where the sweeps' poses come
    from, as ``HDF5Dataset`` reads them ("auto": the group's ``pose``, else ``<scene_id>.pose.npz`` of python -m deflow_amd.odometry)."""
    from .h5scene import H5File
    from .odometry import check_pose_source, load_pose_sidecar, sweep_pose
    check_pose_source(pose_source, pose_sidecar)
    directory, scene_id = os.path.dirname(h5_path) or ".", os.path.basename(h5_path)[:-3]
    with H5File(h5_path) as f:
        keys = sorted(f.keys(), key=int)
        lidars = [f[k]["lidar"].read() for k in keys]
        side = None
        if pose_source == "sidecar" or any("pose" not in f[k] for k in keys):
            side = load_pose_sidecar(directory, scene_id, pose_sidecar)
        poses = [sweep_pose(f[k], side, scene_id=scene_id, ts=k, pose_source=pose_source, pose_sidecar=pose_sidecar, directory=directory)
                 for k in keys]
    flags = label_sweeps(lidars, poses, voxel=voxel, range_xy=range_xy, z_half=z_half, sensor_offset=sensor_offset, hit_margin=hit_margin,
                         erode=erode, max_range=max_range, device=device, grid=grid, report=report)
    return dict(zip(keys, flags))


def write_sidecar(path: str, flags: Dict[str, np.ndarray], meta: Dict[str, Any]) -> None:
    """<scene_id>.dufo.npz: one uint8 array per timestamp and the parameters as a JSON string under ``meta``"""
    tmp = path + ".tmp.npz"
    np.savez(tmp, meta=np.array(json.dumps(meta, sort_keys=True)), **{str(k): np.asarray(v, dtype=np.uint8) for k, v in flags.items()})
    os.replace(tmp, path)


def read_sidecar(path: str) -> Dict[str, np.ndarray]:
    """the per-timestamp arrays of a sidecar (without ``meta``)"""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files if k != "meta"}


# ---- command line -----------------------------------------------------------------------------------------------------------------------
CLI_DEFAULTS: Dict[str, Any] = {"data_dir": None, "scenes": None, "overwrite": False, "voxel": 0.1, "range_xy": 51.2, "z_half": 4.0,
                                "sensor_offset": list(SENSOR_OFFSET), "hit_margin": 2, "erode": 1, "max_range": 80.0}
POSE_SOURCES = ("auto", "file", "sidecar")      # pose_source=: where poses are read; not a parameter of the map, so not among the defaults


def parse_args(argv: List[str]) -> Dict[str, Any]:
    """key=value arguments in the style of deflow_amd.train"""
    cfg = dict(CLI_DEFAULTS)
    for a in argv:
        if "=" not in a:
            raise SystemExit(f"expected key=value, got {a!r}")
        k, v = a.split("=", 1)
        k = k.lstrip("+")
        if k not in CLI_DEFAULTS and k != "pose_source":
            raise SystemExit(f"unknown key {k!r}; known: {', '.join(sorted((*CLI_DEFAULTS, 'pose_source')))}")
        try:
            if k == "data_dir":
                cfg[k] = v
            elif k == "scenes":
                cfg[k] = [s for s in v.split(",") if s]
            elif k == "overwrite":
                if v.lower() not in ("true", "false", "1", "0"):
                    raise ValueError(v)
                cfg[k] = v.lower() in ("true", "1")
            elif k == "pose_source":
                if v not in POSE_SOURCES:
                    raise ValueError(v)
                cfg[k] = v
            elif k == "sensor_offset":
                cfg[k] = [float(x) for x in v.strip("[]()").split(",")]
                if len(cfg[k]) != 3:
                    raise ValueError(v)
            elif k in ("hit_margin", "erode"):
                cfg[k] = int(v)
            else:
                cfg[k] = float(v)
        except ValueError:
            raise SystemExit(f"bad value for {k}: {v!r}")
    if not cfg["data_dir"]:
        raise SystemExit("usage: python -m deflow_amd.voidmap data_dir=<dir> [scenes=a,b] [overwrite=false] [voxel=0.1] [range_xy=51.2] "
                         "[z_half=4.0] [sensor_offset=1.35,0,1.64] [hit_margin=2] [erode=1] [max_range=80] [pose_source=auto|file|sidecar]")
    return cfg


def main(argv=None) -> int:
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    assert torch.cuda.is_available(), "the void map runs on the HIP engine only"
    d = cfg["data_dir"]
    scenes = cfg["scenes"] or sorted(n[:-3] for n in os.listdir(d) if n.endswith(".h5"))
    params = {k: cfg[k] for k in ("voxel", "range_xy", "z_half", "sensor_offset", "hit_margin", "erode", "max_range")}
    for sid in scenes:
        out = os.path.join(d, sid + SIDECAR_SUFFIX)
        if os.path.exists(out) and not cfg["overwrite"]:
            print(json.dumps({"scene": sid, "skipped": "sidecar exists (overwrite=true replaces it)"}), flush=True)
            continue
        rep: Dict[str, Any] = {}
        t0 = time.perf_counter()
        flags = label_scene(os.path.join(d, sid + ".h5"), report=rep, pose_source=cfg.get("pose_source", "auto"),
                            **{**params, "sensor_offset": tuple(params["sensor_offset"])})
        write_sidecar(out, flags, {**params, **{k: rep[k] for k in ("grid_min", "dims")}, "definition": "DESIGN.md 6c (UNPINNED)"})
        rows = sum(int(v.shape[0]) for v in flags.values())
        print(json.dumps({"scene": sid, "sweeps": len(flags), "rows": rows,
                          "flagged_fraction": round(sum(int(v.sum()) for v in flags.values()) / max(rows, 1), 6),
                          "seconds": round(time.perf_counter() - t0, 3), "status": rep["status"]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
