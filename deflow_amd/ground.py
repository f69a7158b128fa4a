"""Ground segmentation on the GPU: the per-point ``ground_mask`` of a raw sweep, the one input of the self-supervised chain that plain
``lidar`` + ``pose`` scene files could not supply (``HDF5Dataset`` reads it, ``collate_fn_pad`` drops those rows).

UNPINNED: upstream writes the mask offline on the CPU with a line-fit ground segmenter (the code is in the absent submodule).  What runs
here is a height-map segmenter with every choice fixed -- the definition is in include/deflow_amd.h and DESIGN.md section 6d -- so the
maps and the mask are a pure integer function of the input and bit-reproducible.  Parity with upstream's masks is not claimed and was not
measured.  Per xy cell the lowest return; from the cell under the vehicle outwards every cell follows its own chain of ancestors and takes
over a cell's minimum when it continues the ground height reached so far (within ``rise`` up, ``drop`` down, widened by ``widen`` per cell
missed); a return no higher than ``tol`` above its cell's ground height is ground.

``GroundSegmenter`` is the op (CUDA tensors only: there is no CPU fallback, and nothing in it reads a device value back);
``label_scene`` segments every sweep of a scene file with it, and ``python -m deflow_amd.ground data_dir=<dir>`` writes
``<scene_id>.ground.npz`` beside every scene, which ``HDF5Dataset`` picks up when the file has no ``ground_mask``."""
from __future__ import annotations

import functools
import json
import math
import os
import sys
import time
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from ._lib import call, ptr, stream
from .args import tensor

SIDECAR_SUFFIX = ".ground.npz"
EMPTY = 2 ** 31 - 1
# seed_z: the recalled height of the AV2 vehicle frame above the road, negated -- UNPINNED, hence an argument everywhere
DEFAULTS: Dict[str, Any] = {"xy_min": (-51.2, -51.2), "cell": 0.5, "dims": (205, 205), "z_min": -5.0, "z_unit": 0.01, "z_levels": 1000,
                            "origin": (0.0, 0.0), "seed_z": -0.33, "rise": 0.10, "drop": 0.15, "widen": 0.03, "miss_cap": 8, "tol": 0.15}


def _quant(v: float, lo: float, k) -> np.float32:
    """fp32(fp32(v - lo) * k), the rows' quantisation, on the host"""
    with np.errstate(all="ignore"):
        return np.float32(np.float32(np.float32(v) - np.float32(lo)) * np.float32(k))


_check = functools.partial(tensor, "GroundSegmenter", other="the segmenter is")


class GroundSegmenter:
    """The ground height map of ``batch`` samples over one xy grid, and the mask of the last sweep.

    xy_min: the grid's lower corner (rounded to fp32); cell: the cell size; dims (Gx, Gy), each in 1..4096; heights are counted in
    z_levels (1..2^20) levels of z_unit from z_min.  origin: the xy position the chains start from (its cell, clamped into the grid);
    seed_z: the ground height expected there.  rise / drop: how far a cell's minimum may lie above / below the height reached so far to
    continue it; widen: added to both per cell missed since (at most miss_cap, 0..64, of them); tol: a row at most this far above its
    cell's ground height is ground.  The four lengths count in whole levels, round(v / z_unit)."""

    def __init__(self, batch: int, *, xy_min: Sequence[float] = DEFAULTS["xy_min"], cell: float = DEFAULTS["cell"],
                 dims: Sequence[int] = DEFAULTS["dims"], z_min: float = DEFAULTS["z_min"], z_unit: float = DEFAULTS["z_unit"],
                 z_levels: int = DEFAULTS["z_levels"], origin: Sequence[float] = DEFAULTS["origin"], seed_z: float = DEFAULTS["seed_z"],
                 rise: float = DEFAULTS["rise"], drop: float = DEFAULTS["drop"], widen: float = DEFAULTS["widen"],
                 miss_cap: int = DEFAULTS["miss_cap"], tol: float = DEFAULTS["tol"], device):
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError("GroundSegmenter: device must be a CUDA device (deflow_amd has no CPU fallback)")
        if device.index is None:               # "cuda" -> the current device, so that tensors' devices compare equal to the segmenter's
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else device
        if int(batch) != batch or not 1 <= int(batch) <= 65535:
            raise ValueError(f"GroundSegmenter: batch must be in 1..65535, got {batch}")
        if len(tuple(xy_min)) != 2 or len(tuple(dims)) != 2 or len(tuple(origin)) != 2:
            raise ValueError("GroundSegmenter: xy_min, dims and origin have two entries each")
        xy = tuple(float(np.float32(v)) for v in xy_min)
        org = tuple(float(v) for v in origin)
        Gx, Gy = (int(v) for v in dims)
        if not all(math.isfinite(v) for v in xy):
            raise ValueError(f"GroundSegmenter: xy_min must be finite, got {xy_min}")
        if not all(math.isfinite(v) for v in org):
            raise ValueError(f"GroundSegmenter: origin must be finite, got {origin}")
        if not (1 <= Gx <= 4096 and 1 <= Gy <= 4096):
            raise ValueError(f"GroundSegmenter: dims must each be in 1..4096, got {(Gx, Gy)}")
        for name, v in (("cell", cell), ("z_unit", z_unit)):
            if not (v > 0 and math.isfinite(v) and math.isfinite(1.0 / v)):
                raise ValueError(f"GroundSegmenter: {name} must be a positive finite size, got {v}")
        for name, v in (("z_min", z_min), ("seed_z", seed_z)):
            if not math.isfinite(v):
                raise ValueError(f"GroundSegmenter: {name} must be finite, got {v}")
        if int(z_levels) != z_levels or not 1 <= int(z_levels) <= 1 << 20:
            raise ValueError(f"GroundSegmenter: z_levels must be in 1..2^20, got {z_levels}")
        if int(miss_cap) != miss_cap or not 0 <= int(miss_cap) <= 64:
            raise ValueError(f"GroundSegmenter: miss_cap must be an integer in 0..64, got {miss_cap}")
        levels = {}
        for name, v in (("rise", rise), ("drop", drop), ("widen", widen), ("tol", tol)):
            if not (math.isfinite(v) and v >= 0) or round(float(v) / float(z_unit)) > 1 << 24:
                raise ValueError(f"GroundSegmenter: {name} must be a finite length >= 0 of at most 2^24 levels, got {v}")
            levels[name] = int(round(float(v) / float(z_unit)))
        self.batch, self.xy_min, self.cell, self.dims, self.device = int(batch), xy, float(cell), (Gx, Gy), device
        self.z_min, self.z_unit, self.z_levels = float(np.float32(z_min)), float(z_unit), int(z_levels)
        self.origin, self.seed_z, self.miss_cap = org, float(seed_z), int(miss_cap)
        self.rise, self.drop, self.widen, self.tol = float(rise), float(drop), float(widen), float(tol)
        self.RISE, self.DROP, self.WIDEN, self.TOL = levels["rise"], levels["drop"], levels["widen"], levels["tol"]
        self.kxy = float(np.float32(1.0 / float(cell)))                # fp32(1 / cell) and fp32(1 / z_unit), computed on the host
        self.kz = float(np.float32(1.0 / float(z_unit)))
        self.ox = int(min(max(np.floor(_quant(org[0], xy[0], self.kxy)), 0), Gx - 1))     # the origin cell, clamped into the grid
        self.oy = int(min(max(np.floor(_quant(org[1], xy[1], self.kxy)), 0), Gy - 1))
        seed = float(np.floor(_quant(seed_z, z_min, self.kz)))
        if not abs(seed) <= 1 << 24:
            raise ValueError(f"GroundSegmenter: seed_z {seed_z} lies {seed} levels from z_min, the limit is 2^24")
        self.seed = int(seed)
        self._zmin = torch.full((self.batch, Gy, Gx), EMPTY, dtype=torch.int32, device=device)
        self._height = torch.full((self.batch, Gy, Gx), self.seed, dtype=torch.int32, device=device)
        self._observed = torch.zeros(self.batch, Gy, Gx, dtype=torch.uint8, device=device)

    def params(self) -> Dict[str, Any]:
        """every parameter, as plain values (the sidecar's ``meta``)"""
        return {"xy_min": list(self.xy_min), "cell": self.cell, "dims": list(self.dims), "z_min": self.z_min, "z_unit": self.z_unit,
                "z_levels": self.z_levels, "origin": list(self.origin), "seed_z": self.seed_z, "rise": self.rise, "drop": self.drop,
                "widen": self.widen, "miss_cap": self.miss_cap, "tol": self.tol}

    # the maps of the last sweep, [batch, Gy, Gx]
    @property
    def cell_min(self) -> torch.Tensor:
        """i32: the lowest level of each cell's rows, 2^31 - 1 where the cell has none"""
        return self._zmin

    @property
    def height(self) -> torch.Tensor:
        """i32: the ground level of each cell"""
        return self._height

    @property
    def observed(self) -> torch.Tensor:
        """u8: 1 where the cell's own minimum was taken as its ground level, 0 where the level is carried over from an ancestor"""
        return self._observed

    def height_m(self) -> torch.Tensor:
        """f32 [batch, Gy, Gx]: the ground height in metres (the lower edge of the level), for callers that want height above ground"""
        return self._height.to(torch.float32) * self.z_unit + self.z_min

    def _row_args(self):
        return (*self.xy_min, self.kxy, self.z_min, self.kz, *self.dims, self.z_levels)

    def segment(self, points: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
        """One sweep per sample: points [B,N,3] f32 with count [B] i32 valid leading rows -> bool [B,N], True = ground.  Afterwards
        ``cell_min``, ``height`` and ``observed`` hold this sweep's maps."""
        _check("points", points)
        if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] != self.batch or points.shape[1] < 1:
            raise ValueError(f"GroundSegmenter: points [{self.batch},N,3] with N >= 1 expected, got {tuple(points.shape)}")
        B, N, _ = points.shape
        _check("points", points, torch.float32, (B, N, 3), self.device)
        _check("count", count, torch.int32, (B,), self.device)
        points, count = points.detach().contiguous(), count.contiguous()
        mask = torch.empty(B, N, dtype=torch.uint8, device=self.device)
        s = stream()
        call("df_ground_cells", ptr(points), ptr(count), B, N, *self._row_args(), ptr(self._zmin), s)
        call("df_ground_height", ptr(self._zmin), B, *self.dims, self.ox, self.oy, self.seed, self.RISE, self.DROP, self.WIDEN,
             self.miss_cap, ptr(self._height), ptr(self._observed), s)
        call("df_ground_mask", ptr(points), ptr(count), B, N, *self._row_args(), ptr(self._height), self.TOL, ptr(mask), s)
        return mask != 0


# ---- scene labeller ---------------------------------------------------------------------------------------------------------------------
def label_sweeps(lidars: Sequence[np.ndarray], *, device="cuda", report: Optional[dict] = None, **params) -> List[np.ndarray]:
    """Masks of sweeps given as arrays [N_i, >= 3], each in its own vehicle frame, all rows used: one B = 1 segmenter, one call per sweep.
    -> uint8 [N_i] per sweep.  report: a dict that receives the parameters and the fraction of observed cells."""
    seg = GroundSegmenter(1, device=device, **params)
    out, observed = [], []
    for lidar in lidars:
        p = np.ascontiguousarray(np.asarray(lidar)[:, :3], dtype=np.float32)
        if p.shape[0] == 0:
            out.append(np.zeros(0, dtype=np.uint8))
            continue
        dp = torch.from_numpy(p).to(seg.device)[None]
        dc = torch.full((1,), p.shape[0], dtype=torch.int32, device=seg.device)
        out.append(seg.segment(dp, dc)[0].to(torch.uint8).cpu().numpy())
        observed.append(seg.observed.sum(dtype=torch.int64))
    if report is not None:
        cells = seg.dims[0] * seg.dims[1] * max(len(observed), 1)
        report.update(params=seg.params(), observed_cell_fraction=(int(torch.stack(observed).sum()) / cells if observed else 0.0))
    return out


def label_scene(h5_path: str, *, device="cuda", report: Optional[dict] = None, **params) -> Dict[str, np.ndarray]:
    """Masks of every sweep of a preprocessed scene file: {timestamp: uint8 [N]}, N the rows of that sweep's ``lidar``, each sweep
    segmented in its own vehicle frame."""
    from .h5scene import H5File
    with H5File(h5_path) as f:
        keys = sorted(f.keys(), key=int)
        lidars = [f[k]["lidar"].read() for k in keys]
    return dict(zip(keys, label_sweeps(lidars, device=device, report=report, **params)))


def write_sidecar(path: str, masks: Dict[str, np.ndarray], meta: Dict[str, Any]) -> None:
    """<scene_id>.ground.npz: one uint8 array per timestamp and the parameters as a JSON string under ``meta``"""
    tmp = path + ".tmp.npz"
    np.savez(tmp, meta=np.array(json.dumps(meta, sort_keys=True)), **{str(k): np.asarray(v, dtype=np.uint8) for k, v in masks.items()})
    os.replace(tmp, path)


def read_sidecar(path: str) -> Dict[str, np.ndarray]:
    """the per-timestamp arrays of a sidecar (without ``meta``)"""
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files if k != "meta"}


# ---- command line -----------------------------------------------------------------------------------------------------------------------
CLI_DEFAULTS: Dict[str, Any] = {"data_dir": None, "scenes": None, "overwrite": False,
                                **{k: (list(v) if isinstance(v, tuple) else v) for k, v in DEFAULTS.items()}}
USAGE = ("usage: python -m deflow_amd.ground data_dir=<dir> [scenes=a,b] [overwrite=false] [xy_min=-51.2,-51.2] [cell=0.5] [dims=205,205] "
         "[z_min=-5] [z_unit=0.01] [z_levels=1000] [origin=0,0] [seed_z=-0.33] [rise=0.1] [drop=0.15] [widen=0.03] [miss_cap=8] [tol=0.15]")


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
            elif k == "overwrite":
                if v.lower() not in ("true", "false", "1", "0"):
                    raise ValueError(v)
                cfg[k] = v.lower() in ("true", "1")
            elif k in ("xy_min", "origin", "dims"):
                cfg[k] = [(int if k == "dims" else float)(x) for x in v.strip("[]()").split(",")]
                if len(cfg[k]) != 2:
                    raise ValueError(v)
            elif k in ("z_levels", "miss_cap"):
                cfg[k] = int(v)
            else:
                cfg[k] = float(v)
        except ValueError:
            raise SystemExit(f"bad value for {k}: {v!r}")
    if not cfg["data_dir"]:
        raise SystemExit(USAGE)
    return cfg


def main(argv=None) -> int:
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    assert torch.cuda.is_available(), "the ground segmenter runs on the HIP engine only"
    d = cfg["data_dir"]
    scenes = cfg["scenes"] or sorted(n[:-3] for n in os.listdir(d) if n.endswith(".h5"))
    params = {k: (tuple(cfg[k]) if isinstance(cfg[k], list) else cfg[k]) for k in DEFAULTS}
    for sid in scenes:
        out = os.path.join(d, sid + SIDECAR_SUFFIX)
        if os.path.exists(out) and not cfg["overwrite"]:
            print(json.dumps({"scene": sid, "skipped": "sidecar exists (overwrite=true replaces it)"}), flush=True)
            continue
        rep: Dict[str, Any] = {}
        t0 = time.perf_counter()
        masks = label_scene(os.path.join(d, sid + ".h5"), report=rep, **params)
        write_sidecar(out, masks, {**rep["params"], "definition": "DESIGN.md 6d (UNPINNED)"})
        rows = sum(int(v.shape[0]) for v in masks.values())
        print(json.dumps({"scene": sid, "sweeps": len(masks), "rows": rows,
                          "ground_fraction": round(sum(int(v.sum()) for v in masks.values()) / max(rows, 1), 6),
                          "observed_cell_fraction": round(rep["observed_cell_fraction"], 6),
                          "seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
