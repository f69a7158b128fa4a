"""``python -m deflow_amd.save checkpoint=<ckpt> dataset_path=<dir>``: the reference's third command for this model plugin
([REF README.md:106-111]: ``python save.py checkpoint=/home/kin/deflow_best.ckpt dataset_path=.../vis`` writes the estimated flow of every
sweep into the dataset under the checkpoint's name).  UNPINNED: upstream's save.py is absent; what is written per row is this project's
definition, DESIGN.md section 6f.

``dataset_path`` is the directory that holds the ``.h5`` scene files themselves.  Every sweep of every scene is paired with its successor in
timestamp order (a scene's last sweep has no successor and gets no entry; the reader's index file is not used), the raw rows go to the
device once, and ``sweeps.SweepFlow`` removes the ground rows, runs the model and puts the flow of ALL rows of the sweep together there;
one copy per batch and output array comes back.  Per scene ``<scene_id>.<res_name>.flow.npz`` holds ``"<ts>"`` (f32, or f16 with
``half=true``, [N_raw,3]) and ``"<ts>.dynamic"`` (u8 [N_raw]) per timestamp and ``meta`` (a JSON string); ``read_flow`` reads it back.

The configuration is the checkpoint's, overridden by the command line, exactly as ``deflow_amd.eval`` resolves it.  ``res_name`` defaults
to the checkpoint's file stem; ``ground_source=auto|file|sidecar`` as ``HDF5Dataset`` reads masks, ``online`` computes them on the GPU per
batch (``ground.GroundSegmenter``) and needs no mask on disk.  ``av2_mode`` is refused: the leaderboard submission (a zip of feather files) is
``python -m deflow_amd.eval checkpoint=<ckpt> av2_mode=test dataset_path=<root>``.

``python -m deflow_amd.save model=<name> dataset_path=<dir> [res_name=<name>] [ground_source=...] [<prefix>_*=...]`` needs no checkpoint:
the flow comes from a checkpoint-free pair model of the table in ``deflow_amd.pairflow`` (DESIGN.md sections 6j to 6n, UNPINNED; 6o for
the table).  ``voxel_size`` and ``point_cloud_range`` decide which rows are decoded, the model's own keys (its module's ``COMMAND_KEYS``)
are its parameters; all of them go into the file's ``meta``.  Another model's keys are refused.  ``python -m deflow_amd.train ...
pseudo_flow=<res_name>`` then trains on the file as pseudo labels."""
from __future__ import annotations

import json
import os
import sys
import threading
import time
from collections import OrderedDict
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import pairflow
from .data import HDF5Dataset
from .odometry import check_pose_source
from .train import DEFAULTS, _TARGET_ALIASES

FLOW_SUFFIX = ".flow.npz"
POSE_SOURCES = ("auto", "file", "sidecar")
GROUND_SOURCES = ("auto", "file", "sidecar", "online")
OWN_DEFAULTS: Dict[str, Any] = {"checkpoint": None, "dataset_path": None, "res_name": None, "scenes": None, "ground_source": "auto",
                                "half": False, "overwrite": False, "inference_dtype": None, "pose_source": "auto"}
USAGE = ("usage: python -m deflow_amd.save checkpoint=<ckpt> dataset_path=<dir of .h5 files> [res_name=<checkpoint file stem>] [scenes=a,b] "
         "[batch_size=] [num_workers=] [ground_source=auto|file|sidecar|online] [half=false] [overwrite=false] [inference_dtype=fp32|bf16] "
         "[pose_source=auto|file|sidecar]")


def _flag(k: str, v: str) -> bool:
    if v.lower() not in ("true", "false", "1", "0"):
        raise SystemExit(f"bad value for {k}: {v!r} (true, false)")
    return v.lower() in ("true", "1")


def parse_args(argv: List[str]) -> Dict[str, Any]:
    """key=value arguments -> this command's own options, plus under ``_rest`` ({key: "key=value"}) the hyper-parameter overrides that
    ``eval.resolve_config`` lays over the checkpoint's configuration.  Reads no file."""
    opt = dict(OWN_DEFAULTS)
    rest: Dict[str, str] = {}
    own: Dict[str, str] = {}            # the keys of the checkpoint-free pair models (deflow_amd/pairflow.py), whichever model's
    for a in argv:
        if "=" not in a:
            raise SystemExit(f"expected key=value, got {a!r}")
        k, v = a.split("=", 1)
        k = k.lstrip("+")
        if k == "av2_mode":
            raise SystemExit("deflow_amd.save writes <scene_id>.<res_name>.flow.npz beside the scene files and takes no av2_mode: the "
                             "av2_mode=test leaderboard submission, a zip of feather files, is written by  python -m deflow_amd.eval checkpoint=<ckpt> "
                             "av2_mode=test dataset_path=<root>")
        if k in ("checkpoint", "dataset_path", "res_name"):
            if not v:
                raise SystemExit(f"bad value for {k}: {v!r}")
            opt[k] = v
        elif k == "scenes":
            opt[k] = [s for s in v.split(",") if s]
        elif k in ("half", "overwrite"):
            opt[k] = _flag(k, v)
        elif k == "ground_source":
            if v not in GROUND_SOURCES:
                raise SystemExit(f"bad value for ground_source: {v!r} ({', '.join(GROUND_SOURCES)})")
            opt[k] = v
        elif k == "pose_source":                # where poses are read (HDF5Dataset(pose_source=...)); never written into the file's meta
            if v not in POSE_SOURCES:
                raise SystemExit(f"bad value for pose_source: {v!r} ({', '.join(POSE_SOURCES)})")
            opt[k] = v
        elif k == "inference_dtype":
            if v not in ("fp32", "bf16"):
                raise SystemExit(f"bad value for inference_dtype: {v!r} (fp32, bf16)")
            opt[k] = v
        elif pairflow.owner(k):
            own[k] = v
        elif k in DEFAULTS or k in _TARGET_ALIASES or k == "model.target.grid_feature_size":
            if k in ("batch_size", "num_workers"):
                try:
                    ok = int(v) >= (1 if k == "batch_size" else 0)
                except ValueError:
                    ok = False
                if not ok:
                    raise SystemExit(f"bad value for {k}: {v!r}")
            rest[k] = f"{k}={v}"
        else:
            raise SystemExit(f"unknown key {k!r}; known: {', '.join(sorted(OWN_DEFAULTS))}, and the hyper-parameters of deflow_amd.train")
    pair = pairflow.selected(rest, keys=("model", "model.name"))
    opt["model"], opt["params"] = (pair.name if pair else None), None       # a model of pairflow.TABLE and its parameters, or None
    wrong = pairflow.foreign_keys(own, pair)
    if pair:
        usage = pairflow.usage(pair)
        if opt["checkpoint"] or opt["inference_dtype"]:
            raise SystemExit(f"model={pair.name} has no weights: it takes neither checkpoint= nor inference_dtype=\n" + usage)
        if wrong:
            raise SystemExit(wrong[1] + "\n" + usage)
        if not opt["dataset_path"]:
            raise SystemExit(usage)
        rest.pop("model", None), rest.pop("model.name", None)
        if pairflow.module(pair).COMMAND_BATCH_SIZE is not None:
            rest.setdefault("batch_size", f"batch_size={pairflow.module(pair).COMMAND_BATCH_SIZE}")
        opt["params"] = pairflow.params_from_command(pair, own)
        if opt["res_name"] is None:
            opt["res_name"] = pair.name
    elif wrong:
        raise SystemExit(wrong[1] + "\n" + pairflow.usage(wrong[0]))
    elif not opt["checkpoint"] or not opt["dataset_path"]:
        raise SystemExit(USAGE)
    if opt["res_name"] is None:
        opt["res_name"] = os.path.splitext(os.path.basename(opt["checkpoint"]))[0]
    if not opt["res_name"] or os.sep in opt["res_name"]:
        raise SystemExit(f"bad value for res_name: {opt['res_name']!r}")
    opt["_rest"] = rest
    return opt


# ---- the flow file --------------------------------------------------------------------------------------------------------------------
def flow_path(directory: str, scene_id: str, res_name: str) -> str:
    return os.path.join(directory, f"{scene_id}.{res_name}{FLOW_SUFFIX}")


def write_flow(path: str, flows: Dict[str, Tuple[np.ndarray, np.ndarray]], meta: Dict[str, Any]) -> None:
    """<scene_id>.<res_name>.flow.npz: per timestamp ``"<ts>"`` (f32 or f16 [N,3]) and ``"<ts>.dynamic"`` (u8 [N]); ``meta`` a JSON string.
    Written to a temporary file and moved into place."""
    arrays: Dict[str, np.ndarray] = {}
    for ts, (flow, dynamic) in flows.items():
        flow = np.asarray(flow)
        if flow.dtype not in (np.float32, np.float16) or flow.ndim != 2 or flow.shape[1] != 3:
            raise ValueError(f"write_flow: sweep {ts}: float32 or float16 [N,3] expected, got {flow.dtype} {flow.shape}")
        dynamic = np.asarray(dynamic, dtype=np.uint8).reshape(-1)
        if dynamic.shape[0] != flow.shape[0]:
            raise ValueError(f"write_flow: sweep {ts}: {flow.shape[0]} flow rows, {dynamic.shape[0]} dynamic flags")
        arrays[str(ts)] = flow
        arrays[f"{ts}.dynamic"] = dynamic
    tmp = path + ".tmp.npz"
    np.savez(tmp, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    os.replace(tmp, path)


def read_flow(path: str) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """{timestamp: (flow [N,3], dynamic u8 [N])} of a flow file (without ``meta``)"""
    with np.load(path, allow_pickle=False) as z:
        return {k: (z[k], z[k + ".dynamic"]) for k in z.files if k != "meta" and not k.endswith(".dynamic")}


def read_meta(path: str) -> Dict[str, Any]:
    with np.load(path, allow_pickle=False) as z:
        return json.loads(str(z["meta"]))


# ---- the pairs of one scene -----------------------------------------------------------------------------------------------------------
class ScenePairs(HDF5Dataset):
    """``HDF5Dataset`` items for every sweep of ONE scene file that has a successor, in timestamp order -- its reading of sweeps, poses and
    ground masks without its index file (and so without the step-back rule for a scene's last sweep).  ``ground_source="online"``: the
    items carry all-False masks; the caller computes them on the GPU."""

    def __init__(self, directory: str, scene_id: str, ground_source: str = "auto", ground_sidecar: str = ".ground.npz",
                 pose_source: str = "auto", pose_sidecar: Optional[str] = ".pose.npz"):
        if ground_source not in GROUND_SOURCES:
            raise ValueError(f"ground_source must be one of {', '.join(GROUND_SOURCES)}, got {ground_source!r}")
        check_pose_source(pose_source, pose_sidecar)
        self.pose_source, self.pose_sidecar = pose_source, pose_sidecar
        self._pose_sidecars: "OrderedDict[str, Optional[dict]]" = OrderedDict()
        self.directory, self.ground_source, self.ground_sidecar = directory, ground_source, ground_sidecar
        self.dynamic_key, self.dynamic_sidecar = "", None           # the dynamic flags are not needed here
        self._sidecars: "OrderedDict[str, Optional[dict]]" = OrderedDict()
        self._ground_sidecars: "OrderedDict[str, Optional[dict]]" = OrderedDict()
        self._files: "OrderedDict[str, Any]" = OrderedDict()
        self._lock = threading.Lock()
        self._max_open = 8
        self.index_file = None
        self.sweeps: List[str] = list(self._file(scene_id).sweeps)
        self.data_index = [[scene_id, ts] for ts in self.sweeps[:-1]]

    def _ground(self, scene_id, ts, group, rows):
        if self.ground_source == "online":
            return torch.zeros(rows, dtype=torch.bool)
        return super()._ground(scene_id, ts, group, rows)


class _Pinned:
    """one growing page-locked buffer per output array: the target of the batch's device-to-host copy"""

    def __init__(self):
        self._buf: Dict[str, torch.Tensor] = {}

    def like(self, name: str, t: torch.Tensor) -> torch.Tensor:
        b = self._buf.get(name)
        if b is None or b.dtype != t.dtype or b.numel() < t.numel():
            b = self._buf[name] = torch.empty(t.numel(), dtype=t.dtype, pin_memory=True)
        return b[: t.numel()].view(t.shape)


def save_scene(sweep_flow_for, pairs: ScenePairs, batch_size: int, device, *, half: bool = False, online: bool = False,
               num_workers: int = 0, pinned: Optional[_Pinned] = None) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
    """{timestamp: (flow_est [N_raw,3], dynamic [N_raw])} for every pair of ``pairs``.  ``sweep_flow_for(B)`` returns the ``SweepFlow`` for
    a batch of B (a ground segmenter belongs to one batch size).  Per batch: one host-to-device copy per input, one device-to-host copy
    per output array into pinned memory, no per-sample reads."""
    from torch.utils.data import DataLoader
    from .sweeps import collate_raw_pad
    pinned = pinned or _Pinned()
    out: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
    if len(pairs) == 0:
        return out
    loader = DataLoader(pairs, batch_size=batch_size, shuffle=False, collate_fn=collate_raw_pad, num_workers=max(0, num_workers),
                        pin_memory=True, drop_last=False)
    for host in loader:
        d = {k: v.to(device, non_blocking=True) for k, v in host.items() if isinstance(v, torch.Tensor)}
        sf = sweep_flow_for(len(host["timestamp"]))
        flow_est, dynamic = sf.infer(d["raw0"], d["n0"], None if online else d["drop0"], d["raw1"], d["n1"], None if online else d["drop1"],
                                     d["pose0"], d["pose1"], ego_motion=d.get("ego_motion"), half=half)
        hf, hd = pinned.like("flow_est", flow_est), pinned.like("dynamic", dynamic)
        hf.copy_(flow_est, non_blocking=True)
        hd.copy_(dynamic, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        for i, (ts, n) in enumerate(zip(host["timestamp"], host["n0"].tolist())):      # n0 is the collate's host tensor
            out[str(ts)] = (hf[i, :n].numpy().copy(), hd[i, :n].numpy().copy())
    return out


def main(argv=None, wrap=None) -> int:
    """wrap: optional callable (model, meta) -> model, applied to the finished model before any sweep runs; it may amend the flow file's
    meta (``python -m deflow_amd.refine save`` passes one).  Without it the command is what it was."""
    opt = parse_args(list(sys.argv[1:] if argv is None else argv))
    assert torch.cuda.is_available(), "the save command runs on the HIP engine only"
    from .eval import resolve_config
    from .sweeps import SweepFlow
    from .train import build_model, parse_overrides
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    d, res_name, online = opt["dataset_path"], opt["res_name"], opt["ground_source"] == "online"
    pair = pairflow.entry(opt["model"])
    if pair:
        # no checkpoint, no weights: the configuration is the defaults under the command line
        cfg = parse_overrides(list(opt["_rest"].values()))
        model = pairflow.build(pair, cfg, opt["params"])
        meta = {"res_name": res_name, "checkpoint": None, "model": pair.name, "voxel_size": [float(v) for v in cfg["voxel_size"]],
                "point_cloud_range": [float(v) for v in cfg["point_cloud_range"]], "ground_source": opt["ground_source"],
                "half": bool(opt["half"]), "params": dict(model.params), "definition": f"DESIGN.md 6f, {pair.section} (UNPINNED)"}
    else:
        cfg = resolve_config(opt["checkpoint"], opt["_rest"])
        model = build_model(cfg).to(dev)
        res = model.load_from_checkpoint(opt["checkpoint"])
        if res.missing_keys or res.unexpected_keys:
            print(f"[deflow_amd.save] WARNING: checkpoint / model mismatch (model={cfg['model']}): {len(res.missing_keys)} missing keys "
                  f"{res.missing_keys[:4]}..., {len(res.unexpected_keys)} unexpected keys {res.unexpected_keys[:4]}...", file=sys.stderr)
        model.eval()
        if opt["inference_dtype"]:
            model.inference_dtype = opt["inference_dtype"]
        meta = {"res_name": res_name, "checkpoint": os.path.basename(opt["checkpoint"]), "model": cfg["model"],
                "voxel_size": [float(v) for v in cfg["voxel_size"]], "point_cloud_range": [float(v) for v in cfg["point_cloud_range"]],
                "ground_source": opt["ground_source"], "half": bool(opt["half"]), "definition": "DESIGN.md 6f (UNPINNED)"}
    if wrap is not None:
        model = wrap(model, meta)
    scenes =opt["scenes"] or sorted(n[:-3] for n in os.listdir(d) if n.endswith(".h5"))
    flows_for: Dict[int, SweepFlow] = {}

    def sweep_flow_for(B: int) -> SweepFlow:
        if B not in flows_for:
            ground = None
            if online:
                from .ground import GroundSegmenter
                ground = GroundSegmenter(B, device=dev)
            flows_for[B] = SweepFlow(model, ground=ground)
        return flows_for[B]

    pinned = _Pinned()
    for sid in scenes:
        out = flow_path(d, sid, res_name)
        if os.path.exists(out) and not opt["overwrite"]:
            print(json.dumps({"scene": sid, "skipped": "flow file exists (overwrite=true replaces it)"}), flush=True)
            continue
        t0 = time.perf_counter()
        pairs = ScenePairs(d, sid, opt["ground_source"], pose_source=opt["pose_source"])
        flows = save_scene(sweep_flow_for, pairs, int(cfg["batch_size"]), dev, half=opt["half"], online=online,
                           num_workers=int(cfg["num_workers"]), pinned=pinned)
        write_flow(out, flows, meta)
        rows = sum(int(f.shape[0]) for f, _ in flows.values())
        print(json.dumps({"scene": sid, "sweeps": len(flows), "rows": rows,
                          "dynamic_fraction": round(sum(int(m.sum()) for _, m in flows.values()) / max(rows, 1), 6),
                          "seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
