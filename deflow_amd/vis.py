"""``python -m deflow_amd.vis dataset_path=<dir> res_name=<name>``: the fourth thing the reference's README does with this model
([REF README.md section 3]: ``tools/visualization.py --res_name ...`` opens an interactive window on the flow ``save.py`` wrote).  A
headless node has no window, so this command writes image files: per sweep one PNG, a bird's-eye view of the raw rows coloured by their
flow with the ego motion taken out -- direction as hue, magnitude as saturation, ground rows grey -- rasterised on the GPU
(``render.render_rows``, csrc/render.hip).  UNPINNED: upstream's colour wheel and camera are absent; the picture is this project's
definition, DESIGN.md section 6i.

``flow_source=file`` (the default) draws ``<scene_id>.<res_name>.flow.npz`` as ``deflow_amd.save`` wrote it; ``flow_source=model
checkpoint=<ckpt>`` runs ``SweepFlow.infer`` inline, and the flow never leaves the device.  ``panels=est,gt,err`` puts the estimate, the
ground truth (rows with ``flow_is_valid == 0`` left out) and their difference side by side; without the key, ``gt`` and ``err`` are drawn
where the scene file carries ``flow``.  One file ``<out_dir>/<scene_id>/<timestamp>.png`` per sweep that has a successor; an existing
file is skipped unless ``overwrite=true``; one JSON line per scene on stdout.  Per batch one device-to-host copy, into pinned memory."""
from __future__ import annotations

import json
import math
import os
import sys
import time
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from .save import GROUND_SOURCES, POSE_SOURCES, ScenePairs, _Pinned, _flag, flow_path, read_flow
from .train import DEFAULTS, _TARGET_ALIASES

PANELS = ("est", "gt", "err")
OWN_DEFAULTS: Dict[str, Any] = {"dataset_path": None, "res_name": None, "flow_source": "file", "checkpoint": None, "scenes": None,
                                "out_dir": None, "panels": None, "range": 51.2, "res": 0.1, "vmax": 1.0, "vmax_err": 0.5, "radius": 1,
                                "legend": None, "every": 1, "batch_size": None, "overwrite": False, "ground_source": "auto",
                                "inference_dtype": None, "pose_source": "auto"}
USAGE = ("usage: python -m deflow_amd.vis dataset_path=<dir of .h5 files> res_name=<name> [flow_source=file|model] [checkpoint=<ckpt>] "
         "[scenes=a,b] [out_dir=<dataset_path>/vis_<res_name>] [panels=est,gt,err] [range=51.2] [res=0.1] [vmax=1.0] [vmax_err=0.5] "
         "[radius=1] [legend=<disc radius in pixels, 0 = none>] [every=1] [batch_size=] [overwrite=false] "
         "[ground_source=auto|file|sidecar|online] [pose_source=auto|file|sidecar]")


def _num(k: str, v: str, kind, lo, hi=None):
    try:
        x = kind(v)
        ok = x >= lo and (hi is None or x <= hi) and math.isfinite(x)
    except ValueError:
        ok = False
    if not ok:
        raise SystemExit(f"bad value for {k}: {v!r}")
    return x


def parse_args(argv: List[str]) -> Dict[str, Any]:
    """key=value arguments -> the options (``size``, ``view`` and ``legend`` resolved), plus under ``_rest`` the hyper-parameter overrides
    ``eval.resolve_config`` lays over the checkpoint's configuration with ``flow_source=model``.  Reads no file, needs no GPU."""
    opt = dict(OWN_DEFAULTS)
    rest: Dict[str, str] = {}
    for a in argv:
        if "=" not in a:
            raise SystemExit(f"expected key=value, got {a!r}")
        k, v = a.split("=", 1)
        k = k.lstrip("+")
        if k in ("dataset_path", "res_name", "checkpoint", "out_dir"):
            if not v:
                raise SystemExit(f"bad value for {k}: {v!r}")
            opt[k] = v
        elif k == "flow_source":
            if v not in ("file", "model"):
                raise SystemExit(f"bad value for flow_source: {v!r} (file, model)")
            opt[k] = v
        elif k == "scenes":
            opt[k] = [s for s in v.split(",") if s]
        elif k == "panels":
            names = v.split(",")
            if not v or any(n not in PANELS for n in names) or len(set(names)) != len(names):
                raise SystemExit(f"bad value for panels: {v!r} (a comma-separated selection of {', '.join(PANELS)}, each at most once)")
            opt[k] = names
        elif k in ("range", "res", "vmax", "vmax_err"):
            opt[k] = _num(k, v, float, 1e-6)
        elif k == "radius":
            opt[k] = _num(k, v, int, 0, 4)
        elif k == "legend":
            opt[k] = _num(k, v, int, 0, 2045)
        elif k == "every":
            opt[k] = _num(k, v, int, 1)
        elif k == "batch_size":
            opt[k] = _num(k, v, int, 1, 65535)
        elif k == "overwrite":
            opt[k] = _flag(k, v)
        elif k == "ground_source":
            if v not in GROUND_SOURCES:
                raise SystemExit(f"bad value for ground_source: {v!r} ({', '.join(GROUND_SOURCES)})")
            opt[k] = v
        elif k == "pose_source":
            if v not in POSE_SOURCES:
                raise SystemExit(f"bad value for pose_source: {v!r} ({', '.join(POSE_SOURCES)})")
            opt[k] = v
        elif k == "inference_dtype":
            if v not in ("fp32", "bf16"):
                raise SystemExit(f"bad value for inference_dtype: {v!r} (fp32, bf16)")
            opt[k] = v
        elif k in DEFAULTS or k in _TARGET_ALIASES or k == "model.target.grid_feature_size":
            rest[k] = f"{k}={v}"
        else:
            raise SystemExit(f"unknown key {k!r}; known: {', '.join(sorted(OWN_DEFAULTS))}, and the hyper-parameters of deflow_amd.train")
    if not opt["dataset_path"]:
        raise SystemExit(USAGE)
    if opt["flow_source"] == "model":
        if not opt["checkpoint"]:
            raise SystemExit("flow_source=model needs checkpoint=<ckpt>\n" + USAGE)
        if opt["res_name"] is None:
            opt["res_name"] = os.path.splitext(os.path.basename(opt["checkpoint"]))[0]
    elif opt["checkpoint"]:
        raise SystemExit("checkpoint= is only read with flow_source=model (flow_source=file draws the flow file of res_name)")
    elif rest:
        raise SystemExit(f"{', '.join(sorted(rest))}: the model's hyper-parameters are only read with flow_source=model")
    if not opt["res_name"] or os.sep in opt["res_name"]:
        raise SystemExit(f"bad value for res_name: {opt['res_name']!r}\n" + USAGE)
    side = int(round(2.0 * opt["range"] / opt["res"]))
    if not 1 <= side <= 4096:
        raise SystemExit(f"2 range / res = {side} pixels per side: 1 .. 4096 expected")
    opt["size"] = (side, side)
    opt["view"] = (-opt["range"], -opt["range"], 1.0 / opt["res"])
    if opt["legend"] is None:
        opt["legend"] = max(0, min(32, (side - 5) // 2))
    elif opt["legend"] > 0 and 2 * opt["legend"] + 5 > side:
        raise SystemExit(f"bad value for legend: {opt['legend']} (2 L + 5 <= {side}, the image's side, expected)")
    if opt["out_dir"] is None:
        opt["out_dir"] = os.path.join(opt["dataset_path"], "vis_" + opt["res_name"])
    opt["_rest"] = rest
    return opt


def image_path(out_dir: str, scene_id: str, timestamp) -> str:
    return os.path.join(out_dir, str(scene_id), f"{timestamp}.png")


def collate_vis_pad(items: List[Dict[str, object]]) -> Dict[str, object]:
    """``sweeps.collate_raw_pad`` plus, when every item carries it, the ground truth of the first sweep's raw rows: ``gt`` [B,N,3] f32
    padded with NaN and ``gt_valid`` [B,N] u8 padded with 0"""
    from .sweeps import collate_raw_pad
    res = collate_raw_pad(items)
    if all("flow" in b for b in items):
        n = res["raw0"].shape[1]
        gt = torch.full((len(items), n, 3), float("nan"), dtype=torch.float32)
        valid = torch.zeros(len(items), n, dtype=torch.uint8)
        for i, b in enumerate(items):
            rows = int(b["pc0"].shape[0])
            gt[i, :rows] = b["flow"].float()
            valid[i, :rows] = (b["flow_is_valid"].reshape(-1) != 0).to(torch.uint8)
        res["gt"], res["gt_valid"] = gt, valid
    return res


def draw_panels(d: Dict[str, torch.Tensor], est: torch.Tensor, panels: Sequence[str], opt: Dict[str, Any]) -> torch.Tensor:
    """the batch's device tensors (``raw0 n0 drop0`` u8, the poses, ``gt gt_valid`` for the gt / err panels) and ``est`` [B,N,3] f32 ->
    the panels side by side as scanlines [B, H, 1 + 3 W len(panels)] u8 on the device"""
    from . import render
    from .deflow import batch_transform
    raw, n = d["raw0"], d["n0"]
    T = batch_transform({k: d[k] for k in ("pose0", "pose1", "ego_motion") if k in d}, raw.device)
    cls = torch.where(d["drop0"] != 0, 2, 1).to(torch.uint8)             # ground rows grey
    kw = dict(view=opt["view"], size=opt["size"], radius=opt["radius"], legend=opt["legend"])
    out = []
    for p in panels:
        if p == "est":
            s = render.render_rows(raw, n, render.flow_vectors(raw, n, est, T), cls, vmax=opt["vmax"], **kw)
        else:
            seen = torch.where(d["gt_valid"] != 0, cls, torch.zeros_like(cls))            # rows without a valid ground truth are not drawn
            if p == "gt":
                s = render.render_rows(raw, n, render.flow_vectors(raw, n, d["gt"], T), seen, vmax=opt["vmax"], **kw)
            else:
                s = render.render_rows(raw, n, torch.sub(est, d["gt"]), seen, vmax=opt["vmax_err"], **kw)
        out.append(s if not out else s[:, :, 1:])
    return out[0] if len(out) == 1 else torch.cat(out, dim=2)


def vis_scene(pairs: ScenePairs, todo: List[int], est_for, panels: Optional[Sequence[str]], opt: Dict[str, Any], device,
              batch_size: int, ground_for=None, num_workers: int = 0, pinned: Optional[_Pinned] = None) -> Dict[str, Any]:
    """writes the images of ``pairs``' items ``todo``.  ``est_for(host_batch, device_batch)`` returns the estimate [B,N,3] f32 on the
    device; ``ground_for(B)`` a ``GroundSegmenter`` when the masks are computed online.  -> {"images": n, "panels": [...]}"""
    from torch.utils.data import DataLoader, Subset
    from .png import write_png
    pinned = pinned or _Pinned()
    W, H = opt["size"]
    written, used = 0, list(panels) if panels else None
    if not todo:
        return {"images": 0, "panels": used or []}
    loader = DataLoader(Subset(pairs, todo), batch_size=batch_size, shuffle=False, collate_fn=collate_vis_pad, num_workers=max(0, num_workers),
                        pin_memory=True, drop_last=False)
    for host in loader:
        d = {k: v.to(device, non_blocking=True) for k, v in host.items() if isinstance(v, torch.Tensor)}
        if ground_for is not None:
            d["drop0"] = ground_for(len(host["timestamp"])).segment(d["raw0"], d["n0"]).clone()
        mine = list(panels) if panels else (list(PANELS) if "gt" in d else ["est"])
        if "gt" not in d and any(p != "est" for p in mine):
            raise SystemExit(f"{host['scene_id'][0]}: panels={','.join(mine)} needs the scene file's flow and flow_is_valid, which it lacks")
        used = mine
        lines = draw_panels(d, est_for(host, d), mine, opt)
        h = pinned.like("scanlines", lines)
        h.copy_(lines, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        for i, (sid, ts) in enumerate(zip(host["scene_id"], host["timestamp"])):
            path = image_path(opt["out_dir"], sid, ts)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            write_png(path, h[i].numpy(), W * len(mine), H)
            written += 1
    return {"images": written, "panels": used or []}


def main(argv=None) -> int:
    opt = parse_args(list(sys.argv[1:] if argv is None else argv))
    assert torch.cuda.is_available(), "the vis command rasterises on the HIP engine only"
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    d, res_name, online = opt["dataset_path"], opt["res_name"], opt["ground_source"] == "online"
    batch_size, num_workers = opt["batch_size"] or 4, 0
    grounds: Dict[int, Any] = {}

    def ground_for(B: int):
        if B not in grounds:
            from .ground import GroundSegmenter
            grounds[B] = GroundSegmenter(B, device=dev)
        return grounds[B]

    sweep_flow = None
    if opt["flow_source"] == "model":
        from .eval import resolve_config
        from .sweeps import SweepFlow
        from .train import build_model
        rest = dict(opt["_rest"])
        if opt["batch_size"]:
            rest["batch_size"] = f"batch_size={opt['batch_size']}"
        cfg = resolve_config(opt["checkpoint"], rest)
        model = build_model(cfg).to(dev)
        res = model.load_from_checkpoint(opt["checkpoint"])
        if res.missing_keys or res.unexpected_keys:
            print(f"[deflow_amd.vis] WARNING: checkpoint / model mismatch (model={cfg['model']}): {len(res.missing_keys)} missing keys "
                  f"{res.missing_keys[:4]}..., {len(res.unexpected_keys)} unexpected keys {res.unexpected_keys[:4]}...", file=sys.stderr)
        model.eval()
        if opt["inference_dtype"]:
            model.inference_dtype = opt["inference_dtype"]
        batch_size, num_workers = int(cfg["batch_size"]), int(cfg["num_workers"])
        sweep_flow = SweepFlow(model)

    scenes = opt["scenes"] or sorted(n[:-3] for n in os.listdir(d) if n.endswith(".h5"))
    pinned = _Pinned()
    for sid in scenes:
        t0 = time.perf_counter()
        pairs = ScenePairs(d, sid, opt["ground_source"], pose_source=opt["pose_source"])
        every = [i for i in range(0, len(pairs), opt["every"])]
        todo = [i for i in every if opt["overwrite"] or not os.path.exists(image_path(opt["out_dir"], sid, pairs.data_index[i][1]))]
        if sweep_flow is not None:
            def est_for(host, db):
                # the masks go in as they are (ground_for has filled drop0 already when they are computed online; drop1 likewise here)
                drop1 = ground_for(len(host["timestamp"])).segment(db["raw1"], db["n1"]) if online else db["drop1"]
                return sweep_flow.infer(db["raw0"], db["n0"], db["drop0"], db["raw1"], db["n1"], drop1, db["pose0"], db["pose1"],
                                        ego_motion=db.get("ego_motion"))[0]
        else:
            path = flow_path(d, sid, res_name)
            if not os.path.exists(path):
                raise SystemExit(f"{path} not found: write it with  python -m deflow_amd.save checkpoint=<ckpt> dataset_path={d} "
                                 f"res_name={res_name}  (or draw with flow_source=model checkpoint=<ckpt>)")
            flows = read_flow(path) if todo else {}

            def est_for(host, db, flows=flows, path=path):
                est = pinned.like("est", host["raw0"])           # free again: vis_scene synchronises once per batch
                est.fill_(float("nan"))
                for i, (ts, n) in enumerate(zip(host["timestamp"], host["n0"].tolist())):      # n0 is the collate's host tensor
                    f = flows.get(str(ts))
                    if f is None or f[0].shape != (n, 3):
                        raise SystemExit(f"{path}: sweep {ts} has {n} rows, the flow file "
                                         + ("has no entry for it" if f is None else f"holds {f[0].shape[0]}"))
                    est[i, :n] = torch.from_numpy(np.ascontiguousarray(f[0], dtype=np.float32))
                return est.to(dev, non_blocking=True)
        r = vis_scene(pairs, todo, est_for, opt["panels"], opt, dev, batch_size, ground_for=ground_for if online else None,
                      num_workers=num_workers, pinned=pinned)
        print(json.dumps({"scene": sid, "images": r["images"], "skipped": len(every) - len(todo), "panels": r["panels"],
                          "size": [opt["size"][0] * max(len(r["panels"]), 1), opt["size"][1]], "out_dir": os.path.join(opt["out_dir"], sid),
                          "seconds": round(time.perf_counter() - t0, 3)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
