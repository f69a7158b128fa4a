"""``python -m deflow_amd.eval checkpoint=<ckpt> av2_mode=val dataset_path=<root>``: the reference's evaluation entry for this
model plugin ([REF README.md:88]: "python eval.py checkpoint=... av2_mode=val  # it will directly prints all metric";
[REF assets/slurm/2_eval.sh:33-35]: ``eval.py wandb_mode=online dataset_path=/scratch/local/av2/sensor av2_mode=val checkpoint=...``
-> the scene files under ``<dataset_path>/val``; ``val_data=<dir>`` names the directory directly).

The checkpoint carries its training configuration (``hyper_parameters``, as Lightning checkpoints do), so only the
checkpoint and the data need naming.  Metrics: deflow_amd/metrics.py -- ``leaderboard_version=1`` (default) the Argoverse-2 three-way
EPE table, ``leaderboard_version=2`` the bucketed normalised EPE; plus a range-free EPE / accuracy summary -- over the sweeps
of ``val_data`` (preprocessed scene files, deflow_amd/data.py) or over seeded synthetic pairs with ``val_data=synthetic``.
``metrics_impl=device`` accumulates the same tables and summary on the GPU (deflow_amd/metrics_device.py: no host sync per batch; default
``host``).

``python -m deflow_amd.eval checkpoint=<ckpt> av2_mode=test dataset_path=<root> [leaderboard_version=1|2]`` ([REF README.md:90-91]: "it
will output a command with absolute path of a zip file for you to submit to leaderboard") writes the Argoverse-2 submission of the frames
under ``<root>/test`` (``test_data=<dir>`` names the directory itself): per frame of the directory's index that carries an ``eval_mask`` and
has a successor, ``<scene_id>/<timestamp>.feather`` with the fp16 flow of the masked rows, in one zip (``output=<zip>``, default
``<checkpoint stem>.av2_submit_v<version>.zip`` beside the checkpoint).  The rows are selected, rounded and laid out as the file's body on
the GPU (deflow_amd/submit.py, DESIGN.md section 6g, UNPINNED); deflow_amd/feather.py wraps the metadata around it.  ``ground_source=
auto|file|sidecar|online``, ``batch_size=``, ``num_workers=`` and ``inference_dtype=`` as in ``deflow_amd.save``.

``python -m deflow_amd.eval model=<name> [av2_mode=val] [<prefix>_*=]`` evaluates a checkpoint-free pair model of the table in
``deflow_amd.pairflow`` instead: no ``checkpoint=``, its own keys validated by its module, another model's keys refused."""
from __future__ import annotations

import json
import os
import sys
from typing import Any, Dict, List

import torch

from . import pairflow
from .train import DATA_KEYS, DEFAULTS, _TARGET_ALIASES, build_model, grid_from, parse_overrides, split_metrics_impl, split_pose_source


def resolve_config(path: str, given: dict, skip=()) -> dict:
    """The configuration of a command that works from a checkpoint (eval, save): defaults < what the checkpoint was trained with < what
    the command line names.  ``given``: {key: "key=value"} as typed; the keys in ``skip`` are the command's own and are left out.  The
    reference's Lightning checkpoints hold a NESTED (omegaconf) config -- model.target.num_iters etc. -- so it is flattened to the
    dotted keys used here; keys this trainer does not know are ignored."""
    from .ckpt import flatten, load_checkpoint, plain
    ckpt = load_checkpoint(path)
    cfg = dict(DEFAULTS)
    hp = plain(ckpt.get("hyper_parameters", {}))
    saved = flatten(hp.get("cfg", hp) if isinstance(hp, dict) else {})
    # nested reference configs name the architecture ``model.name`` (and repeat voxel_size / point_cloud_range under
    # ``model.target``): map them onto this trainer's keys BEFORE filtering, or a fastflow3d checkpoint is built as DeFlow and
    # loaded with strict=False
    saved = {_TARGET_ALIASES.get(k, k): v for k, v in saved.items()}
    cfg.update({k: v for k, v in saved.items() if k in DEFAULTS and k not in DATA_KEYS and not isinstance(v, dict)})
    typed = parse_overrides([a for k, a in given.items() if k not in skip])
    cfg.update({k: typed[k] for k in typed["_given"] if k in typed})
    for k in ("train_data", "val_data"):       # dataset_path=<root> [REF 2_eval.sh:33-35] -> <root>/val
        if typed[k] != DEFAULTS[k]:
            cfg[k] = typed[k]
    if cfg["model"] == "fastflow3d":
        cfg["model.target.decoder_option"] = "linear"
    return cfg


# ---- av2_mode=test: the leaderboard submission ---------------------------------------------------------------------------------------------
TEST_OWN_KEYS = ("leaderboard_version", "test_data", "output", "ground_source", "inference_dtype")     # not hyper-parameters: kept from resolve_config
TEST_USAGE = ("usage: python -m deflow_amd.eval checkpoint=<ckpt> av2_mode=test dataset_path=<root> [leaderboard_version=1|2] [test_data=<dir>] "
              "[output=<zip>] [ground_source=auto|file|sidecar|online] [batch_size=] [num_workers=] [inference_dtype=fp32|bf16]")


def parse_test_args(argv: List[str]) -> Dict[str, Any]:
    """The key=value arguments of ``av2_mode=test`` -> checkpoint, version, test_dir (None when neither ``test_data=`` nor
    ``dataset_path=`` names one: the reference reads its configuration's default there, this command then stops), output, ground_source,
    inference_dtype, and under ``_given`` ({key: "key=value"}) everything ``resolve_config`` lays over the checkpoint's configuration.
    Needs no GPU and reads no file."""
    from .save import GROUND_SOURCES
    given: Dict[str, str] = {}
    for a in argv:
        if "=" not in a:
            raise SystemExit(f"expected key=value, got {a!r}")
        given[a.split("=", 1)[0].lstrip("+")] = a
    val = lambda k, default=None: given[k].split("=", 1)[1] if k in given else default
    if val("av2_mode") != "test":
        raise SystemExit(TEST_USAGE)
    if not val("checkpoint"):
        raise SystemExit(TEST_USAGE)
    opt: Dict[str, Any] = {"checkpoint": val("checkpoint"), "ground_source": val("ground_source", "auto"), "inference_dtype": val("inference_dtype")}
    if val("leaderboard_version", "1") not in ("1", "2"):
        raise SystemExit("leaderboard_version must be 1 (flow and is_dynamic) or 2 (is_valid and flow)")
    opt["version"] = int(val("leaderboard_version", "1"))
    if opt["ground_source"] not in GROUND_SOURCES:
        raise SystemExit(f"bad value for ground_source: {opt['ground_source']!r} ({', '.join(GROUND_SOURCES)})")
    if opt["inference_dtype"] not in (None, "fp32", "bf16"):
        raise SystemExit(f"bad value for inference_dtype: {opt['inference_dtype']!r} (fp32, bf16)")
    for k, low in (("batch_size", 1), ("num_workers", 0)):
        if k in given:
            try:
                ok = int(val(k)) >= low
            except ValueError:
                ok = False
            if not ok:
                raise SystemExit(f"bad value for {k}: {val(k)!r}")
    for k in ("test_data", "dataset_path", "output"):
        if k in given and not val(k):
            raise SystemExit(f"bad value for {k}: {val(k)!r}")
    opt["test_dir"] = val("test_data") or (os.path.join(val("dataset_path"), "test") if "dataset_path" in given else None)
    stem = os.path.splitext(os.path.basename(opt["checkpoint"]))[0]
    opt["output"] = val("output") or os.path.join(os.path.dirname(opt["checkpoint"]), f"{stem}.av2_submit_v{opt['version']}.zip")
    opt["_given"] = given
    return opt


def main_test(argv: List[str]) -> Dict[str, Any]:
    opt = parse_test_args(argv)
    if not opt["test_dir"]:
        raise SystemExit("av2_mode=test needs the data: dataset_path=<root> (reads <root>/test) or test_data=<dir>\n" + TEST_USAGE)
    assert torch.cuda.is_available(), "the submission is computed on the HIP engine only"
    from torch.utils.data import DataLoader
    from .feather import body_len, feather_file
    from .save import _Pinned
    from .submit import SubmissionZip, SubmitFlow, collate_submit_pad, submission_frames
    path, version, online = opt["checkpoint"], opt["version"], opt["ground_source"] == "online"
    cfg = resolve_config(path, opt["_given"], skip=TEST_OWN_KEYS)
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    model = build_model(cfg).to(dev)
    res = model.load_from_checkpoint(path)
    if res.missing_keys or res.unexpected_keys:
        print(f"[deflow_amd.eval] WARNING: checkpoint / model mismatch (model={cfg['model']}): {len(res.missing_keys)} missing keys "
              f"{res.missing_keys[:4]}..., {len(res.unexpected_keys)} unexpected keys {res.unexpected_keys[:4]}...", file=sys.stderr)
    model.eval()
    if opt["inference_dtype"]:
        model.inference_dtype = opt["inference_dtype"]
    frames, skipped = submission_frames(opt["test_dir"], opt["ground_source"])
    flows: Dict[int, SubmitFlow] = {}

    def submit_flow_for(B: int) -> SubmitFlow:           # a ground segmenter belongs to one batch size
        if B not in flows:
            ground = None
            if online:
                from .ground import GroundSegmenter
                ground = GroundSegmenter(B, device=dev)
            flows[B] = SubmitFlow(model, ground=ground)
        return flows[B]

    pinned = _Pinned()
    rows = 0
    out = os.path.abspath(opt["output"])
    with SubmissionZip(out) as zf:
        loader = DataLoader(frames, batch_size=int(cfg["batch_size"]), shuffle=False, collate_fn=collate_submit_pad,
                            num_workers=max(0, int(cfg["num_workers"])), pin_memory=True, drop_last=False) if len(frames) else ()
        for host in loader:
            d = {k: v.to(dev, non_blocking=True) for k, v in host.items() if isinstance(v, torch.Tensor)}
            body, kept = submit_flow_for(len(host["timestamp"])).infer(
                d["raw0"], d["n0"], None if online else d["drop0"], d["raw1"], d["n1"], None if online else d["drop1"], d["pose0"], d["pose1"],
                d["eval0"], ego_motion=d.get("ego_motion"), version=version)
            hb, hk = pinned.like("body", body), pinned.like("kept", kept)
            hb.copy_(body, non_blocking=True)
            hk.copy_(kept, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            hbn = hb.numpy()
            for i, (sid, ts, M) in enumerate(zip(host["scene_id"], host["timestamp"], hk.tolist())):      # hk is on the host
                zf.add(sid, ts, feather_file(version, M, hbn[i, : body_len(M, version)]))
                rows += M
        members = zf.members
    result = {"zip": out, "frames": members, "rows": rows, "skipped": skipped, "leaderboard_version": version, "checkpoint": path,
              "model": cfg["model"], "test_data": opt["test_dir"]}
    print(f"[deflow_amd.eval] submission of {members} frames written: upload {out} to the Argoverse-2 scene flow leaderboard "
          f"(version {version})", file=sys.stderr, flush=True)
    print(json.dumps(result), flush=True)
    return result


def main(argv=None, wrap=None):
    # wrap: optional callable (model, None) -> model, applied to the finished model before the first batch (python -m deflow_amd.refine
    # eval passes one); without it the command is what it was
    # metrics_impl=host|device: where the metrics are accumulated; not a hyper-parameter, taken off before parse_overrides
    metrics_impl, args = split_metrics_impl(list(sys.argv[1:] if argv is None else argv))
    pose_source, args = split_pose_source(args)      # where poses are read (HDF5Dataset(pose_source=...)); not a hyper-parameter either
    given = {a.split("=", 1)[0].lstrip("+"): a for a in args if "=" in a}
    pair = pairflow.selected(given)         # a checkpoint-free pair model (deflow_amd/pairflow.py), or None
    if pair and given.get("av2_mode", "av2_mode=val") == "av2_mode=test":
        raise SystemExit(f"model={pair.name} writes no leaderboard submission (av2_mode=test is out of its scope): av2_mode=val prints its "
                         f"metrics, python -m deflow_amd.save model={pair.name} writes its flow")
    wrong = pairflow.foreign_keys(given, pair)
    if wrong:
        raise SystemExit(wrong[1])
    if given.get("av2_mode", "av2_mode=val") == "av2_mode=test":
        return main_test(args)          # the leaderboard submission: no metrics (the test split has no labels)
    if given.get("av2_mode", "av2_mode=val") != "av2_mode=val":
        raise SystemExit(f"unknown {given['av2_mode']} (val: the metrics, test: the leaderboard submission)")
    if pair:
        (cfg, pair_params), path = pairflow.config(pair, given), None
    elif "checkpoint" not in given:
        raise SystemExit("usage: python -m deflow_amd.eval checkpoint=<path> [av2_mode=val] [val_data=<dir>|synthetic]\n" + TEST_USAGE + "".join(
            f"\n       python -m deflow_amd.eval model={e.name} [av2_mode=val] [val_data=<dir>|synthetic] [{e.prefix}_*=]" for e in pairflow.TABLE))
    else:
        path = given["checkpoint"].split("=", 1)[1]
        cfg = resolve_config(path, given, skip=("leaderboard_version", "inference_dtype"))
    if not any(k in given for k in DATA_KEYS):
        print("[deflow_amd.eval] NOTE: no dataset_path= / val_data= given -- evaluating on seeded SYNTHETIC pairs, not on a "
              "dataset (the reference reads its config's dataset_path default here)", file=sys.stderr)
    elif cfg["val_data"] == "synthetic" and given.get("val_data") != "val_data=synthetic":
        raise SystemExit("a data key was given but no validation directory resulted from it; refusing to fall back to synthetic data")
    assert torch.cuda.is_available(), "evaluation runs on the HIP engine only"
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    from .metrics import OfficialMetrics, evaluate_batch
    version = int(given.get("leaderboard_version", "leaderboard_version=1").split("=", 1)[1])
    if version not in (1, 2):
        raise SystemExit("leaderboard_version must be 1 (three-way EPE) or 2 (bucketed normalised EPE)")
    if metrics_impl == "device":      # the same tables and summary accumulated on the GPU, no host sync per batch (metrics_device.py)
        from .metrics_device import DeviceMetrics, evaluate_batch_device
        official = DeviceMetrics(dev)
    else:
        official = OfficialMetrics()
    if pair:
        model = pairflow.build(pair, cfg, pair_params)
    else:
        model = build_model(cfg).to(dev)
        res = model.load_from_checkpoint(path)
        if res.missing_keys or res.unexpected_keys:   # strict=False as the reference loads [REF deflow.py:47] -- but never silently
            print(f"[deflow_amd.eval] WARNING: checkpoint / model mismatch (model={cfg['model']}): {len(res.missing_keys)} missing keys "
                  f"{res.missing_keys[:4]}..., {len(res.unexpected_keys)} unexpected keys {res.unexpected_keys[:4]}...", file=sys.stderr)
        model.eval()
        if "inference_dtype" in given:
            model.inference_dtype = given["inference_dtype"].split("=", 1)[1]
    if wrap is not None:
        model = wrap(model, None)
    B = int(cfg["batch_size"])
    if cfg["val_data"] != "synthetic":
        from .data import HDF5Dataset, SceneLoader, ShardedSampler
        ds = HDF5Dataset(str(cfg["val_data"]), eval=True, pose_source=pose_source)      # index_eval.pkl (the benchmark's frames) when the directory has one
        batches = SceneLoader(ds, B, ShardedSampler(len(ds), shuffle=False), device=dev,
                              num_workers=max(0, int(cfg["num_workers"])), drop_last=False)
    else:
        from .synth import synth_batch
        H = grid_from(cfg)[0]
        batches = (synth_batch(B, int(cfg["points_per_cloud"]), seed=int(cfg["seed"]) + 10 ** 6 + i * B, grid_hw=(H, H), device=dev)
                   for i in range(max(1, int(cfg["pairs_per_epoch"]) // B)))
    tot, wsum = {}, {}
    with torch.no_grad():
        for batch in batches:
            if metrics_impl == "device":
                evaluate_batch_device(model, batch, official)
                continue
            m = evaluate_batch(model(batch), batch, official)
            w = len(batch["pose0"])
            for k, v in m.items():
                tot[k] = tot.get(k, 0.0) + v * w
                wsum[k] = wsum.get(k, 0) + w
    out = official.summary() if metrics_impl == "device" else {k: tot[k] / wsum[k] for k in tot}
    # the leaderboard table the reference prints at the end of validation [REF README.md:88-91]: leaderboard_version=1 the three-way
    # EPE (+ IoU, accuracies, angle error inside the 35 m box), leaderboard_version=2 the bucketed normalised EPE
    board = official.result(version)
    print(official.table(version), file=sys.stderr, flush=True)
    print(json.dumps({"checkpoint": path, "model": cfg["model"], "val_data": cfg["val_data"], "metrics": out,
                      "leaderboard_version": version, "leaderboard": board}), flush=True)
    out = dict(out)
    out["leaderboard"] = board
    return out


if __name__ == "__main__":
    main()
