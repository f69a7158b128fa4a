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
auto|file|sidecar|online``, ``batch_size=``, ``num_workers=`` and ``inference_dtype=`` as in ``deflow_amd.save``."""
from __future__ import annotations

import json
import os
import sys
from typing import Any, Dict, List

import torch

from .train import DATA_KEYS, DEFAULTS, _TARGET_ALIASES, build_model, grid_from, parse_overrides, split_metrics_impl


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


def icpflow_config(given: Dict[str, str]):
    """``model=icpflow``: (configuration, rigid parameters) from the command line alone -- the defaults of deflow_amd.train under the keys
    as typed ({key: "key=value"}), the ``icp_*`` keys validated by deflow_amd.rigid.  Needs no GPU and reads no file."""
    from .rigid import COMMAND_KEYS, params_from_command
    for k in ("checkpoint", "inference_dtype"):
        if k in given:
            raise SystemExit(f"model=icpflow has no weights: it takes no {k}=")
    icp = {k: a.split("=", 1)[1] for k, a in given.items() if k in COMMAND_KEYS}
    cfg = parse_overrides([a for k, a in given.items() if k not in COMMAND_KEYS and k != "model"])
    cfg["model"] = "icpflow"
    return cfg, params_from_command(icp)


def nsfp_config(given: Dict[str, str]):
    """``model=nsfp``: (configuration, nsfp parameters) from the command line alone, as ``icpflow_config``; batch_size defaults to
    nsfp.COMMAND_BATCH_SIZE.  ``icp_*`` keys are refused.  Needs no GPU and reads no file."""
    from . import nsfp, rigid
    for k in ("checkpoint", "inference_dtype"):
        if k in given:
            raise SystemExit(f"model=nsfp has no weights: it takes no {k}=")
    wrong = sorted(k for k in given if k in rigid.COMMAND_KEYS)
    if wrong:
        raise SystemExit(f"{', '.join(wrong)}: the icp_* keys belong to model=icpflow")
    own = {k: a.split("=", 1)[1] for k, a in given.items() if k in nsfp.COMMAND_KEYS}
    cfg = parse_overrides([a for k, a in given.items() if k not in nsfp.COMMAND_KEYS and k != "model"])
    cfg["model"] = "nsfp"
    if "batch_size" not in given:
        cfg["batch_size"] = nsfp.COMMAND_BATCH_SIZE
    return cfg, nsfp.params_from_command(own)


def fastnsf_config(given: Dict[str, str]):
    """``model=fastnsf``: (configuration, fastnsf parameters) from the command line alone, as ``nsfp_config``; batch_size defaults to
    fastnsf.COMMAND_BATCH_SIZE.  ``icp_*`` and ``nsfp_*`` keys are refused.  Needs no GPU and reads no file."""
    from . import fastnsf, nsfp, rigid
    for k in ("checkpoint", "inference_dtype"):
        if k in given:
            raise SystemExit(f"model=fastnsf has no weights: it takes no {k}=")
    wrong = sorted(k for k in given if k in rigid.COMMAND_KEYS)
    if wrong:
        raise SystemExit(f"{', '.join(wrong)}: the icp_* keys belong to model=icpflow")
    wrong = sorted(k for k in given if k in nsfp.COMMAND_KEYS)
    if wrong:
        raise SystemExit(f"{', '.join(wrong)}: the nsfp_* keys belong to model=nsfp")
    own = {k: a.split("=", 1)[1] for k, a in given.items() if k in fastnsf.COMMAND_KEYS}
    cfg = parse_overrides([a for k, a in given.items() if k not in fastnsf.COMMAND_KEYS and k != "model"])
    cfg["model"] = "fastnsf"
    if "batch_size" not in given:
        cfg["batch_size"] = fastnsf.COMMAND_BATCH_SIZE
    return cfg, fastnsf.params_from_command(own)


def mbnsf_config(given: Dict[str, str]):
    """``model=mbnsf``: (configuration, mbnsf parameters) from the command line alone, as ``fastnsf_config``; batch_size defaults to
    mbnsf.COMMAND_BATCH_SIZE.  ``icp_*``, ``nsfp_*`` and ``fastnsf_*`` keys are refused.  Needs no GPU and reads no file."""
    from . import fastnsf, mbnsf, nsfp, rigid
    for k in ("checkpoint", "inference_dtype"):
        if k in given:
            raise SystemExit(f"model=mbnsf has no weights: it takes no {k}=")
    for keys, owner in ((rigid.COMMAND_KEYS, "icpflow"), (nsfp.COMMAND_KEYS, "nsfp"), (fastnsf.COMMAND_KEYS, "fastnsf")):
        wrong = sorted(k for k in given if k in keys)
        if wrong:
            raise SystemExit(f"{', '.join(wrong)}: the {'icp' if owner == 'icpflow' else owner}_* keys belong to model={owner}")
    own = {k: a.split("=", 1)[1] for k, a in given.items() if k in mbnsf.COMMAND_KEYS}
    cfg = parse_overrides([a for k, a in given.items() if k not in mbnsf.COMMAND_KEYS and k != "model"])
    cfg["model"] = "mbnsf"
    if "batch_size" not in given:
        cfg["batch_size"] = mbnsf.COMMAND_BATCH_SIZE
    return cfg, mbnsf.params_from_command(own)


def floxels_config(given: Dict[str, str]):
    """``model=floxels``: (configuration, floxels parameters) from the command line alone, as ``mbnsf_config``; batch_size defaults to
    floxels.COMMAND_BATCH_SIZE.  ``icp_*``, ``nsfp_*``, ``fastnsf_*`` and ``mbnsf_*`` keys are refused.  Needs no GPU and reads no file."""
    from . import fastnsf, floxels, mbnsf, nsfp, rigid
    for k in ("checkpoint", "inference_dtype"):
        if k in given:
            raise SystemExit(f"model=floxels has no weights: it takes no {k}=")
    for keys, owner in ((rigid.COMMAND_KEYS, "icpflow"), (nsfp.COMMAND_KEYS, "nsfp"), (fastnsf.COMMAND_KEYS, "fastnsf"),
                        (mbnsf.COMMAND_KEYS, "mbnsf")):
        wrong = sorted(k for k in given if k in keys)
        if wrong:
            raise SystemExit(f"{', '.join(wrong)}: the {'icp' if owner == 'icpflow' else owner}_* keys belong to model={owner}")
    own = {k: a.split("=", 1)[1] for k, a in given.items() if k in floxels.COMMAND_KEYS}
    cfg = parse_overrides([a for k, a in given.items() if k not in floxels.COMMAND_KEYS and k != "model"])
    cfg["model"] = "floxels"
    if "batch_size" not in given:
        cfg["batch_size"] = floxels.COMMAND_BATCH_SIZE
    return cfg, floxels.params_from_command(own)


def main(argv=None):
    # metrics_impl=host|device: where the metrics are accumulated; not a hyper-parameter, taken off before parse_overrides
    metrics_impl, args = split_metrics_impl(list(sys.argv[1:] if argv is None else argv))
    given = {a.split("=", 1)[0].lstrip("+"): a for a in args if "=" in a}
    is_floxels = given.get("model") == "model=floxels"
    if is_floxels and given.get("av2_mode", "av2_mode=val") == "av2_mode=test":
        raise SystemExit("model=floxels writes no leaderboard submission (av2_mode=test is out of its scope): av2_mode=val prints its "
                         "metrics, python -m deflow_amd.save model=floxels writes its flow")
    if not is_floxels:
        from .floxels import COMMAND_KEYS as FLOXELS_KEYS
        wrong = sorted(k for k in given if k in FLOXELS_KEYS)
        if wrong:
            raise SystemExit(f"{', '.join(wrong)}: the floxels_* keys belong to model=floxels")
    is_mbnsf = given.get("model") == "model=mbnsf"
    if is_mbnsf and given.get("av2_mode", "av2_mode=val") == "av2_mode=test":
        raise SystemExit("model=mbnsf writes no leaderboard submission (av2_mode=test is out of its scope): av2_mode=val prints its "
                         "metrics, python -m deflow_amd.save model=mbnsf writes its flow")
    if not is_mbnsf:
        from .mbnsf import COMMAND_KEYS as MBNSF_KEYS
        wrong = sorted(k for k in given if k in MBNSF_KEYS)
        if wrong:
            raise SystemExit(f"{', '.join(wrong)}: the mbnsf_* keys belong to model=mbnsf")
    icpflow = given.get("model") == "model=icpflow"
    if icpflow and given.get("av2_mode", "av2_mode=val") == "av2_mode=test":
        raise SystemExit("model=icpflow writes no leaderboard submission (av2_mode=test is out of its scope): av2_mode=val prints its "
                         "metrics, python -m deflow_amd.save model=icpflow writes its flow")
    is_nsfp = given.get("model") == "model=nsfp"
    if is_nsfp and given.get("av2_mode", "av2_mode=val") == "av2_mode=test":
        raise SystemExit("model=nsfp writes no leaderboard submission (av2_mode=test is out of its scope): av2_mode=val prints its "
                         "metrics, python -m deflow_amd.save model=nsfp writes its flow")
    is_fastnsf = given.get("model") == "model=fastnsf"
    if is_fastnsf and given.get("av2_mode", "av2_mode=val") == "av2_mode=test":
        raise SystemExit("model=fastnsf writes no leaderboard submission (av2_mode=test is out of its scope): av2_mode=val prints its "
                         "metrics, python -m deflow_amd.save model=fastnsf writes its flow")
    if not is_fastnsf:
        from .fastnsf import COMMAND_KEYS as FASTNSF_KEYS
        wrong = sorted(k for k in given if k in FASTNSF_KEYS)
        if wrong:
            raise SystemExit(f"{', '.join(wrong)}: the fastnsf_* keys belong to model=fastnsf")
    if not is_nsfp and not icpflow and not is_fastnsf:
        from .nsfp import COMMAND_KEYS as NSFP_KEYS
        wrong = sorted(k for k in given if k in NSFP_KEYS)
        if wrong:
            raise SystemExit(f"{', '.join(wrong)}: the nsfp_* keys belong to model=nsfp")
    if given.get("av2_mode", "av2_mode=val") == "av2_mode=test":
        return main_test(args)          # the leaderboard submission: no metrics (the test split has no labels)
    if given.get("av2_mode", "av2_mode=val") != "av2_mode=val":
        raise SystemExit(f"unknown {given['av2_mode']} (val: the metrics, test: the leaderboard submission)")
    if icpflow:
        (cfg, icp_params), path = icpflow_config(given), None
    elif is_nsfp:
        (cfg, nsfp_params), path = nsfp_config(given), None
    elif is_fastnsf:
        (cfg, fastnsf_params), path = fastnsf_config(given), None
    elif is_mbnsf:
        (cfg, mbnsf_params), path = mbnsf_config(given), None
    elif is_floxels:
        (cfg, floxels_params), path = floxels_config(given), None
    elif "checkpoint" not in given:
        raise SystemExit("usage: python -m deflow_amd.eval checkpoint=<path> [av2_mode=val] [val_data=<dir>|synthetic]\n" + TEST_USAGE +
                         "\n       python -m deflow_amd.eval model=icpflow [av2_mode=val] [val_data=<dir>|synthetic] [icp_*=]"
                         "\n       python -m deflow_amd.eval model=nsfp [av2_mode=val] [val_data=<dir>|synthetic] [nsfp_*=]"
                         "\n       python -m deflow_amd.eval model=fastnsf [av2_mode=val] [val_data=<dir>|synthetic] [fastnsf_*=]"
                         "\n       python -m deflow_amd.eval model=mbnsf [av2_mode=val] [val_data=<dir>|synthetic] [mbnsf_*=]"
                         "\n       python -m deflow_amd.eval model=floxels [av2_mode=val] [val_data=<dir>|synthetic] [floxels_*=]")
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
    if icpflow:
        from .rigid import IcpFlow
        model = IcpFlow(point_cloud_range=cfg["point_cloud_range"], voxel_size=cfg["voxel_size"], **icp_params)
    elif is_nsfp:
        from .nsfp import Nsfp
        model = Nsfp(point_cloud_range=cfg["point_cloud_range"], voxel_size=cfg["voxel_size"], **nsfp_params)
    elif is_fastnsf:
        from .fastnsf import FastNsf
        model = FastNsf(point_cloud_range=cfg["point_cloud_range"], voxel_size=cfg["voxel_size"], **fastnsf_params)
    elif is_mbnsf:
        from .mbnsf import MbNsf
        model = MbNsf(point_cloud_range=cfg["point_cloud_range"], voxel_size=cfg["voxel_size"], **mbnsf_params)
    elif is_floxels:
        from .floxels import Floxels
        model = Floxels(point_cloud_range=cfg["point_cloud_range"], voxel_size=cfg["voxel_size"], **floxels_params)
    else:
        model = build_model(cfg).to(dev)
        res = model.load_from_checkpoint(path)
        if res.missing_keys or res.unexpected_keys:   # strict=False as the reference loads [REF deflow.py:47] -- but never silently
            print(f"[deflow_amd.eval] WARNING: checkpoint / model mismatch (model={cfg['model']}): {len(res.missing_keys)} missing keys "
                  f"{res.missing_keys[:4]}..., {len(res.unexpected_keys)} unexpected keys {res.unexpected_keys[:4]}...", file=sys.stderr)
        model.eval()
        if "inference_dtype" in given:
            model.inference_dtype = given["inference_dtype"].split("=", 1)[1]
    B = int(cfg["batch_size"])
    if cfg["val_data"] != "synthetic":
        from .data import HDF5Dataset, SceneLoader, ShardedSampler
        ds = HDF5Dataset(str(cfg["val_data"]), eval=True)      # index_eval.pkl (the benchmark's frames) when the directory has one
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
