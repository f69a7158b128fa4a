"""No GPU: the table of checkpoint-free pair models (deflow_amd/pairflow.py) as the eval and save commands use it --
every model refuses every other model's keys in both commands, the defaults, the generated usage text, the flow file's meta and the
texts of the shared parameter checks."""
import ast
import os
import re
import shutil

import numpy as np
import pytest
import torch

from deflow_amd import pairflow

NAMES = [e.name for e in pairflow.TABLE]


def test_table():
    assert NAMES == ["icpflow", "nsfp", "fastnsf", "mbnsf", "floxels"]
    assert [e.prefix for e in pairflow.TABLE] == ["icp", "nsfp", "fastnsf", "mbnsf", "floxels"]
    assert [e.section for e in pairflow.TABLE] == ["6j", "6k", "6l", "6m", "6n"]
    for e in pairflow.TABLE:
        m = pairflow.module(e)
        assert pairflow.entry(e.name) is e and issubclass(getattr(m, e.cls), pairflow.PairFlowModel)
        assert all(k.startswith(e.prefix + "_") and pairflow.owner(k) is e for k in m.COMMAND_KEYS)
        assert list(m.COMMAND_KEYS.values()) == list(m.DEFAULTS)
        assert pairflow.selected({"model": f"model={e.name}"}) is e and pairflow.selected({"model.name": f"model.name={e.name}"}) is None
        assert pairflow.selected({"model.name": f"model.name={e.name}"}, keys=("model", "model.name")) is e
    assert pairflow.entry("deflow") is None and pairflow.entry(None) is None and pairflow.owner("lr") is None
    assert pairflow.selected({"model": "model=fastflow3d"}) is None and pairflow.selected({}) is None
    from deflow_amd import rigid
    assert rigid.PairFlowModel is pairflow.PairFlowModel and rigid.COMMAND_BATCH_SIZE is None


# ---- every model refuses every other model's keys, in both commands ---------------------------------------------------------------------
@pytest.mark.parametrize("model,foreign", [(m, f) for m in NAMES + [None] for f in NAMES if m != f])      # (None: a checkpoint's model)
def test_foreign_keys_are_refused_by_both_commands(model, foreign):
    from deflow_amd import eval as ev, save
    f = pairflow.entry(foreign)
    head = [f"model={model}"] if model else ["checkpoint=a.ckpt"]
    what = f"the {f.prefix}_\\* keys belong to model={f.name}"
    for key in (next(iter(pairflow.module(f).COMMAND_KEYS)), f.prefix + "_iters"):
        with pytest.raises(SystemExit, match=f"{key}: {what}"):
            ev.main(head + [f"{key}=3"])
        with pytest.raises(SystemExit, match=f"{key}: {what}"):
            save.parse_args(head + ["dataset_path=/d", f"{key}=3"])
    assert pairflow.foreign_keys([f.prefix + "_iters"], pairflow.entry(model))[0] is f
    assert pairflow.foreign_keys([f.prefix + "_iters"], f) is None and pairflow.foreign_keys(["lr", "batch_size"], None) is None


def test_the_first_foreign_family_in_table_order_is_named():
    given = ["floxels_iters", "nsfp_lr", "nsfp_iters", "icp_iters"]
    nsfp = pairflow.entry("nsfp")
    assert pairflow.foreign_keys(given, pairflow.entry("icpflow")) == (nsfp, "nsfp_iters, nsfp_lr: the nsfp_* keys belong to model=nsfp")
    assert pairflow.foreign_keys(given, None)[1] == "icp_iters: the icp_* keys belong to model=icpflow"


# ---- defaults ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_defaults_of_both_commands(name):
    from deflow_amd import save, train
    e = pairflow.entry(name)
    m = pairflow.module(e)
    assert (m.COMMAND_BATCH_SIZE is None) == (name == "icpflow")
    batch = train.DEFAULTS["batch_size"] if m.COMMAND_BATCH_SIZE is None else m.COMMAND_BATCH_SIZE
    cfg, params = pairflow.config(e, {"model": f"model={name}", "dataset_path": "dataset_path=/r"})
    assert params == m.DEFAULTS and cfg["model"] == name and cfg["batch_size"] == batch and cfg["val_data"] == os.path.join("/r", "val")
    assert pairflow.config(e, {"model": f"model={name}", "batch_size": "batch_size=5"})[0]["batch_size"] == 5
    for k in ("checkpoint", "inference_dtype"):
        with pytest.raises(SystemExit, match=f"model={name} has no weights: it takes no {k}="):
            pairflow.config(e, {"model": f"model={name}", k: f"{k}=x"})
    opt = save.parse_args([f"model={name}", "dataset_path=/d"])
    assert opt["model"] == name and opt["res_name"] == name and opt["params"] == m.DEFAULTS and opt["checkpoint"] is None
    assert opt["_rest"] == ({} if name == "icpflow" else {"batch_size": f"batch_size={m.COMMAND_BATCH_SIZE}"})
    assert save.parse_args([f"model.name={name}", "dataset_path=/d", "batch_size=5"])["_rest"] == {"batch_size": "batch_size=5"}
    with pytest.raises(SystemExit, match=f"model={name} has no weights: it takes neither checkpoint= nor inference_dtype=\nusage: .* model={name} "):
        save.parse_args([f"model={name}", "dataset_path=/d", "checkpoint=a.ckpt"])
    first = next(iter(m.COMMAND_KEYS))
    with pytest.raises(SystemExit, match=f"bad value for {first}: 'many'"):
        save.parse_args([f"model={name}", "dataset_path=/d", f"{first}=many"])
    # true / false are Python's only for a model that has a flag: icp_eps=true is no eps = 1.0
    with pytest.raises(SystemExit, match=f"bad value for {first}: 'true'" if name == "icpflow" else f"bad value among the {e.prefix}_\\* keys"):
        m.params_from_command({first: "true"})


# ---- the usage text ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_usage(name):
    from deflow_amd import save
    e = pairflow.entry(name)
    m = pairflow.module(e)
    text = pairflow.usage(e)
    assert text.startswith(f"usage: python -m deflow_amd.save model={name} dataset_path=")
    for k in m.COMMAND_KEYS:
        assert text.count(f"[{k}=") == 1, k
    shown = re.findall(r"\[(\w+)=([^\]]*)\]", text)
    own = [(k, v) for k, v in shown if k in m.COMMAND_KEYS]
    assert [k for k, _ in own] == list(m.COMMAND_KEYS)                                    # in the module's order
    for k, v in own:                                                                      # every default shown is the module's
        assert ast.literal_eval(v.capitalize() if v in ("true", "false") else v) == m.DEFAULTS[m.COMMAND_KEYS[k]], k
    assert dict(shown)["res_name"] == name and dict(shown)["batch_size"] == ("" if m.COMMAND_BATCH_SIZE is None else str(m.COMMAND_BATCH_SIZE))
    assert [k for k, _ in shown if k not in m.COMMAND_KEYS] == ["res_name", "scenes", "batch_size", "num_workers", "ground_source", "half",
                                                                "overwrite", "voxel_size", "point_cloud_range"]
    if m.COMMAND_BATCH_SIZE is None:
        assert "\n" not in text and e.memory == ""
    else:
        head, note = text.split("\n")
        assert note == e.memory and note.startswith(f"batch_size defaults to {m.COMMAND_BATCH_SIZE}: ")
    with pytest.raises(SystemExit) as err:                                                # no dataset_path: the usage text and nothing else
        save.parse_args([f"model={name}"])
    assert str(err.value) == text


# ---- the flow file's meta ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,letter", list(zip(NAMES, "jklmn")))
def test_meta_of_a_saved_file(name, letter, tmp_path, golden_dir, monkeypatch):
    from deflow_amd import save
    e = pairflow.entry(name)
    m = pairflow.module(e)
    shutil.copy(os.path.join(golden_dir, "av2_mini", "train", "scene_a.h5"), tmp_path / "scene_a.h5")     # never written under tests/golden
    built = []

    class Stub:                                           # nothing launches: the model is its parameters, the scene's flow is made up
        def __init__(self, point_cloud_range, voxel_size, **params):
            self.params = m.check_params(params)
            built.append((point_cloud_range, voxel_size))

    def scene(sweep_flow_for, pairs, batch_size, device, **kw):
        built.append(batch_size)
        return {ts: (np.zeros((2, 3), np.float32), np.zeros(2, np.uint8)) for ts in pairs.sweeps[:-1]}

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(m, e.cls, Stub)
    monkeypatch.setattr(save, "save_scene", scene)
    assert save.main([f"model={name}", f"dataset_path={tmp_path}", "scenes=scene_a", "voxel_size=[0.4,0.4,6]"]) == 0
    from deflow_amd import train
    assert built == [(train.DEFAULTS["point_cloud_range"], [0.4, 0.4, 6]), m.COMMAND_BATCH_SIZE or train.DEFAULTS["batch_size"]]
    meta = save.read_meta(save.flow_path(str(tmp_path), "scene_a", name))
    assert meta == {"res_name": name, "checkpoint": None, "model": name, "voxel_size": [0.4, 0.4, 6.0],
                    "point_cloud_range": [float(v) for v in train.DEFAULTS["point_cloud_range"]], "ground_source": "auto", "half": False,
                    "params": m.DEFAULTS, "definition": f"DESIGN.md 6f, 6{letter} (UNPINNED)"}
    assert len(save.read_flow(save.flow_path(str(tmp_path), "scene_a", name))) >= 1


# ---- the texts of the parameter checks ---------------------------------------------------------------------------------------------------
# recorded from the modules' own check_params before they shared pairflow's checks: one bad value per kind of check and module (a
# non-integer, an integer out of range, a value that is not positive, a negative one, a graph that is no bool, a trunc that is no whole
# number of cells), then values that are no finite numbers, which mbnsf's own keys and floxels report differently from nsfp and fastnsf
MESSAGES = {
    "nsfp": [({"depth": 1.5}, "nsfp_optimize: depth must be an integer in [0, 15], got 1.5"),
             ({"depth": 16}, "nsfp_optimize: depth must be an integer in [0, 15], got 16"),
             ({"lr": 0}, "nsfp_optimize: lr must be positive and finite, got 0"),
             ({"min_delta": -1e-3}, "nsfp_optimize: min_delta must be finite and >= 0, got -0.001"),
             ({"graph": 1}, "nsfp_optimize: graph must be True or False, got 1"),
             ({"depth": True}, "nsfp_optimize: depth must be an integer in [0, 15], got True"),
             ({"lr": float("nan")}, "nsfp_optimize: lr must be positive and finite, got nan"),
             ({"lr": "x"}, "nsfp_optimize: lr must be positive and finite, got 'x'"),
             ({"min_delta": float("inf")}, "nsfp_optimize: min_delta must be finite and >= 0, got inf"),
             ({"width": 3}, "nsfp_optimize: unknown parameter 'width'; known: check_every, depth, graph, iters, lr, min_delta, patience, seed, "
                            "trunc_d2")],
    "fastnsf": [({"depth": 1.5}, "fastnsf_optimize: depth must be an integer in [0, 15], got 1.5"),
                ({"depth": 16}, "fastnsf_optimize: depth must be an integer in [0, 15], got 16"),
                ({"lr": 0}, "fastnsf_optimize: lr must be positive and finite, got 0"),
                ({"min_delta": -1e-3}, "fastnsf_optimize: min_delta must be finite and >= 0, got -0.001"),
                ({"graph": 1}, "fastnsf_optimize: graph must be True or False, got 1"),
                ({"cell": 0.3}, "fastnsf_optimize: trunc must be a whole number of cells, 1 to 255 of them, got trunc = 2.0, cell = 0.3"),
                ({"depth": True}, "fastnsf_optimize: depth must be an integer in [0, 15], got True"),
                ({"trunc": float("nan")}, "fastnsf_optimize: trunc must be positive and finite, got nan")],
    "mbnsf": [({"rigid_pairs": 2.5}, "mbnsf_optimize: rigid_pairs must be an integer in [1, 16], got 2.5"),
              ({"rigid_pairs": 17}, "mbnsf_optimize: rigid_pairs must be an integer in [1, 16], got 17"),
              ({"rigid_delta": 0.0}, "mbnsf_optimize: rigid_delta must be positive and finite, got 0.0"),
              ({"rigid_weight": -1.0}, "mbnsf_optimize: rigid_weight must be finite and >= 0, got -1.0"),
              ({"graph": 1}, "mbnsf_optimize: graph must be True or False, got 1"),
              ({"cell": 0.3}, "mbnsf_optimize: trunc must be a whole number of cells, 1 to 255 of them, got trunc = 2.0, cell = 0.3"),
              ({"depth": 1.5}, "mbnsf_optimize: depth must be an integer in [0, 15], got 1.5"),
              ({"depth": 16}, "mbnsf_optimize: depth must be an integer in [0, 15], got 16"),
              ({"lr": 0}, "mbnsf_optimize: lr must be positive and finite, got 0"),
              ({"min_delta": -1e-3}, "mbnsf_optimize: min_delta must be finite and >= 0, got -0.001"),
              ({"rigid_weight": True}, "mbnsf_optimize: rigid_weight must be a finite number, got True"),
              ({"rigid_weight": float("nan")}, "mbnsf_optimize: rigid_weight must be a finite number, got nan"),
              ({"rigid_pairs": True}, "mbnsf_optimize: rigid_pairs must be a finite number, got True"),
              ({"eps": float("inf")}, "mbnsf_optimize: eps must be a finite number, got inf")],
    "floxels": [({"iters": 2.5}, "floxels_optimize: iters must be an integer in [1, 1048576], got 2.5"),
                ({"iters": 0}, "floxels_optimize: iters must be an integer in [1, 1048576], got 0"),
                ({"voxel": 0}, "floxels_optimize: voxel must be positive and finite, got 0"),
                ({"smooth_weight": -1.0}, "floxels_optimize: smooth_weight must be finite and >= 0, got -1.0"),
                ({"graph": 1}, "floxels_optimize: graph must be True or False, got 1"),
                ({"cell": 0.3}, "floxels_optimize: trunc must be a whole number of cells, 1 to 255 of them, got trunc = 2.0, cell = 0.3"),
                ({"iters": True}, "floxels_optimize: iters must be a finite number, got True"),
                ({"voxel": float("nan")}, "floxels_optimize: voxel must be a finite number, got nan"),
                ({"min_delta": float("inf")}, "floxels_optimize: min_delta must be a finite number, got inf"),
                ({"depth": 1}, "floxels_optimize: unknown parameter 'depth'; known: cell, check_every, graph, iters, lr, min_delta, patience, "
                               "smooth_weight, trunc, voxel")],
    "icpflow": [({"min_points": 0}, "rigid_cluster_flow: min_points must be an integer in [1, 1073741824], got 0"),
                ({"eps": 0}, "rigid_cluster_flow: eps must be positive and finite, got 0"),
                ({"bins": 1}, "rigid_cluster_flow: unknown parameter 'bins'; known: eps, icp_cap, icp_iters, icp_max_dist, max_cluster_points, "
                              "max_disp, max_yaw, min_cluster_size, min_inlier_frac, min_points, min_side, vote_bin, vote_cap")],
}


@pytest.mark.parametrize("name", NAMES)
def test_check_params_messages_are_the_recorded_ones(name):
    e = pairflow.entry(name)
    m = pairflow.module(e)
    for bad, text in MESSAGES[name]:
        with pytest.raises(ValueError) as err:
            m.check_params(bad)
        assert str(err.value) == text, bad
        (k, v), = bad.items()
        if isinstance(v, (int, float)) and not isinstance(v, bool) and k in m.DEFAULTS and v == v and abs(v) != float("inf"):
            key = next(c for c, p in m.COMMAND_KEYS.items() if p == k)
            with pytest.raises(SystemExit) as err:                                        # the commands wrap the same text
                m.params_from_command({key: repr(v)})
            assert str(err.value) == f"bad value among the {e.prefix}_* keys: {text}"
    assert m.check_params({}) == m.DEFAULTS


# ---- the texts that name the caller -------------------------------------------------------------------------------------------------------
# recorded from the parent of the commit that gave dt_grid, vox_grid and fastnsf.check_params their fn= argument: until then mbnsf and
# floxels caught these errors and replaced the prefix in the text
R, BIG = (-51.2, -51.2, -3, 51.2, 51.2, 3), (-200, -200, -20, 200, 200, 20)
DT_GRID = [((R[:4], 0.1, 2.0), "grid_range must be 6 finite values (minx, miny, minz, maxx, maxy, maxz), got (-51.2, -51.2, -3, 51.2)"),
           ((R, 0, 2.0), "cell must be positive and finite, got 0"),
           ((R, 0.1, True), "trunc must be positive and finite, got True"),
           ((R, 0.3, 2.0), "trunc must be a whole number of cells, 1 to 255 of them, got trunc = 2.0, cell = 0.3"),
           (((0, 0, 0, 1, 1, 0), 0.1, 2.0), "grid_range is empty: (0, 0, 0, 1, 1, 0)"),
           ((BIG, 0.1, 2.0), "grid_range / cell: 4040 x 4040 x 440 voxels do not fit 31 bits")]
VOX_GRID = [((R[:4], 0.4), "grid_range must be 6 finite values (minx, miny, minz, maxx, maxy, maxz), got (-51.2, -51.2, -3, 51.2)"),
            ((R, -0.4), "voxel must be positive and finite, got -0.4"),
            (((0, 0, 0, 1, 1, 0), 0.4), "grid_range is empty: (0, 0, 0, 1, 1, 0)"),
            ((R, 1e-9), "grid_range / voxel: 1.02e+11 nodes on one axis do not fit 31 bits"),
            ((R, 0.01), "grid_range / voxel: 3 x 10241 x 10241 x 601 node components do not fit 31 bits")]
FASTNSF_AS_MBNSF = [({"seed": -1}, "mbnsf_optimize: seed must be an integer in [0, 9223372036854775807], got -1"),
                    ({"trunc": float("nan")}, "mbnsf_optimize: trunc must be positive and finite, got nan"),
                    ({"patience": 0}, "mbnsf_optimize: patience must be an integer in [1, 1073741824], got 0"),
                    ({"depth": 16}, "mbnsf_optimize: depth must be an integer in [0, 15], got 16")]


def _text(call, *args, **kw):
    with pytest.raises(ValueError) as err:
        call(*args, **kw)
    return str(err.value)


def test_messages_that_name_the_caller_are_the_recorded_ones():
    from deflow_amd import fastnsf, floxels, mbnsf
    for args, text in DT_GRID:
        assert _text(fastnsf.dt_grid, *args) == "dt_grid: " + text                       # fastnsf_optimize and FastNsf report it as dt_grid's
        for fn in ("mbnsf_optimize", "floxels_optimize", "Floxels"):
            assert _text(fastnsf.dt_grid, *args, fn=fn) == f"{fn}: {text}"
    for args, text in VOX_GRID:
        assert _text(floxels.vox_grid, *args) == "vox_grid: " + text
        for fn in ("floxels_optimize", "Floxels"):
            assert _text(floxels.vox_grid, *args, fn=fn) == f"{fn}: {text}"
    for bad, text in FASTNSF_AS_MBNSF:
        assert _text(mbnsf.check_params, bad) == text == _text(fastnsf.check_params, bad, fn="mbnsf_optimize")
        assert _text(fastnsf.check_params, bad) == text.replace("mbnsf_optimize:", "fastnsf_optimize:")
    # the models' constructors refuse a grid that does not fit with the same texts as before
    assert _text(fastnsf.FastNsf, point_cloud_range=BIG) == _text(mbnsf.MbNsf, point_cloud_range=BIG) == "dt_grid: " + DT_GRID[5][1]
    assert _text(floxels.Floxels, point_cloud_range=BIG) == "Floxels: " + DT_GRID[5][1]
    assert _text(floxels.Floxels, voxel=0.01) == "Floxels: " + VOX_GRID[4][1]
