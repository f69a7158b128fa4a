"""CPU: the numpy restatement of the whole-sweep flow (tests/helpers/sweep_flow_ref.py) on hand-made cases and
against collate_fn_pad on the scene fixtures, and the host side of ``python -m deflow_amd.save``: the raw collate, the argument parser and
the flow file."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sweep_flow_ref as SR  # noqa: E402

F = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


# ---- the definition on hand-made rows -----------------------------------------------------------------------------------------------------
def test_threshold_rows_are_exact():
    t = SR.threshold_flows()
    assert bits(SR.sq_norm(t["at"])) == bits(F(0.0025)) == 0x3B23D70A
    assert bits(SR.sq_norm(t["below"])) == 0x3B23D709 and bits(SR.sq_norm(t["above"])) == 0x3B23D70B
    # the sum stated exactly: (fl(fx fx) + fl(fy fy)) + fl(fz fz), every operation in fp32
    fx, fy, fz = t["at"]
    assert F(F(F(fx * fx) + F(fy * fy)) + F(fz * fz)) == F(0.0025)


def test_hand_made_sweep():
    t = SR.threshold_flows()
    T = np.eye(4, dtype=F)
    T[:3, 3] = (0.5, -0.25, 0.125)
    T[0, 1], T[1, 0] = -0.001, 0.001
    # rows: 0 decoded (below), 1 ground, 2 out of range (kept, not decoded), 3 NaN, 4 decoded (at), 5 decoded (above), 6 inf; 7.. padding
    raw = np.array([[1, 2, 0.5], [3, 4, -1.5], [80, 0, 0], [np.nan, 1, 1], [-2, 1, 0.25], [2.5, -1.5, 1], [1, np.inf, 0], [9, 9, 9],
                    [np.nan] * 3], dtype=F)
    count, drop = 7, np.array([0, 1, 0, 0, 0, 0, 0, 0, 0])
    pc, row_of, pos_of, kept = SR.compact(raw, count, drop)
    assert kept == 6 and list(row_of) == [0, 2, 3, 4, 5, 6, -1, -1, -1] and list(pos_of) == [0, -1, 1, 2, 3, 4, 5, -1, -1]
    assert np.array_equal(bits(pc[:6]), bits(raw[[0, 2, 3, 4, 5, 6]])) and (bits(pc[6:]) == 0x7FC00000).all()
    # the model decoded compact rows 4, 0, 3 (raw rows 5, 0, 4), in that order; a fourth flow row lies past counts
    flow = np.stack([t["above"], t["below"], t["at"], np.array([9, 9, 9], dtype=F)])
    idx_c = np.array([4, 0, 3, 1])
    est, dyn = SR.compose(raw, count, T, pos_of, flow, idx_c, 3)
    pf = SR.pose_flow(raw[:7], T)
    # the pose flow, stated operation by operation for row 0
    x, y, z = raw[0]
    a = F(F(F(F(x * T[0, 0]) + F(y * T[0, 1])) + F(z * T[0, 2])) + T[0, 3])
    assert pf[0, 0] == F(a - x)
    assert np.array_equal(bits(est[0]), bits(pf[0] + t["below"])) and dyn[0] == 0
    assert np.array_equal(bits(est[1]), bits(pf[1])) and dyn[1] == 0           # ground
    assert np.array_equal(bits(est[2]), bits(pf[2])) and dyn[2] == 0           # out of range: never decoded
    assert np.array_equal(bits(est[4]), bits(pf[4] + t["at"])) and dyn[4] == 1
    assert np.array_equal(bits(est[5]), bits(pf[5] + t["above"])) and dyn[5] == 1
    for r in (3, 6, 7, 8):                                                      # NaN, inf, padded rows: zeros of positive sign
        assert (bits(est[r]) == 0).all() and dyn[r] == 0
    h, dh = SR.compose(raw, count, T, pos_of, flow, idx_c, 3, half=True)
    assert h.dtype == np.float16 and np.array_equal(bits(h), bits(est.astype(np.float16))) and np.array_equal(dh, dyn)
    # counts = 0: nothing decoded
    est0, dyn0 = SR.compose(raw, count, T, pos_of, flow, idx_c, 0)
    assert np.array_equal(bits(est0[:3]), bits(pf[:3])) and not dyn0.any()


# ---- compaction = collate_fn_pad ----------------------------------------------------------------------------------------------------------
def _items(golden_dir, split, scene=None):
    from deflow_amd.data import HDF5Dataset
    ds = HDF5Dataset(os.path.join(golden_dir, "av2_mini", split))
    return [ds[i] for i, e in enumerate(ds.data_index) if scene is None or e[0] == scene]


@pytest.mark.parametrize("split,scene", [("val", None), ("train", "scene_chunked")])
def test_compaction_equals_collate_fn_pad(golden_dir, split, scene):
    from deflow_amd.data import collate_fn_pad
    from deflow_amd.sweeps import collate_raw_pad
    items = _items(golden_dir, split, scene)
    assert len(items) >= 2
    if scene == "scene_chunked":
        assert min(int(it["pc0"].shape[0]) for it in items) == 0 or min(int(it["pc1"].shape[0]) for it in items) == 0   # the zero-row sweep
    want, rawb = collate_fn_pad(items), collate_raw_pad(items)
    for g in ("0", "1"):
        raw, n, drop = rawb["raw" + g].numpy(), rawb["n" + g].numpy(), rawb["drop" + g].numpy()
        pc, row_of, pos_of, kept = SR.compact_batch(raw, n, drop)
        w = want["pc" + g].numpy()
        assert w.shape[1] == int(kept.max())
        assert np.array_equal(bits(pc[:, : w.shape[1]]), bits(w))                 # the NaN padding included, bit for bit
        assert (bits(pc[:, w.shape[1]:]) == 0x7FC00000).all()
        for b, it in enumerate(items):
            keep = ~it["gm" + g].numpy()
            assert kept[b] == keep.sum() and np.array_equal(row_of[b, : kept[b]], np.nonzero(keep)[0]) and (row_of[b, kept[b]:] == -1).all()
            assert np.array_equal(pos_of[b, : n[b]][keep], np.arange(kept[b])) and (pos_of[b, : n[b]][~keep] == -1).all()
            assert (pos_of[b, n[b]:] == -1).all()


def test_collate_raw_pad_shapes_and_padding(golden_dir):
    from deflow_amd.sweeps import collate_raw_pad
    items = _items(golden_dir, "val")[:3]
    b = collate_raw_pad(items)
    for g in ("0", "1"):
        rows = [int(it["pc" + g].shape[0]) for it in items]
        N = max(rows)
        assert b["raw" + g].dtype == torch.float32 and tuple(b["raw" + g].shape) == (3, N, 3)
        assert b["drop" + g].dtype == torch.uint8 and tuple(b["drop" + g].shape) == (3, N)
        assert b["n" + g].dtype == torch.int32 and b["n" + g].tolist() == rows
        for i, it in enumerate(items):
            assert torch.equal(b["raw" + g][i, : rows[i]], it["pc" + g].float()) and bool(torch.isnan(b["raw" + g][i, rows[i]:]).all())
            assert torch.equal(b["drop" + g][i, : rows[i]] != 0, it["gm" + g]) and not bool(b["drop" + g][i, rows[i]:].any())
    assert tuple(b["pose0"].shape) == tuple(b["pose1"].shape) == tuple(b["ego_motion"].shape) == (3, 4, 4) and b["pose0"].dtype == torch.float32
    assert b["scene_id"] == ["scene_val"] * 3 and b["timestamp"] == [it["timestamp"] for it in items]
    # every sweep empty: one NaN row, so that the kernels' N >= 1 holds
    empty = [{"pc0": torch.zeros(0, 3), "gm0": torch.zeros(0, dtype=torch.bool), "pc1": torch.zeros(0, 3), "gm1": torch.zeros(0, dtype=torch.bool),
              "pose0": torch.eye(4), "pose1": torch.eye(4), "scene_id": "s", "timestamp": 1}]
    e = collate_raw_pad(empty)
    assert tuple(e["raw0"].shape) == (1, 1, 3) and bool(torch.isnan(e["raw0"]).all()) and e["n0"].tolist() == [0] and "ego_motion" not in e


# ---- the command's arguments ----------------------------------------------------------------------------------------------------------------
def test_parse_args():
    from deflow_amd import save
    o = save.parse_args(["checkpoint=/x/y/deflow_best.ckpt", "dataset_path=/data/vis"])
    assert o["res_name"] == "deflow_best" and o["dataset_path"] == "/data/vis" and o["ground_source"] == "auto"
    assert o["half"] is False and o["overwrite"] is False and o["scenes"] is None and o["_rest"] == {}
    o = save.parse_args(["checkpoint=a.ckpt", "dataset_path=d", "res_name=mine", "scenes=a,b", "half=true", "overwrite=1", "batch_size=4",
                         "num_workers=2", "ground_source=online", "inference_dtype=bf16", "voxel_size=[0.2, 0.2, 6]"])
    assert o["res_name"] == "mine" and o["scenes"] == ["a", "b"] and o["half"] is True and o["overwrite"] is True
    assert o["ground_source"] == "online" and o["inference_dtype"] == "bf16"
    assert o["_rest"] == {"batch_size": "batch_size=4", "num_workers": "num_workers=2", "voxel_size": "voxel_size=[0.2, 0.2, 6]"}
    with pytest.raises(SystemExit, match="unknown key 'datset_path'"):
        save.parse_args(["checkpoint=a.ckpt", "datset_path=d"])
    for bad in ("half=maybe", "overwrite=2", "ground_source=lidar", "batch_size=0", "batch_size=x", "num_workers=-1", "inference_dtype=fp8"):
        with pytest.raises(SystemExit, match="bad value for " + bad.split("=")[0]):
            save.parse_args(["checkpoint=a.ckpt", "dataset_path=d", bad])
    with pytest.raises(SystemExit, match="expected key=value"):
        save.parse_args(["checkpoint"])
    with pytest.raises(SystemExit, match="usage"):
        save.parse_args(["checkpoint=a.ckpt"])
    for mode in ("test", "val"):
        with pytest.raises(SystemExit, match="feather"):
            save.parse_args(["checkpoint=a.ckpt", "dataset_path=d", "av2_mode=" + mode])


# ---- the flow file --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_flow_file_round_trip(tmp_path, dtype):
    from deflow_amd import save
    rng = np.random.default_rng(5)
    flows = {"315969904359876000": (rng.standard_normal((7, 3)).astype(dtype), rng.integers(0, 2, 7).astype(np.uint8)),
             "315969904459876000": (np.zeros((0, 3), dtype=dtype), np.zeros(0, dtype=np.uint8))}
    flows["315969904359876000"][0][0] = (np.inf, -0.0, 65504.0)
    meta = {"res_name": "r", "half": dtype == np.float16, "definition": "DESIGN.md 6f (UNPINNED)"}
    path = save.flow_path(str(tmp_path), "scene_x", "r")
    assert path.endswith("scene_x.r.flow.npz")
    save.write_flow(path, flows, meta)
    assert sorted(os.listdir(tmp_path)) == ["scene_x.r.flow.npz"]              # the temporary file is gone
    back = save.read_flow(path)
    assert list(back) == list(flows)
    for ts, (f, d) in flows.items():
        assert back[ts][0].dtype == dtype and back[ts][0].shape == f.shape and np.array_equal(bits(back[ts][0]), bits(f))
        assert back[ts][1].dtype == np.uint8 and np.array_equal(back[ts][1], d)
    assert save.read_meta(path) == json.loads(json.dumps(meta))
    with pytest.raises(ValueError, match="dynamic flags"):
        save.write_flow(path, {"1": (np.zeros((2, 3), dtype=dtype), np.zeros(3, dtype=np.uint8))}, meta)
    with pytest.raises(ValueError, match="float32 or float16"):
        save.write_flow(path, {"1": (np.zeros((2, 3), dtype=np.float64), np.zeros(2, dtype=np.uint8))}, meta)


def test_existing_file_is_skipped(tmp_path, monkeypatch, capsys):
    """overwrite=false: a scene whose flow file exists is reported as skipped and nothing of it is read (the model here is a stub and the
    scene file does not even exist)"""
    from deflow_amd import eval as ev
    from deflow_amd import save, train

    class Stub(torch.nn.Module):
        inference_dtype = "fp32"

        def load_from_checkpoint(self, path):
            return torch.nn.Module().load_state_dict({})

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.nn.Module, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(train, "build_model", lambda cfg: Stub())
    monkeypatch.setattr(ev, "resolve_config", lambda path, given, skip=(): dict(train.DEFAULTS))
    existing = save.flow_path(str(tmp_path), "scene_q", "best")
    save.write_flow(existing, {"5": (np.ones((1, 3), dtype=F), np.ones(1, dtype=np.uint8))}, {"res_name": "best"})
    before = open(existing, "rb").read()
    assert save.main(["checkpoint=/nowhere/best.ckpt", f"dataset_path={tmp_path}", "scenes=scene_q"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["scene"] == "scene_q" and "skipped" in line
    assert open(existing, "rb").read() == before
