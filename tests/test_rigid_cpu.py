"""CPU: the rigid cluster flow's reference helper (tests/helpers/rigid_ref.py), the argument checks of deflow_amd/rigid.py and of the C
entry points (before any launch), the new command-line keys of save / eval / train, and HDF5Dataset(flow_sidecar=...).  The GPU side is
tests/test_gpu_rigid.py; its inputs' well-posedness is checked here too, with the objects themselves as clusters."""
import ctypes as C
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

from helpers import rigid_ref as rr


# ---- the helper ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[1, 2])
def planted(request):
    s = rr.planted_sample(request.param)
    labels = rr.object_labels(s["obj0"], s["obj1"])
    return s, labels, rr.rigid_ref(s["pc0s"], s["pc1"], labels), rr.rigid_ref(s["pc0s"], s["pc1"], labels, dtype=np.float32)


def test_helper_recovers_planted_motions(planted):
    s, labels, r, q = planted
    st = r["table"][:, 7]
    assert labels.max() == 12 and (st[:12] == 1).sum() == 10 and (st[:12] == 2).sum() == 2 and not st[12:].any()
    rows = np.nonzero(r["rigid_id"] > 0)[0]
    truth = s["truth"]
    moving = rows[np.linalg.norm(truth[rows], axis=1) > 0.25]
    assert len(moving) > 800 and np.linalg.norm(truth[moving], axis=1).max() > 1.5
    # independent re-sampling lets a face slide along itself: centimetres, against motions of up to 2.5 m
    assert rr.planted_epe(r["flow"], truth, rows) < 0.08
    assert np.linalg.norm(r["flow"][rows] - truth[rows], axis=1).max() < 0.25
    # one-sided clusters, padded rows and rows of no cluster: zero
    assert not r["flow"][r["rigid_id"] == 0].any() and not r["rigid_id"][s["n0"]:].any()
    # per slot the yaw is the planted one to a few hundredths of a radian
    for k in np.nonzero(st == 1)[0]:
        assert abs(r["table"][k, 0]) < 0.13


def test_gpu_cases_are_well_posed_with_the_objects_as_clusters(planted):
    """what tests/test_gpu_rigid.py asserts on the op's own labels holds for the seeds it uses (conditions on the input)"""
    s, labels, r, q = planted
    assert r["band_pairs"].sum() == 0 and q["band_pairs"].sum() == 0
    voted = r["vote"][:, 2] > 0
    assert ((r["vote"][:, 2] - r["runner_up"])[voted] > r["edge_pairs"][voted]).all()
    for m_frac, m_yaw, m_disp in r["margins"].values():
        assert m_frac >= 0.05 and m_yaw >= 0.02 and m_disp >= 0.05
    assert np.array_equal(q["table"][:, 5:8], r["table"][:, 5:8]) and np.array_equal(q["vote"][:, :2], r["vote"][:, :2])
    assert np.array_equal(q["rigid_id"], r["rigid_id"])
    assert np.abs(q["flow"] - r["flow"]).max() < 2.5e-5 and np.abs(q["table"][:, :5] - r["table"][:, :5]).max() < 2.5e-5


def test_lattice_votes_are_exact_in_both_precisions():
    from helpers.dbscan_ref import dbscan_ref
    s = rr.lattice_sample(11, True)
    labels = dbscan_ref(torch.from_numpy(np.concatenate([s["pc0s"], s["pc1"]])), eps=0.7, min_points=4, min_cluster_size=20)["labels"].numpy()
    r = rr.rigid_ref(s["pc0s"], s["pc1"], labels, **rr.LATTICE_PARAMS)
    q = rr.rigid_ref(s["pc0s"], s["pc1"], labels, dtype=np.float32, **rr.LATTICE_PARAMS)
    assert r["R"] == 12 and np.array_equal(r["hist"], q["hist"]) and np.array_equal(r["vote"], q["vote"])
    st = r["table"][:, 7]
    assert {0, 1, 2, 5} <= set(int(v) for v in st)
    tie = [k for k in range(len(st)) if r["vote"][k, 2] > 0 and r["runner_up"][k] == r["vote"][k, 2]]
    assert any(tuple(r["vote"][k]) == (-2, 0, 256) for k in tie)             # 16 sources x 16 targets in each of two bins: the lowest wins


def test_stride_rule_and_radius():
    rows = np.arange(100, 110)
    assert list(rr._pick(rows, 4)) == [100, 102, 105, 107] and list(rr._pick(rows, 10)) == list(rows) and list(rr._pick(rows, 64)) == list(rows)
    from deflow_amd import rigid
    for md, vb in ((3.4, 0.2), (3.0, 0.25), (1.0, 0.3), (0.0, 0.2), (12.8, 0.2)):
        assert rigid.vote_radius(md, vb) == rr.vote_radius(md, vb)
    assert rigid.vote_radius(3.4, 0.2) == 17 and rigid.vote_radius(3.0, 0.25) == 12 and rigid.vote_radius(1.0, 0.3) == 4
    assert rigid.kcap(100, 57, 20) == 7 and rigid.kcap(3, 4, 20) == 1
    assert {k: v for k, v in rigid.DEFAULTS.items() if k in rr.DEFAULTS} == rr.DEFAULTS


# ---- argument errors, before any launch ---------------------------------------------------------------------------------------------------
def test_python_argument_errors():
    from deflow_amd import rigid
    pc = torch.zeros(1, 8, 3)
    cnt = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(TypeError, match="pc0s must be a CUDA tensor"):
        rigid.rigid_cluster_flow(pc, cnt, pc, cnt)
    with pytest.raises(TypeError, match="pc0s must be a CUDA tensor"):
        rigid.rigid_cluster_flow(pc.numpy(), cnt, pc, cnt)
    for key, bad in (("eps", 0.0), ("eps", float("nan")), ("min_points", 0), ("min_cluster_size", 2.5), ("min_side", 0), ("max_cluster_points", -1),
                     ("vote_cap", 0), ("vote_cap", (1 << 20) + 1), ("vote_bin", 0.0), ("vote_bin", float("inf")), ("max_disp", -1.0),
                     ("icp_cap", True), ("icp_iters", -1), ("icp_iters", 1025), ("icp_max_dist", 0.0), ("min_inlier_frac", float("nan")),
                     ("max_yaw", -0.1)):
        with pytest.raises(ValueError, match=key):
            rigid.check_params({key: bad})
    with pytest.raises(ValueError, match="at most 64 bins"):
        rigid.check_params({"max_disp": 13.1, "vote_bin": 0.2})
    with pytest.raises(ValueError, match="unknown parameter 'epsilon'"):
        rigid.check_params({"epsilon": 1.0})
    assert rigid.check_params({}) == rigid.DEFAULTS
    with pytest.raises(ValueError, match="unknown parameter"):
        rigid.IcpFlow(vote_bins=3)
    with pytest.raises(ValueError, match="point_cloud_range"):
        rigid.IcpFlow(point_cloud_range=[0, 0, 1, 1])
    with pytest.raises(ValueError, match="voxel_size"):
        rigid.IcpFlow(voxel_size=[0.2, 0.0, 6])
    m = rigid.IcpFlow(point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], vote_bin=0.25)
    assert m.grid == [64, 64, 1] and m.params["vote_bin"] == 0.25 and list(m.parameters()) == [] and m.eval() is m
    with pytest.raises(TypeError, match="CUDA tensors"):
        m.forward_padded({"pc0": pc, "pc1": pc, "pose0": torch.eye(4)[None], "pose1": torch.eye(4)[None]})


def test_entry_points_reject_bad_arguments_without_launching():
    from deflow_amd import build
    from deflow_amd._lib import load
    build.build()
    lib = load()
    P, p = C.c_void_p, C.c_void_p(0x1000)
    E_SHAPE, E_ALIGN, E_ARG = -1, -2, -3
    assert lib.df_rigid_segments_ws_bytes(2, 100, 60, 8) == 128 + 1280 and lib.df_rigid_segments_ws_bytes(0, 100, 60, 8) == E_SHAPE
    assert lib.df_rigid_segments_ws_bytes(1, 100, 60, 161) == E_SHAPE and lib.df_rigid_segments_ws_bytes(65536, 100, 60, 8) == E_SHAPE
    assert lib.df_rigid_icp_ws_bytes(2, 100, 60) == 1280 and lib.df_rigid_icp_ws_bytes(2, 2 ** 30, 1) == E_SHAPE
    assert lib.df_rigid_segments(P(0), 1, 8, 8, 1, p, p, p, p, P(0)) == E_ARG
    assert lib.df_rigid_segments(p, 1, 0, 8, 1, p, p, p, p, P(0)) == E_SHAPE
    assert lib.df_rigid_segments(p, 1, 8, 8, 0, p, p, p, p, P(0)) == E_SHAPE
    assert lib.df_rigid_segments(p, 1, 8, 8, 1, p, p, p, P(0x1002), P(0)) == E_ALIGN
    vote = lambda **k: lib.df_rigid_vote(k.get("pc", p), p, p, p, k.get("B", 1), 8, 8, 1, k.get("min_side", 8), 8192, k.get("cap", 1024),
                                         C.c_float(k.get("bin", 0.2)), k.get("R", 17), p, P(0), P(0))
    assert vote(pc=P(0)) == E_ARG and vote(B=0) == E_SHAPE and vote(R=65) == E_SHAPE and vote(R=-1) == E_SHAPE
    assert vote(min_side=0) == E_ARG and vote(cap=0) == E_ARG and vote(bin=0.0) == E_ARG and vote(bin=float("nan")) == E_ARG
    icp = lambda **k: lib.df_rigid_icp(p, p, p, p, p, k.get("B", 1), 8, 8, 1, 8, 8192, k.get("cap", 2048), k.get("iters", 8), C.c_float(0.2),
                                       C.c_float(k.get("dist", 0.5)), C.c_float(0.6), C.c_float(k.get("yaw", 0.35)), C.c_float(3.4),
                                       k.get("table", p), k.get("ws", p), P(0))
    assert icp(table=P(0)) == E_ARG and icp(B=70000) == E_SHAPE and icp(cap=0) == E_ARG and icp(iters=-1) == E_ARG and icp(iters=1025) == E_ARG
    assert icp(dist=0.0) == E_ARG and icp(yaw=-1.0) == E_ARG and icp(ws=P(0x1001)) == E_ALIGN
    assert lib.df_rigid_apply(p, p, p, p, p, p, 1, 8, 8, 1, P(0), p, P(0)) == E_ARG
    assert lib.df_rigid_apply(p, p, p, p, p, p, 1, 8, 8, 17, p, p, P(0)) == E_SHAPE


# ---- the commands' new keys -----------------------------------------------------------------------------------------------------------------
def test_save_arguments():
    from deflow_amd import rigid, save
    opt = save.parse_args(["model=icpflow", "dataset_path=/d"])
    assert opt["model"] == "icpflow" and opt["res_name"] == "icpflow" and opt["checkpoint"] is None and opt["params"] == rigid.DEFAULTS and opt["_rest"] == {}
    opt = save.parse_args(["model=icpflow", "dataset_path=/d", "res_name=r", "icp_vote_bin=0.25", "icp_iters=4", "icp_min_side=10",
                           "ground_source=online", "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]", "batch_size=2"])
    assert opt["res_name"] == "r" and opt["params"]["vote_bin"] == 0.25 and opt["params"]["icp_iters"] == 4 and opt["params"]["min_side"] == 10
    assert sorted(opt["_rest"]) == ["batch_size", "point_cloud_range"] and opt["ground_source"] == "online"
    assert set(rigid.COMMAND_KEYS) == {"icp_eps", "icp_min_points", "icp_min_cluster_size", "icp_min_side", "icp_max_cluster_points",
                                       "icp_vote_cap", "icp_vote_bin", "icp_max_disp", "icp_cap", "icp_iters", "icp_max_dist",
                                       "icp_min_inlier_frac", "icp_max_yaw"}
    for argv, what in ((["model=icpflow"], "usage: python -m deflow_amd.save model=icpflow"),
                       (["model=icpflow", "dataset_path=/d", "checkpoint=a.ckpt"], "has no weights"),
                       (["model=icpflow", "dataset_path=/d", "inference_dtype=bf16"], "has no weights"),
                       (["model=icpflow", "dataset_path=/d", "icp_vote_bin=0"], "vote_bin"),
                       (["model=icpflow", "dataset_path=/d", "icp_iters=many"], "bad value for icp_iters"),
                       (["model=icpflow", "dataset_path=/d", "icp_bins=3"], "unknown key 'icp_bins'"),
                       (["checkpoint=a.ckpt", "dataset_path=/d", "icp_iters=4"], "belong to model=icpflow"),
                       (["dataset_path=/d"], "usage: python -m deflow_amd.save checkpoint=")):
        with pytest.raises(SystemExit, match=what):
            save.parse_args(argv)
    # existing invocations are unchanged
    opt = save.parse_args(["checkpoint=/x/best.ckpt", "dataset_path=/d", "model=fastflow3d"])
    assert opt["model"] is None and opt["res_name"] == "best" and opt["_rest"] == {"model": "model=fastflow3d"}


def test_eval_and_train_arguments():
    from deflow_amd import eval as ev, pairflow, rigid, train
    config = lambda given: pairflow.config(pairflow.entry("icpflow"), given)
    cfg, params = config({"model": "model=icpflow", "dataset_path": "dataset_path=/r", "icp_max_yaw": "icp_max_yaw=0.2",
                                     "batch_size": "batch_size=2"})
    assert cfg["model"] == "icpflow" and cfg["val_data"] == os.path.join("/r", "val") and cfg["batch_size"] == 2
    assert params["max_yaw"] == 0.2 and params["vote_bin"] == rigid.DEFAULTS["vote_bin"]
    with pytest.raises(SystemExit, match="no checkpoint="):
        config({"model": "model=icpflow", "checkpoint": "checkpoint=a.ckpt"})
    with pytest.raises(SystemExit, match="min_inlier_frac"):
        config({"model": "model=icpflow", "icp_min_inlier_frac": "icp_min_inlier_frac=-1"})
    with pytest.raises(SystemExit, match="av2_mode=test is out of its scope"):            # refused before anything touches a GPU
        ev.main(["model=icpflow", "av2_mode=test", "dataset_path=/r"])
    with pytest.raises(SystemExit, match="unknown model 'icpflow'"):                      # the trainer has nothing to train there
        train.parse_overrides(["model=icpflow"])
    assert train.split_pseudo_flow(["lr=1e-3", "pseudo_flow=icpflow", "model=fastflow3d"]) == ("icpflow", ["lr=1e-3", "model=fastflow3d"])
    assert train.split_pseudo_flow(["lr=1e-3"]) == (None, ["lr=1e-3"])
    assert train.split_pseudo_flow(["pseudo_flow=a", "+pseudo_flow=b"])[0] == "b"
    for bad in ("pseudo_flow=", "pseudo_flow=a/b"):
        with pytest.raises(SystemExit, match="bad value for pseudo_flow"):
            train.split_pseudo_flow([bad])
    assert "pseudo_flow" not in train.DEFAULTS                                            # never saved as a hyper-parameter
    with pytest.raises(SystemExit, match="pseudo_flow=<res_name> reads"):                 # synthetic pairs have no scene files
        train.main(["pseudo_flow=icpflow"])


# ---- HDF5Dataset(flow_sidecar=...) ----------------------------------------------------------------------------------------------------------
def test_flow_sidecar(tmp_path, golden_dir):
    from deflow_amd import save
    from deflow_amd.data import HDF5Dataset, collate_fn_pad
    src = os.path.join(golden_dir, "av2_mini", "train")
    for n in ("scene_a.h5", "index_total.pkl"):
        shutil.copy(os.path.join(src, n), tmp_path / n)                                   # never written under tests/golden
    with open(tmp_path / "index_total.pkl", "rb") as f:
        index = [e for e in pickle.load(f) if e[0] == "scene_a"]
    with open(tmp_path / "index_total.pkl", "wb") as f:
        pickle.dump(index, f)
    plain = HDF5Dataset(str(tmp_path))
    items = [plain[i] for i in range(len(plain))]
    rng = np.random.default_rng(3)
    flows = {str(it["timestamp"]): (rng.standard_normal((it["pc0"].shape[0], 3)).astype(np.float32),
                                    np.zeros(it["pc0"].shape[0], np.uint8)) for it in items}
    save.write_flow(save.flow_path(str(tmp_path), "scene_a", "icpflow"), flows, {"model": "icpflow"})
    # a group that has `flow` keeps it
    ds = HDF5Dataset(str(tmp_path), flow_sidecar="icpflow")
    for a, b in zip(items, (ds[i] for i in range(len(ds)))):
        assert sorted(a) == sorted(b) and torch.equal(a["flow"], b["flow"]) and torch.equal(a["flow_is_valid"], b["flow_is_valid"])
    # a group without one takes the file's: the scene's in-memory directory loses its labels (the file itself is not touched)
    ds = HDF5Dataset(str(tmp_path), flow_sidecar="icpflow")
    f = ds._file("scene_a")
    for ts in f.sweeps:
        for k in ("flow", "flow_is_valid", "flow_category_indices"):
            f.root[ts].pop(k, None)
    got = [ds[i] for i in range(len(ds))]
    for a, b in zip(items, got):
        want = flows[str(a["timestamp"])][0]
        assert b["flow"].dtype == torch.float32 and np.array_equal(b["flow"].numpy(), want)
        assert b["flow_is_valid"].dtype == torch.bool and bool(b["flow_is_valid"].all()) and b["flow_is_valid"].shape == (want.shape[0],)
        assert b["flow_category_indices"].dtype == torch.uint8 and not bool(b["flow_category_indices"].any())
        assert torch.equal(a["pc0"], b["pc0"]) and sorted(a) == sorted(b)
    batch = collate_fn_pad(got[:2])
    keep = ~got[0]["gm0"]
    assert torch.equal(batch["flow"][0, : int(keep.sum())], got[0]["flow"][keep]) and batch["flow_is_valid"].dtype == torch.bool
    # without the argument such a group gives an item without labels, as before
    off = HDF5Dataset(str(tmp_path))
    g = off._file("scene_a")
    for ts in g.sweeps:
        g.root[ts].pop("flow", None)
    assert "flow" not in off[0]
    # a length mismatch is a ValueError, a missing file or timestamp a KeyError naming the command
    ts0 = str(items[0]["timestamp"])
    bad = dict(flows)
    bad[ts0] = (flows[ts0][0][:-1], flows[ts0][1][:-1])
    save.write_flow(save.flow_path(str(tmp_path), "scene_a", "short"), bad, {})
    ds = HDF5Dataset(str(tmp_path), flow_sidecar="short")
    ds._file("scene_a").root[ts0].pop("flow")
    with pytest.raises(ValueError, match="another version of the scene file"):
        ds[[str(e[1]) for e in ds.data_index].index(ts0)]
    ds = HDF5Dataset(str(tmp_path), flow_sidecar="absent")
    ds._file("scene_a").root[ts0].pop("flow")
    with pytest.raises(KeyError, match="python -m deflow_amd.save"):
        ds[[str(e[1]) for e in ds.data_index].index(ts0)]
    with pytest.raises(ValueError, match="flow_sidecar"):
        HDF5Dataset(str(tmp_path), flow_sidecar="a/b")
