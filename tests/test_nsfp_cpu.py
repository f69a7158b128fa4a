"""No GPU: the reference helper of model=nsfp (tests/helpers/nsfp_ref.py) against torch.autograd in float64, the parameter layout, the
parameter checks and the commands' keys and refusals."""
import math
import os
import pickle
import re
import shutil

import numpy as np
import pytest
import torch

from helpers import nsfp_ref as nr


# ---- the helper -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [0, 2])
def test_helper_backward_matches_autograd_in_float64(depth):
    gen = torch.Generator().manual_seed(depth)
    flat = nr.xavier_params(depth, gen, torch.float64, bias=0.3).requires_grad_(True)
    x = torch.randn(40, 3, generator=gen, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(40, 3, generator=gen, dtype=torch.float64)
    y, zs, acts = nr.mlp_forward(x, flat, depth)
    gf, gx = torch.autograd.grad((y * dy).sum(), (flat, x))
    g2, dx2 = nr.mlp_backward(x.detach(), flat.detach(), depth, dy, [z > 0 for z in zs])
    assert float((gf - g2).abs().max()) <= 1e-12 * max(1.0, float(gf.abs().max()))
    assert float((gx - dx2).abs().max()) <= 1e-12 * max(1.0, float(gx.abs().max()))
    assert all(torch.equal(a > 0, z > 0) for a, z in zip(acts, zs))


def test_helper_chamfer_and_iteration():
    """the truncated chamfer term by all pairs: rows beyond trunc_d2 are left out of the means, a mean over no rows is 0, and the hand-fed
    neighbour route gives the all-pairs loss and gradients"""
    A = torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [10.0, 0, 0]], dtype=torch.float64)
    Bc = torch.tensor([[0.5, 0, 0], [1.0, 1.0, 0]], dtype=torch.float64)
    rep = {}
    v, (ia, ib) = nr.tc(A, Bc, 4.0, rep)
    assert ia.tolist() == [0, 0, -1] and ib.tolist() == [0, 1]
    assert abs(float(v) - ((0.25 + 0.25) / 2 + (0.25 + 1.0) / 2)) < 1e-15
    assert rep["min_gap"] == 0 and rep["min_trunc_edge"] == 3.0         # the tie of Bc[0] between A[0] and A[1] is reported; |1.0 - 4.0|
    assert float(nr.tc(A + 100, Bc, 4.0)[0]) == 0.0
    P0, P1, _ = nr.planted_blobs(1, blobs=2, per_blob=20)
    gen = torch.Generator().manual_seed(3)
    f, g = nr.xavier_params(1, gen, torch.float64), nr.xavier_params(1, gen, torch.float64)
    P0, P1 = torch.from_numpy(P0).double(), torch.from_numpy(P1).double()
    loss, F, df, dg, nn = nr.iteration(P0, P1, f, g, 1, 4.0)
    loss2, F2, df2, dg2, _ = nr.iteration(P0, P1, f, g, 1, 4.0, nn=nn)
    assert float(loss) == float(loss2) and torch.equal(df, df2) and torch.equal(dg, dg2) and float(df.abs().max()) > 0
    # Adam: three steps of torch.optim.Adam
    q = f.clone().requires_grad_(True)
    opt = torch.optim.Adam([q], lr=8e-3)
    p, m, v = f, torch.zeros_like(f), torch.zeros_like(f)
    for t in (1, 2, 3):
        q.grad = df * t
        opt.step()
        p, m, v = nr.adam_step(p, df * t, m, v, t)
    assert float((p - q.detach()).abs().max()) < 1e-12 and float((p - f).abs().max()) > 1e-2
    assert nr.replay([3.0, 2.0, 2.0, 1.99995, 1.0], patience=2, min_delta=1e-4)[:3] == (np.float32(2.0), 2, True)


# ---- layout, parameters, initialisation -----------------------------------------------------------------------------------------------
def test_parameter_layout_and_count():
    from deflow_amd import nsfp
    for depth in (0, 1, 7, 15):
        P = (128 * 3 + 128) + depth * (128 * 128 + 128) + (3 * 128 + 3)
        assert nsfp.num_params(depth) == P == nr.num_params(depth)
        assert nsfp.param_stride(depth) % 4 == 0 and 0 <= nsfp.param_stride(depth) - P < 4
        sl = nsfp.param_slices(depth)
        names = ["W_in", "b_in"] + [f"{k}_{l}" for l in range(1, depth + 1) for k in ("W", "b")] + ["W_out", "b_out"]
        assert list(sl) == names
        o = 0
        for (off, shape), (W, b) in zip(list(sl.values())[0::2], nr.unpack(torch.arange(P), depth)):
            assert off == int(W.reshape(-1)[0]) and tuple(W.shape) == shape
        assert sl["W_in"] == (0, (128, 3)) and sl["b_in"] == (384, (128,)) and sl["b_out"] == (P - 3, (3,))
    assert nsfp.num_params(7) == 116483


def test_seeded_initialisation():
    from deflow_amd import nsfp
    a, b, c = nsfp.init_params(2, 5), nsfp.init_params(2, 5), nsfp.init_params(2, 6)
    assert a.shape == (2, nsfp.param_stride(2)) and a.dtype == torch.float32
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a[0], a[1])          # reproducible; f and g differ
    for name, (o, shape) in nsfp.param_slices(2).items():
        blk = a[:, o:o + math.prod(shape)]
        if name.startswith("b"):
            assert not blk.any()
        else:
            lim = math.sqrt(6.0 / (shape[0] + shape[1]))
            assert float(blk.abs().max()) <= lim and float(blk.abs().max()) > 0.9 * lim and abs(float(blk.mean())) < 0.1 * lim
    assert not a[:, nsfp.num_params(2):].any()
    # every sample of a batch starts from the same copy: the arena is this block repeated (nsfp_optimize: start[None].repeat(B, 1, 1))
    src = open(nsfp.__file__).read()
    assert "repeat(B, 1, 1)" in src
    # the loop, its Adam call and its graph capture are pairopt's, imported and not copied
    assert "requires_grad" not in src and ".backward(" not in src and "from .pairopt import" in src
    assert "df_adam_step_dev" not in src and "torch.cuda.graph" not in src and "CUDAGraph" not in src
    assert re.search(r"def \w*(snapshot|freeze|run)\w*\(", src) is None


def test_check_params():
    from deflow_amd import nsfp
    assert nsfp.check_params({}) == nsfp.DEFAULTS == {"depth": 7, "iters": 1000, "lr": 8e-3, "trunc_d2": 4.0, "patience": 100,
                                                      "min_delta": 1e-4, "check_every": 50, "seed": 0, "graph": False}
    assert nsfp.check_params({"depth": 0, "check_every": 0, "graph": True, "iters": 3.0})["iters"] == 3
    for bad, what in (({"depth": 16}, "depth"), ({"depth": -1}, "depth"), ({"depth": 1.5}, "depth"), ({"iters": 0}, "iters"),
                      ({"lr": 0}, "lr"), ({"lr": float("nan")}, "lr"), ({"trunc_d2": -1}, "trunc_d2"), ({"patience": 0}, "patience"),
                      ({"min_delta": -1e-3}, "min_delta"), ({"check_every": -1}, "check_every"), ({"seed": -1}, "seed"),
                      ({"graph": 1}, "graph"), ({"width": 64}, "unknown parameter 'width'"), ({"depth": True}, "depth")):
        with pytest.raises(ValueError, match=what):
            nsfp.check_params(bad)
    assert set(nsfp.COMMAND_KEYS) == {"nsfp_depth", "nsfp_iters", "nsfp_lr", "nsfp_trunc_d2", "nsfp_patience", "nsfp_min_delta",
                                      "nsfp_check_every", "nsfp_seed", "nsfp_graph"}
    assert nsfp.params_from_command({"nsfp_graph": "true", "nsfp_lr": "1e-3"})["graph"] is True
    with pytest.raises(SystemExit, match="bad value for nsfp_iters"):
        nsfp.params_from_command({"nsfp_iters": "many"})
    # CPU tensors are refused by name
    x = torch.zeros(1, 4, 3)
    with pytest.raises(TypeError, match="x must be a CUDA tensor"):
        nsfp.mlp_forward(x, torch.zeros(1, dtype=torch.int32), torch.zeros(1, nsfp.param_stride(1)), 1)
    with pytest.raises(TypeError, match="pc0s must be a CUDA tensor"):
        nsfp.nsfp_optimize(x, torch.zeros(1, dtype=torch.int32), x, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="voxel_size"):
        nsfp.Nsfp(voxel_size=(0.2, 0.2))
    with pytest.raises(ValueError, match="depth"):
        nsfp.Nsfp(depth=99)
    m = nsfp.Nsfp(iters=5)
    assert m.eval() is m and m.to("cuda") is m and list(m.parameters()) == [] and m.params["iters"] == 5


# ---- the commands' keys and refusals --------------------------------------------------------------------------------------------------
def test_save_arguments():
    from deflow_amd import nsfp, pairflow, save
    opt = save.parse_args(["model=nsfp", "dataset_path=/d"])
    assert opt["model"] == "nsfp" and opt["res_name"] == "nsfp" and opt["checkpoint"] is None
    assert opt["params"] == nsfp.DEFAULTS and opt["_rest"] == {"batch_size": f"batch_size={nsfp.COMMAND_BATCH_SIZE}"}
    opt = save.parse_args(["model=nsfp", "dataset_path=/d", "res_name=r", "nsfp_iters=4", "nsfp_depth=2", "nsfp_graph=true", "batch_size=3"])
    assert opt["res_name"] == "r" and opt["params"]["iters"] == 4 and opt["params"]["depth"] == 2 and opt["params"]["graph"]
    assert opt["_rest"] == {"batch_size": "batch_size=3"}
    for argv, what in ((["model=nsfp"], "usage: python -m deflow_amd.save model=nsfp"),
                       (["model=nsfp", "dataset_path=/d", "checkpoint=a.ckpt"], "has no weights"),
                       (["model=nsfp", "dataset_path=/d", "inference_dtype=bf16"], "has no weights"),
                       (["model=nsfp", "dataset_path=/d", "nsfp_depth=16"], "depth"),
                       (["model=nsfp", "dataset_path=/d", "nsfp_iters=many"], "bad value for nsfp_iters"),
                       (["model=nsfp", "dataset_path=/d", "nsfp_width=64"], "unknown key 'nsfp_width'"),
                       (["model=nsfp", "dataset_path=/d", "icp_iters=4"], "belong to model=icpflow"),
                       (["model=icpflow", "dataset_path=/d", "nsfp_iters=4"], "belong to model=nsfp"),
                       (["checkpoint=a.ckpt", "dataset_path=/d", "nsfp_iters=4"], "belong to model=nsfp"),
                       (["model=nsfp", "dataset_path=/d", "av2_mode=test"], "takes no av2_mode")):
        with pytest.raises(SystemExit, match=what):
            save.parse_args(argv)
    assert "512 bytes" in pairflow.usage(pairflow.entry("nsfp"))
    # existing invocations are unchanged
    opt = save.parse_args(["checkpoint=/x/best.ckpt", "dataset_path=/d", "model=fastflow3d"])
    assert opt["model"] is None and opt["res_name"] == "best" and opt["_rest"] == {"model": "model=fastflow3d"}
    assert save.parse_args(["model=icpflow", "dataset_path=/d"])["_rest"] == {}


def test_eval_and_train_arguments():
    from deflow_amd import eval as ev, pairflow, nsfp, train
    config = lambda given: pairflow.config(pairflow.entry("nsfp"), given)
    cfg, params = config({"model": "model=nsfp", "dataset_path": "dataset_path=/r", "nsfp_iters": "nsfp_iters=20"})
    assert cfg["model"] == "nsfp" and cfg["val_data"] == os.path.join("/r", "val") and cfg["batch_size"] == nsfp.COMMAND_BATCH_SIZE
    assert params["iters"] == 20 and params["depth"] == 7
    assert config({"model": "model=nsfp", "batch_size": "batch_size=5"})[0]["batch_size"] == 5
    with pytest.raises(SystemExit, match="no checkpoint="):
        config({"model": "model=nsfp", "checkpoint": "checkpoint=a.ckpt"})
    with pytest.raises(SystemExit, match="belong to model=icpflow"):
        config({"model": "model=nsfp", "icp_iters": "icp_iters=2"})
    with pytest.raises(SystemExit, match="patience"):
        config({"model": "model=nsfp", "nsfp_patience": "nsfp_patience=0"})
    with pytest.raises(SystemExit, match="av2_mode=test is out of its scope.*deflow_amd.save model=nsfp"):   # names the alternative
        ev.main(["model=nsfp", "av2_mode=test", "dataset_path=/r"])
    with pytest.raises(SystemExit, match="belong to model=nsfp"):
        ev.main(["checkpoint=a.ckpt", "nsfp_iters=3"])
    with pytest.raises(SystemExit, match="unknown model 'nsfp'"):                          # the trainer has nothing to train there
        train.parse_overrides(["model=nsfp"])
    assert train.split_pseudo_flow(["lr=1e-3", "pseudo_flow=nsfp"]) == ("nsfp", ["lr=1e-3"])


def test_pseudo_flow_reads_an_nsfp_sidecar(tmp_path, golden_dir):
    """what `train ... pseudo_flow=nsfp` reads: HDF5Dataset(flow_sidecar="nsfp") on a file written under the command's default res_name"""
    from deflow_amd import save
    from deflow_amd.data import HDF5Dataset
    src = os.path.join(golden_dir, "av2_mini", "train")
    for n in ("scene_a.h5", "index_total.pkl"):
        shutil.copy(os.path.join(src, n), tmp_path / n)                                   # never written under tests/golden
    with open(tmp_path / "index_total.pkl", "rb") as f:
        index = [e for e in pickle.load(f) if e[0] == "scene_a"]
    with open(tmp_path / "index_total.pkl", "wb") as f:
        pickle.dump(index, f)
    plain = HDF5Dataset(str(tmp_path))
    items = [plain[i] for i in range(len(plain))]
    rng = np.random.default_rng(4)
    flows = {str(it["timestamp"]): (rng.standard_normal((it["pc0"].shape[0], 3)).astype(np.float32), np.zeros(it["pc0"].shape[0], np.uint8))
             for it in items}
    path = save.flow_path(str(tmp_path), "scene_a", save.parse_args(["model=nsfp", f"dataset_path={tmp_path}"])["res_name"])
    assert os.path.basename(path) == "scene_a.nsfp.flow.npz"
    save.write_flow(path, flows, {"model": "nsfp"})
    ds = HDF5Dataset(str(tmp_path), flow_sidecar="nsfp")
    f = ds._file("scene_a")
    for ts in f.sweeps:
        for k in ("flow", "flow_is_valid", "flow_category_indices"):
            f.root[ts].pop(k, None)
    for a, b in zip(items, (ds[i] for i in range(len(ds)))):
        assert np.array_equal(b["flow"].numpy(), flows[str(a["timestamp"])][0]) and bool(b["flow_is_valid"].all())
