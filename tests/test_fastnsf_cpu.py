"""No GPU: the reference helper of model=fastnsf (tests/helpers/dt_ref.py) against scipy's exact distance transform and torch.autograd in
float64, the grid, the parameter checks and the commands' keys and refusals."""
import os
import pickle
import re
import shutil

import numpy as np
import pytest
import torch

from helpers import dt_ref as dr
from helpers import nsfp_ref as nr


# ---- the helper -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,R,n", [((2, 2, 2), 1, 1), ((5, 3, 2), 3, 2), ((23, 11, 7), 3, 9), ((23, 11, 7), 20, 4), ((9, 8, 7), 2, 0)])
def test_helper_transform_equals_scipy(dims, R, n):
    from scipy import ndimage
    gen = torch.Generator().manual_seed(sum(dims) + R)
    occ = torch.zeros(dims[2], dims[1], dims[0], dtype=torch.bool)
    for _ in range(n):
        occ[int(torch.randint(dims[2], (1,), generator=gen)), int(torch.randint(dims[1], (1,), generator=gen)),
            int(torch.randint(dims[0], (1,), generator=gen))] = True
    got = dr.brute_dt2(occ, R)
    assert got.dtype == torch.int64 and got.shape == occ.shape
    if n:
        want = np.minimum(np.rint(ndimage.distance_transform_edt(~occ.numpy()) ** 2), R * R).astype(np.int64)
        assert np.array_equal(got.numpy(), want) and int(got.min()) == 0
    else:
        assert bool((got == R * R).all())
    assert torch.equal(got, dr.edt_dt2(occ, R))


def test_helper_occupancy_and_single_point():
    origin, dims, R = dr.grid((-1.0, -0.5, 0.0, 1.0, 0.5, 0.5), 0.25, 0.75)
    assert origin == (-1.75, -1.25, -0.75) and dims == (8 + 6, 4 + 6, 2 + 6) and R == 3
    P1 = np.array([[0.1, 0.1, 0.1], [np.nan, 0, 0], [100.0, 0, 0], [-1.75, -1.25, -0.75], [1.7499, 1.2499, 1.2499], [1.75, 0, 0]], np.float32)
    occ = dr.occupancy(P1, origin, 0.25, dims)
    assert int(occ.sum()) == 3 and bool(occ[3, 5, 7]) and bool(occ[0, 0, 0]) and bool(occ[7, 9, 13])       # the faces: the low one is inside
    one = dr.brute_dt2(dr.occupancy(P1[:1], origin, 0.25, dims), R)
    z, y, x = torch.meshgrid(torch.arange(8), torch.arange(10), torch.arange(14), indexing="ij")
    assert torch.equal(one, ((x - 7) ** 2 + (y - 5) ** 2 + (z - 3) ** 2).clamp_max(9))


def test_helper_gradient_matches_autograd_in_float64():
    gen = torch.Generator().manual_seed(3)
    origin, dims, R = dr.grid((-1.0, -1.0, 0.0, 1.0, 1.0, 0.5), 0.25, 0.75)
    P1 = (torch.rand(12, 3, generator=gen) * torch.tensor([2.0, 2.0, 0.5]) + torch.tensor([-1.0, -1.0, 0.0])).float()
    dt2 = dr.brute_dt2(dr.occupancy(P1, origin, 0.25, dims), R)
    lo, hi = torch.tensor(origin, dtype=torch.float64), torch.tensor(origin, dtype=torch.float64) + 0.25 * torch.tensor(dims)
    q = (lo - 0.4 + torch.rand(400, 3, generator=gen, dtype=torch.float64) * (hi - lo + 0.8)).requires_grad_(True)     # beyond every face too
    d, g, cells, clamped = dr.lookup(q, dt2, origin, 0.25, R)
    auto, = torch.autograd.grad(d.sum(), q)
    assert float((auto - g).abs().max()) <= 1e-12 and float(g.abs().max()) > 0.5
    assert bool(clamped.any(dim=0).all()) and bool((g[clamped] == 0).all()) and bool((~clamped).all(dim=1).any())
    assert float(d.detach().min()) >= 0 and float(d.detach().max()) <= R * 0.25 + 1e-12
    # GIVEN cells: the same interpolant, also one cell further (t leaves [0, 1]) -- continuous across the plane, so equal there
    d2 = dr.lookup(q.detach(), dt2, origin, 0.25, R, cells=cells)[0]
    assert torch.equal(d2, d.detach())
    u = (torch.tensor([[0.0, 0.1, 0.1]], dtype=torch.float64) - lo) / 0.25 - 0.5          # u_x = 6.5 -> on a plane after a shift of cell / 2
    on = torch.tensor([[0.125, 0.1, 0.1]], dtype=torch.float64)
    a = dr.lookup(on, dt2, origin, 0.25, R)
    b = dr.lookup(on, dt2, origin, 0.25, R, cells=a[2] - torch.tensor([[1, 0, 0]]))
    assert abs(float(a[0] - b[0])) < 1e-14 and float(u[0, 0]) == 6.5
    # the report: distance to the nearest plane in voxels
    assert float(dr.plane_distance(on, origin, 0.25, dims)) < 1e-12
    assert abs(float(dr.plane_distance(torch.tensor([[0.0, 0.0625, 0.3125]]), origin, 0.25, dims)) - 0.25) < 1e-12
    out = torch.tensor([[-2.0, 0.0, 0.3]], dtype=torch.float64)                 # u = (-1.5, 6.5, 3.7): 1.5 outside on x, 0.5 and 0.3 inside
    assert abs(float(dr.plane_distance(out, origin, 0.25, dims)) - 0.3) < 1e-12
    assert abs(float(dr.plane_distance(torch.tensor([[-1.8, 0.0, 0.25]], dtype=torch.float64), origin, 0.25, dims)) - 0.5) < 1e-12
    # non-finite rows
    d3, g3, _, _ = dr.lookup(torch.tensor([[float("nan"), 0, 0]], dtype=torch.float64), dt2, origin, 0.25, R)
    assert float(d3) == 0.75 and not g3.any()


def test_helper_iteration_and_loop():
    P0, P1, truth = nr.planted_blobs(1, blobs=2, per_blob=30, shift=0.3, spacing=2.5, size=(1.2, 0.8, 0.6))
    origin, dims, R = dr.grid((-6.4, -6.4, -1.6, 6.4, 6.4, 1.6), 0.2, 1.0)
    occ = dr.occupancy(P1, origin, dr.f32(0.2), dims)
    dt2 = dr.edt_dt2(occ, R)
    from deflow_amd import nsfp
    f = nsfp.init_params(1, 0)[0, :nr.num_params(1)].double()
    loss, F, df, cells, W = dr.iteration(torch.from_numpy(P0).double(), dt2, origin, dr.f32(0.2), R, f, 1)
    loss2, _, df2, _, _ = dr.iteration(torch.from_numpy(P0).double(), dt2, origin, dr.f32(0.2), R, f, 1, cells=cells)
    assert float(loss) == float(loss2) and torch.equal(df, df2) and float(df.abs().max()) > 0
    flow, best, hist = dr.optimize(torch.from_numpy(P0).double(), dt2, origin, dr.f32(0.2), R, f, 1, 30)
    assert len(hist) == 30 and best < hist[0] and best == min(hist)


# ---- the grid, the parameters, the start ----------------------------------------------------------------------------------------------
def test_dt_grid():
    from deflow_amd import fastnsf
    origin, dims, R = fastnsf.dt_grid((-51.2, -51.2, -3, 51.2, 51.2, 3), 0.1, 2.0)
    assert dims == (1064, 1064, 100) and R == 20 and origin == (dr.f32(-53.2), dr.f32(-53.2), -5.0)
    assert dims[0] * dims[1] * dims[2] * 2 == 226419200                                   # 226 MB per sample
    for rng, cell, trunc in (((-6.4, -6.4, -1.6, 6.4, 6.4, 1.6), 0.1, 2.0), ((-6.4, -6.4, -3, 6.4, 6.4, 3), 0.4, 2.0), ((0, 0, 0, 1, 0.3, 0.05), 0.25, 0.75)):
        assert fastnsf.dt_grid(rng, cell, trunc) == dr.grid(rng, cell, trunc)
    assert fastnsf.dt_grid((0, 0, 0, 0.01, 0.01, 0.01), 0.1, 0.1)[1] == (3, 3, 3)
    for args, what in ((((0, 0, 0, 1, 1), 0.1, 2.0), "grid_range"), (((0, 0, 0, 1, 1, float("nan")), 0.1, 2.0), "grid_range"),
                       (((0, 0, 0, 1, 1, 0), 0.1, 2.0), "grid_range"), (((0, 0, 0, 1, 1, 1), 0.0, 2.0), "cell"),
                       (((0, 0, 0, 1, 1, 1), 0.1, -2.0), "trunc"), (((0, 0, 0, 1, 1, 1), 0.3, 2.0), "trunc"),
                       (((0, 0, 0, 1, 1, 1), 0.001, 2.0), "trunc"), (((0, 0, 0, 1, 1, 1), 0.1, 0.04), "trunc"),
                       (((-200, -200, -20, 200, 200, 20), 0.1, 2.0), "grid_range")):
        with pytest.raises(ValueError, match=what):
            fastnsf.dt_grid(*args)


def test_check_params_and_start():
    from deflow_amd import fastnsf, nsfp
    assert fastnsf.check_params({}) == fastnsf.DEFAULTS == {"depth": 7, "iters": 1000, "lr": 8e-3, "cell": 0.1, "trunc": 2.0, "patience": 100,
                                                            "min_delta": 1e-4, "check_every": 50, "seed": 0, "graph": False}
    assert fastnsf.check_params({"depth": 0, "check_every": 0, "graph": True, "iters": 3.0, "cell": 0.4})["iters"] == 3
    for bad, what in (({"depth": 16}, "depth"), ({"depth": 1.5}, "depth"), ({"iters": 0}, "iters"), ({"lr": 0}, "lr"), ({"cell": -0.1}, "cell"),
                      ({"trunc": float("nan")}, "trunc"), ({"cell": 0.3}, "trunc"), ({"trunc": 30.0}, "trunc"), ({"patience": 0}, "patience"),
                      ({"min_delta": -1e-3}, "min_delta"), ({"check_every": -1}, "check_every"), ({"seed": -1}, "seed"),
                      ({"graph": 1}, "graph"), ({"trunc_d2": 4.0}, "unknown parameter 'trunc_d2'"), ({"depth": True}, "depth")):
        with pytest.raises(ValueError, match=what):
            fastnsf.check_params(bad)
    assert set(fastnsf.COMMAND_KEYS) == {"fastnsf_depth", "fastnsf_iters", "fastnsf_lr", "fastnsf_cell", "fastnsf_trunc", "fastnsf_patience",
                                         "fastnsf_min_delta", "fastnsf_check_every", "fastnsf_seed", "fastnsf_graph"}
    assert fastnsf.params_from_command({"fastnsf_graph": "true", "fastnsf_cell": "0.4"})["cell"] == 0.4
    with pytest.raises(SystemExit, match="bad value for fastnsf_iters"):
        fastnsf.params_from_command({"fastnsf_iters": "many"})
    # the start is row 0 (the forward net f) of nsfp.init_params: the same seed starts both estimators from the same f
    for depth, seed in ((0, 0), (2, 5), (7, 1)):
        a = fastnsf.start_params(depth, seed)
        assert a.shape == (1, nsfp.param_stride(depth)) and a.dtype == torch.float32 and torch.equal(a[0], nsfp.init_params(depth, seed)[0])
    src = open(fastnsf.__file__).read()
    assert 'start_params(depth, p["seed"]) if init is None' in src and "repeat(B, 1, 1)" in src      # every sample starts from that copy
    # the optimiser uses no autograd, and the loop, its Adam call and its graph capture are pairopt's, imported and not copied
    assert "requires_grad" not in src and ".backward(" not in src and "from .pairopt import" in src
    assert "df_adam_step_dev" not in src and "torch.cuda.graph" not in src and "CUDAGraph" not in src
    assert re.search(r"def \w*(snapshot|freeze|run)\w*\(", src) is None
    # CPU tensors are refused by name
    x, c = torch.zeros(1, 4, 3), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(TypeError, match="ref must be a CUDA tensor"):
        fastnsf.dt_build(x, c, origin=(0, 0, 0), cell=0.1, dims=(4, 4, 4), radius=2)
    with pytest.raises(TypeError, match="query must be a CUDA tensor"):
        fastnsf.dt_lookup(x, c, torch.zeros(1, 4, 4, 4, dtype=torch.uint16), origin=(0, 0, 0), cell=0.1, radius=2)
    with pytest.raises(TypeError, match="pc0s must be a CUDA tensor"):
        fastnsf.fastnsf_optimize(x, c, x, c, grid_range=(-1, -1, -1, 1, 1, 1))
    with pytest.raises(ValueError, match="voxel_size"):
        fastnsf.FastNsf(voxel_size=(0.2, 0.2))
    with pytest.raises(ValueError, match="trunc"):
        fastnsf.FastNsf(cell=0.3)
    with pytest.raises(ValueError, match="grid_range"):
        fastnsf.FastNsf(point_cloud_range=(-200, -200, -20, 200, 200, 20))
    m = fastnsf.FastNsf(iters=5)
    assert m.eval() is m and m.to("cuda") is m and list(m.parameters()) == [] and m.params["iters"] == 5


# ---- the commands' keys and refusals --------------------------------------------------------------------------------------------------
def test_save_arguments():
    from deflow_amd import fastnsf, save
    opt = save.parse_args(["model=fastnsf", "dataset_path=/d"])
    assert opt["model"] == "fastnsf" and opt["res_name"] == "fastnsf" and opt["checkpoint"] is None
    assert opt["params"] == fastnsf.DEFAULTS and opt["_rest"] == {"batch_size": f"batch_size={fastnsf.COMMAND_BATCH_SIZE}"}
    opt = save.parse_args(["model=fastnsf", "dataset_path=/d", "res_name=r", "fastnsf_iters=4", "fastnsf_cell=0.4", "fastnsf_graph=true", "batch_size=3"])
    assert opt["res_name"] == "r" and opt["params"]["iters"] == 4 and opt["params"]["cell"] == 0.4 and opt["params"]["graph"]
    assert opt["_rest"] == {"batch_size": "batch_size=3"}
    for argv, what in ((["model=fastnsf"], "usage: python -m deflow_amd.save model=fastnsf"),
                       (["model=fastnsf", "dataset_path=/d", "checkpoint=a.ckpt"], "has no weights"),
                       (["model=fastnsf", "dataset_path=/d", "inference_dtype=bf16"], "has no weights"),
                       (["model=fastnsf", "dataset_path=/d", "fastnsf_depth=16"], "depth"),
                       (["model=fastnsf", "dataset_path=/d", "fastnsf_cell=0.3"], "trunc"),
                       (["model=fastnsf", "dataset_path=/d", "fastnsf_iters=many"], "bad value for fastnsf_iters"),
                       (["model=fastnsf", "dataset_path=/d", "fastnsf_width=64"], "unknown key 'fastnsf_width'"),
                       (["model=fastnsf", "dataset_path=/d", "icp_iters=4"], "belong to model=icpflow"),
                       (["model=fastnsf", "dataset_path=/d", "nsfp_iters=4"], "belong to model=nsfp"),
                       (["model=icpflow", "dataset_path=/d", "fastnsf_iters=4"], "belong to model=fastnsf"),
                       (["model=nsfp", "dataset_path=/d", "fastnsf_iters=4"], "belong to model=fastnsf"),
                       (["checkpoint=a.ckpt", "dataset_path=/d", "fastnsf_iters=4"], "belong to model=fastnsf"),
                       (["model=fastnsf", "dataset_path=/d", "av2_mode=test"], "takes no av2_mode")):
        with pytest.raises(SystemExit, match=what):
            save.parse_args(argv)
    # existing invocations are unchanged
    opt = save.parse_args(["checkpoint=/x/best.ckpt", "dataset_path=/d", "model=fastflow3d"])
    assert opt["model"] is None and opt["res_name"] == "best" and opt["_rest"] == {"model": "model=fastflow3d"}
    assert save.parse_args(["model=icpflow", "dataset_path=/d"])["_rest"] == {}
    assert save.parse_args(["model=nsfp", "dataset_path=/d"])["_rest"] == {"batch_size": "batch_size=2"}


def test_eval_and_train_arguments():
    from deflow_amd import eval as ev, pairflow, fastnsf, train
    config = lambda given: pairflow.config(pairflow.entry("fastnsf"), given)
    cfg, params = config({"model": "model=fastnsf", "dataset_path": "dataset_path=/r", "fastnsf_iters": "fastnsf_iters=20"})
    assert cfg["model"] == "fastnsf" and cfg["val_data"] == os.path.join("/r", "val") and cfg["batch_size"] == fastnsf.COMMAND_BATCH_SIZE
    assert params["iters"] == 20 and params["depth"] == 7
    assert config({"model": "model=fastnsf", "batch_size": "batch_size=5"})[0]["batch_size"] == 5
    with pytest.raises(SystemExit, match="no checkpoint="):
        config({"model": "model=fastnsf", "checkpoint": "checkpoint=a.ckpt"})
    with pytest.raises(SystemExit, match="belong to model=icpflow"):
        config({"model": "model=fastnsf", "icp_iters": "icp_iters=2"})
    with pytest.raises(SystemExit, match="belong to model=nsfp"):
        config({"model": "model=fastnsf", "nsfp_iters": "nsfp_iters=2"})
    with pytest.raises(SystemExit, match="patience"):
        config({"model": "model=fastnsf", "fastnsf_patience": "fastnsf_patience=0"})
    with pytest.raises(SystemExit, match="av2_mode=test is out of its scope.*deflow_amd.save model=fastnsf"):
        ev.main(["model=fastnsf", "av2_mode=test", "dataset_path=/r"])
    for argv in (["checkpoint=a.ckpt", "fastnsf_iters=3"], ["model=nsfp", "fastnsf_iters=3"], ["model=icpflow", "fastnsf_iters=3"]):
        with pytest.raises(SystemExit, match="belong to model=fastnsf"):
            ev.main(argv)
    with pytest.raises(SystemExit, match="unknown model 'fastnsf'"):                       # the trainer has nothing to train there
        train.parse_overrides(["model=fastnsf"])
    assert train.split_pseudo_flow(["lr=1e-3", "pseudo_flow=fastnsf"]) == ("fastnsf", ["lr=1e-3"])


def test_pseudo_flow_reads_a_fastnsf_sidecar(tmp_path, golden_dir):
    """what `train ... pseudo_flow=fastnsf` reads: HDF5Dataset(flow_sidecar="fastnsf") on a file written under the command's default res_name"""
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
    path = save.flow_path(str(tmp_path), "scene_a", save.parse_args(["model=fastnsf", f"dataset_path={tmp_path}"])["res_name"])
    assert os.path.basename(path) == "scene_a.fastnsf.flow.npz"
    save.write_flow(path, flows, {"model": "fastnsf"})
    ds = HDF5Dataset(str(tmp_path), flow_sidecar="fastnsf")
    f = ds._file("scene_a")
    for ts in f.sweeps:
        for k in ("flow", "flow_is_valid", "flow_category_indices"):
            f.root[ts].pop(k, None)
    for a, b in zip(items, (ds[i] for i in range(len(ds)))):
        assert np.array_equal(b["flow"].numpy(), flows[str(a["timestamp"])][0]) and bool(b["flow_is_valid"].all())
