"""No GPU: the reference helper of model=floxels (tests/helpers/vox_ref.py) -- the grid, the plan, the field's and the smoothness term's
gradients against finite differences in float64, the transpose identity, the planted case's helper values -- the parameter checks and the
commands' keys and refusals."""
import os
import pickle
import re
import shutil

import numpy as np
import pytest
import torch

from helpers import dt_ref as dr
from helpers import nsfp_ref as nr
from helpers import vox_ref as vr

RANGE = (-6.4, -6.4, -1.6, 6.4, 6.4, 1.6)
# the planted case of section 6n(7) by the committed helper: EPE in float64 and float32 (test_gpu_floxels.py holds the same constants)
PLANTED64, PLANTED32 = 0.06888271436466897, 0.06892478529339785


# ---- the grid and the plan ------------------------------------------------------------------------------------------------------------
def test_grid_dims():
    from deflow_amd import floxels
    default = (-51.2, -51.2, -3, 51.2, 51.2, 3)
    origin, dims = floxels.vox_grid(default, 0.4)
    assert dims == (257, 257, 16) and origin == (dr.f32(-51.2), dr.f32(-51.2), -3.0) and 12 * 257 * 257 * 16 == 12681408
    assert (origin, dims) == vr.grid(default, 0.4)
    # a range the voxel does not divide: the last node lies beyond the range's end; at least 2 nodes per axis
    for rng, voxel, want in (((0, 0, 0, 1.0, 0.9, 0.05), 0.4, (4, 4, 2)), ((-1, -1, -1, 1, 1, 1), 0.3, (8, 8, 8)), (RANGE, 0.4, (33, 33, 9)),
                             (RANGE, 0.5, (27, 27, 8)), ((0, 0, 0, 4.0, 3.0, 2.0), 0.5, (9, 7, 5)), ((0, 0, 0, 1, 1, 1), 5.0, (2, 2, 2))):
        origin, dims = floxels.vox_grid(rng, voxel)
        assert dims == want == vr.grid(rng, voxel)[1], (rng, voxel, dims)
        assert all(origin[a] + voxel * (dims[a] - 1) >= rng[3 + a] - 1e-5 for a in range(3)), "the nodes cover the range"
    for bad, what in (((0, 0, 0, 1, 1), "grid_range"), ((0, 0, 0, 1, 1, float("nan")), "grid_range"), ((0, 0, 0, 1, 0, 1), "grid_range")):
        with pytest.raises(ValueError, match=what):
            floxels.vox_grid(bad, 0.4)
    for bad in (0.0, -0.4, float("inf"), True, "0.4"):
        with pytest.raises(ValueError, match="voxel"):
            floxels.vox_grid(RANGE, bad)
    with pytest.raises(ValueError, match="31 bits"):
        floxels.vox_grid(default, 0.01)


def _case(seed=0, n=90, dims=(6, 5, 4), voxel=0.5):
    """n rows in a small grid: inside cells, on node planes, on the upper faces, outside the range, a NaN row, rows behind the count"""
    rng = np.random.default_rng(seed)
    hi = voxel * (np.array(dims) - 1)
    x = (rng.random((n, 3)) * hi).astype(np.float32)
    x[:6] = np.round(x[:6] / voxel) * voxel                       # on node planes
    x[6:9] = hi                                                    # the upper corner: i = V - 2, t = 1
    x[9] = (-1.0, 0.7, hi[2] + 2)                                  # outside: clamped
    x[10] = (np.nan, 0.2, 0.2)
    return x, n - 7


def test_helper_plan_and_grouping():
    dims, voxel = (6, 5, 4), 0.5
    x, count = _case()
    cell, frac, idx = vr.plan(x, count, (0.0, 0.0, 0.0), voxel, dims)
    NC = vr.n_cells(dims)
    assert NC == 60 and cell.shape == (90,) and frac.dtype == np.float32
    assert (cell[count:] == -1).all() and cell[10] == -1 and not frac[cell < 0].any() and (cell[:count][np.arange(count) != 10] >= 0).all()
    assert (frac >= 0).all() and (frac <= 1).all() and cell.max() < NC
    assert (idx[6:9] == np.array(dims) - 2).all() and (frac[6:9] == 1).all() and cell[6] == NC - 1, "the upper corner"
    assert idx[9].tolist() == [0, 1, 2] and frac[9, 0] == 0 and frac[9, 2] == 1 and abs(frac[9, 1] - 0.4) < 1e-6, "clamped"
    on = np.isin(frac[:6], (0.0, 1.0))
    assert on.all(), "rows on node planes have t = 0 (or 1 at the upper face)"
    # position = origin + voxel (i + t), where the row is inside the range
    inside = cell >= 0
    inside[9] = False
    assert np.abs((idx[inside] + frac[inside]) * voxel - x[inside]).max() < 1e-6
    # grouping of two samples: every participating row once, ascending inside a cell, ranges tile the grouped rows
    cell2 = vr.plan(x[::-1].copy(), 90, (0.0, 0.0, 0.0), voxel, dims)[0]
    idx_sorted, rng2 = vr.grouping([cell, cell2], NC)
    kept = int((cell >= 0).sum() + (cell2 >= 0).sum())
    assert idx_sorted.shape == (180,) and (idx_sorted[kept:] == -1).all() and sorted(idx_sorted[:kept]) == sorted(
        np.concatenate([np.flatnonzero(cell >= 0), 90 + np.flatnonzero(cell2 >= 0)]))
    assert rng2.shape == (2 * NC, 2) and rng2[0, 0] == 0 and rng2[-1, 1] == kept and (rng2[1:, 0] == rng2[:-1, 1]).all()
    both = np.concatenate([cell, cell2])
    for k in range(2 * NC):
        rows = idx_sorted[rng2[k, 0]:rng2[k, 1]]
        assert (np.diff(rows) > 0).all() and (rows // 90 == k // NC).all() and (both[rows] == k % NC).all()
    # active nodes: the corners of the occupied cells; the pair count by brute force
    act, M = vr.active_nodes(cell, dims)
    want = np.zeros((4, 5, 6), bool)
    for c in np.unique(cell[cell >= 0]):
        ix, iy, iz = c % 5, (c // 5) % 4, c // 20
        want[iz:iz + 2, iy:iy + 2, ix:ix + 2] = True
    nodes = np.argwhere(want)
    brute = sum(1 for p in nodes for q in nodes if tuple(q - p) in ((0, 0, 1), (0, 1, 0), (1, 0, 0)))
    assert np.array_equal(act, want) and M == brute > 0
    assert vr.active_nodes(np.full(5, -1), dims)[1] == 0 and vr.n_pairs(np.ones((4, 5, 6), bool)) == 4 * 5 * 5 + 4 * 4 * 6 + 3 * 5 * 6


# ---- the field, its transpose and the term --------------------------------------------------------------------------------------------
def test_helper_field_transpose_and_gradients():
    dims, voxel = (6, 5, 4), 0.5
    x, count = _case(1)
    pl = vr.plan(x, count, (0.0, 0.0, 0.0), voxel, dims)
    gen = torch.Generator().manual_seed(4)
    theta = torch.randn(4, 5, 6, 3, generator=gen, dtype=torch.float64)
    dF = torch.randn(90, 3, generator=gen, dtype=torch.float64)
    dF[count:] = float("nan")                                     # never read
    F = vr.sample(theta, *pl)
    assert not F[pl[0] < 0].any() and float(F.abs().max()) > 0.5
    # a field that is linear in the position is read back exactly (trilinear interpolation reproduces it)
    z, y, xx = torch.meshgrid(torch.arange(4.0), torch.arange(5.0), torch.arange(6.0), indexing="ij")
    lin = torch.stack([xx, y, z], dim=-1).double() * voxel
    inside = pl[0] >= 0
    inside[9] = False
    assert float((vr.sample(lin, *pl)[inside] - torch.from_numpy(x[inside]).double()).abs().max()) < 1e-6
    # <sample(theta), dF> = <theta, scatter(dF)>
    dth = vr.scatter(dF, *pl, dims, torch.float64)
    lhs = float((F[:count] * torch.nan_to_num(dF[:count])).sum())
    assert abs(lhs - float((theta * dth).sum())) <= 1e-12 * max(1.0, abs(lhs)) and abs(lhs) > 1e-3
    act, M = vr.active_nodes(pl[0], dims)
    assert not dth[~torch.from_numpy(act)].any(), "nothing is scattered to an inactive node"
    # the scatter against central differences of <sample(theta), dF>
    keep = torch.from_numpy(pl[0] >= 0)[:, None]
    dFc = torch.where(keep, dF, torch.zeros(1, dtype=torch.float64))
    total = lambda th: float((vr.sample(th, *pl) * dFc).sum())
    h = 1e-6
    nodes = np.argwhere(act)
    for (iz, iy, ix), comp in ((nodes[0], 0), (nodes[len(nodes) // 2], 1), (nodes[-1], 2)):
        up, dn = theta.clone(), theta.clone()
        up[iz, iy, ix, comp] += h
        dn[iz, iy, ix, comp] -= h
        assert abs((total(up) - total(dn)) / (2 * h) - float(dth[iz, iy, ix, comp])) <= 1e-6 * max(1.0, abs(float(dth[iz, iy, ix, comp])))
    # the smoothness term's gradient against central differences; inactive nodes get exactly 0
    v, g = vr.smooth_and_grad(theta, act)
    assert not g[~torch.from_numpy(act)].any() and not v[~torch.from_numpy(act)].any() and float(g.abs().max()) > 1.0 and 0 < act.sum() < act.size
    stot = lambda th: float(vr.smooth_nodes(th, act).sum())
    for (iz, iy, ix), comp in ((nodes[1], 0), (nodes[len(nodes) // 3], 1), (nodes[-2], 2)):
        up, dn = theta.clone(), theta.clone()
        up[iz, iy, ix, comp] += h
        dn[iz, iy, ix, comp] -= h
        assert abs((stot(up) - stot(dn)) / (2 * h) - float(g[iz, iy, ix, comp])) <= 1e-6 * max(1.0, abs(float(g[iz, iy, ix, comp])))
    # the closed form of the GPU test: two active x-neighbours with theta = (0,0,0) and (1,2,2)
    a2 = np.zeros((2, 2, 2), bool)
    a2[0, 0, :] = True
    t2 = torch.zeros(2, 2, 2, 3, dtype=torch.float64)
    t2[0, 0, 1] = torch.tensor([1.0, 2.0, 2.0])
    t2[1, 1, 1] = 7.0                                              # inactive: ignored
    v2, g2 = vr.smooth_and_grad(t2, a2)
    assert float(v2[0, 0, 0]) == 9.0 and float(v2.sum()) == 9.0 and g2[0, 0, 0].tolist() == [-2.0, -4.0, -4.0] and g2[0, 0, 1].tolist() == [2.0, 4.0, 4.0]
    assert vr.n_pairs(a2) == 1 and not g2[1].any()


def test_helper_iteration_loop_and_weight_zero():
    P0, P1, truth = nr.planted_blobs(1, blobs=2, per_blob=30, shift=0.3, spacing=2.5, size=(1.2, 0.8, 0.6))
    origin, dims, R = dr.grid(RANGE, 0.2, 1.0)
    dt2 = dr.edt_dt2(dr.occupancy(P1, origin, dr.f32(0.2), dims), R)
    vo, vd = vr.grid(RANGE, 0.4)
    pl = vr.plan(P0, len(P0), vo, dr.f32(0.4), vd)
    act, M = vr.active_nodes(pl[0], vd)
    x = torch.from_numpy(P0).double()
    gen = torch.Generator().manual_seed(0)
    theta = 0.05 * torch.randn(vd[2], vd[1], vd[0], 3, generator=gen, dtype=torch.float64)
    loss0, (data0, sm0), F0, g0, (gd0, gs0), cells, W0 = vr.iteration(x, dt2, origin, dr.f32(0.2), R, theta, pl, act, M, 0.0)
    # smooth_weight = 0 leaves only the data term: section 6l's mean of the lookup at x + F, and its gradient through the field alone
    d, g, _, _ = dr.lookup(W0, dt2, origin, dr.f32(0.2), R)
    assert float(loss0) == float(data0) == float(d.sum() / len(P0)) and float(sm0) > 0 and not gs0.any() and torch.equal(g0, gd0)
    want = vr.scatter(g / len(P0), *pl, vd, torch.float64)
    assert float((gd0 - want).abs().max()) <= 1e-12 and float(gd0.abs().max()) > 1e-4
    loss, (data, sm), _, g1, (gd, gs), _, _ = vr.iteration(x, dt2, origin, dr.f32(0.2), R, theta, pl, act, M, 10.0, cells=cells)
    assert float(data) == float(data0) and float(sm) == float(sm0) and abs(float(loss) - float(data) - 10 * float(sm)) < 1e-15
    assert torch.equal(gd, gd0) and float(gs.abs().max()) > 0 and not g1[~torch.from_numpy(act)].any()
    flow, best, hist = vr.optimize(x, dt2, origin, dr.f32(0.2), R, torch.zeros_like(theta), pl, act, M, 10.0, 30)
    assert len(hist) == 30 and best < hist[0] and best == min(hist) and flow.shape == x.shape


def test_planted_case_helper_values():
    """section 6n(7): the constants of the GPU test, recomputed with the committed helper.  Zero flow 0.600 m, model=fastnsf's helper
    0.1998 m (section 6l(6))."""
    P0, P1, truth = nr.planted_blobs(2, blobs=4, per_blob=200, shift=0.6, spacing=2.5, size=(1.2, 0.8, 0.6))
    from deflow_amd import floxels
    D = floxels.DEFAULTS
    origin, dims, R = dr.grid(RANGE, D["cell"], D["trunc"])
    cell = dr.f32(D["cell"])
    dt2 = dr.edt_dt2(dr.occupancy(P1, origin, cell, dims), R)
    vo, vd = vr.grid(RANGE, D["voxel"])
    pl = vr.plan(P0, len(P0), vo, dr.f32(D["voxel"]), vd)
    act, M = vr.active_nodes(pl[0], vd)
    got = {}
    for dt in (torch.float64, torch.float32):
        theta = torch.zeros(vd[2], vd[1], vd[0], 3, dtype=dt)
        flow, best, hist = vr.optimize(torch.from_numpy(P0).to(dt), dt2, origin, cell, R, theta, pl, act, M, D["smooth_weight"], 200, lr=D["lr"],
                                       patience=D["patience"], min_delta=D["min_delta"])
        got[dt] = float(np.linalg.norm(flow.double().numpy() - truth, axis=1).mean())
        print(dt, "EPE", repr(got[dt]), "best", best, "iterations", len(hist))
    assert abs(got[torch.float64] - PLANTED64) <= 1e-9 and abs(got[torch.float32] - PLANTED32) <= 1e-3 * PLANTED32
    assert PLANTED64 <= 0.6 / 2 and max(PLANTED64, PLANTED32) <= 1.5 * min(PLANTED64, PLANTED32) and 2 * PLANTED64 < 0.1998


# ---- the parameters -------------------------------------------------------------------------------------------------------------------
def test_check_params_and_keys():
    from deflow_amd import fastnsf, floxels, mbnsf, nsfp
    assert floxels.check_params({}) == floxels.DEFAULTS == {"voxel": 0.4, "smooth_weight": 10.0, "iters": 1000, "lr": 0.05, "cell": 0.1,
                                                            "trunc": 2.0, "patience": 100, "min_delta": 1e-4, "check_every": 50, "graph": False}
    assert floxels.COMMAND_BATCH_SIZE == 4 and "depth" not in floxels.DEFAULTS and "seed" not in floxels.DEFAULTS
    got = floxels.check_params({"smooth_weight": 0, "voxel": 1, "iters": 3.0, "cell": 0.4, "graph": True})
    assert got["smooth_weight"] == 0.0 and got["voxel"] == 1.0 and got["iters"] == 3 and isinstance(got["iters"], int) and got["graph"] is True
    for bad, what in (({"smooth_weight": -1.0}, "smooth_weight"), ({"smooth_weight": float("inf")}, "smooth_weight"),
                      ({"smooth_weight": float("nan")}, "smooth_weight"), ({"smooth_weight": True}, "smooth_weight"),
                      ({"voxel": 0.0}, "voxel"), ({"voxel": float("inf")}, "voxel"), ({"voxel": "0.4"}, "voxel"), ({"lr": 0}, "lr"),
                      ({"iters": 0}, "iters"), ({"iters": 2.5}, "iters"), ({"patience": 0}, "patience"), ({"check_every": -1}, "check_every"),
                      ({"min_delta": -1e-4}, "min_delta"), ({"cell": 0.3}, "trunc"), ({"graph": 1}, "graph"),
                      ({"depth": 2}, "unknown parameter 'depth'"), ({"seed": 1}, "unknown parameter 'seed'"),
                      ({"rigid_weight": 1.0}, "unknown parameter")):
        with pytest.raises(ValueError, match=what):
            floxels.check_params(bad)
    assert set(floxels.COMMAND_KEYS) == {"floxels_" + k for k in floxels.DEFAULTS} and len(floxels.COMMAND_KEYS) == 10
    assert floxels.COMMAND_KEYS["floxels_smooth_weight"] == "smooth_weight" and floxels.COMMAND_KEYS["floxels_voxel"] == "voxel"
    p = floxels.params_from_command({"floxels_graph": "true", "floxels_smooth_weight": "2.5", "floxels_voxel": "0.8"})
    assert p["graph"] is True and p["smooth_weight"] == 2.5 and p["voxel"] == 0.8
    with pytest.raises(SystemExit, match="bad value for floxels_iters"):
        floxels.params_from_command({"floxels_iters": "many"})
    with pytest.raises(SystemExit, match="bad value among the floxels_\\* keys.*voxel"):
        floxels.params_from_command({"floxels_voxel": "-1"})
    # the estimators this one is built beside keep their keys
    others = set(fastnsf.COMMAND_KEYS) | set(mbnsf.COMMAND_KEYS) | set(nsfp.COMMAND_KEYS)
    assert not set(floxels.COMMAND_KEYS) & others and len(fastnsf.DEFAULTS) == 10 and len(mbnsf.DEFAULTS) == 17
    # CPU tensors are refused by name
    x, c = torch.zeros(1, 4, 3), torch.zeros(1, dtype=torch.int32)
    th = torch.zeros(1, 2, 2, 2, 3)
    with pytest.raises(TypeError, match="x must be a CUDA tensor"):
        floxels.vox_plan(x, c, origin=(0, 0, 0), voxel=0.5, dims=(2, 2, 2))
    with pytest.raises(TypeError, match="theta must be a CUDA tensor"):
        floxels.vox_sample(th, torch.zeros(1, 4, dtype=torch.int32), x)
    with pytest.raises(TypeError, match="dF must be a CUDA tensor"):
        floxels.vox_scatter(x, x, torch.zeros(4, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32), dims=(2, 2, 2))
    with pytest.raises(TypeError, match="theta must be a CUDA tensor"):
        floxels.vox_smooth(th, torch.zeros(1, 8, dtype=torch.uint8))
    with pytest.raises(TypeError, match="pc0s must be a CUDA tensor"):
        floxels.floxels_optimize(x, c, x, c, grid_range=(-1, -1, -1, 1, 1, 1))
    with pytest.raises(ValueError, match="voxel_size"):
        floxels.Floxels(voxel_size=(0.2, 0.2))
    with pytest.raises(ValueError, match="smooth_weight"):
        floxels.Floxels(smooth_weight=-1)
    with pytest.raises(ValueError, match="grid_range"):
        floxels.Floxels(point_cloud_range=(-200, -200, -20, 200, 200, 20))
    with pytest.raises(ValueError, match="31 bits"):
        floxels.Floxels(voxel=0.01)
    m = floxels.Floxels(iters=5, smooth_weight=1.0)
    assert m.eval() is m and m.to("cuda") is m and list(m.parameters()) == [] and m.params["iters"] == 5 and m.params["smooth_weight"] == 1.0
    # the optimiser uses no autograd and no net, and the loop, its Adam call and its graph capture are pairopt's, imported and not copied
    src = open(floxels.__file__).read()
    assert "requires_grad" not in src and ".backward(" not in src and "mlp_forward" not in src and "from .pairopt import" in src
    assert "df_adam_step_dev" not in src and "torch.cuda.graph" not in src and "CUDAGraph" not in src
    assert re.search(r"def \w*(snapshot|freeze|run)\w*\(", src) is None


# ---- the commands' keys and refusals --------------------------------------------------------------------------------------------------
def test_save_arguments():
    from deflow_amd import floxels, save
    opt = save.parse_args(["model=floxels", "dataset_path=/d"])
    assert opt["model"] == "floxels"
    assert opt["res_name"] == "floxels" and opt["checkpoint"] is None
    assert opt["params"] == floxels.DEFAULTS and opt["_rest"] == {"batch_size": f"batch_size={floxels.COMMAND_BATCH_SIZE}"}
    opt = save.parse_args(["model=floxels", "dataset_path=/d", "res_name=r", "floxels_iters=4", "floxels_smooth_weight=3", "floxels_graph=true",
                           "batch_size=3"])
    assert opt["res_name"] == "r" and opt["params"]["iters"] == 4 and opt["params"]["smooth_weight"] == 3.0
    assert opt["params"]["graph"] and opt["_rest"] == {"batch_size": "batch_size=3"}
    for argv, what in ((["model=floxels"], "usage: python -m deflow_amd.save model=floxels"),
                       (["model=floxels", "dataset_path=/d", "checkpoint=a.ckpt"], "has no weights"),
                       (["model=floxels", "dataset_path=/d", "inference_dtype=bf16"], "has no weights"),
                       (["model=floxels", "dataset_path=/d", "floxels_voxel=0"], "voxel"),
                       (["model=floxels", "dataset_path=/d", "floxels_smooth_weight=-1"], "smooth_weight"),
                       (["model=floxels", "dataset_path=/d", "floxels_cell=0.3"], "trunc"),
                       (["model=floxels", "dataset_path=/d", "floxels_iters=many"], "bad value for floxels_iters"),
                       (["model=floxels", "dataset_path=/d", "floxels_depth=2"], "unknown key 'floxels_depth'"),
                       (["model=floxels", "dataset_path=/d", "icp_iters=4"], "belong to model=icpflow"),
                       (["model=floxels", "dataset_path=/d", "nsfp_iters=4"], "belong to model=nsfp"),
                       (["model=floxels", "dataset_path=/d", "fastnsf_iters=4"], "belong to model=fastnsf"),
                       (["model=floxels", "dataset_path=/d", "mbnsf_rigid_weight=4"], "belong to model=mbnsf"),
                       (["model=icpflow", "dataset_path=/d", "floxels_iters=4"], "belong to model=floxels"),
                       (["model=nsfp", "dataset_path=/d", "floxels_iters=4"], "belong to model=floxels"),
                       (["model=fastnsf", "dataset_path=/d", "floxels_voxel=0.8"], "belong to model=floxels"),
                       (["model=mbnsf", "dataset_path=/d", "floxels_voxel=0.8"], "belong to model=floxels"),
                       (["checkpoint=a.ckpt", "dataset_path=/d", "floxels_iters=4"], "belong to model=floxels"),
                       (["model=floxels", "dataset_path=/d", "av2_mode=test"], "takes no av2_mode")):
        with pytest.raises(SystemExit, match=what):
            save.parse_args(argv)
    # existing invocations are unchanged
    opt = save.parse_args(["checkpoint=/x/best.ckpt", "dataset_path=/d", "model=fastflow3d"])
    assert opt["model"] is None and opt["res_name"] == "best" and opt["_rest"] == {"model": "model=fastflow3d"}
    assert save.parse_args(["model=icpflow", "dataset_path=/d"])["_rest"] == {}
    assert save.parse_args(["model=nsfp", "dataset_path=/d"])["_rest"] == {"batch_size": "batch_size=2"}
    assert save.parse_args(["model=fastnsf", "dataset_path=/d"])["res_name"] == "fastnsf"
    assert save.parse_args(["model=mbnsf", "dataset_path=/d"])["res_name"] == "mbnsf"


def test_eval_and_train_arguments():
    from deflow_amd import eval as ev, pairflow, floxels, train
    config = lambda given: pairflow.config(pairflow.entry("floxels"), given)
    cfg, params = config({"model": "model=floxels", "dataset_path": "dataset_path=/r", "floxels_iters": "floxels_iters=20"})
    assert cfg["model"] == "floxels" and cfg["val_data"] == os.path.join("/r", "val") and cfg["batch_size"] == floxels.COMMAND_BATCH_SIZE
    assert params["iters"] == 20 and params["voxel"] == 0.4 and params["smooth_weight"] == 10.0
    assert config({"model": "model=floxels", "batch_size": "batch_size=5"})[0]["batch_size"] == 5
    with pytest.raises(SystemExit, match="no checkpoint="):
        config({"model": "model=floxels", "checkpoint": "checkpoint=a.ckpt"})
    with pytest.raises(SystemExit, match="no inference_dtype="):
        config({"model": "model=floxels", "inference_dtype": "inference_dtype=bf16"})
    for key, owner in (("icp_iters", "icpflow"), ("nsfp_iters", "nsfp"), ("fastnsf_iters", "fastnsf"), ("mbnsf_iters", "mbnsf")):
        with pytest.raises(SystemExit, match=f"{key}: the {key.split('_')[0]}_\\* keys belong to model={owner}"):
            config({"model": "model=floxels", key: f"{key}=2"})
    with pytest.raises(SystemExit, match="voxel"):
        config({"model": "model=floxels", "floxels_voxel": "floxels_voxel=0"})
    with pytest.raises(SystemExit, match="model=floxels writes no leaderboard submission \\(av2_mode=test is out of its scope\\).*deflow_amd.save model=floxels"):
        ev.main(["model=floxels", "av2_mode=test", "dataset_path=/r"])
    for argv in (["checkpoint=a.ckpt", "floxels_iters=3"], ["model=nsfp", "floxels_iters=3"], ["model=icpflow", "floxels_iters=3"],
                 ["model=fastnsf", "floxels_voxel=0.8"], ["model=mbnsf", "floxels_smooth_weight=3"]):
        with pytest.raises(SystemExit, match="belong to model=floxels"):
            ev.main(argv)
    for argv, what in ((["model=floxels", "mbnsf_iters=3"], "belong to model=mbnsf"), (["model=floxels", "fastnsf_iters=3"], "belong to model=fastnsf"),
                       (["model=floxels", "nsfp_iters=3"], "belong to model=nsfp"), (["model=floxels", "icp_iters=3"], "belong to model=icpflow"),
                       (["model=floxels", "checkpoint=a.ckpt"], "has no weights")):
        with pytest.raises(SystemExit, match=what):
            ev.main(argv)
    with pytest.raises(SystemExit, match="model=floxels"):                                  # the usage text names the new command
        ev.main([])
    with pytest.raises(SystemExit, match="unknown model 'floxels'"):                       # the trainer has nothing to train there
        train.parse_overrides(["model=floxels"])
    assert train.split_pseudo_flow(["lr=1e-3", "pseudo_flow=floxels"]) == ("floxels", ["lr=1e-3"])


def test_pseudo_flow_reads_a_floxels_sidecar(tmp_path, golden_dir):
    """what `train ... pseudo_flow=floxels` reads: HDF5Dataset(flow_sidecar="floxels") on a file written under the command's default res_name"""
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
    rng = np.random.default_rng(7)
    flows = {str(it["timestamp"]): (rng.standard_normal((it["pc0"].shape[0], 3)).astype(np.float32), np.zeros(it["pc0"].shape[0], np.uint8))
             for it in items}
    path = save.flow_path(str(tmp_path), "scene_a", save.parse_args(["model=floxels", f"dataset_path={tmp_path}"])["res_name"])
    assert os.path.basename(path) == "scene_a.floxels.flow.npz"
    save.write_flow(path, flows, {"model": "floxels"})
    ds = HDF5Dataset(str(tmp_path), flow_sidecar="floxels")
    f = ds._file("scene_a")
    for ts in f.sweeps:
        for k in ("flow", "flow_is_valid", "flow_category_indices"):
            f.root[ts].pop(k, None)
    for a, b in zip(items, (ds[i] for i in range(len(ds)))):
        assert np.array_equal(b["flow"].numpy(), flows[str(a["timestamp"])][0]) and bool(b["flow_is_valid"].all())
