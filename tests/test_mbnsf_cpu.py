"""No GPU: the reference helper of model=mbnsf (tests/helpers/iso_ref.py) -- the stride rule, the neighbour table, the term's gradient
against finite differences in float64 -- the parameter checks and the commands' keys and refusals."""
import os
import pickle
import re
import shutil

import numpy as np
import pytest
import torch

from helpers import dt_ref as dr
from helpers import iso_ref as ir
from helpers import nsfp_ref as nr


# ---- the helper -----------------------------------------------------------------------------------------------------------------------
def test_stride_rule():
    for n in range(2, 41):
        for P in range(1, 17):
            s = ir.strides(n, P)
            assert len(s) == P and s[0] == 1 and all(1 <= v <= n - 1 for v in s) and s == sorted(s), (n, P, s)
    assert ir.strides(2, 4) == [1, 1, 1, 1] and ir.strides(9, 4) == [1, 3, 5, 7] and ir.strides(257, 4) == [1, 65, 129, 193]
    assert ir.strides(5, 16)[-1] == 4 and ir.strides(40, 1) == [1]


def _interleaved(N, sizes, seed):
    """labels [N]: cluster l (1-based) has sizes[l - 1] rows, scattered over the rows (the clusters interleave); the rest is 0"""
    rng = np.random.default_rng(seed)
    labels = np.zeros(N, np.int32)
    rows = rng.permutation(N)[:sum(sizes)]
    o = 0
    for l, n in enumerate(sizes, start=1):
        labels[rows[o:o + n]] = l
        o += n
    return labels


@pytest.mark.parametrize("P", [1, 3, 4, 16])
def test_tables_are_each_others_inverse_and_count_the_instances(P):
    sizes = [1, 2, 3, P, P + 1, 40, 70, 23]
    labels = _interleaved(300, sizes, 5 + P)
    count, cap = 260, 64
    nbr, M = ir.table(labels, count, P, cap)
    L = ir.lists(labels, count)
    eligible = {l: r for l, r in L.items() if 2 <= len(r) <= cap}
    assert all(r.max() < count and (np.diff(r) > 0).all() for r in L.values()) and int((labels[count:] > 0).sum()) > 0   # rows behind the count left the lists
    assert M == P * sum(len(r) for r in eligible.values()) and M > 0
    with_partners = np.flatnonzero((nbr >= 0).all(axis=1))
    assert np.array_equal(with_partners, np.sort(np.concatenate(list(eligible.values())))) and ((nbr >= 0).all(axis=1) | (nbr < 0).all(axis=1)).all()
    assert (nbr[count:] == -1).all() and (nbr[labels == 0] == -1).all() and nbr.max() < count
    for a in with_partners:
        for k in range(P):
            assert nbr[nbr[a, k], P + k] == a and nbr[nbr[a, P + k], k] == a            # the k-th backward partner: whose k-th forward partner a is
            assert labels[nbr[a, k]] == labels[a] and nbr[a, k] != a
    # the forward half lists every instance once: as many as the backward half, pair by pair
    fwd = sorted((int(a), int(nbr[a, k]), k) for a in with_partners for k in range(P))
    bwd = sorted((int(nbr[a, P + k]), int(a), k) for a in with_partners for k in range(P))
    assert fwd == bwd and len(fwd) == M
    # a list in ascending order: position i's first forward partner is the next row of the cluster, cyclically
    for r in eligible.values():
        assert np.array_equal(nbr[r, 0], np.roll(r, -1)) and np.array_equal(nbr[r, P], np.roll(r, 1))
    assert ir.table(labels, 0, P, cap)[1] == 0 and ir.table(labels, count, P, 2)[1] == 2 * P * sum(len(r) == 2 for r in L.values())
    assert ir.table(labels, count, P, cap, kcap=2)[1] == P * sum(len(r) for l, r in eligible.items() if l <= 2)


def test_helper_term_and_gradient():
    gen = torch.Generator().manual_seed(2)
    labels = _interleaved(120, [2, 30, 50], 1)
    nbr, M = ir.table(labels, 120, 4, 64)
    x = torch.rand(120, 3, generator=gen, dtype=torch.float64) * 2
    r0 = ir.rest(x, nbr)
    assert bool((r0[torch.as_tensor(nbr) < 0] == 0).all()) and float(r0.max()) > 1.0
    W = x + 0.15 * torch.randn(120, 3, generator=gen, dtype=torch.float64)
    delta = 0.1
    v, g, e = ir.term_and_grad(W, nbr, r0, delta)
    frac = float((e[torch.as_tensor(nbr[:, :4]) >= 0] > delta).double().mean())
    assert 0.1 < frac < 0.9, frac                                                         # both branches of rho
    assert not g[labels == 0].any() and not v[labels == 0].any() and float(g.abs().max()) > 0.1
    # torch.autograd against central differences of the summed term
    total = lambda w: float(ir.term(w, nbr, r0, delta)[0].sum())
    h = 1e-6
    for row, axis in ((int(np.flatnonzero(labels == 1)[0]), 0), (int(np.flatnonzero(labels == 2)[3]), 1), (int(np.flatnonzero(labels == 3)[7]), 2)):
        up, dn = W.clone(), W.clone()
        up[row, axis] += h
        dn[row, axis] -= h
        assert abs((total(up) - total(dn)) / (2 * h) - float(g[row, axis])) <= 1e-6 * max(1.0, abs(float(g[row, axis])))
    # rho: value and slope are continuous at delta; the 2-row cluster's gradients are opposite
    d = torch.tensor([delta - 1e-9, delta + 1e-9], dtype=torch.float64)
    r = ir.rho(d, torch.tensor(delta, dtype=torch.float64))
    assert abs(float(r[1] - r[0])) < 1e-9 and abs(float((r[1] - r[0]) / 2e-9) - 2 * delta) < 1e-6
    two = np.flatnonzero(labels == 1)
    assert float((g[two[0]] + g[two[1]]).abs().max()) < 1e-12 and float(g[two[0]].abs().max()) > 0
    # two partners on one point: the value counts, the gradient is 0 (and finite)
    W2 = W.clone()
    W2[two[1]] = W2[two[0]]
    v2, g2, e2 = ir.term_and_grad(W2, nbr, r0, delta)
    assert bool(torch.isfinite(g2).all()) and not g2[two].any() and float(e2[two[0], 0]) == float(r0[two[0], 0])
    assert abs(float(v2[two[0]]) - 4 * float(ir.rho(r0[two[0], 0], torch.tensor(delta, dtype=torch.float64)))) < 1e-12
    # the closed form of the GPU test: 1 m apart at rest, 2 m apart warped, delta 0.25
    xa = torch.tensor([[0.0, 0, 0], [1.0, 0, 0]], dtype=torch.float64)
    n2, M2 = ir.table(np.array([1, 1]), 2, 4, 64)
    v3, g3, _ = ir.term_and_grad(xa * 2, n2, ir.rest(xa, n2), 0.25)
    assert M2 == 8 and v3.tolist() == [4 * 0.25 * 1.75] * 2 and g3.tolist() == [[-4.0, 0, 0], [4.0, 0, 0]]


def test_helper_iteration_and_loop():
    P0, P1, truth = nr.planted_blobs(1, blobs=2, per_blob=30, shift=0.3, spacing=2.5, size=(1.2, 0.8, 0.6))
    origin, dims, R = dr.grid((-6.4, -6.4, -1.6, 6.4, 6.4, 1.6), 0.2, 1.0)
    dt2 = dr.edt_dt2(dr.occupancy(P1, origin, dr.f32(0.2), dims), R)
    from deflow_amd import nsfp
    f = nsfp.init_params(1, 0)[0, :nr.num_params(1)].double()
    nbr, M = ir.table(np.repeat([1, 2], 30), 60, 4, 8192)
    x = torch.from_numpy(P0).double()
    loss0, _, F0, df0, cells, _ = ir.iteration(x, dt2, origin, dr.f32(0.2), R, f, 1, nbr, M, 0.0, 0.2)
    ref = dr.iteration(x, dt2, origin, dr.f32(0.2), R, f, 1)
    assert float(loss0) == float(ref[0]) and torch.equal(df0, ref[2]) and torch.equal(F0, ref[1]), "weight 0 is section 6l's iteration"
    loss, (data, iso), _, df, _, _ = ir.iteration(x, dt2, origin, dr.f32(0.2), R, f, 1, nbr, M, 10.0, 0.2, cells=cells)
    assert float(data) == float(loss0) and float(iso) > 0 and abs(float(loss) - float(data) - 10 * float(iso)) < 1e-15 and not torch.equal(df, df0)
    flow, best, hist = ir.optimize(x, dt2, origin, dr.f32(0.2), R, f, 1, 30, nbr, M, 10.0, 0.2)
    assert len(hist) == 30 and best < hist[0] and best == min(hist)
    assert ir.same_partition([0, 3, 3, 1], [0, 1, 1, 2]) and not ir.same_partition([0, 3, 3, 1], [0, 1, 2, 2]) and not ir.same_partition([0, 1], [1, 1])


# ---- the parameters -------------------------------------------------------------------------------------------------------------------
def test_check_params_and_keys():
    from deflow_amd import fastnsf, mbnsf
    assert mbnsf.check_params({}) == mbnsf.DEFAULTS == dict(fastnsf.DEFAULTS, rigid_weight=10.0, rigid_pairs=4, rigid_delta=0.2, eps=0.7,
                                                            min_points=4, min_cluster_size=20, max_cluster_points=8192)
    assert list(mbnsf.DEFAULTS)[:10] == list(fastnsf.DEFAULTS) and mbnsf.COMMAND_BATCH_SIZE == 4
    got = mbnsf.check_params({"rigid_weight": 0, "rigid_pairs": 16.0, "iters": 3.0, "cell": 0.4, "graph": True})
    assert got["rigid_weight"] == 0.0 and got["rigid_pairs"] == 16 and got["iters"] == 3 and isinstance(got["rigid_pairs"], int)
    for bad, what in (({"rigid_weight": -1.0}, "rigid_weight"), ({"rigid_weight": float("inf")}, "rigid_weight"),
                      ({"rigid_weight": float("nan")}, "rigid_weight"), ({"rigid_weight": True}, "rigid_weight"),
                      ({"rigid_pairs": 0}, "rigid_pairs"), ({"rigid_pairs": 17}, "rigid_pairs"), ({"rigid_pairs": 2.5}, "rigid_pairs"),
                      ({"rigid_delta": 0.0}, "rigid_delta"), ({"rigid_delta": float("inf")}, "rigid_delta"), ({"eps": -0.7}, "eps"),
                      ({"min_points": 0}, "min_points"), ({"min_cluster_size": 0}, "min_cluster_size"),
                      ({"max_cluster_points": 0}, "max_cluster_points"), ({"depth": 16}, "mbnsf_optimize: depth"), ({"cell": 0.3}, "trunc"),
                      ({"graph": 1}, "graph"), ({"trunc_d2": 4.0}, "unknown parameter 'trunc_d2'"), ({"vote_bin": 0.2}, "unknown parameter")):
        with pytest.raises(ValueError, match=what):
            mbnsf.check_params(bad)
    assert set(mbnsf.COMMAND_KEYS) == {"mbnsf_" + k for k in mbnsf.DEFAULTS} and len(mbnsf.COMMAND_KEYS) == 17
    assert mbnsf.COMMAND_KEYS["mbnsf_rigid_weight"] == "rigid_weight" and mbnsf.COMMAND_KEYS["mbnsf_eps"] == "eps"
    p = mbnsf.params_from_command({"mbnsf_graph": "true", "mbnsf_rigid_weight": "2.5", "mbnsf_rigid_pairs": "8"})
    assert p["graph"] is True and p["rigid_weight"] == 2.5 and p["rigid_pairs"] == 8
    with pytest.raises(SystemExit, match="bad value for mbnsf_iters"):
        mbnsf.params_from_command({"mbnsf_iters": "many"})
    with pytest.raises(SystemExit, match="bad value among the mbnsf_\\* keys.*rigid_pairs"):
        mbnsf.params_from_command({"mbnsf_rigid_pairs": "17"})
    assert mbnsf.kcap(700, 20) == 35 and mbnsf.kcap(5, 20) == 1
    # the estimators this one is built beside keep their keys
    assert not set(mbnsf.COMMAND_KEYS) & (set(fastnsf.COMMAND_KEYS)) and len(fastnsf.DEFAULTS) == 10
    # CPU tensors are refused by name
    x, c, l = torch.zeros(1, 4, 3), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32)
    with pytest.raises(TypeError, match="x must be a CUDA tensor"):
        mbnsf.iso_plan(x, c, l, pairs=4, max_cluster_points=64)
    with pytest.raises(TypeError, match="w must be a CUDA tensor"):
        mbnsf.iso_pairs(x, torch.zeros(1, 4, 8, dtype=torch.int32), torch.zeros(1, 4, 8), delta=0.2)
    with pytest.raises(TypeError, match="pc0s must be a CUDA tensor"):
        mbnsf.mbnsf_optimize(x, c, x, c, grid_range=(-1, -1, -1, 1, 1, 1))
    with pytest.raises(ValueError, match="voxel_size"):
        mbnsf.MbNsf(voxel_size=(0.2, 0.2))
    with pytest.raises(ValueError, match="rigid_pairs"):
        mbnsf.MbNsf(rigid_pairs=0)
    with pytest.raises(ValueError, match="grid_range"):
        mbnsf.MbNsf(point_cloud_range=(-200, -200, -20, 200, 200, 20))
    m = mbnsf.MbNsf(iters=5, rigid_weight=1.0)
    assert m.eval() is m and m.to("cuda") is m and list(m.parameters()) == [] and m.params["iters"] == 5 and m.params["rigid_weight"] == 1.0
    # nothing of the term leaves the estimator's own module: the optimiser uses no autograd, and the loop, its Adam call and its graph
    # capture are pairopt's, imported and not copied
    src = open(mbnsf.__file__).read()
    assert "requires_grad" not in src and ".backward(" not in src and "from .pairopt import" in src
    assert "df_adam_step_dev" not in src and "torch.cuda.graph" not in src and "CUDAGraph" not in src
    assert re.search(r"def \w*(snapshot|freeze|run)\w*\(", src) is None


# ---- the commands' keys and refusals --------------------------------------------------------------------------------------------------
def test_save_arguments():
    from deflow_amd import mbnsf, save
    opt = save.parse_args(["model=mbnsf", "dataset_path=/d"])
    assert opt["model"] == "mbnsf" and opt["res_name"] == "mbnsf" and opt["checkpoint"] is None
    assert opt["params"] == mbnsf.DEFAULTS and opt["_rest"] == {"batch_size": f"batch_size={mbnsf.COMMAND_BATCH_SIZE}"}
    opt = save.parse_args(["model=mbnsf", "dataset_path=/d", "res_name=r", "mbnsf_iters=4", "mbnsf_rigid_weight=3", "mbnsf_graph=true", "batch_size=3"])
    assert opt["res_name"] == "r" and opt["params"]["iters"] == 4 and opt["params"]["rigid_weight"] == 3.0 and opt["params"]["graph"]
    assert opt["_rest"] == {"batch_size": "batch_size=3"}
    for argv, what in ((["model=mbnsf"], "usage: python -m deflow_amd.save model=mbnsf"),
                       (["model=mbnsf", "dataset_path=/d", "checkpoint=a.ckpt"], "has no weights"),
                       (["model=mbnsf", "dataset_path=/d", "inference_dtype=bf16"], "has no weights"),
                       (["model=mbnsf", "dataset_path=/d", "mbnsf_rigid_pairs=17"], "rigid_pairs"),
                       (["model=mbnsf", "dataset_path=/d", "mbnsf_rigid_weight=-1"], "rigid_weight"),
                       (["model=mbnsf", "dataset_path=/d", "mbnsf_cell=0.3"], "trunc"),
                       (["model=mbnsf", "dataset_path=/d", "mbnsf_iters=many"], "bad value for mbnsf_iters"),
                       (["model=mbnsf", "dataset_path=/d", "mbnsf_width=64"], "unknown key 'mbnsf_width'"),
                       (["model=mbnsf", "dataset_path=/d", "icp_iters=4"], "belong to model=icpflow"),
                       (["model=mbnsf", "dataset_path=/d", "nsfp_iters=4"], "belong to model=nsfp"),
                       (["model=mbnsf", "dataset_path=/d", "fastnsf_iters=4"], "belong to model=fastnsf"),
                       (["model=icpflow", "dataset_path=/d", "mbnsf_iters=4"], "belong to model=mbnsf"),
                       (["model=nsfp", "dataset_path=/d", "mbnsf_iters=4"], "belong to model=mbnsf"),
                       (["model=fastnsf", "dataset_path=/d", "mbnsf_rigid_weight=4"], "belong to model=mbnsf"),
                       (["checkpoint=a.ckpt", "dataset_path=/d", "mbnsf_iters=4"], "belong to model=mbnsf"),
                       (["model=mbnsf", "dataset_path=/d", "av2_mode=test"], "takes no av2_mode")):
        with pytest.raises(SystemExit, match=what):
            save.parse_args(argv)
    # existing invocations are unchanged
    opt = save.parse_args(["checkpoint=/x/best.ckpt", "dataset_path=/d", "model=fastflow3d"])
    assert opt["model"] is None and opt["res_name"] == "best" and opt["_rest"] == {"model": "model=fastflow3d"}
    assert save.parse_args(["model=icpflow", "dataset_path=/d"])["_rest"] == {}
    assert save.parse_args(["model=nsfp", "dataset_path=/d"])["_rest"] == {"batch_size": "batch_size=2"}
    assert save.parse_args(["model=fastnsf", "dataset_path=/d"])["res_name"] == "fastnsf"


def test_eval_and_train_arguments():
    from deflow_amd import eval as ev, pairflow, mbnsf, train
    config = lambda given: pairflow.config(pairflow.entry("mbnsf"), given)
    cfg, params = config({"model": "model=mbnsf", "dataset_path": "dataset_path=/r", "mbnsf_iters": "mbnsf_iters=20"})
    assert cfg["model"] == "mbnsf" and cfg["val_data"] == os.path.join("/r", "val") and cfg["batch_size"] == mbnsf.COMMAND_BATCH_SIZE
    assert params["iters"] == 20 and params["depth"] == 7 and params["rigid_weight"] == 10.0
    assert config({"model": "model=mbnsf", "batch_size": "batch_size=5"})[0]["batch_size"] == 5
    with pytest.raises(SystemExit, match="no checkpoint="):
        config({"model": "model=mbnsf", "checkpoint": "checkpoint=a.ckpt"})
    with pytest.raises(SystemExit, match="no inference_dtype="):
        config({"model": "model=mbnsf", "inference_dtype": "inference_dtype=bf16"})
    with pytest.raises(SystemExit, match="icp_iters: the icp_\\* keys belong to model=icpflow"):
        config({"model": "model=mbnsf", "icp_iters": "icp_iters=2"})
    with pytest.raises(SystemExit, match="nsfp_iters: the nsfp_\\* keys belong to model=nsfp"):
        config({"model": "model=mbnsf", "nsfp_iters": "nsfp_iters=2"})
    with pytest.raises(SystemExit, match="fastnsf_iters: the fastnsf_\\* keys belong to model=fastnsf"):
        config({"model": "model=mbnsf", "fastnsf_iters": "fastnsf_iters=2"})
    with pytest.raises(SystemExit, match="rigid_delta"):
        config({"model": "model=mbnsf", "mbnsf_rigid_delta": "mbnsf_rigid_delta=0"})
    with pytest.raises(SystemExit, match="model=mbnsf writes no leaderboard submission \\(av2_mode=test is out of its scope\\).*deflow_amd.save model=mbnsf"):
        ev.main(["model=mbnsf", "av2_mode=test", "dataset_path=/r"])
    for argv in (["checkpoint=a.ckpt", "mbnsf_iters=3"], ["model=nsfp", "mbnsf_iters=3"], ["model=icpflow", "mbnsf_iters=3"],
                 ["model=fastnsf", "mbnsf_rigid_weight=3"]):
        with pytest.raises(SystemExit, match="belong to model=mbnsf"):
            ev.main(argv)
    for argv, what in ((["model=mbnsf", "fastnsf_iters=3"], "belong to model=fastnsf"), (["model=mbnsf", "nsfp_iters=3"], "belong to model=nsfp"),
                       (["model=mbnsf", "icp_iters=3"], "belong to model=icpflow"), (["model=mbnsf", "checkpoint=a.ckpt"], "has no weights")):
        with pytest.raises(SystemExit, match=what):
            ev.main(argv)
    with pytest.raises(SystemExit, match="unknown model 'mbnsf'"):                         # the trainer has nothing to train there
        train.parse_overrides(["model=mbnsf"])
    assert train.split_pseudo_flow(["lr=1e-3", "pseudo_flow=mbnsf"]) == ("mbnsf", ["lr=1e-3"])


def test_pseudo_flow_reads_a_mbnsf_sidecar(tmp_path, golden_dir):
    """what `train ... pseudo_flow=mbnsf` reads: HDF5Dataset(flow_sidecar="mbnsf") on a file written under the command's default res_name"""
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
    rng = np.random.default_rng(6)
    flows = {str(it["timestamp"]): (rng.standard_normal((it["pc0"].shape[0], 3)).astype(np.float32), np.zeros(it["pc0"].shape[0], np.uint8))
             for it in items}
    path = save.flow_path(str(tmp_path), "scene_a", save.parse_args(["model=mbnsf", f"dataset_path={tmp_path}"])["res_name"])
    assert os.path.basename(path) == "scene_a.mbnsf.flow.npz"
    save.write_flow(path, flows, {"model": "mbnsf"})
    ds = HDF5Dataset(str(tmp_path), flow_sidecar="mbnsf")
    f = ds._file("scene_a")
    for ts in f.sweeps:
        for k in ("flow", "flow_is_valid", "flow_category_indices"):
            f.root[ts].pop(k, None)
    for a, b in zip(items, (ds[i] for i in range(len(ds)))):
        assert np.array_equal(b["flow"].numpy(), flows[str(a["timestamp"])][0]) and bool(b["flow_is_valid"].all())
