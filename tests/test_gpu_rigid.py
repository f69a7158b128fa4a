"""GPU: the rigid cluster flow (csrc/rigid.hip, deflow_amd/rigid.py) against tests/helpers/rigid_ref.py.

The integer results -- vote histograms, winners, statuses, rigid_id -- are compared exactly on inputs the helper reports as well-posed
(conditions asserted on the INPUT, never tolerances on the result); the fp32 results within max(1e-4, 4 x the helper's own float32-vs-
float64 difference on that case).  The helper takes the op's own DBSCAN labels (tests/test_gpu_cluster.py guards those)."""
import numpy as np
import pytest
import torch

from helpers import rigid_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _batch(samples):
    """list of dict(pc0s, pc1, n0, n1) -> padded CUDA tensors"""
    n0 = max(max(len(s["pc0s"]) for s in samples), 1)
    n1 = max(max(len(s["pc1"]) for s in samples), 1)
    pc0s = torch.from_numpy(rr.pad_batch(samples, "pc0s", n0)).to(DEV)
    pc1 = torch.from_numpy(rr.pad_batch(samples, "pc1", n1)).to(DEV)
    c0 = torch.tensor([s["n0"] for s in samples], dtype=torch.int32, device=DEV)
    c1 = torch.tensor([s["n1"] for s in samples], dtype=torch.int32, device=DEV)
    return pc0s, c0, pc1, c1


def _run(samples, **params):
    """the op on a batch, with the labels it clusters by handed to the helper too -> (gpu dict of numpy arrays, [helper f64 per sample])"""
    from deflow_amd import rigid
    pc0s, c0, pc1, c1 = _batch(samples)
    p = rigid.check_params(params)
    labels = rigid.joint_labels(pc0s, c0, pc1, c1, eps=p["eps"], min_points=p["min_points"], min_cluster_size=p["min_cluster_size"])
    flow, rid, table, vote, status, hist = rigid.rigid_cluster_flow(pc0s, c0, pc1, c1, labels=labels, return_hist=True, **params)
    torch.cuda.synchronize()
    g = {"flow": flow.cpu().numpy(), "rigid_id": rid.cpu().numpy(), "table": table.cpu().numpy(), "vote": vote.cpu().numpy(),
         "hist": hist.cpu().numpy(), "status": int(status.item()), "labels": labels.cpu().numpy(), "pc0s": pc0s.cpu().numpy(),
         "pc1": pc1.cpu().numpy()}
    return g


def _ref(g, b, dtype=np.float64, **params):
    return rr.rigid_ref(g["pc0s"][b], g["pc1"][b], g["labels"][b], dtype=dtype, **params)


EMPTY = {"pc0s": np.zeros((0, 3), np.float32), "pc1": np.zeros((0, 3), np.float32), "n0": 0, "n1": 0}


# ---- 1. votes are exact ---------------------------------------------------------------------------------------------------------------
def test_vote_histograms_are_exact_on_a_lattice():
    """coordinates on a 1/64 m lattice and vote_bin = 0.25: every difference and quotient is exact in fp32, so the WHOLE histogram of every
    slot equals the helper's -- with a side over vote_cap = 64 (the stride rule), displacements beyond max_disp, a planted exact tie
    (the lowest bin wins), a one-sided cluster, an empty sample and NaN / inf rows inside the counted part"""
    samples = [rr.lattice_sample(11, True), rr.lattice_sample(12, False), EMPTY]
    g = _run(samples, **rr.LATTICE_PARAMS)
    assert g["status"] == 0
    seen = set()
    for b in range(3):
        r = _ref(g, b, **rr.LATTICE_PARAMS)
        assert np.array_equal(g["hist"][b], r["hist"]), b
        assert np.array_equal(g["vote"][b], r["vote"]), b
        assert np.array_equal(g["table"][b][:, 5:8], r["table"][:, 5:8].astype(np.float32)), b
        seen |= set(int(v) for v in r["table"][:, 7])
        if b == 0:
            st = r["table"][:, 7]
            assert (r["table"][:, 5] > 64).any() and (st == 2).any() and (st == 5).any()            # stride rule, one-sided, beyond max_disp
            tie = [k for k in range(len(st)) if r["vote"][k, 2] > 0 and r["runner_up"][k] == r["vote"][k, 2]]
            assert tie, "the planted exact tie"
            assert any(tuple(r["vote"][k, :2]) == (-2, 0) for k in tie)                             # of (-2, 0) and (+2, 0) the lowest bin
            used = np.minimum(r["table"][:, 5], 64) * np.minimum(r["table"][:, 6], 64)
            assert (r["hist"].sum((1, 2)) < used)[st == 5].all()                                      # pairs beyond max_disp: not counted
        if b == 2:
            assert not g["hist"][b].any() and not g["vote"][b].any() and not g["table"][b].any() and not g["rigid_id"][b].any()
    assert {0, 1, 2, 5} <= seen


# ---- 2. / 3. planted rigid motions at the default parameters --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    samples = [rr.planted_sample(1), rr.planted_sample(2)]
    g = _run(samples)
    return samples, g, [_ref(g, b) for b in range(2)], [_ref(g, b, dtype=np.float32) for b in range(2)]


def test_vote_winners_at_the_default_bin(planted):
    """random continuous inputs, vote_bin = 0.2: a pair can change its bin in fp32 only when its quotient is within 1e-4 of a half-integer
    (edge_pairs), so where the winner leads by more than that, the winner is the same"""
    samples, g, r64, _ = planted
    for b in range(2):
        r = r64[b]
        voted = r["vote"][:, 2] > 0
        assert voted.sum() >= 9
        lead = r["vote"][:, 2] - r["runner_up"]
        assert (lead[voted] > r["edge_pairs"][voted]).all(), (lead[voted], r["edge_pairs"][voted])    # a condition on the input
        assert np.array_equal(g["vote"][b][:, :2], r["vote"][:, :2])
        assert (np.abs(g["vote"][b][:, 2] - r["vote"][:, 2]) <= r["edge_pairs"]).all()


def test_planted_rigid_motions(planted):
    """B = 2, 12 clusters per sample: vehicles with yaw within +-0.1 and up to 2.5 m of translation, static clutter, one-sided clusters.
    Statuses, rigid_id and vote bins exactly; theta, t and every flow component within max(1e-4, 4 x the helper's float32-vs-float64
    difference); the end-point error against the PLANTED motion no worse than the float64 helper's own (0.042 m and 0.060 m on these two
    samples: independent re-sampling of the surfaces lets a face slide along itself) plus that tolerance"""
    samples, g, r64, r32 = planted
    assert g["status"] == 0
    for b in range(2):
        r, q, s = r64[b], r32[b], samples[b]
        st = r["table"][:, 7]
        assert (st == 1).sum() >= 9 and (st == 2).sum() == 2
        assert r["band_pairs"].sum() == 0 and q["band_pairs"].sum() == 0                              # well-posed: conditions on the input
        for k, (m_frac, m_yaw, m_disp) in r["margins"].items():
            assert m_frac >= 0.05 and m_yaw >= 0.02 and m_disp >= 0.05, (k, m_frac, m_yaw, m_disp)
        assert np.array_equal(g["table"][b][:, 5:8], r["table"][:, 5:8].astype(np.float32))
        assert np.array_equal(g["rigid_id"][b], r["rigid_id"])
        assert np.array_equal(g["vote"][b][:, :2], r["vote"][:, :2])
        own = max(np.abs(q["table"][:, :5] - r["table"][:, :5]).max(), np.abs(q["flow"] - r["flow"]).max())
        tol = max(1e-4, 4 * own)
        err_t = np.abs(g["table"][b][:, :5] - r["table"][:, :5]).max()
        err_f = np.abs(g["flow"][b] - r["flow"]).max()
        print(f"sample {b}: helper fp32-vs-fp64 {own:.3e}, tolerance {tol:.3e}, kernel table {err_t:.3e}, flow {err_f:.3e}")
        assert err_t <= tol and err_f <= tol
        rows = np.nonzero(r["rigid_id"] > 0)[0]
        truth = s["truth"]
        assert np.abs(truth[rows]).max() > 1.0                                                        # the planted motions are not small
        e64, eg = rr.planted_epe(r["flow"], truth, rows), rr.planted_epe(g["flow"][b], truth, rows)
        print(f"sample {b}: end-point error against the planted motion: helper {e64:.4f} m, kernel {eg:.4f} m over {len(rows)} rows")
        assert eg <= e64 + tol
        # static clutter is registered with (nearly) no motion, and rows of no registered cluster are exactly zero
        assert not g["flow"][b][r["rigid_id"] == 0].any()


# ---- 4. caps and rejects --------------------------------------------------------------------------------------------------------------
def test_max_cluster_points_gives_status_3(planted):
    samples, _, _, _ = planted
    g = _run(samples[:1], max_cluster_points=300)
    r = _ref(g, 0, max_cluster_points=300)
    st = r["table"][:, 7]
    assert (st == 3).sum() >= 2 and (st == 1).sum() >= 2
    assert np.array_equal(g["table"][0][:, 5:8], r["table"][:, 5:8].astype(np.float32))
    assert np.array_equal(g["rigid_id"][0], r["rigid_id"])
    assert not g["flow"][0][r["rigid_id"] == 0].any() and not g["table"][0][st == 3][:, :5].any()


def test_icp_cap_subsamples_by_the_stride_rule():
    rng = np.random.default_rng(5)
    s = dict(zip(("pc0s", "pc1"), rr.vehicle(rng, (3.0, -7.0, 0.0), 0.4, 300, 300, yaw=0.06, forward=1.7)[:2]), n0=300, n1=300)
    g = _run([s], icp_cap=64)
    r, q = _ref(g, 0, icp_cap=64), _ref(g, 0, dtype=np.float32, icp_cap=64)
    full = _ref(g, 0)
    assert r["table"][0, 7] == 1 and r["table"][0, 5] == 300 and r["band_pairs"].sum() == 0
    assert np.abs(full["table"][0, :4] - r["table"][0, :4]).max() > 1e-3               # the cap matters on this input
    tol = max(1e-4, 4 * np.abs(q["table"][:, :5] - r["table"][:, :5]).max())
    assert g["table"][0][0, 7] == 1
    assert np.abs(g["table"][0][:, :5] - r["table"][:, :5]).max() <= tol
    assert np.abs(g["flow"][0] - r["flow"]).max() <= max(1e-4, 4 * np.abs(q["flow"] - r["flow"]).max())


def test_unrelated_shapes_are_rejected_with_status_4():
    """a 6 m bar in the first sweep, a 1.2 m blob at one of its ends in the second: one DBSCAN cluster, but most of the bar has no
    neighbour within icp_max_dist"""
    rng = np.random.default_rng(9)
    bar = (np.array([10.0, 4.0, 0.0]) + rng.random((200, 3)) * [6.0, 0.3, 0.8]).astype(np.float32)
    blob = (np.array([10.0, 3.6, 0.0]) + rng.random((120, 3)) * [1.2, 1.2, 0.8]).astype(np.float32)
    g = _run([{"pc0s": bar, "pc1": blob, "n0": 200, "n1": 120}])
    r = _ref(g, 0)
    assert r["table"][0, 7] == 4 and r["margins"][0][0] <= -0.05 and r["band_pairs"].sum() == 0
    assert g["table"][0][0, 7] == 4 and not g["flow"].any() and not g["rigid_id"].any()
    assert abs(g["table"][0][0, 4] - r["table"][0, 4]) < 1e-6


# ---- 5. the shape of the contract -----------------------------------------------------------------------------------------------------
def _dirty(value):
    """leave `value` in freed blocks of the caching allocator, so that an output element the kernels skip shows it"""
    junk = [torch.full((n,), value, dtype=torch.float32, device=DEV) for n in (1 << 20, 1 << 18, 1 << 16, 4096, 512)]
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize("case", ["b1_n0_ne_n1", "count0_zero", "odd_total"])
def test_contract(case, planted):
    from deflow_amd import rigid
    samples = planted[0]
    if case == "b1_n0_ne_n1":
        batch = [samples[0]]
    elif case == "count0_zero":
        z = dict(samples[1])
        z["n0"] = 0                                       # the rows are there, the count says none is valid
        batch = [samples[0], z]
    else:
        s = rr.planted_sample(3, n_vehicles=2, n_static=1, n_one=1, pad0=2, pad1=0)
        batch = [s]
    pc0s, c0, pc1, c1 = _batch(batch)
    if case == "odd_total" and (pc0s.shape[1] + pc1.shape[1]) % 2 == 0:
        pc0s = torch.cat([pc0s, torch.full((1, 1, 3), float("nan"), device=DEV)], dim=1)
    N0, N1 = pc0s.shape[1], pc1.shape[1]
    assert N0 != N1 and (case != "odd_total" or (N0 + N1) % 2 == 1)                                   # no multiple of any tile size
    outs = []
    for fill in (float("nan"), 1.0e30):
        _dirty(fill)
        o = rigid.rigid_cluster_flow(pc0s, c0, pc1, c1, return_hist=True)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in o])
    for a, b in zip(*outs):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))           # bit-identical, NaN patterns included
    flow, rid, table, vote, status, hist = outs[0]
    K = rigid.kcap(N0, N1, 20)
    assert flow.shape == (len(batch), N0, 3) and rid.shape == (len(batch), N0) and table.shape == (len(batch), K, 8)
    assert vote.shape == (len(batch), K, 3) and hist.shape == (len(batch), K, 35, 35)
    assert int(status) == 0
    assert torch.isfinite(flow).all() and torch.isfinite(table).all()
    assert (rid >= 0).all() and (rid <= K).all() and (rid > 0).any()
    assert not flow[rid == 0].any()                                                                   # rows of no registered cluster
    for b, s in enumerate(batch):
        assert not flow[b, s["n0"]:].any() and not rid[b, s["n0"]:].any()                             # padded rows
        st = table[b, :, 7]
        assert set(st.tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
        assert (table[b, :, 5] + table[b, :, 6])[st == 0].sum() == 0
    if case == "count0_zero":
        assert not rid[1].any() and not flow[1].any() and not (table[1, :, 7] == 1).any() and (table[1, :, 7] == 2).any()
    # the labels argument is what the op computes itself
    labels = rigid.joint_labels(pc0s, c0, pc1, c1, eps=0.7, min_points=4, min_cluster_size=20)
    again = rigid.rigid_cluster_flow(pc0s, c0, pc1, c1, labels=labels)
    assert torch.equal(again[0].cpu(), flow) and torch.equal(again[1].cpu(), rid)


# ---- 6. through the stack -----------------------------------------------------------------------------------------------------------------
def _raw_pair(seed):
    """a planted scene as RAW sweeps: besides the objects ground rows (to be dropped), rows outside the model's range and a NaN row, shuffled"""
    s = rr.planted_sample(seed, n_vehicles=3, n_static=1, n_one=1, pad0=0, pad1=0)
    rng = np.random.default_rng(100 + seed)
    out = {}
    for g, key in (("0", "pc0s"), ("1", "pc1")):
        obj = s[key]
        ground = np.stack([rng.uniform(-45, 45, 150), rng.uniform(-45, 45, 150), rng.normal(-1.6, 0.02, 150)], axis=1).astype(np.float32)
        far = np.stack([rng.uniform(52, 60, 30), rng.uniform(-10, 10, 30), rng.uniform(0, 1, 30)], axis=1).astype(np.float32)
        high = np.stack([rng.uniform(-5, 5, 10), rng.uniform(-5, 5, 10), rng.uniform(3.5, 5, 10)], axis=1).astype(np.float32)
        nan = np.full((1, 3), np.nan, dtype=np.float32)
        raw = np.concatenate([obj, ground, far, high, nan])
        drop = np.concatenate([np.zeros(len(obj)), np.ones(150), np.zeros(41)]).astype(np.uint8)
        p = rng.permutation(len(raw))
        out["raw" + g], out["drop" + g] = raw[p], drop[p]
    return out


def test_icpflow_inside_sweepflow_and_metrics():
    from helpers import sweep_flow_ref as SR
    from deflow_amd import metrics, rigid, sweeps
    from deflow_amd.deflow import batch_transform
    pairs = [_raw_pair(4), _raw_pair(5)]
    host = {}
    for g in ("0", "1"):
        n = max(len(p["raw" + g]) for p in pairs) + 3
        raw = np.full((2, n, 3), np.nan, dtype=np.float32)
        drop = np.zeros((2, n), dtype=np.uint8)
        for b, p in enumerate(pairs):
            raw[b, : len(p["raw" + g])], drop[b, : len(p["raw" + g])] = p["raw" + g], p["drop" + g]
        host["raw" + g], host["drop" + g] = raw, drop
        host["n" + g] = np.array([len(p["raw" + g]) for p in pairs], dtype=np.int32)
    pose0 = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    pose1 = pose0.copy()
    for b in range(2):
        a = 0.004 * (b + 1)
        pose1[b, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        pose1[b, :3, 3] = (0.3 + 0.1 * b, -0.02, 0.004)
    d = lambda a: torch.from_numpy(a).to(DEV)
    model = rigid.IcpFlow()
    sf = sweeps.SweepFlow(model)
    args = (d(host["raw0"]), d(host["n0"]), d(host["drop0"]), d(host["raw1"]), d(host["n1"]), d(host["drop1"]), d(pose0), d(pose1))
    est, dyn = sf.infer(*args)
    st = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in model.last_state.items()}
    est2, dyn2 = sf.infer(*args)
    assert torch.equal(est.view(torch.int32), est2.view(torch.int32)) and torch.equal(dyn, dyn2)
    est, dyn = est.cpu().numpy(), dyn.cpu().numpy()
    assert int(st["status"][0]) == 0
    T = batch_transform({"pose0": d(pose0), "pose1": d(pose1)}, DEV).cpu().numpy()
    _, _, pos_of, kept = SR.compact_batch(host["raw0"], host["n0"], host["drop0"])
    # the composition over the model's own padded outputs: ground, out-of-range and NaN rows get the pose flow (or zeros), decoded rows
    # pose flow + rigid flow, bit for bit
    want, want_dyn = SR.compose_batch(host["raw0"], host["n0"], T, pos_of, st["flow"], st["idx_c0"], st["counts0"])
    assert np.array_equal(est.view(np.int32), want.view(np.int32)) and np.array_equal(dyn, want_dyn)
    labels = rigid.joint_labels(d(st["points_c0"]), d(st["counts0"]), d(st["points_c1"]), d(st["counts1"]), eps=0.7, min_points=4,
                                min_cluster_size=20).cpu().numpy()
    for b in range(2):
        n0, c0 = int(host["n0"][b]), int(st["counts0"][b])
        raw = host["raw0"][b]
        # which rows are decoded: the voxeliser's rule on the ego-compensated compact rows, ascending
        pc = st["pc0s"][b]
        with np.errstate(invalid="ignore"):
            ok = ~np.isnan(pc).any(1)
            for i, (lo, v, gsz) in enumerate(((-51.2, 0.2, 512), (-51.2, 0.2, 512), (-3.0, 6.0, 1))):
                f = np.floor((pc[:, i] - np.float32(lo)) / np.float32(v))
                ok &= (f >= 0) & (f < gsz)
        assert np.array_equal(st["idx_c0"][b][:c0], np.nonzero(ok)[0]) and c0 == int(kept[b]) - 41        # 30 far, 10 high, one NaN row
        ground = np.nonzero((host["drop0"][b] != 0) & (np.arange(raw.shape[0]) < n0))[0]
        outside = np.nonzero((np.abs(raw[:, 0]) > 51.9) | (raw[:, 2] > 3.4))[0]
        for rows in (ground, outside):
            assert len(rows) >= 40 and np.array_equal(est[b][rows].view(np.int32), SR.pose_flow(raw[rows], T[b]).view(np.int32))
            assert not dyn[b][rows].any()
        assert not est[b][n0:].any() and not est[b][np.isnan(raw).any(1)].any()
        # the rigid flow of the decoded rows is the helper's on the same compact clouds
        r = rr.rigid_ref(st["points_c0"][b], st["points_c1"][b], labels[b])
        q = rr.rigid_ref(st["points_c0"][b], st["points_c1"][b], labels[b], dtype=np.float32)
        assert (r["table"][:, 7] == 1).sum() >= 3 and r["band_pairs"].sum() == 0
        assert np.array_equal(st["rigid_id"][b], r["rigid_id"]) and np.array_equal(st["table"][b][:, 7], r["table"][:, 7].astype(np.float32))
        tol = max(1e-4, 4 * np.abs(q["flow"] - r["flow"]).max())
        assert np.abs(st["flow"][b] - r["flow"]).max() <= tol
        moved = np.nonzero(np.linalg.norm(st["flow"][b], axis=1) > 0.3)[0]
        assert len(moved) > 100 and dyn[b].sum() >= len(moved)
    # the object goes where the model goes: forward()'s dict of lists into evaluate_batch
    keep0 = [(np.arange(host["raw0"].shape[1]) < host["n0"][b]) & (host["drop0"][b] == 0) for b in range(2)]
    batch = {"pc0": d(st["pc0s"] * 0 + np.stack([np.concatenate([host["raw0"][b][keep0[b]],
                                                                np.full((st["pc0s"].shape[1] - keep0[b].sum(), 3), np.nan, np.float32)])
                                                 for b in range(2)])),
             "pc1": d(st["points_c1"]), "pose0": d(pose0), "pose1": d(pose1)}
    batch["flow"] = torch.zeros_like(batch["pc0"])
    batch["flow_is_valid"] = torch.ones(batch["pc0"].shape[:2], dtype=torch.bool, device=DEV)
    batch["flow_category_indices"] = torch.ones(batch["pc0"].shape[:2], dtype=torch.uint8, device=DEV)
    res = model(batch)
    assert sorted(res) == ["flow", "pc0_points_lst", "pc0_valid_point_idxes", "pc1_points_lst", "pc1_valid_point_idxes", "pose_flow"]
    assert [int(f.shape[0]) for f in res["flow"]] == st["counts0"].tolist()
    m = metrics.evaluate_batch(res, batch)
    assert {"EPE", "AccS", "AccR"} <= set(m) and all(np.isfinite(v) for v in m.values())
    from deflow_amd.metrics_device import DeviceMetrics, evaluate_batch_device
    dm = DeviceMetrics(torch.device(DEV))
    evaluate_batch_device(model, batch, dm)
    assert abs(dm.summary()["EPE"] - m["EPE"]) < 1e-4


def test_save_and_vis_commands(tmp_path, golden_dir, capsys):
    import json
    import os
    import shutil
    from deflow_amd import rigid, save, vis
    from deflow_amd.h5scene import H5File
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "scene_val.h5"), tmp_path / "scene_val.h5")      # never written under tests/golden
    shutil.copy(os.path.join(golden_dir, "av2_mini", "train", "scene_chunked.h5"), tmp_path / "scene_chunked.h5")
    argv = ["model=icpflow", f"dataset_path={tmp_path}", "icp_min_side=6", "icp_vote_bin=0.25", "batch_size=4",
            "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"]
    assert save.main(argv) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert [x["scene"] for x in lines] == ["scene_chunked", "scene_val"] and all(x["sweeps"] >= 2 for x in lines)
    for sid in ("scene_chunked", "scene_val"):
        path = save.flow_path(str(tmp_path), sid, "icpflow")
        assert os.path.basename(path) == f"{sid}.icpflow.flow.npz"
        got, meta = save.read_flow(path), save.read_meta(path)
        want_params = dict(rigid.DEFAULTS, min_side=6, vote_bin=0.25)
        assert meta == {"res_name": "icpflow", "checkpoint": None, "model": "icpflow", "voxel_size": [0.2, 0.2, 6.0],
                        "point_cloud_range": [-6.4, -6.4, -3.0, 6.4, 6.4, 3.0], "ground_source": "auto", "half": False,
                        "params": want_params, "definition": "DESIGN.md 6f, 6j (UNPINNED)"}
        with H5File(str(tmp_path / (sid + ".h5"))) as f:
            ts = sorted(f.keys(), key=int)
            rows = {t: int(f[t]["lidar"].read().shape[0]) for t in ts}
        assert list(got) == ts[:-1]
        for t in ts[:-1]:
            assert got[t][0].dtype == np.float32 and got[t][0].shape == (rows[t], 3) and got[t][1].shape == (rows[t],)
            assert np.isfinite(got[t][0]).all()
    # a second run skips; the vis command draws the file with no further change
    assert save.main(argv) == 0
    assert all("skipped" in json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{"))
    out_dir = tmp_path / "png"
    assert vis.main([f"dataset_path={tmp_path}", "res_name=icpflow", "scenes=scene_val", f"out_dir={out_dir}", "range=6.4", "res=0.2",
                     "panels=est"]) == 0
    line = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")][0]
    assert line["scene"] == "scene_val" and line["images"] >= 2 and line["panels"] == ["est"]
    assert len(os.listdir(out_dir / "scene_val")) == line["images"]
    # eval with model=icpflow prints the usual result line on the same files
    from deflow_amd import eval as ev
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "index_total.pkl"), tmp_path / "index_total.pkl")
    os.remove(tmp_path / "scene_chunked.h5")
    out = ev.main(["model=icpflow", f"val_data={tmp_path}", "batch_size=4", "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"])
    result = json.loads([x for x in capsys.readouterr().out.splitlines() if x.startswith("{")][-1])
    assert result["model"] == "icpflow" and result["checkpoint"] is None and "EPE" in result["metrics"] and "leaderboard" in out
