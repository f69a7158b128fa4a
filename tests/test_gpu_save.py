"""GPU: the whole-sweep flow (csrc/sweep.hip, deflow_amd/sweeps.py, ``python -m deflow_amd.save``) against the numpy restatement in
tests/helpers/sweep_flow_ref.py.  Compaction moves bits and composition is a fixed sequence of separately rounded fp32 operations, so every
comparison is exact: torch.equal, for floats on the int32 / int16 view so that NaN padding and signed zeros count."""
import json
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import sweep_flow_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], grid_feature_size=[64, 64])   # tests/test_gpu_ground.py's
F = np.float32
B = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.fixture(scope="module")
def R():
    from deflow_amd import sweeps
    r = sweeps.rows_per_block()
    assert r >= 64 and r % 64 == 0
    return r


def ibits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same(got: torch.Tensor, want: np.ndarray, what: str):
    w = torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == w.dtype and tuple(got.shape) == tuple(w.shape), (what, got.dtype, tuple(got.shape), w.dtype, tuple(w.shape))
    g, w = ibits(got), ibits(w)
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ"


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def make_case(N, mode, seed):
    """B = 3 raw sweeps of N rows: counts straddle {0, 1, N}; drop: all / none / a random 30 %, with values 1, 2 and 255 all counting as
    set; a few NaN and inf rows among the valid ones; rows behind count hold finite garbage or NaN"""
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal((B, N, 3)) * (20.0, 20.0, 1.5)).astype(F)
    for b in range(B):
        bad = rng.choice(N, size=max(1, N // 50), replace=False)
        raw[b, bad[::2], rng.integers(0, 3)] = np.nan
        raw[b, bad[1::2], rng.integers(0, 3)] = np.inf * (-1) ** b
    count = {"none": [N, 1, 0], "all": [N, 0, 1], "random": [N, N - 7, N // 2]}[mode]
    raw[1, count[1]:] = np.nan                                           # as the collate pads; sample 2 keeps finite garbage behind count
    if mode == "none":
        drop = np.zeros((B, N), dtype=np.uint8)
    elif mode == "all":
        drop = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=(B, N))
    else:
        drop = np.where(rng.random((B, N)) < 0.3, rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=(B, N)), 0).astype(np.uint8)
    return raw, np.array(count, dtype=np.int32), drop


def make_flow(raw, kept, seed):
    """synthetic decoder output for a compacted case: idx_c a random unsorted subset of each sample's kept compact rows, counts 0 / kept /
    in between, flow rows with exact zeros, the three rows around the 0.0025f threshold and magnitudes past the fp16 range; entries
    behind counts hold values a kernel must not use"""
    rng = np.random.default_rng(seed)
    Bn, N, _ = raw.shape
    T = np.tile(np.eye(4, dtype=F), (Bn, 1, 1))
    for b in range(Bn):
        a = 0.02 * (b + 1)
        T[b, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[b, :3, 3] = rng.standard_normal(3) * (1.0, 0.3, 0.05)
    flow = (rng.standard_normal((Bn, N, 3)) * 0.04).astype(F)
    idx_c = np.full((Bn, N), -1, dtype=np.int64)
    counts = np.zeros(Bn, dtype=np.int32)
    thr = SR.threshold_flows()
    special = [np.zeros(3, dtype=F), np.array([-0.0, 0.0, -0.0], dtype=F), thr["below"], thr["at"], thr["above"], -thr["at"],
               np.array([7e4, -1e5, 65520.0], dtype=F), np.array([65519.0, -65504.0, 3e38], dtype=F)]
    order = np.argsort(kept)                                             # the sample with most kept rows decodes them all, the one with fewest none
    for rank, b in enumerate(order[::-1]):
        k = int(kept[b])
        m = [k, k // 2, 0][min(rank, 2)]
        counts[b] = m
        idx_c[b, :m] = rng.permutation(k)[:m]
        idx_c[b, m:] = rng.choice(np.array([-1, 0, N, 1 << 40], dtype=np.int64), size=N - m)
        for i, row in enumerate(special[:m]):
            flow[b, i] = row
    return T, flow, idx_c, counts


def gpu_compact_poisoned(dev, raw, count, drop):
    """df_sweep_compact through the binding on buffers of this test's own, every byte 0x5A beforehand"""
    from deflow_amd._lib import call, ptr, stream
    Bn, N, _ = raw.shape
    d = lambda a: torch.from_numpy(a).to(dev)
    raw_d, count_d, drop_d = d(raw), d(count), d(drop)
    need = int(call("df_sweep_compact_ws_bytes", Bn, N))
    assert need > 0
    ws = torch.full(((need + 3) // 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    pc = torch.full((Bn, N, 3), 0x5A5A5A5A, dtype=torch.int32, device=dev).view(torch.float32)
    row_of = torch.full((Bn, N), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    pos_of = torch.full((Bn, N), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    kept = torch.full((Bn,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    call("df_sweep_compact", ptr(raw_d), ptr(count_d), ptr(drop_d), Bn, N, ptr(ws), ptr(pc), ptr(row_of), ptr(pos_of), ptr(kept), stream())
    return pc, row_of, pos_of, kept


def gpu_compose_poisoned(dev, raw, count, T, pos_of, flow, idx_c, counts, half):
    """df_flow_compose through the binding, every output byte 0xFF beforehand: a row written zero times or left stale shows"""
    from deflow_amd._lib import call, ptr, stream
    Bn, N, _ = raw.shape
    d = lambda a: torch.from_numpy(a).to(dev)
    args = [d(a) for a in (raw, count, T, pos_of, flow, idx_c, counts)]
    need = int(call("df_flow_compose_ws_bytes", Bn, N))
    assert need == Bn * N * 4
    ws = torch.full((need // 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    est = torch.full((Bn, N, 3), -1, dtype=torch.int16 if half else torch.int32, device=dev).view(torch.float16 if half else torch.float32)
    dyn = torch.full((Bn, N), 0xFF, dtype=torch.uint8, device=dev)
    call("df_flow_compose", *(ptr(a) for a in args), Bn, N, int(flow.shape[1]), int(half), ptr(ws), ptr(est), ptr(dyn), stream())
    return est, dyn


# ---- compaction ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", "all", "random"])
@pytest.mark.parametrize("which", ["R-1", "R", "R+1", "2R+3"])
def test_compaction_and_composition(dev, R, which, mode):
    from deflow_amd import sweeps
    N = {"R-1": R - 1, "R": R, "R+1": R + 1, "2R+3": 2 * R + 3}[which]
    raw, count, drop = make_case(N, mode, seed=N * 3 + len(mode))
    want = SR.compact_batch(raw, count, drop)
    print(f"[save] N = {N}, {mode}: counts {count.tolist()}, kept {want[3].tolist()}")
    names = ("pc", "row_of", "pos_of", "kept")
    for name, g, w in zip(names, gpu_compact_poisoned(dev, raw, count, drop), want):
        same(g, w, f"df_sweep_compact {name}")
    d = lambda a: torch.from_numpy(a).to(dev)
    raw_d, count_d = d(raw), d(count)
    got = sweeps.compact_rows(raw_d, count_d, d(drop))
    for name, g, w in zip(names, got, want):
        same(g, w, f"compact_rows {name}")
    got_b = sweeps.compact_rows(raw_d, count_d, d(drop) != 0)           # a bool mask is the same mask
    for name, g, w in zip(names, got_b, want):
        same(g, w, f"compact_rows(bool) {name}")
    # ---- composition at the same shape
    T, flow, idx_c, counts = make_flow(raw, want[3], seed=N + 11)
    assert counts.min() == 0 and (counts.max() == want[3].max())
    for half in (False, True):
        w_est, w_dyn = SR.compose_batch(raw, count, T, want[2], flow, idx_c, counts, half=half)
        assert not np.isnan(w_est.astype(F)).any()
        est, dyn = gpu_compose_poisoned(dev, raw, count, T, want[2], flow, idx_c, counts, half)
        same(est, w_est, f"df_flow_compose flow_est half={half}")
        same(dyn, w_dyn, f"df_flow_compose dynamic half={half}")
        a = sweeps.compose_flow(raw_d, count_d, d(T), got[2], d(flow), d(idx_c), d(counts), half=half)
        b = sweeps.compose_flow(raw_d, count_d, d(T), got[2], d(flow), d(idx_c), d(counts), half=half)
        same(a[0], w_est, f"compose_flow flow_est half={half}")
        same(a[1], w_dyn, f"compose_flow dynamic half={half}")
        assert torch.equal(ibits(a[0]), ibits(b[0])) and torch.equal(a[1], b[1]), "a second call differs"
    if mode != "all":
        assert w_dyn.any() and not w_dyn.all()
        assert np.isinf(w_est.astype(F)).any()                           # the rows past the fp16 range


def test_compaction_of_the_val_fixture_equals_collate_fn_pad(dev, golden_dir):
    from deflow_amd import sweeps
    from deflow_amd.data import HDF5Dataset, collate_fn_pad
    ds = HDF5Dataset(os.path.join(golden_dir, "av2_mini", "val"))
    items = [ds[i] for i in range(len(ds))]
    host, rawb = collate_fn_pad(items), sweeps.collate_raw_pad(items)
    for g in ("0", "1"):
        pc, row_of, pos_of, kept = sweeps.compact_rows(rawb["raw" + g].to(dev), rawb["n" + g].to(dev), rawb["drop" + g].to(dev))
        w = host["pc" + g]
        n = w.shape[1]
        assert int(kept.max()) == n and kept.tolist() == [int((~it["gm" + g]).sum()) for it in items]
        assert torch.equal(ibits(pc[:, :n]), ibits(w)), "the kept rows differ from collate_fn_pad's"
        assert bool((ibits(pc[:, n:]) == 0x7FC00000).all())
        wp = SR.compact_batch(rawb["raw" + g].numpy(), rawb["n" + g].numpy(), rawb["drop" + g].numpy())
        same(row_of, wp[1], "row_of")
        same(pos_of, wp[2], "pos_of")


# ---- no host reads: both ops captured in a graph ------------------------------------------------------------------------------------------
def test_graph_replay_on_overwritten_inputs(dev, R):
    from deflow_amd import sweeps
    N = R + 37
    d = lambda a: torch.from_numpy(a).to(dev)
    cases = []
    for seed in (1, 2):
        raw, count, drop = make_case(N, "random", seed=seed)
        want = SR.compact_batch(raw, count, drop)
        T, flow, idx_c, counts = make_flow(raw, want[3], seed=seed + 5)
        cases.append((raw, count, drop, T, flow, idx_c, counts, want))
    static = [d(a) for a in cases[0][:7]]
    sweeps.compose_flow(static[0], static[1], static[3], sweeps.compact_rows(*static[:3])[2], *static[4:])     # eager first: sizes everything
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                            # one stream, a linear chain
        pc, row_of, pos_of, kept = sweeps.compact_rows(*static[:3])
        est, dyn = sweeps.compose_flow(static[0], static[1], static[3], pos_of, *static[4:])
    for case in (cases[1], cases[0]):
        for s, a in zip(static, case[:7]):
            s.copy_(d(a))
        for t in (pc, row_of, pos_of, kept, est, dyn):
            t.view(torch.uint8).fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        raw, count, drop, T, flow, idx_c, counts, want = case
        for name, got, w in zip(("pc", "row_of", "pos_of", "kept"), (pc, row_of, pos_of, kept), want):
            same(got, w, f"replay {name}")
        w_est, w_dyn = SR.compose_batch(raw, count, T, want[2], flow, idx_c, counts)
        same(est, w_est, "replay flow_est")
        same(dyn, w_dyn, "replay dynamic")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def small_model(dev, seed=31):
    import deflow_amd
    torch.manual_seed(seed)
    return deflow_amd.DeFlow(**SMALL, num_iters=2).to(dev).eval()


def street(N, seed):
    """a B = 2 cloud around the SMALL range: rows outside +-6.4 m, a ground plane near z = -0.33, NaN rows"""
    rng = np.random.default_rng(seed)
    raw = np.empty((2, N, 3), dtype=F)
    raw[..., :2] = rng.uniform(-8.0, 8.0, (2, N, 2))
    raw[..., 2] = rng.uniform(-0.2, 2.0, (2, N))
    plane = rng.random((2, N)) < 0.3
    raw[..., 2][plane] = (-0.33 + 0.02 * rng.standard_normal(int(plane.sum()))).astype(F)
    raw[0, rng.choice(N, 5, replace=False), 0] = np.nan
    raw[1, rng.choice(N, 5, replace=False), 2] = np.nan
    count = np.array([N, N - N // 4], dtype=np.int32)
    raw[1, count[1]:] = np.nan
    return raw, count, plane.astype(np.uint8)


def test_end_to_end_against_the_host_path(dev):
    from deflow_amd import sweeps
    from deflow_amd.data import _pad
    from deflow_amd.deflow import batch_transform
    from deflow_amd.ground import GroundSegmenter
    model = small_model(dev)
    raw0, n0, drop0 = street(700, 3)
    raw1, n1, drop1 = street(640, 4)
    rng = np.random.default_rng(9)
    pose0 = np.tile(np.eye(4, dtype=F), (2, 1, 1))
    pose1 = pose0.copy()
    for b in range(2):
        a = 0.01 * (b + 1)
        pose1[b, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        pose1[b, :3, 3] = (0.4 + 0.1 * b, 0.02, 0.003)
        pose0[b, :3, 3] = rng.standard_normal(3) * 0.01
    d = lambda a: torch.from_numpy(a).to(dev)
    args = (d(raw0), d(n0), d(drop0), d(raw1), d(n1), d(drop1), d(pose0), d(pose1))
    sf = sweeps.SweepFlow(model)
    est, dyn = sf.infer(*args)
    est2, dyn2 = sf.infer(*args)
    assert torch.equal(ibits(est), ibits(est2)) and torch.equal(dyn, dyn2)
    # ---- the existing path: host filtering as collate_fn_pad does it, then model.forward
    keep0 = [(np.arange(raw0.shape[1]) < n0[b]) & (drop0[b] == 0) for b in range(2)]
    keep1 = [(np.arange(raw1.shape[1]) < n1[b]) & (drop1[b] == 0) for b in range(2)]
    batch = {"pc0": _pad([torch.from_numpy(raw0[b][keep0[b]]) for b in range(2)], float("nan")).to(dev),
             "pc1": _pad([torch.from_numpy(raw1[b][keep1[b]]) for b in range(2)], float("nan")).to(dev),
             "pose0": d(pose0), "pose1": d(pose1)}
    with torch.no_grad():
        res = model(batch)
    T = batch_transform(batch, dev).cpu().numpy()
    want = np.zeros(raw0.shape, dtype=F)
    want_dyn = np.zeros(raw0.shape[:2], dtype=np.uint8)
    covered = np.zeros(raw0.shape[:2], dtype=np.int32)
    for b in range(2):
        rows = np.nonzero(keep0[b])[0]
        idx = res["pc0_valid_point_idxes"][b].cpu().numpy()
        flow = res["flow"][b].cpu().numpy()
        pf = res["pose_flow"][b].cpu().numpy()
        assert 50 < idx.shape[0] < rows.shape[0]                         # rows outside the range and NaN rows were kept but not decoded
        fin = np.isfinite(raw0[b]).all(axis=1) & (np.arange(raw0.shape[1]) < n0[b])
        want[b][fin] = SR.pose_flow(raw0[b][fin], T[b])                  # every finite row: its pose flow ...
        covered[b][fin] += 1
        covered[b][~fin] += 1                                            # ... every other row: zeros
        want[b][rows[idx]] = pf[idx] + flow                              # ... and the decoded rows: the model's pose flow + flow, one fp32 add
        want_dyn[b][rows[idx]] = SR.sq_norm(flow) >= SR.DYN2
        assert np.array_equal(SR.pose_flow(raw0[b][rows[idx]], T[b]).view(np.int32), pf[idx].view(np.int32))
        assert fin[rows[idx]].all()
    assert (covered == 1).all()
    print(f"[save] end to end: {int(want_dyn.sum())} of {int(sum(len(i) for i in res['pc0_valid_point_idxes']))} decoded rows dynamic")
    same(est, want, "SweepFlow.infer flow_est")
    same(dyn, want_dyn, "SweepFlow.infer dynamic")
    h, dh = sf.infer(*args, half=True)
    with np.errstate(all="ignore"):
        same(h, want.astype(np.float16), "SweepFlow.infer flow_est (half)")
    same(dh, want_dyn, "SweepFlow.infer dynamic (half)")
    # ---- the fully raw path: masks from a segmenter
    seg = GroundSegmenter(2, device=dev)
    m0 = seg.segment(args[0], args[1]).clone()
    m1 = seg.segment(args[3], args[4]).clone()
    assert bool(m0.any()) and not bool(m0.all())
    a = sf.infer(args[0], args[1], m0, args[3], args[4], m1, args[6], args[7])
    b = sweeps.SweepFlow(model, ground=seg).infer(args[0], args[1], None, args[3], args[4], None, args[6], args[7])
    assert torch.equal(ibits(a[0]), ibits(b[0])) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError, match="no ground segmenter"):
        sf.infer(args[0], args[1], None, args[3], args[4], m1, args[6], args[7])


# ---- the command --------------------------------------------------------------------------------------------------------------------------
def test_save_command(dev, tmp_path, golden_dir, capsys):
    from deflow_amd import save, sweeps, train
    from deflow_amd.h5scene import H5File
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "scene_val.h5"), tmp_path / "scene_val.h5")      # never written under tests/golden
    shutil.copy(os.path.join(golden_dir, "av2_mini", "train", "scene_chunked.h5"), tmp_path / "scene_chunked.h5")
    model = small_model(dev, seed=47)
    cfg = dict(train.DEFAULTS)
    cfg.update({"voxel_size": SMALL["voxel_size"], "point_cloud_range": SMALL["point_cloud_range"], "model.target.num_iters": 2, "batch_size": 4})
    ckpt = str(tmp_path / "small_best.ckpt")
    train.save_checkpoint(ckpt, model, types.SimpleNamespace(opt=types.SimpleNamespace(state_dict=lambda: {})), cfg, 0, 0)
    argv = [f"checkpoint={ckpt}", f"dataset_path={tmp_path}"]
    assert save.main(argv) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert [x["scene"] for x in lines] == ["scene_chunked", "scene_val"] and all(x["sweeps"] >= 2 and "seconds" in x for x in lines)
    sf = sweeps.SweepFlow(model)
    first = {}
    for sid in ("scene_chunked", "scene_val"):
        path = save.flow_path(str(tmp_path), sid, "small_best")
        assert os.path.basename(path) == f"{sid}.small_best.flow.npz"
        got = first[sid] = save.read_flow(path)
        meta = save.read_meta(path)
        assert meta == {"res_name": "small_best", "checkpoint": "small_best.ckpt", "model": "deflow", "voxel_size": [0.2, 0.2, 6.0],
                        "point_cloud_range": [-6.4, -6.4, -3.0, 6.4, 6.4, 3.0], "ground_source": "auto", "half": False,
                        "definition": "DESIGN.md 6f (UNPINNED)"}
        with H5File(str(tmp_path / (sid + ".h5"))) as f:
            sweeps_ts = sorted(f.keys(), key=int)
            rows = {t: int(f[t]["lidar"].read().shape[0]) for t in sweeps_ts}
        assert list(got) == sweeps_ts[:-1]                               # every sweep but the scene's last
        for t in sweeps_ts[:-1]:
            assert got[t][0].dtype == np.float32 and got[t][0].shape == (rows[t], 3) and got[t][1].dtype == np.uint8 and got[t][1].shape == (rows[t],)
        if sid == "scene_chunked":
            assert 0 in [rows[t] for t in sweeps_ts[:-1]]                # the zero-row sweep has an entry, and it is empty
        # the arrays are SweepFlow.infer's on the same pairs
        pairs = save.ScenePairs(str(tmp_path), sid)
        items = [pairs[i] for i in range(len(pairs))]
        decoded = 0
        for k in range(0, len(items), 4):
            hb = sweeps.collate_raw_pad(items[k:k + 4])
            db = {key: v.to(dev) for key, v in hb.items() if isinstance(v, torch.Tensor)}
            est, dyn = sf.infer(db["raw0"], db["n0"], db["drop0"], db["raw1"], db["n1"], db["drop1"], db["pose0"], db["pose1"],
                                ego_motion=db.get("ego_motion"))
            decoded += int(sf.model.last_state["counts0"].sum())
            for i, (ts, n) in enumerate(zip(hb["timestamp"], hb["n0"].tolist())):
                same(est[i, :n], got[str(ts)][0], f"{sid} {ts} flow_est")
                same(dyn[i, :n], got[str(ts)][1], f"{sid} {ts} dynamic")
        print(f"[save] {sid}: {len(got)} sweeps, {sum(rows[t] for t in sweeps_ts[:-1])} rows, {decoded} decoded")
    # a second run skips both; overwrite=true rewrites the same arrays
    mtime = {sid: os.path.getmtime(save.flow_path(str(tmp_path), sid, "small_best")) for sid in first}
    assert save.main(argv) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 2 and all("skipped" in x for x in lines)
    assert all(os.path.getmtime(save.flow_path(str(tmp_path), sid, "small_best")) == mtime[sid] for sid in first)
    assert save.main(argv + ["overwrite=true", "scenes=scene_val"]) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1 and lines[0]["scene"] == "scene_val" and "skipped" not in lines[0]
    again = save.read_flow(save.flow_path(str(tmp_path), "scene_val", "small_best"))
    assert list(again) == list(first["scene_val"])
    for t, (f, m) in first["scene_val"].items():
        assert np.array_equal(again[t][0].view(np.int32), f.view(np.int32)) and np.array_equal(again[t][1], m)
    # half=true under another name: the same flow rounded to fp16
    assert save.main(argv + ["res_name=h", "half=true", "scenes=scene_val"]) == 0
    capsys.readouterr()
    halves = save.read_flow(save.flow_path(str(tmp_path), "scene_val", "h"))
    for t, (f, m) in first["scene_val"].items():
        with np.errstate(all="ignore"):
            assert halves[t][0].dtype == np.float16 and np.array_equal(halves[t][0].view(np.int16), f.astype(np.float16).view(np.int16))
        assert np.array_equal(halves[t][1], m)
    assert save.read_meta(save.flow_path(str(tmp_path), "scene_val", "h"))["half"] is True
    # ground_source=online: the masks come from a segmenter on the GPU, none is read from the files
    from deflow_amd.ground import GroundSegmenter
    assert save.main(argv + ["res_name=on", "ground_source=online", "scenes=scene_val"]) == 0
    capsys.readouterr()
    online = save.read_flow(save.flow_path(str(tmp_path), "scene_val", "on"))
    assert save.read_meta(save.flow_path(str(tmp_path), "scene_val", "on"))["ground_source"] == "online"
    pairs = save.ScenePairs(str(tmp_path), "scene_val", "online")
    items = [pairs[i] for i in range(len(pairs))]
    assert list(online) == [str(it["timestamp"]) for it in items] and not any(bool(it["gm0"].any()) or bool(it["gm1"].any()) for it in items)
    for k in range(0, len(items), 4):
        hb = sweeps.collate_raw_pad(items[k:k + 4])
        db = {key: v.to(dev) for key, v in hb.items() if isinstance(v, torch.Tensor)}
        seg = GroundSegmenter(len(hb["timestamp"]), device=dev)
        est, dyn = sweeps.SweepFlow(model, ground=seg).infer(db["raw0"], db["n0"], None, db["raw1"], db["n1"], None, db["pose0"], db["pose1"],
                                                             ego_motion=db.get("ego_motion"))
        for i, (ts, n) in enumerate(zip(hb["timestamp"], hb["n0"].tolist())):
            same(est[i, :n], online[str(ts)][0], f"online {ts} flow_est")
            same(dyn[i, :n], online[str(ts)][1], f"online {ts} dynamic")


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors(dev):
    from deflow_amd import sweeps
    from deflow_amd._lib import call, ptr
    N = 16
    raw = torch.zeros(2, N, 3, device=dev)
    cnt = torch.full((2,), N, dtype=torch.int32, device=dev)
    drop = torch.zeros(2, N, dtype=torch.uint8, device=dev)
    pc, row_of, pos_of, kept = sweeps.compact_rows(raw, cnt, drop)
    T = torch.eye(4, device=dev).repeat(2, 1, 1)
    flow = torch.zeros(2, N, 3, device=dev)
    idx = torch.zeros(2, N, dtype=torch.int64, device=dev)
    m = torch.zeros(2, dtype=torch.int32, device=dev)
    sweeps.compose_flow(raw, cnt, T, pos_of, flow, idx, m)
    with pytest.raises(TypeError, match="CUDA tensor"):
        sweeps.compact_rows(raw.cpu(), cnt, drop)
    with pytest.raises(TypeError, match="CUDA tensor"):
        sweeps.compact_rows(raw, cnt.cpu(), drop)
    with pytest.raises(TypeError, match="CUDA tensor"):
        sweeps.compose_flow(raw, cnt, T, pos_of, flow.cpu(), idx, m)
    with pytest.raises(ValueError, match="raw must be torch.float32"):
        sweeps.compact_rows(raw.double(), cnt, drop)
    with pytest.raises(ValueError, match="count_raw must be torch.int32"):
        sweeps.compact_rows(raw, cnt.long(), drop)
    with pytest.raises(ValueError, match="count_raw must be"):
        sweeps.compact_rows(raw, cnt[:1], drop)
    with pytest.raises(ValueError, match="drop must be torch.bool or torch.uint8"):
        sweeps.compact_rows(raw, cnt, drop.int())
    with pytest.raises(ValueError, match="drop must be"):
        sweeps.compact_rows(raw, cnt, drop[:, :-1])
    with pytest.raises(ValueError, match="N >= 1"):
        sweeps.compact_rows(raw[:, :0], cnt, drop[:, :0])
    with pytest.raises(ValueError, match="idx_c must be torch.int64"):
        sweeps.compose_flow(raw, cnt, T, pos_of, flow, idx.int(), m)
    with pytest.raises(ValueError, match="T must be"):
        sweeps.compose_flow(raw, cnt, T[:, :3], pos_of, flow, idx, m)
    with pytest.raises(ValueError, match="pos_of must be"):
        sweeps.compose_flow(raw, cnt, T, pos_of.long(), flow, idx, m)
    with pytest.raises(ValueError, match="Nc >= 1"):
        sweeps.compose_flow(raw, cnt, T, pos_of, flow[:, :0], idx[:, :0], m)
    # the entry points' own guards: no launch, a negative status
    assert int(call("df_sweep_compact_ws_bytes", 0, N)) < 0 and int(call("df_sweep_compact_ws_bytes", 2, 0)) < 0
    assert int(call("df_flow_compose_ws_bytes", 65536, N)) < 0 and int(call("df_flow_compose_ws_bytes", 65535, 40000)) < 0    # B N >= 2^31
    ws = torch.zeros(64, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="DF_E_SHAPE"):
        call("df_sweep_compact", ptr(raw), ptr(cnt), ptr(drop), 2, 0, ptr(ws), ptr(pc), ptr(row_of), ptr(pos_of), ptr(kept), None)
    with pytest.raises(RuntimeError, match="DF_E_ARG"):
        call("df_sweep_compact", None, ptr(cnt), ptr(drop), 2, N, ptr(ws), ptr(pc), ptr(row_of), ptr(pos_of), ptr(kept), None)
    est = torch.zeros(2, N, 3, device=dev)
    dyn = torch.zeros(2, N, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="DF_E_ARG"):
        call("df_flow_compose", ptr(raw), ptr(cnt), ptr(T), ptr(pos_of), ptr(flow), ptr(idx), ptr(m), 2, N, N, 2, ptr(ws), ptr(est), ptr(dyn), None)
    with pytest.raises(RuntimeError, match="DF_E_SHAPE"):
        call("df_flow_compose", ptr(raw), ptr(cnt), ptr(T), ptr(pos_of), ptr(flow), ptr(idx), ptr(m), 2, N, 0, 0, ptr(ws), ptr(est), ptr(dyn), None)
