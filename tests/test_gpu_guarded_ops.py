"""GPU: every point-cloud entry point run on buffers of exactly the size include/deflow_amd.h states, between guard bytes.

Each scenario goes three times through the PUBLIC wrapper: plain, then twice with the ``call`` / ``ptr`` names of the op modules replaced
by tests/helpers/guarded.py's shim, with fill 0xA5 and with fill 0x7F.  The shim asserts that the wrapper's tensors are at least as large
as tests/helpers/abi_sizes.py (the header's sizes; a workspace: what its df_*_ws_bytes returns) says, runs the entry on regions of exactly
that size at addresses that are 16 mod 32, and asserts that no byte around them changed.  Every returned tensor the header says is written
completely must be bit-identical across the three runs (all these ops document bit-identical repeats): a read past an input or into a
workspace's guard shows as a difference between the fills.  B = 3 with counts (N, N // 2 + 1, 0) and NaN rows behind the counts; N is one
past the op's largest row tile; grids are small and no multiples of 8.

Outputs that the header does NOT promise completely are compared where it does: df_cell_sort's idx_sorted up to the number of keys below
ncells, df_submit_pack's body up to each sample's L(kept).

No entry point, workspace query or wrapper was found wanting: every guard held and every output came back bit-identical at both fills.

Measured on an MI355X: the 28 tests take 1.0 s together (the slowest, the first one, 0.8 s with the context's start; every other one
under 0.15 s); the whole GPU suite's tests take 360 s with this module and 359 s without it, in the same run."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi_sizes  # noqa: E402
import guarded  # noqa: E402

pytestmark = pytest.mark.gpu

B = 3
RANGE = (-4.0, -4.0, 4.4, 4.4)        # DBSCAN's cell 0.70175 -> G = 12, the 0.5 m search grid -> G = 17
FILLS = (0xA5, 0x7F)
WS_SEEN = set()                        # (query, arguments) of every workspace the guarded runs sized
ENTRIES_SEEN = set()                   # every entry that went through the shim
_DBSCAN = ["df_nn_grid_build", "df_dbscan_core", "df_dbscan_link", "df_dbscan_finish"]
EXPECT = {                             # family -> the entries its scenario must send through the shim; together: the whole table
    "cell_sort": ["df_cell_sort"],
    "chamfer": ["df_nn_grid_build", "df_chamfer_nn", "df_chamfer_bwd"],
    "dbscan": _DBSCAN,
    "voidmap": ["df_void_cast", "df_void_merge", "df_void_query"],
    "ground": ["df_ground_cells", "df_ground_height", "df_ground_mask"],
    "metrics": ["df_metrics_rows", "df_metrics_accumulate"],
    "sweep": ["df_sweep_compact", "df_flow_compose"],
    "submit": ["df_sweep_compact", "df_submit_pack"],
    "augment": ["df_augment", "df_augment_params"],
    "render": ["df_render_splat", "df_render_resolve"],
    "rigid": _DBSCAN + ["df_rigid_segments", "df_rigid_vote", "df_rigid_icp", "df_rigid_apply"],
    "mlp": ["df_mlp_fwd", "df_mlp_bwd"],
    "dt": ["df_dt_build", "df_dt_lookup"],
    "iso": ["df_rigid_segments", "df_iso_plan", "df_iso_pairs"],
    "vox": ["df_vox_plan", "df_vox_sample", "df_vox_scatter", "df_vox_smooth"],
    "refine": _DBSCAN + ["df_rigid_segments", "df_refine_fit", "df_refine_apply", "df_chamfer_nn", "df_refine_score"],
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def counts(N, dev):
    return torch.tensor([N, N // 2 + 1, 0], dtype=torch.int32, device=dev)


def cloud(N, seed, dev, cnt=None, lo=(-3.5, -3.5, -1.0), hi=(3.5, 3.5, 1.0), blobs=0):
    """[B,N,3] f32: uniform in the box, or `blobs` tight clusters (DBSCAN finds them); NaN rows behind the counts"""
    g = torch.Generator().manual_seed(seed)
    lo_t, hi_t = torch.tensor(lo), torch.tensor(hi)
    if blobs:
        c = lo_t + (hi_t - lo_t) * (0.1 + 0.8 * torch.rand(B, blobs, 3, generator=g))
        which = torch.randint(0, blobs, (B, N), generator=g)
        p = torch.gather(c, 1, which[..., None].expand(B, N, 3)) + 0.15 * torch.randn(B, N, 3, generator=g)
    else:
        p = lo_t + (hi_t - lo_t) * torch.rand(B, N, 3, generator=g)
    p = p.float()
    cnt = [N, N // 2 + 1, 0] if cnt is None else cnt
    for b in range(B):
        p[b, cnt[b]:] = float("nan")
    return p.to(dev)


def three_runs(monkeypatch, scenario, expect):
    """plain, fill 0xA5, fill 0x7F -> the plain run's outputs; asserts the guards (inside the shim), that every entry of `expect` really
    went through the shim, and that every output is bit-identical across the three runs"""
    outs = [scenario()]
    for fill in FILLS:
        with monkeypatch.context() as m:
            g = guarded.install(m, fill)
            seen_ws = []
            q = g.query
            g.query = lambda fn, *a: (seen_ws.append((fn, tuple(int(v) for v in a))), q(fn, *a))[1]
            outs.append(scenario())
        torch.cuda.synchronize()
        assert set(expect) <= set(g.seen), (sorted(set(expect) - set(g.seen)), g.seen)
        WS_SEEN.update(s for s in seen_ws if s[0].endswith("_ws_bytes"))
        ENTRIES_SEEN.update(g.seen)
    plain = outs[0]
    for fill, o in zip(FILLS, outs[1:]):
        assert o.keys() == plain.keys()
        for k in plain:
            assert guarded.same_bits(plain[k], o[k]), f"{k} differs between the plain run and the guarded run with fill {fill:#x}"
    return plain


# ---- df_cell_sort -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2049])
def test_cell_sort(dev, monkeypatch, n):
    from deflow_amd import decoder
    if n == 1:
        H, W, yx = 1, 1, torch.zeros(1, 2, dtype=torch.int64)
    else:                                            # 2049 cells: two 2048-cell scan chunks; one run of 17; keys >= ncells
        H, W = 3, 683
        g = torch.Generator().manual_seed(11)
        key = torch.randint(0, H * W, (n,), generator=g)
        key[torch.randperm(n, generator=g)[:40]] += H * W     # y >= H: dropped
        key[100:117] = 1500                          # 17 rows of one cell
        key[n - 1] = H * W - 1
        yx = torch.stack([key // W, key % W], dim=1)
    coords = torch.cat([torch.zeros(n, 1, dtype=torch.int64), yx], dim=1).to(torch.int32)
    info = [{"voxel_coords": coords, "point_offsets": torch.zeros(n, 3)}]
    valid = int(((yx[:, 0] * W + yx[:, 1]) < H * W).sum())

    def scenario():
        ps = decoder.pack_infos(info, H, W, dev, need_bwd=True)
        return {"cell_rng": ps.cell_rng, "idx_sorted": ps.idx_sorted[:valid]}

    out = three_runs(monkeypatch, scenario, EXPECT["cell_sort"])
    assert int(out["cell_rng"][-1, 1]) == valid
    if n > 1:
        s, e = out["cell_rng"][1500].tolist()
        assert e - s >= 17


# ---- chamfer ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_dist2", [math.inf, 4.0])
def test_chamfer(dev, monkeypatch, max_dist2):
    from deflow_amd import chamfer
    Nq, Nr = 257, 513
    qc, rc = counts(Nq, dev), counts(Nr, dev)
    query, ref = cloud(Nq, 1, dev), cloud(Nr, 2, dev)
    g = torch.Generator().manual_seed(3)
    ql = (torch.rand(B, Nq, generator=g) < 0.9).to(torch.int32).to(dev)
    rl = (torch.rand(B, Nr, generator=g) < 0.9).to(torch.int32).to(dev) * 2
    gr = torch.randn(B, Nq, generator=g).to(dev)

    def scenario():
        far = torch.zeros(1, dtype=torch.int32, device=dev)
        d2, idx = chamfer.chamfer_nn(query, qc, ref, rc, ql, rl, max_dist2, grid_range=(-4.0, -4.0, 4.0, 4.0), cell=1.0, far_count=far)
        out = {"d2": d2, "idx": idx, "far": far}
        gz = torch.where(idx >= 0, gr, torch.zeros_like(gr))
        q0, r0 = torch.nan_to_num(query), torch.nan_to_num(ref)
        for name, want_q, want_r in (("both", True, True), ("dquery", True, False), ("dref", False, True)):
            dq = torch.zeros_like(query) if want_q else None
            dr = torch.zeros_like(ref) if want_r else None
            chamfer.chamfer_bwd(q0, r0, idx, gz, dq, dr)
            if want_q:
                out[name + ".dq"] = dq
            if want_r:
                out[name + ".dr"] = dr
        return out

    out = three_runs(monkeypatch, scenario, EXPECT["chamfer"])
    assert int((out["idx"][0] >= 0).sum()) > 100 and int((out["idx"][2] >= 0).sum()) == 0
    assert torch.equal(out["both.dq"], out["dquery.dq"]) and torch.equal(out["both.dr"], out["dref.dr"])


# ---- DBSCAN -------------------------------------------------------------------------------------------------------------------------------
def test_dbscan(dev, monkeypatch):
    from deflow_amd import cluster
    N = 257
    cnt = counts(N, dev)
    pts = cloud(N, 4, dev, blobs=5)
    g = torch.Generator().manual_seed(5)
    mask = (torch.rand(B, N, generator=g) < 0.9).to(dev)
    dyn = (torch.rand(B, N, generator=g) < 0.5).to(dev)

    def scenario():
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        lab, ncl = cluster.dbscan(pts, cnt, mask, eps=0.7, min_points=4, min_cluster_size=5, grid_range=RANGE, status=st)
        lab2, ncl2, st2 = cluster.dynamic_cluster_labels(pts, cnt, dyn, grid_range=RANGE)
        return {"labels": lab, "n": ncl, "status": st, "labels_dyn": lab2, "n_dyn": ncl2, "status_dyn": st2}

    out = three_runs(monkeypatch, scenario, EXPECT["dbscan"])
    assert int(out["n"][0]) >= 2 and int(out["n"][2]) == 0 and int(out["status"]) == 0 and int(out["status_dyn"]) == 0


# ---- void map -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("erode", [0, 1, 2])
def test_voidmap(dev, monkeypatch, erode):
    from deflow_amd.voidmap import VoidMap
    N = 257
    cnt = counts(N, dev)
    pts = cloud(N, 6, dev, lo=(-1.7, -0.3, -0.2), hi=(1.7, 0.3, 0.2))          # a few rows outside the 32 x 5 x 3 grid of 0.1 m voxels
    origin = torch.tensor([[0.01, 0.02, 0.0], [-1.0, 0.1, 0.05], [0.0, 0.0, 0.0]], device=dev)

    def scenario():
        vm = VoidMap(B, (-1.6, -0.25, -0.15), (32, 5, 3), 0.1, hit_margin=1, erode=erode, max_range=80.0, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        vm.integrate(pts, cnt, origin, st)
        flags = vm.query(pts, cnt)
        return {"V": vm.words.view(torch.int32), "F": vm.last_free.view(torch.int32), "O": vm.last_occ.view(torch.int32),
                "flags": flags, "status": st}

    out = three_runs(monkeypatch, scenario, EXPECT["voidmap"])
    assert int((out["F"] != 0).sum()) > 0 and int((out["O"][2] != 0).sum()) == 0 and int(out["status"]) == 0


# ---- ground -------------------------------------------------------------------------------------------------------------------------------
def test_ground(dev, monkeypatch):
    from deflow_amd.ground import GroundSegmenter
    N = 257
    cnt = counts(N, dev)
    pts = cloud(N, 7, dev, lo=(-2.8, -3.8, -0.6), hi=(2.8, 3.8, 0.4))           # a few rows outside the 5 x 7 grid of 1 m cells

    def scenario():
        seg = GroundSegmenter(B, xy_min=(-2.5, -3.5), cell=1.0, dims=(5, 7), device=dev)
        m = seg.segment(pts, cnt)
        return {"mask": m, "zmin": seg.cell_min, "height": seg.height, "observed": seg.observed}

    out = three_runs(monkeypatch, scenario, EXPECT["ground"])
    assert 0 < int(out["mask"][0].sum()) < N and int(out["mask"][2].sum()) == 0


# ---- metrics ------------------------------------------------------------------------------------------------------------------------------
def test_metrics(dev, monkeypatch):
    from deflow_amd import metrics_device
    N = metrics_device.rows_per_block() + 1
    cnt = counts(N, dev)
    g = torch.Generator().manual_seed(8)
    pc0 = cloud(N, 9, dev, cnt=[N, N, N], lo=(-40.0, -40.0, -1.0), hi=(40.0, 40.0, 1.0))
    gt = (0.3 * torch.randn(B, N, 3, generator=g)).to(dev)
    pose = (0.05 * torch.randn(B, N, 3, generator=g)).to(dev)
    flow = gt - pose + (0.05 * torch.randn(B, N, 3, generator=g)).to(dev)
    for b in range(B):
        flow[b, int(cnt[b]):] = float("nan")
    idx_c = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(dev)
    valid = (torch.rand(B, N, generator=g) < 0.9).to(dev)
    emask = (torch.rand(B, N, generator=g) < 0.8).to(dev)
    cats = torch.randint(0, 31, (B, N), generator=g).to(torch.uint8).to(dev)
    has = torch.tensor([1, 1, 0], dtype=torch.uint8, device=dev)

    def scenario():
        dm = metrics_device.DeviceMetrics(dev)
        dm.update(flow, pose, pc0, gt, idx_c, cnt, is_valid=valid, eval_mask=emask, categories=cats, has_eval_mask=has)
        return {"state": dm._state.clone(), "status": dm.status.clone()}

    out = three_runs(monkeypatch, scenario, EXPECT["metrics"])
    assert int(out["status"]) == 0 and int((out["state"] != 0).sum()) > 20


# ---- whole-sweep flow ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [0, 1])
def test_sweep(dev, monkeypatch, half):
    from deflow_amd import sweeps
    N, Nc = sweeps.rows_per_block() + 1, 257
    cnt_raw, cnt = counts(N, dev), counts(Nc, dev)
    raw = cloud(N, 10, dev)
    raw[0, 5] = float("inf")
    g = torch.Generator().manual_seed(12)
    drop = (torch.rand(B, N, generator=g) < 0.3).to(dev)
    T = torch.eye(4).repeat(B, 1, 1)
    T[:, :3, 3] = torch.randn(B, 3, generator=g) * 0.1
    T = T.to(dev)
    flow = (0.1 * torch.randn(B, Nc, 3, generator=g)).to(dev)
    idx_c = torch.stack([torch.randperm(N, generator=g)[:Nc] for _ in range(B)]).to(dev)

    def scenario():
        pc, row_of, pos_of, kept = sweeps.compact_rows(raw, cnt_raw, drop)
        est, dyn = sweeps.compose_flow(raw, cnt_raw, T, pos_of, flow, idx_c, cnt, half=bool(half))
        return {"pc": pc, "row_of": row_of, "pos_of": pos_of, "kept": kept, "est": est, "dyn": dyn}

    out = three_runs(monkeypatch, scenario, EXPECT["sweep"])
    assert 0 < int(out["kept"][0]) < N and int(out["kept"][2]) == 0
    assert out["est"].dtype == (torch.float16 if half else torch.float32)


# ---- submission ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
def test_submit(dev, monkeypatch, version):
    from deflow_amd import feather, submit
    N = 257
    cnt = counts(N, dev)
    g = torch.Generator().manual_seed(13)
    est = torch.randn(B, N, 3, generator=g).to(dev)
    dyn = (torch.rand(B, N, generator=g) < 0.4).to(torch.uint8).to(dev)
    emask = (torch.rand(B, N, generator=g) < 0.7).to(dev)

    def scenario():
        body, kept = submit.pack_rows(est, dyn, emask, cnt, version)
        out = {"kept": kept}
        for b, m in enumerate(kept.tolist()):
            out[f"body{b}"] = body[b, :feather.body_len(m)]
        return out

    out = three_runs(monkeypatch, scenario, EXPECT["submit"])
    assert 100 < int(out["kept"][0]) < N and int(out["kept"][2]) == 0 and out["body0"].numel() > 600


# ---- augmentation -------------------------------------------------------------------------------------------------------------------------
def test_augment(dev, monkeypatch):
    from deflow_amd.augment import Augmenter
    N = 257
    g = torch.Generator().manual_seed(14)
    pose = lambda: torch.cat([torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0], torch.randn(B, 3, 1, generator=g)], dim=2)
    full = lambda p: torch.cat([p, torch.tensor([0.0, 0.0, 0.0, 1.0]).expand(B, 1, 4)], dim=1).to(dev)
    batch = {"pc0": cloud(N, 15, dev), "pc1": cloud(N, 16, dev), "flow": torch.randn(B, N, 3, generator=g).to(dev),
             "ego_motion": full(pose()), "pose0": full(pose()), "pose1": full(pose())}
    ids = torch.tensor([1234567890123, -5, 0], dtype=torch.int64, device=dev)
    aug = Augmenter(7, flip_x_p=0.5, flip_y_p=0.5, yaw_deg=10.0, height=0.2, jitter_sigma=0.01, drop_p=0.1)

    def scenario():
        r = aug(batch, ids, 3)
        out = {k: r[k] for k in ("pc0", "pc1", "flow", "ego_motion", "pose0", "pose1")}
        out["params"] = aug.params(ids, 3)
        return out

    out = three_runs(monkeypatch, scenario, EXPECT["augment"])
    assert not torch.equal(torch.nan_to_num(out["pc0"]), torch.nan_to_num(batch["pc0"]))


# ---- rendering ----------------------------------------------------------------------------------------------------------------------------
def test_render(dev, monkeypatch):
    from deflow_amd import render
    N = 257
    cnt = counts(N, dev)
    pts = cloud(N, 17, dev, lo=(-4.3, -2.3, -1.0), hi=(4.3, 2.3, 1.0))          # a few rows outside the 33 x 17 image
    g = torch.Generator().manual_seed(18)
    vec = torch.randn(B, N, 3, generator=g).to(dev)
    cls = torch.randint(0, 3, (B, N), generator=g).to(torch.uint8).to(dev)

    def scenario():
        return {"lines": render.render_rows(pts, cnt, vec, cls, view=(-4.0, -2.0, 4.0), size=(33, 17), vmax=1.0, radius=1, legend=4)}

    out = three_runs(monkeypatch, scenario, EXPECT["render"])
    assert tuple(out["lines"].shape) == (B, 17, 100) and not torch.equal(out["lines"][0], out["lines"][2])


# ---- rigid cluster flow -------------------------------------------------------------------------------------------------------------------
def _pair(dev, N0, N1, seed):
    """a blobby first sweep and a second one that is its first rows, shifted; counts with one empty sample"""
    c0, c1 = [N0, N0 // 2 + 1, 0], [N1, N1 // 2 + 1, 0]
    p0 = cloud(N0, seed, dev, cnt=c0, blobs=4)
    p1 = torch.full((B, N1, 3), float("nan"), device=dev)
    for b in range(B):
        k = min(c1[b], c0[b])
        p1[b, :k] = p0[b, :k] + torch.tensor([0.2, 0.05, 0.0], device=dev)
    return p0, torch.tensor(c0, dtype=torch.int32, device=dev), p1, torch.tensor(c1, dtype=torch.int32, device=dev)


def test_rigid(dev, monkeypatch):
    from deflow_amd import rigid
    p0, c0, p1, c1 = _pair(dev, 257, 130, 19)

    def scenario():
        flow, rid, table, vote, st, hist = rigid.rigid_cluster_flow(p0, c0, p1, c1, grid_range=RANGE, return_hist=True)
        return {"flow": flow, "rigid_id": rid, "table": table, "vote": vote, "status": st, "hist": hist}

    out = three_runs(monkeypatch, scenario, EXPECT["rigid"])
    assert int(out["status"]) == 0 and int((out["table"][0, :, 5] > 0).sum()) >= 1 and int((out["table"][2, :, 7] != 0).sum()) == 0


# ---- MLP ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,depth", [(65, 0), (65, 1), (1025, 1)])
def test_mlp(dev, monkeypatch, N, depth):
    from deflow_amd import nsfp
    cnt = counts(N, dev)
    x = cloud(N, 20, dev)
    g = torch.Generator().manual_seed(21)
    params = (0.2 * torch.randn(B, nsfp.param_stride(depth), generator=g)).to(dev)
    dy = torch.randn(B, N, 3, generator=g).to(dev)
    for b in range(B):
        dy[b, int(cnt[b]):] = float("nan")

    def scenario():
        y, acts = nsfp.mlp_forward(x, cnt, params, depth)
        dparams, dx = nsfp.mlp_backward(x, cnt, params, depth, acts, dy)
        return {"y": y, "acts": acts, "dparams": dparams, "dx": dx}

    out = three_runs(monkeypatch, scenario, EXPECT["mlp"])
    assert bool(torch.isfinite(out["dparams"]).all()) and float(out["dparams"][0].abs().sum()) > 0 and float(out["dparams"][2].abs().sum()) == 0


# ---- distance transform -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,R", [((257, 3, 2), 2), ((5, 4, 3), 3)])
def test_dt(dev, monkeypatch, dims, R):
    from deflow_amd import fastnsf
    N, cell = 257, 0.5
    cnt = counts(N, dev)
    hi = tuple(d * cell + 0.3 for d in dims)
    ref = cloud(N, 22, dev, lo=(-0.3, -0.3, -0.3), hi=hi)                       # a few rows outside the grid
    query = cloud(N, 23, dev, lo=(-0.6, -0.6, -0.6), hi=tuple(h + 0.3 for h in hi))
    query[0, 3, 1] = float("inf")
    kw = dict(origin=(0.0, 0.0, 0.0), cell=cell, radius=R)

    def scenario():
        dt2 = fastnsf.dt_build(ref, cnt, dims=dims, **kw)
        d, g, cells, clamped = fastnsf.dt_lookup(query, cnt, dt2, return_cells=True, **kw)
        return {"dt2": dt2.view(torch.int16), "d": d, "g": g, "cells": cells, "clamped": clamped}

    out = three_runs(monkeypatch, scenario, EXPECT["dt"])
    assert int((out["dt2"][0] == 0).sum()) > 0 and int((out["dt2"][2] != R * R).sum()) == 0


# ---- rigidity term ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 4])
def test_iso(dev, monkeypatch, P):
    from deflow_amd import mbnsf
    N = 257
    cnt = counts(N, dev)
    x = torch.nan_to_num(cloud(N, 24, dev))
    g = torch.Generator().manual_seed(25)
    labels = torch.randint(0, 6, (B, N), generator=g).to(torch.int32).to(dev)
    w = x + (0.1 * torch.randn(B, N, 3, generator=g)).to(dev)

    def scenario():
        nbr, r0, n_pairs = mbnsf.iso_plan(x, cnt, labels, pairs=P, max_cluster_points=8192)
        v, gr = mbnsf.iso_pairs(w, nbr, r0, delta=0.1)
        return {"nbr": nbr, "r0": r0, "pairs": n_pairs, "v": v, "g": gr}

    out = three_runs(monkeypatch, scenario, EXPECT["iso"])
    assert int(out["pairs"][0]) > P * 100 and int(out["pairs"][2]) == 0


# ---- voxel flow ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(2, 2, 2), (5, 4, 3)])
def test_vox(dev, monkeypatch, dims):
    from deflow_amd import floxels
    N, voxel = 257, 0.5
    cnt = counts(N, dev)
    hi = tuple((d - 1) * voxel + 0.2 for d in dims)
    x = cloud(N, 26, dev, lo=(-0.2, -0.2, -0.2), hi=hi)
    g = torch.Generator().manual_seed(27)
    theta = torch.randn(B, dims[2], dims[1], dims[0], 3, generator=g).to(dev)
    dF = torch.randn(B, N, 3, generator=g).to(dev)
    for b in range(B):
        dF[b, int(cnt[b]):] = float("nan")

    def scenario():
        plan = floxels.vox_plan(x, cnt, origin=(0.0, 0.0, 0.0), voxel=voxel, dims=dims)
        F = floxels.vox_sample(theta, plan["cell"], plan["frac"])
        dtheta = floxels.vox_scatter(dF, plan["frac"], plan["idx_sorted"], plan["cell_rng"], dims=dims)
        v, gr = floxels.vox_smooth(theta, plan["active"])
        out = {k: plan[k] for k in ("cell", "frac", "idx_sorted", "cell_rng", "active", "pairs")}
        out.update(F=F, dtheta=dtheta, v=v, g=gr)
        return out

    out = three_runs(monkeypatch, scenario, EXPECT["vox"])
    assert int(out["pairs"][0]) > 0 and int(out["pairs"][2]) == 0 and bool(torch.isfinite(out["dtheta"]).all())


# ---- refine -------------------------------------------------------------------------------------------------------------------------------
def test_refine(dev, monkeypatch):
    from deflow_amd import refine
    x, c0, p1, c1 = _pair(dev, 257, 130, 28)
    g = torch.Generator().manual_seed(29)
    flow = (torch.tensor([0.2, 0.05, 0.0]) + 0.02 * torch.randn(B, 257, 3, generator=g)).to(dev)
    for b in range(B):
        flow[b, int(c0[b]):] = float("nan")

    def scenario():
        out, info = refine.rigid_refine(x, c0, flow, p1, c1, grid_range=RANGE)
        return {"flow_out": out, "table": info["table"], "rigid_id": info["rigid_id"], "labels": info["labels"], "anchor": info["anchor"],
                "status": info["cluster_status"]}

    out = three_runs(monkeypatch, scenario, EXPECT["refine"])
    assert int(out["status"]) == 0 and int((out["table"][0, :, 6] > 0).sum()) >= 1 and int((out["rigid_id"][2] != 0).sum()) == 0


# ---- the shared checks and the row grid the wrappers above are written on (not guarded: the scenarios above are) ---------------------------
def test_args_tensor_and_row_grid(dev):
    from deflow_amd import args, chamfer
    g = torch.Generator().manual_seed(31)
    x = (4.0 * torch.rand(2, 5, 3, generator=g) - 2.0).to(dev)
    cnt = torch.tensor([5, 3], dtype=torch.int32, device=dev)
    assert args.tensor("op", "x", x, torch.float32, (2, 5, 3), dev, "y is") is x and args.cloud("op", "x", x, 3) == (2, 5)
    with pytest.raises(ValueError, match=r"op: x must be torch.int32 of shape \(2, 5, 3\), got torch.float32 \(2, 5, 3\)"):
        args.tensor("op", "x", x, torch.int32, (2, 5, 3))
    with pytest.raises(ValueError, match=r"op: x must be torch.bool or torch.uint8 of shape \(2, 5\), got torch.float32 \(2, 5, 3\)"):
        args.tensor("op", "x", x, (torch.bool, torch.uint8), (2, 5))
    with pytest.raises(ValueError, match=r"op: cnt must be torch.float32 of shape \(B, N, 3\) with B >= 1 and N >= 1, got torch.int32 \(2,\)"):
        args.cloud("op", "cnt", cnt)
    if torch.cuda.device_count() > 1:
        other = torch.device("cuda", (dev.index + 1) % torch.cuda.device_count())
        with pytest.raises(ValueError, match=f"op: x is on {dev}, y is on {other}"):
            args.tensor("op", "x", x, torch.float32, (2, 5, 3), other, "y is")
    # file + nn are chamfer_nn, bit for bit (one sample with rows behind its count, a gate that cuts some pairs)
    ref = (4.0 * torch.rand(2, 5, 3, generator=g) - 2.0).to(dev)
    rng, cell, gate = (-2.0, -2.0, 2.0, 2.0), 1.0, 2.5
    grid = chamfer.RowGrid(2, rng, cell, dev)
    d2, idx = grid.nn(x, cnt, None, grid.file(ref, cnt), gate)
    want_d2, want_idx = chamfer.chamfer_nn(x, cnt, ref, cnt, max_dist2=gate, grid_range=rng, cell=cell)
    assert guarded.same_bits(d2, want_d2) and guarded.same_bits(idx, want_idx)
    assert int((idx[0] >= 0).sum()) >= 1 and bool((idx[1, 3:] == -1).all())


# ---- the table covers what ran ------------------------------------------------------------------------------------------------------------
def test_the_scenarios_cover_the_table_and_the_cpu_modules_workspace_cases():
    """the scenarios' entry lists are the whole table; and what the guarded runs of this process asked the df_*_ws_bytes functions is
    among the cases tests/test_abi_sizes_cpu.py holds positive without a GPU -- all of them, once every scenario has run"""
    assert {e for v in EXPECT.values() for e in v} == set(abi_sizes.TABLE)
    cases = {(fn, tuple(a)) for fn, sets in abi_sizes.ws_cases().items() for a in sets}
    assert WS_SEEN <= cases, sorted(WS_SEEN - cases)
    if ENTRIES_SEEN == set(abi_sizes.TABLE):
        assert WS_SEEN == cases, sorted(cases - WS_SEEN)
