"""CPU: the DBSCAN feature's plumbing -- the float64 helper (tests/helpers/dbscan_ref.py) on hand-made cases and against sklearn, the new
C-ABI entries' argument checks, the absence of a CPU fallback, the command line, the collate and the scene-file reader."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from dbscan_ref import blob_scatter, dbscan_ref, dbscan_ref_padded  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the helper on hand-made cases ------------------------------------------------------------------------------------------------------
def two_blobs():
    g = torch.Generator().manual_seed(1)
    a = torch.randn(40, 3, generator=g) * 0.15 + torch.tensor([5.0, 5.0, 0.0])
    b = torch.randn(30, 3, generator=g) * 0.15 + torch.tensor([-5.0, 2.0, 0.5])
    noise = torch.tensor([[20.0, 20.0, 0.0], [-20.0, 0.0, 0.0], [0.0, -30.0, 1.0]])
    return torch.cat([noise[:1], b, noise[1:2], a, noise[2:]])      # rows: 0 noise, 1..30 b, 31 noise, 32..71 a, 72 noise


def test_helper_two_blobs_and_noise():
    r = dbscan_ref(two_blobs(), eps=0.7, min_points=4)
    lab = r["labels"]
    assert r["n_clusters"] == 2 and r["band_pairs"] == 0
    assert lab[[0, 31, 72]].tolist() == [0, 0, 0]
    assert bool((lab[1:31] == 1).all()) and bool((lab[32:72] == 2).all())        # numbered by lowest core row: b first
    assert int(r["core"].sum()) == 70 and int(r["border"].sum()) == 0


def test_helper_chain_and_numbering_order():
    # a chain of 50 rows 0.5 m apart: every row has >= 2 rows within 0.7 m; one cluster with min_points 2, none with min_points 4
    x = torch.arange(50, dtype=torch.float32) * 0.5
    chain = torch.stack([x, torch.zeros(50), torch.zeros(50)], 1)
    perm = torch.randperm(50, generator=torch.Generator().manual_seed(2))
    r = dbscan_ref(chain[perm], eps=0.7, min_points=2)
    assert r["n_clusters"] == 1 and bool((r["labels"] == 1).all()) and bool((r["root"] == 0).all())
    assert dbscan_ref(chain[perm], eps=0.7, min_points=4)["n_clusters"] == 0
    # interior rows have 3 rows within eps, the two ends 2: with min_points 3 the ends are border rows
    r = dbscan_ref(chain, eps=0.7, min_points=3)
    assert r["border"].nonzero()[:, 0].tolist() == [0, 49] and bool((r["labels"] == 1).all())
    # numbering: ascending lowest core row, whatever the position in space
    three = torch.cat([chain[:10] + torch.tensor([100.0, 0, 0]), chain[:10] - torch.tensor([100.0, 0, 0]), chain[:10]])
    r = dbscan_ref(three, eps=0.7, min_points=2)
    assert r["labels"].tolist() == [1] * 10 + [2] * 10 + [3] * 10
    order = torch.tensor([25, 5, 15] + [i for i in range(30) if i not in (25, 5, 15)])
    r = dbscan_ref(three[order], eps=0.7, min_points=2)
    assert r["labels"][:3].tolist() == [1, 2, 3]


def test_helper_equidistant_border_row_goes_to_the_lower_row():
    right = torch.tensor([[0.6, 0.0, 0.0], [0.9, 0.0, 0.0], [0.9, 0.25, 0.0], [1.1, 0.0, 0.25]])
    left = right * torch.tensor([-1.0, 1.0, 1.0])
    mid = torch.tensor([[0.0, 0.0, 0.0]])
    pts = torch.cat([right[1:], left[1:], mid, right[:1], left[:1]])         # the two nearest core rows: 7 (right) and 8 (left)
    r = dbscan_ref(pts, eps=0.7, min_points=4)
    assert r["border"].tolist() == [False] * 6 + [True, False, False] and r["border_ties"] == 0
    assert r["labels"].tolist() == [1, 1, 1, 2, 2, 2, 1, 1, 2]
    sw = pts.clone()
    sw[[7, 8]] = pts[[8, 7]]
    r = dbscan_ref(sw, eps=0.7, min_points=4)
    assert int(r["labels"][6]) == int(r["labels"][7]) == 2                   # row 7 is the left-hand one now (cluster 2: lowest core row 3)
    # a NEAR tie is reported, not decided silently
    near = pts.clone()
    near[8, 0] -= 1e-7
    assert dbscan_ref(near, eps=0.7, min_points=4)["border_ties"] == 1


def test_helper_duplicates_counts_mask_and_bad_rows():
    pts = torch.tensor([[1.0, 2.0, 3.0]]).repeat(6, 1)
    assert dbscan_ref(pts, eps=0.1, min_points=6)["labels"].tolist() == [1] * 6
    assert dbscan_ref(pts, eps=0.1, min_points=7)["labels"].tolist() == [0] * 6
    assert dbscan_ref(pts, count=4, eps=0.1, min_points=4)["labels"].tolist() == [1, 1, 1, 1, 0, 0]
    assert dbscan_ref(pts, mask=torch.tensor([1, 0, -1, 2, 0, 3]), eps=0.1, min_points=4)["labels"].tolist() == [1, 0, 1, 1, 0, 1]
    bad = pts.clone()
    bad[2, 1] = float("nan")
    bad[3, 0] = float("inf")
    assert dbscan_ref(bad, eps=0.1, min_points=4)["labels"].tolist() == [1, 1, 0, 0, 1, 1]
    assert dbscan_ref(bad, eps=0.1, min_points=5)["n_clusters"] == 0


def test_helper_filters():
    pts = two_blobs()
    dyn = torch.zeros(73, dtype=torch.bool)
    dyn[1:10] = True                 # 9 of blob b's 30 members: exactly 0.3 -- kept (flagged < frac * members drops)
    dyn[32:43] = True                # 11 of blob a's 40: 0.275 -- dropped
    r = dbscan_ref(pts, dynamic=dyn, eps=0.7, min_points=4, min_cluster_size=20, min_dynamic_frac=0.3)
    assert r["n_clusters"] == 1 and bool((r["labels"][1:31] == 1).all()) and bool((r["labels"][32:72] == 0).all())
    dyn[43] = True                   # 12 of 40: kept, and numbered second
    r = dbscan_ref(pts, dynamic=dyn, eps=0.7, min_points=4, min_cluster_size=20, min_dynamic_frac=0.3)
    assert r["n_clusters"] == 2 and bool((r["labels"][32:72] == 2).all())
    r = dbscan_ref(pts, dynamic=dyn, eps=0.7, min_points=4, min_cluster_size=31, min_dynamic_frac=0.3)      # the size filter drops b
    assert r["n_clusters"] == 1 and bool((r["labels"][1:31] == 0).all()) and bool((r["labels"][32:72] == 1).all())
    r = dbscan_ref(pts, eps=0.7, min_points=4, min_cluster_size=41)
    assert r["n_clusters"] == 0 and int(r["core"].sum()) == 70


def test_helper_equals_sklearn_on_the_blob_case():
    """core flags and the partition of the core rows equal sklearn.cluster.DBSCAN's (border rows are assigned by visiting order there)"""
    sk = pytest.importorskip("sklearn.cluster")
    pts = blob_scatter(seed=1)
    r = dbscan_ref(pts, eps=0.7, min_points=4)
    assert r["band_pairs"] == 0 and r["border_ties"] == 0
    print(f"blob case: {r['n_clusters']} clusters, {int(r['core'].sum())} core rows, {int(r['border'].sum())} border rows")
    assert r["n_clusters"] > 40 and int(r["border"].sum()) > 50
    m = sk.DBSCAN(eps=0.7, min_samples=4, algorithm="brute").fit(pts.double().numpy())
    core = torch.zeros(pts.shape[0], dtype=torch.bool)
    core[torch.from_numpy(m.core_sample_indices_).long()] = True
    assert torch.equal(core, r["core"])
    ours, theirs = r["root"][core], torch.from_numpy(m.labels_).long()[core]
    pairs = torch.unique(torch.stack([ours, theirs], 1), dim=0)
    assert len(pairs) == len(torch.unique(ours)) == len(torch.unique(theirs)) == r["n_clusters"]      # a bijection: the same partition


def test_padded_helper():
    pts = torch.stack([two_blobs(), two_blobs().flip(0)])
    lab, k, rep = dbscan_ref_padded(pts, [73, 40], eps=0.7, min_points=4)
    assert k.tolist() == [2, 1] and lab.shape == (2, 73) and rep["band_pairs"] == 0 and bool((lab[1, 40:] == 0).all())


# ---- the library's entries and the Python op --------------------------------------------------------------------------------------------
def test_dbscan_entries_reject_bad_arguments_without_launching():
    """NULL buffers, B <= 0, sizes past the 32-bit key range, a cell below eps: negative DF_E_* codes, no launch (no GPU here)"""
    from deflow_amd import build
    from deflow_amd._lib import load
    build.build()
    lib = load()
    P, F, D = C.c_void_p, C.c_float, C.c_double
    ok = P(0x1000)
    SHAPE, ARG, ALIGN = -1, -3, -2
    # df_dbscan_core(cell_rng, sorted, B, N, minx, miny, cell, G, eps, min_points, ws, stream)
    core = lambda rng=ok, srt=ok, B=2, N=100, cell=0.8, G=16, eps=0.7, mp=4, ws=ok: lib.df_dbscan_core(
        rng, srt, B, N, F(-4.0), F(-4.0), F(cell), G, F(eps), mp, ws, P(0))
    assert core(rng=P(0)) == ARG and core(srt=P(0)) == ARG and core(ws=P(0)) == ARG
    assert core(B=0) == SHAPE and core(B=-1) == SHAPE and core(N=0) == SHAPE and core(G=0) == SHAPE and core(G=5000) == SHAPE
    assert core(B=40000, N=80000) == SHAPE and core(B=64, G=4096) == SHAPE and core(B=70000, N=10) == SHAPE
    assert core(cell=0.5) == ARG and core(eps=0.0) == ARG and core(eps=float("nan")) == ARG and core(cell=float("inf")) == ARG
    assert core(mp=0) == ARG and core(srt=P(0x1004)) == ALIGN and core(ws=P(0x1008)) == ALIGN
    # df_dbscan_link(cell_rng, B, N, minx, miny, cell, G, eps, status, ws, stream)
    link = lambda rng=ok, B=2, N=100, cell=0.8, G=16, eps=0.7, ws=ok: lib.df_dbscan_link(
        rng, B, N, F(-4.0), F(-4.0), F(cell), G, F(eps), P(0), ws, P(0))
    assert link(rng=P(0)) == ARG and link(ws=P(0)) == ARG and link(B=0) == SHAPE and link(N=-5) == SHAPE and link(G=4097) == SHAPE
    assert link(B=40000, N=80000) == SHAPE and link(cell=0.69) == ARG and link(eps=-1.0) == ARG and link(ws=P(0x1004)) == ALIGN
    # df_dbscan_finish(cell_rng, dynamic, B, N, minx, miny, cell, G, eps, min_cluster_size, min_dynamic_frac, labels, n_clusters, status, ws, stream)
    fin = lambda rng=ok, B=2, N=100, cell=0.8, G=16, eps=0.7, mcs=20, frac=0.3, lab=ok, k=ok, ws=ok: lib.df_dbscan_finish(
        rng, P(0), B, N, F(-4.0), F(-4.0), F(cell), G, F(eps), mcs, D(frac), lab, k, P(0), ws, P(0))
    assert fin(rng=P(0)) == ARG and fin(lab=P(0)) == ARG and fin(k=P(0)) == ARG and fin(ws=P(0)) == ARG
    assert fin(B=0) == SHAPE and fin(N=0) == SHAPE and fin(G=0) == SHAPE and fin(B=40000, N=80000) == SHAPE and fin(B=64, G=4096) == SHAPE
    assert fin(mcs=0) == ARG and fin(frac=-0.1) == ARG and fin(frac=float("nan")) == ARG and fin(cell=0.1) == ARG
    lib.df_dbscan_ws_bytes.restype = C.c_int64
    assert lib.df_dbscan_ws_bytes(2, 100) >= 2 * 100 * (16 + 6 * 4) and lib.df_dbscan_ws_bytes(0, 100) == 0
    assert lib.df_dbscan_ws_bytes(40000, 80000) == 0 and lib.df_dbscan_ws_bytes(16, 80000) % 16 == 0


def test_cluster_api_has_no_cpu_fallback():
    import deflow_amd
    from deflow_amd.cluster import dbscan, dynamic_cluster_labels
    assert deflow_amd.dbscan is dbscan and deflow_amd.dynamic_cluster_labels is dynamic_cluster_labels
    p = torch.zeros(1, 8, 3)
    n = torch.full((1,), 8, dtype=torch.int32)
    with pytest.raises(TypeError, match="CUDA"):
        dbscan(p, n)
    with pytest.raises(TypeError, match="CUDA"):
        dynamic_cluster_labels(p, n, torch.ones(1, 8, dtype=torch.bool))
    with pytest.raises(ValueError):
        dbscan(p[0], n)
    with pytest.raises(ValueError):
        dbscan(p, n, eps=-1.0)
    with pytest.raises(ValueError):
        dynamic_cluster_labels(p, n, None)
    src = open(os.path.join(ROOT, "deflow_amd", "cluster.py")).read()
    for word in (".cpu()", ".item()", ".tolist()", "int(labels", "sklearn"):       # no read-back, no other implementation
        assert word not in src, word


def test_trainer_keyword():
    import deflow_amd
    from deflow_amd.optim import Trainer
    m = deflow_amd.DeFlow(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], grid_feature_size=[64, 64], num_iters=2)
    t = Trainer(m, loss_fn="seflowLoss", cluster_labels=dict(eps=0.5, min_cluster_size=10))
    assert t.cluster_labels == {"eps": 0.5, "min_cluster_size": 10} and t.last_cluster_status is None
    assert Trainer(m, loss_fn="seflowLoss", cluster_labels={}).cluster_labels == {}
    assert Trainer(m, loss_fn="seflowLoss").cluster_labels is None
    with pytest.raises(ValueError):
        Trainer(m, loss_fn="seflowLoss", cluster_labels=dict(epsilon=0.5))
    with pytest.raises(ValueError):
        Trainer(m, loss_fn="deflowLoss", cluster_labels={})
    with pytest.raises(ValueError):
        Trainer(m, loss_fn="seflowLoss", cluster_labels="online")
    with pytest.raises(ValueError):                              # loss_args and its validation are as they were
        Trainer(m, loss_fn="seflowLoss", loss_args=dict(eps=0.5))


def test_command_line_keys():
    from deflow_amd.train import cluster_args, parse_overrides
    cfg = parse_overrides(["loss_fn=seflowLoss", "cluster_labels=online", "cluster_eps=0.5", "cluster_min_points=6", "cluster_min_size=30",
                           "cluster_min_dynamic_frac=0.25"])
    assert cluster_args(cfg) == {"eps": 0.5, "min_points": 6, "min_cluster_size": 30, "min_dynamic_frac": 0.25}
    cfg = parse_overrides(["loss_fn=seflowLoss", "cluster_labels=online"])
    assert cluster_args(cfg) == {"eps": 0.7, "min_points": 4, "min_cluster_size": 20, "min_dynamic_frac": 0.3}
    assert cluster_args(parse_overrides(["loss_fn=seflowLoss"])) is None and cluster_args(parse_overrides([])) is None
    with pytest.raises(SystemExit, match="cluster_labels"):
        parse_overrides(["loss_fn=seflowLoss", "cluster_labels=offline"])
    with pytest.raises(SystemExit, match="seflowLoss"):
        parse_overrides(["cluster_labels=online"])
    with pytest.raises(SystemExit, match="seflowLoss"):
        parse_overrides(["loss_fn=deflowLoss", "cluster_labels=online"])


# ---- data -----------------------------------------------------------------------------------------------------------------------------
def test_collate_dynamic_flags():
    from deflow_amd.data import collate_fn_pad

    def item(n0, n1, flagged, seed):
        g = torch.Generator().manual_seed(seed)
        it = {"scene_id": "s", "timestamp": seed, "pc0": torch.randn(n0, 3, generator=g), "pc1": torch.randn(n1, 3, generator=g),
              "gm0": torch.rand(n0, generator=g) < 0.3, "gm1": torch.rand(n1, generator=g) < 0.3, "pose0": torch.eye(4), "pose1": torch.eye(4)}
        if flagged:
            it["dufo0"] = torch.rand(n0, generator=g) < 0.4
            it["dufo1"] = torch.rand(n1, generator=g) < 0.4
        return it

    items = [item(50, 60, True, 1), item(80, 40, True, 2)]
    res = collate_fn_pad(items)
    assert res["pc0_dufo"].shape == res["pc0"].shape[:2] and res["pc1_dufo"].shape == res["pc1"].shape[:2]
    assert not res["pc0_dufo"].dtype.is_floating_point
    for b, it in enumerate(items):
        for key, src, gm in (("pc0_dufo", "dufo0", "gm0"), ("pc1_dufo", "dufo1", "gm1")):
            kept = it[src][~it[gm]].long()
            assert torch.equal(res[key][b, : kept.numel()], kept) and bool((res[key][b, kept.numel():] == 0).all())
    assert "pc0_dynamic" not in res and "max_label" not in res
    plain_items = [item(50, 60, False, 1), item(80, 40, False, 2)]
    plain = collate_fn_pad(plain_items)
    assert "pc0_dufo" not in plain and "pc1_dufo" not in plain
    assert set(plain) == set(res) - {"pc0_dufo", "pc1_dufo"}
    for k in plain:                                             # the other keys are what they were
        same = torch.equal(plain[k], res[k]) if isinstance(plain[k], torch.Tensor) and not plain[k].is_floating_point() else True
        assert same, k
    assert torch.equal(torch.nan_to_num(plain["pc0"]), torch.nan_to_num(res["pc0"]))
    mixed = collate_fn_pad([item(50, 60, True, 1), item(80, 40, False, 2)])
    assert "pc0_dufo" not in mixed


def test_scene_reader_yields_the_flags(golden_dir):
    """the committed av2_mini files have no DUFO flags; any per-point 0 / 1 dataset stands in: dynamic_key='flow_is_valid'"""
    from deflow_amd.data import HDF5Dataset, collate_fn_pad
    d = os.path.join(golden_dir, "av2_mini")
    sub = [os.path.join(d, s) for s in sorted(os.listdir(d)) if os.path.exists(os.path.join(d, s, "index_total.pkl"))]
    root = d if os.path.exists(os.path.join(d, "index_total.pkl")) else sub[0]
    ds = HDF5Dataset(root, dynamic_key="flow_is_valid")
    plain = HDF5Dataset(root)
    assert plain.dynamic_key == "dufo_label"
    seen = 0
    for i in range(min(len(ds), 3)):
        it, pl = ds[i], plain[i]
        assert "dufo0" not in pl and "dufo1" not in pl and set(it) - set(pl) <= {"dufo0", "dufo1"}
        if "dufo0" not in it:
            continue                                            # a pair whose second sweep is unlabelled
        seen += 1
        assert it["dufo0"].dtype == torch.bool and it["dufo0"].shape == (it["pc0"].shape[0],) and it["dufo1"].shape == (it["pc1"].shape[0],)
        assert torch.equal(it["dufo0"], it["flow_is_valid"].reshape(-1) != 0)
    assert seen > 0
    items = [ds[i] for i in range(min(len(ds), 2))]
    if all("dufo0" in it for it in items):
        res = collate_fn_pad(items)
        assert res["pc0_dufo"].shape == res["pc0"].shape[:2]
        assert int(res["pc0_dufo"].sum()) == sum(int((it["dufo0"] & ~it["gm0"]).sum()) for it in items)
    assert "pc0_dufo" not in collate_fn_pad([plain[i] for i in range(min(len(plain), 2))])
