"""GPU: the ground segmenter (csrc/ground.hip, deflow_amd/ground.py) against the naive integer restatement in tests/helpers/ground_ref.py.
Cell minima, height map, observed map and mask are integers after one fp32 quantisation that the helper restates operation by operation:
every comparison is exact equality (torch.equal); a second segmenter fed the same input must be bit-identical."""
import json
import os
import pickle
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ground_ref as GR  # noqa: E402
from test_ground_cpu import quality, synthetic_scene  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], grid_feature_size=[64, 64])   # tests/test_gpu_cluster.py's


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def check(name, dev, pts, count, **kw):
    """segment points [B,N,3] on the GPU (twice, with two segmenters) and in the helper: cell minima, height, observed and mask are equal"""
    from deflow_amd.ground import GroundSegmenter
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    B, N, _ = pts.shape
    want = GR.segment(pts, count, **kw)
    dp, dc = torch.from_numpy(pts).to(dev), torch.tensor(list(count), dtype=torch.int32, device=dev)
    segs = [GroundSegmenter(B, device=dev, **kw) for _ in range(2)]
    masks = [s.segment(dp, dc) for s in segs]
    a, b = segs
    Gx, Gy = GR.params(**kw)["dims"]
    assert masks[0].dtype == torch.bool and tuple(masks[0].shape) == (B, N)
    assert a.cell_min.dtype == torch.int32 and a.height.dtype == torch.int32 and a.observed.dtype == torch.uint8
    assert tuple(a.cell_min.shape) == tuple(a.height.shape) == tuple(a.observed.shape) == (B, Gy, Gx)
    print(f"[ground] {name}: {int((want['cell_min'] != GR.EMPTY).sum())} cells with rows, {int(want['observed'].sum())} observed, "
          f"{int(want['mask'].sum())} of {int(sum(count))} rows ground")
    assert torch.equal(a.cell_min.cpu().long(), torch.from_numpy(want["cell_min"])), f"{name}: the cell minima differ"
    assert torch.equal(a.height.cpu().long(), torch.from_numpy(want["height"])), f"{name}: the height map differs"
    assert torch.equal(a.observed.cpu(), torch.from_numpy(want["observed"])), f"{name}: the observed map differs"
    assert torch.equal(masks[0].cpu(), torch.from_numpy(want["mask"]) != 0), f"{name}: {int((masks[0].cpu() != (torch.from_numpy(want['mask']) != 0)).sum())} mask rows differ"
    for x, y in ((a.cell_min, b.cell_min), (a.height, b.height), (a.observed, b.observed), (masks[0], masks[1])):
        assert torch.equal(x, y), f"{name}: a second segmenter differs"
    hm = a.height_m()
    assert hm.dtype == torch.float32 and torch.equal(hm, a.height.float() * a.z_unit + a.z_min)
    return want, a, masks[0]


# ---- (d) corners -------------------------------------------------------------------------------------------------------------------------
# 16 x 12 cells of 0.5 m from (-4, -3): xy_min plus whole cells is exactly representable and k = 2, so those rows lie EXACTLY on cell edges.
# H = 300 levels of 0.01 from z_min = -1; seed_z = 0 is level 100.  Levels are hit in their middle (level L <- z_min + (L + 0.5) * z_unit).
CORNER = dict(xy_min=(-4.0, -3.0), cell=0.5, dims=(16, 12), z_min=-1.0, z_unit=0.01, z_levels=300, seed_z=0.0)
LEVEL = lambda L: -1.0 + (L + 0.5) * 0.01
CENTRE = (0.25, 0.25)                                                  # cell (8, 6)


def corner_case():
    g = np.random.default_rng(21)
    lo, hi = np.array([-4.0, -3.0]), np.array([4.0, 3.0])

    def cloud(n):                                                      # rows in and beyond every face, heights around the seed
        xy = g.uniform(lo - 1.0, hi + 1.0, (n, 2))
        z = 0.02 * (xy[:, 0] + xy[:, 1]) + g.normal(0.0, 0.06, n) + (g.random(n) < 0.25) * g.uniform(0.0, 1.5, n)
        return np.concatenate([xy, z[:, None]], 1)

    edges = np.stack(np.meshgrid(-4.0 + 0.5 * np.arange(17), -3.0 + 0.5 * np.arange(13), indexing="ij"), -1).reshape(-1, 2)   # every cell
    edges = np.concatenate([edges, g.normal(0.0, 0.05, (len(edges), 1))], 1)                # corner, the grid's four faces included
    zface = np.array([[0.3, 0.3, -1.0], [1.3, 0.3, 2.0], [0.8, -0.7, 1.995], [0.8, 0.7, -1.0000001], [-0.7, 0.3, np.nextafter(np.float32(2.0), np.float32(0))]])
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1e12, 0.5, 0.0], [0.5, -1e12, 0.0], [0.5, 0.5, 1e12], [3e38, 3e38, 3e38],
                    [0.5, 0.5, -3e38]])
    general = np.concatenate([cloud(500), edges, zface, bad])
    # the inclusive bounds, seen from the centre origin (cell (8, 6)): the origin cell and its four neighbours at the seed's level 100,
    # the cells two away at +RISE (+x), +RISE + 1 (-x), -DROP (+y), -DROP - 1 (-y)
    cx, cy = lambda c: -4.0 + 0.5 * c + 0.25, lambda c: -3.0 + 0.5 * c + 0.25
    steps = [[cx(8), cy(6), LEVEL(100)], [cx(9), cy(6), LEVEL(100)], [cx(7), cy(6), LEVEL(100)], [cx(8), cy(7), LEVEL(100)],
             [cx(8), cy(5), LEVEL(100)], [cx(10), cy(6), LEVEL(110)], [cx(6), cy(6), LEVEL(111)], [cx(8), cy(8), LEVEL(85)],
             [cx(8), cy(4), LEVEL(84)], [cx(10), cy(6), LEVEL(125)], [cx(10), cy(6), LEVEL(126)], [cx(6), cy(6), LEVEL(115)],
             [cx(6), cy(6), LEVEL(116)]]
    shared = np.concatenate([np.full((64, 1), cx(2)) + g.uniform(-0.2, 0.2, (64, 1)), np.full((64, 1), cy(9)) + g.uniform(-0.2, 0.2, (64, 1)),
                             g.uniform(-0.5, 1.5, (64, 1))], 1)        # 64 rows, one wave's worth, in one cell
    special = np.concatenate([np.array(steps), shared])
    N = len(general) + 40
    pts = np.full((4, N, 3), np.nan, dtype=np.float32)
    pts[0] = np.concatenate([general, cloud(40)]).astype(np.float32)
    pts[1] = pts[0]
    pts[2] = cloud(N).astype(np.float32)
    pts[3, : len(special)] = special.astype(np.float32)
    pts[3, len(special):] = cloud(N - len(special)).astype(np.float32)                      # rows past count: they must not be seen
    return pts, [N, N - 40, 0, len(special)], len(steps)


@pytest.mark.parametrize("origin", [CENTRE, (-3.9, 2.9), (1e6, -1e6)], ids=["centre", "corner", "outside"])
@pytest.mark.parametrize("miss_cap,widen", [(8, 0.03), (0, 0.03), (8, 0.0)])
def test_corners(dev, origin, miss_cap, widen):
    pts, count, n_steps = corner_case()
    kw = dict(CORNER, origin=origin, miss_cap=miss_cap, widen=widen)
    want, seg, mask = check(f"corners origin={origin} miss_cap={miss_cap} widen={widen}", dev, pts, count, **kw)
    p = GR.params(**kw)
    assert GR.origin_cell(p)[:2] == {CENTRE: (8, 6), (-3.9, 2.9): (0, 11), (1e6, -1e6): (15, 0)}[origin]
    assert (want["height"][2] == 100).all() and not want["observed"][2].any() and (want["cell_min"][2] == GR.EMPTY).all()   # count = 0
    assert not want["mask"][2].any() and not want["mask"][1][count[1]:].any() and want["mask"][0][count[1]:].any()
    assert (want["cell_min"][0] != GR.EMPTY).all() and want["cell_min"][0].min() == 0      # every cell has its corner row; a row at z_min
    assert (want["cell_min"][3] != GR.EMPTY).sum() == 10                                    # the rows past count stayed unseen
    assert want["cell_min"][3][9, 2] != GR.EMPTY and GR.rows(pts[3, n_steps:n_steps + 64], 64, p)[0].all()   # 64 rows share cell (2, 9)
    if origin == CENTRE:                                               # the inclusive bounds: +10 yes, +11 no, -15 yes, -16 no
        assert want["cell_min"][3][6, 10] == 110 and want["cell_min"][3][6, 6] == 111 and want["cell_min"][3][8, 8] == 85
        assert [int(want["observed"][3][y, x]) for x, y in ((10, 6), (6, 6), (8, 8), (8, 4))] == [1, 0, 1, 0]
        assert [int(want["height"][3][y, x]) for x, y in ((10, 6), (6, 6), (8, 8), (8, 4))] == [110, 100, 85, 100]
        # TOL = 15, inclusive, on the GPU's mask: 110 + 15 is ground, 110 + 16 is not; 100 + 15 is, 100 + 16 is not
        assert mask[3, n_steps - 4: n_steps].cpu().tolist() == [True, False, True, False]


def test_argument_errors(dev):
    from deflow_amd.ground import GroundSegmenter
    seg = GroundSegmenter(1, device=dev, **CORNER)
    p, c = torch.zeros(1, 8, 3, device=dev), torch.full((1,), 8, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError, match="points"):
        seg.segment(p.cpu(), c)
    with pytest.raises(TypeError, match="count"):
        seg.segment(p, c.cpu())
    with pytest.raises(ValueError, match="count"):
        seg.segment(p, c.long())
    with pytest.raises(ValueError, match="points"):
        seg.segment(p.double(), c)
    with pytest.raises(ValueError, match="points"):
        seg.segment(p.repeat(2, 1, 1), c)
    with pytest.raises(ValueError, match="points"):
        seg.segment(p[:, :0], c)
    assert seg.segment(p, c).tolist() == [[True] * 8]                  # z = 0 = the seed's height, at the origin cell


# ---- (e) the synthetic street scene at the default grid ----------------------------------------------------------------------------------
def test_street_scene_at_the_default_grid(dev):
    scenes = [synthetic_scene(0, 0.03), synthetic_scene(1, 0.03)]
    N = max(len(s[0]) for s in scenes)
    pts = np.full((2, N, 3), np.nan, dtype=np.float32)
    for b, s in enumerate(scenes):
        pts[b, : len(s[0])] = s[0]
    want, seg, mask = check("street scene", dev, pts, [len(s[0]) for s in scenes])
    assert tuple(seg.height.shape) == (2, 205, 205)
    for b, (p, above, _) in enumerate(scenes):
        recall, wrong = quality(mask[b, : len(p)].cpu().numpy(), p, above)
        print(f"[ground] GPU, seed {b}: recall {recall:.4f}, objects called ground {wrong:.4f}, rows {len(p)}")
        assert recall >= 0.99 and wrong <= 0.01


# ---- (f) a non-square, non-default grid --------------------------------------------------------------------------------------------------
def test_non_square_grid(dev):
    kw = dict(xy_min=(-38.4, -16.0), cell=0.8, dims=(96, 40), z_min=-4.0, z_unit=0.02, z_levels=400, origin=(3.0, -2.0), seed_z=-1.7)
    g = np.random.default_rng(33)
    N = 20000
    xy = g.uniform((-40.0, -17.0), (40.0, 17.0), (2, N, 2))
    z = -1.7 + 0.03 * xy[..., 0] - 0.02 * xy[..., 1] + g.normal(0.0, 0.05, (2, N)) + (g.random((2, N)) < 0.3) * g.uniform(0.0, 3.0, (2, N))
    pts = np.concatenate([xy, z[..., None]], -1).astype(np.float32)
    want, _, _ = check("96 x 40 grid", dev, pts, [N, 12345], **kw)
    assert 0 < want["observed"].sum() < 2 * 96 * 40 and 0.2 < want["mask"][0].mean() < 0.9


# ---- (g) scene files ---------------------------------------------------------------------------------------------------------------------
def test_scene_file_sidecar_and_training_step(dev, tmp_path, golden_dir):
    import deflow_amd
    from deflow_amd import ground
    from deflow_amd.data import HDF5Dataset, collate_fn_pad
    from deflow_amd.h5scene import H5File
    from deflow_amd.optim import Trainer
    src = os.path.join(golden_dir, "av2_mini", "train")
    for sid in ("scene_a", "scene_b"):
        shutil.copy(os.path.join(src, sid + ".h5"), tmp_path / (sid + ".h5"))    # never written under tests/golden
    with open(os.path.join(src, "index_total.pkl"), "rb") as f:
        index = [e for e in pickle.load(f) if e[0] in ("scene_a", "scene_b")]
    with open(tmp_path / "index_total.pkl", "wb") as f:
        pickle.dump(index, f)
    h5 = str(tmp_path / "scene_b.h5")
    with H5File(h5) as f:
        sweeps = sorted(f.keys(), key=int)
        lidars = {t: f[t]["lidar"].read() for t in sweeps}
    rep = {}
    got = ground.label_scene(h5, device=dev, report=rep)
    assert list(got) == sweeps and 0.0 < rep["observed_cell_fraction"] < 1.0
    for t in sweeps:
        want = GR.segment_sweep(lidars[t])
        assert got[t].dtype == np.uint8 and got[t].shape == (lidars[t].shape[0],) and np.array_equal(got[t], want), t
    # the command line: one sidecar per scene, the parameters under `meta`
    assert ground.main([f"data_dir={tmp_path}", "miss_cap=6"]) == 0
    for sid in ("scene_a", "scene_b"):
        back = ground.read_sidecar(str(tmp_path / (sid + ".ground.npz")))
        rows, flagged = sum(len(v) for v in back.values()), sum(int(v.sum()) for v in back.values())
        print(f"[ground] {sid}: {len(back)} sweeps, {rows} rows, {flagged} flagged with the default seed_z")
        assert flagged > 0                                             # the default seed_z flags rows in both scenes: no seed of their own needed
        with np.load(str(tmp_path / (sid + ".ground.npz"))) as z:
            meta = json.loads(str(z["meta"]))
        assert meta.pop("definition").startswith("DESIGN.md 6d")
        assert meta == ground.GroundSegmenter(1, device=dev, miss_cap=6).params() and meta["miss_cap"] == 6 and meta["seed_z"] == -0.33
    want6 = ground.label_scene(h5, device=dev, miss_cap=6)
    back = ground.read_sidecar(str(tmp_path / "scene_b.ground.npz"))
    assert list(back) == sweeps and all(np.array_equal(back[t], want6[t]) for t in sweeps)
    # reader -> collate -> one training step
    ds = HDF5Dataset(str(tmp_path), ground_source="sidecar")
    picks = [i for i, e in enumerate(ds.data_index) if e[0] == "scene_b"][1:40:11]
    items = [ds[i] for i in picks]
    for i, it in zip(picks, items):
        k = sweeps.index(str(it["timestamp"]))
        assert np.array_equal(it["gm0"].numpy(), back[sweeps[k]] != 0) and np.array_equal(it["gm1"].numpy(), back[sweeps[k + 1]] != 0)
        assert bool(it["gm0"].any()) and not bool(it["gm0"].all())
    host = collate_fn_pad(items)
    for b, it in enumerate(items):                                    # the batch's clouds lost exactly the flagged rows
        for key, gm in (("pc0", "gm0"), ("pc1", "gm1")):
            kept = it[key][~it[gm]].float()
            assert torch.equal(host[key][b, : kept.shape[0]], kept) and bool(torch.isnan(host[key][b, kept.shape[0]:]).all())
    batch = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in host.items()}
    torch.manual_seed(79)
    m = deflow_amd.DeFlow(**SMALL, num_iters=2).to(dev).train()
    loss = float(Trainer(m, lr=1e-3, loss_fn="deflowLoss").step(batch))
    print(f"[ground] deflowLoss step on the segmented scene: loss {loss}")
    assert np.isfinite(loss)
