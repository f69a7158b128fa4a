"""CPU: the ground segmenter's plumbing -- the integer helper (tests/helpers/ground_ref.py) on hand-computed known answers and on a
synthetic street scene (the quality of the definition itself), the new C-ABI entries' argument checks, the absence of a CPU fallback, the
command line's keys and the reader's ``ground_source`` / ``ground_sidecar``."""
import ctypes as C
import inspect
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ground_ref as GR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEHICLE_HEIGHT = 0.33                  # the vehicle frame above the road, the default seed_z negated


# ---- a synthetic street scene ------------------------------------------------------------------------------------------------------------
def synthetic_scene(seed, slope=0.03, n_road=60000, hide=False):
    """One sweep in the vehicle frame: -> (points fp32 [N,3], above float64 [N]: each row's height above the road surface under it,
    kind [N]: which element the row belongs to).
    The road is a plane tilted by up to `slope` per axis with a +-0.15 m undulation of ~60 m wavelength and 2 cm noise, seen at ranges of
    3 - 70 m (denser near the vehicle, as a spinning lidar's returns are); on it ~40 car-sized boxes whose rows start 0.25 m above the
    road (`hide` removes the road rows below them), ~30 pedestrian columns from the road up, a dozen 20 m walls from the road to 6 m, and 200 rows
    0.5 - 2 m below the road (multipath)."""
    g = np.random.default_rng(seed)
    sx, sy = slope * g.choice([-1.0, 1.0]) * g.uniform(0.6, 1.0), slope * g.choice([-1.0, 1.0]) * g.uniform(0.6, 1.0)
    px, py = g.uniform(0, 2 * np.pi, 2)
    surface = lambda x, y: -VEHICLE_HEIGHT + sx * x + sy * y + 0.15 * np.sin(x / 9.0 + px) * np.cos(y / 11.0 + py)

    def polar(n, lo, hi):
        r, a = g.uniform(lo, hi, n), g.uniform(0, 2 * np.pi, n)
        return r * np.cos(a), r * np.sin(a)

    def boxes(n, size, lo, hi):
        cx, cy = polar(n, lo, hi)
        return cx, cy, g.uniform(0, np.pi, n), size

    def inside(x, y, b, grow=0.0):
        cx, cy, yaw, (L, W) = b
        hit = np.zeros(x.shape, dtype=bool)
        for i in range(len(cx)):
            u = (x - cx[i]) * np.cos(yaw[i]) + (y - cy[i]) * np.sin(yaw[i])
            v = -(x - cx[i]) * np.sin(yaw[i]) + (y - cy[i]) * np.cos(yaw[i])
            hit |= (np.abs(u) <= L / 2 + grow) & (np.abs(v) <= W / 2 + grow)
        return hit

    def fill(b, per, zlo, zhi):
        cx, cy, yaw, (L, W) = b
        n = len(cx)
        u, v = g.uniform(-L / 2, L / 2, (n, per)), g.uniform(-W / 2, W / 2, (n, per))
        x = cx[:, None] + u * np.cos(yaw)[:, None] - v * np.sin(yaw)[:, None]
        y = cy[:, None] + u * np.sin(yaw)[:, None] + v * np.cos(yaw)[:, None]
        return x.ravel(), y.ravel(), g.uniform(zlo, zhi, n * per)

    cars = boxes(40, (4.5, 1.9), 6.0, 48.0)
    rx, ry = polar(n_road, 3.0, 70.0)
    if hide:                                                          # the harder variant DESIGN.md section 6d records: no road rows below a car
        keep = ~inside(rx, ry, cars)
        rx, ry = rx[keep], ry[keep]
    parts = [(rx, ry, g.normal(0.0, 0.02, rx.shape[0]))]
    parts.append(fill(cars, 150, 0.25, 1.6))
    parts.append(fill(boxes(30, (0.5, 0.5), 4.0, 40.0), 60, 0.0, 1.75))
    parts.append(fill(boxes(12, (20.0, 0.2), 12.0, 50.0), 600, 0.0, 6.0))
    ox, oy = polar(200, 3.0, 60.0)
    parts.append((ox, oy, -g.uniform(0.5, 2.0, 200)))
    x, y, above = (np.concatenate([p[i] for p in parts]) for i in range(3))
    kind = np.concatenate([np.full(p[0].shape[0], i) for i, p in enumerate(parts)])      # 0 road, 1 car, 2 pedestrian, 3 wall, 4 outlier
    order = g.permutation(x.shape[0])
    x, y, above, kind = x[order], y[order], above[order], kind[order]
    pts = np.stack([x, y, surface(x, y) + above], 1).astype(np.float32)
    return pts, above, kind


def quality(mask, pts, above, p=None):
    """-> (recall over the true ground rows, fraction of the object rows called ground), inside the grid"""
    p = GR.params() if p is None else p
    lo = np.array(p["xy_min"])
    hi = lo + np.array(p["dims"]) * p["cell"]
    inside = ((pts[:, :2] >= lo) & (pts[:, :2] < hi)).all(1)
    ground, obj = inside & (np.abs(above) < 0.10), inside & (above > 0.30)
    assert ground.sum() > 20000 and obj.sum() > 5000
    m = np.asarray(mask) != 0
    return m[ground].mean(), m[obj].mean()


# ---- the helper on hand-computed cases ---------------------------------------------------------------------------------------------------
SMALL = dict(xy_min=(0.0, 0.0), cell=1.0, dims=(6, 5), z_min=0.0, z_unit=0.01, z_levels=300, origin=(0.5, 2.5), seed_z=1.0)


def zmap(p, cells):
    z = np.full((p["dims"][1], p["dims"][0]), GR.EMPTY, dtype=np.int64)
    for (cx, cy), v in cells.items():
        z[cy, cx] = v
    return z


def test_quantisation_is_two_rounded_fp32_operations():
    p = GR.params()
    pts = np.array([[0.0, 0.0, -0.33], [-51.2, -51.2, -5.0], [51.29, 0, 0], [51.4, 0, 0], [0, 0, 4.995], [0, 0, 5.0], [0, 0, -5.01],
                    [np.nan, 0, 0], [0, np.inf, 0], [1e12, 0, 0], [0, 0, 3e38]], dtype=np.float32)
    ok, cx, cy, h = GR.rows(pts, len(pts), p)
    assert ok.tolist() == [True, True, True, False, True, False, False, False, False, False, False]
    assert (cx[0], cy[0], h[0]) == (102, 102, 467) and (cx[1], cy[1], h[1]) == (0, 0, 0) and cx[2] == 204 and h[4] == 999
    assert not GR.rows(pts, 0, p)[0].any() and GR.rows(pts, 2, p)[0].sum() == 2            # rows past count
    # a case where the fused form differs: the difference rounds before the product
    x, lo, k = np.float32(0.1), np.float32(-51.2), np.float32(2.0)
    assert GR.quant(x, lo, k) == np.float32(np.float32(x - lo) * k)
    assert GR.origin_cell(p) == (102, 102, 467) and GR.thresholds(p) == (10, 15, 3, 15)
    assert GR.origin_cell(GR.params(origin=(1e9, -1e9))) == (204, 0, 467)                  # clamped into the grid


def test_chain_path_and_inclusive_bounds():
    p = GR.params(**SMALL)                                             # origin cell (0, 2), seed 100
    assert GR.origin_cell(p) == (0, 2, 100)
    z = zmap(p, {(0, 2): 100})
    assert GR.chain(z, 4, 0, p)[2] == [(0, 2), (1, 1), (2, 0), (3, 0), (4, 0)]             # diagonal first, then straight
    assert GR.chain(z, 2, 4, p)[2] == [(0, 2), (1, 3), (2, 4)] and GR.chain(z, 0, 2, p)[2] == [(0, 2)]
    # RISE = 10, DROP = 15, inclusive; after an accepted cell miss = 0, so no widening
    for step, want in ((10, True), (11, False), (-15, True), (-16, False)):
        z = zmap(p, {(0, 2): 100, (1, 2): 100 + step})
        g, obs, _ = GR.chain(z, 1, 2, p)
        assert (g, obs) == ((100 + step, 1) if want else (100, 0)), step
    # widening: WIDEN = 3 per missed cell; two empty cells, then a cell 16 above: 10 + 2 * 3 = 16 is accepted, 17 is not
    for step, want in ((16, True), (17, False)):
        z = zmap(p, {(0, 2): 100, (3, 2): 100 + step})
        assert GR.chain(z, 3, 2, p)[:2] == ((100 + step, 1) if want else (100, 0))
    # the seed starts with miss = miss_cap: 10 + 8 * 3 = 34 above the seed is accepted at the origin cell, 35 is not
    assert GR.chain(zmap(p, {(0, 2): 134}), 0, 2, p)[:2] == (134, 1) and GR.chain(zmap(p, {(0, 2): 135}), 0, 2, p)[:2] == (100, 0)
    # miss_cap = 0: never any widening
    p0 = GR.params(**SMALL, miss_cap=0)
    assert GR.chain(zmap(p0, {(0, 2): 111}), 0, 2, p0)[:2] == (100, 0) and GR.chain(zmap(p0, {(0, 2): 110}), 0, 2, p0)[:2] == (110, 1)
    # an empty map: uniformly the seed, nothing observed
    hgt, obs = GR.height_map(zmap(p, {}), p)
    assert (hgt == 100).all() and not obs.any()


def test_vector_form_equals_the_chain_form():
    g = np.random.default_rng(9)
    for kw in (dict(dims=(16, 12), origin=(4.2, 3.3)), dict(dims=(9, 14), origin=(-50.0, 99.0)), dict(dims=(11, 7), origin=(5.5, 3.5), miss_cap=0),
               dict(dims=(13, 13), origin=(12.5, 0.5), widen=0.0, miss_cap=3)):
        p = GR.params(**{**SMALL, **kw})
        Gx, Gy = p["dims"]
        z = g.integers(80, 130, (Gy, Gx)).astype(np.int64)
        z = np.where(g.random((Gy, Gx)) < 0.35, GR.EMPTY, z)
        a, b = GR.height_map_cells(z, p), GR.height_map(z, p)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert 0 < b[1].sum() < Gx * Gy


def test_mask_on_a_hand_made_cloud():
    p = GR.params(**SMALL)
    # heights in the middle of a level, so that the level does not hang on the last bit of the product
    pts = np.array([[0.5, 2.5, 1.005], [0.5, 2.5, 1.155], [0.5, 2.5, 1.165], [0.5, 2.5, 0.205],   # the origin cell: min 20 -> not accepted
                    [1.5, 2.5, 1.055], [1.5, 2.5, 1.205], [1.5, 2.5, 1.215], [1.5, 2.5, 2.995], [1.5, 2.5, 3.0],
                    [2.5, 2.5, 1.505], [2.5, 2.5, np.nan]], dtype=np.float32)
    out = GR.segment(pts[None], [len(pts)], **SMALL)
    assert out["cell_min"][0, 2, :3].tolist() == [20, 105, 150] and out["height"][0, 2, :3].tolist() == [100, 105, 105]
    assert out["observed"][0, 2, :3].tolist() == [0, 1, 0]
    # TOL = 15 above the cell's height, inclusive; rows below the ground are ground; uz >= H and NaN rows are not
    assert out["mask"][0].tolist() == [1, 1, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert GR.segment(pts[None], [4], **SMALL)["mask"][0].tolist() == [1, 1, 0, 1] + [0] * 7


# ---- (a) the quality of the definition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,slope", [(0, 0.03), (1, 0.03), (2, 0.0)])
def test_definition_separates_ground_from_objects(seed, slope):
    pts, above, _ = synthetic_scene(seed, slope)
    mask = GR.segment_sweep(pts)
    recall, wrong = quality(mask, pts, above)
    print(f"[ground] helper, seed {seed} slope {slope}: recall {recall:.4f}, objects called ground {wrong:.4f}, rows {len(pts)}")
    assert recall >= 0.99 and wrong <= 0.01


# ---- (b) the library's entries and the Python layer --------------------------------------------------------------------------------------
def test_ground_entries_reject_bad_arguments_without_launching():
    """NULL buffers, Gx = 0 / 4097, H = 0, miss_cap = 65, B = 0: negative DF_E_* codes, no launch (no GPU here)"""
    from deflow_amd import build
    from deflow_amd._lib import load
    build.build()
    lib = load()
    P, F = C.c_void_p, C.c_float
    ok = P(0x1000)
    SHAPE, ARG = -1, -3
    cells = lambda pts=ok, cnt=ok, B=1, N=100, xmin=-51.2, kxy=2.0, kz=100.0, G=(205, 205), H=1000, z=ok: lib.df_ground_cells(
        pts, cnt, B, N, F(xmin), F(-51.2), F(kxy), F(-5.0), F(kz), G[0], G[1], H, z, P(0))
    assert cells(pts=P(0)) == ARG and cells(cnt=P(0)) == ARG and cells(z=P(0)) == ARG
    assert cells(G=(0, 205)) == SHAPE and cells(G=(4097, 205)) == SHAPE and cells(G=(205, 0)) == SHAPE and cells(G=(205, 4097)) == SHAPE
    assert cells(B=0) == SHAPE and cells(B=65536) == SHAPE and cells(N=0) == SHAPE and cells(B=40000, N=80000) == SHAPE
    assert cells(H=0) == ARG and cells(H=(1 << 20) + 1) == ARG and cells(xmin=float("nan")) == ARG and cells(kxy=0.0) == ARG
    assert cells(kz=float("inf")) == ARG and cells(kz=-1.0) == ARG
    height = lambda z=ok, B=1, G=(205, 205), o=(102, 102), seed=467, rise=10, drop=15, widen=3, cap=8, h=ok, ob=ok: lib.df_ground_height(
        z, B, G[0], G[1], o[0], o[1], seed, rise, drop, widen, cap, h, ob, P(0))
    assert height(z=P(0)) == ARG and height(h=P(0)) == ARG and height(ob=P(0)) == ARG
    assert height(G=(0, 205)) == SHAPE and height(G=(4097, 205)) == SHAPE and height(B=0) == SHAPE and height(B=65536) == SHAPE
    assert height(cap=65) == ARG and height(cap=-1) == ARG and height(rise=-1) == ARG and height(drop=-1) == ARG and height(widen=-1) == ARG
    assert height(o=(205, 0)) == ARG and height(o=(0, -1)) == ARG
    mask = lambda pts=ok, cnt=ok, B=1, N=100, kxy=2.0, G=(205, 205), H=1000, h=ok, tol=15, m=ok: lib.df_ground_mask(
        pts, cnt, B, N, F(-51.2), F(-51.2), F(kxy), F(-5.0), F(100.0), G[0], G[1], H, h, tol, m, P(0))
    assert mask(pts=P(0)) == ARG and mask(cnt=P(0)) == ARG and mask(h=P(0)) == ARG and mask(m=P(0)) == ARG
    assert mask(G=(0, 205)) == SHAPE and mask(G=(4097, 205)) == SHAPE and mask(B=0) == SHAPE and mask(N=-1) == SHAPE
    assert mask(H=0) == ARG and mask(tol=-1) == ARG and mask(kxy=float("nan")) == ARG


def test_ground_api_has_no_cpu_fallback():
    import deflow_amd
    from deflow_amd import ground
    assert deflow_amd.GroundSegmenter is ground.GroundSegmenter
    with pytest.raises(TypeError, match="CUDA"):
        ground.GroundSegmenter(1, device="cpu")
    cls = inspect.getsource(ground.GroundSegmenter)
    for word in (".cpu()", ".item()", ".tolist()", ".numpy()", "ground_ref"):                # no read-back, no other implementation
        assert word not in cls, word
    for bad in (dict(dims=(0, 4)), dict(dims=(4097, 4)), dict(z_levels=0), dict(z_levels=(1 << 20) + 1), dict(miss_cap=65), dict(cell=0.0),
                dict(z_unit=-1.0), dict(rise=-0.1), dict(tol=float("nan")), dict(xy_min=(0.0, float("nan"))), dict(origin=(float("inf"), 0.0)),
                dict(batch=0), dict(seed_z=float("nan")), dict(xy_min=(0.0, 0.0, 0.0))):
        kw = dict(batch=1, device="cuda")
        kw.update(bad)
        with pytest.raises(ValueError):
            ground.GroundSegmenter(**kw)
    assert {k: (list(v) if isinstance(v, tuple) else v) for k, v in GR.DEFAULTS.items()} == \
        {k: (list(v) if isinstance(v, tuple) else v) for k, v in ground.DEFAULTS.items()}


def test_command_line_keys():
    from deflow_amd.ground import parse_args
    cfg = parse_args(["data_dir=/d", "scenes=a,b", "overwrite=true", "cell=0.8", "dims=96,40", "xy_min=-38.4,-16", "seed_z=-1.7", "miss_cap=4",
                      "z_levels=500", "origin=1,2"])
    assert cfg["data_dir"] == "/d" and cfg["scenes"] == ["a", "b"] and cfg["overwrite"] is True and cfg["cell"] == 0.8
    assert cfg["dims"] == [96, 40] and cfg["xy_min"] == [-38.4, -16.0] and cfg["seed_z"] == -1.7 and cfg["miss_cap"] == 4
    assert cfg["z_levels"] == 500 and cfg["origin"] == [1.0, 2.0] and cfg["tol"] == 0.15
    cfg = parse_args(["data_dir=/d"])
    assert cfg["scenes"] is None and cfg["overwrite"] is False and {k: cfg[k] for k in ("cell", "seed_z", "rise", "drop", "widen")} == \
        {"cell": 0.5, "seed_z": -0.33, "rise": 0.10, "drop": 0.15, "widen": 0.03}
    for bad in (["cell=0.2"], ["data_dir=/d", "cel=0.2"], ["data_dir=/d", "overwrite=maybe"], ["data_dir=/d", "miss_cap=x"],
                ["data_dir=/d", "dims=4"], ["data_dir"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


# ---- (c) the reader --------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def train_dir(tmp_path, golden_dir):
    """a copy of the committed training directory: nothing is ever written under tests/golden"""
    dst = tmp_path / "train"
    shutil.copytree(os.path.join(golden_dir, "av2_mini", "train"), dst)
    return str(dst)


def same_items(a, b):
    return set(a) == set(b) and all((torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype) if isinstance(a[k], torch.Tensor) else a[k] == b[k]
                                    for k in a)


READER = dict(cell=1.6, dims=(64, 64))                                # the default extent in coarser cells: the reader tests only need masks


def helper_masks(ds, scene_id):
    """the helper's masks of every sweep of a scene"""
    f = ds._file(scene_id)
    return {ts: GR.segment_sweep(f[ts]["lidar"].read(), **READER) for ts in f.sweeps}


def scenes_of(ds):
    return sorted({e[0] for e in ds.data_index})


def test_sidecar_masks_reach_the_items_and_the_collate(train_dir):
    from deflow_amd.data import HDF5Dataset, collate_fn_pad
    from deflow_amd.ground import read_sidecar, write_sidecar
    plain = HDF5Dataset(train_dir)
    masks = {}
    g = np.random.default_rng(4)
    for sid in scenes_of(plain):
        masks[sid] = helper_masks(plain, sid)
        for ts in list(masks[sid])[::3]:                               # the committed clouds are tiny: make sure every pattern occurs
            masks[sid][ts] = (g.random(masks[sid][ts].shape[0]) < 0.4).astype(np.uint8)
        write_sidecar(os.path.join(train_dir, sid + ".ground.npz"), masks[sid], GR.params(**READER))
        back = read_sidecar(os.path.join(train_dir, sid + ".ground.npz"))
        assert set(back) == set(masks[sid]) and all(np.array_equal(back[k], masks[sid][k]) and back[k].dtype == np.uint8 for k in back)
    ds = HDF5Dataset(train_dir, ground_source="sidecar")
    assert ds.ground_sidecar == ".ground.npz" and plain.ground_source == "auto"
    picks = list(range(0, len(ds), 7)) + [len(ds) - 1]
    items = [ds[i] for i in picks]
    differs = 0
    for i, it in zip(picks, items):
        sid = it["scene_id"]
        sweeps = ds._file(sid).sweeps
        k = sweeps.index(str(it["timestamp"]))
        for key, ts, pc in (("gm0", sweeps[k], "pc0"), ("gm1", sweeps[k + 1], "pc1")):
            assert it[key].dtype == torch.bool and it[key].shape == (it[pc].shape[0],)
            assert torch.equal(it[key], torch.from_numpy(masks[sid][ts]) != 0)
        ref = plain[i]
        assert set(it) == set(ref) and all(same_items({k: it[k]}, {k: ref[k]}) for k in it if k not in ("gm0", "gm1"))
        differs += int((it["gm0"] != ref["gm0"]).sum())
    assert differs > 0                                                # the datasets were ignored
    res = collate_fn_pad(items)
    for b, it in enumerate(items):                                    # the batch's clouds lost exactly the flagged rows
        for key, gm in (("pc0", "gm0"), ("pc1", "gm1")):
            kept = it[key][~it[gm]].float()
            assert torch.equal(res[key][b, : kept.shape[0]], kept) and bool(torch.isnan(res[key][b, kept.shape[0]:]).all())
    assert ds._sidecar(scenes_of(ds)[0], ground=True) is ds._sidecar(scenes_of(ds)[0], ground=True)     # cached per scene


def test_sidecar_length_mismatch_and_missing_sidecar_raise(train_dir):
    from deflow_amd.data import HDF5Dataset
    from deflow_amd.ground import write_sidecar
    plain = HDF5Dataset(train_dir)
    sid = plain.data_index[0][0]
    with pytest.raises(KeyError, match="python -m deflow_amd.ground data_dir="):
        HDF5Dataset(train_dir, ground_source="sidecar")[0]           # no sidecar at all
    masks = helper_masks(plain, sid)
    sweeps = plain._file(sid).sweeps
    masks[sweeps[3]] = masks[sweeps[3]][:-1]
    del masks[sweeps[6]]
    write_sidecar(os.path.join(train_dir, sid + ".ground.npz"), masks, {})
    ds = HDF5Dataset(train_dir, ground_source="sidecar")
    first = [i for i, e in enumerate(ds.data_index) if e[0] == sid and str(e[1]) == sweeps[0]][0]
    at = lambda k: [i for i, e in enumerate(ds.data_index) if e[0] == sid and str(e[1]) == sweeps[k]][0]
    assert "gm0" in ds[first]
    with pytest.raises(ValueError, match="ground flags for sweep"):
        ds[at(3)]
    with pytest.raises(ValueError, match="ground flags for sweep"):
        ds[at(2)]                                                     # as the pair's second sweep
    with pytest.raises(KeyError, match="has no entry for sweep"):
        ds[at(6)]
    with pytest.raises(ValueError, match="ground_source"):
        HDF5Dataset(train_dir, ground_source="npz")


def test_auto_and_file_yield_todays_items(golden_dir, train_dir):
    """the unmodified directory: every group carries `ground_mask`, so "auto" and "file" equal the reader called without the arguments --
    also when a sidecar lies beside the files ("auto": the group's own dataset wins)"""
    from deflow_amd.data import HDF5Dataset
    from deflow_amd.ground import write_sidecar
    src = os.path.join(golden_dir, "av2_mini", "train")
    base = HDF5Dataset(src)
    auto, file_ = HDF5Dataset(src, ground_source="auto"), HDF5Dataset(src, ground_source="file", ground_sidecar=".ground.npz")
    for i in range(len(base)):
        a = base[i]
        assert same_items(a, auto[i]) and same_items(a, file_[i])
    plain = HDF5Dataset(train_dir)
    for sid in scenes_of(plain):
        f = plain._file(sid)
        write_sidecar(os.path.join(train_dir, sid + ".ground.npz"), {ts: np.ones(f[ts]["lidar"].read().shape[0], np.uint8) for ts in f.sweeps}, {})
    beside = HDF5Dataset(train_dir)
    for i in range(0, len(base), 5):
        assert same_items(base[i], beside[i])
