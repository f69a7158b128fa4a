"""CPU: the void map's plumbing -- the integer helper (tests/helpers/voidmap_ref.py) on hand-computed known answers, the new C-ABI entries'
argument checks, the absence of a CPU fallback, the sidecar reader, scene_grid and the command line.  Hand-made cases use gmin = 0 and
voxel = 1, so a coordinate p quantises to floor(256 p) exactly."""
import ctypes as C
import inspect
import os
import pickle
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import voidmap_ref as VR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G0 = (0.0, 0.0, 0.0)
DIMS = (32, 6, 5)


def set_voxels(bits):
    """the set voxels of a bool [Gz, Gy, Gx] as sorted (x, y, z)"""
    z, y, x = np.nonzero(bits)
    return sorted(zip(x.tolist(), y.tolist(), z.tolist()))


def one_ray(a, e, **kw):
    return VR.sweep_bits(np.array([e], dtype=np.float32), 1, np.array(a, dtype=np.float32), G0, 1.0, DIMS, **kw)


# ---- the helper on hand-computed cases ---------------------------------------------------------------------------------------------------
def test_quantise_is_two_rounded_fp32_operations():
    q, ok = VR.quantise(np.array([[0.5, 1.0, -0.25], [np.nan, 0, 0], [0, np.inf, 0], [1e12, 0, 0], [4194303.5, 0, 0], [4194304.0, 0, 0]],
                                 dtype=np.float32), G0, np.float32(256))
    assert q[0].tolist() == [128, 256, -64] and ok.tolist() == [True, False, False, False, True, False]      # |u| < 2^30 exactly
    assert (q[0] >> 8).tolist() == [0, 1, -1]                                                                 # arithmetic shift: floor
    # a case where the fused form differs: p - g rounds before the product
    p, g, k = np.float32(0.1), np.float32(-51.2), VR.k_of(0.1)
    want = int(np.floor(np.float32(np.float32(p - g) * k)))
    assert VR.quantise(np.array([[p, p, p]]), (g, g, g), k)[0][0, 0] == want
    assert VR.k_of(0.1) == np.float32(2560.0) and VR.ray_limit(80.0, 0.1) == 204800


def test_axis_aligned_ray_and_the_margin():
    for hm, last in ((0, 4), (1, 3), (2, 2)):
        F, O, over = one_ray((0.5, 0.5, 0.5), (5.5, 0.5, 0.5), hit_margin=hm)
        assert set_voxels(F) == [(x, 0, 0) for x in range(last + 1)] and set_voxels(O) == [(5, 0, 0)] and over == 0
    v, s, cut, e = VR.walk((128, 128, 128), (1408, 128, 128), 204800, 2)
    assert v == [(x, 0, 0) for x in range(6)] and s == [True, True, True, False, False, False] and not cut and e == (5, 0, 0)


def test_corner_diagonal_steps_x_then_y_then_z():
    v, s, cut, e = VR.walk((256, 256, 256), (896, 896, 896), 204800, 0)
    assert v == [(1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)]
    assert s == [True] * 6 + [False] and e == (3, 3, 3)
    F, O, _ = one_ray((1, 1, 1), (3.5, 3.5, 3.5), hit_margin=0)
    assert set_voxels(F) == sorted(v[:-1]) and set_voxels(O) == [(3, 3, 3)]


def test_negative_direction_start_on_a_boundary():
    # x = 2.0 exactly, going down: num_x = 0, the first step leaves voxel 2 at once
    v, s, _, e = VR.walk((512, 128, 128), (128, 128, 128), 204800, 0)
    assert v == [(2, 0, 0), (1, 0, 0), (0, 0, 0)] and s == [True, True, False]
    v, _, _, e = VR.walk((512, 128, 128), (128, 384, 128), 204800, 0)           # x at t = 0, y at 1/2, x at 2/3
    assert v == [(2, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)] and e == (0, 1, 0)
    # the positive direction from the same boundary stays a whole voxel in voxel 2
    v, _, _, _ = VR.walk((512, 128, 128), (896, 128, 128), 204800, 0)
    assert v == [(2, 0, 0), (3, 0, 0)]
    F, O, _ = one_ray((2.0, 0.5, 0.5), (0.5, 1.5, 0.5), hit_margin=0)
    assert set_voxels(F) == [(1, 0, 0), (1, 1, 0), (2, 0, 0)] and set_voxels(O) == [(0, 1, 0)]


def test_zero_length_ray():
    v, s, cut, e = VR.walk((300, 300, 300), (300, 300, 300), 204800, 0)
    assert v == [(1, 1, 1)] and s == [False] and not cut and e == (1, 1, 1)
    F, O, _ = one_ray((1.2, 1.2, 1.2), (1.2, 1.2, 1.2), hit_margin=0)
    assert not F.any() and set_voxels(O) == [(1, 1, 1)]


def test_truncation_is_a_chebyshev_cut_in_integers():
    R = VR.ray_limit(2.0, 1.0)
    assert R == 512
    v, s, cut, e = VR.walk((128, 128, 128), (2688, 1408, 128), R, 2)             # d = (2560, 1280, 0) -> (512, 256, 0)
    assert cut and e == (2, 1, 0) and v == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0)] and s == [True] * 4     # the end voxel too
    v, s, cut, e = VR.walk((1408, 0, 128), (-1152, -1, 128), R, 2)               # floor_div(-1 * 512, 2560) = -1: y ends in voxel -1
    assert cut and e == (3, -1, 0) and v[0] == (5, 0, 0) and v[-1] == (3, -1, 0) and len(v) == 4
    v, s, cut, e = VR.walk((128, 128, 128), (640, 128, 128), R, 2)               # m == R: not truncated
    assert not cut and e == (2, 0, 0) and s == [False] * 3
    F, O, _ = one_ray((0.5, 0.5, 0.5), (10.5, 5.5, 0.5), hit_margin=2, max_range=2.0)
    assert set_voxels(F) == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 1, 0)] and set_voxels(O) == [(10, 5, 0)]   # O: the ORIGINAL endpoint


def test_vector_walk_equals_the_scalar_walk():
    g = np.random.default_rng(5)
    pts = g.uniform(-3, 35, (300, 3)).astype(np.float32)
    pts[:, 1:] = g.uniform(-2, 8, (300, 2))
    pts[::7, 0] = np.round(pts[::7, 0])                                          # boundaries
    pts[::11, 1] = pts[::11, 2] = 2.5                                            # zero components
    origin = np.array([7.0, 2.5, 2.5], dtype=np.float32)
    for hm, mr in ((0, 80.0), (2, 6.0)):
        F, O, over = VR.sweep_bits(pts, 300, origin, G0, 1.0, DIMS, hit_margin=hm, max_range=mr)
        want = np.zeros_like(F)
        A, _ = VR.quantise(origin, G0, np.float32(256))
        E, _ = VR.quantise(pts, G0, np.float32(256))
        for row in E:
            v, s, _, _ = VR.walk(A, row, VR.ray_limit(mr, 1.0), hm)
            for (x, y, z), on in zip(v, s):
                if on and 0 <= x < DIMS[0] and 0 <= y < DIMS[1] and 0 <= z < DIMS[2]:
                    want[z, y, x] = True
        assert over == 0 and np.array_equal(F, want) and F.sum() > 50


def test_erosion_and_packing():
    b = np.zeros((7, 7, 32), dtype=bool)
    b[2:5, 2:5, 10:13] = True
    assert set_voxels(VR.erode(b, 1)) == [(11, 3, 3)] and not VR.erode(b, 2).any() and np.array_equal(VR.erode(b, 0), b)
    face = np.zeros((7, 7, 32), dtype=bool)
    face[0:2, 2:5, 10:13] = True                                                 # a 3^3 block centred ON the z = 0 face: one layer is
    assert not VR.erode(face, 1).any()                                           # outside the grid, and outside counts as not free
    face = np.zeros((7, 7, 32), dtype=bool)
    face[2:5, 2:5, 0:2] = True                                                   # centred on the x = 0 face
    assert not VR.erode(face, 1).any()
    full1 = VR.erode(np.ones((7, 7, 32), dtype=bool), 1)                         # a full grid loses exactly its face layers
    assert full1.sum() == 5 * 5 * 30 and not full1[0].any() and not full1[:, 0].any() and not full1[:, :, 0].any() and not full1[:, :, 31].any()
    full = np.ones((7, 7, 32), dtype=bool)
    assert VR.erode(full, 2).sum() == 3 * 3 * 28
    p = np.zeros((2, 3, 64), dtype=bool)
    p[0, 0, 0] = p[0, 0, 31] = p[0, 0, 33] = p[1, 2, 63] = True
    w = VR.pack(p)
    assert w.dtype == np.uint32 and w.shape == (12,) and w[0] == 0x80000001 and w[1] == 2 and w[11] == 0x80000000 and w[2:11].sum() == 0


def test_map_is_the_or_over_sweeps():
    m = VR.RefMap(1, G0, DIMS, 1.0, hit_margin=0, erode=0)
    a = np.array([[[9.5, 0.5, 0.5]]], dtype=np.float32)
    m.integrate(a, [1], np.array([[0.5, 0.5, 0.5]], dtype=np.float32))
    assert set_voxels(m.V[0]) == [(x, 0, 0) for x in range(9)]
    b = np.array([[[4.5, 0.5, 0.5], [4.5, 3.5, 0.5]]], dtype=np.float32)          # a return INSIDE the void of the first sweep
    assert m.query(b, [2]).tolist() == [[1, 0]] and m.query(b, [0]).tolist() == [[0, 0]]
    m.integrate(b, [2], np.array([[4.5, 5.5, 0.5]], dtype=np.float32))           # seen from y = 5.5: frees y = 5..1 at x = 4
    assert set_voxels(m.V[0]) == sorted([(x, 0, 0) for x in range(9)] + [(4, y, 0) for y in (1, 2, 4, 5)])   # void stays void; O masks F
    assert set_voxels(m.O[0]) == [(4, 0, 0), (4, 3, 0)] and m.status == 0
    e1 = VR.RefMap(1, G0, DIMS, 1.0, hit_margin=0, erode=1)
    e1.integrate(a, [1], np.array([[0.5, 0.5, 0.5]], dtype=np.float32))
    assert not e1.V.any()                                                        # a single line of free voxels does not survive erosion


# ---- the library's entries and the Python layer ------------------------------------------------------------------------------------------
def test_void_entries_reject_bad_arguments_without_launching():
    """Gx % 32, a 2^31-bit grid, erode = 3, NULL buffers: negative DF_E_* codes, no launch (no GPU here)"""
    from deflow_amd import build
    from deflow_amd._lib import load
    build.build()
    lib = load()
    P, F = C.c_void_p, C.c_float
    ok = P(0x1000)
    SHAPE, ARG = -1, -3
    cast = lambda pts=ok, cnt=ok, org=ok, B=1, N=100, gx=-5.0, k=2560.0, G=(64, 48, 12), hm=2, R=204800, f=ok, o=ok: lib.df_void_cast(
        pts, cnt, org, B, N, F(gx), F(-5.0), F(-1.0), F(k), G[0], G[1], G[2], hm, R, f, o, P(0), P(0))
    probe = lambda pts=ok, G=(64, 48, 12), R=204800: lib.df_void_cast_probe(
        pts, ok, ok, 1, 100, F(-5.0), F(-5.0), F(-1.0), F(2560.0), G[0], G[1], G[2], 2, R, ok, ok, P(0), P(0), 1, P(0))
    assert probe(pts=P(0)) == ARG and probe(G=(48, 48, 12)) == SHAPE and probe(R=0) == ARG          # the measuring form checks alike
    assert cast(pts=P(0)) == ARG and cast(cnt=P(0)) == ARG and cast(org=P(0)) == ARG and cast(f=P(0)) == ARG and cast(o=P(0)) == ARG
    assert cast(G=(48, 48, 12)) == SHAPE and cast(G=(2048, 1024, 1024)) == SHAPE and cast(G=(0, 4, 4)) == SHAPE and cast(G=(32, -1, 4)) == SHAPE
    assert cast(G=(1024, 1024, 2048)) == SHAPE                                   # exactly 2^31 bits
    assert cast(B=0) == SHAPE and cast(N=0) == SHAPE and cast(B=40000, N=80000) == SHAPE and cast(B=70000, N=1) == SHAPE
    assert cast(gx=float("nan")) == ARG and cast(k=0.0) == ARG and cast(k=float("inf")) == ARG and cast(hm=-1) == ARG
    assert cast(R=0) == ARG and cast(R=(1 << 24) + 1) == ARG
    merge = lambda f=ok, o=ok, v=ok, B=1, G=(64, 48, 12), r=1: lib.df_void_merge(f, o, v, B, G[0], G[1], G[2], r, P(0))
    assert merge(f=P(0)) == ARG and merge(o=P(0)) == ARG and merge(v=P(0)) == ARG and merge(r=3) == ARG and merge(r=-1) == ARG
    assert merge(G=(33, 48, 12)) == SHAPE and merge(G=(1024, 1024, 2048)) == SHAPE and merge(B=0) == SHAPE
    query = lambda pts=ok, cnt=ok, B=1, N=100, k=2560.0, G=(64, 48, 12), v=ok, fl=ok: lib.df_void_query(
        pts, cnt, B, N, F(-5.0), F(-5.0), F(-1.0), F(k), G[0], G[1], G[2], v, fl, P(0))
    assert query(pts=P(0)) == ARG and query(cnt=P(0)) == ARG and query(v=P(0)) == ARG and query(fl=P(0)) == ARG
    assert query(G=(16, 48, 12)) == SHAPE and query(G=(1024, 1024, 2048)) == SHAPE and query(N=-1) == SHAPE and query(k=-1.0) == ARG


def test_voidmap_api_has_no_cpu_fallback():
    import deflow_amd
    from deflow_amd import voidmap
    assert deflow_amd.VoidMap is voidmap.VoidMap and deflow_amd.label_scene is voidmap.label_scene
    with pytest.raises(TypeError, match="CUDA"):
        voidmap.VoidMap(1, G0, DIMS, 1.0, device="cpu")
    cls = inspect.getsource(voidmap.VoidMap)
    for word in (".cpu()", ".item()", ".tolist()", ".numpy()", "int(status", "voidmap_ref"):     # no read-back, no other implementation
        assert word not in cls, word
    for bad in (dict(dims=(48, 4, 4)), dict(dims=(2048, 1024, 1024)), dict(erode=3), dict(hit_margin=-1), dict(voxel=0.0),
                dict(max_range=0.0), dict(grid_min=(0.0, float("nan"), 0.0)), dict(batch=0)):
        kw = dict(batch=1, grid_min=G0, dims=DIMS, voxel=1.0, device="cuda")
        kw.update(bad)
        with pytest.raises(ValueError):
            voidmap.VoidMap(**kw)
    assert voidmap.ray_limit(80.0, 0.1) == VR.ray_limit(80.0, 0.1) == 204800


def test_scene_grid_values():
    from deflow_amd.voidmap import scene_grid
    gmin, dims = scene_grid([[0, 0, 0], [10, 0, 0]], 0.5, 8.0, 2.0)
    assert gmin == (-8.0, -8.0, -2.0) and dims == (64, 32, 8)                    # (52, 32, 8), Gx rounded up to a multiple of 32
    gmin, dims = scene_grid([[1.0, 2.0, 3.0]], 0.25, 4.0, 1.0)
    assert gmin == (-3.0, -2.0, 2.0) and dims == (32, 32, 8)
    gmin, dims = scene_grid(np.array([[0.0, 0.0, 1.64], [16.8, 1.2, 1.64]]), 0.2, 25.6, 4.0)
    assert dims[0] % 32 == 0 and dims[0] >= 340 and dims[1] in (262, 263) and dims[2] in (40, 41)
    with pytest.raises(ValueError, match="coarsen voxel"):
        scene_grid([[0, 0, 0], [300, 0, 0]], 0.05, 51.2, 4.0)
    with pytest.raises(ValueError):
        scene_grid(np.zeros((0, 3)), 0.1, 51.2, 4.0)


def test_sweep_frames_are_float64_then_fp32():
    from deflow_amd.voidmap import sweep_frames
    p0, p1 = np.eye(4), np.eye(4)
    p0[:3, 3], p1[:3, 3] = (100.0, 50.0, 0.0), (100.7, 50.05, 0.0)
    lidar = np.array([[1.0, 2.0, 3.0, 0.5]], dtype=np.float32)                   # further columns (intensity) are ignored
    pts, org = sweep_frames([lidar, lidar], [p0.astype(np.float32), p1.astype(np.float32)], (1.0, 0.0, 2.0))
    assert pts[0].dtype == np.float32 and pts[0].tolist() == [[1.0, 2.0, 3.0]] and org[0].tolist() == [1.0, 0.0, 2.0]
    want = (np.array([1.0, 2.0, 3.0]) + (np.float64(np.float32(100.7)) - 100.0, np.float64(np.float32(50.05)) - 50.0, 0.0)).astype(np.float32)
    assert np.array_equal(pts[1][0], want) and org.dtype == np.float64


def test_sweep_frames_rotation_and_order():
    """T_i = inv(pose_0) @ pose_i with a yaw: a transposed rotation, a swapped product or a wrong origin give other numbers"""
    from deflow_amd.voidmap import sweep_frames
    yaw = lambda deg, t: np.array([[np.cos(np.radians(deg)), -np.sin(np.radians(deg)), 0, t[0]],
                                   [np.sin(np.radians(deg)), np.cos(np.radians(deg)), 0, t[1]], [0, 0, 1, t[2]], [0, 0, 0, 1.0]])
    p0, p1 = yaw(90, (10.0, 20.0, 1.0)), yaw(180, (10.0, 23.0, 1.0))             # the vehicle turned left by 90 degrees and moved 3 m in world y
    lidar = np.array([[2.0, 0.0, 0.5], [0.0, 1.0, 0.0]], dtype=np.float32)
    pts, org = sweep_frames([lidar, lidar], [p0, p1], (1.0, 0.0, 2.0))
    assert np.allclose(pts[0], lidar, atol=1e-6) and np.allclose(org[0], (1.0, 0.0, 2.0), atol=1e-12)
    # in frame 0 (x = world y, y = -world x): frame 1 sits at (3, 0, 0) and is turned by +90 degrees: (x, y) -> (3 - y, x)
    assert np.allclose(pts[1], [[3.0, 2.0, 0.5], [2.0, 0.0, 0.0]], atol=1e-6) and np.allclose(org[1], (3.0, 1.0, 2.0), atol=1e-12)


def test_command_line_keys():
    from deflow_amd.voidmap import parse_args
    cfg = parse_args(["data_dir=/d", "scenes=a,b", "overwrite=true", "voxel=0.2", "range_xy=25.6", "hit_margin=1", "erode=2",
                      "sensor_offset=1,0,2", "max_range=60"])
    assert cfg == {"data_dir": "/d", "scenes": ["a", "b"], "overwrite": True, "voxel": 0.2, "range_xy": 25.6, "z_half": 4.0,
                   "sensor_offset": [1.0, 0.0, 2.0], "hit_margin": 1, "erode": 2, "max_range": 60.0}
    cfg = parse_args(["data_dir=/d"])
    assert cfg["scenes"] is None and cfg["overwrite"] is False and cfg["voxel"] == 0.1 and cfg["sensor_offset"] == [1.35, 0.0, 1.64]
    for bad in (["voxel=0.2"], ["data_dir=/d", "voxle=0.2"], ["data_dir=/d", "overwrite=maybe"], ["data_dir=/d", "erode=x"], ["data_dir"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


# ---- the sidecar -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def scene_dir(tmp_path, golden_dir):
    """a copy of scene_a.h5 with an index of its own: nothing is ever written under tests/golden"""
    src = os.path.join(golden_dir, "av2_mini", "train")
    shutil.copy(os.path.join(src, "scene_a.h5"), tmp_path / "scene_a.h5")
    with open(os.path.join(src, "index_total.pkl"), "rb") as f:
        index = [e for e in pickle.load(f) if e[0] == "scene_a"]
    with open(tmp_path / "index_total.pkl", "wb") as f:
        pickle.dump(index, f)
    return str(tmp_path)


def random_flags(ds, seed=3):
    f = ds._file("scene_a")
    g = np.random.default_rng(seed)
    return {ts: (g.random(f[ts]["lidar"].read().shape[0]) < 0.4).astype(np.uint8) for ts in f.sweeps}


def test_directory_without_a_sidecar_yields_todays_items(scene_dir):
    from deflow_amd.data import HDF5Dataset, collate_fn_pad
    ds, off = HDF5Dataset(scene_dir), HDF5Dataset(scene_dir, dynamic_sidecar=None)
    assert ds.dynamic_sidecar == ".dufo.npz" and len(ds) == 24
    for i in (0, 5, 23):
        a, b = ds[i], off[i]
        assert set(a) == set(b) and "dufo0" not in a
        assert all(torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k] for k in a)
    assert "pc0_dufo" not in collate_fn_pad([ds[0], ds[1]])


def test_sidecar_is_read_and_carried_through_the_collate(scene_dir):
    from deflow_amd.data import HDF5Dataset, collate_fn_pad
    from deflow_amd.voidmap import read_sidecar, write_sidecar
    plain = HDF5Dataset(scene_dir, dynamic_sidecar=None)
    flags = random_flags(plain)
    write_sidecar(os.path.join(scene_dir, "scene_a.dufo.npz"), flags, {"voxel": 0.2})
    back = read_sidecar(os.path.join(scene_dir, "scene_a.dufo.npz"))
    assert set(back) == set(flags) and all(np.array_equal(back[k], flags[k]) and back[k].dtype == np.uint8 for k in flags)
    with np.load(os.path.join(scene_dir, "scene_a.dufo.npz")) as z:
        assert '"voxel": 0.2' in str(z["meta"])
    ds = HDF5Dataset(scene_dir)
    sweeps = ds._file("scene_a").sweeps
    items = [ds[i] for i in (0, 7, 23)]                                          # 23: the last indexed sweep pairs with the unlabelled one
    for i, it in zip((0, 7, 23), items):
        assert it["dufo0"].dtype == torch.bool and it["dufo0"].shape == (it["pc0"].shape[0],)
        assert torch.equal(it["dufo0"], torch.from_numpy(flags[sweeps[i]]) != 0)
        assert torch.equal(it["dufo1"], torch.from_numpy(flags[sweeps[i + 1]]) != 0)
        assert set(it) - set(plain[i]) == {"dufo0", "dufo1"} and set(plain[i]) <= set(it)
    res = collate_fn_pad(items)
    assert res["pc0_dufo"].shape == res["pc0"].shape[:2] and res["pc1_dufo"].shape == res["pc1"].shape[:2]
    for b, it in enumerate(items):                                              # ground rows dropped like the points, padded rows 0
        for key, src, gm in (("pc0_dufo", "dufo0", "gm0"), ("pc1_dufo", "dufo1", "gm1")):
            kept = it[src][~it[gm]].long()
            assert torch.equal(res[key][b, : kept.numel()], kept) and bool((res[key][b, kept.numel():] == 0).all())
    assert "dufo0" not in HDF5Dataset(scene_dir, dynamic_sidecar=None)[0]
    assert ds._sidecar("scene_a") is ds._sidecar("scene_a")                      # cached per scene


def test_sidecar_length_mismatch_raises(scene_dir):
    from deflow_amd.data import HDF5Dataset
    from deflow_amd.voidmap import write_sidecar
    flags = random_flags(HDF5Dataset(scene_dir))
    ts = sorted(flags, key=int)[3]
    flags[ts] = flags[ts][:-1]
    write_sidecar(os.path.join(scene_dir, "scene_a.dufo.npz"), flags, {})
    ds = HDF5Dataset(scene_dir)
    assert "dufo0" in ds[0]
    with pytest.raises(ValueError, match="flags for sweep"):
        ds[3]
    with pytest.raises(ValueError, match="flags for sweep"):
        ds[2]                                                                    # as the pair's second sweep
