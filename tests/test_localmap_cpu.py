"""CPU: the scan-to-map odometry's command-line keys, the restatement of tests/helpers/map_ref.py against an independent "first K per
voxel" written another way, and the conditions of the loop scene that tests/test_gpu_localmap.py registers on the GPU, on the float64
reference alone.

The loop scene (17 sweeps of reg_ref.lattice(700, seed 2) on a closed loop of radius 0.7 m, a random 70 % of the nodes and 1 cm of noise
per sweep, the last sweep a row-permuted copy of sweep 0, levels ((1.0, 6), (0.5, 6)), map voxel 0.5 m).  Measured on the reference:
closing pose off the truth by 8.2e-9 (K = 1) and 8.7e-9 (K = 2) with the map and by 1.6e-3 scan-to-scan; the intermediate poses are
noise-limited at 1.4e-3 with either; smallest nearest / second-nearest margin at K = 1: 1.35e-4 m (seeds 0 and 1: 4.8e-5, 1.5e-5, which
is why the scene takes seed 2).  K = 4 is registered on the GPU against the truth (tests/test_gpu_localmap.py); it takes 10 s here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import map_ref  # noqa: E402


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_command_parser_takes_the_map_keys():
    from deflow_amd.odometry import CLI_DEFAULTS, MAP_DEFAULTS, USAGE, parse_args
    assert MAP_DEFAULTS == {"target": "scan", "map_voxel": 0.5, "map_max_per_voxel": 4, "map_capacity": 524288}
    cfg = parse_args(["data_dir=/d", "target=map", "map_voxel=0.25"])
    assert (cfg["target"], cfg["map_voxel"], cfg["map_max_per_voxel"], cfg["map_capacity"]) == ("map", 0.25, 4, 524288)
    assert {k: v for k, v in cfg.items() if k not in ("data_dir", "target", "map_voxel")} == \
        {k: v for k, v in CLI_DEFAULTS.items() if k not in ("data_dir", "target", "map_voxel")}
    assert parse_args(["data_dir=/d"])["target"] == "scan"
    cfg = parse_args(["data_dir=/d", "map_max_per_voxel=2", "map_capacity=4096"])
    assert (cfg["map_max_per_voxel"], cfg["map_capacity"]) == (2, 4096)
    for bad in ("target=foo", "map_max_per_voxel=0", "map_capacity=0", "map_voxel=0", "map_voxel=nan", "map_voxel=-1", "map_capacity=1.5"):
        with pytest.raises(SystemExit):
            parse_args(["data_dir=/d", bad])
    for key in ("target=scan|map", "map_voxel=", "map_max_per_voxel=", "map_capacity="):
        assert key in USAGE


def test_register_sweeps_refuses_bad_map_arguments_before_the_gpu():
    from deflow_amd.odometry import register_sweeps
    with pytest.raises(ValueError, match="target must be 'scan' or 'map'"):
        register_sweeps([np.zeros((4, 3))], target="both")
    with pytest.raises(ValueError, match="map_capacity must be an integer"):
        register_sweeps([np.zeros((4, 3))], target="map", map_capacity=0)
    with pytest.raises(ValueError, match="map_voxel must be positive"):
        register_sweeps([np.zeros((4, 3))], target="map", map_voxel=float("nan"))
    with pytest.raises(TypeError, match="device must be a CUDA device"):
        register_sweeps([np.zeros((4, 3))], target="map", device="cpu")


def test_bindings_of_the_map_entries_match_the_header():
    import abi_sizes
    from deflow_amd import _lib
    protos = abi_sizes.header_prototypes()
    names = list(_lib._SIGS)
    new = ["df_map_ws_bytes", "df_map_keys", "df_map_select", "df_map_compact", "df_map_view"]
    assert names[-5:] == new and names[-6] == "df_reg_accumulate_plane"            # appended: the sized window stays as it is
    for n in new:
        assert len(_lib._SIGS[n]) == len(protos[n])
        for t, p in zip(_lib._SIGS[n], protos[n]):
            assert (t is _lib.P) == p.pointer, (n, p.name)
    assert [p.name for p in protos["df_map_keys"] if p.nullable] == ["mask", "gate"]
    assert "df_map_ws_bytes" in _lib._RAW and _lib._RESTYPE["df_map_ws_bytes"] is _lib.C.c_int64


def test_map_entries_reject_bad_arguments_without_launching():
    """every check fails before the launch: fake (aligned, never dereferenced) addresses do on a machine without a GPU"""
    import ctypes as C
    from deflow_amd import _lib, build
    build.build()
    lib = _lib.load()
    P, a = C.c_void_p, 0x10000

    def keys(map_=a, B=2, cap=700, N=600, voxel=0.5, W=8, vz=a):
        return lib.df_map_keys(P(map_), P(a), P(a), P(a), P(0), P(0), P(a), B, cap, N, voxel, W, P(a), P(a), P(vz), P(0))

    assert keys(map_=0) == -3 and keys(vz=0) == -3 and keys(map_=a + 4) == -2
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert keys(voxel=v) == -3, v
    assert keys(B=0) == -1 and keys(B=65536) == -1 and keys(cap=0) == -1 and keys(N=0) == -1 and keys(W=0) == -1 and keys(W=2048) == -1
    assert keys(B=2, cap=2 ** 29, N=1) == -1 and keys(B=65535, W=64) == -1                       # B n, B S S >= 2^30
    assert lib.df_map_select(P(a), P(a), P(a), P(a), 2, 1300, 8, 0, P(a), P(0)) == -3
    assert lib.df_map_select(P(a), P(a), P(a), P(a), 2, 0, 8, 1, P(a), P(0)) == -1
    assert lib.df_map_select(P(a), P(0), P(a), P(a), 2, 1300, 8, 1, P(a), P(0)) == -3
    assert lib.df_map_compact(P(a), P(a), P(a), P(a), 2, 700, 600, 8, P(a), P(a), P(a), P(a), P(0)) == -3        # map_out == cand
    assert lib.df_map_compact(P(a), P(a), P(a), P(a), 2, 700, 600, 8, P(2 * a), P(a), P(a), P(0), P(0)) == -3
    assert lib.df_map_compact(P(a), P(a), P(a), P(a), 2, 700, 600, 2048, P(2 * a), P(a), P(a), P(a), P(0)) == -1
    assert lib.df_map_view(P(a), P(a), P(a), 0, 700, P(a), P(0)) == -1 and lib.df_map_view(P(a), P(a), P(0), 2, 700, P(a), P(0)) == -3
    assert _lib.call("df_map_ws_bytes", 3, 700, 600) == 8 * 3 * 6 and _lib.call("df_map_ws_bytes", 0, 700, 600) == -1


# ---- the restatement against "first K per voxel" written another way -------------------------------------------------------------------
def first_k_per_voxel(world, ok, voxel, anchor, W, K):
    """vectorised numpy, no dict: the rows (in candidate order) whose voxel is in the window, ranked inside their voxel by a stable sort
    -> (kept candidates in (dy, dx, candidate) order, keep [n])"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.floor(world / voxel)
    fin = ok & np.isfinite(world).all(axis=1) & (np.abs(np.where(np.isfinite(v), v, 0.0)) < 2.0 ** 30).all(axis=1)
    v = np.where(fin[:, None], v, 0.0).astype(np.int64)
    d = v[:, :2] - np.asarray(anchor) + W
    fin &= ((d >= 0) & (d <= 2 * W)).all(axis=1)
    rows = np.flatnonzero(fin)
    order = rows[np.lexsort((rows, v[rows, 2], d[rows, 0], d[rows, 1]))]            # by (dy, dx, vz), candidate order inside a voxel
    vox = np.stack((d[order, 1], d[order, 0], v[order, 2]), axis=1)
    first = np.ones(len(order), dtype=bool)
    first[1:] = (vox[1:] != vox[:-1]).any(axis=1)
    start = np.maximum.accumulate(np.where(first, np.arange(len(order)), 0))
    keep = np.zeros(world.shape[0], dtype=np.int32)
    keep[order[np.arange(len(order)) - start < K]] = 1
    kept = np.flatnonzero(keep)
    return kept[np.lexsort((kept, d[kept, 0], d[kept, 1]))], keep


@pytest.mark.parametrize("K", [1, 3, 20])
def test_restatement_agrees_with_an_independent_first_k_per_voxel(K):
    rng = np.random.default_rng(K)
    voxel, W, cap, N = 0.3, 8, 700, 600
    pose = np.eye(4)
    pose[:3, 3] = (-5.1, -7.3, 0.0)
    ax, ay = -17, -25
    pts = pose[:3, 3] + rng.uniform(-2.9, 2.9, size=(cap, 3))
    r = 0
    for k in (-20, -12, -9, -25):                                    # exact integers of w / voxel and one ulp either side
        w = np.float64(k) * voxel
        for x in (w, np.nextafter(w, -np.inf), np.nextafter(w, np.inf)):
            pts[r] = (x, (ay + 0.5) * voxel, x)
            r += 1
    for d in (-W - 1, -W, W, W + 1):                                 # dx, dy at -1, 0, 2 W, 2 W + 1
        pts[r], pts[r + 1] = ((ax + d + 0.5) * voxel, (ay + 0.5) * voxel, 0.0), ((ax + 0.5) * voxel, (ay + d + 0.5) * voxel, 0.0)
        r += 2
    pts[r], pts[r + 1, 0], pts[r + 2, 1], pts[r + 3, 2] = np.nan, np.inf, 1e300, 0.3 * 2.0 ** 30
    sweep = rng.uniform(-3.0, 3.0, size=(N, 3)).astype(np.float32)
    sweep[:200] = (np.array((2, -3, 1)) + rng.uniform(0.05, 0.95, size=(200, 3))) * voxel      # a crowded voxel
    sweep[200:260, 2] = np.where(np.arange(60) % 2 == 0, 0.5, -1.0)                            # two z voxels interleaved ...
    sweep[200:260, :2] = (0.31, 0.31)                                                          # ... in one column
    sweep[300], sweep[301, 1], sweep[302, 0] = np.nan, np.inf, 3e38
    mask = np.ones(N, dtype=np.int32)
    mask[::7] = 0
    count, sweep_count = 650, N - 20
    cand, key, vz = map_ref.keys(pts, count, sweep, sweep_count, mask, None, pose, voxel, W)
    drop = (2 * W + 1) ** 2
    keep = map_ref.select(key, vz, drop, K)
    out, cnt, stat = map_ref.compact(cand, key, keep, drop, cap)
    world = np.concatenate((pts, sweep.astype(np.float64) + pose[:3, 3]))                       # (R = I: a + t, one rounding)
    ok = np.concatenate((np.arange(cap) < count, (np.arange(N) < sweep_count) & (mask > 0) & np.isfinite(sweep).all(axis=1)))
    kept, keep2 = first_k_per_voxel(world, ok, voxel, (ax, ay), W, K)
    assert np.array_equal(keep, keep2) and keep[:count].sum() > 300 and keep[cap:].sum() > 50
    assert stat == ((key < drop).sum(), len(kept), (kept >= cap).sum(), max(0, len(kept) - cap)) and cnt == min(len(kept), cap)
    assert np.array_equal(out[:cnt].view(np.int64), world[kept[:cap]].view(np.int64)) and np.isnan(out[cnt:]).all()
    gated = map_ref.keys(pts, count, sweep, sweep_count, mask, 2, pose, voxel, W)[1]
    assert (gated[cap:] == drop).all() and np.array_equal(gated[:cap], key[:cap])
    bad = pose.copy()
    bad[1, 3] = np.nan
    assert (map_ref.keys(pts, count, sweep, sweep_count, mask, None, bad, voxel, W)[1] == drop).all()


def test_view_restatement_inverts_the_insert():
    rng = np.random.default_rng(0)
    from reg_ref import se3_exp
    pose = se3_exp((0.1, -0.2, 0.7, 200.0, -150.0, 2.0))
    sweep = rng.uniform(-1.3, 1.3, size=(50, 3)).astype(np.float32)               # (inside the window under any rotation)
    m, cnt, stat = map_ref.insert(np.full((64, 3), np.nan), 0, sweep, 50, pose, 0.3, 8, 50)
    back = map_ref.view(m, cnt, pose)
    assert cnt == 50 and stat == (50, 50, 50, 0) and (back[cnt:].view(np.uint32) == 0x7FC00000).all()
    assert np.abs(np.sort(back[:cnt], axis=0) - np.sort(sweep, axis=0)).max() <= 2e-6      # 300 m out: float64 keeps what fp32 had


# ---- the loop scene on the reference alone ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return map_ref.loop_scene(map_ref.LOOP_SEED, nodes=map_ref.LOOP_NODES)


@pytest.mark.parametrize("K", [1, 2])
def test_loop_scene_conditions_on_the_reference(scene, K):
    sweeps, truth = scene
    assert len(sweeps) == 17 and np.array_equal(np.sort(sweeps[-1], axis=0), np.sort(sweeps[0], axis=0)) and not np.array_equal(sweeps[-1], sweeps[0])
    r = map_ref.register_sweeps_map(sweeps, map_ref.LOOP["levels"], voxel=map_ref.LOOP["voxel"], K=K, cap=4096, W=map_ref.LOOP_W, gaps=K == 1)
    assert r["status"] == [0] * 16 and r["maps"][-1][2][3] == 0
    m, cnt, _ = r["maps"][-1]
    have = {tuple(x) for x in m[:cnt]}
    assert all(tuple(x) in have for x in sweeps[0].astype(np.float64))            # every row of sweep 0 is in the final map
    closing = np.abs(r["poses"][-1] - truth[-1]).max()
    mid = max(np.abs(P - T).max() for P, T in zip(r["poses"][1:-1], truth[1:-1]))
    print("K", K, "closing", closing, "intermediate", mid, "map rows", cnt, "gap", min(r["gap"]) if r["gap"] else None)
    assert closing <= 1e-6 and mid <= 1e-2
    if K == 1:                                                                    # (K > 1 cannot hold it: see map_ref.LOOP_SEED)
        assert len(r["gap"]) == 16 and min(r["gap"]) >= 1e-4


def test_loop_scene_scan_to_scan_drifts(scene):
    sweeps, truth = scene
    poses = map_ref.register_sweeps_scan(sweeps, map_ref.LOOP["levels"])
    closing = np.abs(poses[-1] - truth[-1]).max()
    print("scan closing", closing)
    assert closing > 1e-4
