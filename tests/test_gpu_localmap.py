"""GPU: the local map of the scan-to-map odometry -- df_map_keys, df_map_select, df_map_compact, df_map_view,
``localmap.LocalMap``, ``odometry.register_sweeps(target="map")`` and the command -- against the integer / float64 restatement of
tests/helpers/map_ref.py, whose own conditions tests/test_localmap_cpu.py checks without a GPU.

Shapes: cap = 700 map rows and N = 600 sweep rows (640 in the select test), so n = 1300 candidates are six blocks of 256, the last one
partial; B <= 3; W = 8 (17 x 17 columns); voxel 0.3 (non-dyadic).  Everything but the registration is EQUAL to the restatement, bit for
bit.

Measured on an MI355X, the loop scene of map_ref (seed 2): every pose of ``register_sweeps(target="map")`` within 6.8e-8 of the
restatement's at K = 1, stride 1 (bound 1e-4); closing pose off the truth by 2.2e-8 (K = 1), 4.8e-8 (K = 2), 5.1e-8 (K = 4), 6.7e-8
(K = 4, stride 3), ``target="scan"`` on the same arrays by 1.6e-3.  ``residual="plane"`` on plane_ref's planar scene out and back:
closing pose 1.2e-8 off the truth, the intermediate ones <= 1.1e-7.  The restatement is compared at K = 1 only: there the nearest and
the second-nearest map row of every used row differ by >= 1e-4 m (tests/test_localmap_cpu.py), so fp32 and float64 pick the same
partners; with K > 1 a voxel holds several noisy copies of one node and no seed gives that margin."""
import json
import os
import pickle
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi_sizes  # noqa: E402
import guarded  # noqa: E402
import map_ref  # noqa: E402
import reg_ref  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, N, W, VOXEL = 700, 600, 8, 0.3
MAX_RANGE = 2.0                      # ceil(2.0 / 0.3) + 1 = 8
TOL = 1e-4                           # section 6r's bound: the per-row fp32 roundings carried through a well-conditioned fit


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def i32(dev, v):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def f64bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def new_map(dev, B, K, cap=CAP):
    from deflow_amd.localmap import LocalMap
    m = LocalMap(B, cap, voxel=VOXEL, max_per_voxel=K, max_range=MAX_RANGE, device=dev)
    assert m.W == W and m.S == 2 * W + 1
    return m


def load(m, pts, counts):
    """put a state of the test's own into the map (rows >= count stay as given: the entries must not read them as taking part)"""
    m.points = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(m.dev)
    m.count = i32(m.dev, counts)


def check_insert(m, state, sweep, sweep_count, pose, K, mask=None, gate=None):
    """one LocalMap.insert from ``state`` = (map [B,cap,3], counts) against the restatement, stage by stage and bit for bit"""
    pts, counts = state
    B, cap = pts.shape[0], pts.shape[1]
    load(m, pts, counts)
    dev = m.dev
    m.insert(torch.from_numpy(sweep).to(dev), i32(dev, sweep_count), torch.from_numpy(pose).to(dev),
             mask=None if mask is None else torch.from_numpy(mask).to(dev), gate=None if gate is None else i32(dev, gate))
    n = cap + sweep.shape[1]
    S = 2 * W + 1
    got = {k: v.cpu().numpy() for k, v in m.last.items()}
    total = 0
    for b in range(B):
        cand, key, vz = map_ref.keys(pts[b], counts[b], sweep[b], sweep_count[b], None if mask is None else mask[b],
                                     None if gate is None else gate[b], pose[b], VOXEL, W, b, B)
        drop = B * S * S
        assert np.array_equal(f64bits(got["cand"][b]), f64bits(cand)), b
        assert np.array_equal(got["key"].reshape(B, n)[b].astype(np.int64), key), b
        assert np.array_equal(got["vz"].reshape(B, n)[b].astype(np.int64), vz), b
        keep = map_ref.select(key, vz, drop, K)
        assert np.array_equal(got["keep"].reshape(B, n)[b], keep), b
        order = map_ref.sorted_order(key, drop)
        assert np.array_equal(got["idx_sorted"][total:total + len(order)].astype(np.int64), order + b * n), b
        total += len(order)
        want, cnt, stat = map_ref.compact(cand, key, keep, drop, cap)
        assert np.array_equal(f64bits(m.points[b].cpu().numpy()), f64bits(want)), b
        assert int(m.count[b]) == cnt and tuple(m.stat[b].tolist()) == stat, (b, int(m.count[b]), m.stat[b].tolist(), cnt, stat)
    return m.points.cpu().numpy(), m.count.cpu().numpy()


# ---- keys -------------------------------------------------------------------------------------------------------------------------------
def far_pose():
    T = reg_ref.se3_exp((0.0, 0.2, 0.7, 0.0, 0.0, 0.0))              # pitch and yaw
    T[:3, 3] = (212.3, -211.9, 1.7)                                  # 300 m from the origin
    return T


def keys_batch():
    rng = np.random.default_rng(3)
    pose = np.stack((far_pose(), np.eye(4), reg_ref.se3_exp((0.01, -0.02, 0.3, 1.0, -2.0, 0.1))))
    pose[1, :3, 3] = (-5.1, -7.3, 0.0)
    sweep = rng.uniform(-3.0, 3.0, size=(3, N, 3)).astype(np.float32)  # the window reaches 2.4 .. 2.7 m: some rows fall outside it
    sweep[0, 5], sweep[0, 6, 1], sweep[0, 7, 2], sweep[0, 8, 0] = np.nan, np.inf, -np.inf, 3e38
    mask = np.ones((3, N), dtype=np.int32)
    mask[1, ::7] = 0
    mask[0, :] = 5
    mask[2, 3] = -1
    pts = pose[:, None, :3, 3] + rng.uniform(-2.9, 2.9, size=(3, CAP, 3))
    ax, ay = map_ref.voxel_of(-5.1, VOXEL), map_ref.voxel_of(-7.3, VOXEL)
    assert (ax, ay) == (-17, -25)
    r, sides = 0, set()
    for k in (-20, -12, -9, -25, -15):                               # w / voxel an exact integer, and one ulp either side
        w = np.float64(k) * VOXEL
        if w / VOXEL != k:
            continue
        for x in (w, np.nextafter(w, -np.inf), np.nextafter(w, np.inf)):
            pts[1, r] = (x, (ay + 0.5) * VOXEL, 0.1)
            pts[1, r + 1] = ((ax + 0.5) * VOXEL, np.float64(k - 8) * VOXEL + (x - w), x)
            sides.add(map_ref.voxel_of(float(x), VOXEL) - k)
            r += 2
    assert r >= 18 and sides == {-1, 0}                              # floor, not truncation: one ulp below a negative integer is k - 1
    for d in (-W - 1, -W, W, W + 1):                                 # dx, dy at -1, 0, 2 W, 2 W + 1
        pts[1, r] = ((ax + d + 0.5) * VOXEL, (ay + 0.5) * VOXEL, 0.0)
        pts[1, r + 1] = ((ax + 0.5) * VOXEL, (ay + d + 0.5) * VOXEL, 0.0)
        r += 2
    pts[1, r], pts[1, r + 1, 0], pts[1, r + 2, 1], pts[1, r + 3, 2], pts[1, r + 4, 2] = np.nan, np.inf, 1e300, -1e300, 0.3 * 2.0 ** 30
    counts = [650, CAP, 0]                                           # sample 2: count 0, its rows are finite
    return pts, counts, sweep, [N, N - 20, N], pose, mask


def test_keys_and_the_whole_update_on_the_edge_cases(dev):
    pts, counts, sweep, sc, pose, mask = keys_batch()
    m = new_map(dev, 3, 3)
    _, cnt = check_insert(m, (pts, counts), sweep, sc, pose, 3, mask)
    assert cnt[0] > 100 and cnt[1] > 100 and cnt[2] > 100
    key = m.last["key"].cpu().numpy().reshape(3, CAP + N)
    drop = 3 * 17 * 17
    assert (key[0, CAP + 5:CAP + 9] == drop).all() and (key[2, :CAP] == drop).all() and key[2, CAP + 3] == drop
    assert (key[1, CAP + N - 20:] == drop).all() and (key[1, CAP::7] == drop).all() and (key[0, 650:CAP] == drop).all()
    # gate = 2 drops the whole sweep of that sample only
    check_insert(m, (pts, counts), sweep, sc, pose, 3, mask, gate=[0, 2, 0])
    key = m.last["key"].cpu().numpy().reshape(3, CAP + N)
    assert (key[1, CAP:] == drop).all() and (key[1, :CAP] < drop).sum() > 100 and (key[0, CAP:] < drop).sum() > 100
    assert int(m.stat[1, 2]) == 0
    # a pose that is not finite empties the sample
    for bad in (np.nan, np.inf, 1e300):
        p2 = pose.copy()
        p2[1, 0, 3] = bad
        check_insert(m, (pts, counts), sweep, sc, p2, 3, mask)
        assert int(m.count[1]) == 0 and m.stat[1].tolist() == [0, 0, 0, 0] and int(m.count[0]) == cnt[0]
        assert bool(torch.isnan(m.points[1]).all())


# ---- select -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 20])
def test_select_keeps_the_first_k_of_a_voxel(dev, K):
    n_s = 640
    rng = np.random.default_rng(K)
    pose = np.stack((np.eye(4), np.eye(4)))

    def inside(vox, size):
        return (np.asarray(vox, dtype=np.float64) + rng.uniform(0.05, 0.95, size=(size, 3))) * VOXEL

    sweep = np.empty((2, n_s, 3), dtype=np.float32)
    sweep[0] = inside((2, -3, 1), n_s)                               # 640 rows in one voxel: more than two blocks
    full, short, col = (-4, 5, 0), (6, 6, -2), (0, 0)
    pts = np.full((2, CAP, 3), np.nan)
    pts[1, :K] = inside(full, K)                                     # a voxel that holds K map rows
    pts[1, K:2 * K - 1] = inside(short, K - 1)                       # a voxel that holds K - 1
    sweep[1, :10] = inside(full, 10)
    sweep[1, 10:20] = inside(short, 10)
    z = np.where(np.arange(n_s - 20) % 2 == 0, 3, -4)                # two z voxels interleaved in one column
    sweep[1, 20:] = (np.stack((np.full(n_s - 20, col[0]), np.full(n_s - 20, col[1]), z), axis=1) +
                     rng.uniform(0.05, 0.95, size=(n_s - 20, 3))) * VOXEL
    counts = [0, 2 * K - 1]
    m = new_map(dev, 2, K)
    check_insert(m, (pts, counts), sweep, [n_s, n_s], pose, K)
    keep = m.last["keep"].cpu().numpy().reshape(2, CAP + n_s)
    assert keep[0, CAP:].tolist() == [1] * K + [0] * (n_s - K)
    assert keep[1, :2 * K - 1].all() and not keep[1, 2 * K - 1:CAP].any()          # map rows inside the window are never dropped
    assert not keep[1, CAP:CAP + 10].any()                                         # the full voxel refuses every new row
    assert keep[1, CAP + 10:CAP + 20].tolist() == [1] + [0] * 9                    # K - 1 rows: exactly the first new row
    want = np.zeros(n_s - 20, dtype=np.int32)
    want[:2 * K] = 1
    assert keep[1, CAP + 20:].tolist() == want.tolist()
    assert m.stat.tolist() == [[n_s, K, K, 0], [2 * K - 1 + n_s, 2 * K - 1 + 1 + 2 * K, 1 + 2 * K, 0]]


# ---- compact ----------------------------------------------------------------------------------------------------------------------------
def test_compact_order_tail_overflow_and_an_empty_sample(dev):
    rng = np.random.default_rng(11)
    vox = np.stack(np.meshgrid(np.arange(-8, 9), np.arange(-8, 9), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3)
    vox = vox[rng.permutation(len(vox))]                             # 867 voxels of the window
    centre = (vox + 0.5) * VOXEL
    pts = np.full((3, CAP, 3), np.nan)
    pts[0, :300] = centre[:300]
    sweep = np.zeros((3, N, 3), dtype=np.float32)
    sweep[0, :405] = centre[300:705]                                 # 405 new voxels: kept = 705 = cap + 5
    sweep[0, 405:] = centre[rng.integers(0, 705, size=N - 405)] + 0.01             # occupied: refused at K = 1
    pts[1, :200] = centre[:200] + rng.uniform(-0.1, 0.1, size=(200, 3))
    sweep[1] = rng.uniform(-2.5, 2.5, size=(N, 3))
    sweep[1, :, 2] = rng.uniform(0.01, 0.29, size=N)                 # one z voxel: fewer new voxels than free rows
    pts[2] = centre[:CAP]                                            # finite rows behind count = 0
    pose = np.stack((np.eye(4),) * 3)
    m = new_map(dev, 3, 1)
    out, cnt = check_insert(m, ((pts, [300, 200, 0])), sweep, [N, N, 0], pose, 1)
    assert m.stat[0].tolist() == [300 + N, CAP + 5, 405, 5] and cnt[0] == CAP and np.isfinite(out[0]).all()
    assert 200 < cnt[1] < CAP and np.isfinite(out[1, :cnt[1]]).all() and np.isnan(out[1, cnt[1]:]).all()
    assert (f64bits(out[1, cnt[1]:]) == 0x7FF8000000000000).all()
    assert cnt[2] == 0 and m.stat[2].tolist() == [0, 0, 0, 0] and (f64bits(out[2]) == 0x7FF8000000000000).all()
    # the stored order is the sorted one: columns ascending
    S = 17
    col = (np.floor(out[1, :cnt[1], 1] / VOXEL) + W) * S + np.floor(out[1, :cnt[1], 0] / VOXEL) + W
    assert (np.diff(col) >= 0).all()


# ---- view -------------------------------------------------------------------------------------------------------------------------------
def test_view_is_float64_arithmetic_rounded_to_fp32(dev):
    pts, counts, sweep, sc, pose, mask = keys_batch()
    m = new_map(dev, 3, 3)
    load(m, pts, counts)
    m.insert(torch.from_numpy(sweep).to(dev), i32(dev, sc), torch.from_numpy(pose).to(dev))
    state, cnt = m.points.cpu().numpy(), m.count.cpu().numpy()
    pose2 = pose.copy()
    pose2[:, :3, 3] += (0.11, -0.07, 0.013)
    pose2[2] = reg_ref.se3_exp((0.3, -0.2, 0.1, 1.0, 2.0, 3.0))
    dst, c = m.view(torch.from_numpy(pose2).to(dev))
    assert dst.dtype == torch.float32 and tuple(dst.shape) == (3, CAP, 3) and c.tolist() == cnt.tolist()
    got = dst.cpu().numpy()
    for b in range(3):
        want = map_ref.view(state[b], cnt[b], pose2[b])
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), b
        assert (got[b, cnt[b]:].view(np.uint32) == 0x7FC00000).all() and np.isfinite(got[b, :cnt[b]]).all()
    assert np.abs(got[0, :cnt[0]]).max() < 6.0                       # 300 m from the origin, and the view is about the sensor


# ---- invariants -------------------------------------------------------------------------------------------------------------------------
def test_reinsertion_repetition_and_batch_independence(dev):
    pts, counts, sweep, sc, pose, mask = keys_batch()
    dsweep, dsc, dpose = torch.from_numpy(sweep).to(dev), i32(dev, sc), torch.from_numpy(pose).to(dev)

    def run(K, twice, B=3):
        m = new_map(dev, B, K)
        for _ in range(2 if twice else 1):
            m.insert(dsweep[:B], dsc[:B], dpose[:B])
        return m.points.clone(), m.count.clone(), m.stat.clone()

    once, again = run(1, False), run(1, True)
    assert guarded.same_bits(once[0], again[0]) and guarded.same_bits(once[1], again[1])          # K = 1: the same sweep adds nothing
    assert again[2][:, 2].tolist() == [0, 0, 0] and int(once[1].min()) > 50
    a, b = run(3, True), run(3, True)
    assert all(guarded.same_bits(x, y) for x, y in zip(a, b))
    one = run(3, True, B=1)
    assert all(guarded.same_bits(x, y[:1]) for x, y in zip(one, a))


# ---- the guarded-call harness -----------------------------------------------------------------------------------------------------------
_i, _o = abi_sizes.i, abi_sizes.o
_ROWS = "4 * B * (cap + N)"
_RNG = "8 * B * (2 * W + 1) * (2 * W + 1)"
MAP_TABLE = {            # the header's sizes of the new entries, local to this file (abi_sizes.TABLE stays as it is)
    "df_cell_sort": abi_sizes.TABLE["df_cell_sort"],
    "df_map_keys": abi_sizes._e("map count sweep sweep_count mask gate pose B cap N voxel W cand key vz",
                                map=_i("24 * B * cap"), count=_i("4 * B"), sweep=_i("12 * B * N"), sweep_count=_i("4 * B"),
                                mask=_i("4 * B * N", True), gate=_i("4 * B", True), pose=_i("128 * B"),
                                cand=_o("24 * B * (cap + N)"), key=_o(_ROWS), vz=_o(_ROWS)),
    "df_map_select": abi_sizes._e("key idx_sorted cell_rng vz B n W max_per_voxel keep",
                                  key=_i("4 * B * n"), idx_sorted=_i("4 * B * n"), cell_rng=_i(_RNG), vz=_i("4 * B * n"),
                                  keep=_o("4 * B * n")),
    "df_map_compact": abi_sizes._e("cand idx_sorted cell_rng keep B cap N W map_out count_out stat ws",
                                   cand=_i("24 * B * (cap + N)"), idx_sorted=_i(_ROWS), cell_rng=_i(_RNG), keep=_i(_ROWS),
                                   map_out=_o("24 * B * cap"), count_out=_o("4 * B"), stat=_o("16 * B"),
                                   ws=abi_sizes.ws("df_map_ws_bytes", "B, cap, N")),
    "df_map_view": abi_sizes._e("map count pose B cap dst", map=_i("24 * B * cap"), count=_i("4 * B"), pose=_i("128 * B"),
                                dst=_o("12 * B * cap")),
}
NEW = ("df_map_keys", "df_map_select", "df_map_compact", "df_map_view")


def test_guarded_map_entries_write_nothing_outside_their_buffers(dev, monkeypatch):
    from deflow_amd import _lib, args, localmap
    protos = abi_sizes.header_prototypes()
    for name in NEW:                                                   # the local table against the header's prototypes
        assert [p.name for p in protos[name]][:-1] == list(MAP_TABLE[name].params) and protos[name][-1].name == "stream"
        for p in protos[name][:-1]:
            assert p.pointer == (p.name in MAP_TABLE[name].bufs) and (not p.pointer or p.nullable == MAP_TABLE[name].bufs[p.name].nullable)
            assert not p.pointer or p.const == (MAP_TABLE[name].bufs[p.name].role == abi_sizes.IN)
        assert len(_lib._SIGS[name]) == len(protos[name])
        for t, p in zip(_lib._SIGS[name], protos[name]):
            assert (t is _lib.P) == p.pointer, (name, p.name)
    assert [p.name for p in protos["df_map_ws_bytes"]] == ["B", "cap", "N"]
    names = list(_lib._SIGS)
    assert names[-5:] == ["df_map_ws_bytes", *NEW] and names[-6] == "df_reg_accumulate_plane"
    pts, counts, sweep, sc, pose, mask = keys_batch()
    dsweep, dsc, dpose, dmask = torch.from_numpy(sweep).to(dev), i32(dev, sc), torch.from_numpy(pose).to(dev), torch.from_numpy(mask).to(dev)

    def scenario():
        m = new_map(dev, 3, 2)
        load(m, pts, counts)
        m.insert(dsweep, dsc, dpose, mask=dmask)
        m.insert(dsweep.flip(1).contiguous(), dsc, dpose, gate=i32(dev, [0, 2, 0]))
        dst, c = m.view(dpose)
        return [m.points, m.count, m.stat, dst, *m.last.values()]

    outs = [scenario()]
    for fill in (0xA5, 0x7F):
        with monkeypatch.context() as mp:
            g = guarded.Guard(fill, _lib.call, table=MAP_TABLE)
            for mod in (localmap, args):
                mp.setattr(mod, "call", g.call)
                mp.setattr(mod, "ptr", g.ptr)
            outs.append(scenario())
        assert g.seen == ["df_map_keys", "df_cell_sort", "df_map_select", "df_map_compact"] * 2 + ["df_map_view"]
    total = int(outs[0][2][:, 0].sum())                                # idx_sorted is written up to the rows in the window only
    for k, (a, b, c) in enumerate(zip(*outs)):
        if k == 7:
            a, b, c = a[:total], b[:total], c[:total]
        assert guarded.same_bits(a, b) and guarded.same_bits(a, c), k


def test_map_argument_errors(dev):
    from deflow_amd.localmap import LocalMap
    from deflow_amd.odometry import register_sweeps
    with pytest.raises(TypeError, match="LocalMap: device must be a CUDA device"):
        LocalMap(1, 8, voxel=0.5, max_per_voxel=1, max_range=5.0, device="cpu")
    with pytest.raises(ValueError, match="LocalMap: max_per_voxel must be an integer"):
        LocalMap(1, 8, voxel=0.5, max_per_voxel=0, max_range=5.0, device=dev)
    with pytest.raises(ValueError, match="LocalMap: voxel must be positive"):
        LocalMap(1, 8, voxel=0.0, max_per_voxel=1, max_range=5.0, device=dev)
    with pytest.raises(ValueError, match="window of"):
        LocalMap(1, 8, voxel=0.01, max_per_voxel=1, max_range=51.2, device=dev)
    m = new_map(dev, 2, 1)
    x, c, p = torch.zeros(2, 5, 3, device=dev), i32(dev, [5, 5]), torch.eye(4, dtype=torch.float64, device=dev).repeat(2, 1, 1)
    with pytest.raises(TypeError, match="LocalMap.insert: points must be a CUDA tensor"):
        m.insert(x.cpu(), c, p)
    with pytest.raises(ValueError, match="LocalMap.insert: pose must be torch.float64"):
        m.insert(x, c, p.float())
    with pytest.raises(ValueError, match="LocalMap.insert: points must hold 2 samples"):
        m.insert(x[:1], c[:1], p[:1])
    with pytest.raises(ValueError, match="LocalMap.insert: gate must be torch.int32"):
        m.insert(x, c, p, gate=c.long())
    with pytest.raises(ValueError, match="register_sweeps: target must be 'scan' or 'map', got 'x'"):
        register_sweeps([np.zeros((4, 3))], device=dev, target="x")
    with pytest.raises(ValueError, match="register_sweeps: map_max_per_voxel must be an integer"):
        register_sweeps([np.zeros((4, 3))], device=dev, target="map", map_max_per_voxel=0)


# ---- end to end: the loop scene ---------------------------------------------------------------------------------------------------------
LOOP = dict(stride=1, levels=map_ref.LOOP["levels"], min_range=0.0, max_range=map_ref.LOOP["max_range"], map_voxel=map_ref.LOOP["voxel"],
            map_capacity=4096)


def dist(P, Q):
    return float(np.abs(np.asarray(P) - np.asarray(Q)).max())


@pytest.fixture(scope="module")
def loop():
    sweeps, truth = map_ref.loop_scene(map_ref.LOOP_SEED, nodes=map_ref.LOOP_NODES)
    ref = map_ref.register_sweeps_map(sweeps, map_ref.LOOP["levels"], voxel=map_ref.LOOP["voxel"], K=1, cap=4096, W=map_ref.LOOP_W)
    return sweeps, truth, ref


def test_loop_scene_against_the_restatement_and_the_truth(dev, loop):
    from deflow_amd.odometry import chain_poses, register_sweeps
    sweeps, truth, ref = loop
    rep = {}
    rel = register_sweeps(sweeps, None, device=dev, report=rep, target="map", map_max_per_voxel=1, **LOOP)
    poses = chain_poses(rel)
    assert rep["failed"] == [] and rep["params"]["target"] == "map" and rep["params"]["map_voxel"] == 0.5
    assert rep["params"]["map_max_per_voxel"] == 1 and rep["params"]["map_capacity"] == 4096
    assert rep["map_count"] == [m[1] for m in ref["maps"]] and rep["map_overflow"] == [0] * len(sweeps)
    worst = max(dist(P, Q) for P, Q in zip(poses, ref["poses"]))
    print("K 1: |pose - restatement|max", worst, "closing pose off the truth by", dist(poses[-1], truth[-1]))
    assert worst <= TOL and dist(poses[-1], truth[-1]) <= TOL
    scan = chain_poses(register_sweeps(sweeps, None, device=dev, target="scan", **{k: v for k, v in LOOP.items() if not k.startswith("map_")}))
    print("scan: closing pose off the truth by", dist(scan[-1], truth[-1]))
    assert dist(scan[-1], truth[-1]) > TOL


@pytest.mark.parametrize("K,stride", [(2, 1), (4, 1), (4, 3)])
def test_loop_scene_closes_at_other_k_and_stride(dev, loop, K, stride):
    from deflow_amd.odometry import chain_poses, register_sweeps
    sweeps, truth, _ = loop
    rep = {}
    poses = chain_poses(register_sweeps(sweeps, None, device=dev, report=rep, target="map", map_max_per_voxel=K, **{**LOOP, "stride": stride}))
    print("K", K, "stride", stride, "closing pose off the truth by", dist(poses[-1], truth[-1]), "map rows", rep["map_count"][-1])
    assert rep["failed"] == [] and dist(poses[-1], truth[-1]) <= TOL


def test_failed_registration_inserts_nothing(dev, loop):
    from deflow_amd.localmap import LocalMap
    from deflow_amd.odometry import register, register_sweeps
    sweeps = loop[0][:2]
    t = [torch.from_numpy(s).to(dev)[None] for s in sweeps]
    c = [i32(dev, [len(s)]) for s in sweeps]
    eye = torch.eye(4, dtype=torch.float64, device=dev)[None]
    m = LocalMap(1, 4096, voxel=0.5, max_per_voxel=4, max_range=51.2, device=dev)
    m.insert(t[0], c[0], eye)
    before = (m.points.clone(), m.count.clone())
    dst, cd = m.view(eye)
    T, info = register(t[1], c[1], dst, cd, stride=1, levels=map_ref.LOOP["levels"], min_inliers=10 ** 6)
    assert info["status"].tolist() == [2] and guarded.same_bits(T, eye)
    m.insert(t[1], c[1], T, gate=info["status"])
    assert guarded.same_bits(m.points, before[0]) and guarded.same_bits(m.count, before[1]) and int(m.count) == len(sweeps[0])
    assert m.stat.tolist() == [[len(sweeps[0]), len(sweeps[0]), 0, 0]]
    m.insert(t[1], c[1], T, gate=i32(dev, [0]))                       # the same call with the gate open does insert
    assert int(m.count) > len(sweeps[0])
    rep = {}
    rel = register_sweeps(sweeps, None, device=dev, report=rep, target="map", **{**LOOP, "min_inliers": 10 ** 6})
    assert rep["failed"] == [{"pair": 0, "status": 2}] and rep["map_count"] == [len(sweeps[0])] * 2 and np.array_equal(rel[0], np.eye(4))


def test_plane_residual_closes_on_the_planar_scene(dev):
    """plane_ref's planar scene out and back -- the planes seen from I, A, B, A, I at positions fixed in the sensor's frame, the closing
    sweep a row-permuted copy of sweep 0: the normals are the map's"""
    import plane_ref
    from deflow_amd.odometry import chain_poses, register_sweeps
    A = reg_ref.se3_exp(plane_ref.MOTION)
    Bm = reg_ref.se3_exp((0.0, 0.0, 0.025, 0.22, -0.10, 0.04)) @ A
    moves = (np.eye(4), A, Bm, A, np.eye(4))
    sweeps = plane_ref.planar_sweeps(moves)
    sweeps[-1] = sweeps[-1][np.random.default_rng(5).permutation(len(sweeps[-1]))]
    rep = {}
    rel = register_sweeps(sweeps, None, device=dev, report=rep, target="map", map_voxel=0.5, map_max_per_voxel=4, map_capacity=4096,
                          stride=1, min_range=0.0, max_range=24.0, init="identity", xy_range=plane_ref.RANGE, cell=plane_ref.CELL,
                          residual="plane", normal_radius=plane_ref.RADIUS, normal_min_pts=plane_ref.MIN_PTS,
                          normal_max_curv=plane_ref.MAX_CURV)
    poses = chain_poses(rel)
    errs = [dist(P, np.linalg.inv(T)) for P, T in zip(poses, moves)]
    print("plane: |pose - truth|max per sweep", errs, "map rows", rep["map_count"], "inliers", rep["inliers"])
    assert rep["failed"] == [] and rep["params"]["residual"] == "plane" and errs[-1] <= TOL


# ---- the command ------------------------------------------------------------------------------------------------------------------------
def test_command_records_the_target(dev, tmp_path, golden_dir, capsys):
    from deflow_amd import odometry
    src = os.path.join(golden_dir, "av2_mini", "train")
    shutil.copy(os.path.join(src, "scene_a.h5"), tmp_path / "scene_a.h5")
    with open(os.path.join(src, "index_total.pkl"), "rb") as f:
        index = [e for e in pickle.load(f) if e[0] == "scene_a"]
    with open(tmp_path / "index_total.pkl", "wb") as f:
        pickle.dump(index, f)
    assert odometry.main([f"data_dir={tmp_path}", "min_inliers=5", "stride=1", "iters=2", "target=map", "map_voxel=0.25",
                          "map_max_per_voxel=2", "map_capacity=65536"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["scene"] == "scene_a" and line["sweeps"] == 25
    poses = odometry.read_sidecar(str(tmp_path / "scene_a.pose.npz"))
    assert len(poses) == 25
    for P in poses.values():
        assert P.shape == (4, 4) and P.dtype == np.float64 and np.isfinite(P).all()
        assert np.abs(P[:3, :3] @ P[:3, :3].T - np.eye(3)).max() <= 1e-6
    with np.load(tmp_path / "scene_a.pose.npz", allow_pickle=False) as z:
        meta = json.loads(str(z["meta"]))
    assert (meta["target"], meta["map_voxel"], meta["map_max_per_voxel"], meta["map_capacity"]) == ("map", 0.25, 2, 65536)
    assert "6t" in meta["definition"]
