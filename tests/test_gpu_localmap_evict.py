"""GPU: nearest-first eviction of the local map (UNPINNED) -- df_map_compact_near, ``LocalMap(evict="near")``,
``odometry.register_sweeps(map_evict="near")`` and the command -- against the integer restatement of tests/helpers/map_evict_ref.py,
whose own conditions tests/test_localmap_evict_cpu.py checks without a GPU.

Shapes: section 6t's -- cap = 700 map rows (300 in the R = 0 case), N = 600 or 640 sweep rows, so n <= 1340 candidates are six blocks of
256, the last one partial; B <= 3; W = 8 (17 x 17 columns, rings 0 .. 8); voxel 0.3.  One case runs W = 300 (601 x 601 columns) at
B = 1: the ring scan beyond one 256-wide pass.  Wherever a map is compared, map_out's bits, count_out, stat and cut are EQUAL to the
restatement's.  The hand-made states put every row at the centre of a chosen window column, all in one z voxel with K = 10^6, so that
every row is kept and the ring counts are the test's own.

The loop scene under overflow (map_evict_ref.EVICT_SEED, EVICT_CAP: seed 3, capacity 450, every one of the 17 updates overflows): the
GPU's poses are held to the float64 restatement's within 1e-4, section 6r's and 6t's bound, which is sound because the reference's
nearest / second-nearest margin is 1.27e-4 m there (tests/test_localmap_evict_cpu.py).  No accuracy is claimed for nearest-first: on the
reference the closing pose is off the truth by 3.2e-4 with it and by 1.2e-4 with the sorted-order cut.

Measured on an MI355X: every pose within 3.9e-8 of the restatement's; closing pose off the truth by 3.248e-4 with map_evict="near" and
1.231e-4 with "order", the float64 reference's own figures; map_count, map_overflow and map_cut equal to the reference's at every sweep."""
import json
import math
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
import map_evict_ref  # noqa: E402
import map_ref  # noqa: E402
import reg_ref  # noqa: E402
import vis_ref  # noqa: E402

pytestmark = pytest.mark.gpu

CAP, N, W, VOXEL = 700, 600, 8, 0.3
MAX_RANGE = 2.0                      # ceil(2.0 / 0.3) + 1 = 8
ALL = 10 ** 6                        # a K no voxel reaches: every row in the window is kept
TOL = 1e-4                           # section 6r's bound: the per-row fp32 roundings carried through a well-conditioned fit


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def i32(dev, v):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def f64bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def new_map(dev, B, K, cap=CAP, evict="near", voxel=VOXEL, max_range=MAX_RANGE, w=W):
    from deflow_amd.localmap import LocalMap
    m = LocalMap(B, cap, voxel=voxel, max_per_voxel=K, max_range=max_range, device=dev, evict=evict)
    assert m.W == w and m.S == 2 * w + 1
    return m


def load(m, pts, counts):
    m.points = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(m.dev)
    m.count = i32(m.dev, counts)


def check_insert(m, state, sweep, sweep_count, pose, K, mask=None, gate=None):
    """one LocalMap(evict="near").insert from ``state`` = (map [B,cap,3], counts) against the restatement: keep, then map, count, stat and
    cut bit for bit -> (map, counts, per sample dict(order=kept candidates in sorted order, ring=their rings, cut=...))"""
    pts, counts = state
    B, cap = pts.shape[0], pts.shape[1]
    load(m, pts, counts)
    dev = m.dev
    m.insert(torch.from_numpy(sweep).to(dev), i32(dev, sweep_count), torch.from_numpy(pose).to(dev),
             mask=None if mask is None else torch.from_numpy(mask).to(dev), gate=None if gate is None else i32(dev, gate))
    n, S = cap + sweep.shape[1], 2 * m.W + 1
    keep_g, got, cnt_g, stat_g, cut_g = (t.cpu().numpy() for t in (m.last["keep"], m.points, m.count, m.stat, m.cut))
    assert m.last["cut"] is m.cut and cut_g.shape == (B, 2) and cut_g.dtype == np.int32
    info = []
    for b in range(B):
        cand, key, vz = map_ref.keys(pts[b], counts[b], sweep[b], sweep_count[b], None if mask is None else mask[b],
                                     None if gate is None else gate[b], pose[b], m.voxel, m.W, b, B)
        drop = B * S * S
        keep = map_ref.select(key, vz, drop, K)
        assert np.array_equal(keep_g.reshape(B, n)[b], keep), b
        want, cnt, stat, cut = map_evict_ref.compact_near(cand, key, keep, drop, cap, m.W, b)
        assert np.array_equal(f64bits(got[b]), f64bits(want)), b
        assert int(cnt_g[b]) == cnt and tuple(stat_g[b].tolist()) == stat and tuple(cut_g[b].tolist()) == cut, \
            (b, int(cnt_g[b]), stat_g[b].tolist(), cut_g[b].tolist(), cnt, stat, cut)
        assert (f64bits(got[b, cnt:]) == 0x7FF8000000000000).all()
        order = [int(c) for c in map_ref.sorted_order(key, drop) if keep[c]]
        info.append(dict(order=order, ring=[map_evict_ref.ring_of(key[c], m.W, b) for c in order], cut=cut, cand=cand))
    return got, cnt_g, info


# ---- hand-made states: every row at the centre of a chosen column -----------------------------------------------------------------------
def rows_at(cols, dz=1e-4, voxel=VOXEL):
    """float64 rows at the centres of the window columns (ox, oy) about the anchor column of the identity pose, z distinct"""
    cols = np.asarray(cols, dtype=np.float64).reshape(-1, 2)
    p = np.empty((len(cols), 3))
    p[:, :2] = (cols + 0.5) * voxel
    p[:, 2] = 0.01 + dz * np.arange(len(cols))
    return p


def crafted(cols, count, cap=CAP, n_sweep=N, dz=1e-4, voxel=VOXEL):
    """B = 1: the first ``count`` columns' rows are the map's state, the others the sweep's (rows past them do not take part)"""
    p = rows_at(cols, dz, voxel)
    pts = np.full((1, cap, 3), np.nan)
    pts[0, :count] = p[:count]
    sweep = np.full((1, n_sweep, 3), np.nan, dtype=np.float32)
    sweep[0, :len(p) - count] = p[count:]
    assert len(p) - count <= n_sweep and count <= cap
    return (pts, [count]), sweep, [len(p) - count], np.eye(4)[None].copy()


def ring_cols(rng, ring, size):
    """``size`` random columns of the ring, as offsets from the anchor column"""
    side = np.arange(-ring, ring + 1)
    border = np.array([(x, y) for x in side for y in side if max(abs(x), abs(y)) == ring])
    return border[rng.integers(0, len(border), size=size)]


def shuffled(rng, *parts):
    cols = np.concatenate(parts)
    return cols[rng.permutation(len(cols))]


def run_crafted(dev, cols, count, K=ALL, **kw):
    state, sweep, sc, pose = crafted(cols, count, **kw)
    m = new_map(dev, 1, K, cap=state[0].shape[1])
    got, cnt, info = check_insert(m, state, sweep, sc, pose, K)
    return m, got[0], int(cnt[0]), info[0]


# ---- the entry on its own ---------------------------------------------------------------------------------------------------------------
def stage_call(m, near, fill=None, B=None):
    """df_map_compact_near (or df_map_compact) on the stage tensors of m's last insert, into buffers of the test's own"""
    from deflow_amd._lib import call, ptr, stream
    B, cap, dev, L = m.B, m.capacity, m.dev, m.last
    n_sweep = L["cand"].shape[1] - cap
    out = torch.empty(B, cap, 3, dtype=torch.float64, device=dev)
    cnt, stat, cut = (torch.empty(s, dtype=torch.int32, device=dev) for s in ((B,), (B, 4), (B, 2)))
    q = ("df_map_near_ws_bytes", (B, cap, n_sweep, m.W)) if near else ("df_map_ws_bytes", (B, cap, n_sweep))
    ws = torch.empty(call(q[0], *q[1]) // 4, dtype=torch.int32, device=dev)
    if fill is not None:
        for t in (out, cnt, stat, cut, ws):
            t.view(torch.uint8).fill_(fill)
    if near:
        call("df_map_compact_near", ptr(L["cand"]), ptr(L["key"]), ptr(L["idx_sorted"]), ptr(L["cell_rng"]), ptr(L["keep"]), B, cap, n_sweep,
             m.W, ptr(out), ptr(cnt), ptr(stat), ptr(cut), ptr(ws), stream())
        return out, cnt, stat, cut
    call("df_map_compact", ptr(L["cand"]), ptr(L["idx_sorted"]), ptr(L["cell_rng"]), ptr(L["keep"]), B, cap, n_sweep, m.W, ptr(out), ptr(cnt),
         ptr(stat), ptr(ws), stream())
    return out, cnt, stat


def random_batch(seed=3):
    rng = np.random.default_rng(seed)
    pose = np.stack((reg_ref.se3_exp((0.0, 0.2, 0.7, 0.0, 0.0, 0.0)), np.eye(4), reg_ref.se3_exp((0.01, -0.02, 0.3, 1.0, -2.0, 0.1))))
    pose[0, :3, 3], pose[1, :3, 3] = (212.3, -211.9, 1.7), (-5.1, -7.3, 0.0)
    sweep = rng.uniform(-3.0, 3.0, size=(3, N, 3)).astype(np.float32)
    sweep[0, 5], sweep[0, 6, 1] = np.nan, np.inf
    mask = np.ones((3, N), dtype=np.int32)
    mask[1, ::7] = 0
    pts = pose[:, None, :3, 3] + rng.uniform(-2.9, 2.9, size=(3, CAP, 3))
    return pts, sweep, pose, mask


def test_without_overflow_it_is_df_map_compact(dev):
    pts, sweep, pose, mask = random_batch()
    m = new_map(dev, 3, 1)
    _, cnt, info = check_insert(m, (pts, [60, 0, 25]), sweep, [N, N - 20, N], pose, 1, mask)
    assert all(50 < c < CAP for c in cnt) and [i["cut"] for i in info] == [(W + 1, 0)] * 3 and m.stat[:, 3].tolist() == [0, 0, 0]
    a, b = stage_call(m, True, 0xA5), stage_call(m, False, 0x7F)
    assert all(guarded.same_bits(x, y) for x, y in zip(a[:3], b)) and a[3].tolist() == [[W + 1, 0]] * 3
    assert guarded.same_bits(a[0], m.points) and guarded.same_bits(a[1], m.count) and guarded.same_bits(a[2], m.stat)


@pytest.mark.parametrize("extra", [0, 1])
def test_kept_equal_to_the_capacity_and_one_more(dev, extra):
    rng = np.random.default_rng(7)
    cols = rng.integers(-W, W + 1, size=(CAP + extra, 2))
    cols[cols[:, 1] == W, 1] = W - 1                                   # the last occupied row of columns, dy = W - 1, holds rows of ring 7 only:
    cols[cols[:, 1] == W - 1, 0] //= 2                                 # the end of the sorted order is not what nearest-first loses
    m, got, cnt, info = run_crafted(dev, cols, 100 + extra, n_sweep=N)
    assert cnt == CAP and m.stat[0].tolist() == [CAP + extra, CAP + extra, N, extra]
    if not extra:
        assert info["cut"] == (W + 1, 0)
        return
    outer = max(info["ring"])
    gone = [c for c, r in zip(info["order"], info["ring"]) if r == outer][-1]    # the last row of the outermost occupied ring
    assert info["cut"] == (outer, info["ring"].count(outer) - 1) and info["ring"].count(outer) > 20
    assert np.array_equal(f64bits(got), f64bits(info["cand"][[c for c in info["order"] if c != gone]]))
    assert info["order"].index(gone) < CAP                             # not the row the sorted-order cut would lose
    assert not guarded.same_bits(stage_call(m, False)[0], m.points)


def test_inner_rings_sum_to_the_capacity(dev):
    rng = np.random.default_rng(8)
    inner = np.concatenate([ring_cols(rng, r, s) for r, s in ((0, 40), (1, 160), (2, 200), (3, 300))])
    m, got, cnt, info = run_crafted(dev, shuffled(rng, inner, ring_cols(rng, 5, 50)), 150)
    assert info["cut"] == (5, 0) and cnt == CAP and m.stat[0].tolist() == [750, 750, 600, 50]   # ring 4 is empty: R is the LARGEST that fits
    assert np.array_equal(f64bits(got), f64bits(info["cand"][[c for c, r in zip(info["order"], info["ring"]) if r < 5]]))


def test_anchor_column_alone_overflows(dev):
    m, got, cnt, info = run_crafted(dev, np.zeros((640, 2)), 0, cap=300, n_sweep=640, dz=0.002)      # z voxels 0 .. 4
    assert info["cut"] == (0, 300) and cnt == 300 and m.stat[0].tolist() == [640, 640, 640, 340]
    assert info["order"][:300] == list(range(300, 600))                # candidates: the map's 300 rows first, then the sweep's
    assert np.array_equal(f64bits(got), f64bits(info["cand"][300:600]))
    vz = m.last["vz"].cpu().numpy()[300:]
    assert sorted(set(vz.tolist())) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("budget", [255, 256, 257])
def test_budget_either_side_of_a_block_boundary(dev, budget):
    """ring 4's rows lie in the window's row dy = -4, before every inner row in sorted order: the cut inside the partial ring falls at the
    sorted positions 255, 256, 257"""
    rng = np.random.default_rng(budget)
    inner = np.concatenate([ring_cols(rng, r, s) for r, s in ((0, 45), (1, 150), (2, CAP - budget - 195))])
    part = np.stack((rng.integers(-4, 5, size=300), np.full(300, -4)), axis=1)
    m, got, cnt, info = run_crafted(dev, shuffled(rng, inner, part), 145)
    assert info["cut"] == (4, budget) and info["ring"][:300] == [4] * 300 and max(info["ring"][300:]) == 2
    keep_rows = info["order"][:budget] + info["order"][300:]
    assert cnt == CAP and np.array_equal(f64bits(got), f64bits(info["cand"][keep_rows]))


def test_partial_ring_interleaved_with_inner_and_outer_rows(dev):
    rng = np.random.default_rng(9)
    cols = rng.integers(-W, W + 1, size=(CAP + N, 2))                  # 1300 rows over the whole window, all kept
    m, got, cnt, info = run_crafted(dev, cols, CAP)
    R, budget = info["cut"]
    ring = np.array(info["ring"])
    at = np.flatnonzero(ring == R)
    between = ring[at[0]:at[-1] + 1]
    assert 2 <= R <= 6 and 0 < budget < len(at) and (between < R).sum() > 100 and (between > R).sum() > 100      # all three kinds
    assert len(set(np.array(info["order"])[at] // 1)) == len(at) and m.stat[0].tolist() == [CAP + N, CAP + N, N, N]
    cut_pos = at[budget]                                               # the first partial row that goes
    assert (ring[:cut_pos] > R).any() and (ring[cut_pos:] < R).any()   # rows of outer rings before the cut, inner ones after it
    survivors = [c for k, (c, r) in enumerate(zip(info["order"], info["ring"])) if r < R or (r == R and k < cut_pos)]
    assert np.array_equal(f64bits(got), f64bits(info["cand"][survivors]))


def three_cuts():
    """sample 0: no overflow; sample 1: the anchor column holds the whole map and the sweep (R = 0); sample 2: R in the middle"""
    rng = np.random.default_rng(10)
    pts = np.full((3, CAP, 3), np.nan)
    sweep = np.full((3, N, 3), np.nan, dtype=np.float32)
    pts[0, :80], sweep[0, :500] = rows_at(rng.integers(-W, W + 1, size=(80, 2))), rows_at(rng.integers(-W, W + 1, size=(500, 2)))
    pts[1], sweep[1] = rows_at(np.zeros((CAP, 2)), 1e-4), rows_at(np.zeros((N, 2)), 1e-4) + (0.0, 0.0, 0.1)
    pts[2], sweep[2] = rows_at(rng.integers(-W, W + 1, size=(CAP, 2))), rows_at(rng.integers(-W, W + 1, size=(N, 2))) + (0.0, 0.0, 0.1)
    return pts, [80, CAP, CAP], sweep, [500, N, N], np.stack((np.eye(4),) * 3)


def test_three_samples_with_three_different_cuts(dev):
    pts, counts, sweep, sc, pose = three_cuts()
    m = new_map(dev, 3, ALL)
    got, cnt, info = check_insert(m, (pts, counts), sweep, sc, pose, ALL)
    cuts = [i["cut"] for i in info]
    assert cuts[0] == (W + 1, 0) and cuts[1] == (0, CAP) and 2 <= cuts[2][0] <= 6 and cnt.tolist() == [580, CAP, CAP]
    assert np.array_equal(f64bits(got[1]), f64bits(pts[1]))            # R = 0: the map's own rows, the oldest of the column
    batch = (m.points.clone(), m.count.clone(), m.stat.clone(), m.cut.clone())
    # B = 1 against sample 0 of B = 3
    for b in range(3):
        one = new_map(dev, 1, ALL)
        check_insert(one, (pts[b:b + 1], counts[b:b + 1]), sweep[b:b + 1], sc[b:b + 1], pose[b:b + 1], ALL)
        assert all(guarded.same_bits(x, y[b:b + 1]) for x, y in zip((one.points, one.count, one.stat, one.cut), batch)), b
    # a sample with count 0 and an empty sweep; gate = 2 on the sample whose sweep made it overflow
    got, cnt, info = check_insert(m, (pts, [0, CAP, CAP]), sweep, [0, N, N], pose, ALL, gate=[0, 2, 0])
    assert cnt.tolist() == [0, CAP, CAP] and m.stat[:2].tolist() == [[0, 0, 0, 0], [CAP, CAP, 0, 0]]
    assert [i["cut"] for i in info] == [(W + 1, 0), (W + 1, 0), cuts[2]] and (f64bits(got[0]) == 0x7FF8000000000000).all()
    assert guarded.same_bits(m.points[2], batch[0][2]) and np.array_equal(f64bits(got[1]), f64bits(pts[1]))


def test_ring_scan_beyond_one_pass_at_w_300(dev):
    from deflow_amd._lib import call
    voxel, max_range = 0.3, 89.7
    assert math.ceil(max_range / voxel) + 1 == 300                     # LocalMap's own formula
    rng = np.random.default_rng(11)
    parts = [ring_cols(rng, r, s) for r, s in ((0, 200), (255, 300), (256, 300), (257, 100), (300, 100))]
    state, sweep, sc, pose = crafted(shuffled(rng, *parts), 400)
    m = new_map(dev, 1, ALL, max_range=max_range, w=300)
    got, cnt, info = check_insert(m, state, sweep, sc, pose, ALL)
    assert info[0]["cut"] == (256, 200) and sorted(set(info[0]["ring"])) == [0, 255, 256, 257, 300] and int(cnt[0]) == CAP
    assert m.stat[0].tolist() == [1000, 1000, 600, 300]
    with pytest.raises(RuntimeError, match="df_map_compact_near failed: DF_E_SHAPE"):         # refused before anything is touched
        call("df_map_compact_near", 0x10000, 0x10000, 0x10000, 0x10000, 0x10000, 1, CAP, N, 2048, 0x20000, 0x10000, 0x10000, 0x10000,
             0x10000, 0)
    assert call("df_map_near_ws_bytes", 1, CAP, N, 2048) == -1


def test_repeated_calls_are_bit_identical_over_garbage(dev):
    pts, counts, sweep, sc, pose = three_cuts()
    m = new_map(dev, 3, ALL)
    load(m, pts, counts)
    m.insert(torch.from_numpy(sweep).to(dev), i32(dev, sc), torch.from_numpy(pose).to(dev))
    want = (m.points, m.count, m.stat, m.cut)
    for fill in (None, 0xA5, 0x7F):
        got = stage_call(m, True, fill)
        assert all(guarded.same_bits(x, y) for x, y in zip(got, want)), fill


# ---- the guarded-call harness -----------------------------------------------------------------------------------------------------------
_i, _o = abi_sizes.i, abi_sizes.o
_ROWS = "4 * B * (cap + N)"
_RNG = "8 * B * (2 * W + 1) * (2 * W + 1)"
NEAR_TABLE = {           # the header's sizes of the entries of an update under evict="near", local to this file (abi_sizes.TABLE stays as it is)
    "df_cell_sort": abi_sizes.TABLE["df_cell_sort"],
    "df_map_keys": abi_sizes._e("map count sweep sweep_count mask gate pose B cap N voxel W cand key vz",
                                map=_i("24 * B * cap"), count=_i("4 * B"), sweep=_i("12 * B * N"), sweep_count=_i("4 * B"),
                                mask=_i("4 * B * N", True), gate=_i("4 * B", True), pose=_i("128 * B"),
                                cand=_o("24 * B * (cap + N)"), key=_o(_ROWS), vz=_o(_ROWS)),
    "df_map_select": abi_sizes._e("key idx_sorted cell_rng vz B n W max_per_voxel keep",
                                  key=_i("4 * B * n"), idx_sorted=_i("4 * B * n"), cell_rng=_i(_RNG), vz=_i("4 * B * n"),
                                  keep=_o("4 * B * n")),
    "df_map_compact_near": abi_sizes._e("cand key idx_sorted cell_rng keep B cap N W map_out count_out stat cut ws",
                                        cand=_i("24 * B * (cap + N)"), key=_i(_ROWS), idx_sorted=_i(_ROWS), cell_rng=_i(_RNG),
                                        keep=_i(_ROWS), map_out=_o("24 * B * cap"), count_out=_o("4 * B"), stat=_o("16 * B"),
                                        cut=_o("8 * B"), ws=abi_sizes.ws("df_map_near_ws_bytes", "B, cap, N, W")),
}


def test_guarded_near_update_writes_nothing_outside_its_buffers(dev, monkeypatch):
    from deflow_amd import _lib, args, localmap
    protos = abi_sizes.header_prototypes()
    name, entry = "df_map_compact_near", NEAR_TABLE["df_map_compact_near"]             # the local table against the header's prototype
    assert [p.name for p in protos[name]][:-1] == list(entry.params) and protos[name][-1].name == "stream"
    for p in protos[name][:-1]:
        assert p.pointer == (p.name in entry.bufs) and (not p.pointer or p.nullable == entry.bufs[p.name].nullable)
        assert not p.pointer or p.const == (entry.bufs[p.name].role == abi_sizes.IN)
    assert len(_lib._SIGS[name]) == len(protos[name])
    for t, p in zip(_lib._SIGS[name], protos[name]):
        assert (t is _lib.P) == p.pointer, p.name
    assert [p.name for p in protos["df_map_near_ws_bytes"]] == ["B", "cap", "N", "W"]
    assert _lib.call("df_map_near_ws_bytes", 3, CAP, N, W) == 4 * 3 * (W + 1 + 4 * 6)   # the header's formula
    pts, counts, sweep, sc, pose = three_cuts()
    dsweep, dsc, dpose = torch.from_numpy(sweep).to(dev), i32(dev, sc), torch.from_numpy(pose).to(dev)

    def scenario():
        m = new_map(dev, 3, ALL)
        load(m, pts, counts)
        m.insert(dsweep, dsc, dpose)
        first = [m.points.clone(), m.count.clone(), m.stat.clone(), m.cut.clone()]
        m.insert(dsweep.flip(1).contiguous(), dsc, dpose, gate=i32(dev, [0, 2, 0]))
        return first + [m.points, m.count, m.stat, m.cut, m.last["keep"], m.last["key"]]

    outs = [scenario()]
    for fill in (0xA5, 0x7F):
        with monkeypatch.context() as mp:
            g = guarded.Guard(fill, _lib.call, table=NEAR_TABLE)
            for mod in (localmap, args):
                mp.setattr(mod, "call", g.call)
                mp.setattr(mod, "ptr", g.ptr)
            outs.append(scenario())
        assert g.seen == ["df_map_keys", "df_cell_sort", "df_map_select", "df_map_compact_near"] * 2
    for k, (a, b, c) in enumerate(zip(*outs)):
        assert guarded.same_bits(a, b) and guarded.same_bits(a, c), k
    assert outs[0][3].tolist()[1] == [0, CAP] and outs[0][7].tolist()[1] == [W + 1, 0]


def test_evict_argument_errors(dev):
    from deflow_amd._lib import call, ptr
    from deflow_amd.localmap import LocalMap
    from deflow_amd.odometry import register_sweeps
    with pytest.raises(ValueError, match="LocalMap: evict must be 'order' or 'near', got None"):
        LocalMap(1, 8, voxel=0.5, max_per_voxel=1, max_range=5.0, device=dev, evict=None)
    assert LocalMap(1, 8, voxel=0.5, max_per_voxel=1, max_range=5.0, device=dev).cut is None
    m = new_map(dev, 1, 1, cap=64)
    x, c, p = torch.zeros(1, 5, 3, device=dev), i32(dev, [5]), torch.eye(4, dtype=torch.float64, device=dev)[None]
    assert m.cut is None
    m.insert(x, c, p)
    assert m.cut.tolist() == [[W + 1, 0]]
    L, s = m.last, torch.cuda.current_stream().cuda_stream
    spare = torch.empty_like(m.points)
    with pytest.raises(RuntimeError, match="df_map_compact_near failed: DF_E_ARG"):            # map_out == cand
        call("df_map_compact_near", ptr(L["cand"]), ptr(L["key"]), ptr(L["idx_sorted"]), ptr(L["cell_rng"]), ptr(L["keep"]), 1, 64, 5, W,
             ptr(L["cand"]), ptr(c), ptr(m.stat), ptr(m.cut), ptr(L["keep"]), s)
    with pytest.raises(RuntimeError, match="df_map_compact_near failed: DF_E_ARG"):            # cut is not nullable
        call("df_map_compact_near", ptr(L["cand"]), ptr(L["key"]), ptr(L["idx_sorted"]), ptr(L["cell_rng"]), ptr(L["keep"]), 1, 64, 5, W,
             ptr(spare), ptr(c), ptr(m.stat), None, ptr(L["keep"]), s)
    with pytest.raises(ValueError, match="register_sweeps: map_evict must be 'order' or 'near', got 'x'"):
        register_sweeps([np.zeros((4, 3))], device=dev, target="map", map_evict="x")
    with pytest.raises(ValueError, match="map_evict='near' needs target='map'"):
        register_sweeps([np.zeros((4, 3))], device=dev, map_evict="near")


# ---- the loops ----------------------------------------------------------------------------------------------------------------------------
def moving_sweeps(steps=3):
    """sweeps of 600 random rows about a sensor that moves by about two voxels (0.6 m) a step along +x and +y: rows leave the window on the
    far side, new ones enter on the near side, and with K = 2 the map overflows from the second update on"""
    rng = np.random.default_rng(12)
    sweeps = rng.uniform(-2.6, 2.6, size=(steps, 1, N, 3)).astype(np.float32)
    sweeps[:, :, :, 2] = rng.uniform(0.0, 0.55, size=(steps, 1, N))                # two z voxels
    poses = np.stack([np.eye(4)] * steps)[:, None].copy()
    for k in range(steps):
        poses[k, 0, :3, 3] = (0.61 * k, 0.58 * k, 0.0)
    return sweeps, poses


def test_three_successive_inserts_under_near(dev):
    sweeps, poses = moving_sweeps()
    m = new_map(dev, 1, 2)
    state = (np.full((1, CAP, 3), np.nan), [0])
    seen = []
    for k in range(3):
        got, cnt, info = check_insert(m, state, sweeps[k], [N], poses[k], 2)
        state = (got, cnt.tolist())
        seen.append((info[0]["cut"], m.stat[0].tolist()))
    print("cuts and stats of the three updates", seen)
    assert seen[0][0] == (W + 1, 0) and all(c[0] <= W and s[3] > 0 for c, s in seen[1:])       # an evicted map is a valid input to the next
    assert seen[2][1][0] < CAP + N                                     # rows of the map left the window on the far side


def test_carve_between_two_inserts_under_near(dev):
    sweeps, poses = moving_sweeps()
    carve = dict(res=8, halo=1, margin=0.05, rel=0.02, near=0.3)
    m = new_map(dev, 1, 2)
    state = (np.full((1, CAP, 3), np.nan), [0])
    got, cnt, _ = check_insert(m, state, sweeps[0], [N], poses[0], 2)
    got, cnt, info = check_insert(m, (got, cnt.tolist()), sweeps[1], [N], poses[1], 2)
    assert info[0]["cut"][0] <= W
    far = (sweeps[2] * np.float32(1.9)).astype(np.float32)             # returns well behind the map's rows: many are seen through
    m.carve(torch.from_numpy(far).to(dev), i32(dev, [N]), torch.from_numpy(poses[2]).to(dev), **carve)
    want, c, stat, _ = vis_ref.carve(got[0], int(cnt[0]), far[0], N, poses[2, 0], mask=None, gate=None, **carve)
    assert np.array_equal(f64bits(m.points[0].cpu().numpy()), f64bits(want)) and int(m.count[0]) == c
    assert tuple(m.carve_stat[0].tolist()) == stat and stat[1] > 20 and m.cut is not None
    carved = (m.points.cpu().numpy(), m.count.tolist())
    _, _, info = check_insert(m, carved, sweeps[2], [N], poses[2], 2)
    print("carved", stat, "then cut", info[0]["cut"], "stat", m.stat[0].tolist())


LOOP = dict(stride=1, levels=map_ref.LOOP["levels"], min_range=0.0, max_range=map_ref.LOOP["max_range"], map_voxel=map_ref.LOOP["voxel"],
            map_capacity=map_evict_ref.EVICT_CAP, map_max_per_voxel=1, target="map")


def dist(P, Q):
    return float(np.abs(np.asarray(P) - np.asarray(Q)).max())


@pytest.fixture(scope="module")
def loop():
    sweeps, truth = map_ref.loop_scene(map_evict_ref.EVICT_SEED, nodes=map_ref.LOOP_NODES)
    ref = map_evict_ref.register_sweeps_map(sweeps, map_ref.LOOP["levels"], voxel=map_ref.LOOP["voxel"], K=1, cap=map_evict_ref.EVICT_CAP,
                                            W=map_ref.LOOP_W, evict="near")
    return sweeps, truth, ref


@pytest.fixture
def calls(monkeypatch):
    """the names of the library calls LocalMap makes, and the maps a run made"""
    from deflow_amd import localmap
    seen = dict(names=[], maps=[])
    real, init = localmap.call, localmap.LocalMap.__init__

    def spy_call(name, *a):
        seen["names"].append(name)
        return real(name, *a)

    def spy_init(self, *a, **k):
        init(self, *a, **k)
        seen["maps"].append(self)

    def spy_insert(self, *a, **k):
        insert(self, *a, **k)
        # (a copy of the rows: the map double-buffers, so the update after the next one writes into this buffer again)
        seen["inserts"].append(dict(self.last, points=self.points.clone(), count=self.count, stat=self.stat, cut=self.cut))

    insert = localmap.LocalMap.insert
    seen["inserts"] = []
    monkeypatch.setattr(localmap, "call", spy_call)
    monkeypatch.setattr(localmap.LocalMap, "__init__", spy_init)
    monkeypatch.setattr(localmap.LocalMap, "insert", spy_insert)
    return seen


def test_loop_scene_under_overflow_against_the_restatement(dev, loop, calls):
    from deflow_amd.odometry import chain_poses, register_sweeps
    sweeps, truth, ref = loop
    rep = {}
    poses = chain_poses(register_sweeps(sweeps, None, device=dev, report=rep, map_evict="near", **LOOP))
    assert rep["failed"] == [] and rep["params"]["map_evict"] == "near" and rep["params"]["map_capacity"] == map_evict_ref.EVICT_CAP
    assert rep["map_count"] == [m[1] for m in ref["maps"]] and rep["map_overflow"] == [m[2][3] for m in ref["maps"]]
    assert rep["map_cut"] == ref["cuts"] and min(rep["map_overflow"]) > 0 and len(rep["map_cut"]) == len(sweeps)
    assert calls["names"].count("df_map_compact_near") == len(sweeps) and "df_map_compact" not in calls["names"]
    cap, Wl = map_evict_ref.EVICT_CAP, map_ref.LOOP_W
    for k, st in enumerate(calls["inserts"]):                          # every update: the restatement on the GPU's own stage tensors
        cand, key, keep = st["cand"][0].cpu().numpy(), st["key"].cpu().numpy().astype(np.int64), st["keep"].cpu().numpy()
        want, cnt, stat, cut = map_evict_ref.compact_near(cand, key, keep, (2 * Wl + 1) ** 2, cap, Wl)
        assert np.array_equal(f64bits(st["points"][0].cpu().numpy()), f64bits(want)), k
        assert int(st["count"][0]) == cnt and tuple(st["stat"][0].tolist()) == stat and tuple(st["cut"][0].tolist()) == cut, k
    worst = max(dist(P, Q) for P, Q in zip(poses, ref["poses"]))
    mid = max(dist(P, T) for P, T in zip(poses[1:-1], truth[1:-1]))
    print("near: |pose - restatement|max", worst, "closing pose off the truth by", dist(poses[-1], truth[-1]), "(restatement:",
          dist(ref["poses"][-1], truth[-1]), ") intermediate", mid, "cuts", rep["map_cut"])
    assert worst <= TOL
    rep2 = {}
    order = chain_poses(register_sweeps(sweeps, None, device=dev, report=rep2, **LOOP))       # reported beside it; nothing is claimed
    print("order: closing pose off the truth by", dist(order[-1], truth[-1]), "overflow", rep2["map_overflow"])
    assert rep2["failed"] == [] and "map_cut" not in rep2 and min(rep2["map_overflow"]) > 0


def test_evict_order_is_the_call_without_the_key(dev, loop, calls):
    from deflow_amd.odometry import register_sweeps
    sweeps = loop[0][:5]
    a = register_sweeps(sweeps, None, device=dev, **LOOP)
    first = list(calls["names"])
    rep = {}
    b = register_sweeps(sweeps, None, device=dev, map_evict="order", report=rep, **LOOP)
    update = ["df_map_keys", "df_cell_sort", "df_map_select", "df_map_compact"]
    assert first == update + (["df_map_view"] + update) * 4 and calls["names"][len(first):] == first       # today's calls in today's order
    assert all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b)) and "map_cut" not in rep
    assert rep["params"]["map_evict"] == "order" and rep["map_overflow"][-1] > 0
    ma, mb = calls["maps"]
    assert ma.cut is None and mb.cut is None and ma.evict == mb.evict == "order" and "cut" not in mb.last
    assert guarded.same_bits(ma.points, mb.points) and guarded.same_bits(ma.count, mb.count) and guarded.same_bits(ma.stat, mb.stat)


# ---- the command ------------------------------------------------------------------------------------------------------------------------
def test_command_records_the_eviction(dev, tmp_path, golden_dir, capsys, monkeypatch):
    from deflow_amd import odometry
    src = os.path.join(golden_dir, "av2_mini", "train")
    shutil.copy(os.path.join(src, "scene_a.h5"), tmp_path / "scene_a.h5")
    with open(os.path.join(src, "index_total.pkl"), "rb") as f:
        index = [e for e in pickle.load(f) if e[0] == "scene_a"]
    with open(tmp_path / "index_total.pkl", "wb") as f:
        pickle.dump(index, f)
    reports, real = [], odometry.scene_poses

    def spy(*a, report=None, **k):
        out = real(*a, report=report, **k)
        reports.append(report)
        return out

    monkeypatch.setattr(odometry, "scene_poses", spy)
    with pytest.raises(SystemExit, match="map_evict=near needs target=map"):
        odometry.main([f"data_dir={tmp_path}", "map_evict=near", "target=scan"])
    assert not os.path.exists(tmp_path / "scene_a.pose.npz") and reports == []
    assert odometry.main([f"data_dir={tmp_path}", "min_inliers=5", "stride=1", "iters=2", "target=map", "map_voxel=0.25",
                          "map_max_per_voxel=2", "map_capacity=4096", "map_evict=near"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["scene"] == "scene_a" and line["sweeps"] == 25
    with np.load(tmp_path / "scene_a.pose.npz", allow_pickle=False) as z:
        meta = json.loads(str(z["meta"]))
    assert (meta["target"], meta["map_evict"], meta["map_capacity"]) == ("map", "near", 4096) and "6v" in meta["definition"]
    rep = reports[0]
    W_cmd = math.ceil(51.2 / 0.25) + 1
    assert len(rep["map_cut"]) == 25 and all(0 <= R <= W_cmd + 1 and b >= 0 for R, b in rep["map_cut"])
    assert [R <= W_cmd for R, _ in rep["map_cut"]] == [o > 0 for o in rep["map_overflow"]]      # a cut inside the window exactly on overflow
    print("map_cut", rep["map_cut"], "overflow", rep["map_overflow"])
