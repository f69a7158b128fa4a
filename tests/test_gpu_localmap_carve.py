"""GPU: carving seen-through rows out of the local map (UNPINNED) -- df_map_drop, ``localmap.LocalMap.carve`` and
``odometry.register_sweeps(target="map", map_carve=True)`` -- against the restatement of tests/helpers/vis_ref.py, whose own conditions
(no static row carved, at least half of the old block rows carved, flags stable under +-2e-5 m) tests/test_visibility_cpu.py checks
without a GPU.

Shapes: cap = 700 map rows (three blocks of 256, the last one partial) and 768 (exact), B <= 3.  The drop's map, count and stat, the
carve's view, bins and flags and the rows carved per sweep are EQUAL to the restatement; the poses are held to 1e-4, section 6t's
bound for fp32 rows through a well-conditioned fit.

Measured on an MI355X, the room scene of vis_ref: rows carved per later sweep 0, 15, 26, 25, 23, the float64 restatement's counts; every
pose within 1.1e-7 of the restatement's; largest pose error against the truth 1.84e-6 with the carve and 1.82e-6 without (restatement:
1.74e-6 and 1.72e-6) -- the carve does not change the accuracy on this scene, so nothing is asserted between the two."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi_sizes  # noqa: E402
import guarded  # noqa: E402
import map_ref  # noqa: E402
import plane_ref  # noqa: E402
import vis_ref  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = 700
TOL = 1e-4                           # section 6t's bound: the per-row fp32 roundings carried through a well-conditioned fit


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def i32(dev, v):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def f64bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---- df_map_drop ------------------------------------------------------------------------------------------------------------------------
def run_drop(dev, pts, counts, flag, gate=None):
    from deflow_amd._lib import call, ptr, stream
    B, cap = pts.shape[0], pts.shape[1]
    m, f, c = torch.from_numpy(pts).to(dev), torch.from_numpy(flag).to(dev), i32(dev, counts)
    g = None if gate is None else i32(dev, gate)
    out = torch.full((B, cap, 3), 123.0, dtype=torch.float64, device=dev)
    cnt, stat = torch.full((B,), -7, dtype=torch.int32, device=dev), torch.full((B, 2), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(call("df_map_drop_ws_bytes", B, cap) // 4, dtype=torch.int32, device=dev)
    call("df_map_drop", ptr(m), ptr(c), ptr(f), ptr(g), B, cap, ptr(out), ptr(cnt), ptr(stat), ptr(ws), stream())
    return out.cpu().numpy(), cnt.cpu().numpy(), stat.cpu().numpy()


def check_drop(dev, pts, counts, flag, gate=None):
    out, cnt, stat = run_drop(dev, pts, counts, flag, gate)
    for b in range(pts.shape[0]):
        want, c, s = vis_ref.drop(pts[b], counts[b], flag[b], None if gate is None else gate[b])
        assert np.array_equal(f64bits(out[b]), f64bits(want)), b
        assert int(cnt[b]) == c and tuple(stat[b].tolist()) == s, (b, cnt[b], stat[b], c, s)
    return out, cnt, stat


@pytest.mark.parametrize("cap", [700, 768])
def test_drop_equals_the_restatement_on_the_edge_cases(dev, cap):
    rng = np.random.default_rng(cap)
    pts = rng.normal(size=(3, cap, 3))                                 # finite rows behind the counts: they must not be read as rows
    flag = (rng.uniform(size=(3, cap)) < 0.3).astype(np.int32)
    flag[0, ::5] = -3                                                  # any value but 0 drops
    check_drop(dev, pts, [cap, 300, 0], flag)                          # count == cap, flags set beyond the count, count == 0
    out, cnt, stat = check_drop(dev, pts, [cap, 300, 0], flag, gate=[0, 2, 0])
    assert cnt[1] == 300 and stat[1].tolist() == [0, 0] and np.array_equal(f64bits(out[1, :300]), f64bits(pts[1, :300]))
    assert (f64bits(out[1, 300:]) == 0x7FF8000000000000).all() and (f64bits(out[2]) == 0x7FF8000000000000).all()
    none, every = np.zeros((3, cap), dtype=np.int32), np.ones((3, cap), dtype=np.int32)
    out, cnt, stat = check_drop(dev, pts, [cap, 513, 256], none)       # none of the rows dropped
    assert cnt.tolist() == [cap, 513, 256] and stat.tolist() == [[cap, 0], [513, 0], [256, 0]] and np.array_equal(f64bits(out[0]), f64bits(pts[0]))
    out, cnt, stat = check_drop(dev, pts, [cap, 513, 256], every)      # all of them
    assert cnt.tolist() == [0, 0, 0] and stat.tolist() == [[cap, cap], [513, 513], [256, 256]] and np.isnan(out).all()
    for r in (255, 256, 257):                                          # one row alone, at a block's edge
        flag = np.zeros((3, cap), dtype=np.int32)
        flag[:, r] = 1
        out, cnt, stat = check_drop(dev, pts, [cap, 257, 256], flag)
        assert cnt.tolist() == [cap - 1, 257 - (r < 257), 256 - (r < 256)]
        assert np.array_equal(f64bits(out[0, r:cap - 1]), f64bits(pts[0, r + 1:]))
    big = check_drop(dev, pts, [cap + 5, -3, 1], none)[1]              # a count outside 0 .. cap is held to it
    assert big.tolist() == [cap, 0, 1]


def test_drop_repetition_and_batch_independence(dev):
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(3, CAP, 3))
    flag = (rng.uniform(size=(3, CAP)) < 0.5).astype(np.int32)
    a, b = run_drop(dev, pts, [CAP, 300, 650], flag), run_drop(dev, pts, [CAP, 300, 650], flag)
    one = run_drop(dev, pts[:1], [CAP], flag[:1])
    for x, y, z in zip(a, b, one):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x[:1].view(np.uint8), z.view(np.uint8))


# ---- LocalMap.carve ---------------------------------------------------------------------------------------------------------------------
CARVE = dict(res=8, halo=1, margin=0.5, rel=0.02, near=1.0)


def carve_batch(seed=0):
    """a map of random rows about three poses and a sweep of returns mostly behind them, so that many rows are seen through"""
    import reg_ref
    rng = np.random.default_rng(seed)
    pose = np.stack((reg_ref.se3_exp((0.02, -0.03, 0.4, 0.0, 0.0, 0.0)), np.eye(4), reg_ref.se3_exp((0.0, 0.0, -1.1, 0.0, 0.0, 0.0))))
    pose[:, :3, 3] = ((50.3, -20.1, 1.2), (0.0, 0.0, 0.0), (-7.7, 3.1, -0.4))

    def rows(n, lo, hi):
        d = rng.normal(size=(n, 3))
        return d / np.abs(d).max(axis=1, keepdims=True) * rng.uniform(lo, hi, size=(n, 1))

    pts = np.stack([pose[b, :3, 3] + rows(CAP, 0.5, 12.0) for b in range(3)])
    sweep = np.stack([rows(600, 6.0, 9.0) for _ in range(3)]).astype(np.float32)
    sweep[0, 3], sweep[0, 4, 1] = np.nan, np.inf
    mask = np.ones((3, 600), dtype=np.int32)
    mask[1, ::3] = 0
    return pts, [650, CAP, 0], sweep, [600, 580, 600], pose, mask


def do_carve(m, batch, gate=None, use_mask=True):
    pts, counts, sweep, sc, pose, mask = batch
    dev = m.dev
    m.points = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(dev)     # a state of the test's own (rows >= count are finite)
    m.count = i32(dev, counts)
    m.carve(torch.from_numpy(sweep).to(dev), i32(dev, sc), torch.from_numpy(pose).to(dev), mask=torch.from_numpy(mask).to(dev) if use_mask else None,
            gate=None if gate is None else i32(dev, gate), **CARVE)


def new_map(dev, B, cap=CAP):
    from deflow_amd.localmap import LocalMap
    return LocalMap(B, cap, voxel=0.5, max_per_voxel=4, max_range=24.0, device=dev)


def test_carve_equals_the_restatement_stage_by_stage(dev):
    batch = carve_batch()
    pts, counts, sweep, sc, pose, mask = batch
    m = new_map(dev, 3)
    dropped = []
    for gate in (None, [0, 2, 0]):
        do_carve(m, batch, gate)
        last = {k: v.cpu().numpy() for k, v in m.last_carve.items()}
        assert last["count"].tolist() == counts
        for b in range(3):
            want, cnt, stat, st = vis_ref.carve(pts[b], counts[b], sweep[b], sc[b], pose[b], mask=mask[b], gate=None if gate is None else gate[b],
                                                **CARVE)
            assert np.array_equal(last["view"][b].view(np.uint32), st["view"].view(np.uint32)), b
            assert np.array_equal(last["img"][b].view(np.uint32), vis_ref.image(st["img"], CARVE["res"])), b
            assert np.array_equal(last["flag"][b], st["flag"]), b
            assert np.array_equal(f64bits(m.points[b].cpu().numpy()), f64bits(want)), b
            assert int(m.count[b]) == cnt and tuple(m.carve_stat[b].tolist()) == stat, (b, int(m.count[b]), m.carve_stat[b].tolist(), cnt, stat)
        dropped.append(m.carve_stat[:, 1].tolist())
    assert dropped[0][0] > 100 and dropped[0][1] > 100 and dropped[0][2] == 0 and dropped[1] == [dropped[0][0], 0, 0]
    # a carved map is a valid map: the next insert takes it
    dsweep, dsc, dpose = torch.from_numpy(sweep).to(dev), i32(dev, sc), torch.from_numpy(pose).to(dev)
    state, cnt = m.points.cpu().numpy(), m.count.cpu().numpy()
    m.insert(dsweep, dsc, dpose)
    for b in range(3):
        want, c, stat = map_ref.insert(state[b], cnt[b], sweep[b], sc[b], pose[b], 0.5, m.W, 4)
        assert np.array_equal(f64bits(m.points[b].cpu().numpy()), f64bits(want)) and int(m.count[b]) == c, b


def test_carve_repetition_and_batch_independence(dev):
    batch = carve_batch(1)

    def run(B):
        m = new_map(dev, B)
        do_carve(m, tuple(x[:B] for x in batch))
        return m.points.clone(), m.count.clone(), m.carve_stat.clone(), m.last_carve["flag"].clone(), m.last_carve["img"].clone()

    a, b, one = run(3), run(3), run(1)
    assert all(guarded.same_bits(x, y) for x, y in zip(a, b))
    assert all(guarded.same_bits(x, y[:1]) for x, y in zip(one, a))
    assert int(a[2][0, 1]) > 100


# ---- the guarded-call harness -----------------------------------------------------------------------------------------------------------
_i, _o = abi_sizes.i, abi_sizes.o


CARVE_TABLE = {          # the header's sizes of the entries a carve calls, local to this file (abi_sizes.TABLE stays as it is)
    "df_depth_cube_build": abi_sizes._e("points count mask B N R img", points=_i("12 * B * N"), count=_i("4 * B"),
                                        mask=_i("4 * B * N", True), img=_o("24 * B * R * R")),
    "df_depth_cube_test": abi_sizes._e("query count_q img B M R halo margin rel near flag depth_out", query=_i("12 * B * M"),
                                       count_q=_i("4 * B"), img=_i("24 * B * R * R"), flag=_o("4 * B * M"),
                                       depth_out=_o("4 * B * M", True)),
    "df_map_view": abi_sizes._e("map count pose B cap dst", map=_i("24 * B * cap"), count=_i("4 * B"), pose=_i("128 * B"),
                                dst=_o("12 * B * cap")),
    "df_map_drop": abi_sizes._e("map count flag gate B cap map_out count_out stat ws", map=_i("24 * B * cap"), count=_i("4 * B"),
                                flag=_i("4 * B * cap"), gate=_i("4 * B", True), map_out=_o("24 * B * cap"), count_out=_o("4 * B"),
                                stat=_o("8 * B"), ws=abi_sizes.ws("df_map_drop_ws_bytes", "B, cap")),
}


def test_guarded_carve_writes_nothing_outside_its_buffers(dev, monkeypatch):
    from deflow_amd import _lib, args, localmap, visibility
    table, protos = CARVE_TABLE, abi_sizes.header_prototypes()
    for name, entry in table.items():                                  # the local table against the header's prototypes
        assert [p.name for p in protos[name]][:-1] == list(entry.params) and protos[name][-1].name == "stream"
        for p in protos[name][:-1]:
            assert p.pointer == (p.name in entry.bufs) and (not p.pointer or p.nullable == entry.bufs[p.name].nullable)
            assert not p.pointer or p.const == (entry.bufs[p.name].role == abi_sizes.IN)
        assert len(_lib._SIGS[name]) == len(protos[name])
    assert [p.name for p in abi_sizes.header_prototypes()["df_map_drop_ws_bytes"]] == ["B", "cap"]
    batch = carve_batch(2)

    def scenario():
        m = new_map(dev, 3)
        do_carve(m, batch)
        first = [m.points.clone(), m.count.clone(), m.carve_stat.clone(), *m.last_carve.values()]
        do_carve(m, batch, gate=[0, 2, 0], use_mask=False)
        return first + [m.points, m.count, m.carve_stat, *m.last_carve.values()]

    outs = [scenario()]
    for fill in (0xA5, 0x7F):
        with monkeypatch.context() as mp:
            g = guarded.Guard(fill, _lib.call, table=table)
            for mod in (localmap, visibility, args):
                mp.setattr(mod, "call", g.call)
                mp.setattr(mod, "ptr", g.ptr)
            outs.append(scenario())
        assert g.seen == ["df_map_view", "df_depth_cube_build", "df_depth_cube_test", "df_map_drop"] * 2
    for k, (a, b, c) in enumerate(zip(*outs)):
        assert guarded.same_bits(a, b) and guarded.same_bits(a, c), k


def test_carve_argument_errors(dev):
    from deflow_amd._lib import call, ptr
    from deflow_amd.odometry import register_sweeps
    m = new_map(dev, 2, 64)
    x, c, p = torch.zeros(2, 5, 3, device=dev), i32(dev, [5, 5]), torch.eye(4, dtype=torch.float64, device=dev).repeat(2, 1, 1)
    ok = dict(res=8, halo=1, margin=0.5, rel=0.02, near=1.0)
    with pytest.raises(ValueError, match="DepthCube: res must be even"):
        m.carve(x, c, p, **{**ok, "res": 9})
    with pytest.raises(ValueError, match="LocalMap.carve: gate must be torch.int32"):
        m.carve(x, c, p, gate=c.long(), **ok)
    with pytest.raises(ValueError, match="LocalMap.view: pose must be torch.float64"):
        m.carve(x, c, p.float(), **ok)
    with pytest.raises(ValueError, match="DepthCube.seen_through: halo must be an integer"):
        m.carve(x, c, p, **{**ok, "halo": 7})
    f = torch.zeros(2, 64, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="df_map_drop failed: DF_E_ARG"):
        call("df_map_drop", ptr(m.points), ptr(m.count), ptr(f), None, 2, 64, ptr(m.points), ptr(c), ptr(f), ptr(f), s)
    with pytest.raises(ValueError, match="map_carve=True needs target='map'"):
        register_sweeps([np.zeros((4, 3))], device=dev, map_carve=True)


# ---- end to end: the room scene ---------------------------------------------------------------------------------------------------------
R = vis_ref.ROOM
KW = dict(stride=1, levels=R["levels"], min_range=R["min_range"], max_range=R["max_range"], map_voxel=R["voxel"], map_max_per_voxel=R["K"],
          map_capacity=R["cap"], xy_range=plane_ref.RANGE, cell=plane_ref.CELL, residual="plane", normal_radius=plane_ref.RADIUS,
          normal_min_pts=plane_ref.MIN_PTS, normal_max_curv=plane_ref.MAX_CURV, target="map")
CARVE_KW = dict(map_carve=True, map_carve_res=R["carve"]["res"], map_carve_halo=R["carve"]["halo"], map_carve_margin=R["carve"]["margin"],
                map_carve_rel=R["carve"]["rel"])


def dist(P, Q):
    return float(np.abs(np.asarray(P) - np.asarray(Q)).max())


@pytest.fixture(scope="module")
def room():
    sweeps, truth, is_object = vis_ref.room_scene()
    return sweeps, truth, vis_ref.register_sweeps_carve(sweeps, cube=R["carve"])


@pytest.fixture
def spy(monkeypatch):
    """what every LocalMap.carve of a run left behind, and the maps the run made"""
    from deflow_amd.localmap import LocalMap
    seen = dict(carves=[], maps=[])
    carve, init = LocalMap.carve, LocalMap.__init__

    def spy_carve(self, points, count, *a, **k):
        carve(self, points, count, *a, **k)
        seen["carves"].append(dict(self.last_carve, sweep=points, sweep_count=count, mask=k.get("mask"), stat=self.carve_stat))

    def spy_init(self, *a, **k):
        init(self, *a, **k)
        seen["maps"].append(self)

    monkeypatch.setattr(LocalMap, "carve", spy_carve)
    monkeypatch.setattr(LocalMap, "__init__", spy_init)
    return seen


def test_room_scene_against_the_restatement(dev, room, spy):
    from deflow_amd.odometry import chain_poses, register_sweeps
    sweeps, truth, ref = room
    rep = {}
    poses = chain_poses(register_sweeps(sweeps, None, device=dev, report=rep, **KW, **CARVE_KW))
    assert rep["failed"] == [] and len(spy["carves"]) == len(sweeps) - 1
    assert {k: rep["params"][k] for k in CARVE_KW} == CARVE_KW
    res, halo, sums = R["carve"]["res"], R["carve"]["halo"], []
    for k, c in enumerate(spy["carves"]):                             # the restatement on the GPU's own view and sweep tensors
        view, cnt, sweep = c["view"][0].cpu().numpy(), int(c["count"][0]), c["sweep"][0].cpu().numpy()
        img = vis_ref.build(sweep, int(c["sweep_count"][0]), c["mask"][0].cpu().numpy(), res)
        assert np.array_equal(c["img"][0].cpu().numpy().view(np.uint32), vis_ref.image(img, res)), k
        flag = vis_ref.test(view, cnt, img, res, halo, R["carve"]["margin"], R["carve"]["rel"], R["min_range"])[0]
        assert np.array_equal(c["flag"][0].cpu().numpy(), flag), k
        assert c["stat"][0].tolist() == [cnt, int(flag.sum())], k
        sums.append(int(flag.sum()))
    worst = max(dist(P, Q) for P, Q in zip(poses, ref["poses"]))
    print("map_carved", rep["map_carved"], "restatement", ref["carved"], "|pose - restatement|max", worst,
          "|pose - truth|max", vis_ref.pose_errors(poses, truth), "map rows", rep["map_count"])
    assert rep["map_carved"] == sums
    assert rep["map_carved"] == ref["carved"] and rep["map_count"] == [c for _, c in ref["maps"]]      # (c) holds: tests/test_visibility_cpu.py
    assert worst <= TOL


def test_room_scene_pose_error_without_the_carve(dev, room):
    """reported beside the figure of the test above; the float64 restatement does not separate the two (tests/test_visibility_cpu.py), so
    nothing is asserted between them"""
    from deflow_amd.odometry import chain_poses, register_sweeps
    sweeps, truth, _ = room
    rep = {}
    poses = chain_poses(register_sweeps(sweeps, None, device=dev, report=rep, **KW))
    print("without the carve: |pose - truth|max", vis_ref.pose_errors(poses, truth), "map rows", rep["map_count"])
    assert rep["failed"] == [] and "map_carved" not in rep and vis_ref.pose_errors(poses, truth) <= TOL


def test_failed_sweep_carves_nothing(dev, room, spy):
    from deflow_amd.odometry import register_sweeps
    sweeps = room[0][:3]
    rep = {}
    rel = register_sweeps(sweeps, None, device=dev, report=rep, **{**KW, "min_inliers": 10 ** 6}, **CARVE_KW)
    assert [f["status"] for f in rep["failed"]] == [2, 2] and rep["map_carved"] == [0, 0] and len(set(rep["map_count"])) == 1
    assert all(np.array_equal(T, np.eye(4)) for T in rel) and [c["stat"][0].tolist() for c in spy["carves"]] == [[0, 0], [0, 0]]
    m = spy["maps"][0]                                                 # the same on the map itself: bit-identical rows and count
    before = (m.points.clone(), m.count.clone())
    ps = torch.from_numpy(sweeps[2]).to(dev)[None]
    m.carve(ps, i32(dev, [len(sweeps[2])]), torch.eye(4, dtype=torch.float64, device=dev)[None], gate=i32(dev, [2]),
            **R["carve"], near=R["min_range"])
    assert guarded.same_bits(m.points, before[0]) and guarded.same_bits(m.count, before[1]) and m.carve_stat.tolist() == [[0, 0]]


def test_carve_off_is_the_call_without_the_key(dev, room, spy):
    from deflow_amd.odometry import register_sweeps
    sweeps = room[0][:4]
    a = register_sweeps(sweeps, None, device=dev, **KW)
    b = register_sweeps(sweeps, None, device=dev, map_carve=False, map_carve_res=64, **KW)
    assert spy["carves"] == [] and len(spy["maps"]) == 2               # no carve, so none of the new kernels was launched
    assert all(np.array_equal(x.view(np.int64), y.view(np.int64)) for x, y in zip(a, b))
    assert guarded.same_bits(spy["maps"][0].points, spy["maps"][1].points) and guarded.same_bits(spy["maps"][0].count, spy["maps"][1].count)
