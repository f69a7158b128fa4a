"""CPU: the map-carving keys of the odometry command, the bindings and argument checks of the depth-cube and map-drop entries, the
restatement of tests/helpers/vis_ref.py against a vectorised form written another way, and the conditions of the room scene that
tests/test_gpu_localmap_carve.py registers on the GPU, on the float64 reference alone (UNPINNED).

The room scene (6 sweeps of 72 azimuths x 15 rings ray-cast into four tilted walls and a lid from a sensor that moves 0.22 m per sweep,
a 1 x 1 x 1.8 m block crossing the view by 1 m per sweep; cube of 12 bins, halo 1, margin 0.5, rel 0.02, near 1).  Measured on the
reference: rows carved per later sweep 0, 15, 26, 25, 23, none of them static; of the block rows at least two sweeps old 10 of 20, 20 of
27, 16 of 26 and 12 of 19 are carved; the flags do not change under +-2e-5 m on every coordinate of the view.  Cubes of 8 and 16 bins
carve no static row either; 16 leaves a tenth of the bins inside the rings empty, 8 carves under half of the old rows.  Largest pose
error against the truth 1.74e-6 with the carve and 1.72e-6 without: the plane residual on exact planes is not pulled by the block's trail (its rows
have no valid normal or lie in the planes the new rows lie in), so the two do not separate and nothing about accuracy is asserted."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import vis_ref  # noqa: E402


# ---- the command line and register_sweeps -------------------------------------------------------------------------------------------------
def test_command_parser_takes_the_carve_keys():
    from deflow_amd.odometry import CLI_DEFAULTS, MAP_CARVE_DEFAULTS, USAGE, parse_args
    assert MAP_CARVE_DEFAULTS == {"map_carve": False, "map_carve_res": 256, "map_carve_halo": 1, "map_carve_margin": 0.5, "map_carve_rel": 0.02}
    assert all(CLI_DEFAULTS[k] == v for k, v in MAP_CARVE_DEFAULTS.items())
    cfg = parse_args(["data_dir=/d", "target=map", "map_carve=true", "map_carve_res=64", "map_carve_halo=2", "map_carve_margin=0.25",
                      "map_carve_rel=0.05"])
    assert [cfg[k] for k in MAP_CARVE_DEFAULTS] == [True, 64, 2, 0.25, 0.05]
    assert parse_args(["data_dir=/d"])["map_carve"] is False
    for bad in ("map_carve=yes", "map_carve_res=0", "map_carve_res=7", "map_carve_res=2050", "map_carve_halo=5", "map_carve_halo=-1",
                "map_carve_margin=-0.1", "map_carve_rel=nan", "map_carve_res=1.5"):
        with pytest.raises(SystemExit):
            parse_args(["data_dir=/d", "target=map", bad])
    with pytest.raises(SystemExit, match="map_carve=true needs target=map"):
        parse_args(["data_dir=/d", "map_carve=true"])
    for key in MAP_CARVE_DEFAULTS:
        assert key + "=" in USAGE


def test_register_sweeps_refuses_bad_carve_arguments_before_the_gpu():
    from deflow_amd.odometry import register_sweeps
    one = [np.zeros((4, 3))]
    with pytest.raises(ValueError, match="map_carve=True needs target='map'"):
        register_sweeps(one, map_carve=True)
    with pytest.raises(ValueError, match="map_carve must be True or False"):
        register_sweeps(one, target="map", map_carve=1)
    with pytest.raises(ValueError, match="map_carve_res must be even"):
        register_sweeps(one, target="map", map_carve=True, map_carve_res=15)
    with pytest.raises(ValueError, match="map_carve_res must be an integer"):
        register_sweeps(one, target="map", map_carve=True, map_carve_res=4096)
    with pytest.raises(ValueError, match="map_carve_halo must be an integer"):
        register_sweeps(one, target="map", map_carve=True, map_carve_halo=5)
    with pytest.raises(ValueError, match="map_carve_margin must be finite"):
        register_sweeps(one, target="map", map_carve=True, map_carve_margin=-1.0)
    with pytest.raises(ValueError, match="map_carve_rel must be finite"):
        register_sweeps(one, target="map", map_carve=True, map_carve_rel=float("inf"))
    with pytest.raises(TypeError, match="device must be a CUDA device"):
        register_sweeps(one, target="map", map_carve=True, device="cpu")


# ---- the bindings and the entries' argument checks ---------------------------------------------------------------------------------------
NEW = ["df_depth_cube_build", "df_depth_cube_test", "df_map_drop_ws_bytes", "df_map_drop"]


def test_bindings_of_the_new_entries_match_the_header():
    import abi_sizes
    from deflow_amd import _lib
    protos = abi_sizes.header_prototypes()
    names = list(_lib._SIGS)
    for n in NEW:
        assert names.index("df_refine_apply") < names.index(n) < names.index("df_reg_ws_bytes")   # outside the window abi_sizes sizes
        assert len(_lib._SIGS[n]) == len(protos[n])
        for t, p in zip(_lib._SIGS[n], protos[n]):
            assert (t is _lib.P) == p.pointer, (n, p.name)
    assert [p.name for p in protos["df_depth_cube_build"] if p.nullable] == ["mask"]
    assert [p.name for p in protos["df_depth_cube_test"] if p.nullable] == ["depth_out"]
    assert [p.name for p in protos["df_map_drop"] if p.nullable] == ["gate"]
    assert "df_map_drop_ws_bytes" in _lib._RAW and _lib._RESTYPE["df_map_drop_ws_bytes"] is _lib.C.c_int64
    assert _lib._SIGS["df_depth_cube_test"][7:10] == [_lib.F] * 3


def test_new_entries_reject_bad_arguments_without_launching():
    """every check fails before the launch: fake (aligned, never dereferenced) addresses do on a machine without a GPU"""
    import ctypes as C
    from deflow_amd import _lib, build
    build.build()
    lib = _lib.load()
    P, a = C.c_void_p, 0x10000

    def cube(points=a, B=2, N=600, R=8, img=a):
        return lib.df_depth_cube_build(P(points), P(a), P(0), B, N, R, P(img), P(0))

    assert cube(points=0) == -3 and cube(img=0) == -3 and cube(points=a + 2) == -2
    assert cube(B=0) == -1 and cube(B=65536) == -1 and cube(N=0) == -1 and cube(R=0) == -1 and cube(R=7) == -1 and cube(R=2050) == -1
    assert cube(B=43, R=2048, N=1) == -1 and cube(B=2, N=2 ** 29) == -1                 # 6 B R R >= 2^30, B N >= 2^30

    def test(query=a, R=8, halo=1, margin=0.5, rel=0.02, near=3.0, flag=a, M=640):
        return lib.df_depth_cube_test(P(query), P(a), P(a), 2, M, R, halo, margin, rel, near, P(flag), P(0), P(0))

    assert test(query=0) == -3 and test(flag=0) == -3 and test(flag=a + 1) == -2 and test(R=9) == -1 and test(M=0) == -1
    assert test(halo=-1) == -3 and test(halo=5) == -3
    for bad in (-1.0, float("nan"), float("inf")):
        assert test(margin=bad) == -3 and test(rel=bad) == -3 and test(near=bad) == -3, bad

    def drop(map_=a, out=2 * a, B=2, cap=700, ws=a, flag=a):
        return lib.df_map_drop(P(map_), P(a), P(flag), P(0), B, cap, P(out), P(a), P(a), P(ws), P(0))

    assert drop(out=a) == -3 and drop(map_=0) == -3 and drop(ws=0) == -3 and drop(flag=0) == -3 and drop(map_=a + 4) == -2
    assert drop(B=0) == -1 and drop(cap=0) == -1 and drop(B=2, cap=2 ** 29) == -1
    assert _lib.call("df_map_drop_ws_bytes", 3, 700) == 4 * 3 * 3 and _lib.call("df_map_drop_ws_bytes", 3, 768) == 4 * 3 * 3
    assert _lib.call("df_map_drop_ws_bytes", 0, 700) == -1


# ---- the restatement against a vectorised form written another way ------------------------------------------------------------------------
def cube_vectorised(points, count, mask, R):
    """numpy float32 arrays, np.argmax for the axis, np.minimum.at for the bins -> (img [6,R,R] u32, face, i, j, m, ok)"""
    p = np.asarray(points, dtype=np.float32)
    n = len(p)
    ok = (np.arange(n) < count) & np.isfinite(p).all(axis=1)
    if mask is not None:
        ok &= np.asarray(mask) > 0
    a = np.abs(np.where(np.isfinite(p), p, np.float32(0)))
    axis = np.argmax(a, axis=1)                                       # (the first maximum: on ties the earlier axis)
    rows = np.arange(n)
    m = a[rows, axis]
    ok &= m > 0
    neg = np.signbit(p[rows, axis]) & (p[rows, axis] != 0)
    rest = np.array([[1, 2], [0, 2], [0, 1]])[axis]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ij = []
        for k in range(2):
            t = (p[rows, rest[:, k]] / m + np.float32(1.0)) * np.float32(R // 2)
            ij.append(np.minimum(R - 1, np.floor(np.where(ok, t, 0)).astype(np.int64)))
    face = 2 * axis + neg
    img = np.full((6, R, R), vis_ref.EMPTY, dtype=np.uint32)
    np.minimum.at(img, (face[ok], ij[1][ok], ij[0][ok]), m[ok].view(np.uint32))
    return img, face, ij[0], ij[1], m, ok


def test_vectorised(query, count_q, img, R, halo, margin, rel, near):
    """sliding minimum over a +inf-padded image"""
    _, face, i, j, m, ok = cube_vectorised(query, count_q, None, R)
    pad = np.full((6, R + 2 * halo, R + 2 * halo), vis_ref.EMPTY, dtype=np.uint32)
    pad[:, halo:halo + R, halo:halo + R] = img
    win = np.full((6, R, R), vis_ref.EMPTY, dtype=np.uint32)
    for dj in range(2 * halo + 1):
        for di in range(2 * halo + 1):
            win = np.minimum(win, pad[:, dj:dj + R, di:di + R])
    inside = ok & (i >= halo) & (i <= R - 1 - halo) & (j >= halo) & (j <= R - 1 - halo)
    dmin = np.where(inside, win[face, j, i], np.uint32(vis_ref.EMPTY)).astype(np.uint32)
    q = np.asarray(query, dtype=np.float32)
    c = np.float32(1.0) + np.float32(rel)
    with np.errstate(over="ignore", invalid="ignore"):
        lhs = m * c + np.float32(margin)
        far = np.maximum(np.abs(q[:, 0]), np.abs(q[:, 1])) >= np.float32(near)
        flag = inside & far & (img[face, j, i] != vis_ref.EMPTY) & (lhs < dmin.view(np.float32))
    return flag.astype(np.int32), dmin


test_vectorised.__test__ = False


@pytest.mark.parametrize("R", [2, 8, 256])
@pytest.mark.parametrize("N,M", [(600, 640), (640, 600)])
def test_restatement_agrees_with_the_vectorised_form(R, N, M):
    case = vis_ref.kernel_case(R, N, M)
    flagged = 0
    for b in range(3):
        img = vis_ref.build(case["points"][b], case["count"][b], case["mask"][b], R)
        want = cube_vectorised(case["points"][b], case["count"][b], case["mask"][b], R)[0]
        assert np.array_equal(vis_ref.image(img, R), want), b
        for halo in (0, 1, 2):
            flag, depth = vis_ref.test(case["query"][b], case["count_q"][b], img, R, halo, vis_ref.MARGIN, vis_ref.REL, vis_ref.NEAR)
            f2, d2 = test_vectorised(case["query"][b], case["count_q"][b], want, R, halo, vis_ref.MARGIN, vis_ref.REL, vis_ref.NEAR)
            assert np.array_equal(flag, f2) and np.array_equal(depth, d2), (b, halo)
            flagged += int(flag.sum())
            assert not flag[case["count_q"][b]:].any()
    assert flagged > 20
    assert len(vis_ref.build(case["points"][1], case["count"][1], case["mask"][1], R)) == 1          # N - 5 rows in one bin
    assert vis_ref.build(case["points"][2], 0, None, R) == {}


def test_the_cases_bite():
    """the hand-made rows do what they were made for, at R = 8"""
    R = 8
    sp = vis_ref.special_rows()
    got = [vis_ref.bin_of(r, R) for r in sp]
    assert [g[0] for g in got[:4]] == [0, 2, 0, 0]                    # ties: the earlier axis
    assert [g[0] for g in got[28:32]] == [1, 3, 1, 1]                 # all negative
    assert got[32] is None and got[33] is None and got[34] is None    # the origin, with any zero signs
    assert got[35][0] == 2 and got[36][:3] == (0, 4, 4) and got[37][:3] == (0, 4, 4) and got[38][0] == 4    # -0.0: the positive side
    assert got[39][1:3] == (7, 0) and got[40][1:3] == (0, 7)          # u = +1 is clamped to R - 1, u = -1 is bin 0
    assert got[41][1:3] == (7, 0) and got[42][1:3] == (0, 7) and got[43][0] == 1        # one ulp inside; |x| == |z|: the earlier axis
    assert got[44] is None and got[45] is None and got[46] is None and got[47] is not None and got[48] is not None
    case = vis_ref.kernel_case(R, 600, 640)
    img = vis_ref.build(case["points"][0], 600, case["mask"][0], R)
    k = 2 * len(sp)                                                   # the threshold triple: equal, one ulp behind, one ulp before
    for halo in (0, 1):
        flag, depth = vis_ref.test(case["query"][0], 640, img, R, halo, vis_ref.MARGIN, vis_ref.REL, vis_ref.NEAR)
        assert flag[k:k + 3].tolist() == [0, 1, 0]
        assert [vis_ref.bits(vis_ref.lhs_of(4.0)) - int(d) for d in depth[k:k + 3]] == [0, -1, 1]
    edges = {h: vis_ref.test(case["query"][0], 640, img, R, h, vis_ref.MARGIN, vis_ref.REL, vis_ref.NEAR)[0][k + 3:k + 3 + 24] for h in (0, 1, 2)}
    assert edges[0].all()                                             # every edge query has a return far behind it
    assert edges[1].reshape(2, 6, 2).sum(axis=(0, 2)).tolist() == [0, 4, 4, 4, 4, 0]
    assert edges[2].reshape(2, 6, 2).sum(axis=(0, 2)).tolist() == [0, 0, 4, 4, 0, 0]
    near = vis_ref.test(case["query"][0], 640, img, R, 0, vis_ref.MARGIN, vis_ref.REL, vis_ref.NEAR)[0][k + 27:k + 33]
    assert near.tolist() == [1, 1, 1, 0, 0, 0]                        # max(|x|, |y|) == near is far enough, one ulp below is not
    flag, depth = vis_ref.test(case["query"][0], 640, img, R, 1, vis_ref.MARGIN, vis_ref.REL, vis_ref.NEAR)
    assert case["hole"] not in [(f, i, j) for (f, j, i) in img] and flag[639] == 0 and depth[639] != vis_ref.EMPTY    # the empty own bin


# ---- the drop -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 300, 700])
def test_drop_restatement_is_a_stable_filter(count):
    rng = np.random.default_rng(count)
    pts = rng.normal(size=(700, 3))
    flag = (rng.uniform(size=700) < 0.3).astype(np.int32)
    out, cnt, stat = vis_ref.drop(pts, count, flag)
    keep = (np.arange(700) < count) & (flag == 0)
    assert cnt == keep.sum() and stat == (count, count - cnt)
    assert np.array_equal(out[:cnt], pts[keep]) and (out[cnt:].view(np.int64) == 0x7FF8000000000000).all()
    out, cnt, stat = vis_ref.drop(pts, count, flag, gate=2)
    assert cnt == count and stat == (0, 0) and np.array_equal(out[:cnt], pts[:count]) and np.isnan(out[cnt:]).all()


# ---- the room scene on the reference alone ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def room():
    sweeps, truth, is_object = vis_ref.room_scene()
    carved = vis_ref.register_sweeps_carve(sweeps, is_object, cube=vis_ref.ROOM["carve"], perturb=2e-5)
    plain = vis_ref.register_sweeps_carve(sweeps)
    return sweeps, truth, is_object, carved, plain


def test_room_scene_conditions_on_the_reference(room):
    sweeps, truth, is_object, r, plain = room
    assert len(sweeps) == 6 and all(s.shape == (1080, 3) for s in sweeps) and all(15 <= o.sum() <= 40 for o in is_object)
    assert r["status"] == [0] * 5 and r["overflow"] == [0] * 5 and plain["status"] == [0] * 5
    print("carved", r["carved"], "static", r["static"], "old (in the map, carved)", r["old"], "stable", r["stable"])
    assert r["static"] == [0] * 5                                     # (a) no static row is ever carved
    assert sum(n for n, _ in r["old"]) >= 40 and all(2 * c >= n for n, c in r["old"])          # (b) at least half of the old block rows
    assert r["stable"] == [True] * 5                                  # (c) +-2e-5 m on every coordinate of the view changes no flag
    assert sum(r["carved"]) >= 80 and r["carved"][0] == 0 and r["maps"][-1][1] < plain["maps"][-1][1]
    res = vis_ref.ROOM["carve"]["res"]                                # the cube is coarse enough that the rings leave no bin empty
    img = vis_ref.image(r["stages"][0]["img"], res)                   # above the lowest ring (-8 degrees: v >= -1 / 6 is row 5, partly)
    assert (img[:4, 6:] != vis_ref.EMPTY).all() and (img[4] != vis_ref.EMPTY).sum() >= res * res // 2 and (img[5] == vis_ref.EMPTY).all()


def test_room_scene_pose_error_with_and_without_the_carve(room):
    """reported, not asserted against each other: on exact planes the plane residual is not pulled by the trail (this file's docstring)"""
    sweeps, truth, is_object, r, plain = room
    with_carve, without = vis_ref.pose_errors(r["poses"], truth), vis_ref.pose_errors(plain["poses"], truth)
    print("largest pose error against the truth: with the carve", with_carve, "without", without)
    assert with_carve <= 1e-4 and without <= 1e-4
    assert not (without >= 3.0 * with_carve)                          # no separation by a factor of 3: nothing more may be claimed
