"""CPU: the conditions the point-to-plane tests (tests/test_gpu_odometry_plane.py) put on their INPUT, checked on the float64 restatement
of tests/helpers/plane_ref.py alone, and the command line's new keys.

The scene is plane_ref.planar_scene: four planes sampled at sensor-frame positions, 562 rows, neighbourhoods of radius 1.6 m under a grid
of 2 m cells.  The conditions make the GPU comparison exact where it is stated as exact: no pair of rows is close enough to the radius
for fp32 to put it on the other side, and no neighbourhood's curvature is close enough to max_curv = 1e-5 to change its validity."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plane_ref  # noqa: E402
import reg_ref  # noqa: E402


@pytest.fixture(scope="module")
def scene():
    src, dst, T = plane_ref.planar_scene()
    nrm = plane_ref.normals(dst, len(dst), radius=plane_ref.RADIUS, min_pts=plane_ref.MIN_PTS, max_curv=plane_ref.MAX_CURV)
    return src, dst, T, nrm


def test_scene_is_the_recipe(scene):
    src, dst, T, _ = scene
    assert src.shape == dst.shape == (562, 3) and src.dtype == dst.dtype == np.float32 and plane_ref.ROWS == 562
    assert np.abs(T - reg_ref.se3_exp(plane_ref.MOTION)).max() == 0
    which = plane_ref.plane_of_row()
    for k, (direction, off, _) in enumerate(plane_ref.PLANES):
        n = np.asarray(direction) / np.linalg.norm(direction)
        assert np.abs(src[which == k].astype(np.float64) @ n - off).max() <= 2e-6              # fp32 rows on the plane
        n2 = T[:3, :3] @ n
        assert np.abs(dst[which == k].astype(np.float64) @ n2 - (off + n2 @ T[:3, 3])).max() <= 2e-6
    # the same sensor-frame positions: every target row is its source row moved ALONG the moved plane's normal, by less than the motion
    assert np.abs(dst.astype(np.float64) - src).max() <= 0.5
    # inside the tests' grid
    assert np.abs(dst[:, :2]).max() < plane_ref.RANGE[2] - plane_ref.CELL and plane_ref.RADIUS <= plane_ref.CELL


def test_no_pair_distance_is_near_the_radius(scene):
    _, dst, _, _ = scene
    margin = plane_ref.pair_margin(dst, np.ones(len(dst), dtype=bool), plane_ref.RADIUS)
    print("smallest | |p_j - p_i| - radius |", margin)
    assert margin > 1e-5


def test_no_curvature_is_near_max_curv(scene):
    _, _, _, nrm = scene
    c = nrm["curv_all"]
    assert np.isfinite(c).all()
    pure, mixed = c[c < plane_ref.MAX_CURV / 100], c[c > 5 * plane_ref.MAX_CURV]
    print("largest pure-plane curvature", pure.max(), "smallest mixed", mixed.min(), "valid", int(nrm["valid"].sum()),
          "rows with m < min_pts", int((nrm["m"] < plane_ref.MIN_PTS).sum()))
    assert len(pure) + len(mixed) == len(c)                   # nothing in [max_curv / 100, 5 max_curv]
    assert int(nrm["valid"].sum()) >= 400
    # a valid normal is its plane's, pointing at the origin
    T = scene[2]
    which = plane_ref.plane_of_row()
    for k, (direction, off, _) in enumerate(plane_ref.PLANES):
        n2 = T[:3, :3] @ (np.asarray(direction) / np.linalg.norm(direction))
        n2 = -n2 if off + n2 @ T[:3, 3] > 0 else n2
        sel = nrm["valid"] & (which == k)
        assert sel.sum() > 30 and np.abs(nrm["n"][sel] - n2).max() <= 1e-5


def test_point_restatement_misses_and_plane_restatement_recovers(scene):
    src, dst, T, _ = scene
    Tp, status = reg_ref.register(src, len(src), dst, len(dst), plane_ref.LEVELS)
    err_point = np.abs(Tp - T).max()
    Tq, status_q = plane_ref.register_plane(src, len(src), dst, len(dst), plane_ref.LEVELS, radius=plane_ref.RADIUS,
                                            min_pts=plane_ref.MIN_PTS, max_curv=plane_ref.MAX_CURV)
    err_plane = np.abs(Tq - T).max()
    print("|T - T_true|max: point", err_point, "(|T - I|max", np.abs(Tp - np.eye(4)).max(), ") plane", err_plane)
    assert status == 0 and status_q == 0
    assert err_point > 0.1
    assert err_plane < 1e-6


def test_planar_variant_restatement():
    src, dst, T = plane_ref.planar_scene(motion=plane_ref.MOTION_PLANAR)
    Tq, status = plane_ref.register_plane(src, len(src), dst, len(dst), plane_ref.LEVELS, radius=plane_ref.RADIUS,
                                          min_pts=plane_ref.MIN_PTS, max_curv=plane_ref.MAX_CURV, planar=True)
    err = np.abs(Tq - T).max()
    print("planar: |T - T_true|max", err)
    assert status == 0 and err < 1e-6


def test_sums_plane_against_a_plain_loop():
    """the vectorised sums against the definition written out row by row"""
    rng = np.random.default_rng(1)
    q, d = rng.normal(size=(40, 3)) * 5, rng.normal(size=(40, 3)) * 5
    n = rng.normal(size=(40, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    w = rng.uniform(0.1, 1.0, 40)
    H, g, sw, swe2, k = plane_ref.sums_plane(q, d, n, w)
    H2, g2, s2 = np.zeros((6, 6)), np.zeros(6), 0.0
    for qi, di, ni, wi in zip(q, d, n, w):
        a = np.concatenate((np.cross(qi, ni), ni))
        e = ni @ (qi - di)
        H2 += wi * np.outer(a, a)
        g2 += wi * a * e
        s2 += wi * e * e
    assert np.allclose(H, H2, rtol=1e-13, atol=1e-12) and np.allclose(g, g2, rtol=1e-13, atol=1e-12) and abs(swe2 - s2) <= 1e-12 * s2
    assert k == 40 and abs(sw - w.sum()) <= 1e-13
    # negating the normals changes nothing
    H3, g3, _, s3, _ = plane_ref.sums_plane(q, d, -n, w)
    assert np.array_equal(H3, H) and np.array_equal(g3, g) and s3 == swe2


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def test_command_parser_takes_the_plane_keys():
    from deflow_amd.odometry import CLI_DEFAULTS, DEFAULTS, USAGE, parse_args
    assert DEFAULTS["residual"] == "point" and (DEFAULTS["normal_radius"], DEFAULTS["normal_min_pts"], DEFAULTS["normal_max_curv"]) == \
        (1.0, 5, 0.05)
    cfg = parse_args(["data_dir=/d", "residual=plane", "normal_radius=0.8", "normal_min_pts=6", "normal_max_curv=0.02"])
    assert (cfg["residual"], cfg["normal_radius"], cfg["normal_min_pts"], cfg["normal_max_curv"]) == ("plane", 0.8, 6, 0.02)
    assert {k: v for k, v in cfg.items() if k not in ("data_dir", "residual", "normal_radius", "normal_min_pts", "normal_max_curv")} == \
        {k: v for k, v in CLI_DEFAULTS.items() if k not in ("data_dir", "residual", "normal_radius", "normal_min_pts", "normal_max_curv")}
    assert parse_args(["data_dir=/d"]) == {**CLI_DEFAULTS, "data_dir": "/d"} and CLI_DEFAULTS["residual"] == "point"
    for bad in (["data_dir=/d", "residual=foo"], ["data_dir=/d", "normal_radius=0"], ["data_dir=/d", "normal_max_curv=0.5"],
                ["data_dir=/d", "normal_max_curv=0"], ["data_dir=/d", "normal_min_pts=2"], ["data_dir=/d", "normal_radius=nan"],
                ["data_dir=/d", "residual=plane", "normal_radius=1.5"]):                       # (the radius beyond the default cell of 1)
        with pytest.raises(SystemExit):
            parse_args(bad)
    assert parse_args(["data_dir=/d", "residual=plane", "normal_radius=1.5", "cell=2"])["cell"] == 2.0
    for key in ("residual=point|plane", "normal_radius=", "normal_min_pts=", "normal_max_curv="):
        assert key in USAGE


def test_register_and_normals_refuse_before_the_gpu():
    import torch
    from deflow_amd.odometry import normals, register
    x = torch.zeros(1, 8, 3)
    c = torch.full((1,), 8, dtype=torch.int32)
    with pytest.raises(TypeError, match=r"normals: points must be a CUDA tensor \(deflow_amd has no CPU fallback\)"):
        normals(x, c, xy_range=plane_ref.RANGE, cell=2.0, radius=1.6, min_pts=5, max_curv=0.05)
    with pytest.raises(TypeError, match="register: src must be a CUDA tensor"):
        register(x, c, x, c, residual="plane")


def test_new_bindings_match_the_header():
    import ctypes as C
    import abi_sizes
    from deflow_amd import _lib
    protos = abi_sizes.header_prototypes()
    names = list(_lib._SIGS)
    for n in ("df_normals", "df_reg_accumulate_plane"):
        assert names.index(n) > names.index("df_reg_solve")             # after the range abi_sizes.in_scope sizes
        assert len(_lib._SIGS[n]) == len(protos[n])
        for t, p in zip(_lib._SIGS[n], protos[n]):
            assert (t is C.c_void_p) == p.pointer, (n, p.name)
    assert [p.name for p in protos["df_normals"] if p.nullable] == ["m_out"]
    assert [p.name for p in protos["df_reg_accumulate_plane"] if p.nullable] == ["q_out", "idx_out", "d2_out", "w_out", "e_out"]


def test_new_entries_reject_bad_arguments_without_launching():
    """every check fails before the launch: fake (aligned, never dereferenced) addresses do on a machine without a GPU"""
    import ctypes as C
    from deflow_amd import _lib, build
    build.build()
    lib = _lib.load()
    P, a = C.c_void_p, 0x10000

    def nrm(cell_rng=a, sorted_=a, cell=2.0, G=8, B=2, N=300, radius=1.6, min_pts=5, max_curv=0.05, normals=a, m_out=0):
        return lib.df_normals(P(cell_rng), P(sorted_), -8.0, -8.0, cell, G, B, N, radius, min_pts, max_curv, P(normals), P(m_out), P(0))

    assert nrm(cell_rng=0) == -3 and nrm(sorted_=0) == -3 and nrm(normals=0) == -3                  # DF_E_ARG
    for r in (2.5, 0.0, -1.0, float("nan"), float("inf")):
        assert nrm(radius=r) == -3, r
    assert nrm(min_pts=2) == -3 and nrm(max_curv=0.0) == -3 and nrm(max_curv=0.34) == -3 and nrm(max_curv=float("nan")) == -3
    assert nrm(cell=0.0) == -3
    assert nrm(B=0) == -1 and nrm(B=65536) == -1 and nrm(N=0) == -1 and nrm(G=4097) == -1 and nrm(B=4, N=1 << 28) == -1   # DF_E_SHAPE
    assert nrm(normals=a + 8) == -2 and nrm(sorted_=a + 4) == -2 and nrm(m_out=a + 2) == -2          # DF_E_ALIGN

    def acc(src_rng=a, src_sorted=a, Gs=8, dst_rng=a, dst_sorted=a, dst_normals=a, cell=1.0, G=8, B=2, Ns=300, Nd=300, stride=1, T=a,
            max_dist2=1.0, k2=0.1, partial=a):
        return lib.df_reg_accumulate_plane(P(src_rng), P(src_sorted), Gs, P(dst_rng), P(dst_sorted), P(dst_normals), -4.0, -4.0, cell, G, B,
                                           Ns, Nd, stride, P(T), max_dist2, k2, P(partial), P(0), P(0), P(0), P(0), P(0), P(0))

    for name in ("src_rng", "src_sorted", "dst_rng", "dst_sorted", "dst_normals", "T", "partial"):
        assert acc(**{name: 0}) == -3, name
    assert acc(stride=0) == -3 and acc(stride=1025) == -3
    for v in (float("inf"), float("nan"), 0.0, -1.0):
        assert acc(max_dist2=v) == -3 and acc(k2=v) == -3 and acc(cell=v) == -3, v
    assert acc(B=0) == -1 and acc(B=65536) == -1 and acc(Ns=0) == -1 and acc(Nd=0) == -1 and acc(G=0) == -1 and acc(Gs=4097) == -1
    assert acc(B=4, Nd=1 << 28) == -1
    assert acc(src_sorted=a + 8) == -2 and acc(dst_sorted=a + 4) == -2 and acc(dst_normals=a + 8) == -2 and acc(partial=a + 4) == -2
