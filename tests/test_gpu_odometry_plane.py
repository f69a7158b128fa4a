"""GPU: the point-to-plane part of the sweep-to-sweep registration -- df_normals, df_reg_accumulate_plane,
``odometry.normals``, ``odometry.register(residual="plane")``, the scene driver and the command -- on the planar scene of
tests/helpers/plane_ref.py, whose input conditions tests/test_odometry_plane_cpu.py checks on the float64 restatement.

Shapes: 562 rows (three blocks of 256, the last one partial), B <= 3, a grid of 24 x 24 cells of 2 m, neighbourhoods of 1.6 m.

Measured on an MI355X: largest angle to the reference normal 3.8e-8 rad (0.018 of the Davis-Kahan bound), |curv - ref| 9.4e-16; the 30
sums 2.9e-8 relative at worst (bound 1e-4); ``register(residual="plane")`` 4.6e-8 / 1.1e-7 / 5.3e-8 from the truth at stride 1 / stride
3 / planar (bound 1e-4), ``residual="point"`` 0.244 / 0.242 off on the same tensors."""
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
import plane_ref  # noqa: E402
import reg_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N = plane_ref.ROWS
RANGE, CELL, RADIUS, MIN_PTS, MAX_CURV = plane_ref.RANGE, plane_ref.CELL, plane_ref.RADIUS, plane_ref.MIN_PTS, plane_ref.MAX_CURV
G = 24
GRID = dict(xy_range=RANGE, cell=CELL)
NORMALS = dict(radius=RADIUS, min_pts=MIN_PTS, max_curv=MAX_CURV)
PLANE = dict(residual="plane", normal_radius=RADIUS, normal_min_pts=MIN_PTS, normal_max_curv=MAX_CURV)
TOL = 1e-4            # section 6r's bound: the per-row fp32 roundings carried through a well-conditioned fit
EPS = 2.0 ** -24
ARBITRARY = reg_ref.se3_exp((0.3, -0.2, 0.1, 1.0, 2.0, 3.0))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def i32(dev, v):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ---- test 1: normals against the reference ----------------------------------------------------------------------------------------------
def normals_batch():
    """points [3,N,3] fp32, counts, mask [3,N] i32: sample 0 the scene's target; sample 1 the same rows permuted, 40 of them NaN, a mask
    that drops every 11th row, 20 NaN-free rows hidden behind the count; sample 2 count 0 (its rows are finite and must not be read as
    taking part)"""
    _, dst, _ = plane_ref.planar_scene()
    rng = np.random.default_rng(6)                   # (a seed at which sample 1 keeps the curvature condition: the test asserts it)
    pts = np.stack((dst, dst[rng.permutation(N)], dst))
    pts[1, rng.choice(N - 20, size=40, replace=False)] = np.nan
    mask = np.ones((3, N), dtype=np.int32)
    mask[1, ::11] = 0
    mask[0, :] = 7                                   # any value > 0 takes part
    return pts, [N, N - 20, 0], mask


@pytest.fixture(scope="module")
def normals_ref():
    pts, counts, mask = normals_batch()
    return [plane_ref.normals(pts[b], counts[b], mask[b], **NORMALS) for b in range(3)]


def test_normals_against_the_reference(dev, normals_ref):
    from deflow_amd.odometry import normals
    pts, counts, mask = normals_batch()
    P, C, M = torch.from_numpy(pts).to(dev), i32(dev, counts), torch.from_numpy(mask).to(dev)
    n, curv, m = normals(P, C, mask=M, **GRID, **NORMALS)
    assert n.shape == (3, N, 3) and curv.shape == (3, N) and m.shape == (3, N) and m.dtype == torch.int32 and n.dtype == torch.float32
    n_h, curv_h, m_h = n.cpu().numpy(), curv.cpu().numpy(), m.cpu().numpy()
    worst_angle, worst_ratio, worst_curv = 0.0, 0.0, 0.0
    for b in range(3):
        ref = normals_ref[b]
        # the reference's own conditions on THIS sample: no curvature near max_curv (sample 1's neighbourhoods are not sample 0's)
        c = ref["curv_all"][np.isfinite(ref["curv_all"])]
        assert not np.any((c >= MAX_CURV / 100) & (c <= 5 * MAX_CURV))
        assert np.array_equal(m_h[b], ref["m"]), b
        valid = curv_h[b] >= 0
        assert np.array_equal(valid, ref["valid"]), b
        assert np.all(n_h[b][~valid].view(np.int32) == 0) and np.all(curv_h[b][~valid].view(np.int32) == np.float32(-1).view(np.int32))
        if not valid.any():
            continue
        p64, n64 = pts[b][valid].astype(np.float64), n_h[b][valid].astype(np.float64)
        assert np.abs(np.linalg.norm(n64, axis=1) - 1).max() <= 4 * EPS
        dot = (n64[:, 0] * p64[:, 0] + n64[:, 1] * p64[:, 1]) + n64[:, 2] * p64[:, 2]
        assert np.all(dot <= 0)                                                            # towards the origin
        lam = ref["lam"][valid]
        trace, gap = lam.sum(axis=1), lam[:, 1] - lam[:, 0]
        sel = gap >= 0.01 * trace
        assert sel.sum() >= 0.9 * valid.sum()
        cosang = np.clip(np.abs((n64[sel] * ref["n"][valid][sel]).sum(axis=1)), 0, 1)
        sinang = np.linalg.norm(np.cross(n64[sel], ref["n"][valid][sel]), axis=1)
        angle = np.arctan2(sinang, cosang)
        bound = 16 * EPS * trace[sel] / gap[sel]
        assert np.all((n64[sel] * ref["n"][valid][sel]).sum(axis=1) > 0)                   # the same side, not just the same line
        dc = np.abs(curv_h[b][valid].astype(np.float64) - ref["curv"][valid]).max()
        worst_angle, worst_ratio, worst_curv = max(worst_angle, angle.max()), max(worst_ratio, (angle / bound).max()), max(worst_curv, dc)
        print("sample", b, "valid", int(valid.sum()), "largest angle", angle.max(), "largest angle / bound", (angle / bound).max(),
              "largest |curv - ref|", dc)
        assert np.all(angle <= bound)
        assert dc <= 16 * EPS
    assert int((curv_h[0] >= 0).sum()) >= 400 and int((curv_h[1] >= 0).sum()) >= 200 and not (curv_h[2] >= 0).any()
    assert np.all(m_h[2] == 0)
    print("worst: angle", worst_angle, "angle / bound", worst_ratio, "|curv - ref|", worst_curv)
    # repeats are bit-identical; B = 1 equals sample 0 of B = 3
    again = normals(P, C, mask=M, **GRID, **NORMALS)
    assert all(bits(a) == bits(b) for a, b in zip(again, (n, curv, m)))
    alone = normals(P[:1].contiguous(), C[:1].contiguous(), mask=M[:1].contiguous(), **GRID, **NORMALS)
    assert all(bits(a[0]) == bits(b[0]) for a, b in zip(alone, (n, curv, m)))


# ---- test 2: an exactly flat cloud ------------------------------------------------------------------------------------------------------
def flat_cloud(n_side=17, z=-1.5, seed=3):
    rng = np.random.default_rng(seed)
    a, b = np.meshgrid(np.arange(n_side) - (n_side - 1) / 2.0, np.arange(n_side) - (n_side - 1) / 2.0, indexing="ij")
    xy = np.stack((a, b), axis=-1).reshape(-1, 2) + rng.uniform(-0.2, 0.2, size=(n_side * n_side, 2))
    return np.concatenate((xy, np.full((len(xy), 1), z)), axis=1).astype(np.float32)


@pytest.mark.parametrize("z", [-1.5, 1.5])
def test_flat_cloud_gets_the_axis_exactly(dev, z):
    from deflow_amd.odometry import normals
    pts = flat_cloud(z=z)
    n, curv, m = normals(torch.from_numpy(pts).to(dev)[None], i32(dev, [len(pts)]), xy_range=RANGE, cell=CELL, radius=RADIUS, min_pts=3,
                         max_curv=1.0 / 3.0)
    n_h, curv_h, m_h = n[0].cpu().numpy(), curv[0].cpu().numpy(), m[0].cpu().numpy()
    assert m_h.min() >= 3                                                 # every row is valid: nothing hides behind the default
    want = np.array([0.0, 0.0, 1.0 if z < 0 else -1.0], dtype=np.float32)     # n . p <= 0
    assert n_h.tobytes() == np.tile(want, (len(pts), 1)).tobytes()
    assert curv_h.tobytes() == np.zeros(len(pts), dtype=np.float32).tobytes()


# ---- test 3: one plane accumulate -------------------------------------------------------------------------------------------------------
def accumulate_batch():
    """src, dst [3,N,3]: sample 0 the scene, sample 1 count 0, sample 2 the planar-motion scene with the target's rows permuted"""
    s0, d0, _ = plane_ref.planar_scene()
    s2, d2, _ = plane_ref.planar_scene(motion=plane_ref.MOTION_PLANAR)
    d2 = d2[np.random.default_rng(8).permutation(N)]
    return np.stack((s0, s0, s2)), [N, 0, N], np.stack((d0, d0, d2)), [N, 0, N]


def file_both(src, cs, dst, cd):
    from deflow_amd.chamfer import RowGrid
    grid = RowGrid(src.shape[0], RANGE, CELL, src.device)
    assert (grid.minx, grid.miny, grid.G) == (RANGE[0], RANGE[1], G)
    return grid, grid.file(src, cs), grid.file(dst, cd)


def raw_normals(grid, filed, n):
    from deflow_amd._lib import call, ptr, stream
    out = torch.full((grid.B, n, 4), float("nan"), dtype=torch.float32, device=grid.dev)
    call("df_normals", ptr(filed[0]), ptr(filed[1]), grid.minx, grid.miny, CELL, G, grid.B, n, RADIUS, MIN_PTS, MAX_CURV, ptr(out), None,
         stream())
    return out


def accumulate(kind, src, cs, dst, cd, T, stride, max_dist, flip=False):
    """the two grids as ``register`` files them, the target's normals, then ONE accumulate of that kind with the per-row outputs on"""
    from deflow_amd._lib import call, ptr, stream
    b, ns, nd, dev = src.shape[0], src.shape[1], dst.shape[1], src.device
    grid, (s_rng, s_rows), (d_rng, d_rows) = file_both(src, cs, dst, cd)
    nblk = (ns + 255) // 256
    out = dict(partial=torch.full((b, nblk, 32), float("nan"), dtype=torch.float64, device=dev),
               q=torch.full((b, ns, 3), float("nan"), dtype=torch.float32, device=dev),
               idx=torch.full((b, ns), 12345, dtype=torch.int32, device=dev),
               d2=torch.full((b, ns), float("nan"), dtype=torch.float32, device=dev),
               w=torch.full((b, ns), float("nan"), dtype=torch.float32, device=dev))
    head = (ptr(s_rng), ptr(s_rows), G, ptr(d_rng), ptr(d_rows))
    tail = (ptr(T), max_dist ** 2, (max_dist / 3) ** 2, ptr(out["partial"]), ptr(out["q"]), ptr(out["idx"]), ptr(out["d2"]), ptr(out["w"]))
    if kind == "point":
        call("df_reg_accumulate", *head, RANGE[0], RANGE[1], CELL, G, b, ns, stride, *tail, stream())
        return out
    nrm = raw_normals(grid, (d_rng, d_rows), nd)
    if flip:
        nrm = torch.cat((-nrm[..., :3], nrm[..., 3:]), dim=-1).contiguous()
    out["e"] = torch.full((b, ns), float("nan"), dtype=torch.float32, device=dev)
    out["nrm"] = nrm
    call("df_reg_accumulate_plane", *head, ptr(nrm), RANGE[0], RANGE[1], CELL, G, b, ns, nd, stride, *tail, ptr(out["e"]), stream())
    return out


@pytest.mark.parametrize("stride", [1, 3])
def test_one_plane_accumulate(dev, stride):
    src_h, cs_h, dst_h, cd_h = accumulate_batch()
    src, cs, dst, cd = torch.from_numpy(src_h).to(dev), i32(dev, cs_h), torch.from_numpy(dst_h).to(dev), i32(dev, cd_h)
    T_h = np.stack((reg_ref.se3_exp((0.0005, -0.001, 0.003, 0.08, -0.03, 0.01)), ARBITRARY, reg_ref.se3_exp((0.01, 0.02, -0.01, -0.1, 0.2, 0.1))))
    T = torch.from_numpy(T_h).to(dev).reshape(3, 16).contiguous()
    max_dist = 1.0
    k2 = (max_dist / 3) ** 2
    out = accumulate("plane", src, cs, dst, cd, T, stride, max_dist)
    point = accumulate("point", src, cs, dst, cd, T, stride, max_dist)
    q, idx, d2, w, e = (out[k].cpu().numpy() for k in ("q", "idx", "d2", "w", "e"))
    pq, pidx, pd2 = (point[k].cpu().numpy() for k in ("q", "idx", "d2"))
    nrm = out["nrm"].cpu().numpy()
    partial = out["partial"].cpu().numpy()
    assert bits(out["q"]) == bits(point["q"])                                # the same transform, used or not
    S = partial.sum(axis=1)
    assert np.all(partial[..., 30:] == 0)
    for b in range(3):
        matched = pidx[b] >= 0
        partner_ok = np.zeros(N, dtype=bool)
        partner_ok[matched] = nrm[b][pidx[b][matched], 3] >= 0
        inl = matched & partner_ok
        # with a valid partner: the point entry's idx and d2 bit for bit; without: gated out
        assert np.array_equal(idx[b][inl], pidx[b][inl]) and d2[b][inl].tobytes() == pd2[b][inl].tobytes()
        assert np.all(idx[b][~inl] == -1) and np.all(np.isposinf(d2[b][~inl])) and np.all(w[b][~inl] == 0) and np.all(e[b][~inl] == 0)
        assert S[b, 29] == inl.sum()
        if b == 1:
            assert not matched.any() and np.all(partial[b] == 0)
            continue
        assert inl.sum() >= 100 / stride and (matched & ~partner_ok).sum() >= 20 / stride        # both kinds of row are present
        nj = nrm[b][idx[b][inl], :3].astype(np.float64)
        a64, e64 = plane_ref.rows_plane(q[b][inl], dst_h[b][idx[b][inl]], nj)
        assert np.abs(e[b][inl] - e64).max() <= 1e-5
        w64 = (k2 / (k2 + e64 * e64)) ** 2
        assert np.abs(w[b][inl] / w64 - 1).max() <= 1e-5
        H, g, sw, swe2, n = plane_ref.sums_plane(q[b][inl], dst_h[b][idx[b][inl]], nj, w64)
        Hk, gk, swk, swe2k, nk = reg_ref.unpack_slab(S[b])
        dH = (np.abs(Hk - H) / np.sqrt(np.outer(np.diag(H), np.diag(H)))).max()
        dg = (np.abs(gk - g) / np.sqrt(np.diag(H) * swe2)).max()
        print("stride", stride, "sample", b, "inliers", n, "dH", dH, "dg", dg, "dsw", abs(swk / sw - 1), "dswe2", abs(swe2k / swe2 - 1))
        assert nk == n and dH <= 1e-4 and dg <= 1e-4 and abs(swk / sw - 1) <= 1e-4 and abs(swe2k / swe2 - 1) <= 1e-4
    # negating every target normal: the slab bit for bit, e negated
    neg = accumulate("plane", src, cs, dst, cd, T, stride, max_dist, flip=True)
    assert all(bits(neg[k]) == bits(out[k]) for k in ("partial", "q", "idx", "d2", "w"))
    assert np.array_equal(neg["e"].cpu().numpy(), -e)
    # a second call is bit-identical; sample 0 alone equals sample 0 of the batch
    again = accumulate("plane", src, cs, dst, cd, T, stride, max_dist)
    assert all(bits(again[k]) == bits(out[k]) for k in ("partial", "q", "idx", "d2", "w", "e", "nrm"))
    alone = accumulate("plane", src[:1].contiguous(), cs[:1].contiguous(), dst[:1].contiguous(), cd[:1].contiguous(), T[:1].contiguous(),
                       stride, max_dist)
    assert all(bits(alone[k][0]) == bits(out[k][0]) for k in ("partial", "q", "idx", "d2", "w", "e", "nrm"))


# ---- test 4: the feature ----------------------------------------------------------------------------------------------------------------
def scene_on(dev, motion=plane_ref.MOTION):
    src, dst, T = plane_ref.planar_scene(motion=motion)
    return torch.from_numpy(src).to(dev)[None], i32(dev, [N]), torch.from_numpy(dst).to(dev)[None], i32(dev, [N]), T


@pytest.mark.parametrize("stride", [1, 3])
def test_plane_register_recovers_what_point_register_cannot(dev, stride):
    """From identity, the default schedule.  The target's rows are the source's sensor-frame positions on the moved planes: the nearest
    target of a source row is "itself", the point residual returns (almost) the identity, the plane residual the true motion."""
    from deflow_amd.odometry import register
    src, cs, dst, cd, T_true = scene_on(dev)
    T, info = register(src, cs, dst, cd, stride=stride, rows=True, **GRID, **PLANE)
    err = np.abs(T[0].cpu().numpy() - T_true).max()
    log = info["log"].cpu().numpy()
    print("stride", stride, "plane |T - T_true|max", err, "final log", log[0, -1].tolist(), "normals_valid", info["normals_valid"].tolist())
    assert T.dtype == torch.float64 and info["status"].tolist() == [0] and log.shape == (1, 25, 4)
    assert info["e"].shape == (1, N) and info["normals_valid"].shape == (1,) and int(info["normals_valid"][0]) >= 400
    assert err <= TOL
    T2, _ = register(src, cs, dst, cd, stride=stride, **GRID, **PLANE)
    assert bits(T2) == bits(T)                                              # two calls are bit-identical
    Tp, info_p = register(src, cs, dst, cd, stride=stride, rows=True, residual="point", **GRID)
    err_p = np.abs(Tp[0].cpu().numpy() - T_true).max()
    print("stride", stride, "point |T - T_true|max", err_p)
    assert info_p["status"].tolist() == [0] and err_p > 0.1 and "e" not in info_p and "normals_valid" not in info_p
    Td, _ = register(src, cs, dst, cd, stride=stride, **GRID)               # the default is the point residual, launch for launch
    assert bits(Td) == bits(Tp)


def test_plane_register_planar(dev):
    from deflow_amd.odometry import register
    src, cs, dst, cd, T_true = scene_on(dev, plane_ref.MOTION_PLANAR)
    T, info = register(src, cs, dst, cd, stride=1, planar=True, **GRID, **PLANE)
    T_h = T[0].cpu().numpy()
    err = np.abs(T_h - T_true).max()
    print("planar: |T - T_true|max", err)
    assert info["status"].tolist() == [0] and err <= TOL
    assert np.all(T_h[2, :2] == 0) and np.all(T_h[:2, 2] == 0) and T_h[2, 2] == 1          # omega_x, omega_y are never updated


# ---- test 5: degenerate scenes ----------------------------------------------------------------------------------------------------------
def test_plane_register_reports_degenerate_scenes(dev):
    """a single flat plane: every a = (q_y, -q_x, 0, 0, 0, 1), H has three zero rows exactly -> status 3; no valid normal at all (min_pts
    above every m) -> no inlier, status 2.  T == init bit for bit in both."""
    from deflow_amd.odometry import register
    pts = torch.from_numpy(flat_cloud()).to(dev)[None]
    cnt = i32(dev, [pts.shape[1]])
    init_h = reg_ref.se3_exp((0.0, 0.0, 0.01, 0.05, -0.02, 0.0))[None]
    init = torch.from_numpy(init_h).to(dev)
    T, info = register(pts, cnt, pts.clone(), cnt, init=init, stride=1, levels=((1.0, 3),), **GRID, **PLANE)
    log = info["log"].cpu().numpy()
    print("flat: status", info["status"].tolist(), "inliers", log[0, :, 0].tolist())
    assert info["status"].tolist() == [3] and T.cpu().numpy().tobytes() == init_h.tobytes()
    assert np.all(log[0, :, 0] > 200) and np.all(log[0, :, 2:] == 0)
    src, cs, dst, cd, _ = scene_on(dev)
    T, info = register(src, cs, dst, cd, init=init, stride=1, levels=((1.0, 3),), **GRID, **{**PLANE, "normal_min_pts": 100})
    assert info["status"].tolist() == [2] and T.cpu().numpy().tobytes() == init_h.tobytes()
    assert int(info["normals_valid"][0]) == 0 and np.all(info["log"].cpu().numpy() == 0)


# ---- test 6: a cloud that is not planar, sweeps, the command ----------------------------------------------------------------------------
def test_plane_register_on_the_lattice_cloud_never_gives_nan(dev):
    from deflow_amd.odometry import register
    T_true = reg_ref.se3_exp(reg_ref.MOTION)
    p = reg_ref.lattice(700, seed=0)
    src, dst = torch.from_numpy(p).to(dev)[None], torch.from_numpy(reg_ref.moved(p, T_true, seed=10)).to(dev)[None]
    cnt = i32(dev, [700])
    T, info = register(src, cnt, dst, cnt, stride=1, levels=((1.0, 6),), xy_range=(-24.0, -24.0, 24.0, 24.0), cell=2.0, residual="plane",
                       normal_radius=1.6, normal_min_pts=5, normal_max_curv=1.0 / 3.0, rows=True)
    print("lattice: status", info["status"].tolist(), "normals_valid", info["normals_valid"].tolist(), "final log",
          info["log"][0, -1].tolist())
    assert info["status"].tolist()[0] in (0, 2)
    assert bool(torch.isfinite(T).all()) and bool(torch.isfinite(info["log"]).all()) and bool(torch.isfinite(info["e"]).all())
    assert bool(torch.isfinite(info["w"]).all()) and bool(torch.isfinite(info["q"]).all())


def test_register_sweeps_plane_on_three_planar_sweeps(dev):
    from deflow_amd.odometry import register_sweeps
    T1 = reg_ref.se3_exp(plane_ref.MOTION)
    T2 = reg_ref.se3_exp((0.0, 0.0, 0.025, 0.22, -0.10, 0.04))
    sweeps = plane_ref.planar_sweeps((np.eye(4), T1, T2 @ T1))
    rep = {}
    rel = register_sweeps(sweeps, None, device=dev, report=rep, stride=1, min_range=0.0, **GRID, **PLANE)
    assert len(rel) == 2 and rep["failed"] == [] and rep["params"]["residual"] == "plane" and rep["params"]["normal_radius"] == RADIUS
    for k, (T, want) in enumerate(zip(rel, (T1, T2))):
        err = np.abs(T - want).max()
        print("pair", k, "|T - T_true|max", err, "inliers", rep["inliers"][k])
        assert T.dtype == np.float64 and err <= TOL
    with pytest.raises(TypeError, match="unknown parameters"):
        register_sweeps(sweeps, None, device=dev, residuals="plane")


def test_command_records_the_residual(dev, tmp_path, golden_dir, capsys):
    from deflow_amd import odometry
    from deflow_amd.data import HDF5Dataset
    src = os.path.join(golden_dir, "av2_mini", "train")
    shutil.copy(os.path.join(src, "scene_a.h5"), tmp_path / "scene_a.h5")
    with open(os.path.join(src, "index_total.pkl"), "rb") as f:
        index = [e for e in pickle.load(f) if e[0] == "scene_a"]
    with open(tmp_path / "index_total.pkl", "wb") as f:
        pickle.dump(index, f)
    assert odometry.main([f"data_dir={tmp_path}", "min_inliers=5", "stride=1", "iters=2", "residual=plane"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["scene"] == "scene_a" and line["sweeps"] == 25
    poses = odometry.read_sidecar(str(tmp_path / "scene_a.pose.npz"))
    assert len(poses) == 25
    for P in poses.values():
        assert P.shape == (4, 4) and P.dtype == np.float64 and np.isfinite(P).all()
        assert np.abs(P[:3, :3] @ P[:3, :3].T - np.eye(3)).max() <= 1e-6
    with np.load(tmp_path / "scene_a.pose.npz", allow_pickle=False) as z:
        meta = json.loads(str(z["meta"]))
    assert meta["residual"] == "plane" and meta["normal_radius"] == 1.0 and meta["normal_min_pts"] == 5 and meta["normal_max_curv"] == 0.05
    item = HDF5Dataset(str(tmp_path), pose_source="sidecar")[0]
    ts = sorted(poses, key=int)
    assert np.array_equal(item["pose0"].numpy(), poses[ts[0]]) and np.array_equal(item["pose1"].numpy(), poses[ts[1]])


# ---- test 7: the guarded-call harness ---------------------------------------------------------------------------------------------------
_i, _o, _io = abi_sizes.i, abi_sizes.o, abi_sizes.io
PLANE_TABLE = {          # the header's sizes of the two new entries, local to this file (abi_sizes.TABLE stays as it is)
    "df_nn_grid_build": abi_sizes.TABLE["df_nn_grid_build"],
    "df_normals": abi_sizes._e("cell_rng sorted minx miny cell G B N radius min_pts max_curv normals m_out",
                               cell_rng=_i("8 * B * G * G"), sorted=_i("16 * B * N"), normals=_o("16 * B * N"), m_out=_o("4 * B * N", True)),
    "df_reg_accumulate_plane": abi_sizes._e(
        "src_rng src_sorted Gs dst_rng dst_sorted dst_normals minx miny cell G B Ns Nd stride T max_dist2 k2 partial q_out idx_out d2_out "
        "w_out e_out",
        src_rng=_i("8 * B * Gs * Gs"), src_sorted=_i("16 * B * Ns"), dst_rng=_i("8 * B * G * G"), dst_sorted=_i("16 * B * Nd"),
        dst_normals=_i("16 * B * Nd"), T=_i("128 * B"), partial=abi_sizes.ws("df_reg_ws_bytes", "B, Ns"), q_out=_o("12 * B * Ns", True),
        idx_out=_o("4 * B * Ns", True), d2_out=_o("4 * B * Ns", True), w_out=_o("4 * B * Ns", True), e_out=_o("4 * B * Ns", True)),
    "df_reg_solve": abi_sizes._e("partial B nblk min_inliers planar T log status",
                                 partial=_i("256 * B * nblk"), T=_io("128 * B", True), log=_o("16 * B"), status=_o("4 * B", True)),
}


def test_guarded_plane_entries_write_nothing_outside_their_buffers(dev, monkeypatch):
    from deflow_amd import _lib, args, chamfer, odometry
    protos = abi_sizes.header_prototypes()
    for name in ("df_normals", "df_reg_accumulate_plane"):             # the local table against the header's prototypes
        assert [p.name for p in protos[name]][:-1] == list(PLANE_TABLE[name].params)
        for p in protos[name][:-1]:
            assert p.pointer == (p.name in PLANE_TABLE[name].bufs) and (not p.pointer or p.nullable == PLANE_TABLE[name].bufs[p.name].nullable)
            assert not p.pointer or p.const == (PLANE_TABLE[name].bufs[p.name].role == abi_sizes.IN)
    src_h, cs_h, dst_h, cd_h = accumulate_batch()
    dst_h = np.concatenate((dst_h, np.full((3, 37, 3), np.nan, dtype=np.float32)), axis=1)       # Nd = 599 != Ns = 562
    src, cs, dst, cd = torch.from_numpy(src_h).to(dev), i32(dev, cs_h), torch.from_numpy(dst_h).to(dev), i32(dev, cd_h)
    init = torch.from_numpy(np.stack((np.eye(4), ARBITRARY, np.eye(4)))).to(dev)

    def scenario(stride):
        T, info = odometry.register(src, cs, dst, cd, init=init, stride=stride, levels=((1.0, 2),), rows=True, **GRID, **PLANE)
        n, curv, m = odometry.normals(dst, cd, **GRID, **NORMALS)
        return [T, info["status"], info["log"], info["q"], info["idx"], info["d2"], info["w"], info["e"], info["normals_valid"], n, curv, m]

    for stride in (1, 3):
        outs = [scenario(stride)]
        for fill in (0xA5, 0x7F):
            with monkeypatch.context() as mp:
                g = guarded.Guard(fill, _lib.call, table=PLANE_TABLE)
                for mod in (odometry, chamfer, args):       # register's own entries, the grid build, the workspace query
                    mp.setattr(mod, "call", g.call)
                    mp.setattr(mod, "ptr", g.ptr)
                outs.append(scenario(stride))
            assert g.seen.count("df_reg_accumulate_plane") == 3 and g.seen.count("df_reg_solve") == 3 and g.seen.count("df_normals") == 2
            assert g.seen.count("df_nn_grid_build") == 3 and "df_reg_accumulate" not in g.seen
        for a, b, c in zip(*outs):
            assert guarded.same_bits(a, b) and guarded.same_bits(a, c)
        assert int(outs[0][8][0]) >= 400 and outs[0][1].tolist() == [0, 2, 0]


# ---- test 8: argument errors ------------------------------------------------------------------------------------------------------------
def test_plane_argument_errors(dev):
    from deflow_amd._lib import load
    from deflow_amd.odometry import normals, register
    src, cs, dst, cd, _ = scene_on(dev)
    with pytest.raises(ValueError, match="register: residual must be 'point' or 'plane', got 'x'"):
        register(src, cs, dst, cd, residual="x", **GRID)
    with pytest.raises(ValueError, match=r"register: normal_radius = 2\.5 is larger than the grid's cell = 2\.0"):
        register(src, cs, dst, cd, **GRID, **{**PLANE, "normal_radius": 2.5})
    with pytest.raises(ValueError, match=r"normals: radius = 2\.5 is larger than the grid's cell = 2\.0"):
        normals(dst, cd, **GRID, **{**NORMALS, "radius": 2.5})
    with pytest.raises(ValueError, match=r"register: normal_min_pts must be an integer in \[3, "):
        register(src, cs, dst, cd, **GRID, **{**PLANE, "normal_min_pts": 2})
    with pytest.raises(ValueError, match=r"normals: max_curv must lie in \(0, 1/3\]"):
        normals(dst, cd, **GRID, **{**NORMALS, "max_curv": 0.5})
    with pytest.raises(TypeError, match=r"normals: points must be a CUDA tensor \(deflow_amd has no CPU fallback\)"):
        normals(dst.cpu(), cd, **GRID, **NORMALS)
    with pytest.raises(TypeError, match="register: dst must be a CUDA tensor"):
        register(src, cs, dst.cpu(), cd, **GRID, **PLANE)
    with pytest.raises(ValueError, match="normals: mask must be"):
        normals(dst, cd, mask=torch.ones(1, N, device=dev), **GRID, **NORMALS)
    register(src, cs, dst, cd, levels=((1.0, 1),), **GRID, normal_radius=99.0)          # not looked at with the point residual
    # the raw entry refuses without launching: the outputs keep their bytes
    import ctypes as C
    lib = load()
    grid, _, (d_rng, d_rows) = file_both(src, cs, dst, cd)
    out = torch.full((1, N + 1, 4), 3.0, dtype=torch.float32, device=dev)

    def raw(radius=RADIUS, min_pts=MIN_PTS, normals_ptr=out.data_ptr()):
        return lib.df_normals(C.c_void_p(d_rng.data_ptr()), C.c_void_p(d_rows.data_ptr()), RANGE[0], RANGE[1], CELL, G, 1, N, radius, min_pts,
                              MAX_CURV, C.c_void_p(normals_ptr), C.c_void_p(0), C.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert raw(radius=2.5) == -3 and raw(min_pts=2) == -3 and raw(normals_ptr=out.data_ptr() + 4) == -2
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    assert raw() == 0
    torch.cuda.synchronize()
    assert int((out[0, :N, 3] >= 0).sum()) >= 400 and bool((out[0, N] == 3.0).all())
