"""GPU: the sweep-to-sweep registration of DESIGN.md section 6r -- df_reg_accumulate / df_reg_solve, ``odometry.register``, the scene
driver, the command and the guarded-call harness -- on the lattice cloud of tests/helpers/reg_ref.py, whose correspondences are
unambiguous in fp32 and in float64, so that results are held against the TRUE motion.

Shapes: B = 3, Ns = Nd = 700 (three blocks of 256, the last one partial), counts (700, 0, 333), NaN rows inside the count and NaN padding
behind it, a grid smaller than the cloud (minx = miny = -16, G = 12, cell 2.7: rows beyond it sit in the clamped border cells), stride 1
and 3."""
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
import reg_ref  # noqa: E402

pytestmark = pytest.mark.gpu

B, N = 3, 700
COUNTS = (700, 0, 333)
CELL, G = 2.7, 12
RANGE = (-16.0, -16.0, -16.0 + G * CELL, -16.0 + G * CELL)
GRID = dict(xy_range=RANGE, cell=CELL)
TOL = 1e-4            # the project's stated tolerance: the per-row fp32 transform rounding carried through a well-conditioned fit
ARBITRARY = reg_ref.se3_exp((0.3, -0.2, 0.1, 1.0, 2.0, 3.0))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def make_batch(motion=reg_ref.MOTION, extra=0, nan_dst=False):
    """-> src [B,N+extra,3], dst [B,N,3] (numpy fp32, NaN behind the counts), T_true.  Sample b's dst = its participating-or-not first
    COUNTS[b] source rows moved by T_true, in permuted order.  NaN rows inside the count: source rows 5 and 100 of sample 0, 9 of sample 2
    (their partners stay in dst: unused); nan_dst: also dst row 7 of sample 0.  extra: source rows appended 30 m above the cloud."""
    T = reg_ref.se3_exp(motion)
    src = np.full((B, N + extra, 3), np.nan, dtype=np.float32)
    dst = np.full((B, N, 3), np.nan, dtype=np.float32)
    counts_s = []
    for b, c in enumerate(COUNTS):
        counts_s.append(c + extra if c else 0)
        if not c:
            continue
        p = reg_ref.lattice(c, seed=b)
        src[b, :c] = p
        dst[b, :c] = reg_ref.moved(p, T, seed=10 + b)
        if extra:
            src[b, c:c + extra] = reg_ref.lattice(extra, seed=20 + b) + np.array([0, 0, 30], dtype=np.float32)
    src[0, 5] = src[0, 100] = src[2, 9] = np.nan
    if nan_dst:
        dst[0, 7] = np.nan
    return src, counts_s, dst, list(COUNTS), T


def to_dev(dev, src, cs, dst, cd):
    return (torch.from_numpy(src).to(dev), torch.tensor(cs, dtype=torch.int32, device=dev), torch.from_numpy(dst).to(dev),
            torch.tensor(cd, dtype=torch.int32, device=dev))


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


# ---- test 1: one accumulate -------------------------------------------------------------------------------------------------------------
def accumulate(src, cs, dst, cd, T, stride, max_dist, src_grid=None):
    """the two grids as ``register`` files them, then ONE df_reg_accumulate with the per-row outputs on.  src_grid: (xy_range, cell) of a
    grid of its own for the source (the target's stays)"""
    from deflow_amd._lib import call, ptr, stream
    from deflow_amd.chamfer import RowGrid
    b, ns, dev = src.shape[0], src.shape[1], src.device
    grid = RowGrid(b, GRID["xy_range"], CELL, dev)
    assert (grid.minx, grid.miny, grid.G) == (RANGE[0], RANGE[1], G)
    sgrid = grid if src_grid is None else RowGrid(b, src_grid[0], src_grid[1], dev)
    (s_rng, s_rows), (d_rng, d_rows) = sgrid.file(src, cs), grid.file(dst, cd)
    nblk = (ns + 255) // 256
    assert call("df_reg_ws_bytes", b, ns) == b * nblk * 256
    partial = torch.full((b, nblk, 32), float("nan"), dtype=torch.float64, device=dev)
    q = torch.full((b, ns, 3), float("nan"), dtype=torch.float32, device=dev)
    idx = torch.full((b, ns), 12345, dtype=torch.int32, device=dev)
    d2 = torch.full((b, ns), float("nan"), dtype=torch.float32, device=dev)
    w = torch.full((b, ns), float("nan"), dtype=torch.float32, device=dev)
    call("df_reg_accumulate", ptr(s_rng), ptr(s_rows), sgrid.G, ptr(d_rng), ptr(d_rows), RANGE[0], RANGE[1], CELL, G, b, ns, stride, ptr(T),
         max_dist ** 2, (max_dist / 3) ** 2, ptr(partial), ptr(q), ptr(idx), ptr(d2), ptr(w), stream())
    return dict(partial=partial, q=q, idx=idx, d2=d2, w=w, s_rng=s_rng, s_rows=s_rows, Gs=sgrid.G)


def used_mask(out, b, ns, stride):
    """the subsample rule restated: positions s, s + stride, ... of sample b's span in the source's cell order -> bool [ns] by ROW"""
    rng = out["s_rng"].cpu().numpy().reshape(-1, G * G, 2)
    s, e = int(rng[b, 0, 0]), int(rng[b, -1, 1])
    rows = out["s_rows"].cpu().numpy()[s:e:stride, 3].copy().view(np.int32)
    used = np.zeros(ns, dtype=bool)
    used[rows] = True
    assert used.sum() == len(rows)
    return used, e - s


@pytest.mark.parametrize("stride", [1, 3])
def test_one_accumulate(dev, stride):
    from deflow_amd.chamfer import chamfer_nn
    src_h, cs_h, dst_h, cd_h, T_true = make_batch(nan_dst=True)
    src, cs, dst, cd = to_dev(dev, src_h, cs_h, dst_h, cd_h)
    T_h = np.stack((reg_ref.se3_exp((0.0005, -0.001, 0.003, 0.08, -0.03, 0.01)), ARBITRARY, np.eye(4)))
    T = torch.from_numpy(T_h).to(dev).reshape(B, 16).contiguous()
    max_dist = 1.0
    out = accumulate(src, cs, dst, cd, T, stride, max_dist)
    q, idx, d2, w = (out[k].cpu().numpy() for k in ("q", "idx", "d2", "w"))
    partial = out["partial"].cpu().numpy()
    used = np.zeros((B, N), dtype=bool)
    for b in range(B):
        used[b], span = used_mask(out, b, N, stride)
        assert span == int(reg_ref.participating(src_h[b], cs_h[b]).sum())
        if stride == 1:
            assert np.array_equal(used[b], reg_ref.participating(src_h[b], cs_h[b]))
    assert used[0].sum() == (698 + stride - 1) // stride and used[1].sum() == 0 and used[2].sum() == (332 + stride - 1) // stride
    # rows that are not used: the defaults, every element written
    assert np.all(q[~used] == 0) and np.all(idx[~used] == -1) and np.all(np.isposinf(d2[~used])) and np.all(w[~used] == 0)
    # q against the float64 transform: a coordinate below 128 m has a half-ulp of 3.8e-6, fewer than six roundings give 2.3e-5
    q64 = np.einsum("bij,bnj->bni", T_h[:, :3, :3], src_h.astype(np.float64)) + T_h[:, None, :3, 3]
    dq = np.abs(q[used] - q64[used]).max()
    print("stride", stride, "|q - q64|max", dq)
    assert dq <= 1e-4
    # the search: the same device function as df_chamfer_nn, so bit-equal on q_out (unused rows masked out by the query label)
    cd2, cidx = chamfer_nn(out["q"], cs, dst, cd, qlabel=torch.from_numpy(used.astype(np.int32)).to(dev), max_dist2=max_dist ** 2,
                           grid_range=RANGE, cell=CELL)
    assert bits(cd2) == bits(out["d2"]) and bits(cidx) == bits(out["idx"])
    inl = idx >= 0
    assert np.all(d2[inl] <= max_dist ** 2) and np.all(w[~inl] == 0) and inl[0].sum() > 600 / stride and not inl[1].any()
    k2 = (max_dist / 3) ** 2
    w64 = (k2 / (k2 + d2[inl].astype(np.float64))) ** 2
    assert np.abs(w[inl] / w64 - 1).max() <= 1e-6
    # the 30 sums, restated in float64 from the kernel's own (q_out, idx_out)
    S = partial.sum(axis=1)
    for b in range(B):
        m = inl[b]
        H, g, sw, swr, n = reg_ref.sums(q[b][m], dst_h[b][idx[b][m]], (k2 / (k2 + d2[b][m].astype(np.float64))) ** 2)
        Hk = np.zeros((6, 6))
        Hk[np.triu_indices(6)] = S[b, :21]
        assert S[b, 29] == n and S[b, 30] == 0 and S[b, 31] == 0
        if n == 0:
            assert np.all(partial[b] == 0)
            continue
        dH = np.abs(Hk - np.triu(H)) / np.sqrt(np.outer(np.diag(H), np.diag(H)))
        dg = np.abs(S[b, 21:27] - g) / np.sqrt(np.diag(H) * swr)
        print("sample", b, "dH", dH.max(), "dg", dg.max(), "dsw", abs(S[b, 27] / sw - 1), "dswr", abs(S[b, 28] / swr - 1))
        assert dH.max() <= 1e-4 and dg.max() <= 1e-4 and abs(S[b, 27] / sw - 1) <= 1e-4 and abs(S[b, 28] / swr - 1) <= 1e-4
        assert Hk[0, 3] == 0 and Hk[1, 4] == 0 and Hk[2, 5] == 0 and Hk[3, 4] == 0 and Hk[3, 5] == 0 and Hk[4, 5] == 0
        assert Hk[3, 3] == Hk[4, 4] == Hk[5, 5] == S[b, 27] and Hk[0, 4] == -Hk[1, 3] and Hk[0, 5] == -Hk[2, 3] and Hk[1, 5] == -Hk[2, 4]
    # a second call is bit-identical
    again = accumulate(src, cs, dst, cd, T, stride, max_dist)
    assert all(bits(again[k]) == bits(out[k]) for k in ("partial", "q", "idx", "d2", "w"))
    # sample 0 alone equals sample 0 of the batch
    alone = accumulate(src[:1].contiguous(), cs[:1].contiguous(), dst[:1].contiguous(), cd[:1].contiguous(), T[:1].contiguous(), stride,
                       max_dist)
    assert all(bits(alone[k][0]) == bits(out[k][0]) for k in ("partial", "q", "idx", "d2", "w"))


# ---- test 2, 3: register ----------------------------------------------------------------------------------------------------------------
def check_register(dev, motion, stride, planar=False, extra=0, init_h=None, levels=((1.0, 6),), full=False):
    """full: -> (T, info, T_true) instead of T"""
    from deflow_amd.odometry import register
    src_h, cs_h, dst_h, cd_h, T_true = make_batch(motion, extra=extra)
    src, cs, dst, cd = to_dev(dev, src_h, cs_h, dst_h, cd_h)
    if init_h is None:
        init_h = np.stack((np.eye(4), ARBITRARY, np.eye(4)))
    init = torch.from_numpy(init_h).to(dev)
    T, info = register(src, cs, dst, cd, init=init, stride=stride, levels=levels, planar=planar, rows=True, **GRID)
    assert T.dtype == torch.float64 and T.shape == (B, 4, 4) and info["log"].shape == (B, 7, 4) and info["status"].dtype == torch.int32
    assert info["q"].shape == (B, N + extra, 3) and info["idx"].shape == (B, N + extra)
    T_h, status, log = T.cpu().numpy(), info["status"].cpu().numpy(), info["log"].cpu().numpy()
    err = [np.abs(T_h[b] - T_true).max() for b in (0, 2)]
    print("stride", stride, "planar", planar, "extra", extra, "|T - T_true|max", err, "log[0]", log[0].tolist())
    assert status.tolist() == [0, 2, 0]
    assert max(err) <= TOL
    assert T_h[1].tobytes() == init_h[1].tobytes()                   # count 0: fewer than min_inliers, T untouched bit for bit
    assert np.all(log[1] == 0) and log[0, -1, 0] == (698 + stride - 1) // stride and np.all(log[0, -1, 2:] == 0)
    assert np.all(T_h[:, 3] == [0, 0, 0, 1])
    if extra:                                                        # the rows 30 m above: used, never inliers
        assert np.all(info["idx"][0, N:].cpu().numpy() == -1) and np.all(info["w"][0, N:].cpu().numpy() == 0)
    return (T, info, T_true) if full else T


@pytest.mark.parametrize("stride", [1, 3])
def test_register_recovers_the_lattice_motion(dev, stride):
    T = check_register(dev, reg_ref.MOTION, stride)
    assert bits(check_register(dev, reg_ref.MOTION, stride)) == bits(T)          # two calls are bit-identical


def test_register_ignores_rows_beyond_every_gate(dev):
    check_register(dev, reg_ref.MOTION, 1, extra=100)


def test_register_planar(dev):
    T = check_register(dev, reg_ref.MOTION_PLANAR, 1, planar=True).cpu().numpy()
    # omega_x, omega_y are never updated: from identity the rotation stays about z exactly
    assert np.all(T[0, 2, :2] == 0) and np.all(T[0, :2, 2] == 0) and T[0, 2, 2] == 1


def test_register_from_an_init_near_the_truth(dev):
    """a 0.8 m motion is beyond half the node spacing: identity would mismatch; init = the truth moved by 0.1 m"""
    motion = (0.001, -0.0015, 0.004, 0.8, -0.05, 0.02)
    near = reg_ref.se3_exp((0, 0, 0, 0.06, -0.06, 0.05)) @ reg_ref.se3_exp(motion)
    check_register(dev, motion, 1, init_h=np.stack((near, ARBITRARY, near)))


def test_register_argument_errors(dev):
    from deflow_amd.odometry import register
    src, cs, dst, cd = to_dev(dev, *make_batch()[:4])
    with pytest.raises(ValueError, match="register: count_s must be torch.int32"):
        register(src, cs.long(), dst, cd)
    with pytest.raises(ValueError, match="register: stride must be"):
        register(src, cs, dst, cd, stride=0)
    with pytest.raises(ValueError, match="register: init must be"):
        register(src, cs, dst, cd, init=torch.eye(4, device=dev))
    with pytest.raises(ValueError, match="register: mask_s must be"):
        register(src, cs, dst, cd, mask_s=torch.ones(B, N, device=dev))
    with pytest.raises(TypeError, match="register: dst must be a CUDA tensor"):
        register(src, cs, dst.cpu(), cd)


# ---- the turning branch, status 3, several levels ---------------------------------------------------------------------------------------
def partner_margin(src, count, dst, motion_T):
    """float64, at identity: (every participating source row's nearest target row is the row it was moved to, the smallest distance by
    which the second-nearest target is farther).  ``moved`` permutes: the partner is found as the target nearest to the MOVED row."""
    ok = reg_ref.participating(src, count)
    s = src[ok].astype(np.float64)
    d = dst[:count].astype(np.float64)
    partner = (((s @ motion_T[:3, :3].T + motion_T[:3, 3])[:, None, :] - d[None]) ** 2).sum(axis=2)
    assert partner.min(axis=1).max() <= 1e-10               # (the fp32 rounding of the moved row)
    dist = np.sqrt(((s[:, None, :] - d[None]) ** 2).sum(axis=2))
    order = np.sort(dist, axis=1)
    return bool(np.all(dist.argmin(axis=1) == partner.argmin(axis=1))), float((order[:, 1] - order[:, 0]).min())


@pytest.mark.parametrize("stride", [1, 3])
def test_register_through_the_closed_form_branch(dev, stride):
    """MOTION with three times the yaw: the first iteration's |omega| is 0.0121 >= 1e-2, so the closed form of the exponential runs
    inside the loop.  Conditions on the input: every source row's nearest target at identity is its true partner, the second-nearest at
    least 0.09 m farther (0.0945 m at 700 rows, 0.296 m at 333).  The float64 helper reaches 1.3e-8 and 1.9e-8 in six iterations."""
    src_h, cs_h, dst_h, cd_h, T_true = make_batch(reg_ref.MOTION_TURN)
    for b in (0, 2):
        true_partner, margin = partner_margin(src_h[b], COUNTS[b], dst_h[b], T_true)
        print("sample", b, "second-nearest margin", margin)
        assert true_partner and margin >= 0.09
    T, info, _ = check_register(dev, reg_ref.MOTION_TURN, stride, full=True)
    log = info["log"].cpu().numpy()
    print("stride", stride, "|omega| of iteration 0", log[:, 0, 2].tolist())
    assert log[0, 0, 2] >= 1e-2 and log[2, 0, 2] >= 1e-2


def test_register_reports_a_singular_system(dev):
    """status 3 through ``register``: every row at the origin (H's rotation block is 0) and a cloud on the x axis (rank 5: H[0][0] = sum
    w (qy^2 + qz^2) is exactly 0, also from an init that turns about x and shifts along it).  T == init bit for bit, |omega| = |v| = 0 in
    every log row."""
    from deflow_amd.odometry import register
    n = 60
    pts = np.zeros((2, n, 3), dtype=np.float32)
    pts[1, :, 0] = -15.0 + 0.5 * np.arange(n)
    c, s = np.cos(0.3), np.sin(0.3)
    init_h = np.stack((ARBITRARY.copy(), np.array([[1, 0, 0, 0.125], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1.0]])))
    init_h[0, :3, 3] = 0.0                                   # a rotation about the origin leaves the rows at the origin
    src = torch.from_numpy(pts).to(dev)
    cnt = torch.full((2,), n, dtype=torch.int32, device=dev)
    T, info = register(src, cnt, src.clone(), cnt, init=torch.from_numpy(init_h).to(dev), stride=1, levels=((1.0, 3),), **GRID)
    log = info["log"].cpu().numpy()
    print("status", info["status"].tolist(), "log", log.tolist())
    assert info["status"].tolist() == [3, 3]
    assert T.cpu().numpy().tobytes() == init_h.tobytes()
    assert log.shape == (2, 4, 4) and np.all(log[:, :, 0] == n) and np.all(log[:, :, 2:] == 0)


@pytest.mark.parametrize("stride", [1, 3])
def test_register_over_several_levels(dev, stride):
    """three levels of two iterations: T against the truth, at stride 1 against the float64 restatement with the same levels; the log has
    one row per iteration and one for the final T; the inlier count does not increase from level to level"""
    levels = ((2.0, 2), (1.0, 2), (0.5, 2))
    T, info, T_true = check_register(dev, reg_ref.MOTION, stride, levels=levels, full=True)
    T_h, log = T.cpu().numpy(), info["log"].cpu().numpy()
    assert log.shape == (B, 7, 4)
    for b in (0, 2):
        per_level = log[b, [1, 3, 5, 6], 0]
        print("stride", stride, "sample", b, "inliers per level and final", per_level.tolist(), "|T - T_true|max", np.abs(T_h[b] - T_true).max())
        assert np.all(np.diff(per_level) <= 0) and per_level[-1] > 0
    if stride == 1:
        src_h, cs_h, dst_h, cd_h, _ = make_batch(reg_ref.MOTION)
        for b in (0, 2):
            T_ref, status = reg_ref.register(src_h[b], cs_h[b], dst_h[b], cd_h[b], levels)
            err = np.abs(T_h[b] - T_ref).max()
            print("sample", b, "|T - restatement|max", err)
            assert status == 0 and err <= TOL


# ---- a source grid of its own -----------------------------------------------------------------------------------------------------------
def test_accumulate_with_a_source_grid_of_its_own(dev):
    """The source filed under a 6 x 6 grid of 8 m cells over (-24, -24, 24, 24) while the target keeps its 12 x 12 grid of 2.7 m cells:
    the header lets the source's grid set the ORDER of the rows and nothing else.  Stride 1: q, idx, d2, w bit-identical to the run with
    one grid; the slab summed over blocks within the summation-order bound 2 n 2^-53 (n = 697: 1.5e-13) in test_one_accumulate's norms."""
    src_h, cs_h, dst_h, cd_h, _ = make_batch(nan_dst=True)
    src, cs, dst, cd = to_dev(dev, src_h, cs_h, dst_h, cd_h)
    T_h = np.stack((reg_ref.se3_exp((0.0005, -0.001, 0.003, 0.08, -0.03, 0.01)), ARBITRARY, np.eye(4)))
    T = torch.from_numpy(T_h).to(dev).reshape(B, 16).contiguous()
    one = accumulate(src, cs, dst, cd, T, 1, 1.0)
    own = accumulate(src, cs, dst, cd, T, 1, 1.0, src_grid=((-24.0, -24.0, 24.0, 24.0), 8.0))
    assert one["Gs"] == G and own["Gs"] == 6
    assert not torch.equal(one["s_rows"], own["s_rows"])                 # the order of the rows really differs
    assert all(bits(one[k]) == bits(own[k]) for k in ("q", "idx", "d2", "w"))
    Sa, Sb = one["partial"].cpu().numpy().sum(axis=1), own["partial"].cpu().numpy().sum(axis=1)
    assert np.all(Sb[1] == 0) and np.all(Sa[1] == 0)
    for b in (0, 2):
        n = Sa[b, 29]
        bound = 2 * n * 2.0 ** -53
        Ha, ga, sw, swr, _ = reg_ref.unpack_slab(Sa[b])
        Hb, gb, swb, swrb, nb = reg_ref.unpack_slab(Sb[b])
        dH = (np.abs(Ha - Hb) / np.sqrt(np.outer(np.diag(Ha), np.diag(Ha)))).max()
        dg = (np.abs(ga - gb) / np.sqrt(np.diag(Ha) * swr)).max()
        print("sample", b, "n", n, "bound", bound, "dH", dH, "dg", dg, "dsw", abs(swb / sw - 1), "dswr", abs(swrb / swr - 1))
        assert nb == n and n == int((one["idx"][b] >= 0).sum()) and n == (697, 0, 332)[b]       # (dst row 7 of sample 0 is NaN)
        assert dH <= bound and dg <= bound and abs(swb / sw - 1) <= bound and abs(swrb / swr - 1) <= bound


# ---- test 4: a synthetic scene -------------------------------------------------------------------------------------------------------------
def test_register_sweeps_on_a_synthetic_scene(dev):
    """One lattice world seen from four poses with small steps.  Rows fixed in the SENSOR frame ride along in every sweep: 150 inside
    min_range (the vehicle's own returns) and 150 flagged as ground at 5..9 m -- left in, they would pull every transform towards identity.
    World rows within 0.3 m of the min_range circle in any sweep are left out of the world, so no row changes sides between sweeps."""
    from deflow_amd.odometry import chain_poses, register_sweeps
    rng = np.random.default_rng(4)
    steps = [(0.001, -0.0015, 0.004, 0.10, -0.05, 0.02), (0.0012, -0.001, 0.0035, 0.11, -0.04, 0.015), (0.0008, -0.0012, 0.0045, 0.09, -0.06, 0.02)]
    poses = [np.eye(4)]
    for s in steps:                                   # T_k = exp(step) maps sweep k into sweep k + 1: pose_{k+1} = pose_k inv(T_k)
        poses.append(poses[-1] @ np.linalg.inv(reg_ref.se3_exp(s)))
    world = reg_ref.lattice(1500, seed=7).astype(np.float64)
    views = [world @ np.linalg.inv(P)[:3, :3].T + np.linalg.inv(P)[:3, 3] for P in poses]
    keep = np.all([np.abs(np.hypot(v[:, 0], v[:, 1]) - 3.0) > 0.3 for v in views], axis=0)
    ang = rng.uniform(0, 2 * np.pi, 300)
    rad = np.concatenate((rng.uniform(0.5, 2.5, 150), rng.uniform(5.0, 9.0, 150)))
    rider = np.stack((rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-1, 1, 300)), axis=1)
    lidars, ground = [], []
    for k, v in enumerate(views):
        perm = np.random.default_rng(30 + k).permutation(int(keep.sum()) + 300)
        pts = np.concatenate((v[keep], rider))[perm].astype(np.float32)
        flags = np.concatenate((np.zeros(int(keep.sum())), np.zeros(150), np.ones(150)))[perm].astype(np.uint8)
        lidars.append(np.concatenate((pts, np.ones((len(pts), 1), dtype=np.float32)), axis=1))       # [N, 4]: a column beyond xyz is ignored
        ground.append(flags)
    rep = {}
    rel = register_sweeps(lidars, ground, device=dev, report=rep, stride=2, levels=((1.0, 6),), **GRID)
    assert len(rel) == 3 and rep["failed"] == [] and rep["params"]["min_range"] == 3.0
    for k, T in enumerate(rel):
        want = np.linalg.inv(poses[k + 1]) @ poses[k]
        err = np.abs(T - want).max()
        print("pair", k, "|T - inv(pose_k+1) pose_k|max", err, "inliers", rep["inliers"][k])
        assert T.dtype == np.float64 and err <= TOL
    chained = chain_poses(rel)
    assert max(np.abs(c - p).max() for c, p in zip(chained, poses)) <= 4 * TOL        # three steps' errors, carried along the chain
    # a pair that cannot be registered keeps its initial transform and is reported
    rep2 = {}
    rel2 = register_sweeps([lidars[0], lidars[1][:20], lidars[2]], None, device=dev, report=rep2, stride=2, levels=((1.0, 2),), **GRID)
    assert [f["pair"] for f in rep2["failed"]] == [0, 1] and all(f["status"] == 2 for f in rep2["failed"])
    assert np.array_equal(rel2[0], np.eye(4)) and np.array_equal(rel2[1], np.eye(4))


# ---- test 5: the command ----------------------------------------------------------------------------------------------------------------
def test_command_writes_a_sidecar_the_reader_accepts(dev, tmp_path, golden_dir, capsys):
    from deflow_amd import odometry
    from deflow_amd.data import HDF5Dataset
    src = os.path.join(golden_dir, "av2_mini", "train")
    shutil.copy(os.path.join(src, "scene_a.h5"), tmp_path / "scene_a.h5")
    with open(os.path.join(src, "index_total.pkl"), "rb") as f:
        index = [e for e in pickle.load(f) if e[0] == "scene_a"]
    with open(tmp_path / "index_total.pkl", "wb") as f:
        pickle.dump(index, f)
    assert odometry.main([f"data_dir={tmp_path}", "min_inliers=5", "stride=1", "iters=2"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["scene"] == "scene_a" and line["sweeps"] == 25 and "failed_pairs" in line and "path_length" in line and "seconds" in line
    poses = odometry.read_sidecar(str(tmp_path / "scene_a.pose.npz"))
    assert len(poses) == 25
    for P in poses.values():           # the fixture's clouds carry no known motion: shape, dtype, finiteness, orthonormality only
        assert P.shape == (4, 4) and P.dtype == np.float64 and np.isfinite(P).all()
        assert np.abs(P[:3, :3] @ P[:3, :3].T - np.eye(3)).max() <= 1e-6
    with np.load(tmp_path / "scene_a.pose.npz", allow_pickle=False) as z:
        meta = json.loads(str(z["meta"]))
    assert meta["definition"] == "DESIGN.md 6r (UNPINNED)" and meta["stride"] == 1 and meta["min_inliers"] == 5
    ds = HDF5Dataset(str(tmp_path), pose_source="sidecar")
    item = ds[0]
    ts = sorted(poses, key=int)
    assert np.array_equal(item["pose0"].numpy(), poses[ts[0]]) and np.array_equal(item["pose1"].numpy(), poses[ts[1]])
    assert odometry.main([f"data_dir={tmp_path}"]) == 0             # a second run skips the scene
    assert "skipped" in json.loads(capsys.readouterr().out.strip().splitlines()[-1])


# ---- test 6: the guarded-call harness ---------------------------------------------------------------------------------------------------
_i, _o, _io = abi_sizes.i, abi_sizes.o, abi_sizes.io
REG_TABLE = {            # the sizes of the header's registration section, local to this file (abi_sizes.TABLE stays as it is)
    "df_nn_grid_build": abi_sizes.TABLE["df_nn_grid_build"],
    "df_reg_accumulate": abi_sizes._e(
        "src_rng src_sorted Gs dst_rng dst_sorted minx miny cell G B Ns stride T max_dist2 k2 partial q_out idx_out d2_out w_out",
        src_rng=_i("8 * B * Gs * Gs"), src_sorted=_i("16 * B * Ns"), dst_rng=_i("8 * B * G * G"),
        dst_sorted=abi_sizes.recorded("[B*Nd, 4] f32, and the entry does not receive Nd"), T=_i("128 * B"),
        partial=abi_sizes.ws("df_reg_ws_bytes", "B, Ns"), q_out=_o("12 * B * Ns", True), idx_out=_o("4 * B * Ns", True),
        d2_out=_o("4 * B * Ns", True), w_out=_o("4 * B * Ns", True)),
    "df_reg_solve": abi_sizes._e("partial B nblk min_inliers planar T log status",
                                 partial=_i("256 * B * nblk"), T=_io("128 * B", True), log=_o("16 * B"), status=_o("4 * B", True)),
}


def test_guarded_entries_write_nothing_outside_their_buffers(dev, monkeypatch):
    from deflow_amd import _lib, args, chamfer, odometry
    protos = abi_sizes.header_prototypes()
    for name in ("df_reg_accumulate", "df_reg_solve"):               # the local table against the header's prototypes
        assert [p.name for p in protos[name]][:-1] == list(REG_TABLE[name].params)
        for p in protos[name][:-1]:
            assert p.pointer == (p.name in REG_TABLE[name].bufs) and (not p.pointer or p.nullable == REG_TABLE[name].bufs[p.name].nullable)
    src, cs, dst, cd = to_dev(dev, *make_batch(nan_dst=True)[:4])
    init = torch.from_numpy(np.stack((np.eye(4), ARBITRARY, np.eye(4)))).to(dev)

    def scenario(stride):
        T, info = odometry.register(src, cs, dst, cd, init=init, stride=stride, levels=((1.0, 2),), rows=True, **GRID)
        return [T, info["status"], info["log"], info["q"], info["idx"], info["d2"], info["w"]]

    for stride in (1, 3):
        outs = [scenario(stride)]
        for fill in (0xA5, 0x7F):
            with monkeypatch.context() as m:
                g = guarded.Guard(fill, _lib.call, table=REG_TABLE)
                for mod in (odometry, chamfer, args):       # register's own entries, the grid build, the workspace query
                    m.setattr(mod, "call", g.call)
                    m.setattr(mod, "ptr", g.ptr)
                outs.append(scenario(stride))
            assert g.seen.count("df_reg_accumulate") == 3 and g.seen.count("df_reg_solve") == 3 and g.seen.count("df_nn_grid_build") == 2
        for a, b, c in zip(*outs):
            assert guarded.same_bits(a, b) and guarded.same_bits(a, c)
