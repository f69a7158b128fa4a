"""Float64 numpy restatement of the sweep-to-sweep registration of include/deflow_amd.h / DESIGN.md section 6r: all-pairs search, q formed
in float64, every sum in float64.  Also the lattice cloud the odometry tests register: correspondences that are unambiguous in fp32 and
in float64 alike, so that the GPU result and this restatement can be held against the TRUE motion.

Which helper is what.  RESTATEMENTS of the kernel's own formulas, in float64 -- they agree with the kernel by construction and cannot show
that a formula is wrong: ``se3_exp`` (the same A, B, C, the same series, the same threshold), ``solve`` (the same Cholesky and
substitutions), ``sums``, ``iterate``, ``register``.  INDEPENDENT of the kernel -- what df_reg_solve is pinned against:
``se3_exp_indep`` (torch.linalg.matrix_exp of the 4 x 4 twist: no A, B, C, no series, no threshold), ``solve_hp`` (``solve``'s
elimination in np.longdouble, the header's status rules) and ``solve_ref`` (the two put together).  ``pack_slab`` / ``unpack_slab`` /
``split_slab`` write and read the header's slab layout, so that a test can hand df_reg_solve a slab of its own."""
from __future__ import annotations

import numpy as np

SERIES_THETA = 1e-2
PIVOT_REL = 1e-9


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(delta) -> np.ndarray:
    """exp of (omega, v): R = I + A K + B K^2, t = (I + B K + C K^2) v"""
    delta = np.asarray(delta, dtype=np.float64)
    w, v = delta[:3], delta[3:]
    th2 = float(w @ w)
    th = np.sqrt(th2)
    if th < SERIES_THETA:
        A = 1.0 + th2 * (-1.0 / 6.0 + th2 * (1.0 / 120.0 - th2 / 5040.0))
        B = 0.5 + th2 * (-1.0 / 24.0 + th2 * (1.0 / 720.0 - th2 / 40320.0))
        C = 1.0 / 6.0 + th2 * (-1.0 / 120.0 + th2 * (1.0 / 5040.0 - th2 / 362880.0))
    else:
        A, B, C = np.sin(th) / th, 2.0 * np.sin(0.5 * th) ** 2 / th2, (th - np.sin(th)) / (th2 * th)
    K = hat(w)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * (K @ K)
    T[:3, 3] = (np.eye(3) + B * K + C * (K @ K)) @ v
    return T


def participating(points, count, mask=None) -> np.ndarray:
    p = np.asarray(points, dtype=np.float64)
    ok = (np.arange(p.shape[0]) < int(count)) & np.isfinite(p).all(axis=1)
    if mask is not None:
        ok &= np.asarray(mask) > 0
    return ok


def nearest(q, dst, dst_ok):
    """(d2, j) of every row of q among the participating rows of dst, the lowest row on equal distances; inf / -1 without one"""
    n = q.shape[0]
    rows = np.flatnonzero(dst_ok)
    if rows.size == 0 or n == 0:
        return np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    d = ((q[:, None, :] - dst[None, rows, :].astype(np.float64)) ** 2).sum(axis=2)
    k = d.argmin(axis=1)                      # (numpy's argmin takes the first minimum: the lowest row)
    return d[np.arange(n), k], rows[k]


def sums(q, dstj, w):
    """the 30 sums of the inliers given as q [n,3], their partners dstj [n,3] and weights w [n], float64 -> H [6,6], g [6], sw, swr, n"""
    q, dstj, w = (np.asarray(a, dtype=np.float64) for a in (q, dstj, w))
    r = q - dstj
    H, g = np.zeros((6, 6)), np.zeros(6)
    for qi, ri, wi in zip(q, r, w):
        J = np.hstack((-hat(qi), np.eye(3)))
        H += wi * (J.T @ J)
        g += wi * (J.T @ ri)
    return H, g, float(w.sum()), float((w * (r * r).sum(axis=1)).sum()), int(q.shape[0])


def _cholesky_solve(H, g, inliers, min_inliers, planar, dtype):
    """the header's solve in ``dtype`` -> (status, delta, smallest solved-for pivot / largest solved-for diagonal entry)"""
    if not inliers >= min_inliers:                      # (a NaN count is "fewer than")
        return 2, None, None
    H, g = np.array(H, dtype=dtype), np.array(g, dtype=dtype)
    first = 2 if planar else 0
    dmax = max(H[i, i] for i in range(first, 6)) if np.isfinite(np.diag(H)[first:]).all() else dtype(np.nan)
    for i in range(first):
        H[i, :] = 0
        H[:, i] = 0
        H[i, i] = 1
        g[i] = 0
    if not np.isfinite(dmax):
        return 3, None, None
    L, ratio = np.zeros((6, 6), dtype=dtype), np.inf
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j in range(6):
            d = H[j, j] - (L[j, :j] ** 2).sum()
            if j >= first:
                if not d > dtype(PIVOT_REL) * dmax:
                    return 3, None, (float(d / dmax) if dmax > 0 else 0.0)
                ratio = min(ratio, float(d / dmax))
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                L[i, j] = (H[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
        y, x = np.zeros(6, dtype=dtype), np.zeros(6, dtype=dtype)
        for i in range(6):
            y[i] = (-g[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
        for i in range(5, -1, -1):
            x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    if not np.isfinite(x).all():
        return 3, None, ratio
    return 0, x, ratio


def solve(H, g, inliers, min_inliers, planar):
    """-> (status, delta): 2 too few inliers, 3 a Cholesky pivot of a solved-for row <= 1e-9 x the largest diagonal entry (or anything not
    finite), else 0.  Float64: a restatement of the kernel's elimination."""
    status, delta, _ = _cholesky_solve(H, g, inliers, min_inliers, planar, np.float64)
    return status, delta


def solve_hp(H, g, inliers, min_inliers, planar):
    """``solve`` in np.longdouble, the same status rules -> (status, delta in longdouble)"""
    status, delta, _ = _cholesky_solve(H, g, inliers, min_inliers, planar, np.longdouble)
    return status, delta


def pivot_ratio(H, planar=False):
    """the smallest solved-for Cholesky pivot (the failing one, if one fails) over the largest solved-for diagonal entry, float64; None
    where H's diagonal is not finite"""
    return _cholesky_solve(H, np.zeros(6), 0, 0, planar, np.float64)[2]


# ---- the slab of df_reg_solve ---------------------------------------------------------------------------------------------------------
SLAB = 32
_TRIU = np.triu_indices(6)


def pack_slab(H, g, sw, swr, n) -> np.ndarray:
    """the header's slab row [32] f64: 0..20 the upper triangle of H row by row, 21..26 g, 27 sum w, 28 sum w d2, 29 the inliers, 30 = 31 = 0"""
    S = np.zeros(SLAB)
    S[:21] = np.asarray(H, dtype=np.float64)[_TRIU]
    S[21:27] = np.asarray(g, dtype=np.float64)
    S[27], S[28], S[29] = sw, swr, n
    return S


def unpack_slab(S):
    """-> H [6,6] (symmetric), g [6], sw, swr, n: the inverse of pack_slab (columns 30, 31 are not looked at)"""
    S = np.asarray(S, dtype=np.float64)
    H = np.zeros((6, 6))
    H[_TRIU] = S[:21]
    H = H + np.triu(H, 1).T
    return H, S[21:27].copy(), float(S[27]), float(S[28]), float(S[29])


def sum_rows(rows) -> np.ndarray:
    """[nblk,32] -> [32]: the rows added to 0.0 one after the other in ascending order, float64 -- the header's order"""
    s = np.zeros(SLAB)
    for r in np.asarray(rows, dtype=np.float64):
        s = s + r
    return s


def sum_rows_pairwise(rows) -> np.ndarray:
    """the rows added as a balanced tree: NOT the header's order (what a test holds the ascending sum apart from)"""
    rows = np.asarray(rows, dtype=np.float64)
    if rows.shape[0] == 1:
        return rows[0].copy()
    h = (rows.shape[0] + 1) // 2
    return sum_rows_pairwise(rows[:h]) + sum_rows_pairwise(rows[h:])


def split_slab(S, nblk, scale=2.0 ** 40, seed=0) -> np.ndarray:
    """one slab row spread over nblk rows [nblk,32]: random positive shares of S, and for nblk >= 2 the offset + scale * S in row 0,
    - scale * S in row 2 (row 1 of two or three).  The offsets cancel, but a share added while an offset is in the partial sum loses
    log2(scale) of its bits: in ascending order that is row 1's alone, from the other end or in a tree it is other rows' too, so the
    value of the sum depends on the ORDER of the additions (sum_rows is the header's); it is close to S, not equal to it."""
    S = np.asarray(S, dtype=np.float64)
    if nblk == 1:
        return S[None].copy()
    share = np.random.default_rng(seed).uniform(0.5, 1.5, size=nblk)
    rows = (share / share.sum())[:, None] * S[None]
    rows[0] += scale * S
    rows[1 if nblk <= 3 else 2] -= scale * S
    return rows


# ---- the independent reference of df_reg_solve ------------------------------------------------------------------------------------------
EXP_V0_THETAS = (0.0, 0.3)            # the thetas at which the exponential tests also run v = 0 (see se3_exp_indep)


def se3_exp_indep(delta) -> np.ndarray:
    """exp of the 4 x 4 twist [[hat(omega), v], [0, 0]] by torch.linalg.matrix_exp in float64: shares no formula with the kernel.
    Its own error, measured about a coordinate axis against cos / sin: below 4e-16, except where the norm of the whole twist is around
    1e-2, i.e. v = 0 and theta = 0.0099 (7.7e-14) or 0.0101 (8.6e-14) -- over the 64 ulp the tests allow at max|T| = 1, which is why
    they take v = 0 at EXP_V0_THETAS only."""
    import torch
    delta = np.asarray(delta, dtype=np.float64)
    X = np.zeros((4, 4))
    X[:3, :3] = hat(delta[:3])
    X[:3, 3] = delta[3:]
    return torch.linalg.matrix_exp(torch.from_numpy(X)).numpy()


def solve_ref(S, min_inliers, planar, T0):
    """what df_reg_solve owes for the summed slab row S [32] at state T0 [4,4] -> (status, T, log [4] f64): delta from solve_hp rounded to
    float64, T = se3_exp_indep(delta) @ T0 (T0 itself unless status 0), log = (inliers, sum w d2 / sum w or 0, |omega|, |v|) by the header"""
    H, g, sw, swr, n = unpack_slab(S)
    T0 = np.asarray(T0, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        log = np.array([n, swr / sw if sw > 0 else 0.0, 0.0, 0.0])
    status, delta = solve_hp(H, g, n, min_inliers, planar)
    if status != 0:
        return status, T0.copy(), log
    delta = delta.astype(np.float64)
    log[2], log[3] = np.sqrt(delta[:3] @ delta[:3]), np.sqrt(delta[3:] @ delta[3:])
    return 0, se3_exp_indep(delta) @ T0, log


def iterate(T, src, src_used, dst, dst_ok, max_dist, min_inliers=50, planar=False):
    """one iteration at state T -> (T', status, (inliers, mean residual))"""
    q = src[src_used].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d2, j = nearest(q, dst, dst_ok)
    k2 = (max_dist / 3.0) ** 2
    inl = d2 <= max_dist ** 2
    w = (k2 / (k2 + d2[inl])) ** 2
    H, g, sw, swr, n = sums(q[inl], dst[j[inl]], w)
    status, delta = solve(H, g, n, min_inliers, planar)
    mean = swr / sw if sw > 0 else 0.0
    return (se3_exp(delta) @ T if status == 0 else T), status, (n, mean)


def used_rows(src, count, mask=None) -> np.ndarray:
    """stride = 1: every participating row (the subsample of a larger stride follows the cell order of the GPU's grid)"""
    return participating(src, count, mask)


def register(src, count_s, dst, count_d, levels, init=None, mask_s=None, mask_d=None, min_inliers=50, planar=False):
    """levels: (max_dist, iterations) pairs, stride 1 -> (T, status of the last iteration)"""
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()
    used, dok = used_rows(src, count_s, mask_s), participating(dst, count_d, mask_d)
    status = 2
    for max_dist, n in levels:
        for _ in range(n):
            T, status, _ = iterate(T, src, used, dst, dok, max_dist, min_inliers, planar)
    return T, status


# ---- the lattice cloud ------------------------------------------------------------------------------------------------------------------
MOTION = (0.001, -0.0015, 0.004, 0.10, -0.05, 0.02)          # moves every row of the lattice cloud by at most 0.25 m
MOTION_PLANAR = (0.0, 0.0, 0.004, 0.10, -0.05, 0.0)


def lattice(n: int, seed: int = 0) -> np.ndarray:
    """n nodes of the 1 m lattice in [-20,20]^2 x [-2,2], each jittered by +-0.2 per axis, fp32 [n,3]: distinct rows are >= 0.6 m apart"""
    rng = np.random.default_rng(seed)
    gx, gy, gz = np.meshgrid(np.arange(-20, 21), np.arange(-20, 21), np.arange(-2, 3), indexing="ij")
    nodes = np.stack((gx, gy, gz), axis=-1).reshape(-1, 3).astype(np.float64)
    pick = rng.choice(nodes.shape[0], size=n, replace=False)
    return (nodes[pick] + rng.uniform(-0.2, 0.2, size=(n, 3))).astype(np.float32)


def moved(points, T, seed: int = 1) -> np.ndarray:
    """the rows moved by T (float64), rounded to fp32, in permuted row order"""
    p = np.asarray(points, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]
    return p[np.random.default_rng(seed).permutation(p.shape[0])].astype(np.float32)


MOTION_TURN = (0.001, -0.0015, 0.012, 0.10, -0.05, 0.02)     # MOTION with three times the yaw: |omega| = 0.0121, the closed-form branch


def base_sums():
    """the well-conditioned normal equations the df_reg_solve tests plant their steps in: ``sums`` of lattice(700, seed=0) against its
    rows moved by MOTION_TURN, at identity, gate 1.0 -> H, g, sw, swr, n (cond(H) = 268, diagonal ~ (4.7e4, 4.3e4, 8.8e4, 380, 380, 380))"""
    src = lattice(700, seed=0)
    dst = moved(src, se3_exp(MOTION_TURN))
    q = src.astype(np.float64)
    d2, j = nearest(q, dst, np.ones(len(dst), dtype=bool))
    inl = d2 <= 1.0
    k2 = (1.0 / 3.0) ** 2
    return sums(q[inl], dst[j[inl]].astype(np.float64), (k2 / (k2 + d2[inl])) ** 2)
