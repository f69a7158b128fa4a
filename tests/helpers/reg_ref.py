"""Float64 numpy restatement of the sweep-to-sweep registration of include/deflow_amd.h / DESIGN.md section 6r: all-pairs search, q formed
in float64, every sum in float64.  Also the lattice cloud the odometry tests register: correspondences that are unambiguous in fp32 and
in float64 alike, so that the GPU result and this restatement can be held against the TRUE motion."""
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


def solve(H, g, inliers, min_inliers, planar):
    """-> (status, delta): 2 too few inliers, 3 a Cholesky pivot of a solved-for row <= 1e-9 x the largest diagonal entry, else 0"""
    if inliers < min_inliers:
        return 2, None
    H, g = H.copy(), g.copy()
    first = 2 if planar else 0
    dmax = max(H[i, i] for i in range(first, 6))
    for i in range(first):
        H[i, :] = 0.0
        H[:, i] = 0.0
        H[i, i] = 1.0
        g[i] = 0.0
    L = np.zeros((6, 6))
    for j in range(6):
        d = H[j, j] - (L[j, :j] ** 2).sum()
        if j >= first and not d > PIVOT_REL * dmax:
            return 3, None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (H[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.linalg.solve(L, -g)
    return 0, np.linalg.solve(L.T, y)


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
