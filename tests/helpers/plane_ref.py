"""Float64 numpy restatement of the point-to-plane part of the sweep-to-sweep registration (include/deflow_amd.h):
all-pairs neighbour sets, normals from ``numpy.linalg.eigh`` (which shares no code with the kernel's Jacobi), the header's sign and
validity rules, one plane iteration on top of reg_ref's ``solve`` / ``se3_exp`` / ``pack_slab``, and ``register_plane``.

Also the planar scene the plane tests register: four mutually non-parallel planes sampled at positions that are fixed in the SENSOR
frame, which is what a spinning LiDAR does to walls and ground.  The second sweep samples the moved planes at the same sensor-frame
positions, so every row's nearest target row is "itself" and a point-to-point fit returns (almost) no motion, while the planes
determine all six degrees of freedom."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reg_ref  # noqa: E402


# ---- normals ----------------------------------------------------------------------------------------------------------------------------
def neighbours(points, ok, radius) -> np.ndarray:
    """bool [N,N]: row j is a neighbour of row i -- both take part and |p_j - p_i|^2 <= radius^2 in float64 (i itself included)"""
    p = np.asarray(points, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        near = d2 <= float(radius) ** 2
    return near & ok[:, None] & ok[None, :]


def pair_margin(points, ok, radius) -> float:
    """the smallest | |p_j - p_i| - radius | over the participating pairs: how far every pair is from changing sides in fp32"""
    p = np.asarray(points, dtype=np.float64)[ok]
    d = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2))
    return float(np.abs(d - radius).min())


def eig_sym3(C, later_axis=True):
    """ascending eigenvalues and unit eigenvectors (columns) of the symmetric C [3,3].  An axis whose off-diagonal entries are exactly 0
    is an exact eigenvector with its diagonal entry (the header: a rotation whose off-diagonal entry is exactly 0 is skipped), the rest
    comes from numpy.linalg.eigh of what is left.  On exactly equal eigenvalues the later axis comes first, as the header orders them
    (later_axis=False: the earlier one -- a deliberately wrong variant)."""
    free = [k for k in range(3) if all(C[k, j] == 0 for j in range(3) if j != k)]
    if len(free) == 3 or len(free) == 1:
        rest = [k for k in range(3) if k not in free] if len(free) == 1 else []
        lam, vec, axis = [C[k, k] for k in free], [np.eye(3)[k] for k in free], list(free)
        if rest:
            l2, v2 = np.linalg.eigh(C[np.ix_(rest, rest)])
            for c in range(2):
                v = np.zeros(3)
                v[rest] = v2[:, c]
                lam.append(l2[c]), vec.append(v), axis.append(-1)
        order = sorted(range(3), key=lambda c: (lam[c], -axis[c] if later_axis else axis[c]))
        return np.array([lam[c] for c in order]), np.stack([vec[c] for c in order], axis=1)
    return np.linalg.eigh(C)


def normals(points, count, mask=None, *, radius, min_pts, max_curv, diff32=False, near=None, later_axis=True, tie_break=True):
    """-> dict: n [N,3] f64 (0 where not valid), curv [N] (-1 where not valid), m [N] int, valid [N] bool, lam [N,3] the ascending
    eigenvalues, curv_all [N] = lambda0 / trace of every row with m >= 1 and trace > 0 (nan elsewhere), whatever its validity, and
    cov [N,3,3] the covariances.  The differences from the row are exact (float64) or, with diff32, fp32(v - p) as the header forms
    them.  curv <= max_curv is decided on the fp32 values, as the header states it.  near: a neighbour matrix to use instead of the
    all-pairs one (rows that do not take part must be False in it); later_axis / tie_break = False: deliberately wrong variants of the
    header's rules, for the tests that show a case bites (without the tie-break the raw eigenvector is taken with its largest component
    negative, which a solver is free to return, and only n . p > 0 flips it)."""
    p = np.asarray(points, dtype=np.float64)
    p32 = np.asarray(points, dtype=np.float32)
    N = p.shape[0]
    ok = reg_ref.participating(points, count, mask)
    if near is None:
        near = neighbours(np.where(ok[:, None], p, 0.0), ok, radius)
    out = dict(n=np.zeros((N, 3)), curv=np.full(N, -1.0), m=near.sum(axis=1).astype(np.int64), valid=np.zeros(N, dtype=bool),
               lam=np.full((N, 3), np.nan), curv_all=np.full(N, np.nan), cov=np.full((N, 3, 3), np.nan))
    for i in np.flatnonzero(ok):
        x = (p32[near[i]] - p32[i]).astype(np.float64) if diff32 else p[near[i]] - p[i]
        if x.shape[0] == 0:
            continue
        mean = x.mean(axis=0)
        C = x.T @ x / x.shape[0] - np.outer(mean, mean)
        lam, vec = eig_sym3(C, later_axis)
        out["lam"][i], out["cov"][i] = lam, C
        trace = lam.sum()
        if not trace > 0:
            continue
        curv = max(lam[0] / trace, 0.0)
        out["curv_all"][i] = curv
        if out["m"][i] < min_pts or not np.float32(curv) <= np.float32(max_curv):
            continue
        n = vec[:, 0]
        if not tie_break and n[np.argmax(np.abs(n))] > 0:
            n = -n
        dot = float(n @ p[i])
        lead = n[np.flatnonzero(n != 0)[0]]
        if dot > 0 or (tie_break and dot == 0 and lead < 0):
            n = -n
        out["n"][i], out["curv"][i], out["valid"][i] = n + 0.0, curv, True          # (+ 0.0: a negated zero component is +0)
    return out


# ---- one plane iteration ----------------------------------------------------------------------------------------------------------------
def rows_plane(q, d, n) -> tuple:
    """a [k,6] = (q x n, n) and e [k] = n . (q - d) of the pairs, float64"""
    q, d, n = (np.asarray(a, dtype=np.float64) for a in (q, d, n))
    return np.hstack((np.cross(q, n), n)), ((q - d) * n).sum(axis=1)


def sums_plane(q, d, n, w):
    """the 30 sums of the inliers q [k,3] with partners d [k,3], normals n [k,3] and weights w [k] -> H [6,6], g [6], sw, swe2, k"""
    a, e = rows_plane(q, d, n)
    w = np.asarray(w, dtype=np.float64)
    H = (a * w[:, None]).T @ a
    g = (a * (w * e)[:, None]).sum(axis=0)
    return H, g, float(w.sum()), float((w * e * e).sum()), int(a.shape[0])


def iterate_plane(T, src, src_used, dst, dst_ok, nrm, max_dist, min_inliers=50, planar=False):
    """one iteration at state T with the target's normals nrm (the dict of ``normals``) -> (T', status, slab row [32])"""
    q = src[src_used].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    d2, j = reg_ref.nearest(q, dst, dst_ok)
    k2 = (max_dist / 3.0) ** 2
    inl = (d2 <= max_dist ** 2) & (j >= 0)
    inl[inl] &= nrm["valid"][j[inl]]
    qi, di, ni = q[inl], dst[j[inl]].astype(np.float64), nrm["n"][j[inl]]
    _, e = rows_plane(qi, di, ni)
    w = (k2 / (k2 + e * e)) ** 2
    H, g, sw, swe2, k = sums_plane(qi, di, ni, w)
    status, delta = reg_ref.solve(H, g, k, min_inliers, planar)
    return (reg_ref.se3_exp(delta) @ T if status == 0 else T), status, reg_ref.pack_slab(H, g, sw, swe2, k)


def register_plane(src, count_s, dst, count_d, levels, *, radius, min_pts, max_curv, init=None, mask_s=None, mask_d=None, min_inliers=50,
                   planar=False):
    """levels: (max_dist, iterations) pairs, stride 1 -> (T, status of the last iteration)"""
    T = np.eye(4) if init is None else np.asarray(init, dtype=np.float64).copy()
    used, dok = reg_ref.used_rows(src, count_s, mask_s), reg_ref.participating(dst, count_d, mask_d)
    nrm = normals(dst, count_d, mask_d, radius=radius, min_pts=min_pts, max_curv=max_curv)
    status = 2
    for max_dist, n in levels:
        for _ in range(n):
            T, status, _ = iterate_plane(T, src, used, dst, dok, nrm, max_dist, min_inliers, planar)
    return T, status


# ---- the planar scene -------------------------------------------------------------------------------------------------------------------
PLANES = (((1.0, 0.0, 0.1), 10.0, (13, 7)), ((0.05, 1.0, 0.0), 8.0, (13, 7)), ((0.0, 0.08, 1.0), -1.5, (17, 17)),
          ((1.0, 1.0, 0.2), -9.0, (13, 7)))                                # (direction of the unit normal, offset n . x, lattice)
MOTION = (0.0, 0.0, 0.03, 0.25, -0.12, 0.05)                              # 0.03 rad of yaw and (0.25, -0.12, 0.05) m
MOTION_PLANAR = (0.0, 0.0, 0.03, 0.25, -0.12, 0.0)
SEED = 0
ROWS = sum(a * b for _, _, (a, b) in PLANES)                              # 562: three blocks of 256, the last one partial
RADIUS, CELL, RANGE = 1.6, 2.0, (-24.0, -24.0, 24.0, 24.0)                # the tests' neighbourhood and grid (G = 24)
MIN_PTS, MAX_CURV = 5, 1e-5
LEVELS = ((2.0, 8), (1.0, 8), (0.5, 8))                                  # the command's default schedule


def _frame(direction):
    """unit normal and an in-plane orthonormal pair (u horizontal, v = n x u)"""
    n = np.asarray(direction, dtype=np.float64)
    n = n / np.linalg.norm(n)
    u = np.cross((0.0, 0.0, 1.0), n) if abs(n[2]) < 0.9 else np.cross((0.0, 1.0, 0.0), n)
    u = u / np.linalg.norm(u)
    return n, u, np.cross(n, u)


def planar_sweeps(transforms, seed: int = SEED):
    """One fp32 cloud [562,3] per 4 x 4 transform.  The samples: on every plane of PLANES an in-plane 1 m lattice centred at the plane's
    foot point, each node jittered in the plane by +-0.2 m per axis.  A sweep's cloud is the planes moved by its transform (x -> R x + t
    holds for the SURFACES), sampled at the same sensor-frame positions: the orthogonal projection of the float64 samples onto the moved
    planes, in the same row order."""
    rng = np.random.default_rng(seed)
    clouds = [[] for _ in transforms]
    for direction, off, (na, nb) in PLANES:
        n, u, v = _frame(direction)
        a, b = np.meshgrid(np.arange(na) - (na - 1) / 2.0, np.arange(nb) - (nb - 1) / 2.0, indexing="ij")
        ab = np.stack((a, b), axis=-1).reshape(-1, 2) + rng.uniform(-0.2, 0.2, size=(na * nb, 2))
        s = off * n + ab[:, :1] * u + ab[:, 1:] * v
        for cloud, T in zip(clouds, transforms):
            n2 = T[:3, :3] @ n
            off2 = off + float(n2 @ T[:3, 3])
            cloud.append(s - ((s @ n2) - off2)[:, None] * n2)
    return [np.concatenate(c).astype(np.float32) for c in clouds]


def planar_scene(seed: int = SEED, motion=MOTION):
    """-> (src [562,3] fp32, dst [562,3] fp32, T_true [4,4]): the sweeps of the identity and of T_true = exp(motion)"""
    T = reg_ref.se3_exp(motion)
    src, dst = planar_sweeps((np.eye(4), T), seed)
    return src, dst, T


def plane_of_row() -> np.ndarray:
    """[562] the index into PLANES of every row of planar_scene"""
    return np.concatenate([np.full(a * b, k) for k, (_, _, (a, b)) in enumerate(PLANES)])
