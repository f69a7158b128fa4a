"""Restatement of the depth cube and of the map drop of include/deflow_amd.h / DESIGN.md section 6u -- bin, build, test, drop -- one
numpy float32 scalar at a time (every operation rounded once), a dict of bins and Python loops: no code shared with the kernels and none
with ``deflow_amd.visibility`` / ``deflow_amd.localmap``.  ``register_sweeps_carve`` is the scan-to-map loop of
``odometry.register_sweeps(target="map", map_carve=True, residual="plane")`` on plane_ref's float64 registration (stride 1) and map_ref's
map, and ``room_scene`` the ray-cast recording the carve tests register: a convex enclosure seen from a moving sensor, with a block that
crosses the view and occludes the walls behind it."""
from __future__ import annotations

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import map_ref  # noqa: E402
import plane_ref  # noqa: E402
import reg_ref  # noqa: E402

F = np.float32
EMPTY = 0x7F800000
INF32 = np.frombuffer(np.uint32(EMPTY).tobytes(), dtype=np.float32)[0]


def bits(v) -> int:
    return int(np.frombuffer(F(v).tobytes(), dtype=np.uint32)[0])


def unbits(b: int):
    return np.frombuffer(np.uint32(b).tobytes(), dtype=np.float32)[0]


# ---- the cube ---------------------------------------------------------------------------------------------------------------------------
def index(c, m, R: int) -> int:
    """min(R - 1, floor((c / m + 1) * (R / 2))): a division, an addition and a multiplication, each rounded to fp32"""
    u = F(c) / F(m)
    s = F(u + F(1.0))
    t = F(s * F(R // 2))
    return min(R - 1, int(math.floor(float(t))))


def bin_of(row, R: int):
    """(face, i, j, m) of one row, None where its coordinates keep it from taking part"""
    x, y, z = (F(v) for v in row)
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
        return None
    a = (abs(x), abs(y), abs(z))
    if a[0] >= a[1] and a[0] >= a[2]:
        axis = 0
    elif a[1] >= a[2]:
        axis = 1
    else:
        axis = 2
    major, m = (x, y, z)[axis], a[axis]
    if not m > 0:
        return None
    uc, vc = [c for k, c in enumerate((x, y, z)) if k != axis]
    return 2 * axis + (1 if major < 0 else 0), index(uc, m, R), index(vc, m, R), m


def build(points, count, mask, R: int) -> dict:
    """{(face, j, i): bits of the smallest depth} over the rows that take part; a bin without a row is absent (+inf)"""
    img = {}
    for r in range(min(int(count), len(points))):
        if mask is not None and not int(mask[r]) > 0:
            continue
        b = bin_of(points[r], R)
        if b is None:
            continue
        face, i, j, m = b
        img[(face, j, i)] = min(img.get((face, j, i), EMPTY), bits(m))
    return img


def image(img: dict, R: int) -> np.ndarray:
    """the dict as the entry's [6,R,R] u32"""
    out = np.full((6, R, R), EMPTY, dtype=np.uint32)
    for (face, j, i), v in img.items():
        out[face, j, i] = v
    return out


def test(query, count, img: dict, R: int, halo: int, margin, rel, near):
    """-> flag [M] int32, dmin [M] u32 (bits) of every query row"""
    M = len(query)
    flag, depth = np.zeros(M, dtype=np.int32), np.full(M, EMPTY, dtype=np.uint32)
    c = F(F(1.0) + F(rel))
    margin, near = F(margin), F(near)
    for r in range(min(int(count), M)):
        b = bin_of(query[r], R)
        if b is None:
            continue
        face, i, j, m = b
        if i - halo < 0 or i + halo > R - 1 or j - halo < 0 or j + halo > R - 1:
            continue
        dmin = min(img.get((face, jj, ii), EMPTY) for jj in range(j - halo, j + halo + 1) for ii in range(i - halo, i + halo + 1))
        depth[r] = dmin
        x, y = F(query[r][0]), F(query[r][1])
        if not max(abs(x), abs(y)) >= near or (face, j, i) not in img:
            continue
        lhs = F(F(m * c) + margin)
        flag[r] = 1 if lhs < unbits(dmin) else 0
    return flag, depth


def drop(map_pts, count, flag, gate=None):
    """-> (map_out [cap,3] f64 with a NaN tail, count_out, (tested, dropped)): the rows < count with flag == 0, in their order"""
    cap = map_pts.shape[0]
    cnt = max(0, min(int(count), cap))
    gated = gate is not None and int(gate) != 0
    stay = [j for j in range(cnt) if gated or int(flag[j]) == 0]
    out = np.full((cap, 3), map_ref.NAN64)
    for at, j in enumerate(stay):
        out[at] = map_pts[j]
    return out, len(stay), (0 if gated else cnt, cnt - len(stay))


def carve(map_pts, count, sweep, sweep_count, pose, *, mask=None, gate=None, res, halo, margin, rel, near):
    """one LocalMap.carve of one sample -> (map, count, stat, stages)"""
    dst = map_ref.view(map_pts, count, pose)
    img = build(sweep, sweep_count, mask, res)
    flag, depth = test(dst, count, img, res, halo, margin, rel, near)
    out, cnt, stat = drop(map_pts, count, flag, gate)
    return out, cnt, stat, dict(view=dst, img=img, flag=flag, depth=depth)


# ---- the room scene ---------------------------------------------------------------------------------------------------------------------
# (outward unit normal direction, offset n . x <= d) of the enclosure in the world: four tilted, mutually non-parallel walls and a lid
WALLS = (((1.0, 0.06, 0.10), 7.0), ((-1.0, 0.09, 0.05), 5.5), ((0.07, 1.0, -0.08), 6.0), ((-0.05, -1.0, 0.12), 5.0),
         ((0.04, -0.06, 1.0), 2.6))
ROOM = dict(sweeps=6, az_step=5.0, rings=tuple(-8.0 + 5.0 * r for r in range(15)), step=(0.22, 0.06, 0.02), yaw=0.008, pitch=0.002,
            block_half=(0.5, 0.5, 0.9), block_start=(3.4, -2.6, 0.1), block_step=(0.12, 1.0, 0.0),
            levels=((1.0, 6), (0.5, 6)), voxel=0.5, K=4, cap=4096, min_range=1.0, max_range=24.0,
            carve=dict(res=12, halo=1, margin=0.5, rel=0.02))
ROOM_W = math.ceil(ROOM["max_range"] / ROOM["voxel"]) + 1
NORMALS = dict(radius=plane_ref.RADIUS, min_pts=plane_ref.MIN_PTS, max_curv=plane_ref.MAX_CURV)


def room_truth(k: int) -> np.ndarray:
    T = reg_ref.se3_exp((0.0, ROOM["pitch"] * k, ROOM["yaw"] * k, 0.0, 0.0, 0.0))
    T[:3, 3] = np.asarray(ROOM["step"]) * k
    return T


def room_scene(n: int = ROOM["sweeps"]):
    """-> (sweeps, truth, is_object): per sweep an fp32 cloud [N,3] in the sensor's frame -- where the rays at sensor-fixed directions (an
    azimuth every az_step degrees on every ring) first hit the block or, behind it, the enclosure --, the sensor's pose, and which rows
    lie on the block.  The block moves by block_step per sweep: about its own width across the view, and a little along it."""
    az = np.radians(np.arange(0.0, 360.0, ROOM["az_step"]))
    el = np.radians(np.asarray(ROOM["rings"]))
    v = np.stack([np.stack((np.cos(e) * np.cos(az), np.cos(e) * np.sin(az), np.full_like(az, np.sin(e))), axis=1) for e in el]).reshape(-1, 3)
    sweeps, truth, is_object = [], [], []
    for k in range(n):
        T = room_truth(k)
        o, d = T[:3, 3], v @ T[:3, :3].T
        t_wall = np.full(len(v), np.inf)
        for nrm, off in WALLS:
            nn = np.asarray(nrm) / np.linalg.norm(nrm)
            den = d @ nn
            with np.errstate(divide="ignore"):
                t = np.where(den > 1e-12, (off - o @ nn) / den, np.inf)
            t_wall = np.minimum(t_wall, t)
        assert np.isfinite(t_wall).all() and (t_wall > 0).all()
        centre = np.asarray(ROOM["block_start"]) + k * np.asarray(ROOM["block_step"])
        lo, hi = centre - ROOM["block_half"], centre + ROOM["block_half"]
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - o) / d, (hi - o) / d
        tn, tf = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
        hit = (tn <= tf) & (tn > 0) & (tn < t_wall)
        t = np.where(hit, tn, t_wall)
        sweeps.append((v * t[:, None]).astype(np.float32))
        truth.append(T)
        is_object.append(hit)
    return sweeps, truth, is_object


def neighbours_chunked(p, ok, radius, chunk: int = 512) -> np.ndarray:
    """plane_ref.neighbours without the [N,N,3] temporary"""
    out = np.zeros((len(p), len(p)), dtype=bool)
    for s in range(0, len(p), chunk):
        with np.errstate(invalid="ignore"):
            out[s:s + chunk] = ((p[s:s + chunk, None, :] - p[None, :, :]) ** 2).sum(axis=2) <= float(radius) ** 2
    return out & ok[:, None] & ok[None, :]


def register_plane(src, dst, cnt, levels, init, min_inliers=50):
    """plane_ref.register_plane over the map's leading cnt rows -> (T, status)"""
    d = np.ascontiguousarray(dst[:max(cnt, 1)])
    used, dok = reg_ref.used_rows(src, len(src)), reg_ref.participating(d, cnt)
    nrm = plane_ref.normals(d, cnt, radius=NORMALS["radius"], min_pts=NORMALS["min_pts"], max_curv=NORMALS["max_curv"],
                            near=neighbours_chunked(np.where(dok[:, None], d.astype(np.float64), 0.0), dok, NORMALS["radius"]))
    T, status = init.copy(), 2
    for max_dist, n in levels:
        for _ in range(n):
            T, status, _ = plane_ref.iterate_plane(T, src, used, d, dok, nrm, max_dist, min_inliers)
    return T, status


def world_rows(sweep, pose) -> np.ndarray:
    """the float64 world rows df_map_keys makes of a sweep's rows"""
    return map_ref.keys(np.zeros((0, 3)), 0, sweep, len(sweep), None, None, pose, ROOM["voxel"], ROOM_W)[0]


def register_sweeps_carve(sweeps, is_object=None, *, cube=None, levels=ROOM["levels"], voxel=ROOM["voxel"], K=ROOM["K"], cap=ROOM["cap"],
                          W=ROOM_W, near=ROOM["min_range"], fail=(), perturb=None):
    """sweeps: fp32 arrays [N_i,3], every row taking part.  cube: None (no carving) or dict(res, halo, margin, rel).  fail: the later sweeps (1 ..)
    whose status is forced to 2.  -> dict: poses, status, maps = (map, count) after every sweep, carved = rows dropped per later sweep,
    stages per later sweep, and with is_object per later sweep: static = static rows dropped, old = (object rows at least two sweeps old
    in the map before the carve, those of them dropped), stable = whether the flags survive ``perturb`` on every coordinate of the view"""
    pose, start = np.eye(4), np.eye(4)
    birth = {}                                                         # world row -> (is object, sweep)

    def note(k, p):
        if is_object is not None:
            for w, obj in zip(world_rows(sweeps[k], p), is_object[k]):
                birth.setdefault(tuple(w), (bool(obj), k))

    note(0, pose)
    m, cnt, _ = map_ref.insert(np.full((cap, 3), map_ref.NAN64), 0, sweeps[0], len(sweeps[0]), pose, voxel, W, K)
    out = dict(poses=[pose], status=[], maps=[(m, cnt)], carved=[], stages=[], static=[], old=[], stable=[], overflow=[])
    for k, s in enumerate(sweeps[1:], start=1):
        T, status = register_plane(s, map_ref.view(m, cnt, pose), cnt, levels, start)
        if k in fail:
            status = 2
        if status != 0:
            T = start.copy()
        pose = pose @ T
        if cube is not None:
            m2, cnt2, stat, st = carve(m, cnt, s, len(s), pose, gate=status, near=near, **cube)
            if is_object is not None:
                who = [birth[tuple(w)] for w in m[:cnt]]
                gone = st["flag"][:cnt] == 1 if status == 0 else np.zeros(cnt, dtype=bool)
                out["static"].append(sum(1 for (obj, _), g in zip(who, gone) if g and not obj))
                aged = [g for (obj, b), g in zip(who, gone) if obj and b <= k - 2]
                out["old"].append((len(aged), int(sum(aged))))
            if perturb:
                same = True
                for sx in (-1.0, 1.0):
                    for sy in (-1.0, 1.0):
                        for sz in (-1.0, 1.0):
                            q = (st["view"].astype(np.float64) + np.array((sx, sy, sz)) * perturb).astype(np.float32)
                            same &= np.array_equal(test(q, cnt, st["img"], cube["res"], cube["halo"], cube["margin"], cube["rel"], near)[0],
                                                   st["flag"])
                out["stable"].append(bool(same))
            out["carved"].append(stat[1]), out["stages"].append(st)
            m, cnt = m2, cnt2
        note(k, pose)
        m, cnt, stat = map_ref.insert(m, cnt, s, len(s), pose, voxel, W, K, gate=status)
        out["poses"].append(pose), out["status"].append(status), out["maps"].append((m, cnt)), out["overflow"].append(stat[3])
        start = T
    return out


def pose_errors(poses, truth) -> float:
    return max(float(np.abs(P - T).max()) for P, T in zip(poses, truth))


# ---- the kernel cases -------------------------------------------------------------------------------------------------------------------
NEAR, MARGIN, REL = 3.0, 0.5, 0.02
SIGNS = [(a, b, c) for a in (1.0, -1.0) for b in (1.0, -1.0) for c in (1.0, -1.0)]


def centre_dir(face: int, i: int, j: int, R: int):
    """the direction through the centre of bin (i, j) of a face, major coordinate +-1"""
    u, v = (i + 0.5) / (R / 2) - 1.0, (j + 0.5) / (R / 2) - 1.0
    axis, sign = face // 2, -1.0 if face % 2 else 1.0
    d = [u, v]
    d.insert(axis, sign)
    return np.array(d)


def lhs_of(m) -> np.float32:
    """fadd(fmul(m, c), margin) at the cases' margin and rel"""
    return F(F(F(m) * F(F(1.0) + F(REL))) + F(MARGIN))


def special_rows() -> np.ndarray:
    """face ties with every sign pattern, signed zeros, u = +-1 and one ulp inside, the origin, rows that are not finite, 3e38"""
    rows = []
    for s in SIGNS:
        s = np.array(s)
        rows += [s * (5.0, 5.0, 1.0), s * (1.0, 5.0, 5.0), s * (5.0, 1.0, 5.0), s * (5.0, 5.0, 5.0)]
    one_in = float(np.nextafter(F(7.0), F(0.0)))
    rows += [(-0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-0.0, 2.0, 1.0), (4.0, -0.0, 0.0), (4.0, 0.0, -0.0), (0.0, -0.0, 6.0),
             (7.0, 7.0, -7.0), (7.0, -7.0, 7.0), (7.0, one_in, -one_in), (7.0, -one_in, one_in), (-7.0, one_in, 7.0),
             (np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf), (3e38, 1.0, 1.0), (3e38, 3e38, -3e38), (1.0, 3e38, 2.0),
             (9e-31, 9e-31, -1e-30)]
    return np.array(rows, dtype=np.float32)


def kernel_case(R: int, N: int, M: int, seed: int = 0):
    """-> dict(points [3,N,3], count [3], mask [3,N], query [3,M,3], count_q [3]) fp32 / int32.  Sample 0: the special rows in both clouds,
    threshold triples on three faces, an emptied bin, the face edges, ``near``, then random rows; sample 1: every point in ONE bin, a
    partial count and a mask; sample 2: no points at all."""
    rng = np.random.default_rng(seed)

    def random_rows(n, lo, hi):
        d = rng.normal(size=(n, 3))
        return d / np.abs(d).max(axis=1, keepdims=True) * rng.uniform(lo, hi, size=(n, 1))

    sp = special_rows()
    points = np.zeros((3, N, 3), dtype=np.float32)
    query = np.zeros((3, M, 3), dtype=np.float32)
    mask = np.ones((3, N), dtype=np.int32)
    pts, qs = [sp], [sp, sp * F(0.5)]
    mid = R // 2
    # the threshold: a return exactly at, one ulp behind and one ulp before fadd(fmul(m, c), margin) of a query of depth 4 in its bin
    for face, step in ((0, 0), (1, 1), (2, -1)):
        off = 2 if R < 32 else 8                                     # (clear of the special rows' bins about the face's centre)
        d = centre_dir(face, min(mid + off, R - 1), max(mid - off, 0), R)
        t = lhs_of(4.0)
        t = t if step == 0 else np.nextafter(t, F(np.inf) if step > 0 else F(0.0))
        pts.append((d * float(t))[None]), qs.append((d * 4.0)[None])
    # the face edges: bins 0, 1, 2 and R - 3 .. R - 1 along either index, returns far behind the queries
    edge = sorted({e for e in (0, 1, 2, R - 3, R - 2, R - 1) if 0 <= e < R})
    for face in (1, 3):                                              # (a horizontal major axis: ``near`` is out of the way)
        for e in edge:
            for d in (centre_dir(face, e, mid, R), centre_dir(face, mid, e, R)):
                pts.append((d * 40.0)[None]), qs.append((d * 3.5)[None])
    # ``near``: max(|x|, |y|) equal to it and one ulp below, with a return far behind
    below = float(np.nextafter(F(NEAR), F(0.0)))
    for x in (NEAR, below):
        qs.append(np.array([(x, 0.1 * x, 0.05 * x), (0.1 * x, -x, 0.05 * x), (0.2 * x, x, 3.0 * x)]))
    pts.append(np.array([(30.0, 3.0, 1.5), (3.0, -30.0, 1.5), (2.0, 10.0, 30.0)]))
    # two rows in one bin
    d = centre_dir(5, mid, min(mid + 1, R - 1), R)
    pts.append(np.stack((d * 21.0, d * 20.5)))
    qs.append((d * 6.0)[None])
    fixed_p, fixed_q = np.concatenate(pts), np.concatenate(qs)
    assert len(fixed_p) <= N - 100 and len(fixed_q) <= M - 100
    points[0, :len(fixed_p)] = fixed_p
    points[0, len(fixed_p):] = random_rows(N - len(fixed_p), 20.0, 30.0)
    query[0, :len(fixed_q)] = fixed_q
    query[0, len(fixed_q):] = random_rows(M - len(fixed_q), 2.0, 35.0)
    # own bin empty, the neighbours full: every random point of one bin is masked off, returns go around it, a query goes into it
    hole = (0, mid - 1, mid - 1) if R >= 4 else None
    if hole is not None:
        k = N - 1
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                if (di or dj) and 0 <= hole[1] + di < R and 0 <= hole[2] + dj < R:
                    points[0, k] = centre_dir(0, hole[1] + di, hole[2] + dj, R) * 25.0
                    k -= 1
        for r in range(len(fixed_p), N):
            b = bin_of(points[0, r], R)
            if b is not None and b[:3] == hole:
                mask[0, r] = 0
        query[0, M - 1] = centre_dir(*hole, R) * 5.0
    mask[0, len(fixed_p) + 3] = -2
    mask[0, len(fixed_p) + 4] = 0
    # sample 1: every point in one bin; a masked nearest row, a count that cuts the nearest rows off
    d = centre_dir(2, mid, mid, R)
    depth = rng.uniform(10.0, 20.0, size=N)
    depth[7], depth[N - 3] = 8.0, 6.0                                # masked off / beyond the count
    points[1] = d[None] * depth[:, None]
    mask[1, 7] = 0
    query[1] = random_rows(M, 2.0, 35.0)
    query[1, :40] = d[None] * np.linspace(6.0, 12.0, 40)[:, None]
    query[2] = random_rows(M, 2.0, 35.0)
    points[2] = random_rows(N, 20.0, 30.0)
    return dict(points=points, count=np.array([N, N - 5, 0], dtype=np.int32), mask=mask, query=query,
                count_q=np.array([M, M - 17, M], dtype=np.int32), hole=hole, fixed_q=len(fixed_q), fixed_p=len(fixed_p))
