"""A naive restatement of the ground segmenter's definition (include/deflow_amd.h) in numpy int64, written
independently of the kernels: quantise, cell minima, the chain of every cell, the mask.  Everything after the quantisation is integer, so
the tests compare with it by exact equality.

Two forms of the height map: `chain` follows ONE cell's chain of ancestors step by step in Python integers (form A; `height_map_cells`
runs it for every cell), `height_map` runs all cells at once with one numpy pass per step k (form B); tests/test_ground_cpu.py checks
that they agree."""
import numpy as np

EMPTY = 2 ** 31 - 1
DEFAULTS = dict(xy_min=(-51.2, -51.2), cell=0.5, dims=(205, 205), z_min=-5.0, z_unit=0.01, z_levels=1000, origin=(0.0, 0.0),
                seed_z=-0.33, rise=0.10, drop=0.15, widen=0.03, miss_cap=8, tol=0.15)


def params(**kw):
    p = dict(DEFAULTS)
    unknown = set(kw) - set(p)
    assert not unknown, unknown
    p.update(kw)
    return p


def units(v, z_unit):
    """a length in height levels: round(v / z_unit)"""
    return int(round(float(v) / float(z_unit)))


def quant(v, lo, k):
    """u = fp32(fp32(v - lo) * k): two separately rounded fp32 operations"""
    with np.errstate(all="ignore"):
        d = (np.asarray(v, dtype=np.float32) - np.float32(lo)).astype(np.float32)
        return (d * np.float32(k)).astype(np.float32)


def rows(points, count, p):
    """points [N,3] -> (takes_part bool [N], cx, cy, h int64 [N]; 0 where the row does not take part)"""
    pts = np.asarray(points, dtype=np.float32)
    Gx, Gy = p["dims"]
    H = p["z_levels"]
    kxy, kz = np.float32(1.0 / float(p["cell"])), np.float32(1.0 / float(p["z_unit"]))
    ux, uy, uz = quant(pts[:, 0], p["xy_min"][0], kxy), quant(pts[:, 1], p["xy_min"][1], kxy), quant(pts[:, 2], p["z_min"], kz)
    with np.errstate(all="ignore"):
        ok = (np.arange(len(pts)) < int(count)) & np.isfinite(pts).all(1)
        ok &= (ux >= 0) & (ux < np.float32(Gx)) & (uy >= 0) & (uy < np.float32(Gy)) & (uz >= 0) & (uz < np.float32(H))
    fl = lambda u: np.floor(np.where(ok, u, np.float32(0))).astype(np.int64)
    return ok, fl(ux), fl(uy), fl(uz)


def cell_min(points, count, p):
    """-> zmin int64 [Gy, Gx]"""
    Gx, Gy = p["dims"]
    ok, cx, cy, h = rows(points, count, p)
    z = np.full(Gy * Gx, EMPTY, dtype=np.int64)
    np.minimum.at(z, (cy * Gx + cx)[ok], h[ok])
    return z.reshape(Gy, Gx)


def origin_cell(p):
    """(ox, oy): the origin quantised like a row, each index clamped into the grid; seed likewise from seed_z"""
    Gx, Gy = p["dims"]
    kxy, kz = np.float32(1.0 / float(p["cell"])), np.float32(1.0 / float(p["z_unit"]))
    ox = int(min(max(np.floor(quant(p["origin"][0], p["xy_min"][0], kxy)), 0), Gx - 1))
    oy = int(min(max(np.floor(quant(p["origin"][1], p["xy_min"][1], kxy)), 0), Gy - 1))
    seed = int(np.floor(quant(p["seed_z"], p["z_min"], kz)))
    return ox, oy, seed


def thresholds(p):
    return tuple(units(p[k], p["z_unit"]) for k in ("rise", "drop", "widen", "tol"))


def clamp(v, lo, hi):
    return min(max(v, lo), hi)


def chain(zmin, cx, cy, p):
    """form A: one cell's chain in Python integers -> (height, observed, the ancestors in order)"""
    ox, oy, seed = origin_cell(p)
    RISE, DROP, WIDEN, _ = thresholds(p)
    cap = int(p["miss_cap"])
    dx, dy = cx - ox, cy - oy
    r = max(abs(dx), abs(dy))
    g, miss, acc, path = seed, cap, False, []
    for k in range(r + 1):
        ax, ay = ox + clamp(dx, -k, k), oy + clamp(dy, -k, k)
        path.append((ax, ay))
        z = int(zmin[ay, ax])
        w = WIDEN * min(miss, cap)
        acc = z != EMPTY and g - DROP - w <= z <= g + RISE + w
        if acc:
            g, miss = z, 0
        else:
            miss = min(miss + 1, cap)
    return g, int(acc), path


def height_map_cells(zmin, p):
    """form A for every cell -> (height int64 [Gy,Gx], observed uint8 [Gy,Gx])"""
    Gx, Gy = p["dims"]
    height, obs = np.zeros((Gy, Gx), dtype=np.int64), np.zeros((Gy, Gx), dtype=np.uint8)
    for cy in range(Gy):
        for cx in range(Gx):
            height[cy, cx], obs[cy, cx], _ = chain(zmin, cx, cy, p)
    return height, obs


def height_map(zmin, p):
    """form B: all cells at once, one pass per step k"""
    Gx, Gy = p["dims"]
    ox, oy, seed = origin_cell(p)
    RISE, DROP, WIDEN, _ = thresholds(p)
    cap = int(p["miss_cap"])
    dy, dx = np.meshgrid(np.arange(Gy, dtype=np.int64) - oy, np.arange(Gx, dtype=np.int64) - ox, indexing="ij")
    r = np.maximum(np.abs(dx), np.abs(dy))
    g = np.full((Gy, Gx), seed, dtype=np.int64)
    miss = np.full((Gy, Gx), cap, dtype=np.int64)
    acc = np.zeros((Gy, Gx), dtype=bool)
    for k in range(int(r.max()) + 1):
        live = r >= k
        z = zmin[oy + np.clip(dy, -k, k), ox + np.clip(dx, -k, k)]
        w = WIDEN * np.minimum(miss, cap)
        a = (z != EMPTY) & (g - DROP - w <= z) & (z <= g + RISE + w)
        g = np.where(live & a, z, g)
        miss = np.where(live, np.where(a, 0, np.minimum(miss + 1, cap)), miss)
        acc = np.where(live, a, acc)
    return g, acc.astype(np.uint8)


def mask_of(points, count, height, p):
    """-> uint8 [N]: the row takes part and h <= height[cell] + TOL"""
    ok, cx, cy, h = rows(points, count, p)
    TOL = thresholds(p)[3]
    return (ok & (h <= height[cy, cx] + TOL)).astype(np.uint8)


def segment(points, count, **kw):
    """points [B,N,3], count [B] -> dict(cell_min int64 [B,Gy,Gx], height int64 [B,Gy,Gx], observed uint8 [B,Gy,Gx], mask uint8 [B,N])"""
    p = params(**kw)
    zs, hs, os_, ms = [], [], [], []
    for pts, c in zip(np.asarray(points, dtype=np.float32), count):
        z = cell_min(pts, c, p)
        hgt, obs = height_map(z, p)
        zs.append(z), hs.append(hgt), os_.append(obs), ms.append(mask_of(pts, c, hgt, p))
    return dict(cell_min=np.stack(zs), height=np.stack(hs), observed=np.stack(os_), mask=np.stack(ms))


def segment_sweep(lidar, **kw):
    """one sweep [N, >=3] with all of its rows -> uint8 [N]"""
    pts = np.ascontiguousarray(np.asarray(lidar)[:, :3], dtype=np.float32)
    if pts.shape[0] == 0:
        return np.zeros(0, dtype=np.uint8)
    return segment(pts[None], [pts.shape[0]], **kw)["mask"][0]
