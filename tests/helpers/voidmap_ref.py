"""A naive restatement of the void map's definition (include/deflow_amd.h) in numpy int64 / bool, written
independently of the kernels: quantise, walk, truncate, margin, occupied bits, erosion by padded shifts, the map, the flags.  Everything
after the quantisation is integer, so the tests compare with it by exact equality.

Two forms of the walk: `walk` follows ONE ray step by step in Python integers (the form the hand-computed cases read), `sweep_bits` walks
all rays of a sweep at once, one numpy operation per step; tests/test_voidmap_cpu.py checks that they agree."""
import numpy as np

SUB = 256
QMAX = float(2 ** 30)


def ray_limit(max_range, voxel):
    return int(round(float(max_range) / float(voxel) * SUB))


def k_of(voxel):
    return np.float32(SUB / float(voxel))


def quantise(p, gmin, k):
    """p [..., 3] -> (q int64 [..., 3], takes_part bool [...]): u = fp32(fp32(p - gmin) * k), q = floor(u)"""
    p = np.asarray(p, dtype=np.float32)
    with np.errstate(all="ignore"):
        diff = (p - np.asarray(gmin, dtype=np.float32)).astype(np.float32)
        u = (diff * np.float32(k)).astype(np.float32)
        ok = np.isfinite(p).all(-1) & (np.abs(u) < QMAX).all(-1)
    q = np.floor(np.where(ok[..., None], u, np.float32(0))).astype(np.int64)
    return q, ok


def walk(A, E, R, hit_margin):
    """one ray in Python integers: -> (visited voxels in order, set flag per visit (before the inside-the-grid test), truncated, e)"""
    A, E = [int(v) for v in A], [int(v) for v in E]
    d = [E[k] - A[k] for k in range(3)]
    m = max(abs(v) for v in d)
    cut = m > R
    if cut:
        E = [A[k] + (d[k] * R) // m for k in range(3)]          # Python's // floors
        d = [E[k] - A[k] for k in range(3)]
    c = [A[k] >> 8 for k in range(3)]
    e = [E[k] >> 8 for k in range(3)]
    step = [(d[k] > 0) - (d[k] < 0) for k in range(3)]
    den = [abs(d[k]) for k in range(3)]
    rem = [abs(e[k] - c[k]) for k in range(3)]
    num = [((c[k] + 1) << 8) - A[k] if d[k] > 0 else A[k] - (c[k] << 8) for k in range(3)]
    cheb = lambda: max(abs(e[k] - c[k]) for k in range(3))
    visited, sets = [tuple(c)], [cut or cheb() > hit_margin]
    for _ in range(sum(rem)):
        best = None
        for k in range(3):
            if rem[k] > 0 and (best is None or num[k] * den[best] < num[best] * den[k]):
                best = k
        c[best] += step[best]
        num[best] += SUB
        rem[best] -= 1
        visited.append(tuple(c))
        sets.append(cut or cheb() > hit_margin)
    assert c == e
    return visited, sets, cut, tuple(e)


def sweep_bits(points, count, origin, gmin, voxel, dims, hit_margin=2, max_range=80.0):
    """F and O of one sweep of one sample: bool [Gz, Gy, Gx] each, and the number of rays over the walk's bound"""
    Gx, Gy, Gz = dims
    k, R = k_of(voxel), ray_limit(max_range, voxel)
    F = np.zeros((Gz, Gy, Gx), dtype=bool)
    O = np.zeros((Gz, Gy, Gx), dtype=bool)
    pts = np.asarray(points, dtype=np.float32)[: int(count)]
    q, ok = quantise(pts, gmin, k)
    E0 = q[ok]

    def inside(v):
        return (v[:, 0] >= 0) & (v[:, 0] < Gx) & (v[:, 1] >= 0) & (v[:, 1] < Gy) & (v[:, 2] >= 0) & (v[:, 2] < Gz)

    def mark(bits, v, sel):
        s = sel & inside(v)
        bits[v[s, 2], v[s, 1], v[s, 0]] = True

    mark(O, E0 >> 8, np.ones(len(E0), dtype=bool))
    A, a_ok = quantise(np.asarray(origin, dtype=np.float32), gmin, k)
    if not a_ok or len(E0) == 0:
        return F, O, 0
    E = E0.copy()
    d = E - A
    m = np.abs(d).max(1)
    cut = m > R
    E[cut] = A + (d[cut] * R) // m[cut, None]                   # numpy's // floors
    d = E - A
    c = np.broadcast_to(A >> 8, E.shape).copy()
    e = E >> 8
    step, den, rem = np.sign(d), np.abs(d), np.abs(e - c)
    num = np.where(d > 0, ((c + 1) << 8) - A, A - (c << 8))
    total = rem.sum(1)
    bound = 3 * (R // SUB + 1)
    over = int((total > bound).sum())
    total = np.minimum(total, bound)
    far = lambda: np.abs(e - c).max(1) > hit_margin
    mark(F, c, cut | far())
    rows = np.arange(len(E))
    for it in range(int(total.max())):
        act = it < total
        best = np.full(len(E), -1)
        bnum = np.zeros(len(E), dtype=np.int64)
        bden = np.zeros(len(E), dtype=np.int64)
        for ax in range(3):
            better = (rem[:, ax] > 0) & ((best < 0) | (num[:, ax] * bden < bnum * den[:, ax]))
            best = np.where(better, ax, best)
            bnum = np.where(better, num[:, ax], bnum)
            bden = np.where(better, den[:, ax], bden)
        act &= best >= 0
        r, b = rows[act], best[act]
        c[r, b] += step[r, b]
        num[r, b] += SUB
        rem[r, b] -= 1
        mark(F, c, act & (cut | far()))
    return F, O, over


def erode(bits, r):
    """AND over the (2r+1)^3 Chebyshev neighbourhood of a bool [Gz, Gy, Gx]; outside the grid counts as not set"""
    if r == 0:
        return bits.copy()
    Gz, Gy, Gx = bits.shape
    pad = np.zeros((Gz + 2 * r, Gy + 2 * r, Gx + 2 * r), dtype=bool)
    pad[r:r + Gz, r:r + Gy, r:r + Gx] = bits
    out = np.ones_like(bits)
    for dz in range(2 * r + 1):
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                out &= pad[dz:dz + Gz, dy:dy + Gy, dx:dx + Gx]
    return out


def pack(bits):
    """bool [Gz, Gy, Gx] -> uint32 words, bit = (z * Gy + y) * Gx + x, word bit >> 5, bit bit & 31"""
    flat = bits.reshape(-1, 32).astype(np.uint64)
    return (flat << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def flags_of(V, points, count, gmin, voxel):
    """uint8 [N]: the row takes part, its voxel is inside the grid and its bit of V (bool [Gz, Gy, Gx]) is set"""
    Gz, Gy, Gx = V.shape
    pts = np.asarray(points, dtype=np.float32)
    q, ok = quantise(pts, gmin, k_of(voxel))
    v = q >> 8
    ok = ok & (np.arange(len(pts)) < int(count))
    ok &= (v[:, 0] >= 0) & (v[:, 0] < Gx) & (v[:, 1] >= 0) & (v[:, 1] < Gy) & (v[:, 2] >= 0) & (v[:, 2] < Gz)
    out = np.zeros(len(pts), dtype=np.uint8)
    out[ok] = V[v[ok, 2], v[ok, 1], v[ok, 0]]
    return out


class RefMap:
    """the padded-batch wrapper: the same interface as deflow_amd.voidmap.VoidMap on numpy arrays"""

    def __init__(self, batch, grid_min, dims, voxel=0.1, hit_margin=2, erode=1, max_range=80.0):
        self.B, self.gmin, self.dims, self.voxel = batch, np.asarray(grid_min, dtype=np.float32), tuple(dims), voxel
        self.hit_margin, self.r, self.max_range = hit_margin, erode, max_range
        Gx, Gy, Gz = dims
        self.V = np.zeros((batch, Gz, Gy, Gx), dtype=bool)
        self.F, self.O, self.status = self.V.copy(), self.V.copy(), 0
        self.V0 = self.V.copy()                # the map the same sweeps give WITHOUT erosion (for comparisons; not part of the interface)

    def integrate(self, points, count, origin):
        for b in range(self.B):
            self.F[b], self.O[b], over = sweep_bits(points[b], count[b], origin[b], self.gmin, self.voxel, self.dims, self.hit_margin, self.max_range)
            self.status += over
            self.V[b] |= erode(self.F[b] & ~self.O[b], self.r)
            self.V0[b] |= self.F[b] & ~self.O[b]

    def query(self, points, count):
        return np.stack([flags_of(self.V[b], points[b], count[b], self.gmin, self.voxel) for b in range(self.B)])

    words = property(lambda self: np.stack([pack(v) for v in self.V]))
    last_free = property(lambda self: np.stack([pack(v) for v in self.F]))
    last_occ = property(lambda self: np.stack([pack(v) for v in self.O]))


def scene_ref(h5_path, grid, voxel=0.1, sensor_offset=(1.35, 0.0, 1.64), hit_margin=2, erode=1, max_range=80.0):
    """the flags of a scene file on a given grid (grid_min, dims): sweeps in time order, T_i = inv(pose_0) @ pose_i in float64, all lidar
    rows transformed in float64 and rounded to fp32, origin T_i @ (sensor_offset, 1); every sweep integrated, then every sweep queried"""
    from deflow_amd.h5scene import H5File
    with H5File(h5_path) as f:
        keys = sorted(f.keys(), key=int)
        lidar = [np.asarray(f[k]["lidar"].read())[:, :3].astype(np.float64) for k in keys]
        pose = [np.asarray(f[k]["pose"].read()).astype(np.float64) for k in keys]
    inv0 = np.linalg.inv(pose[0])
    m = RefMap(1, grid[0], grid[1], voxel, hit_margin, erode, max_range)
    pts = []
    for p, T in zip(lidar, pose):
        T = inv0 @ T
        x = (p @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        o = (T @ np.array([*sensor_offset, 1.0]))[:3].astype(np.float32)
        pts.append(x)
        if len(x):
            m.integrate(x[None], [len(x)], o[None])
    return {k: (m.query(x[None], [len(x)])[0] if len(x) else np.zeros(0, dtype=np.uint8)) for k, x in zip(keys, pts)}
