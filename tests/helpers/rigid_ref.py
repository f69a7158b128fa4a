"""Naive numpy restatement of the rigid cluster flow of include/deflow_amd.h / DESIGN.md section 6j: all pairs for the vote, all pairs for
every nearest-neighbour pass, numpy sums.  No row lists, no tiles, no LDS: nothing shared with csrc/rigid.hip.

``dtype`` is the precision of every floating-point step: float64 is the reference the kernels are compared with, float32 measures what
the definition's own rounding does to a case (the tolerance of a comparison is a multiple of the difference of the two).  The cluster
labels are an INPUT (DBSCAN is pinned by tests/test_gpu_cluster.py and tests/helpers/dbscan_ref.py).

What makes an input well-posed for an exact comparison of the integer results is reported per cluster slot:
  edge_pairs    used pairs whose vote quotient (d - s) / vote_bin lies within 1e-4 of a half-integer in x or in y (inside the histogram or one
                bin around it): only these can land in another bin in fp32;
  band_pairs    nearest-neighbour d2 within 1e-4 relative of icp_max_dist^2, in any pass: only these can change sides as inliers;
  margins       for a slot that reaches the accept step: (inlier_frac - min_inlier_frac, max_yaw - |theta|, max_disp - displacement)."""
import math

import numpy as np

DEFAULTS = {"min_cluster_size": 20, "min_side": 8, "max_cluster_points": 8192, "vote_cap": 1024, "vote_bin": 0.2, "max_disp": 3.4,
            "icp_cap": 2048, "icp_iters": 8, "icp_max_dist": 0.5, "min_inlier_frac": 0.6, "max_yaw": 0.35}
EDGE = 1e-4
BAND = 1e-4


def vote_radius(max_disp, vote_bin):
    return int(math.ceil(float(np.float32(max_disp)) / float(np.float32(vote_bin)) - 1e-6))


def _pick(rows, cap):
    n = len(rows)
    if n <= cap:
        return rows
    return rows[(np.arange(cap, dtype=np.int64) * n) // cap]


def _rot(theta, x, y, dtype):
    c, s = np.cos(dtype(theta)).astype(dtype), np.sin(dtype(theta)).astype(dtype)
    return c * x - s * y, s * x + c * y


def _nn(p, d):
    """nearest row of d for every row of p: (position, d2); the lowest position on equal d2 (np.argmin returns the first)"""
    dx = p[:, None, 0] - d[None, :, 0]
    dy = p[:, None, 1] - d[None, :, 1]
    dz = p[:, None, 2] - d[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    j = np.argmin(d2, axis=1)
    return j, d2[np.arange(p.shape[0]), j]


def rigid_ref(pc0s, pc1, labels, dtype=np.float64, **params):
    """one sample: pc0s [N0,3], pc1 [N1,3] float32 arrays, labels [N0+N1] of the concatenation (0 = none, 1..K).
    -> dict: flow [N0,3], rigid_id [N0], table [Kcap,8] (theta, tx, ty, tz, inlier_frac, n_src, n_dst, status), vote [Kcap,3], hist
    [Kcap,2R+1,2R+1], edge_pairs [Kcap], band_pairs [Kcap], margins {slot: (frac, yaw, disp)}, runner_up [Kcap] (the second-highest count)"""
    P = dict(DEFAULTS)
    P.update(params)
    dt = np.dtype(dtype).type
    pc0s, pc1 = np.asarray(pc0s, dtype=np.float32), np.asarray(pc1, dtype=np.float32)
    labels = np.asarray(labels).astype(np.int64)
    N0, N1 = pc0s.shape[0], pc1.shape[0]
    assert labels.shape == (N0 + N1,)
    pts = np.concatenate([pc0s, pc1]).astype(dt)
    K = max((N0 + N1) // int(P["min_cluster_size"]), 1)
    vbin = dt(np.float32(P["vote_bin"]))
    R = vote_radius(P["max_disp"], P["vote_bin"])
    W = 2 * R + 1
    md2 = dt(np.float32(P["icp_max_dist"])) * dt(np.float32(P["icp_max_dist"]))
    max_disp, max_yaw, min_frac = dt(np.float32(P["max_disp"])), dt(np.float32(P["max_yaw"])), dt(np.float32(P["min_inlier_frac"]))
    flow = np.zeros((N0, 3), dtype=dt)
    rigid_id = np.zeros(N0, dtype=np.int32)
    table = np.zeros((K, 8), dtype=dt)
    vote = np.zeros((K, 3), dtype=np.int32)
    hist = np.zeros((K, W, W), dtype=np.int32)
    edge = np.zeros(K, dtype=np.int64)
    band = np.zeros(K, dtype=np.int64)
    runner = np.zeros(K, dtype=np.int64)
    margins = {}
    assert labels.max(initial=0) <= K
    for k in range(K):
        rows = np.nonzero(labels == k + 1)[0]
        src, dst = rows[rows < N0], rows[rows >= N0]
        table[k, 5], table[k, 6] = len(src), len(dst)
        if len(rows) == 0:
            continue
        if len(src) < P["min_side"] or len(dst) < P["min_side"]:
            table[k, 7] = 2
            continue
        if len(rows) > P["max_cluster_points"]:
            table[k, 7] = 3
            continue
        # ---- vote
        s, d = pts[_pick(src, P["vote_cap"])], pts[_pick(dst, P["vote_cap"])]
        qx = (d[None, :, 0] - s[:, None, 0]) / vbin
        qy = (d[None, :, 1] - s[:, None, 1]) / vbin
        ix, iy = np.floor(qx + dt(0.5)), np.floor(qy + dt(0.5))
        ok = (np.abs(ix) <= R) & (np.abs(iy) <= R)
        idx = ((iy[ok] + R) * W + (ix[ok] + R)).astype(np.int64)
        h = np.bincount(idx, minlength=W * W).astype(np.int32)
        hist[k] = h.reshape(W, W)
        near = (np.abs(qx) <= R + 1.5) & (np.abs(qy) <= R + 1.5)
        fx, fy = np.abs(qx - np.floor(qx) - 0.5), np.abs(qy - np.floor(qy) - 0.5)
        edge[k] = int((near & ((fx < EDGE) | (fy < EDGE))).sum())
        win = int(np.argmax(h))                         # the first maximum: the lowest bin on equal counts
        cnt = int(h[win])
        runner[k] = int(np.sort(h)[-2]) if h.size > 1 else 0
        if cnt == 0:
            table[k, 7] = 5
            continue
        vote[k] = (win % W - R, win // W - R, cnt)
        # ---- icp, relative to the anchor
        a = pts[src[0]]
        su, du = pts[_pick(src, P["icp_cap"])] - a, pts[_pick(dst, P["icp_cap"])] - a
        theta, t = dt(0), np.array([dt(vote[k, 0]) * vbin, dt(vote[k, 1]) * vbin, dt(0)], dtype=dt)

        def moved(theta, t):
            x, y = _rot(theta, su[:, 0], su[:, 1], dt)
            return np.stack([x + t[0], y + t[1], su[:, 2] + t[2]], axis=1)

        for _ in range(int(P["icp_iters"])):
            j, d2 = _nn(moved(theta, t), du)
            band[k] += int((np.abs(d2 - md2) <= BAND * md2).sum())
            inl = d2 <= md2
            n = int(inl.sum())
            if n < 3:
                continue
            ms, md = su[inl].sum(0) / dt(n), du[j[inl]].sum(0) / dt(n)
            u, v = su[inl] - ms, du[j[inl]] - md
            theta = np.arctan2((u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]).sum(), (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]).sum()).astype(dt)
            rx, ry = _rot(theta, ms[0], ms[1], dt)
            t = np.array([md[0] - rx, md[1] - ry, md[2] - ms[2]], dtype=dt)
        j, d2 = _nn(moved(theta, t), du)
        band[k] += int((np.abs(d2 - md2) <= BAND * md2).sum())
        frac = dt(int((d2 <= md2).sum())) / dt(su.shape[0])
        c = su.sum(0) / dt(su.shape[0])
        rx, ry = _rot(theta, c[0], c[1], dt)
        mx, my = rx + t[0] - c[0], ry + t[1] - c[1]
        disp2 = (mx * mx + my * my) + t[2] * t[2]
        margins[k] = (float(frac - min_frac), float(max_yaw - abs(theta)), float(max_disp - np.sqrt(disp2)))
        status = 1
        if not frac >= min_frac:
            status = 4
        elif not (abs(theta) <= max_yaw and disp2 <= max_disp * max_disp):
            status = 5
        table[k, :5] = (theta, t[0], t[1], t[2], frac)
        table[k, 7] = status
        if status == 1:
            sr = pts[src] - a
            x, y = _rot(theta, sr[:, 0], sr[:, 1], dt)
            flow[src, 0] = (x + t[0]) - sr[:, 0]
            flow[src, 1] = (y + t[1]) - sr[:, 1]
            flow[src, 2] = t[2]
            rigid_id[src] = k + 1
    return {"flow": flow, "rigid_id": rigid_id, "table": table, "vote": vote, "hist": hist, "edge_pairs": edge, "band_pairs": band,
            "margins": margins, "runner_up": runner, "R": R}


def planted_epe(flow, truth, rows):
    """mean end-point error of flow [N,3] against the planted flow truth [N,3] over rows"""
    return float(np.linalg.norm(np.asarray(flow, dtype=np.float64)[rows] - np.asarray(truth, dtype=np.float64)[rows], axis=1).mean())


# ---- generators ----------------------------------------------------------------------------------------------------------------------
def l_shape(rng, n, length=4.6, width=1.9, height=1.5):
    """n points on two faces of a box in the object's frame: the long side y = -width/2 and the rear x = -length/2 (what a LiDAR sees of a
    vehicle), in proportion to their areas; float64 [n,3]"""
    on_long = rng.random(n) < length / (length + width)
    u, z = rng.random(n), rng.random(n) * height
    x = np.where(on_long, (u - 0.5) * length, -0.5 * length)
    y = np.where(on_long, -0.5 * width, (u - 0.5) * width)
    return np.stack([x, y, z], axis=1)


def _rz(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def vehicle(rng, centre, heading, n0, n1, yaw=0.0, forward=0.0, lateral=0.0, sigma=0.01, **box):
    """an L-shaped vehicle at `centre` with `heading`, seen in both sweeps: n0 points in the first, n1 independently drawn points in the
    second after the planted motion p -> Rz(yaw) (p - centre) + centre + Rz(heading) (forward, lateral, 0), plus N(0, sigma) noise.
    -> (src [n0,3] f32, dst [n1,3] f32, truth [n0,3] f64: the planted flow of the source rows (of their float32 positions))"""
    centre = np.asarray(centre, dtype=np.float64)
    H, M = _rz(heading), _rz(yaw)
    tau = H @ np.array([forward, lateral, 0.0])
    src = (l_shape(rng, n0, **box) @ H.T + centre).astype(np.float32)
    w1 = l_shape(rng, n1, **box) @ H.T + centre
    dst = ((w1 - centre) @ M.T + centre + tau + rng.normal(0.0, sigma, (n1, 3))).astype(np.float32)
    s64 = src.astype(np.float64)
    truth = (s64 - centre) @ M.T + centre + tau - s64
    return src, dst, truth


def clutter(rng, centre, n0, n1, extent=(1.2, 1.2, 1.0), sigma=0.01):
    """static clutter: ONE set of surface points (a box of `extent` filled uniformly) of which each sweep sees its own draw; truth = 0"""
    centre = np.asarray(centre, dtype=np.float64)
    e = np.asarray(extent, dtype=np.float64)
    src = (centre + (rng.random((n0, 3)) - 0.5) * e).astype(np.float32)
    dst = (centre + (rng.random((n1, 3)) - 0.5) * e + rng.normal(0.0, sigma, (n1, 3))).astype(np.float32)
    return src, dst, np.zeros((n0, 3))


def one_sided(rng, centre, n, first=True, extent=(1.5, 1.5, 1.0)):
    """a cluster seen in one sweep only"""
    centre = np.asarray(centre, dtype=np.float64)
    p = (centre + (rng.random((n, 3)) - 0.5) * np.asarray(extent)).astype(np.float32)
    z = np.zeros((0, 3), dtype=np.float32)
    return (p, z, np.zeros((n, 3))) if first else (z, p, np.zeros((0, 3)))


def assemble(rng, objects, pad0=0, pad1=0, shuffle=True):
    """objects: list of (src, dst, truth) -> pc0s [N0,3] f32, pc1 [N1,3] f32, truth [N0,3] f64, obj0 [N0] (object index of each pc0s row, -1 in
    the padding), counts (n0, n1); rows shuffled inside each sweep, then pad0 / pad1 NaN rows appended"""
    src = np.concatenate([o[0] for o in objects]).astype(np.float32)
    dst = np.concatenate([o[1] for o in objects]).astype(np.float32)
    truth = np.concatenate([o[2] for o in objects])
    obj0 = np.concatenate([np.full(len(o[0]), i) for i, o in enumerate(objects)])
    if shuffle:
        p0, p1 = rng.permutation(len(src)), rng.permutation(len(dst))
        src, truth, obj0, dst = src[p0], truth[p0], obj0[p0], dst[p1]
    n0, n1 = len(src), len(dst)
    nan = np.float32("nan")
    src = np.concatenate([src, np.full((pad0, 3), nan, dtype=np.float32)])
    dst = np.concatenate([dst, np.full((pad1, 3), nan, dtype=np.float32)])
    truth = np.concatenate([truth, np.zeros((pad0, 3))])
    obj0 = np.concatenate([obj0, np.full(pad0, -1)])
    return src, dst, truth, obj0, (n0, n1)


def grid_centres(n, spacing=12.0, extent=40.0):
    """n well-separated centres on a square grid inside +-extent (so that DBSCAN's clusters are the objects)"""
    side = int(2 * extent // spacing) + 1
    assert n <= side * side
    out = []
    for i in range(n):
        out.append((-extent + spacing * (i % side), -extent + spacing * (i // side), 0.0))
    return out


def object_labels(obj0, obj1, min_cluster_size=20):
    """labels of the concatenation when every object is one cluster: numbered 1..K in ascending order of the object's lowest row (the
    order DBSCAN numbers its clusters in when each object is one component whose lowest row is a core row); objects with fewer than
    min_cluster_size rows get 0.  For CPU-only use of the helper; the GPU tests take the op's own labels."""
    obj = np.concatenate([obj0, obj1])
    labels = np.zeros(len(obj), dtype=np.int64)
    k = 0
    seen = set()
    for o in obj:
        if o < 0 or o in seen:
            continue
        seen.add(o)
        if (obj == o).sum() >= min_cluster_size:
            k += 1
            labels[obj == o] = k
    return labels


# ---- the cases of tests/test_gpu_rigid.py (built once per session; the CPU tests check their well-posedness with object_labels) -------
def planted_sample(seed, n_vehicles=7, n_static=3, n_one=2, pad0=37, pad1=5):
    """~12 clusters: vehicles with yaw within +-0.1 rad and up to 2.5 m along their heading (so that both sweeps overlap and DBSCAN joins
    them), static clutter, one-sided clusters.  -> dict(pc0s, pc1, truth, obj0, obj1, n0, n1)"""
    rng = np.random.default_rng(seed)
    cs = grid_centres(n_vehicles + n_static + n_one)
    objects = []
    for i in range(n_vehicles):
        n0, n1 = int(rng.integers(60, 401)), int(rng.integers(60, 401))
        objects.append(vehicle(rng, cs[len(objects)], rng.uniform(-math.pi, math.pi), n0, n1, yaw=rng.uniform(-0.1, 0.1),
                               forward=rng.uniform(0.3, 2.5), lateral=rng.uniform(-0.15, 0.15), length=rng.uniform(4.4, 6.0)))
    for i in range(n_static):
        objects.append(clutter(rng, cs[len(objects)], int(rng.integers(60, 200)), int(rng.integers(60, 200))))
    for i in range(n_one):
        objects.append(one_sided(rng, cs[len(objects)], int(rng.integers(40, 120)), first=(i % 2 == 0)))
    obj1 = np.concatenate([np.full(len(o[1]), i) for i, o in enumerate(objects)])
    src = np.concatenate([o[0] for o in objects])
    dst = np.concatenate([o[1] for o in objects])
    truth = np.concatenate([o[2] for o in objects])
    obj0 = np.concatenate([np.full(len(o[0]), i) for i, o in enumerate(objects)])
    p0, p1 = rng.permutation(len(src)), rng.permutation(len(dst))
    src, truth, obj0, dst, obj1 = src[p0], truth[p0], obj0[p0], dst[p1], obj1[p1]
    nan = np.float32("nan")
    return {"pc0s": np.concatenate([src, np.full((pad0, 3), nan, np.float32)]), "pc1": np.concatenate([dst, np.full((pad1, 3), nan, np.float32)]),
            "truth": np.concatenate([truth, np.zeros((pad0, 3))]), "obj0": np.concatenate([obj0, np.full(pad0, -1)]),
            "obj1": np.concatenate([obj1, np.full(pad1, -1)]), "n0": len(src), "n1": len(dst), "n_objects": len(objects)}


def pad_batch(samples, key, width=None):
    """stack per-sample arrays [n_i, ...] into [B, max n_i, ...], float arrays padded with NaN, integer ones with -1"""
    width = width or max(len(s[key]) for s in samples)
    first = np.asarray(samples[0][key])
    fill = np.nan if first.dtype.kind == "f" else -1
    out = np.full((len(samples), width) + first.shape[1:], fill, dtype=first.dtype)
    for b, s in enumerate(samples):
        out[b, : len(s[key])] = s[key]
    return out


LATTICE = 64.0            # coordinates of the exact-vote case are multiples of 1 / 64 m: differences and quotients by 0.25 are exact
LATTICE_PARAMS = {"vote_bin": 0.25, "max_disp": 3.0, "vote_cap": 64}


def _lat(rng, n, lo, hi):
    """n lattice points, uniformly in the box [lo, hi)"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return (np.floor((lo + rng.random((n, 3)) * (hi - lo)) * LATTICE) / LATTICE).astype(np.float32)


def lattice_sample(seed, special=True):
    """clusters of 16-300 rows per side on the lattice: compact ones displaced by a lattice vector, one 300-row pair (over vote_cap = 64:
    the stride rule), and with `special` an elongated one whose sides lie up to 9 m apart (displacements beyond max_disp), a planted exact
    tie, a one-sided one, and NaN / inf rows inside the counted part"""
    rng = np.random.default_rng(seed)
    cs = grid_centres(12)
    objects = []
    for i in range(6):
        n0, n1 = (300, 300) if i == 0 else (int(rng.integers(16, 120)), int(rng.integers(16, 120)))
        c = np.asarray(cs[len(objects)])
        shift = np.round(rng.uniform(-0.6, 0.6, 3) * [1, 1, 0] * LATTICE) / LATTICE
        objects.append((_lat(rng, n0, c - [0.6, 0.6, 0.3], c + [0.6, 0.6, 0.3]), _lat(rng, n1, c - [0.6, 0.6, 0.3] + shift, c + [0.6, 0.6, 0.3] + shift),
                        np.zeros((n0, 3))))
    if special:
        c = np.asarray(cs[len(objects)])                    # elongated: sources in the left half, targets in the right half of a 9 m bar
        objects.append((_lat(rng, 150, c + [0.0, -0.25, 0.0], c + [4.5, 0.25, 0.4]), _lat(rng, 150, c + [4.0, -0.25, 0.0], c + [9.0, 0.25, 0.4]),
                        np.zeros((150, 3))))
        c = np.asarray(cs[len(objects)])                    # exact tie: every difference to either copy falls into the copy's own bin
        a = _lat(rng, 16, c, c + [0.09, 0.09, 0.09])
        d1, d2 = _lat(rng, 16, c, c + [0.09, 0.09, 0.09]), _lat(rng, 16, c, c + [0.09, 0.09, 0.09])
        d1[:, 0] += np.float32(0.5)
        d2[:, 0] -= np.float32(0.5)
        objects.append((a, np.concatenate([d1, d2]), np.zeros((16, 3))))
        objects.append(one_sided(rng, cs[len(objects)], 40, first=True, extent=(0.8, 0.8, 0.5)))
    s = assemble(rng, objects)
    pc0s, pc1, n0, n1 = s[0], s[1], s[4][0], s[4][1]
    if special:                                            # non-finite rows inside the counted part
        pc0s[5] = (np.nan, 1.0, 0.0)
        pc0s[n0 // 2] = (np.inf, 0.0, 0.0)
        pc1[7] = (0.0, -np.inf, 0.0)
        pc1[n1 - 1] = (np.nan, np.nan, np.nan)
    return {"pc0s": pc0s, "pc1": pc1, "n0": n0, "n1": n1, "tie_object": 7 if special else None}
