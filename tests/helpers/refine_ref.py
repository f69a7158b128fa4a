"""Naive numpy restatement of the per-cluster rigid snap of include/deflow_amd.h / DESIGN.md section 6p (a - f): boolean masks instead of
row lists, numpy sums, all pairs for the check's nearest neighbours.  Nothing shared with csrc/refine.hip.

``dtype`` is the precision of every floating-point step: float64 is the reference the kernels are compared with, float32 measures what
the definition's own rounding does to a case (the bound of a comparison is a multiple of the difference of the two).  The cluster labels
are an INPUT (DBSCAN is pinned by tests/test_gpu_cluster.py and tests/helpers/dbscan_ref.py).

What makes an input well-posed for an exact comparison of the integer results is reported per cluster slot:
  margins      for a slot that reaches the accept step, the RELATIVE distance of every tested value from its threshold, by name
               (``inlier_frac``, ``max_yaw``, ``max_disp``, ``static_disp``, ``static_yaw``; ``check`` for step e), signed: positive on
               the accepting side;
  near_inlier  rows whose last residual lies within NEAR (1e-3 m) of inlier_dist: only these can change sides in fp32."""
import numpy as np

DEFAULTS = {"min_cluster_size": 20, "min_rows": 8, "max_cluster_points": 8192, "iters": 4, "delta": 0.1, "inlier_dist": 0.2,
            "min_inlier_frac": 0.5, "max_yaw": 0.35, "max_disp": 3.4, "static_disp": 0.05, "static_yaw": 0.02, "check": True,
            "check_trunc": 2.0, "check_tol": 0.05}
COLS = 12
NEAR = 1e-3


def takes_part(x, f, count):
    """[N] bool: rows inside the count whose x and f are finite"""
    n = x.shape[0]
    return (np.arange(n) < min(max(int(count), 0), n)) & np.isfinite(x).all(1) & np.isfinite(f).all(1)


def _rot(theta, px, py):
    c, s = np.cos(theta), np.sin(theta)
    return c * px - s * py, s * px + c * py


def residual2(s, d, theta, t):
    qx, qy = _rot(theta, s[:, 0], s[:, 1])
    ex, ey, ez = (qx + t[0]) - d[:, 0], (qy + t[1]) - d[:, 1], (s[:, 2] + t[2]) - d[:, 2]
    return (ex * ex + ey * ey) + ez * ez


def fit_once(s, d, w):
    """one weighted fit of step c: theta, t"""
    W = w.sum()
    ms, md = (w[:, None] * s).sum(0) / W, (w[:, None] * d).sum(0) / W
    u, v = s - ms, d - md
    theta = np.arctan2((w * (u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0])).sum(), (w * (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1])).sum())
    rx, ry = _rot(theta, ms[0], ms[1])
    t = np.array([md[0] - rx, md[1] - ry, md[2] - ms[2]], dtype=s.dtype)
    return theta.astype(s.dtype), t


def irls(s, d, iters, delta):
    """iters re-weightings, iters + 1 fits (step c) -> theta, t, the last residuals r"""
    w = np.ones(s.shape[0], dtype=s.dtype)
    for it in range(int(iters) + 1):
        theta, t = fit_once(s, d, w)
        r = np.sqrt(residual2(s, d, theta, t))
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(r <= delta, s.dtype.type(1), np.where(np.isfinite(r), delta / r, 0)).astype(s.dtype)
    return theta, t, r


def snap(s, theta, t):
    """step f: the flow Rz(theta) s + t - s"""
    qx, qy = _rot(theta, s[:, 0], s[:, 1])
    return np.stack([(qx + t[0]) - s[:, 0], (qy + t[1]) - s[:, 1], np.broadcast_to(t[2], qx.shape)], axis=1)


def _nn_trunc(q, ref, trunc):
    """min(distance to the nearest finite row of ref, trunc) for every row of q; trunc without a neighbour"""
    out = np.full(q.shape[0], trunc, dtype=q.dtype)
    ref = ref[np.isfinite(ref).all(1)]
    if ref.shape[0] == 0 or q.shape[0] == 0:
        return out
    for lo in range(0, q.shape[0], 512):
        diff = q[lo:lo + 512, None, :] - ref[None, :, :]
        d2 = ((diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]).min(1)
        out[lo:lo + 512] = np.where(d2 <= trunc * trunc, np.minimum(np.sqrt(d2), trunc), trunc)
    return out


def trunc_dist(d2, trunc):
    """step e on given squared distances: min(sqrt(d2), trunc), trunc for inf / NaN / beyond"""
    with np.errstate(invalid="ignore"):
        ok = (d2 >= 0) & (d2 <= trunc * trunc)
        return np.where(ok, np.minimum(np.sqrt(np.where(ok, d2, 0)), trunc), trunc)


def refine_ref(x, f, labels, count, pc1=None, count1=0, dtype=np.float64, d2_before=None, d2_after=None, **params):
    """one sample: x, f [N,3] float32 arrays, labels [N] (0 = none, 1..K), count; the second sweep pc1 [N1,3] with count1 valid rows, or
    the check's squared distances given (d2_before / d2_after [N], then count1 only says whether there is a second sweep).
    -> dict: flow [N,3] (in dtype; rows that get no motion hold f's values), rigid_id [N], moved [N] bool (rows whose flow was written),
    table [K,12], anchor [K], margins {slot: {name: relative margin}}, near_inlier [K], provisional [N,3] (f' of step e)"""
    P = dict(DEFAULTS)
    P.update(params)
    dt = np.dtype(dtype)
    T = dt.type
    x32, f32 = np.asarray(x, dtype=np.float32), np.asarray(f, dtype=np.float32)
    labels = np.asarray(labels).astype(np.int64)
    N = x32.shape[0]
    K = max(N // int(P["min_cluster_size"]), 1)
    th = {k: T(np.float32(P[k])) for k in ("delta", "inlier_dist", "min_inlier_frac", "max_yaw", "max_disp", "static_disp", "static_yaw",
                                           "check_trunc", "check_tol")}
    n = min(max(int(count), 0), N)
    part = takes_part(x32, f32, n)
    with np.errstate(invalid="ignore", over="ignore"):
        xs, fs = x32.astype(dt), f32.astype(dt)
    table = np.zeros((K, COLS), dtype=dt)
    anchor = np.full(K, -1, dtype=np.int64)
    near = np.zeros(K, dtype=np.int64)
    margins = {}
    members = {}
    for k in range(K):
        rows = np.nonzero((labels == k + 1) & (np.arange(N) < n))[0]
        if rows.size == 0:
            continue
        if rows.size > int(P["max_cluster_points"]):
            table[k, 6], table[k, 7] = rows.size, 3
            continue
        use = rows[part[rows]]
        table[k, 6] = use.size
        if use.size > 0:
            anchor[k] = use[0]
        if use.size < int(P["min_rows"]):
            table[k, 7] = 2
            continue
        members[k] = use
        s = xs[use] - xs[use[0]]
        d = s + fs[use]
        theta, t, r = irls(s, d, P["iters"], th["delta"])
        frac = T((r <= th["inlier_dist"]).sum()) / T(use.size)
        near[k] = int((np.abs(r - th["inlier_dist"]) <= NEAR).sum())
        c = s.sum(0) / T(use.size)
        mx, my = _rot(theta, c[0], c[1])
        mx, my = (mx + t[0]) - c[0], (my + t[1]) - c[1]
        disp = np.sqrt((mx * mx + my * my) + t[2] * t[2])
        rel = lambda v, lim: float((lim - v) / lim) if lim > 0 else float(lim - v)
        m = {"inlier_frac": -rel(frac, th["min_inlier_frac"])}
        status = 1
        if not frac >= th["min_inlier_frac"]:
            status = 4
        else:
            m["max_yaw"], m["max_disp"] = rel(abs(theta), th["max_yaw"]), rel(disp, th["max_disp"])
            if not (abs(theta) <= th["max_yaw"] and disp <= th["max_disp"]):
                status = 5
            else:
                m["static_disp"], m["static_yaw"] = rel(disp, th["static_disp"]), rel(abs(theta), th["static_yaw"])
                if disp <= th["static_disp"] and abs(theta) <= th["static_yaw"]:
                    status = 6
                    theta, t = T(0), np.zeros(3, dtype=dt)
        margins[k] = m
        table[k, 0], table[k, 1:4], table[k, 4] = theta, t, frac
        table[k, 5] = np.sqrt((r * r).sum() / T(use.size))
        table[k, 7] = status

    def apply():
        flow, rid, moved = fs.copy(), np.zeros(N, dtype=np.int32), np.zeros(N, dtype=bool)
        for k, use in members.items():
            if table[k, 7] == 1:
                flow[use] = snap(xs[use] - xs[use[0]], table[k, 0], table[k, 1:4])
            elif table[k, 7] == 6:
                flow[use] = 0
            else:
                continue
            rid[use], moved[use] = k + 1, True
        return flow, rid, moved

    provisional = apply()[0]
    if P["check"] and int(count1) > 0:
        trunc = th["check_trunc"]
        if d2_before is not None:
            with np.errstate(invalid="ignore", over="ignore"):
                tb, ta = trunc_dist(np.asarray(d2_before, np.float32).astype(dt), trunc), trunc_dist(np.asarray(d2_after, np.float32).astype(dt), trunc)
        else:
            ref = np.asarray(pc1, dtype=np.float32)[:max(int(count1), 0)].astype(dt)
            tb, ta = np.full(N, trunc, dtype=dt), np.full(N, trunc, dtype=dt)
            rows = np.concatenate([u for k, u in members.items() if table[k, 7] in (1, 6)] or [np.zeros(0, dtype=np.int64)])
            # (the kernels query what fp32 holds of x + f: the sum is rounded to fp32 first)
            tb[rows] = _nn_trunc((x32[rows] + f32[rows]).astype(dt), ref, trunc)
            ta[rows] = _nn_trunc((x32[rows] + provisional[rows].astype(np.float32)).astype(dt), ref, trunc)
        for k, use in members.items():
            if table[k, 7] not in (1, 6):
                continue
            cb, ca = tb[use].sum() / T(use.size), ta[use].sum() / T(use.size)
            table[k, 8], table[k, 9] = cb, ca
            margins[k]["check"] = float((cb + th["check_tol"]) - ca)
            if ca > cb + th["check_tol"]:
                table[k, 7] = 7
    flow, rid, moved = apply()
    return {"flow": flow, "rigid_id": rid, "moved": moved, "table": table, "anchor": anchor, "margins": margins, "near_inlier": near,
            "provisional": provisional}


# ---- the planted case of DESIGN.md section 6p ---------------------------------------------------------------------------------------------
PLANTED_SEED = 20240116
PLANTED_ROWS = (200, 300, 64, 120)
PLANTED_HALF = (2.2, 0.9, 0.8)
PLANTED_MOTION = ((0.05, (1.0, 0.2, 0.0)), (-0.08, (-0.6, 0.9, 0.02)), (0.0, (0.0, 0.0, 0.0)), (0.1, (0.3, -1.2, 0.0)))
PLANTED_CENTRE = ((10.0, 5.0, 0.0), (-12.0, 8.0, 0.0), (3.0, -15.0, 0.0), (-8.0, -9.0, 0.0))


def rigid_motion(x, centre, yaw, t):
    """the flow of rows x under a yaw about ``centre`` followed by the translation t (float64)"""
    x, c = np.asarray(x, np.float64), np.asarray(centre, np.float64)
    qx, qy = _rot(np.float64(yaw), x[:, 0] - c[0], x[:, 1] - c[1])
    return np.stack([qx + c[0] + t[0] - x[:, 0], qy + c[1] + t[1] - x[:, 1], np.full(x.shape[0], float(t[2]))], axis=1)


def planted_case():
    """four bodies of 200, 300, 64 and 120 rows, uniform in boxes of half-extent (2.2, 0.9, 0.8) m; flow = truth + N(0, 0.05) per
    component, a random 25 % of each body's rows replaced: zero flow for bodies 1, 2 and 4, N(0, 0.5) for body 3 (which does not move).
    -> x [684,3] f32, flow [684,3] f32, truth [684,3] f64, body [684] (1..4)"""
    rng = np.random.default_rng(PLANTED_SEED)
    xs, fl, tr, body = [], [], [], []
    for i, n in enumerate(PLANTED_ROWS):
        x = (rng.uniform(-1.0, 1.0, (n, 3)) * np.array(PLANTED_HALF) + np.array(PLANTED_CENTRE[i])).astype(np.float32)
        yaw, t = PLANTED_MOTION[i]
        truth = rigid_motion(x, PLANTED_CENTRE[i], yaw, t)
        f = truth + rng.normal(0.0, 0.05, (n, 3))
        bad = rng.permutation(n)[: n // 4]
        f[bad] = rng.normal(0.0, 0.5, (bad.size, 3)) if i == 2 else 0.0
        xs.append(x), fl.append(f.astype(np.float32)), tr.append(truth), body.append(np.full(n, i + 1))
    return np.concatenate(xs), np.concatenate(fl), np.concatenate(tr), np.concatenate(body)


def epe(flow, truth):
    return float(np.linalg.norm(np.asarray(flow, np.float64) - truth, axis=1).mean())


# ---- the planted-label case of tests/test_gpu_refine.py: sizes, rejects and both sides of every threshold of step d -----------------------
OPS_N = 9000
OPS_COUNTS = (9000, 700, 0)
# sample 1: (name, rows, yaw, |t|, which side): the motion is about the rows' own centroid, so the centroid moves by |t| exactly
OPS_EDGES = (("yaw_in", 40, 0.345, 1.0), ("yaw_out", 40, 0.355, 1.0), ("disp_in", 40, 0.05, 3.38), ("disp_out", 40, 0.05, 3.42),
             ("static_disp_in", 40, 0.004, 0.0495), ("static_disp_out", 40, 0.004, 0.0505), ("static_yaw_in", 40, 0.0198, 0.01),
             ("static_yaw_out", 40, 0.0202, 0.01))


def _body(rng, n, centre, half=(1.5, 0.8, 0.6)):
    return (rng.uniform(-1.0, 1.0, (n, 3)) * np.array(half) + np.array(centre)).astype(np.float32)


def _moved(x, yaw, t):
    """the exact rigid flow about the centroid of x"""
    return rigid_motion(x, np.asarray(x, np.float64).mean(0), yaw, t).astype(np.float32)


def ops_case(big=8192, seed=7):
    """x, f [3, 9000, 3] f32, labels [3, 9000] i32, counts (9000, 700, 0) and names {(sample, label): what the cluster is for}.
    Sample 0: the big cluster (``big`` rows: 8192 fits, 8193 is status 3), then clusters of 10 rows of which 7 take part (status 2), 8, 64,
    65 and 300 rows (the 300 with NaN / inf rows inside and in front), label-0 rows in between.  Sample 1: both sides of every threshold of
    step d, a cluster of one repeated point, labelled NaN rows behind the count.  Sample 2: count 0, NaN everywhere."""
    rng = np.random.default_rng(seed)
    N = OPS_N
    x = np.full((3, N, 3), np.nan, dtype=np.float32)
    f = np.full((3, N, 3), np.nan, dtype=np.float32)
    lab = np.zeros((3, N), dtype=np.int32)
    names = {}
    # ---- sample 0
    at, label = 0, 0

    def put(b, pts, flow, name, gap=5):
        nonlocal at, label
        label += 1
        n = pts.shape[0]
        x[b, at:at + n], f[b, at:at + n], lab[b, at:at + n] = pts, flow, label
        names[(b, label)] = name
        rows = np.arange(at, at + n)
        at += n
        g = _body(rng, gap, (40.0, 40.0, 0.0))                      # label-0 rows between the clusters, with a flow of their own
        x[b, at:at + gap], f[b, at:at + gap] = g, rng.normal(0, 1, (gap, 3)).astype(np.float32)
        at += gap
        return rows

    pts = _body(rng, big, (0.0, 0.0, 0.0), (12.0, 6.0, 1.0))
    put(0, pts, _moved(pts, 0.03, (0.8, -0.4, 0.05)) + rng.normal(0, 0.01, (big, 3)).astype(np.float32), "big")
    pts = _body(rng, 10, (20.0, 0.0, 0.0))
    r = put(0, pts, _moved(pts, 0.0, (0.5, 0.0, 0.0)), "seven")
    f[0, r[[1, 4]]] = np.nan
    x[0, r[8], 1] = np.inf
    for n, name in ((8, "eight"), (64, "n64"), (65, "n65")):
        pts = _body(rng, n, (20.0 + 0.1 * n, 20.0, 0.0))
        put(0, pts, _moved(pts, 0.1, (0.3, 0.6, -0.02)) + rng.normal(0, 0.005, (n, 3)).astype(np.float32), name)
    pts = _body(rng, 300, (-20.0, 20.0, 0.0))
    fl = _moved(pts, -0.06, (-1.1, 0.4, 0.0)) + rng.normal(0, 0.02, (300, 3)).astype(np.float32)
    zero = rng.permutation(300)[:60]
    fl[zero] = 0.0                                                   # a fifth of the rows: the network's typical failure
    r = put(0, pts, fl, "n300")
    f[0, r[0]] = np.nan                                              # the list's first row takes no part: the anchor is the second
    f[0, r[17], 2] = np.inf
    x[0, r[[33, 170]]] = np.nan
    x[0, r[250], 0] = -np.inf
    rest = N - at
    x[0, at:], f[0, at:] = _body(rng, rest, (-40.0, -40.0, 0.0), (5.0, 5.0, 1.0)), rng.normal(0, 1, (rest, 3)).astype(np.float32)
    assert at <= N
    # ---- sample 1
    at, label = 0, 0
    for i, (name, n, yaw, disp) in enumerate(OPS_EDGES):
        pts = _body(rng, n, (8.0 * i - 30.0, 10.0, 0.0))
        ang = 0.7 * i
        put(1, pts, _moved(pts, yaw, (disp * np.cos(ang), disp * np.sin(ang), 0.0)), name, gap=3)
    for name, good in (("frac_in", 33), ("frac_out", 31)):
        pts = _body(rng, 64, (-30.0 if good == 33 else 30.0, -10.0, 0.0))
        fl = _moved(pts, 0.02, (0.7, 0.1, 0.0))
        bad = rng.permutation(64)[: 64 - good]
        off = rng.normal(0, 3.0, (bad.size, 3))
        off[np.linalg.norm(off, axis=1) < 1.0] += 2.0                 # gross errors only: none near inlier_dist
        fl[bad] += off.astype(np.float32)
        put(1, pts, fl, name, gap=3)
    put(1, np.tile(np.array([[5.0, -20.0, 0.5]], np.float32), (30, 1)), np.tile(np.array([[0.5, -0.25, 0.125]], np.float32), (30, 1)), "point",
        gap=3)
    rest = OPS_COUNTS[1] - at
    assert rest >= 0
    x[1, at:at + rest], f[1, at:at + rest] = _body(rng, rest, (0.0, 40.0, 0.0)), rng.normal(0, 1, (rest, 3)).astype(np.float32)
    lab[1, OPS_COUNTS[1]:] = 1                                       # labelled rows behind the count: they belong to no list
    lab[2, :] = 2
    return x, f, lab, np.array(OPS_COUNTS, dtype=np.int32), names
