"""Named inputs that pin df_normals (include/deflow_amd.h) off the plane and at the grid's edges, their float64
reference (plane_ref.normals: all-pairs neighbours, numpy.linalg.eigh, the header's sign and validity rules) and the conditions every
case puts on its own INPUT, so that the comparison with the kernel is exact where it is stated as exact:

  * no participating pair has |d2 / r2 - 1| < 1e-6, except where d2 == r2 holds exactly (fp32 cannot move a pair across the radius);
  * no row has |curv / max_curv - 1| < 1e-5, except where fp32(curv) == fp32(max_curv) by construction (``exact_radius``);
  * no trace lies within 1e-12 r2 of 0 unless it is exactly 0.

Cases (all N <= 1500 rows per sample, B <= 3):
  generic       the command's defaults (range +-51.2, cell = radius = 1, G = 103): spheres, a sinusoidal sheet, a noisy plane
  spread        isolated blobs 4 cells apart, rotated ellipsoids with lambda0 / lambda1 in 1e-10 .. 0.9, lambda1 / lambda2 in 1e-3 .. 1
  binade        pairs a hair less than one cell apart that fp32 files TWO cells apart, in x and in y: on the default grid, at the cell
                coordinate's binade edge 64 (cells 63 and 65); ``binade_33``: the same at the edge 32 of a grid of the same size that
                starts at -30.2 (the default grid has no such pair there, and no grid has one below 32: see ``binade_pairs``)
  exact_radius  a dyadic lattice with spacing == radius == cell: the six lattice neighbours sit at d2 == r2 exactly
  border        G = 8, B = 3: rows outside the range on every side, a border cell of 600 rows, masks, counts, non-finite rows
  degenerate    collinear rows, forty copies of a point, m == min_pts - 1 and min_pts, a flat cloud at z = 0, a row at the origin, a
                neighbourhood of 1e-3 m at 50 m

Also the deliberately wrong variants of the reference with which tests/test_normals_cases_cpu.py shows that each case bites."""
from __future__ import annotations

import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_ref  # noqa: E402
import reg_ref  # noqa: E402

EPS = 2.0 ** -24
THIRD = 1.0 / 3.0
DEFAULT_GRID = dict(xy_range=(-51.2, -51.2, 51.2, 51.2), cell=1.0)            # the odometry command's defaults: G = 103
NAMES = ("generic", "spread", "binade", "binade_33", "exact_radius", "exact_radius_half", "border", "degenerate")


# ---- the fp32 cell rule (nn_search.h: nn_cell), restated in numpy -----------------------------------------------------------------------
def grid_size(xy_range, cell) -> int:
    return int(np.ceil(max(xy_range[2] - xy_range[0], xy_range[3] - xy_range[1]) / cell - 1e-6))


def cell_f32(v, lo, cell, G) -> np.ndarray:
    """the cell of the finite fp32 coordinates v: fp32(fp32(v - lo) * fp32(1 / cell)) clamped to [0, G], truncated, at most G - 1"""
    v = np.asarray(v, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(cell)
    f = np.minimum(np.maximum((v - np.float32(lo)) * inv, np.float32(0.0)), np.float32(G))
    return np.minimum(f.astype(np.int64), G - 1)


def cells(points, case):
    G = grid_size(case.xy_range, case.cell)
    p = np.nan_to_num(np.asarray(points, dtype=np.float32), nan=0.0, posinf=0.0, neginf=0.0)
    return cell_f32(p[:, 0], case.xy_range[0], case.cell, G), cell_f32(p[:, 1], case.xy_range[1], case.cell, G)


# ---- the reference and its wrong variants -----------------------------------------------------------------------------------------------
def _d2(points, ok):
    p = np.where(ok[:, None], np.asarray(points, dtype=np.float64), 0.0)
    return ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)


def reference(case, b, max_curv, variant=None, diff32=False):
    """plane_ref.normals of sample b.  variant: None (the header's definition) or one of the deliberately wrong ones --
    'cells3x3' (neighbours only from the 3 x 3 cells of the fp32 cell rule around the row's own), 'strict' (d2 < r2), 'drop_outside'
    (rows outside xy_range do not take part), 'earlier_axis' (on equal eigenvalues), 'no_tie_break' (of the sign rule)."""
    pts, count, mask = case.points[b], case.counts[b], None if case.mask is None else case.mask[b]
    ok = reg_ref.participating(pts, count, mask)
    kw = dict(radius=case.radius, min_pts=case.min_pts, max_curv=max_curv, diff32=diff32)
    if variant in (None, "earlier_axis", "no_tie_break"):
        return plane_ref.normals(pts, count, mask, later_axis=variant != "earlier_axis", tie_break=variant != "no_tie_break", **kw)
    if variant == "drop_outside":
        x0, y0, x1, y1 = case.xy_range
        with np.errstate(invalid="ignore"):
            inside = (pts[:, 0] >= x0) & (pts[:, 0] < x1) & (pts[:, 1] >= y0) & (pts[:, 1] < y1)
        keep = (np.ones(len(pts), dtype=np.int32) if mask is None else (np.asarray(mask) > 0).astype(np.int32)) * inside
        return plane_ref.normals(pts, count, keep, **kw)
    d2 = _d2(pts, ok)
    near = (d2 < case.radius ** 2 if variant == "strict" else d2 <= case.radius ** 2) & ok[:, None] & ok[None, :]
    if variant == "cells3x3":
        cx, cy = cells(pts, case)
        near &= (np.abs(cx[:, None] - cx[None, :]) <= 1) & (np.abs(cy[:, None] - cy[None, :]) <= 1)
    elif variant != "strict":
        raise ValueError(variant)
    return plane_ref.normals(pts, count, mask, near=near, **kw)


@functools.lru_cache(maxsize=None)
def ref(name, b, max_curv, variant=None, diff32=False):
    """``reference`` of the named case, computed once and shared (read-only) among the tests"""
    out = reference(case(name), b, max_curv, variant, diff32)
    for v in out.values():
        v.setflags(write=False)
    return out


def check_conditions(case) -> dict:
    """asserts the case's input conditions on the float64 reference -> the margins found"""
    r2 = case.radius ** 2
    found = dict(pair=np.inf, curv=np.inf, trace=np.inf, exact_pairs=0)
    for b in range(len(case.counts)):
        mask = None if case.mask is None else case.mask[b]
        ok = reg_ref.participating(case.points[b], case.counts[b], mask)
        if not ok.any():
            continue
        d2 = _d2(case.points[b], ok)[np.ix_(ok, ok)]
        exact = d2 == r2
        assert case.exact_pairs or not exact.any(), (case.name, b)
        found["exact_pairs"] += int(exact.sum())
        found["pair"] = min(found["pair"], float(np.abs(d2[~exact] / r2 - 1).min()))
        for max_curv in case.max_curvs:
            out = ref(case.name, b, max_curv)
            c = out["curv_all"][np.isfinite(out["curv_all"])]
            same = c.astype(np.float32) == np.float32(max_curv)
            assert case.exact_pairs or not same.any(), (case.name, b)
            if (~same).any():
                found["curv"] = min(found["curv"], float(np.abs(c[~same] / max_curv - 1).min()))
        trace = out["lam"][ok].sum(axis=1)
        assert np.isfinite(trace).all()
        if (trace != 0).any():
            found["trace"] = min(found["trace"], float(np.abs(trace[trace != 0]).min() / r2))
    assert found["pair"] >= 1e-6, (case.name, found)
    assert found["curv"] >= 1e-5, (case.name, found)
    assert found["trace"] >= 1e-12, (case.name, found)
    return found


# ---- generators -------------------------------------------------------------------------------------------------------------------------
def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def _ball(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, 1, size=(n, 1)) ** (1.0 / 3.0)


def _case(name, points, counts=None, mask=None, *, xy_range=DEFAULT_GRID["xy_range"], cell=1.0, radius=1.0, min_pts=5,
          max_curvs=(0.05, THIRD), exact_pairs=False, **extra):
    points = np.ascontiguousarray(points, dtype=np.float32)
    if points.ndim == 2:
        points = points[None]
    B, N = points.shape[:2]
    assert N <= 1500 and B <= 3
    counts = [N] * B if counts is None else list(counts)
    points.setflags(write=False)
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.int32)
        mask.setflags(write=False)
    return SimpleNamespace(name=name, points=points, counts=counts, mask=mask, xy_range=tuple(xy_range), cell=cell, radius=radius,
                           min_pts=min_pts, max_curvs=tuple(max_curvs), exact_pairs=exact_pairs, G=grid_size(xy_range, cell), **extra)


def _generic():
    rng = np.random.default_rng(11)
    parts = []
    # two sphere caps (radius 3 m and 1.2 m) and a whole sphere that fits into one neighbourhood: curvature from 5e-3 to near 1/3
    spheres = (((10.3, 5.1, -2.0), 3.0, 330, 0.5), ((-20.4, 15.2, 0.0), 1.2, 170, 0.0), ((30.1, -30.6, 0.3), 0.45, 80, -1.0))
    for centre, R, n, zmin in spheres:
        z = rng.uniform(zmin, 1.0, n)
        phi = rng.uniform(0, 2 * np.pi, n)
        s = np.sqrt(1 - z * z)
        parts.append(np.asarray(centre) + R * np.stack((s * np.cos(phi), s * np.sin(phi), z), axis=1))
    # a sinusoidal sheet over 6 m x 6 m, across the origin
    xy = rng.uniform(-3, 3, size=(330, 2))
    parts.append(np.concatenate((xy + (-1.3, 0.7), 0.3 * np.sin(2 * xy[:, :1]) * np.sin(1.5 * xy[:, 1:]) - 1.7), axis=1))
    # a tilted plane of 5 m x 5 m whose noise grows along it from 3 mm to 0.6 m
    ab = rng.uniform(-2.5, 2.5, size=(290, 2))
    n, u, v = plane_ref._frame((0.3, -0.2, 1.0))
    sigma = 0.003 * (0.6 / 0.003) ** ((ab[:, :1] + 2.5) / 5.0)
    parts.append(np.asarray((-40.2, -39.7, 1.0)) + ab[:, :1] * u + ab[:, 1:] * v + sigma * rng.normal(size=(290, 1)) * n)
    pts = np.concatenate(parts)
    return _case("generic", pts[rng.permutation(len(pts))])


def _spread():
    rng = np.random.default_rng(5)
    nb, per = 48, 30
    centres = np.stack(np.meshgrid(np.arange(-46.0, 47.0, 4.0), np.arange(-46.0, 47.0, 4.0), indexing="ij"), axis=-1).reshape(-1, 2)
    centres = centres[rng.choice(len(centres), nb, replace=False)] + rng.uniform(-0.5, 0.5, size=(nb, 2))
    r01 = 10.0 ** np.linspace(-10, np.log10(0.9), nb)[rng.permutation(nb)]                 # lambda0 / lambda1 of the ellipsoid
    # lambda1 / lambda2: 1e-3 .. 1, six blobs below 0.02 (needle-like: gap < 0.01 trace) and the rest above it
    r12 = np.concatenate((10.0 ** np.linspace(-3, np.log10(0.02), 6), 10.0 ** np.linspace(np.log10(0.03), 0, nb - 6)))[rng.permutation(nb)]
    parts = []
    for c, a, b in zip(centres, r01, r12):
        axes = 0.45 * np.array([np.sqrt(a * b), np.sqrt(b), 1.0])                          # every pair of a blob is closer than 0.9 m
        parts.append(np.asarray((c[0], c[1], rng.uniform(-2, 2))) + (_ball(rng, per) * axes) @ _rotation(rng).T)
    return _case("spread", np.concatenate(parts), ratios=(r01, r12))


def binade_pairs(lo, edge, cell=1.0, G=103):
    """Every fp32 coordinate pair (a, b) with b - a < cell that the fp32 cell rule files in the cells edge - 1 and edge + 1, with
    (b - a)^2 <= cell^2 (1 - 1e-6): a sits just below the cell coordinate ``edge`` = a power of two, where the cell coordinate's ulp is
    half of what it is just below edge + 1, so b's cell coordinate rounds UP to edge + 1 while a's stays below edge.  Such a pair is at
    most a quarter ulp(edge) short of one cell, and it needs coordinates at least 8 x finer than ulp(edge): at lo = -51.2 only the
    edge 64 has any (ONE pair of values: the coordinates near 12.8 m are fine enough, those near -19.2 m and -35.2 m are not), at
    lo = -30.2 the edge 32 has four, and below the edge 32 no pair is 1e-6 r2 short of the radius at all."""
    a, b = (np.float32(np.float32(lo) + np.float32(e * cell)) for e in (edge, edge + 1))
    cand_a, cand_b = [a], [b]
    for _ in range(40):
        cand_a.append(np.nextafter(cand_a[-1], np.float32(-np.inf)))
        cand_b.append(np.nextafter(cand_b[-1], np.float32(-np.inf)))
    return [(a, b) for a in cand_a for b in cand_b
            if cell_f32(a, lo, cell, G) == edge - 1 and cell_f32(b, lo, cell, G) == edge + 1
            and (float(b) - float(a)) ** 2 <= cell * cell * (1 - 1e-6)]


def _binade(name, lo, edge, copies):
    rng = np.random.default_rng(2)
    found = binade_pairs(lo, edge)
    assert found, (lo, edge)
    rows, pairs = [], []
    other = lo + 5.9
    for axis in (0, 1):
        for k in range(copies):
            a, b = found[k % len(found)]
            z = np.float32(rng.uniform(-1, 1))
            for side, v in ((-1, a), (1, b)):
                p = np.array([other, other, z], dtype=np.float32)
                p[axis] = v
                rows.append(p)
                # filler: five rows within 0.3 m per axis, on the far side of the pair's partner
                f = p + rng.uniform(-0.3, 0.3, size=(5, 3)).astype(np.float32)
                f[:, axis] = p[axis] + side * rng.uniform(0.02, 0.3, size=5).astype(np.float32)
                rows.extend(f)
            pairs.append((len(rows) - 12, len(rows) - 6, axis, edge))
            other += 5.5
    return _case(name, np.stack(rows), xy_range=(lo, lo, lo + 102.4, lo + 102.4), pairs=pairs)


def binade_condition(case) -> int:
    """the number of pairs with cells 2 apart (the fp32 cell rule) and d2 <= r2 (1 - 1e-6): a condition on the input only"""
    cx, cy = cells(case.points[0], case)
    n = 0
    for i, j, axis, _ in case.pairs:
        d2 = float(((case.points[0][i].astype(np.float64) - case.points[0][j]) ** 2).sum())
        c = (cx, cy)[axis]
        n += int(abs(int(c[i]) - int(c[j])) == 2 and d2 <= case.radius ** 2 * (1 - 1e-6))
    return n


def _exact_radius(name, r, offset):
    k = np.arange(-5, 6) * r
    pts = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(offset)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    idx = np.stack(np.meshgrid(*(np.arange(11),) * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    interior = np.all((idx > 0) & (idx < 10), axis=1)
    perm = np.random.default_rng(4).permutation(len(pts))
    return _case(name, pts[perm], xy_range=(-16.0, -16.0, 16.0, 16.0), cell=r, radius=r, max_curvs=(THIRD,), exact_pairs=True,
                 interior=interior[perm])


def _border():
    rng = np.random.default_rng(9)
    N = 1400
    parts = []
    blob = np.asarray((-3.6, 3.5, 0.2)) + 0.2 * _ball(rng, 640)                              # one border cell, every pair within 0.4 m
    parts.append(blob)
    xy = rng.uniform(-4, 4, size=(330, 2))                                                   # an undulating ground over the whole range
    parts.append(np.concatenate((xy, 0.2 * np.sin(xy[:, :1]) * np.cos(0.7 * xy[:, 1:]) - 1.0 + 0.02 * rng.normal(size=(330, 1))), axis=1))
    # clusters across and outside the range's edge: the four sides and the corners, 0.1 m to 1e4 m out
    centres = []
    for d in (0.1, -0.1, 0.9, 30.0, 1e4):
        centres += [(4 + d, 0.3), (-4 - d, -1.2), (1.7, 4 + d), (-2.2, -4 - d)]
    centres += [(4.1, 4.1), (-4.1, -4.1), (4.1, -4.1), (-4.1, 4.1), (1e4, 1e4), (-1e4, 34.0), (35.0, -1e4), (-4.9, 1e4), (-1e3, -1e3)]
    for cx, cy in centres:
        flat = np.concatenate((rng.uniform(-0.25, 0.25, size=(12, 2)), 0.01 * rng.normal(size=(12, 1))), axis=1)
        parts.append(np.asarray((cx, cy, rng.uniform(-1, 1))) + flat @ _rotation(rng).T)
    pts = np.concatenate(parts).astype(np.float32)
    pad = N - len(pts) - 10
    assert pad >= 0
    pts = np.concatenate((pts, rng.uniform(-6, 6, size=(pad, 3)).astype(np.float32),
                          np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [np.nan] * 3, [np.inf, 1e4, 0], [1, np.nan, 2],
                                    [-np.inf, -np.inf, 0], [3, 3, np.nan], [np.inf] * 3, [0.5, -np.inf, 1]], dtype=np.float32)))
    order = np.concatenate((np.arange(640), 640 + rng.permutation(N - 640)))
    s0 = pts[order]
    mask = np.ones((3, N), dtype=np.int32)
    mask[0, 640:] = rng.integers(0, 10, size=N - 640) > 0                                    # sample 0: a mask that spares the blob
    mask[0, :640] = 3
    s1 = pts[rng.permutation(N)]                                                             # sample 1: rows behind count = 900
    return _case("border", np.stack((s0, s1, s0)), counts=[N - 40, 900, 0], mask=mask, xy_range=(-4.0, -4.0, 4.0, 4.0), blob=640)


def _degenerate():
    rng = np.random.default_rng(7)
    parts, where = [], {}

    def add(key, rows):
        where[key] = (sum(len(p) for p in parts), sum(len(p) for p in parts) + len(rows))
        parts.append(np.asarray(rows, dtype=np.float64))

    add("collinear", np.asarray((8.0, 8.0, 1.0)) + np.arange(-4, 5)[:, None] * np.asarray((0.125, 0.0625, 0.03125)))
    add("copies", np.tile((20.25, -12.5, 3.0), (40, 1)))
    add("four", np.asarray((-10.0, 20.0, 0.0)) + rng.uniform(-0.3, 0.3, size=(4, 3)))
    add("five", np.asarray((-20.0, 20.0, 0.0)) + rng.uniform(-0.3, 0.3, size=(5, 3)))
    a, b = np.meshgrid(np.arange(15) - 7.0, np.arange(15) - 7.0, indexing="ij")
    xy = 0.4 * np.stack((a, b), axis=-1).reshape(-1, 2) + rng.uniform(-0.1, 0.1, size=(225, 2)) + (-30.0, 30.0)
    add("flat", np.concatenate((xy, np.zeros((225, 1))), axis=1))
    n, u, v = plane_ref._frame((-0.3, 0.5, 0.8))
    ab = rng.uniform(-0.6, 0.6, size=(14, 2))
    add("origin", np.concatenate((np.zeros((1, 3)), ab[:, :1] * u + ab[:, 1:] * v + 0.002 * rng.normal(size=(14, 1)) * n)))
    add("tiny", np.asarray((50.3, -49.7, 2.0)) + rng.uniform(-5e-4, 5e-4, size=(12, 3)))
    return _case("degenerate", np.concatenate(parts), xy_range=(-64.0, -64.0, 64.0, 64.0), where=where)


_MAKERS = dict(generic=_generic, spread=_spread, binade=lambda: _binade("binade", -51.2, 64, 3),
               binade_33=lambda: _binade("binade_33", -30.2, 32, 4),
               exact_radius=lambda: _exact_radius("exact_radius", 1.0, (0.0, 0.0, 0.0)),
               exact_radius_half=lambda: _exact_radius("exact_radius_half", 0.5, (0.25, 0.125, 0.0)), border=_border,
               degenerate=_degenerate)


@functools.lru_cache(maxsize=None)
def case(name):
    return _MAKERS[name]()


# ---- the comparison of a result with the reference, shared by the CPU and the GPU tests -------------------------------------------------
def compare(case, b, max_curv, n, curv, m, bound=16 * EPS, against=None) -> dict:
    """Holds n [N,3], curv [N], m [N] of sample b (fp32 / int, or a float64 result of another reference) against ``against`` (default:
    the exact-differences reference), every row, by the rules of the issue that set this file up.  Asserts; -> the worst figures."""
    want = ref(case.name, b, max_curv) if against is None else against
    pts = case.points[b]
    n, curv, m = np.asarray(n), np.asarray(curv), np.asarray(m)
    assert np.array_equal(m, want["m"]), (case.name, b, np.flatnonzero(m != want["m"])[:10])
    valid = curv >= 0
    assert np.array_equal(valid, want["valid"]), (case.name, b, np.flatnonzero(valid != want["valid"])[:10])
    assert np.all(n[~valid] == 0) and not np.signbit(n[~valid]).any() and np.all(curv[~valid] == -1), (case.name, b)
    ok = reg_ref.participating(pts, case.counts[b], None if case.mask is None else case.mask[b])
    assert np.all(m[~ok] == 0) and not valid[~ok].any()
    worst = dict(valid=int(valid.sum()), rows=int(ok.sum()), angle=0.0, angle_ratio=0.0, residual_ratio=0.0, curv=0.0, norm=0.0, gapped=0)
    if not valid.any():
        return worst
    p64, n64 = pts[valid].astype(np.float64), n[valid].astype(np.float64)
    worst["norm"] = float(np.abs(np.linalg.norm(n64, axis=1) - 1).max())
    dot = (n64[:, 0] * p64[:, 0] + n64[:, 1] * p64[:, 1]) + n64[:, 2] * p64[:, 2]
    lead = np.where(n64[:, 0] != 0, n64[:, 0], np.where(n64[:, 1] != 0, n64[:, 1], n64[:, 2]))
    lam, C, nr = want["lam"][valid], want["cov"][valid], want["n"][valid]
    trace, gap = lam.sum(axis=1), lam[:, 1] - lam[:, 0]
    res = np.linalg.norm(np.einsum("kij,kj->ki", C, n64) - lam[:, :1] * n64, axis=1)
    worst["residual_ratio"] = float((res / (bound * trace)).max())
    worst["curv"] = float(np.abs(curv[valid].astype(np.float64) - want["curv"][valid]).max())
    sel = gap >= 0.01 * trace
    worst["gapped"] = int(sel.sum())
    if sel.any():
        angle = np.arctan2(np.linalg.norm(np.cross(n64[sel], nr[sel]), axis=1), np.abs((n64[sel] * nr[sel]).sum(axis=1)))
        worst["angle"], worst["angle_ratio"] = float(angle.max()), float((angle / (bound * trace[sel] / gap[sel])).max())
    print(f"[{case.name} b={b} max_curv={max_curv:.3g}] rows {worst['rows']} valid {worst['valid']} gapped {worst['gapped']}: "
          f"| |n| - 1 | {worst['norm']:.3g}, angle {worst['angle']:.3g} rad = {worst['angle_ratio']:.3g} of the bound, residual "
          f"{worst['residual_ratio']:.3g} of the bound, |curv - ref| {worst['curv']:.3g}")
    assert worst["norm"] <= 4 * EPS
    assert np.all(dot <= 0) and np.all(lead[dot == 0] > 0)                                  # towards the origin; the tie-break on 0
    assert worst["curv"] <= bound
    assert worst["residual_ratio"] <= 1
    assert np.all((n64[sel] * nr[sel]).sum(axis=1) > 0)                                     # the same side as the reference's
    assert worst["angle_ratio"] <= 1
    return worst


def differs(a, b) -> bool:
    """two reference results disagree in m, in validity or in n"""
    return bool(not np.array_equal(a["m"], b["m"]) or not np.array_equal(a["valid"], b["valid"]) or np.abs(a["n"] - b["n"]).max() > 1e-6)
