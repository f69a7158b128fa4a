"""Named inputs that pin the two searches over the xy row grid of df_nn_grid_build at cell edges, exact radii and ring ties:

  * the ring walk nn_ring_search (csrc/nn_search.h) behind df_chamfer_nn, df_reg_accumulate and df_reg_accumulate_plane;
  * the fixed-radius window of csrc/cluster.hip (nn_search.h: nn_window) behind df_dbscan_core, _link and _finish.

For the walk: ``ring_walk``, a numpy restatement of nn_ring_search (the fp32 cell rule, rings at Chebyshev distance r, the lower bound and
the break as nn_search.h writes them) with its deliberately WRONG variants, and the float64 all-pairs reference seflow_ref.nn_padded.
For DBSCAN: dbscan_ref.dbscan_ref_padded and its wrong variants ``strict`` (d2 < eps2) and ``cells3x3`` (neighbours only from the 3 x 3
cells of the fp32 cell rule).  tests/test_grid_cases_cpu.py asserts every case's input conditions and that each wrong variant is caught by
the case built for it; tests/test_gpu_grid_cases.py holds the kernels to the references.

Search cases (N <= 1500 rows per sample, B <= 3; every query row is walked on the CPU, so all rows are "designated"):
  beyond_square, beyond_square_33   a query that is member a of a binade pair (normals_cases.binade_pairs): its nearest row b is filed TWO
                    cells away although it is less than one cell away, and a decoy inside the query's 3 x 3 cells is farther than b but
                    nearer than the unslacked bound of ring 1: without the 2e-3 slack the walk stops at the decoy.  Along x and along y.
  ring_ties         a dyadic lattice (cell 1, origin -32): candidates at bit-equal distances in different rings with the lowest row in the
                    outermost; queries on a cell edge and on a cell corner; a query whose unslacked bound equals ``best`` exactly
  z_column          the only rows in and around the query's cell are 20 .. 40 m away in z, the true neighbour 4 .. 6 cells away in xy
  exact_gate, exact_gate_below, exact_gate_zero   the lattice with max_dist2 == some queries' nearest d2, one fp32 step below it, and 0
  g1, g4096, outside, single_ref, one_cell, sparse, sparse_gated   the ``extremes``

DBSCAN cases: exact_eps_{1,half} x min_points {7, 8}, count_stop x {1, 2, 600}, binade_abi_{1,half}, rank_edges_{256,257,1025}."""
from __future__ import annotations

import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dbscan_ref  # noqa: E402
import normals_cases as nc  # noqa: E402
import reg_ref  # noqa: E402
import seflow_ref  # noqa: E402

F = np.float32
INF = float("inf")
DEFAULT_RANGE = nc.DEFAULT_GRID["xy_range"]
CELL_SLACK = 1.0025                    # deflow_amd/cluster.py (asserted equal in the CPU test)
SEARCH_NAMES = ("beyond_square", "beyond_square_33", "ring_ties", "z_column", "exact_gate", "exact_gate_below", "exact_gate_zero", "g1",
                "g4096", "outside", "single_ref", "one_cell", "sparse", "sparse_gated")
DYADIC = ("ring_ties", "exact_gate", "exact_gate_below", "exact_gate_zero")
WALK_VARIANTS = {"slack0": dict(slack=0.0), "stop_on_equal": dict(slack=0.0, stop_on_equal=True), "ring_cap1": dict(ring_cap=1),
                 "first_seen": dict(tie="first_seen"), "z_bound": dict(z_bound=True)}


def grid_of(xy_range, cell):
    return SimpleNamespace(xy_range=tuple(xy_range), cell=float(cell), G=min(nc.grid_size(xy_range, cell), 4096))


# ---- nn_ring_search restated ------------------------------------------------------------------------------------------------------------
class Filed:
    """the participating rows of one sample's refs with their cells by the fp32 cell rule (what df_nn_grid_build files)"""

    def __init__(self, refs, ok, grid):
        refs = np.asarray(refs, dtype=F)
        self.rows = np.flatnonzero(ok)
        self.p = refs[self.rows]
        self.cx = nc.cell_f32(self.p[:, 0], grid.xy_range[0], grid.cell, grid.G)
        self.cy = nc.cell_f32(self.p[:, 1], grid.xy_range[1], grid.cell, grid.G)


def _pos(v, lo, cell, G):
    """nn_cell: the clamped position in cell units (fp32) and the cell"""
    f = min(max((F(v) - F(lo)) * (F(1.0) / F(cell)), F(0.0)), F(G))
    return F(f), min(int(f), G - 1)


def ring_walk(query, refs, grid, max_dist2=INF, *, slack=2e-3, stop_on_equal=False, ring_cap=None, tie="lowest", z_bound=False, ok=None,
              trace=None):
    """nn_ring_search for ONE finite query [3] over refs (a ``Filed``, or [N,3] with the participating rows in ``ok``), in fp32 as the
    kernel computes (products and sums rounded one by one: no fma) -> (idx, rings_walked): the row named (-1 when none lies within
    max_dist2: the callers' gate) and the number of the last ring scanned.  The keywords are the kernel's rule by default and the
    WRONG variants otherwise: slack=0 (no allowance for the rounding of the cell coordinates), stop_on_equal (break on lb2 >= best),
    ring_cap=k (never past ring k), tie='first_seen' (an equal distance never replaces the row held), z_bound (the bound adds the z
    difference of the row held, as if unseen rows could not be nearer in z).  trace (a dict): 'best' = the fp32 distance found,
    'margin' = the smallest |lb2 / best - 1| over the break decisions taken on lb2 > best (how far each was from flipping)."""
    f = refs if isinstance(refs, Filed) else Filed(refs, np.ones(len(refs), bool) if ok is None else ok, grid)
    G, cell = grid.G, F(grid.cell)
    q = np.asarray(query, dtype=F)
    px, cx = _pos(q[0], grid.xy_range[0], grid.cell, G)
    py, cy = _pos(q[1], grid.xy_range[1], grid.cell, G)
    best, bi, bz = F(np.inf), -1, F(0.0)
    margin = np.inf
    if len(f.rows):
        d = f.p - q
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]             # fp32, left to right
        ring = np.maximum(np.abs(f.cx - cx), np.abs(f.cy - cy))
        order = np.lexsort((f.rows, f.cx, f.cy, ring))                                # by ring, then the kernel's scan order
        ring_s, d2_s, rows_s, dz_s = ring[order], d2[order], f.rows[order], d[order, 2]
        starts = np.searchsorted(ring_s, np.arange(G + 2))
    r = 0
    max2 = F(max_dist2) if np.isfinite(max_dist2) else F(np.inf)
    while r <= G:
        if ring_cap is not None and r > ring_cap:
            r -= 1
            break
        if len(f.rows):
            s, e = starts[r], starts[r + 1]
            if e > s:
                dd = d2_s[s:e]
                k = int(np.argmin(dd))                                                # (the first minimum: first in scan order)
                if tie == "lowest":
                    k = s + int(np.flatnonzero(dd == dd[k])[np.argmin(rows_s[s:e][dd == dd[k]])])
                    if dd[k - s] < best or (dd[k - s] == best and rows_s[k] < bi):
                        best, bi, bz = dd[k - s], int(rows_s[k]), dz_s[k]
                else:
                    if dd[k] < best:
                        best, bi, bz = dd[k], int(rows_s[s + k]), dz_s[s + k]
        x0, x1, y0, y1 = cx - r, cx + r, cy - r, cy + r
        lb = F(np.inf)
        if x0 > 0:
            lb = min(lb, px - F(x0))
        if x1 < G - 1:
            lb = min(lb, F(x1 + 1) - px)
        if y0 > 0:
            lb = min(lb, py - F(y0))
        if y1 < G - 1:
            lb = min(lb, F(y1 + 1) - py)
        if not lb < np.inf:
            break
        lb = F(max(F(lb - F(slack)), F(0.0)) * cell)
        lb2 = F(lb * lb)
        if z_bound and bi >= 0:
            lb2 = F(lb2 + bz * bz)
        if np.isfinite(best) and best > 0 and not (lb2 > max2):
            margin = min(margin, abs(float(lb2) / float(best) - 1))
        if (lb2 >= best or lb2 >= max2) if stop_on_equal else (lb2 > best or lb2 > max2):
            break
        r += 1
    if trace is not None:
        trace["best"], trace["margin"] = best, margin
    return (bi if best <= max2 else -1), r


# ---- search cases -----------------------------------------------------------------------------------------------------------------------
def _search(name, query, refs, *, qcount=None, rcount=None, qlabel=None, rlabel=None, xy_range=DEFAULT_RANGE, cell=1.0, max_dist2=INF,
            narrow=(), **extra):
    query, refs = (np.ascontiguousarray(a, dtype=F) for a in (query, refs))
    if query.ndim == 2:
        query, refs = query[None], refs[None]
    B = query.shape[0]
    assert B <= 3 and query.shape[1] <= 1500 and refs.shape[1] <= 1500
    for a in (query, refs):
        a.setflags(write=False)
    g = grid_of(xy_range, cell)
    return SimpleNamespace(name=name, query=query, refs=refs, qcount=[query.shape[1]] * B if qcount is None else list(qcount),
                           rcount=[refs.shape[1]] * B if rcount is None else list(rcount), qlabel=qlabel, rlabel=rlabel, grid=g,
                           xy_range=g.xy_range, cell=g.cell, G=g.G, max_dist2=float(max_dist2), narrow=tuple(narrow),
                           dyadic=name in DYADIC, **extra)


def _beyond_square(name, lo, edge):
    """per axis and pair: query a, partner b (filed two cells on), a decoy straight above the query with partner d2 < decoy d2 < the
    unslacked bound of ring 1, and a far ref so that the query's 3 x 3 cells are otherwise empty.  Plus ordinary rows elsewhere."""
    rng = np.random.default_rng(3)
    found = nc.binade_pairs(lo, edge)
    assert found, (lo, edge)
    q, r, rows = [], [], []
    other = lo + 7.5
    for axis in (0, 1):
        for k in range(4):
            a, b = found[k % len(found)]
            z = F(0.0)                                                           # (the decoy's dz = its z: exact in fp32)
            qa = np.array([other, other, z], dtype=F)
            qa[axis] = a
            pb = qa.copy()
            pb[axis] = b
            px, _ = _pos(a, lo, 1.0, 103)
            lb_un = F(F(edge + 1) - px)
            d_partner = F((F(b) - F(a)) * (F(b) - F(a)))
            dz = F(np.sqrt(0.5 * (float(d_partner) + float(F(lb_un * lb_un)))))
            decoy = qa.copy()
            decoy[2] = F(z + dz)
            rows.append((len(q), len(r), len(r) + 1, axis))                     # (query row, partner row, decoy row, axis)
            q.append(qa)
            r.extend([pb, decoy])
            other += 6.0                                                         # (stays at the middle of a cell)
    fill_q = rng.uniform(-15, 15, size=(120, 3)) * (1, 1, 0.1) + (lo + 85, lo + 85, 0)
    fill_r = rng.uniform(-15, 15, size=(200, 3)) * (1, 1, 0.1) + (lo + 85, lo + 85, 0)
    perm = rng.permutation(len(r) + len(fill_r))                                 # refs in shuffled row order
    refs = np.concatenate((np.stack(r), fill_r.astype(F)))[perm]
    inv = np.argsort(perm)
    rows = [(i, int(inv[p]), int(inv[d]), ax) for i, p, d, ax in rows]
    return _search(name, np.concatenate((np.stack(q), fill_q.astype(F))), refs, xy_range=(lo, lo, lo + 102.4, lo + 102.4), cell=1.0,
                   pairs=rows, narrow=[i for i, *_ in rows], edge=edge)


def _ring_ties():
    """refs and queries with dyadic coordinates, groups 8 m apart along x at y = 0.  Each group: (query, [refs in ROW order])."""
    groups = [
        # equal distances (6.25) in rings 2, 1, 0 -- the lowest row in ring 2; and a second ring-2 candidate
        ((0.25, 0.25, 0.0), [(2.25, 0.25, 1.5), (1.75, 0.25, 2.0), (0.25, 0.25, 2.5), (2.75, 0.25, 0.0)]),
        # the same with the rings along y and the lowest row in ring 1, the highest in ring 0
        ((0.25, 0.25, 0.0), [(0.25, 1.75, -2.0), (0.25, 2.25, -1.5), (0.25, 0.25, -2.5)]),
        # on a cell edge (x an integer): the equal candidates on either side, the lower row in the cell below (ring 1)
        ((0.0, 0.5, 0.0), [(-0.5, 0.5, 0.0), (0.5, 0.5, 0.0)]),
        # on a cell corner: four diagonal candidates, the lowest row in the diagonal cell below
        ((0.0, 0.0, 0.0), [(-0.5, -0.5, 0.0), (0.5, 0.5, 0.0), (-0.5, 0.5, 0.0), (0.5, -0.5, 0.0)]),
        # the unslacked bound of ring 0 (17 - 16.75 = 0.25 cell) equals best: the ring-1 row AT the next cell's edge has the lower index
        ((0.75, 0.5, 0.0), [(1.0, 0.5, 0.0), (0.75, 0.5, 0.25)]),
        # the same along y, three equal candidates, the lowest row at the edge of the cell above
        ((0.5, 0.75, 0.0), [(0.5, 1.0, 0.0), (0.5, 0.75, -0.25), (0.75, 0.75, 0.0)]),
        # no tie at all: a plain nearest in ring 1
        ((0.5, 0.5, 0.0), [(1.25, 0.5, 0.0), (0.5, 2.5, 0.0)]),
    ]
    q, r, owner = [], [], []
    for g, (qq, rr) in enumerate(groups):
        off = np.array([-24.0 + 8.0 * g, 0.0, 0.0])
        q.append(np.asarray(qq) + off)
        for p in rr:
            r.append(np.asarray(p) + off)
            owner.append(g)
    return _search("ring_ties", np.stack(q), np.stack(r), xy_range=(-32.0, -32.0, 32.0, 32.0), cell=1.0, groups=len(groups),
                   first_ref=[owner.index(g) for g in range(len(groups))], bound_equal=(4, 5))


def _z_column():
    rng = np.random.default_rng(8)
    q, r = [], []
    for k in range(24):
        c = np.array([-40.0 + 14.0 * (k % 6), -30.0 + 18.0 * (k // 6), 0.0]) + rng.uniform(-0.4, 0.4, 3)
        q.append(c)
        sign = 1.0 if k % 2 else -1.0
        for _ in range(6):                                                      # the column: in and around the query's cell, far in z
            r.append(c + np.append(rng.uniform(-1.2, 1.2, 2), sign * rng.uniform(20, 40)))
        ang = rng.uniform(0, 2 * np.pi)
        far = rng.uniform(4.3, 5.7)
        r.append(c + np.array([far * np.cos(ang), far * np.sin(ang), rng.uniform(-0.3, 0.3)]))    # the true neighbour
    r = np.stack(r)
    return _search("z_column", np.stack(q), r[rng.permutation(len(r))])


def _lattice_gate(name, max_dist2):
    k = np.arange(-4, 5, dtype=np.float64)
    nodes = np.stack(np.meshgrid(k, k, np.array([-1.0, 0.0, 1.0]), indexing="ij"), axis=-1).reshape(-1, 3)
    rng = np.random.default_rng(6)
    refs = nodes[rng.permutation(len(nodes))]
    inner = nodes[(np.abs(nodes[:, :2]).max(axis=1) <= 3) & (nodes[:, 2] == 0)]
    q, kind = [], []
    offs = {0.0: (0.0, 0.0, 0.0), 0.0625: (0.25, 0.0, 0.0), 0.125: (0.25, 0.25, 0.0), 0.1875: (0.25, 0.25, 0.25)}
    for i, n in enumerate(inner):
        d2 = list(offs)[i % 4]
        sgn = np.array([1 if (i >> 2) & 1 else -1, 1 if (i >> 3) & 1 else -1, 1 if (i >> 4) & 1 else -1])
        q.append(n + sgn * np.asarray(offs[d2]))
        kind.append(d2)
    return _search(name, np.stack(q), refs, xy_range=(-16.0, -16.0, 16.0, 16.0), cell=1.0, max_dist2=max_dist2, nearest_d2=np.asarray(kind))


def _g1():
    rng = np.random.default_rng(12)
    return _search("g1", rng.uniform(-3, 3, size=(2, 150, 3)), rng.uniform(-3, 3, size=(2, 260, 3)), qcount=[150, 97], rcount=[260, 33],
                   xy_range=(-0.3, -0.3, 0.4, 0.4), cell=1.0)


def _filter_queries(cands, refs, rok, n, gap=1e-4):
    """the first n candidate queries whose float64 best and second-best squared distances differ by more than ``gap`` relative"""
    p = refs[rok].astype(np.float64)
    d = ((cands.astype(F).astype(np.float64)[:, None, :] - p[None]) ** 2).sum(axis=2)
    d.sort(axis=1)
    good = np.flatnonzero((d[:, 1] - d[:, 0] > gap * d[:, 0]) if d.shape[1] > 1 else np.ones(len(d), bool))
    assert len(good) >= n, (len(good), n)
    return cands[good[:n]]


def _g4096():
    """refs and queries at the cell coordinates 0 .. 2 and 4090 .. 4096 of a 4096-cell grid, in x and in y (the four corner regions)"""
    rng = np.random.default_rng(13)
    cell = 102.4 / 4096

    def pts(n):
        u = np.where(rng.integers(0, 2, size=(n, 2)) == 1, rng.uniform(4090, 4096, size=(n, 2)), rng.uniform(0, 2, size=(n, 2)))
        return np.concatenate((-51.2 + u * cell, rng.uniform(-0.02, 0.02, size=(n, 1))), axis=1).astype(F)

    refs = pts(400)
    q = _filter_queries(pts(500), refs, np.ones(400, bool), 300)
    return _search("g4096", q, refs, cell=cell, max_dist2=(10 * cell) ** 2)


def _outside():
    """G = 8: rows up to 1e4 m outside the range on all four sides and at the corners, a border cell of 600 refs, counts and labels"""
    rng = np.random.default_rng(14)
    centres = []
    for d in (0.1, 0.9, 30.0, 1e4):
        centres += [(4 + d, 0.3), (-4 - d, -1.2), (1.7, 4 + d), (-2.2, -4 - d)]
    centres += [(4.1, 4.1), (-4.1, -4.1), (4.1, -4.1), (-4.1, 4.1), (1e4, 1e4), (-1e4, 34.0), (35.0, -1e4), (-4.9, 1e4), (-1e3, -1e3)]
    parts = [np.asarray((-3.6, 3.5, 0.2)) + 0.2 * nc._ball(rng, 600)]
    for cx, cy in centres:
        parts.append(np.asarray((cx, cy, 0.0)) + rng.uniform(-0.4, 0.4, size=(8, 3)))
    parts.append(rng.uniform(-4, 4, size=(150, 3)))
    refs = np.concatenate(parts).astype(F)
    refs = np.concatenate((refs[:600], refs[600:][rng.permutation(len(refs) - 600)]))
    refs[700] = np.nan
    refs[701, 1] = np.inf
    cq = [rng.uniform(-6, 6, size=(300, 3))]
    for cx, cy in centres:
        cq.append(np.asarray((cx, cy, 0.0)) + rng.uniform(-1.5, 1.5, size=(10, 3)))
    cq = np.concatenate(cq)
    cq = cq[rng.permutation(len(cq))]
    rlabel = np.ones((2, len(refs)), dtype=np.int32)
    rlabel[1, rng.uniform(size=len(refs)) < 0.3] = 0
    rcount = [len(refs), len(refs) - 60]
    qs = []
    for b in range(2):
        rok = reg_ref.participating(refs, rcount[b], rlabel[b])
        qs.append(_filter_queries(cq, refs, rok, 400))
    q = np.stack(qs).astype(F)
    q[0, 17] = np.nan
    qlabel = np.ones((2, 400), dtype=np.int32)
    qlabel[1, ::7] = 0
    return _search("outside", q, np.stack((refs, refs)), qcount=[400, 380], rcount=rcount, qlabel=qlabel, rlabel=rlabel,
                   xy_range=(-4.0, -4.0, 4.0, 4.0), cell=1.0, crowd=600)


def _single_ref():
    rng = np.random.default_rng(15)
    refs = rng.uniform(-50, 50, size=(40, 3)) * (1, 1, 0.05)
    rlabel = np.zeros((1, 40), dtype=np.int32)
    rlabel[0, 23] = 2                                                            # the one participating row
    refs[5] = np.nan
    return _search("single_ref", rng.uniform(-60, 60, size=(200, 3)) * (1, 1, 0.05), refs, rlabel=rlabel)


def _one_cell():
    rng = np.random.default_rng(16)
    refs = np.asarray((10.3, -20.7, 0.0)) + rng.uniform(-0.45, 0.45, size=(500, 3))
    cands = np.asarray((10.3, -20.7, 0.0)) + rng.uniform(-30, 30, size=(400, 3)) * (1, 1, 0.02)
    return _search("one_cell", _filter_queries(cands, refs.astype(F), np.ones(500, bool), 250), refs)


def _sparse(name, max_dist2):
    rng = np.random.default_rng(17)
    refs = np.array([(-40.3, -38.2, 0.1), (35.7, 41.2, -0.2), (2.4, -3.3, 0.0), (-44.1, 44.6, 0.3), (47.2, -45.9, 0.1)])
    near = np.concatenate([p + rng.uniform(-1.3, 1.3, size=(12, 3)) * (1, 1, 0.01) for p in refs])      # within the gate of sparse_gated
    cands = np.concatenate((rng.uniform(-51, 51, size=(300, 3)) * (1, 1, 0.01), near))[rng.permutation(360)]
    return _search(name, _filter_queries(cands, refs.astype(F), np.ones(5, bool), 250), refs, max_dist2=max_dist2)


_SEARCH = dict(beyond_square=lambda: _beyond_square("beyond_square", -51.2, 64), beyond_square_33=lambda: _beyond_square("beyond_square_33", -30.2, 32),
               ring_ties=_ring_ties, z_column=_z_column, exact_gate=lambda: _lattice_gate("exact_gate", 0.125),
               exact_gate_below=lambda: _lattice_gate("exact_gate_below", float(np.nextafter(F(0.125), F(0.0)))),
               exact_gate_zero=lambda: _lattice_gate("exact_gate_zero", 0.0), g1=_g1, g4096=_g4096, outside=_outside, single_ref=_single_ref,
               one_cell=_one_cell, sparse=lambda: _sparse("sparse", INF), sparse_gated=lambda: _sparse("sparse_gated", 2.25))


@functools.lru_cache(maxsize=None)
def search_case(name):
    return _SEARCH[name]()


def _t(a, dtype=None):
    return None if a is None else torch.as_tensor(np.array(a), dtype=dtype)      # (a copy: the cases' arrays are read-only)


@functools.lru_cache(maxsize=None)
def search_ref(name):
    """float64 all pairs (seflow_ref.nn_padded) of the named case, once: d2 [B,Nq] f64, idx [B,Nq], second-best d2, and the
    participating queries [B,Nq] bool -- read-only numpy"""
    c = search_case(name)
    d2, idx, d2nd = seflow_ref.nn_padded(_t(c.query).double(), c.qcount, _t(c.refs).double(), c.rcount, _t(c.qlabel), _t(c.rlabel),
                                         c.max_dist2, second=True)
    part = np.stack([reg_ref.participating(c.query[b], c.qcount[b], None if c.qlabel is None else c.qlabel[b]) for b in range(len(c.qcount))])
    out = dict(d2=d2.numpy(), idx=idx.numpy().astype(np.int64), d2nd=d2nd.numpy(), part=part)
    for v in out.values():
        v.setflags(write=False)
    return out


def refs_ok(c, b):
    return reg_ref.participating(c.refs[b], c.rcount[b], None if c.rlabel is None else c.rlabel[b])


@functools.lru_cache(maxsize=None)
def walk(name, variant=None):
    """``ring_walk`` (the kernel's rule, or the named wrong variant) on every participating query of the case -> idx [B,Nq] (-1 elsewhere),
    rings [B,Nq] (-1 elsewhere), the smallest break margin"""
    c = search_case(name)
    kw = {} if variant is None else WALK_VARIANTS[variant]
    part = search_ref(name)["part"]
    idx = np.full(part.shape, -1, dtype=np.int64)
    rings = np.full(part.shape, -1, dtype=np.int64)
    margin = np.inf
    for b in range(part.shape[0]):
        f = Filed(c.refs[b], refs_ok(c, b), c.grid)
        for i in np.flatnonzero(part[b]):
            t = {}
            idx[b, i], rings[b, i] = ring_walk(c.query[b, i], f, c.grid, c.max_dist2, trace=t, **kw)
            margin = min(margin, t["margin"])
    return idx, rings, margin


def search_conditions(name) -> dict:
    """every participating query's best and second-best float64 d2 differ by more than 1e-5 relative, or are equal bit for bit (the
    dyadic cases), or -- the rows ``narrow`` of beyond_square -- by at least 8 fp32 ulp with each formed by ONE rounding (one non-zero
    difference, exact in fp32): the window between the partner and the unslacked bound of ring 1 is narrower than 1e-5.
    -> counts (clear, exact ties, narrow)"""
    c, ref = search_case(name), search_ref(name)
    clear = exact = narrow = 0
    for b in range(ref["part"].shape[0]):
        rok = refs_ok(c, b)
        p = c.refs[b][rok].astype(np.float64)
        for i in np.flatnonzero(ref["part"][b]):
            if len(p) < 2:
                clear += 1
                continue
            d = np.sort(((p - c.query[b, i].astype(np.float64)) ** 2).sum(axis=1))
            if d[1] - d[0] > 1e-5 * d[0]:
                clear += 1
            elif d[1] == d[0]:
                assert c.dyadic, (name, b, i)
                exact += 1
            else:
                assert b == 0 and i in c.narrow, (name, b, i, d[:2])
                assert float(F(d[1])) - float(F(d[0])) >= 8 * float(np.spacing(F(d[0]))), (name, i, d[:2])
                narrow += 1
    return dict(clear=clear, exact=exact, narrow=narrow)


# ---- DBSCAN cases -----------------------------------------------------------------------------------------------------------------------
def _dbscan(name, points, *, eps, min_points, min_cluster_size=1, count=None, xy_range=DEFAULT_RANGE, cell=None, exact_pairs=False, **extra):
    points = np.ascontiguousarray(points, dtype=F)
    if points.ndim == 2:
        points = points[None]
    B, N = points.shape[:2]
    assert B <= 3 and N <= 1500
    points.setflags(write=False)
    cell = CELL_SLACK * eps if cell is None else cell
    g = grid_of(xy_range, cell)
    return SimpleNamespace(name=name, points=points, count=[N] * B if count is None else list(count), eps=float(eps), min_points=int(min_points),
                           min_cluster_size=int(min_cluster_size), grid=g, xy_range=g.xy_range, cell=g.cell, G=g.G, exact_pairs=exact_pairs,
                           **extra)


def _exact_eps(name, eps, min_points):
    base = nc.case("exact_radius" if eps == 1.0 else "exact_radius_half")          # the dyadic lattice with spacing == eps
    return _dbscan(name, base.points[0], eps=eps, min_points=min_points, exact_pairs=True, interior=base.interior)


def _count_stop(name, min_points):
    """eps 0.7 through cluster.dbscan's grid (cell 1.0025 eps over the default range): one cell of 640 rows -- a ball A of 597 rows,
    three probes with exactly 599, 600 and 601 rows within eps (itself, A, and 1, 2, 3 dependents that only the probe reaches: a
    dependent is labelled only if its probe is core), and isolated rows above; every row of A has exactly 600 (itself, A, the probes)."""
    rng = np.random.default_rng(21)
    eps = 0.7
    cell = CELL_SLACK * eps
    c = np.array([-51.2 + 90.5 * cell, -51.2 + 61.5 * cell, 0.0])                # the centre of cell (90, 61)
    A = c + 0.01 * nc._ball(rng, 597)
    probes = c + np.array([(-0.3, -0.3, 0.5), (-0.3, -0.3, -0.5), (0.3, 0.3, 0.0)])
    deps = c + np.array([(-0.3, -0.3, 1.1), (-0.3, -0.3, -1.1), (-0.3, -0.3, -1.15), (0.3, 0.3, 0.65), (0.3, 0.3, -0.65), (0.3, 0.3, 0.62)])
    lone = c + np.stack((np.zeros(34), np.zeros(34), 10.0 + 2.0 * np.arange(34)), axis=1)
    blobs = [np.asarray((x, y, 0.0)) + rng.uniform(-0.25, 0.25, size=(n, 3)) for x, y, n in ((20.0, 20.0, 12), (-30.0, 5.0, 3), (0.0, -40.0, 30))]
    pts = np.concatenate([A, probes, deps, lone] + blobs)
    perm = rng.permutation(len(pts))
    inv = np.argsort(perm)
    return _dbscan(name, pts[perm], eps=eps, min_points=min_points, crowd=inv[:640], A=inv[:597], probes=inv[597:600],
                   deps=(inv[600:601], inv[601:603], inv[603:606]))


def _binade_abi(name, eps, edge):
    """eps == cell on the default range.  Per axis: two copies of two groups of six core rows whose only link is a binade pair (a, b),
    and one binade pair whose member a is alone: a border row whose only core row within eps is its partner b."""
    rng = np.random.default_rng(22)
    lo = DEFAULT_RANGE[0]
    G = nc.grid_size(DEFAULT_RANGE, eps)
    found = nc.binade_pairs(lo, edge, eps, G)
    assert found, (eps, edge)
    rows, links, borders = [], [], []
    other = lo + 6.1
    for axis in (0, 1):
        for k in range(3):
            a, b = found[k % len(found)]
            z = F(rng.uniform(-1, 1))
            ends = []
            for side, v in ((-1, a), (1, b)):
                p = np.array([other, other, z], dtype=F)
                p[axis] = v
                ends.append(len(rows))
                rows.append(p)
                if k == 2 and side == -1:
                    continue                                                     # the lone member: no group of its own
                f = p + (eps * rng.uniform(-0.3, 0.3, size=(5, 3))).astype(F)
                f[:, axis] = p[axis] + side * (eps * rng.uniform(0.02, 0.3, size=5)).astype(F)
                rows.extend(f)
            (borders if k == 2 else links).append((ends[0], ends[1], axis))
            other += 5.5
    return _dbscan(name, np.stack(rows), eps=eps, min_points=4, cell=eps, links=links, borders=borders, edge=edge)


def _rank_edges(name, N):
    """eps 0.7, min_points 3, min_cluster_size 5: tight groups (every member core, the root = the lowest row) with chosen root rows,
    a star whose only core row is the LAST row, a group of three between two survivors that the size filter drops, isolated rows else"""
    eps = 0.7
    rng = np.random.default_rng(23)
    k = np.arange(11) * 1.5
    iso = np.stack(np.meshgrid(k - 40.0, k - 40.0, k[:9], indexing="ij"), axis=-1).reshape(-1, 3)      # 1089 rows, 1.5 m apart
    pts = iso[rng.permutation(len(iso))[:N]].copy()
    groups = {"first": (1, 6), "mid": (N // 2, 6), "drop": (N // 2 + 5, 3), "late": (N - 20, 6)}
    taken = {root for root, _ in groups.values()} | {N - 1}
    roots = {}
    for g, (key, (root, size)) in enumerate(groups.items()):
        members, nxt = [root], root + 2
        while len(members) < size:                                                # every other free row above the root
            if nxt not in taken:
                members.append(nxt)
                nxt += 1
            nxt += 1
        if key == "first":
            members[-1] = N - 2                                                   # one member of the first group far behind
        assert all(0 <= m < N - 1 for m in members) and not (set(members[1:]) & taken), (key, members)
        taken.update(members)
        centre = np.array([30.0, -30.0 + 6.0 * g, 20.0])
        pts[members] = centre + rng.uniform(-0.15, 0.15, size=(size, 3))
        roots[key] = root
    star = [N - 1] + [s for s in range(N - 12, N - 1) if s not in taken][:6]
    centre = np.array([30.0, 10.0, 20.0])
    pts[star] = centre + np.concatenate((np.zeros((1, 3)), 0.9 * eps * np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])))
    roots["star"] = N - 1
    return _dbscan(name, pts, eps=eps, min_points=3, min_cluster_size=5, roots=roots)


_DBSCAN = {}
for _e, _tag in ((1.0, "1"), (0.5, "half")):
    for _m in (7, 8):
        _DBSCAN[f"exact_eps_{_tag}_mp{_m}"] = functools.partial(_exact_eps, f"exact_eps_{_tag}_mp{_m}", _e, _m)
    _DBSCAN[f"binade_abi_{_tag}"] = functools.partial(_binade_abi, f"binade_abi_{_tag}", _e, int(64 / _e))
for _m in (1, 2, 600):
    _DBSCAN[f"count_stop_mp{_m}"] = functools.partial(_count_stop, f"count_stop_mp{_m}", _m)
for _n in (256, 257, 1025):
    _DBSCAN[f"rank_edges_{_n}"] = functools.partial(_rank_edges, f"rank_edges_{_n}", _n)
DBSCAN_NAMES = tuple(_DBSCAN)


@functools.lru_cache(maxsize=None)
def dbscan_case(name):
    return _DBSCAN[name]()


@functools.lru_cache(maxsize=None)
def dbscan_want(name, variant=None):
    """dbscan_ref_padded of the named case (variant None), or its wrong variants 'strict' and 'cells3x3' (over the case's own grid)
    -> labels [B,N] int64, n_clusters [B] int64, report"""
    c = dbscan_case(name)
    kw = dict(eps=c.eps, min_points=c.min_points, min_cluster_size=c.min_cluster_size)
    if variant == "strict":
        kw["strict"] = True
    elif variant == "cells3x3":
        assert c.points.shape[0] == 1
        cx, cy = nc.cells(c.points[0], c)
        kw["allowed"] = (np.abs(cx[:, None] - cx[None, :]) <= 1) & (np.abs(cy[:, None] - cy[None, :]) <= 1)
    elif variant is not None:
        raise ValueError(variant)
    return dbscan_ref.dbscan_ref_padded(torch.from_numpy(c.points.copy()), c.count, **kw)


def dbscan_conditions(name) -> dict:
    """no pair inside eps2 (1 +- 1e-5) except AT eps2 (only where the case says so) and the binade pairs of binade_abi -- a binade pair
    is within 4e-6 of eps2 by its nature, but at least 1e-6 below it, and its d2 is ONE fp32 rounding of the exact square (one non-zero
    difference, exact in fp32), so fp32 cannot move it across eps2; no border row nearly equidistant from two clusters"""
    c = dbscan_case(name)
    _, _, rep = dbscan_want(name)
    exact = sum(s["exact_pairs"] for s in rep["samples"])
    binade = 0
    for i, j, axis in getattr(c, "links", []) + getattr(c, "borders", []):
        a, b = c.points[0][i], c.points[0][j]
        assert all(a[k] == b[k] for k in range(3) if k != axis) and float(F(b[axis] - a[axis])) == float(b[axis]) - float(a[axis])
        d2 = (float(b[axis]) - float(a[axis])) ** 2
        assert c.eps ** 2 * (1 - 1e-5) < d2 <= c.eps ** 2 * (1 - 1e-6), (name, i, j, d2)
        binade += 1
    assert rep["band_pairs"] == exact + binade and rep["border_ties"] == 0, (name, rep["band_pairs"], exact, binade, rep["border_ties"])
    assert (exact > 0) == c.exact_pairs, (name, exact)
    return dict(exact_pairs=exact, core=sum(int(s["core"].sum()) for s in rep["samples"]),
                border=sum(int(s["border"].sum()) for s in rep["samples"]))


def two_cells_apart(lo, edge, cell, G, reach, steps=48):
    """fp32 coordinate pairs (a, b), b - a <= reach, that the fp32 cell rule files two cells apart around the cell coordinate ``edge``:
    a within ``steps`` fp32 values below lo + edge cell, b within ``steps`` values below a + reach"""
    a = F(F(lo) + F(edge * cell))
    found = []
    for _ in range(steps):
        a = np.nextafter(a, F(-np.inf))
        b = np.nextafter(F(float(a) + reach), F(np.inf))
        for _ in range(steps):
            b = np.nextafter(b, F(-np.inf))
            if float(b) - float(a) <= reach and nc.cell_f32(b, lo, cell, G) - nc.cell_f32(a, lo, cell, G) >= 2:
                found.append((a, b))
    return found
