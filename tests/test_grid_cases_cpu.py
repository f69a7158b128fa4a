"""CPU: the cases of tests/helpers/grid_cases.py that pin the row grid's two searches (tests/test_gpu_grid_cases.py) -- the ring walk
nn_ring_search behind df_chamfer_nn / df_reg_accumulate* and the fixed-radius window of the DBSCAN stages -- checked on the references alone:
every case meets its own input conditions, ``ring_walk`` (the numpy restatement of nn_ring_search) with the kernel's rule names the float64
all-pairs neighbour on every participating query of every case, and every case BITES: a deliberately wrong variant disagrees with the
reference on the case built for it.

Which case catches which variant (rows that differ, of the participating queries):
  slack0          beyond_square, beyond_square_33: the decoy instead of the partner on exactly the eight binade queries of each
  stop_on_equal   ring_ties, groups 4 and 5 -- with the slack at 0: on a dyadic lattice the filing is exact and the walk without slack is
                  right (asserted), so what differs is ``>=`` alone.  WITH the 2e-3 slack ``>=`` cannot change a result: a row at a
                  distance equal to the slacked bound would have to lie nearer than the true distance to the unscanned cells
  ring_cap1       z_column (all 24), single_ref, one_cell, sparse, beyond_square*
  first_seen      ring_ties, six of seven groups
  z_bound         z_column (all 24)
  DBSCAN strict   exact_eps_*_mp7 (no core row at all)        cells3x3   binade_abi_* and no other case"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import grid_cases as gc  # noqa: E402
import normals_cases as nc  # noqa: E402

F = np.float32


# ---- the ring walk ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.SEARCH_NAMES)
def test_search_case_meets_its_conditions_and_the_walk_is_right(name):
    c, ref = gc.search_case(name), gc.search_ref(name)
    found = gc.search_conditions(name)
    idx, rings, margin = gc.walk(name)
    part = ref["part"]
    print(name, "G", c.G, "queries", int(part.sum()), found, "rings up to", int(rings.max()), "far", int((rings >= 2).sum()), "margin", margin)
    assert c.query.shape[0] <= 3 and c.query.shape[1] <= 1500 and c.refs.shape[1] <= 1500
    assert found["narrow"] == len(c.narrow) and (found["exact"] > 0) == (name == "ring_ties")
    assert np.array_equal(idx[part], ref["idx"][part]), np.argwhere(part & (idx != ref["idx"]))[:10]
    # no break decision on best is within 1e-6 = 16 fp32 ulp of flipping (exact lattices apart): fused multiply-adds move the kernel's
    # d2 by 2 ulp at the most, so they cannot change a ring count
    assert c.dyadic or margin >= 1e-6


@pytest.mark.parametrize("name,lo,edge", [("beyond_square", -51.2, 64), ("beyond_square_33", -30.2, 32)])
def test_beyond_square(name, lo, edge):
    c, ref = gc.search_case(name), gc.search_ref(name)
    assert c.G == 103 and c.cell == 1.0 and c.xy_range[0] == lo and len(c.pairs) == 8 and {ax for *_, ax in c.pairs} == {0, 1}
    f = gc.Filed(c.refs[0], gc.refs_ok(c, 0), c.grid)
    cx, cy = nc.cell_f32(c.refs[0][:, 0], lo, 1.0, 103), nc.cell_f32(c.refs[0][:, 1], lo, 1.0, 103)
    for i, p, d, axis in c.pairs:
        q = c.query[0, i]
        qc = (nc.cell_f32(q[0], lo, 1.0, 103), nc.cell_f32(q[1], lo, 1.0, 103))
        assert qc[axis] == edge - 1 and (cx, cy)[axis][p] == edge + 1 and (cx[d], cy[d]) == qc            # partner two cells on, decoy at home
        near = np.flatnonzero((np.abs(cx - qc[0]) <= 1) & (np.abs(cy - qc[1]) <= 1))
        assert near.tolist() == [d]                                                                        # alone in the 3 x 3 cells
        dp, dd = F((c.refs[0][p][axis] - q[axis]) ** 2), F((c.refs[0][d][2] - q[2]) ** 2)
        px, _ = gc._pos(q[axis], lo, 1.0, 103)
        lb2 = F(F(F(edge + 1) - px) ** 2)
        assert float(dd) - float(dp) >= 8 * float(np.spacing(dp)) and dd < lb2 and dp <= 1 - 1e-6, (dp, dd, lb2)
        assert ref["idx"][0, i] == p
        assert gc.ring_walk(q, f, c.grid) == (p, 2)
        assert gc.ring_walk(q, f, c.grid, slack=0.0) == (d, 1)
    wrong = gc.walk(name, "slack0")[0]
    assert np.flatnonzero(wrong[0] != ref["idx"][0]).tolist() == sorted(i for i, *_ in c.pairs)          # on exactly these rows


def test_ring_ties():
    c, ref = gc.search_case("ring_ties"), gc.search_ref("ring_ties")
    assert np.array_equal(c.refs.astype(np.float64) * 4, np.round(c.refs.astype(np.float64) * 4)) and c.xy_range[0] == -32.0 and c.cell == 1.0
    f = gc.Filed(c.refs[0], gc.refs_ok(c, 0), c.grid)
    lowest_ring = []
    for g in range(c.groups):
        q = c.query[0, g]
        d2 = ((c.refs[0].astype(np.float64) - q) ** 2).sum(axis=1)
        tied = np.flatnonzero(d2 == d2.min())
        ring = np.maximum(np.abs(f.cx - gc._pos(q[0], -32.0, 1.0, 64)[1]), np.abs(f.cy - gc._pos(q[1], -32.0, 1.0, 64)[1]))
        assert ref["idx"][0, g] == tied[0] == c.first_ref[g] and float(F(d2.min())) == d2.min()
        lowest_ring.append((len(tied), int(ring[tied[0]]), int(ring[tied].min())))
    print(lowest_ring)
    assert lowest_ring[0] == (4, 2, 0) and lowest_ring[1] == (3, 1, 0)            # the lowest row in the outermost ring of the tied ones
    assert lowest_ring[2] == (2, 1, 0) and lowest_ring[3] == (4, 1, 0)            # on a cell edge, on a cell corner
    assert c.query[0, 2, 0] == np.round(c.query[0, 2, 0]) and np.array_equal(c.query[0, 3, :2], np.round(c.query[0, 3, :2]))
    for g in c.bound_equal:                                                        # the unslacked bound of ring 0 equals best, bit for bit
        t = {}
        assert gc.ring_walk(c.query[0, g], f, c.grid, slack=0.0, ring_cap=0, trace=t)[1] == 0 and t["best"] == F(0.0625)
    exact, _, _ = gc.walk("ring_ties", "slack0")
    assert np.array_equal(exact, ref["idx"])                                       # exact filing: the walk without slack is right here
    assert np.flatnonzero(gc.walk("ring_ties", "stop_on_equal")[0][0] != ref["idx"][0]).tolist() == list(c.bound_equal)
    assert np.flatnonzero(gc.walk("ring_ties", "first_seen")[0][0] != ref["idx"][0]).tolist() == [0, 1, 2, 3, 4, 5]


def test_z_column_and_the_gates():
    c, ref = gc.search_case("z_column"), gc.search_ref("z_column")
    rings = gc.walk("z_column")[1]
    d = np.sqrt(ref["d2"][0])
    assert d.min() > 4.2 and d.max() < 5.8 and rings.min() >= 4 and rings.max() <= 7
    for v in ("z_bound", "ring_cap1"):
        wrong, wr, _ = gc.walk("z_column", v)
        assert np.all(wrong[0] != ref["idx"][0]) and wr.max() <= 2 < rings.min()    # stops early at a row of the column, on every query
    for name, kept in (("exact_gate", (0.0, 0.0625, 0.125)), ("exact_gate_below", (0.0, 0.0625)), ("exact_gate_zero", (0.0,))):
        c, ref = gc.search_case(name), gc.search_ref(name)
        hit = ref["idx"][0] >= 0
        assert np.array_equal(hit, np.isin(c.nearest_d2, kept)) and np.array_equal(ref["d2"][0][hit], c.nearest_d2[hit])
        assert {float(v) for v in c.nearest_d2} == {0.0, 0.0625, 0.125, 0.1875}
        rings = gc.walk(name)[1]
        assert rings.max() == 1 and (rings == 1).sum() >= 10                       # kept rows in ring 1 too
    assert gc.search_case("exact_gate").max_dist2 == 0.125 and F(gc.search_case("exact_gate_below").max_dist2) == np.nextafter(F(0.125), F(0))
    assert (gc.search_ref("exact_gate_zero")["idx"] >= 0).sum() == 13 and gc.search_case("exact_gate_zero").max_dist2 == 0.0


def test_extremes():
    assert gc.search_case("g1").G == 1 and gc.search_case("g4096").G == 4096 and gc.search_case("outside").G == 8
    # g4096: cell coordinates 0 .. 2 and 4090 .. 4096 only; nearest pairs that straddle a cell edge
    c, ref = gc.search_case("g4096"), gc.search_ref("g4096")
    lo, cell = c.xy_range[0], c.cell
    cq = np.stack([nc.cell_f32(c.query[0][:, k], lo, cell, 4096) for k in (0, 1)], axis=1)
    cr = np.stack([nc.cell_f32(c.refs[0][:, k], lo, cell, 4096) for k in (0, 1)], axis=1)
    for cc in (cq, cr):
        assert np.all((cc <= 2) | (cc >= 4090)) and (cc <= 2).any() and (cc == 4095).any()
    hit = ref["idx"][0] >= 0
    straddle = (cq[hit] != cr[ref["idx"][0][hit]]).any(axis=1)
    print("g4096: neighbours", int(hit.sum()), "of", len(hit), "in another cell", int(straddle.sum()))
    assert hit.sum() >= 250 and straddle.sum() >= 50
    # outside: all four sides and the corners, 1e4 m out, for queries and refs; a border cell of 600 refs
    c = gc.search_case("outside")
    for pts in (c.query[0], c.refs[0]):
        x, y = pts[:, 0], pts[:, 1]
        with np.errstate(invalid="ignore"):
            for side in (x < -4, x >= 4, y < -4, y >= 4, (x < -4) & (y >= 4), (x >= 4) & (y < -4), (x >= 4) & (y >= 4), (x < -4) & (y < -4)):
                assert side.sum() >= 3
            assert (np.maximum(np.abs(x), np.abs(y)) > 5e3).sum() >= 3
    f = gc.Filed(c.refs[0], gc.refs_ok(c, 0), c.grid)
    assert np.bincount(f.cy * 8 + f.cx, minlength=64).max() >= c.crowd and np.bincount(f.cy * 8 + f.cx, minlength=64).argmax() == 7 * 8 + 0
    # a single participating ref; all refs in one cell; a sparse set with long walks, and the gate that cuts them short
    c = gc.search_case("single_ref")
    assert gc.refs_ok(c, 0).sum() == 1 and np.all(gc.search_ref("single_ref")["idx"][0] == 23)
    c = gc.search_case("one_cell")
    f = gc.Filed(c.refs[0], gc.refs_ok(c, 0), c.grid)
    assert len(set(zip(f.cx.tolist(), f.cy.tolist()))) == 1 and len(f.rows) == 500
    rings = gc.walk("sparse")[1]
    assert (rings >= 20).sum() >= 50 and rings.max() >= 40
    rings, ref = gc.walk("sparse_gated")[1], gc.search_ref("sparse_gated")
    assert rings.max() == 2 and (rings == 2).sum() >= 50 and (rings == 1).sum() >= 10
    assert 20 <= (ref["idx"][0] >= 0).sum() <= 100 and (ref["idx"][0] < 0).sum() >= 100


@pytest.mark.parametrize("variant,names", [("slack0", ("beyond_square", "beyond_square_33")), ("stop_on_equal", ("ring_ties",)),
                                           ("ring_cap1", ("z_column", "single_ref", "one_cell", "sparse")), ("first_seen", ("ring_ties",)),
                                           ("z_bound", ("z_column",))])
def test_wrong_walk_is_caught_by_its_case(variant, names):
    for name in names:
        ref = gc.search_ref(name)
        wrong = gc.walk(name, variant)[0]
        n = int((ref["part"] & (wrong != ref["idx"])).sum())
        print(variant, "on", name, ":", n, "of", int(ref["part"].sum()), "queries differ")
        assert n >= 1


# ---- DBSCAN -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.DBSCAN_NAMES)
def test_dbscan_case_meets_its_conditions(name):
    c = gc.dbscan_case(name)
    found = gc.dbscan_conditions(name)
    lab, k, _ = gc.dbscan_want(name)
    print(name, c.points.shape, "G", c.G, found, "clusters", k.tolist())
    assert c.points.shape[0] <= 3 and c.points.shape[1] <= 1500
    same = gc.dbscan_want(name, "cells3x3")
    if name.startswith("binade_abi"):
        assert not np.array_equal(same[0].numpy(), lab.numpy())
    else:                                                                          # the 3 x 3 window is right everywhere else
        assert np.array_equal(same[0].numpy(), lab.numpy()) and np.array_equal(same[1].numpy(), k.numpy())


@pytest.mark.parametrize("tag,eps", [("1", 1.0), ("half", 0.5)])
def test_exact_eps(tag, eps):
    c = gc.dbscan_case(f"exact_eps_{tag}_mp7")
    assert c.eps == eps and np.array_equal(c.points.astype(np.float64) / eps * 4, np.round(c.points.astype(np.float64) / eps * 4))
    lab, k, rep = gc.dbscan_want(c.name)
    s = rep["samples"][0]
    near = (((c.points[0][:, None, :].astype(np.float64) - c.points[0][None]) ** 2).sum(axis=2) <= eps * eps).sum(axis=1)
    assert np.all(near[c.interior] == 7) and near[~c.interior].max() == 6
    assert np.array_equal(s["core"].numpy(), c.interior) and int(s["border"].sum()) == 6 * 81 and k.tolist() == [1]
    assert np.all(lab[0].numpy()[c.interior | s["border"].numpy()] == 1) and int((lab == 0).sum()) == 1331 - 729 - 486
    lab8, k8, _ = gc.dbscan_want(f"exact_eps_{tag}_mp8")
    assert k8.tolist() == [0] and not lab8.any()
    strict, ks, _ = gc.dbscan_want(c.name, "strict")
    assert ks.tolist() == [0] and not strict.any()                                 # d2 < eps2: every row is alone


@pytest.mark.parametrize("min_points", [1, 2, 600])
def test_count_stop(min_points):
    c = gc.dbscan_case(f"count_stop_mp{min_points}")
    cx, cy = nc.cells(c.points[0], c)
    assert len(set(zip(cx[c.crowd].tolist(), cy[c.crowd].tolist()))) == 1 and len(c.crowd) == 640
    assert ((cx == cx[c.crowd[0]]) & (cy == cy[c.crowd[0]])).sum() == 640
    p = c.points[0].astype(np.float64)
    near = (((p[:, None, :] - p[None]) ** 2).sum(axis=2) <= c.eps ** 2).sum(axis=1)
    assert near[c.probes].tolist() == [599, 600, 601] and np.all(near[c.A] == 600)
    lab, k, rep = gc.dbscan_want(c.name)
    core = rep["samples"][0]["core"].numpy()
    if min_points == 600:
        assert core[c.probes].tolist() == [False, True, True] and np.all(core[c.A]) and core.sum() == 599
        lab = lab[0].numpy()
        assert np.all(lab[c.deps[0]] == 0) and np.all(lab[c.deps[1]] == 1) and np.all(lab[c.deps[2]] == 1) and np.all(lab[c.probes] == 1)


@pytest.mark.parametrize("tag,eps,edge", [("1", 1.0, 64), ("half", 0.5, 128)])
def test_binade_abi(tag, eps, edge):
    c = gc.dbscan_case(f"binade_abi_{tag}")
    assert c.cell == c.eps == eps and c.xy_range == gc.DEFAULT_RANGE and c.edge == edge
    cxy = nc.cells(c.points[0], c)
    for i, j, axis in c.links + c.borders:                                         # the pairs exist at cell == eps
        assert cxy[axis][i] == edge - 1 and cxy[axis][j] == edge + 1
    assert len(c.links) == 4 and len(c.borders) == 2 and {ax for *_, ax in c.links} == {0, 1} == {ax for *_, ax in c.borders}
    lab, k, rep = gc.dbscan_want(c.name)
    lab, s = lab[0].numpy(), rep["samples"][0]
    assert k.tolist() == [6]
    for i, j, _ in c.links:
        assert s["core"][i] and s["core"][j] and lab[i] == lab[j] > 0
    for i, j, _ in c.borders:
        assert s["border"][i] and s["core"][j] and lab[i] == lab[j] > 0
    wrong, kw, _ = gc.dbscan_want(c.name, "cells3x3")
    wrong = wrong[0].numpy()
    assert kw.tolist() == [10]                                                     # two clusters for each linked pair of groups
    for i, j, _ in c.links:
        assert wrong[i] != wrong[j] and wrong[i] > 0 and wrong[j] > 0
    for i, j, _ in c.borders:
        assert wrong[i] == 0 and wrong[j] > 0


def test_the_slacked_cell_files_no_pair_within_eps_two_cells_apart():
    """what keeps cluster.dbscan right whatever the window: at cell = CELL_SLACK eps the fp32 cell rule files no two coordinates that are
    at most 1.002 eps apart two cells apart, at any power-of-two edge below G.  (Pairs within 1e-6 of ONE CELL = 1.0025 eps apart are
    filed two cells apart there as at any cell size -- normals_cases.binade_pairs finds them at the edge 64 -- but they are 0.25 %
    beyond eps.)  At cell == eps the pairs within eps exist: the probes find binade_abi's."""
    from deflow_amd.cluster import CELL_SLACK
    assert CELL_SLACK == gc.CELL_SLACK
    lo = gc.DEFAULT_RANGE[0]
    for eps in (0.025, 0.5, 0.7, 1.0):
        cell = CELL_SLACK * eps
        G = gc.grid_of(gc.DEFAULT_RANGE, cell).G
        edges = [2 ** k for k in range(0, 12) if 2 ** k < G]
        assert len(edges) >= 7
        for edge in edges:
            assert not gc.two_cells_apart(lo, edge, cell, G, eps * 1.002), (eps, edge)
    assert gc.two_cells_apart(lo, 64, 1.0, 103, 1.0) and gc.two_cells_apart(lo, 128, 0.5, 205, 0.5)
    assert nc.binade_pairs(lo, 64, 1.0, 103) and nc.binade_pairs(lo, 128, 0.5, 205)


@pytest.mark.parametrize("N", [256, 257, 1025])
def test_rank_edges(N):
    c = gc.dbscan_case(f"rank_edges_{N}")
    lab, k, rep = gc.dbscan_want(c.name)
    lab, s = lab[0].numpy(), rep["samples"][0]
    root = s["root"].numpy()
    assert c.points.shape[1] == N and k.tolist() == [4]
    r = c.roots
    assert [lab[r[key]] for key in ("first", "mid", "drop", "late", "star")] == [1, 2, 0, 3, 4]
    assert root[r["drop"]] == r["drop"] and (root == r["drop"]).sum() == 3 and r["mid"] < r["drop"] < r["late"]
    assert r["star"] == N - 1 and root[N - 1] == N - 1 and (root == N - 1).sum() == 7 and s["core"].numpy()[root == N - 1].sum() == 1
    assert (root == r["first"]).sum() == 6 and lab[N - 2] == 1
    if N == 1025:                                                                  # roots in the first, a middle and the last block of 256
        assert [r[key] // 256 for key in ("first", "mid", "late", "star")] == [0, 2, 3, 4]
