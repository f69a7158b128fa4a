"""CPU: the cases of tests/helpers/normals_cases.py that pin df_normals (tests/test_gpu_normals_cases.py), checked on the float64
reference alone -- every case meets its own input conditions, and every case BITES: a deliberately wrong variant of the reference
disagrees with the reference on the case that was built for it, in m, in validity or in n.

The 'cells3x3' variant -- neighbours only from the 3 x 3 cells of the fp32 cell rule around a row's own -- is what df_normals did before
it scanned the cells that the clamped position +- (radius / cell + 2e-3) covers: ``binade`` records that defect here, without a GPU.

Also here: how far the reference with the differences formed as fp32(v - p) (the header's definition) lies from the reference with exact
differences, in the units of the GPU test's bounds.  Measured: angle at most 0.0135 of the 16 EPS trace / gap bound, eigen-residual
0.0198 of 16 EPS trace, |curv - ref| 1.8e-8 -- the rounding of the differences takes a fiftieth of the bounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import normals_cases as nc  # noqa: E402
import reg_ref  # noqa: E402


@pytest.mark.parametrize("name", nc.NAMES)
def test_case_meets_its_conditions(name):
    case = nc.case(name)
    found = nc.check_conditions(case)
    print(name, "G", case.G, "rows", case.points.shape, "margins", found)
    assert case.points.dtype == np.float32 and case.points.shape[1] <= 1500 and case.points.shape[0] <= 3
    assert case.radius <= case.cell
    assert (found["exact_pairs"] > 0) == case.exact_pairs


@pytest.mark.parametrize("name", ["generic", "spread"])
def test_most_valid_rows_have_a_gap(name):
    case = nc.case(name)
    assert case.G == 103 and (case.cell, case.radius, case.min_pts, case.max_curvs) == (1.0, 1.0, 5, (0.05, nc.THIRD))
    for max_curv in case.max_curvs:
        out = nc.ref(name, 0, max_curv)
        lam = out["lam"][out["valid"]]
        share = float(((lam[:, 1] - lam[:, 0]) >= 0.01 * lam.sum(axis=1)).mean())
        print(name, "max_curv", max_curv, "valid", int(out["valid"].sum()), "of", len(out["valid"]), "share with gap >= 0.01 trace", share)
        assert share >= 0.8
    c = nc.ref(name, 0, 0.05)["curv_all"]
    c = c[np.isfinite(c)]
    decades = np.histogram(c, bins=[1e-4, 1e-3, 1e-2, 0.1, 0.34])[0]
    print(name, "curvature", c.min(), "..", c.max(), "per decade from 1e-4", decades.tolist())
    if name == "generic":
        assert 1100 <= case.points.shape[1] <= 1300
        assert np.all(decades >= 20) and c.max() >= 0.25                                                     # spread over 1e-4 .. 0.3
        v = nc.ref(name, 0, 0.05)["valid"]
        assert v.sum() >= 300 and (~v).sum() >= 100                                                          # both occur at 0.05
    else:
        r01, r12 = case.ratios
        assert r01.min() == 1e-10 and abs(r01.max() - 0.9) < 1e-12 and r12.min() == 1e-3 and r12.max() == 1.0
        assert np.all(nc.ref(name, 0, 0.05)["m"] == 30)                                                      # isolated blobs of 30 rows


@pytest.mark.parametrize("name,edge", [("binade", 64), ("binade_33", 32)])
def test_binade_pairs_are_filed_two_cells_apart(name, edge):
    case = nc.case(name)
    assert case.G == 103 and case.radius == case.cell == 1.0
    assert name != "binade" or case.xy_range == nc.DEFAULT_GRID["xy_range"]
    n = nc.binade_condition(case)
    edges = sorted({(axis, e) for _, _, axis, e in case.pairs})
    print(name, ": pairs two cells apart with d2 <= r2 (1 - 1e-6):", n, "of", len(case.pairs), "at", edges)
    assert n >= 6 and n == len(case.pairs)
    assert edges == [(0, edge), (1, edge)]
    assert nc.ref(name, 0, nc.THIRD)["m"].min() >= case.min_pts                       # the filler rows: nothing hides behind min_pts


def test_which_binade_edges_have_such_pairs():
    """on the default grid only the edge 64; the edge 32 on a grid that brings it near the origin; below 32 none on any grid tried"""
    have = {(lo, e): len(nc.binade_pairs(lo, e)) for lo in (-51.2, -30.2, -17.7) for e in (64, 32, 16)}
    print(have)
    assert have[(-51.2, 64)] == 1 and have[(-51.2, 32)] == 0 and have[(-51.2, 16)] == 0
    assert have[(-30.2, 32)] >= 3 and have[(-17.7, 16)] == 0


def test_exact_radius_rows_are_exact():
    for name, r in (("exact_radius", 1.0), ("exact_radius_half", 0.5)):
        case = nc.case(name)
        out = nc.ref(name, 0, nc.THIRD)
        inner = case.interior
        assert inner.sum() == 729 and np.all(out["m"][inner] == 7)                    # itself and the six neighbours at d2 == r2
        assert np.all(out["valid"][inner]) and np.all(out["curv"][inner].astype(np.float32) == np.float32(nc.THIRD))
        z = case.points[0][inner][:, 2]
        want = np.stack((np.zeros_like(z), np.zeros_like(z), np.where(z > 0, -1.0, 1.0)), axis=1)
        assert out["n"][inner].tobytes() == want.astype(np.float64).tobytes()         # (+0 components)
        assert (z == 0).sum() == 81 and np.any(np.all(case.points[0] == 0, axis=1)) == (name == "exact_radius")


def test_border_and_degenerate_hold_what_they_promise():
    case = nc.case("border")
    assert case.G == 8 and case.counts[2] == 0 and case.counts[1] < case.points.shape[1] and case.mask is not None
    cx, cy = nc.cells(case.points[0], case)
    ok = reg_ref.participating(case.points[0], case.counts[0], case.mask[0])
    x, y = case.points[0][:, 0], case.points[0][:, 1]
    with np.errstate(invalid="ignore"):
        for side in (x < -4, x >= 4, y < -4, y >= 4, (x < -4) & (y >= 4), (x >= 4) & (y < -4)):
            assert (side & ok).sum() >= 12
        far = np.maximum(np.abs(x), np.abs(y))
        assert (ok & (far > 4) & (far < 4.4)).any() and (ok & (far > 5e3)).any()
    crowd = np.bincount((cy * 8 + cx)[ok], minlength=64)
    assert crowd.max() >= 600 and crowd.argmax() in (0 * 8 + 0, 7, 56, 63, 7 * 8 + 0)  # a border cell
    assert (~np.isfinite(case.points[0]).all(axis=1)).sum() == 10
    out = nc.ref("border", 0, 0.05)
    with np.errstate(invalid="ignore"):
        assert (out["valid"] & (far > 4)).sum() >= 50                                  # rows outside the range have normals of their own
    deg = nc.case("degenerate")
    out = nc.ref("degenerate", 0, 0.05)
    w = deg.where
    a, b = w["collinear"]
    assert np.all(out["valid"][a:b]) and np.abs(out["curv"][a:b]).max() <= 1e-12 and np.abs(out["lam"][a:b, :2]).max() <= 1e-15
    a, b = w["copies"]
    assert np.all(out["m"][a:b] == 40) and not out["valid"][a:b].any() and np.all(out["lam"][a:b] == 0)
    assert np.all(out["m"][slice(*w["four"])] == deg.min_pts - 1) and np.all(out["m"][slice(*w["five"])] == deg.min_pts)
    a, b = w["flat"]
    assert np.all(out["valid"][a:b]) and out["n"][a:b].tobytes() == np.tile((0.0, 0.0, 1.0), (b - a, 1)).tobytes()
    a, b = w["origin"]
    assert np.all(deg.points[0][a] == 0) and out["valid"][a] and out["n"][a][0] > 0
    a, b = w["tiny"]
    assert np.all(out["m"][a:b] == 12) and np.abs(deg.points[0][a:b, :2]).min() > 49


@pytest.mark.parametrize("variant,name,max_curv", [("cells3x3", "binade", nc.THIRD), ("cells3x3", "binade_33", nc.THIRD),
                                                   ("strict", "exact_radius", nc.THIRD), ("drop_outside", "border", 0.05),
                                                   ("earlier_axis", "exact_radius", nc.THIRD), ("no_tie_break", "degenerate", 0.05)])
def test_wrong_variant_is_caught_by_its_case(variant, name, max_curv):
    case = nc.case(name)
    right, wrong = nc.ref(name, 0, max_curv), nc.reference(case, 0, max_curv, variant)
    dm, dv = int((right["m"] != wrong["m"]).sum()), int((right["valid"] != wrong["valid"]).sum())
    dn = int((np.abs(right["n"] - wrong["n"]).max(axis=1) > 1e-6).sum())
    print(variant, "on", name, ": rows that differ in m", dm, "in validity", dv, "in n", dn)
    assert nc.differs(right, wrong)
    if variant == "cells3x3":                                                         # every pair's two rows lose exactly one neighbour
        rows = sorted(i for p in case.pairs for i in p[:2])
        assert np.flatnonzero(right["m"] != wrong["m"]).tolist() == rows and np.all(right["m"][rows] - wrong["m"][rows] == 1)
    if variant == "strict":
        assert np.all(wrong["m"][case.interior] == 1)
    if variant == "earlier_axis":
        assert dm == 0 and dv == 0 and dn == int(case.interior.sum())
    if variant == "no_tie_break":
        assert dm == 0 and dv == 0 and dn >= 225
    # ... and by no case that was not built for it: the other cases' references do not move under a variant that is not theirs
    if variant == "cells3x3":
        for other in ("generic", "spread", "degenerate"):
            assert not nc.differs(nc.ref(other, 0, 0.05), nc.reference(nc.case(other), 0, 0.05, variant)), other


@pytest.mark.parametrize("name", nc.NAMES)
def test_fp32_differences_sit_well_inside_the_bounds(name):
    """the reference with fp32 differences held against the exact-differences one by the GPU test's own rules"""
    case = nc.case(name)
    for b in range(len(case.counts)):
        for max_curv in case.max_curvs:
            r32 = nc.ref(name, b, max_curv, None, True)
            w = nc.compare(case, b, max_curv, r32["n"], r32["curv"], r32["m"])
            assert w["angle_ratio"] <= 0.25 and w["residual_ratio"] <= 0.25 and w["curv"] <= 4 * nc.EPS
