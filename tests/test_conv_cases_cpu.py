"""CPU: the conditions that make tests/test_gpu_conv_cases.py meaningful, decided without a GPU (the library's host-side queries launch
nothing).

  * tile selection: df_conv2d_variant / df_conv2d_tile_m give every problem of tests/helpers/conv_cases.py the tile its case was built for,
    with the stated tile count and last-tile size; the class-mode condition of conv_plan(), restated, holds for `s2_class` only;
  * form queries: df_conv2d_x3_ok / df_conv2d_w16_ok say 1 for the halo_* cases and 0 for tail*; the weight-gradient _ok functions answer as
    the forms table says; the *_splits functions return the recorded counts;
  * the forward / data-gradient host layer: every launch entry point's refusal code for one fault in a complete call; the _ok queries
    against the case tables; df_conv2d_plan (family, tile, flags, statistics rows) pinned on the case tables and the benchmark's layer
    shapes, an _ok query saying 1 exactly where the plan is no refusal; the profiler labels ops._conv_label formats from the plan;
  * chunks and splits: the restated wg_chunk / chunks_per_split / c_begin / c_end show which split starts mid-row, which crosses an image,
    which has fewer chunks than the ring is deep and which is empty;
  * the restatements (rows -> tiles; chunks -> splits -> reduce) equal ref64 with no fault, and every fault injected into them (never into
    a kernel) lands at least ten times over the bound the GPU test applies, in the case built for it;
  * the float32 evaluation of every reference meets every bound of the GPU test: a correct fp32 computation can pass.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import conv_cases as CC  # noqa: E402
import ref64 as R  # noqa: E402

ALL = [p for ps in CC.PROBS.values() for p in ps]
WALL = [p for ps in CC.WPROBS.values() for p in ps]


def _by(case, **kw):
    out = [p for p in CC.PROBS[case] if all(getattr(p, k) == v for k, v in kw.items())]
    assert out, (case, kw)
    return out


def _close(a, b, tag):
    e = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert e <= 1e-12, (tag, e)


def _desc(shape, lay, elt=0):
    """a descriptor of that geometry on an aligned address nobody dereferences"""
    from deflow_amd._lib import DfImg
    probe = torch.empty(64, dtype=torch.float32)
    base = (probe.data_ptr() + 127) // 128 * 128
    n, h, w, c = shape
    return DfImg(base + 4 * (lay.lead + lay.off), n, h, w, c, lay.ld, lay.grp_size, lay.img_stride, lay.grp_off, elt, 0)


def _descs(p):
    return (_desc(p.in_shape, CC.layout(p.in_shape, p.grp, p.views, "x")), _desc(p.out_shape, CC.layout(p.out_shape, p.grp, p.views, "y")))


def _wdescs(p):
    xs, ds = (p.n, p.h, p.w, p.cin), (p.n, p.ho, p.wo, p.cout)
    return _desc(xs, CC.layout(xs, p.grp, p.views, "x")), _desc(ds, CC.layout(ds, p.grp, p.views, "y"))


# ---- tile selection -------------------------------------------------------------------------------------------------------------
# per case, per problem in table order: (variant, class mode, row tiles, rows of the last tile)
TILES = {
    "tail64": [(64064, False, 3, 7)] * 8,
    "tail128": [(128064, False, 34, 1)] * 4 + [(128128, False, 34, 1)] * 2 + [(128064, False, 34, 1)] * 2,     # (64->128 data gradient writes 64 channels)
    "n32": [(128032, False, 2, 26)] * 6,
    "s2_odd": [(64064, False, 2, 6)] * 2 + [(128032, False, 2, 106)] * 2,           # forward 70 rows; dx [2,9,13,32]: 234 rows of 32 channels
    "s2_even_ragged": [(64064, False, 1, 35)] + [(128032, False, 2, 12)] * 2,       # dx [1,10,14,32]: 140 rows
    "s2_class": [(64064, True, 8, 64)] * 2 + [(64064, True, 4, 64)] * 2,
    "thin": [(64064, False, 1, 1)] * 2 + [(64064, False, 2, 16)] * 4,
    "halo_thin": [(128064, False, 2, 128)] * 2 + [(128064, False, 6, 128)] + [(128128, False, 2, 128)] * 2 + [(128128, False, 6, 128)],
    "halo_odd": [(128064, False, 33, 128)] * 3 + [(128128, False, 33, 128)] * 3,
    "views": [(64064, False, 3, 52)] * 4 + [(64064, False, 3, 12)] * 2 + [(128032, False, 4, 84)] * 2,
}


@pytest.mark.parametrize("case", CC.NAMES)
def test_tile_selection(case):
    assert len(TILES[case]) == len(CC.PROBS[case])
    for p, (var, cls, ntiles, last) in zip(CC.PROBS[case], TILES[case]):
        tl = CC.tiling(p)
        m0, m1 = tl["tiles"][-1][1:]
        assert (tl["var"], tl["cls"], len(tl["tiles"]), min(m1, tl["m_end"]) - m0) == (var, cls, ntiles, last), (p.pid, tl["var"], tl["cls"], len(tl["tiles"]))
        assert tl["bm"] == var // 1000 and p.out_shape[3] % tl["bn"] == 0
        if p.epi == "stats":
            from deflow_amd._lib import call
            rpg = (p.grp or p.n) * p.ho * p.wo
            assert call("df_conv2d_tile_m", rpg, p.cout) == 128 and rpg % 128 == 0
    assert CC.CASES[case]["why"]


def test_class_mode_condition():
    for p in ALL:
        if p.mode != "dgrad" or p.stride != 2:
            assert not CC.class_mode_asked(p)
    for p in CC.PROBS["s2_class"]:
        assert CC.class_mode_asked(p) and CC.tiling(p)["cls"]
        assert len(CC.tiling(p)["tiles"]) // 4 == (2 if p.n == 2 else 1)            # tiles per parity class
    for p in _by("s2_odd", mode="dgrad") + _by("views", mode="dgrad", stride=2):
        assert not CC.class_mode_asked(p)                                           # odd dx
    for p in _by("s2_even_ragged", mode="dgrad"):
        tl = CC.tiling(p)
        assert CC.class_mode_asked(p) and not tl["cls"] and (p.M // 4) == 35 and 35 % tl["bm"] != 0


def test_cases_are_what_they_claim():
    assert CC.PROBS["tail64"][0].M == 135 == 2 * 64 + 7 and CC.PROBS["tail64"][0].h * CC.PROBS["tail64"][0].w == 45
    assert CC.PROBS["tail128"][0].M == 4225 > 4096 and 4225 == 33 * 128 + 1
    assert CC.PROBS["n32"][0].M == 154 == 128 + 26
    assert CC.PROBS["halo_odd"][0].M == 4224 == 33 * 128
    p = CC.PROBS["s2_odd"][0]
    assert (p.ho, p.wo) == (5, 7) and (p.ho - 1) * 2 == p.h - 1 and (p.wo - 1) * 2 == p.w - 1      # the last window starts on the last row / column
    p = CC.PROBS["s2_even_ragged"][0]
    assert (p.ho, p.wo) == (5, 7) and p.h % 2 == 0 and p.w % 2 == 0
    assert {(p.n, p.h, p.w) for p in CC.PROBS["thin"]} == {(1, 1, 1), (2, 1, 40), (2, 40, 1)}
    for p in CC.PROBS["halo_thin"]:
        assert p.epi == "stats" and ((p.grp == 1 and p.n == 2) or p.n == 1)
    assert CC.stats_layout(_by("halo_thin", cout=64, w=256)[0], "x3") == (256, 2) and CC.stats_layout(_by("halo_thin", cout=64, w=256)[0], "mp") == (128, 1)
    assert CC.stats_layout(_by("halo_thin", cout=128, w=256)[0], "h2") == (128, 1)
    for p in ALL:
        for v in CC.tensors(p).values():
            assert v is None or (v.dtype == torch.float32 and bool(torch.isfinite(v).all()))
        assert set(CC.forms(p.case)) <= set(CC.F_TAIL + CC.F_HALO)
    assert all("yh2" in CC.forms(c) and "ybf16" in CC.forms(c) for c in ("tail64", "tail128"))
    assert all("yh2" not in CC.forms(c) for c in CC.NAMES if not c.startswith("tail"))


def test_layouts():
    for p in ALL + WALL:
        shapes = (p.in_shape, p.out_shape) if isinstance(p, CC.Prob) else ((p.n, p.h, p.w, p.cin), (p.n, p.ho, p.wo, p.cout))
        for shape, side in zip(shapes, "xy"):
            lay = CC.layout(shape, p.grp, p.views, side)
            idx = CC.index(lay, shape)
            assert idx.unique().numel() == idx.numel() and int(idx.min()) == lay.lead + lay.off
            assert lay.lead >= CC.GUARD_ROWS * lay.ld and lay.total - int(idx.max()) - 1 >= CC.GUARD_ROWS * lay.ld - lay.ld
            assert all(v % 4 == 0 for v in (lay.ld, lay.off, lay.img_stride, lay.grp_off, lay.lead))
            if p.views:
                assert p.n == 4 and lay.grp_size == 2 and lay.grp_off != 2 * lay.img_stride and lay.off > 0 and lay.off + shape[3] < lay.ld
            if p.case.startswith("tail"):
                assert lay.ld % 32 == 0 and lay.img_stride % 32 == 0 and (4 * lay.lead) % 128 == 0      # what a pre-split output asks for


# ---- form queries ---------------------------------------------------------------------------------------------------------------
def test_forward_form_queries():
    from deflow_amd._lib import call
    for p in ALL:
        x, y = _descs(p)
        mode = CC.FWD if p.mode == "fwd" else CC.DGRAD
        ok = (call("df_conv2d_x3_ok", x, y, p.k, p.stride, mode, CC.EPI[p.epi]), call("df_conv2d_w16_ok", x, y, p.k, p.stride, mode, CC.EPI[p.epi]))
        if p.case.startswith("halo"):
            assert ok == (1, 1), (p.pid, ok)
        if p.case.startswith("tail"):
            assert ok == (0, 0), (p.pid, ok)
        assert ("x3" in CC.forms(p.case)) <= (ok == (1, 1)), p.pid
    assert CC.refused(_by("tail64", acc=True)[0], "yh2") == CC.E_ARG and CC.refused(_by("tail64", acc=False)[0], "yh2") is None


# ---- the forward / data-gradient host layer: refusals, queries, the plan, the profiler labels ------------------------------------------
E_OK = 0
W_F32, W_B16, W_X3, W_H2, W_WP, W_F32_H2 = range(6)                                 # DF_CONV_W_*
FAM_REG, FAM_DMA, FAM_HALO, FAM_HALO_W16, FAM_HALO_X3, FAM_HALO_X3P = range(6)        # DF_CONV_FAM_*
XP, X16, BWS, DMA, CLS = 1, 2, 4, 8, 16                                              # DF_CONV_PLAN_*


def _with(d, **kw):
    """a copy of descriptor d with fields replaced"""
    from deflow_amd._lib import DfImg
    f = {k: getattr(d, k) for k, _ in DfImg._fields_}
    f.update(kw)
    return DfImg(*(f[k] for k, _ in DfImg._fields_))


def _stage(name, k, elt=0):
    """a 3x3 stride-1 layer's tensor at encoder stage k of a tests/helpers/rect_cases.py grid, as rect_cases.selection builds it (2B images, one
    group, no data)"""
    import rect_cases as RC
    c = RC.case(name)
    n, (h, w), C = 2 * c.B, c.stage_hw(k), RC.STAGE_C[k - 1]
    return _with(_desc((n, h, w, C), CC.layout((n, h, w, C), 0, False, "x")), ptr=_pair(1)[0].ptr, elt=elt)


def _plan(x, y, k, stride, mode, epi, weights):
    """-> (code, the plan's ten integers)"""
    import ctypes
    from deflow_amd._lib import load
    out = (ctypes.c_int32 * 10)()
    rc = load().df_conv2d_plan(x, y, k, stride, mode, epi, weights, ctypes.addressof(out))
    return rc, tuple(out)


def _forward_entries(lib, a):
    """name -> call(f) of the twelve forward / data-gradient launch entry points; f: x, y, t descriptors, w (the weights the entry point
    reads), w2 (df_conv2d_h2f_wp's planes), yb (y_bound), geometry, epilogue; every other pointer is the aligned address a"""
    import ctypes
    P = ctypes.c_void_p
    geo = lambda f: (f["ks"], f["stride"], f["pad"], f["mode"], f["epi"], P(a), P(a), P(f["stats"]), f["acc"])
    return {
        "df_conv2d": lambda f: lib.df_conv2d(f["x"], P(f["w"]), P(a), f["y"], *geo(f), P(0)),
        "df_conv2d_mp": lambda f: lib.df_conv2d_mp(f["x"], P(f["w"]), P(a), f["y"], *geo(f), 0, P(0)),
        "df_conv2d_amax": lambda f: lib.df_conv2d_amax(f["x"], P(f["w"]), P(a), f["y"], *geo(f), P(a), P(0)),
        "df_conv2d_w16": lambda f: lib.df_conv2d_w16(f["x"], P(f["w"]), P(a), f["y"], *geo(f), P(0)),
        "df_conv2d_x3": lambda f: lib.df_conv2d_x3(f["x"], P(f["w"]), P(a), f["y"], *geo(f), P(0)),
        "df_conv2d_h2": lambda f: lib.df_conv2d_h2(f["x"], P(f["w"]), P(a), P(a), P(a), f["y"], *geo(f), P(a), P(0)),
        "df_conv2d_h2p": lambda f: lib.df_conv2d_h2p(f["x"], P(f["w"]), P(a), P(a), P(a), f["y"], P(f["yb"]), *geo(f), P(a), P(0)),
        "df_conv2d_h2p_dgrad_bn": lambda f: lib.df_conv2d_h2p_dgrad_bn(f["x"], P(f["w"]), P(a), P(a), f["y"], P(a), P(a), P(a), P(a), P(0)),
        "df_conv2d_h2f": lambda f: lib.df_conv2d_h2f(f["x"], P(f["w"]), P(a), P(a), P(a), f["y"], *geo(f), P(a), P(0)),
        "df_conv2d_h2f_wp": lambda f: lib.df_conv2d_h2f_wp(f["x"], P(f["w"]), P(f["w2"]), P(a), P(a), P(a), f["y"], P(f["yb"]), *geo(f), P(a), P(0)),
        "df_conv2d_h2f_wp_up": lambda f: lib.df_conv2d_h2f_wp_up(f["x"], P(f["w"]), P(f["w2"]), P(a), P(a), P(a), f["y"], P(f["yb"]), f["t"], 0, P(0)),
        "df_conv2d_yh2": lambda f: lib.df_conv2d_yh2(f["x"], P(f["w"]), P(a), P(a), P(a), f["y"], P(f["yb"]), *geo(f), P(0)),
    }


FIXED_GEOMETRY = ("df_conv2d_h2p_dgrad_bn", "df_conv2d_h2f_wp_up")         # no ksize / stride / pad / mode / epi / accumulate arguments
NEEDS_H2_OUTPUT = ("df_conv2d_yh2", "df_conv2d_h2f_wp_up")                 # refuse y.elt != 2 themselves
READS_H2 = ("df_conv2d_h2", "df_conv2d_h2p", "df_conv2d_h2p_dgrad_bn")      # accept an h2 input


@pytest.mark.parametrize("case", ["tail64", "halo_thin"])
def test_forward_entry_points_refuse_before_launching(case):
    """per launch entry point and ONE fault in an otherwise complete call, the status the entry point documents; every call returns before
    a launch.  The faults: a null / misaligned weight pointer, an h2 image where fp32 is read, an h2 output with accumulate or without its
    bound, x.n != y.n, a bad ksize / stride / pad, DF_EPI_STATS without its buffer or with rows per group that are no tile multiple,
    DF_EPI_BWD_STATS on a forward call, an upsample source of the wrong size"""
    from deflow_amd._lib import load
    p = CC.PROBS[case][0]
    x, y = _descs(p)
    a = x.ptr
    entries = _forward_entries(load(), a)
    for name, fn in entries.items():
        base = dict(x=x, y=_with(y, elt=2) if name in NEEDS_H2_OUTPUT else y, t=_with(y, h=2, w=4), w=a, w2=a, yb=a, ks=p.k, stride=p.stride,
                    pad=p.k // 2, mode=CC.FWD, epi=CC.EPI[p.epi], stats=a, acc=0)
        if name == "df_conv2d_h2f_wp_up":
            base.update(ks=1, pad=0)
        faults = [("w NULL", dict(w=0), E_ALIGN), ("w misaligned", dict(w=a + 4), E_ALIGN),
                  ("y h2 without its bound", dict(y=_with(y, elt=2), yb=0), CC.E_ARG),
                  ("x.n != y.n", dict(y=_with(base["y"], n=2 * y.n)), CC.E_SHAPE)]
        if name not in READS_H2:
            faults.append(("x h2", dict(x=_with(x, elt=2)), CC.E_ARG if name == "df_conv2d_w16" else E_ALIGN))
        if name in ("df_conv2d_h2f_wp", "df_conv2d_h2f_wp_up"):
            faults += [("w2 NULL", dict(w2=0), CC.E_ARG), ("w2 misaligned", dict(w2=a + 4), CC.E_ARG)]
        if name == "df_conv2d_h2f_wp_up":
            faults.append(("t of the wrong size", {}, CC.E_SHAPE))             # (2 t.h != y.h: the only fault of the base call)
        if name not in FIXED_GEOMETRY:
            bwd_code = E_ALIGN if name == "df_conv2d_h2p" else CC.E_ARG      # (df_conv2d_h2p refuses the epilogue in its own first check)
            faults += [("y h2 with accumulate", dict(y=_with(y, elt=2), acc=1), CC.E_ARG),
                       ("ksize 5", dict(ks=5, pad=2), CC.E_SHAPE), ("stride 3", dict(stride=3), CC.E_SHAPE), ("pad 0", dict(pad=0), CC.E_SHAPE),
                       ("stats without a buffer", dict(epi=CC.EPI["stats"], stats=0), CC.E_ARG),
                       ("bwd_stats on a forward call", dict(epi=3), bwd_code)]
            if case == "tail64":
                assert ((p.grp or p.n) * p.ho * p.wo) % 64 != 0
                faults.append(("stats rows per group no tile multiple", dict(epi=CC.EPI["stats"]), CC.E_SHAPE))
        for what, kw, code in faults:
            got = fn({**base, **kw})
            print(f"[conv refusals] {case} {name}: {what} -> {got}")
            assert got == code, (case, name, what, got)


def test_forward_query_consistency():
    """df_conv2d_variant and df_conv2d_tile_m agree; the three _ok queries answer as the case tables say -- on every problem of conv_cases.py
    and every row of rect_cases.py"""
    import rect_cases as RC
    from deflow_amd._lib import call
    for p in ALL:
        x, y = _descs(p)
        mode, epi = CC.FWD if p.mode == "fwd" else CC.DGRAD, CC.EPI[p.epi]
        rpg = (p.grp or p.n) * p.out_shape[1] * p.out_shape[2]
        assert call("df_conv2d_tile_m", rpg, p.out_shape[3]) == call("df_conv2d_variant", rpg, rpg, p.out_shape[3], CC.EPI["stats"]) // 1000, p.pid
        ok = tuple(call(q, x, y, p.k, p.stride, mode, epi) for q in ("df_conv2d_x3_ok", "df_conv2d_h2p_ok", "df_conv2d_w16_ok"))
        assert ok == ((1, 1, 1) if p.case.startswith("halo") else (0, 0, 0)), (p.pid, ok)
        assert ("x3" in CC.forms(p.case)) == ("h2" in CC.forms(p.case)) == ("w16" in CC.forms(p.case)) == (ok == (1, 1, 1)), p.pid
        assert call("df_conv2d_h2p_ok", _with(x, elt=2), y, p.k, p.stride, mode, epi) == 0, p.pid     # (too few tiles for the pre-split forms)
    for (name, k), want in RC.SELECTION.items():
        c = RC.case(name)
        assert RC.selection(c, k) == want, (name, k)
        assert want[0] == call("df_conv2d_variant", c.rows_pg(k), c.rows_pg(k), RC.STAGE_C[k - 1], CC.EPI["stats"]) // 1000


def test_forward_plan():
    """df_conv2d_plan, the one dispatch behind the launches, the queries and the profiler labels, pinned on the case tables"""
    import rect_cases as RC
    from deflow_amd._lib import call
    queries = (("df_conv2d_x3_ok", W_X3), ("df_conv2d_h2p_ok", W_H2), ("df_conv2d_w16_ok", W_B16))

    def check_queries(x, y, k, stride, mode, epi, tag):
        for q, kind in queries:
            rc, pl = _plan(x, y, k, stride, mode, epi, kind)
            assert (call(q, x, y, k, stride, mode, epi) == 1) == (rc == E_OK) == (pl[0] >= 0), (tag, q)
            assert rc in (E_OK, CC.E_SHAPE, CC.E_ARG, E_ALIGN)

    for p in ALL:
        x, y = _descs(p)
        mode, epi = CC.FWD if p.mode == "fwd" else CC.DGRAD, CC.EPI[p.epi]
        rc, pl = _plan(x, y, p.k, p.stride, mode, epi, W_F32)
        tl = CC.tiling(p)
        halo = p.case.startswith("halo") and p.w % 128 == 0                 # (the fp32 tiles have no row-pair form for W == 64)
        assert rc == E_OK and (pl[0] == FAM_HALO) == halo and bool(pl[8] & CLS) == tl["cls"], (p.pid, rc, pl)
        if pl[0] != FAM_HALO:
            assert pl[0] == (FAM_DMA if pl[8] & DMA else FAM_REG) and pl[1] * 1000 + pl[2] == tl["var"] and pl[9] == 1, (p.pid, pl)
        assert bool(pl[8] & DMA) == (not (p.mode == "dgrad" and p.stride == 2 and not tl["cls"])), p.pid       # the generic stride-2 data gradient: registers
        check_queries(x, y, p.k, p.stride, mode, epi, p.pid)
        for xe, ye in ((2, 0), (0, 2), (1, 1)):
            check_queries(_with(x, elt=xe), _with(y, elt=ye), p.k, p.stride, mode, epi, p.pid)
    assert all(_plan(*_descs(p), p.k, p.stride, CC.DGRAD, 0, W_F32)[1][8] & CLS for p in CC.PROBS["s2_class"])
    assert not any(_plan(*_descs(p), p.k, p.stride, CC.DGRAD, 0, W_F32)[1][8] & CLS for p in _by("s2_odd", mode="dgrad"))
    # the benchmark's layer shapes: [320,512] at B = 16 reaches the persistent plane form at 512 x 64 (stage 1: two rows of W = 256), 256 x 128
    # (stage 2: two rows of W = 128; stage 3: four of W = 64), the statistics table still in 128-row tiles
    want = {1: (FAM_HALO_X3P, 512, 64, 8, 1, 2, 3, 2, XP | DMA, 4), 2: (FAM_HALO_X3P, 256, 128, 4, 2, 2, 4, 2, XP | DMA, 2),
            3: (FAM_HALO_X3P, 256, 128, 4, 2, 4, 4, 2, XP | DMA, 2)}
    for k in (1, 2, 3):
        xh, y = _stage("320x512", k, 2), _stage("320x512", k)
        for mode, epi in ((CC.FWD, 0), (CC.FWD, 1), (CC.DGRAD, 0)):
            assert _plan(xh, y, 3, 1, mode, epi, W_H2) == (E_OK, want[k]), (k, mode, epi)
            assert _plan(xh, _with(y, elt=2), 3, 1, mode, epi, W_H2) == (E_OK, want[k]), (k, mode, epi)
            check_queries(xh, y, 3, 1, mode, epi, k)
        assert _plan(xh, y, 3, 1, CC.DGRAD, 3, W_H2) == (E_OK, want[k][:8] + (XP | DMA | BWS,) + want[k][9:])
        rc, pl = _plan(y, y, 3, 1, CC.FWD, 1, W_H2)                      # fp32 input: the same tile on the register-staged halo
        assert rc == E_OK and pl == (FAM_HALO_X3,) + want[k][1:8] + (DMA,) + want[k][9:]
        assert _plan(xh, y, 3, 1, CC.FWD, 0, W_X3)[0] == _plan(xh, y, 3, 1, CC.FWD, 0, W_F32)[0] == E_ALIGN        # (only the fp16x2 planes read an h2 image)
    for (name, k) in RC.SELECTION:
        for mode, epi in ((CC.FWD, 1), (CC.DGRAD, 0)):
            for xe, ye in ((0, 0), (2, 0), (1, 1)):
                check_queries(_stage(name, k, xe), _stage(name, k, ye), 3, 1, mode, epi, (name, k))
    for k in (1, 2, 3):                                                 # [64,96]: W = 48 / 24 / 12 reaches none of the haloed forms
        x = _stage("64x96", k)
        assert _plan(x, x, 3, 1, CC.FWD, 1, W_F32)[1][0] == FAM_DMA
        assert [_plan(x, x, 3, 1, CC.FWD, 1, kind)[0] for kind in (W_X3, W_H2, W_B16)] == [CC.E_SHAPE] * 3
    # a tensor past what a buffer descriptor reaches falls to the register-staged family; a bf16 output needs the DMA kernels' epilogue
    x, y = _pair(1)
    far = _with(x, img_stride=_edge_stride(128, 4, 4))
    assert _plan(x, y, 3, 1, CC.FWD, 0, W_F32)[1][0] == FAM_DMA
    assert _plan(far, y, 3, 1, CC.FWD, 0, W_F32) == (E_OK, (FAM_REG, 64, 64, 2, 2, 1, 0, 0, 0, 1))
    assert _plan(far, _with(y, elt=1), 3, 1, CC.FWD, 0, W_F32)[0] == CC.E_SHAPE and _plan(x, _with(y, elt=1), 3, 1, CC.FWD, 0, W_F32)[0] == E_OK
    assert _plan(x, y, 3, 1, CC.FWD, 0, 6)[0] == CC.E_ARG


# (descriptors, form, h2f) -> the label; the strings are the parent's ops.conv2d, derived by hand
LABELS = [
    (("stage", "320x512", 2, 0, 0), CC.FWD, 1, "h2", False, "conv_halo_x3_kernel<256,128,4,2,2,4,2>"),
    (("stage", "320x512", 2, 2, 0), CC.FWD, 1, "h2p", False, "conv_halo_x3_kernel<256,128,4,2,2,4,2,xp>"),
    (("stage", "320x512", 3, 2, 2), CC.DGRAD, 0, "h2p", False, "conv_halo_x3_kernel<256,128,4,2,4,4,2,xp>"),
    (("stage", "320x512", 1, 2, 0), CC.DGRAD, 0, "dgrad_bn", False, "conv_halo_x3_kernel<512,64,8,1,2,3,2,xp>"),
    (("stage", "320x512", 1, 0, 0), CC.FWD, 1, "x3", False, "conv_halo_x3_kernel<256,64,4,2,1,4>"),
    (("stage", "320x512_b8", 3, 0, 0), CC.FWD, 1, "h2", False, "conv_halo_x3_kernel<128,128,2,4,2,4,2>"),
    (("stage", "192x256", 1, 1, 1), CC.FWD, 1, "w16", False, "conv_halo_w16_kernel<64,4,2,1>"),
    (("stage", "192x256", 2, 0, 0), CC.DGRAD, 0, "w16", False, "conv_halo_w16_kernel<128,2,4,2>"),
    (("stage", "320x512", 2, 0, 0), CC.FWD, 0, "mp", False, "conv_halo_kernel<128,2,4>"),
    (("stage", "320x512", 1, 0, 0), CC.FWD, 0, "amax", False, "conv_halo_kernel<64,4,2>"),
    (("1x1", "320x512", 2, 0, 0), CC.FWD, 0, "h2f_wp", True, "conv_dma_kernel<128,128,2,4>/h2"),
    (("1x1", "320x512", 2, 0, 2), CC.FWD, 0, "yh2", True, "conv_dma_kernel<128,128,2,4>/h2"),
    (("1x1", "320x512", 1, 0, 0), CC.DGRAD, 0, "h2f", True, "conv_dma_kernel<128,64,4,2>/h2"),
    (("1x1", "320x512", 1, 0, 0), CC.FWD, 0, "amax", False, "conv_dma_kernel<128,64,4,2>"),
    (("1x1", "64x96", 3, 0, 0), CC.FWD, 0, "h2f", True, "conv_dma_kernel<64,64,2,2>"),
    (("prob", "tail64", 0), None, None, "mp", False, "conv_dma_kernel<64,64,2,2>"),
    (("prob", "n32", 3), None, None, "mp", False, "conv_dma_kernel<128,32,4,1>"),
    (("prob", "s2_odd", 2), None, None, "mp", False, "conv_kernel<128,32,4,1>"),
    (("prob", "s2_class", 0), None, None, "amax", False, "conv_dma_kernel<64,64,2,2>"),
    (("prob", "halo_thin", 2), None, None, "x3", False, "conv_halo_x3_kernel<256,64,4,2,1,4>"),
    (("prob", "halo_thin", 1), None, None, "h2", False, "conv_halo_x3_kernel<128,64,4,2,2,8,2>"),
    (("prob", "halo_thin", 3), None, None, "x3", False, "conv_halo_x3_kernel<128,128,2,4,1,4>"),
]


def test_profiler_labels():
    """ops._conv_label formats the label from the plan; bench.py keys its roofline block on `conv_halo_x3_kernel<...,2>`, a trailing `,xp>`,
    `conv_dma_kernel<128,...>/h2`, `conv_halo_w16_kernel` and `conv_kernel`"""
    from deflow_amd import ops
    for src, mode, epi, form, h2f, want in LABELS:
        if src[0] == "prob":
            p = CC.PROBS[src[1]][src[2]]
            x, y = _descs(p)
            k, stride, mode, epi = p.k, p.stride, CC.FWD if p.mode == "fwd" else CC.DGRAD, CC.EPI[p.epi]
        else:
            x, y = _stage(src[1], src[2], src[3]), _stage(src[1], src[2], src[4])
            k, stride = (3, 1) if src[0] == "stage" else (1, 1)
        assert ops._conv_label(x, y, k, stride, mode, epi, form, h2f) == want, (src, form)
    for shape in ("conv_halo_x3_kernel<", ",2>", ",xp>", "conv_dma_kernel<128,", "/h2", "conv_halo_w16_kernel<", "conv_kernel<"):
        assert any(shape in row[-1] for row in LABELS), shape


# the library's own split counts (wgrad, wgrad1_h2, wgrad_s2_h2) per weight-gradient problem, in table order
OWN_SPLITS = {"w_ragged": [15], "w_two_seg": [60], "w_x3": [12, 12], "w_s2_odd": [30], "w_k96": [4], "w_1x1": [14, 14, 14], "w_rows": [8], "w_views": [20, 60]}


def test_weight_gradient_form_queries_and_splits():
    from deflow_amd._lib import call
    for case in CC.WNAMES:
        for p, own in zip(CC.WPROBS[case], OWN_SPLITS[case]):
            x, dy = _wdescs(p)
            assert call("df_conv2d_wgrad_splits", x, dy, p.k, p.stride) == own == len(CC.wchunks(p)[2]), p.pid
            x3 = call("df_conv2d_wgrad_x3_ok", x, dy, p.k, p.stride)
            assert x3 == int(p.k == 3 and p.stride == 1 and p.wo % 32 == 0), p.pid
            assert ("x3" in CC.wforms(case, p)) == ("h2" in CC.wforms(case, p)) == ("bf16" in CC.wforms(case, p)) == bool(x3), p.pid
            if p.k == 1:
                assert call("df_conv2d_wgrad1_h2_ok", x, dy) == 1 and call("df_conv2d_wgrad1_h2_splits", x, dy) == own
                assert ("w1h2" in CC.wforms(case, p)) == (p.row_counts is None)           # (row lists: df_conv2d_wgrad_mp only)
            if p.stride == 2:
                assert call("df_conv2d_wgrad_s2_h2_ok", x, dy) == 1 and call("df_conv2d_wgrad_s2_h2_splits", x, dy) == own
                assert "s2h2" in CC.wforms(case, p) and "s2bf16" in CC.wforms(case, p)
            for form in CC.wforms(case, p):
                assert own in CC.wsplits(p, form, x, dy)


def test_pre_split_weight_gradient_query_and_splits():
    """df_conv2d_wgrad_h2p_ok / _splits on the w_x3 problems as h2 images (elt = 2): one 12-wave workgroup per CU = 256 workgroups over
    64 x 64 tiles, 32-pixel chunks, at most one split per chunk, every split non-empty"""
    from deflow_amd._lib import call
    for p in CC.WPROBS["w_x3"]:
        xs, ds = (p.n, p.h, p.w, p.cin), (p.n, p.ho, p.wo, p.cout)
        x, dy = _desc(xs, CC.layout(xs, p.grp, p.views, "x"), 2), _desc(ds, CC.layout(ds, p.grp, p.views, "y"), 2)
        assert call("df_conv2d_wgrad_h2p_ok", x, dy, p.k, p.stride) == 1, p.pid
        tiles, chunks = (p.cin + 63) // 64 * (p.cout // 64), p.n * p.ho * ((p.wo + 31) // 32)
        s = max(1, min(-(-256 // tiles), chunks))
        cps = -(-chunks // s)
        assert call("df_conv2d_wgrad_h2p_splits", x, dy) == -(-chunks // cps) == 12, p.pid
        assert call("df_conv2d_wgrad_h2p_ok", *_wdescs(p), p.k, p.stride) == 0                      # fp32 images are not its operands
        assert call("df_conv2d_wgrad_h2p_ok", x, dy, 3, 2) == 0 and call("df_conv2d_wgrad_h2p_ok", x, dy, 1, 1) == 0


# ---- what a DMA-fed weight-gradient kernel can address -----------------------------------------------------------------------------
DMA_BAD = 0xFFFFFFFF - (8 << 20)          # conv_common.h: buffer extents at or above it are refused
E_ALIGN = -2


def _pair(stride, elt=0, **kw):
    """x [2,4,32,64] -> dy [2,4,32,64] (stride 1) or [2,2,16,64] (stride 2), both one group of two images: `img_stride` counts in the
    extent, `grp_off` does not.  kw: fields to overwrite, as x_<field> / y_<field>; nobody dereferences the address"""
    from deflow_amd._lib import DfImg
    probe = torch.empty(64, dtype=torch.float32)
    base = (probe.data_ptr() + 127) // 128 * 128
    out = []
    for side, (h, w) in (("x", (4, 32)), ("y", (4, 32) if stride == 1 else (2, 16))):
        f = dict(ptr=base, n=2, h=h, w=w, c=64, ld=64, grp_size=2, img_stride=h * w * 64, grp_off=2 * h * w * 64, elt=elt, reserved=0)
        f.update({k[2:]: v for k, v in kw.items() if k.startswith(side + "_")})
        out.append(DfImg(*(f[k] for k, _ in DfImg._fields_)))
    return out


def _edge_stride(hw, elt_bytes, gran):
    """the largest img_stride (a multiple of gran elements) whose extent (img_stride + hw * 64) * elt_bytes stays below DMA_BAD"""
    s = ((DMA_BAD - 1) // elt_bytes - hw * 64) // gran * gran
    assert (s + hw * 64) * elt_bytes < DMA_BAD <= (s + gran + hw * 64) * elt_bytes
    return s


def _not_addressable(hw_x, hw_y, elt_bytes, gran):
    """descriptor changes after which one side is out of a buffer descriptor's reach"""
    out = []
    for side, hw in (("x", hw_x), ("y", hw_y)):
        out += [{side + "_img_stride": -hw * 64}, {side + "_grp_off": -2 * hw * 64}, {side + "_img_stride": _edge_stride(hw, elt_bytes, gran) + gran}]
    return out


def test_weight_gradient_dma_addressability():
    from ctypes import c_void_p as P
    from deflow_amd._lib import call, load
    ws = _pair(1)[0].ptr
    queries = (("df_conv2d_wgrad_x3_ok", 1, (3, 1)), ("df_conv2d_wgrad1_h2_ok", 1, ()), ("df_conv2d_wgrad_s2_h2_ok", 2, ()))
    for name, stride, tail in queries:
        hw_y = 128 if stride == 1 else 32
        assert call(name, *_pair(stride), *tail) == 1, name
        for kw in _not_addressable(128, hw_y, 4, 4):
            assert call(name, *_pair(stride, **kw), *tail) == 0, (name, kw)
        for kw in ({"x_img_stride": _edge_stride(128, 4, 4)}, {"y_img_stride": _edge_stride(hw_y, 4, 4)}):
            assert call(name, *_pair(stride, **kw), *tail) == 1, (name, kw)                          # just below DMA_BAD
    for name, stride, tail in queries[1:]:
        for kw in ({"x_ld": 66}, {"y_ld": 66}):
            assert call(name, *_pair(stride, **kw), *tail) == 0, (name, kw)
    # the pre-split form: geometry and extents of the fp32 tensor (4 bytes per element), 128-byte lines
    assert call("df_conv2d_wgrad_h2p_ok", *_pair(1, 2), 3, 1) == 1
    for kw in _not_addressable(128, 128, 4, 32):
        assert call("df_conv2d_wgrad_h2p_ok", *_pair(1, 2, **kw), 3, 1) == 0, kw
    for kw in ({"x_img_stride": _edge_stride(128, 4, 32)}, {"y_img_stride": _edge_stride(128, 4, 32)}):
        assert call("df_conv2d_wgrad_h2p_ok", *_pair(1, 2, **kw), 3, 1) == 1, kw
    for side in "xy":
        for kw in ({side + "_ld": 68}, {side + "_img_stride": 128 * 64 + 4}, {side + "_ptr": ws + 16}):
            assert call("df_conv2d_wgrad_h2p_ok", *_pair(1, 2, **kw), 3, 1) == 0, kw
    # bfloat16 tensors: 2 bytes per element; the entry point itself refuses (nothing is launched)
    for kw in _not_addressable(128, 128, 2, 8):
        x, dy = _pair(1, 1, **kw)
        assert load().df_conv2d_wgrad_bf16(x, dy, 3, 1, 1, P(ws), 1, P(0), P(0)) == CC.E_SHAPE, kw


def test_weight_gradient_entry_points_refuse_before_launching():
    """per launch entry point, the status for (ws = NULL, splits = 0, both): the first failing check decides, in the order of its
    DF_REQUIREs; wgrad1_h2 / s2_h2 also for one bound without the other.  Every call returns before a launch."""
    import ctypes
    from deflow_amd._lib import load
    lib, P = load(), ctypes.c_void_p
    x, dy = _pair(1)
    x2, dy2 = _pair(2)
    xh, dyh = _pair(1, 2)
    xb, dyb = _pair(1, 1)
    a = x.ptr                  # an aligned non-NULL address for ws and the bounds
    entries = {     # name: (call with (ws, splits), (code for ws = NULL, for splits = 0, for both))
        "df_conv2d_wgrad_mp": (lambda ws, s: lib.df_conv2d_wgrad_mp(x, dy, 3, 1, 1, P(ws), s, P(0), 0, P(0), 0, P(0)), (E_ALIGN, CC.E_SHAPE, E_ALIGN)),
        "df_conv2d_wgrad": (lambda ws, s: lib.df_conv2d_wgrad(x, dy, 3, 1, 1, P(ws), s, P(0), 0, P(0), P(0)), (E_ALIGN, CC.E_SHAPE, E_ALIGN)),
        "df_conv2d_wgrad_x3": (lambda ws, s: lib.df_conv2d_wgrad_x3(x, dy, 3, 1, 1, P(ws), s, P(0), P(0)), (CC.E_SHAPE,) * 3),
        "df_conv2d_wgrad_h2": (lambda ws, s: lib.df_conv2d_wgrad_h2(x, dy, P(a), P(a), 3, 1, 1, P(ws), s, P(0), P(0)), (CC.E_SHAPE,) * 3),
        "df_conv2d_wgrad1_h2": (lambda ws, s: lib.df_conv2d_wgrad1_h2(x, dy, P(a), P(a), P(ws), s, P(0), P(0)), (CC.E_ARG, CC.E_SHAPE, CC.E_ARG)),
        "df_conv2d_wgrad_s2_h2": (lambda ws, s: lib.df_conv2d_wgrad_s2_h2(x2, dy2, P(a), P(a), P(ws), s, P(0), P(0)), (CC.E_ARG, CC.E_SHAPE, CC.E_ARG)),
        "df_conv2d_wgrad_h2p": (lambda ws, s: lib.df_conv2d_wgrad_h2p(xh, dyh, P(a), P(a), 3, 1, 1, P(ws), s, P(0), P(0)), (CC.E_ARG, CC.E_SHAPE, CC.E_ARG)),
        "df_conv2d_wgrad_bf16": (lambda ws, s: lib.df_conv2d_wgrad_bf16(xb, dyb, 3, 1, 1, P(ws), s, P(0), P(0)), (E_ALIGN, CC.E_SHAPE, E_ALIGN)),
    }
    for name, (fn, codes) in entries.items():
        got = (fn(0, 1), fn(a, 0), fn(0, 0))
        print(f"[wgrad refusals] {name}: ws NULL {got[0]}, splits 0 {got[1]}, both {got[2]}")
        assert got == codes, (name, got)
    for b in ((a, 0), (0, a)):
        assert lib.df_conv2d_wgrad1_h2(x, dy, P(b[0]), P(b[1]), P(a), 1, P(0), P(0)) == CC.E_ARG
        assert lib.df_conv2d_wgrad_s2_h2(x2, dy2, P(b[0]), P(b[1]), P(a), 1, P(0), P(0)) == CC.E_ARG
        assert lib.df_conv2d_wgrad_h2(x, dy, P(b[0]), P(b[1]), 3, 1, 1, P(a), 1, P(0), P(0)) == CC.E_ARG
        assert lib.df_conv2d_wgrad_h2p(xh, dyh, P(b[0]), P(b[1]), 3, 1, 1, P(a), 1, P(0), P(0)) == CC.E_ARG


# ---- chunks and splits ----------------------------------------------------------------------------------------------------------
def _split_facts(p, splits):
    P, cpr, chunks = CC.wchunks(p)
    rng = CC.split_ranges(len(chunks), splits)
    return dict(mid_row=[s for s, (lo, hi) in enumerate(rng) if lo < hi and chunks[lo][2] != 0],
                mid_image=[s for s, (lo, hi) in enumerate(rng) if lo < hi and (chunks[lo][1] != 0 or chunks[lo][2] != 0)],
                crosses=[s for s, (lo, hi) in enumerate(rng) if lo < hi and chunks[lo][0] != chunks[hi - 1][0]],
                sizes=[max(hi - lo, 0) for lo, hi in rng], empty=[s for s, (lo, hi) in enumerate(rng) if lo >= hi])


def test_chunk_walk():
    p = CC.WPROBS["w_ragged"][0]
    assert CC.wchunks(p)[:2] == (32, 1) and len(CC.wchunks(p)[2]) == 15 and p.wo == 9
    f = _split_facts(p, 2)
    assert f["sizes"] == [8, 7] and f["crosses"] == [0, 1] and f["mid_image"] == [1]       # split 1 starts at image 1, row 3
    assert _split_facts(p, 9)["empty"] == [8] and _split_facts(p, 9)["sizes"][7] == 1 and _split_facts(p, 15)["sizes"] == [1] * 15
    p = CC.WPROBS["w_two_seg"][0]
    assert CC.wchunks(p)[:2] == (32, 2) and len(CC.wchunks(p)[2]) == 60 and p.wo % 32 == 8
    assert _split_facts(p, 9)["mid_row"] == [1, 3, 5, 7] and _split_facts(p, 7)["mid_row"] == [1, 3, 5]
    assert _split_facts(p, 7)["crosses"] == [3] and _split_facts(p, 16)["empty"] == [15] and _split_facts(p, 60)["empty"] == []
    for p in CC.WPROBS["w_x3"]:
        assert CC.wchunks(p)[:2] == (32, 2) and len(CC.wchunks(p)[2]) == 12
        assert max(_split_facts(p, 12)["sizes"]) == 1 < 2 and _split_facts(p, 8)["empty"] == [6, 7]      # fewer stages than the shallowest ring (2)
    p = CC.WPROBS["w_s2_odd"][0]
    assert CC.wchunks(p)[:2] == (16, 3) and p.wo == 34 == 16 + 16 + 2 and len(CC.wchunks(p)[2]) == 30
    assert (p.wo - 1) * 2 + 1 == p.w and 32 * 2 + 33 - 1 > p.w and p.cin == 32                # the last chunk's 33-pixel patch passes the right border
    assert _split_facts(p, 7)["empty"] == [6] and _split_facts(p, 4)["mid_row"] == [1, 2]
    p = CC.WPROBS["w_k96"][0]
    assert (p.cin + 63) // 64 == 2 and p.cin % 64 == 32 and p.cout // 64 == 3 and _split_facts(p, 3)["empty"] == [2]
    for p in CC.WPROBS["w_1x1"]:
        assert CC.wchunks(p)[:2] == (32, 1) and p.wo == 11 and _split_facts(p, 8)["empty"] == [7]
    assert [(p.cin, p.cout) for p in CC.WPROBS["w_1x1"]] == [(64, 64), (128, 128), (96, 128)]
    p = CC.WPROBS["w_rows"][0]
    ok = CC.row_ok(p).view(6, 40)
    assert ok.sum(1).tolist() == [0, 1, 31, 32, 33, 40] and bool(ok[2, :31].all()) and not bool(ok[2, 31:].any())
    valid = CC.row_ok(p).view(-1)
    assert bool(valid[2 * 40 + 30]) and not bool(valid[2 * 40 + 31]) and bool(valid[3 * 40 + 31]) and bool(valid[4 * 40 + 32])
    assert _split_facts(p, 5)["empty"] == [4]
    # segment 2 (pixels 80 .. 119) ends its valid run at pixel 110; chunk 3 = pixels 96 .. 127 holds the boundary; segment 3 ends on pixel
    # 151, the last valid pixel before chunk boundary 160 is 8 pixels short: both sides of a chunk boundary see valid and invalid pixels
    assert not bool(valid[96:128].all()) and bool(valid[96:111].all()) and bool(valid[120:152].all()) and not bool(valid[152:160].any())


# ---- the restatements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.NAMES)
def test_row_walk_equals_ref64(case):
    for p in CC.PROBS[case]:
        _close(CC.restate(p), CC.reference(p)["plain"][1], p.pid)


def test_chain_reference_is_the_reference():
    p = CC.PROBS["tail64"][1]
    e = R.errors(CC.chain32(p), CC.reference(p)["plain"][1])
    assert e["finite"] and e["max"] <= 2e-6, e


@pytest.mark.parametrize("case", CC.WNAMES)
def test_chunk_walk_equals_ref64(case):
    for p in CC.WPROBS[case]:
        dw64, db64 = CC.wreference(p)["plain"][1]
        for s in p.splits:
            ws, bws = CC.partials64(p, s or len(CC.wchunks(p)[2]))
            assert bool(torch.isfinite(ws).all()) and bool(torch.isfinite(bws).all())
            _close(CC.reduce64(ws), dw64, p.pid)
            _close(bws.sum(0), db64, p.pid)


# ---- the faults -----------------------------------------------------------------------------------------------------------------
def _over(p, got):
    r32, r64 = CC.reference(p)["plain"]
    return CC.excess(R.errors(got, r64), CC.bounds(CC.CONV32, r32, r64, -1))


def _wover(p, got):
    (dw32, _), (dw64, _) = CC.wreference(p)["plain"]
    return CC.excess(R.errors(got, dw64, 0), CC.bounds(CC.CONV32, dw32, dw64, 0))


@pytest.mark.parametrize("case", ["tail64", "tail128", "n32", "s2_odd", "views"])
def test_fault_ragged_tile_dropped_or_doubled(case):
    for p in CC.PROBS[case]:
        assert _over(p, CC.restate(p)) <= 1e-3
        assert _over(p, CC.restate(p, "drop_ragged")) >= 10, p.pid
        if p.acc:
            assert _over(p, CC.restate(p, "dup_ragged")) >= 10, p.pid


@pytest.mark.parametrize("case", ["tail64", "s2_odd", "thin", "views"])
def test_fault_rows_decoded_with_h_and_w_swapped(case):
    for p in CC.PROBS[case]:
        if p.out_shape[1] != p.out_shape[2]:
            assert _over(p, CC.restate(p, "swap_hw")) >= 10, p.pid


@pytest.mark.parametrize("case", ["tail64", "tail128", "thin", "halo_odd", "s2_odd"])
def test_fault_tap_wraps_into_the_neighbouring_row(case):
    for p in CC.PROBS[case]:
        # (one-row images have no neighbouring row; the taps of a stride-2 data gradient onto an odd image never leave dy: the parity
        # test takes out exactly those that would)
        if p.in_shape[1] > 1 and p.k == 3 and not (p.mode == "dgrad" and p.stride == 2):
            assert _over(p, CC.restate(p, "tap_wrap")) >= 10, p.pid


@pytest.mark.parametrize("case", ["tail64", "thin", "s2_class", "views"])
def test_fault_tile_reads_across_an_image_boundary(case):
    for p in CC.PROBS[case]:
        if p.n > 1 and p.k == 3 and not (p.mode == "dgrad" and p.stride == 2 and p.h % 2 == 1):
            assert _over(p, CC.restate(p, "cross_image")) >= 10, p.pid


def test_fault_last_chunk_of_a_row_skipped():
    for p in CC.WPROBS["w_two_seg"] + CC.WPROBS["w_s2_odd"]:
        assert _wover(p, CC.reduce64(CC.partials64(p, 7)[0])) <= 1e-3
        assert _wover(p, CC.reduce64(CC.partials64(p, 7, "skip_last_chunk")[0])) >= 10, p.pid


def test_fault_invalid_pixels_of_a_ragged_chunk_counted():
    for p in CC.WPROBS["w_ragged"] + CC.WPROBS["w_1x1"][:1]:
        assert _wover(p, CC.reduce64(CC.partials64(p, 2, "count_invalid")[0])) >= 10, p.pid


def test_fault_one_split_lost():
    for case in ("w_two_seg", "w_x3", "w_k96"):
        for p in CC.WPROBS[case]:
            assert _wover(p, CC.reduce64(CC.partials64(p, 4)[0], "lose_split")) >= 10, p.pid


def test_fault_row_counts_ignored():
    p = CC.WPROBS["w_rows"][0]
    assert _wover(p, CC.reduce64(CC.partials64(p, 3, "ignore_row_counts")[0])) >= 10


# ---- the fp32 references stay inside the bounds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.NAMES)
def test_fp32_reference_meets_the_bounds(case):
    for p in CC.PROBS[case]:
        for key in ("plain", "bf16"):
            r32, r64 = CC.reference(p)[key]
            e = R.errors(r32, r64)
            print(f"[conv cases] {p.pid} {key}: ref64 in fp32 vs float64 max {e['max']:.2e} rms {e['rms']:.2e} ch {e['ch']:.2e}")
            assert r32.dtype == torch.float32 and CC.bounds(CC.CONV32, r32, r64, -1).ok(e) and e["max"] <= CC.CONV32.max, (p.pid, e)
        r32, r64 = CC.reference(p)["plain"]
        if "ybf16" in CC.forms(case):
            assert R.bf16_excess(r32.bfloat16().float(), r64, CC.BF16_FLOOR) <= 1.0
        if p.epi == "stats":
            for form in ("mp", "x3"):
                a, b = CC.stats64(p, r32.double(), form), CC.stats64(p, r64, form)
                assert float((a - b).abs().max(0)[0].max() / b.abs().max()) <= CC.STATS_TOL


@pytest.mark.parametrize("case", CC.WNAMES)
def test_fp32_weight_gradient_reference_meets_the_bounds(case):
    for p in CC.WPROBS[case]:
        for key in ("plain", "bf16"):
            (dw32, db32), (dw64, db64) = CC.wreference(p)[key]
            e, eb = R.errors(dw32, dw64, 0), R.errors(db32, db64)
            print(f"[conv cases] {p.pid} {key}: ref64 in fp32 vs float64 dw max {e['max']:.2e} rms {e['rms']:.2e} ch {e['ch']:.2e} | db max {eb['max']:.2e}")
            assert CC.bounds(CC.CONV32, dw32, dw64, 0).ok(e) and e["max"] <= CC.CONV32.max and CC.bounds(CC.BIAS32, db32, db64, -1).ok(eb), (p.pid, e, eb)


def test_reduce_shapes():
    """64 x 9 x 36 = 81 blocks of 256 exactly; 65 output channels leave the last block of the weight part 68 threads and the bias part a
    third block with one column"""
    assert CC.REDUCE_COUTS == (64, 65) and CC.REDUCE_SHAPE["taps"] * CC.REDUCE_SHAPE["cin"] == 324 and CC.REDUCE_SHAPE["pad"] == 20
    assert (64 * 324) % 256 == 0 and (65 * 324) % 256 == 68 and 65 % 32 == 1


@pytest.mark.parametrize("cout", CC.REDUCE_COUTS)
@pytest.mark.parametrize("splits", CC.REDUCE_SPLITS)
def test_reduce_case(splits, cout):
    ws, bws, old = CC.reduce_case(splits, cout)
    assert ws.shape == (splits, cout, 324) and bws.shape == (splits, cout) and old.shape == (cout, 324)
    r32, r64 = CC.reduce_refs(ws, old)
    e = R.errors(r32, r64, 0)
    assert e["finite"] and e["max"] <= 1e-6
    b = bws.double().sum(0)
    assert bool(((bws.double().sum(0).float().double() - b).abs() <= CC.ulp32(b)).all())       # the rounded float64 sum is within one ulp
    # the loops' remainders: the 4-way body with 0 .. 3 left over; the bias part's 32-stride body (k + 24 < splits) and its stride-8 tail
    assert {s % 4 for s in CC.REDUCE_SPLITS} == {0, 1, 2, 3} and any(s > 24 for s in CC.REDUCE_SPLITS) and any(s <= 24 for s in CC.REDUCE_SPLITS)
    assert any(s > 32 and s % 8 for s in CC.REDUCE_SPLITS)
