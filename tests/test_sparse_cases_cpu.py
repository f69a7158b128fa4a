"""CPU: the conditions that make tests/test_gpu_sparse_cases.py meaningful, decided without a GPU.

  * the walk: a plain Python restatement of each kernel's iteration (helpers/sparse_cases.py: walk_pig, walk_conv, walk_win), fed with the
    constants read out of csrc/pillarize.hip, reaches in every case what the case table says it was built for -- a retuned kernel (another
    PGQ, window or workgroup size) fails here instead of quietly leaving the cases behind -- and visits every pillar head exactly once;
  * the references: the four ref64 functions agree to 1e-12 with float64 torch autograd of the dense layers (output gradient or input
    masked by occupancy), in every case;
  * the faults: each fault a kernel of this family could plausibly have, injected into the float64 restatement (never into a kernel),
    lands at least ten times over the bound the GPU test applies, in the case built for it.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref64 as R  # noqa: E402
import sparse_cases as SC  # noqa: E402

K = SC.constants()
D = torch.float64


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


# ---- the walk -----------------------------------------------------------------------------------------------------------------
def test_constants_are_what_the_cases_were_built_for():
    assert K == dict(PGQ=128, SW_WIN=256, SIW_WIN=512, PG_THREADS=1024), K


@pytest.mark.parametrize("run", SC.RUNS)
def test_every_walk_visits_every_head_once(run):
    c = SC.case(run)
    want = c.heads.tolist()
    for queued in (True, False):
        assert sorted(SC.walk_pig(c, K, queued=queued)[0]) == want
        assert sorted(SC.walk_conv(c, K, queued=queued)[0]) == want
    for win in (K["SW_WIN"], K["SIW_WIN"]):
        groups, _ = SC.walk_win(c, win)
        assert len(groups) == c.nblk * c.B
        assert sorted(torch.cat(groups).tolist()) == want
    assert c.counts.tolist() == [int(((c.keys.long() // (c.H * c.W)) == b).sum()) for b in range(c.B)]
    assert bool((c.keys[1:] >= c.keys[:-1]).all()) and c.keys.dtype == torch.int32 and c.counts.dtype == torch.int32
    for v in c.t.values():
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all())


def test_wrap_reaches_the_queue_wrap():
    c = SC.case("wrap")
    assert (c.B, c.H, c.W, c.nblk) == (1, 96, 104, 1)
    assert 8900 <= c.heads.numel() <= 9000 and c.keys.numel() == 10000
    for walk in (SC.walk_pig, SC.walk_conv):
        _, st = walk(c, K)
        assert st["max_windows"] >= 8, st
        assert st["max_pushed"] > K["PGQ"] and st["head_wraps"] >= 1, st       # a write index and a head index pass PGQ
        assert st["carried"] >= 8 and st["max_fill"] < K["PGQ"], st            # tails carry over; the queue never overflows
    _, st = SC.walk_pig(c, K)
    assert min(st["wraps_by_class"]) >= 1, st                                  # a head index wraps in every parity class


@pytest.mark.parametrize("name,cls", [("one_class", 0), ("single_tap", 3)])
def test_one_parity_class(name, cls):
    c = SC.case(name)
    cell = c.heads % (c.H * c.W)
    y, x = cell // c.W, cell % c.W
    assert bool((((((y + 1) & 1) << 1) | ((x + 1) & 1)) == cls).all())         # pillar_input_grad's class of every cell
    assert c.heads.numel() == 1152 and 2000 <= c.keys.numel() <= 2200 and c.nblk == 1
    _, st = SC.walk_pig(c, K)
    assert 64 < st["max_fill"] < K["PGQ"] and st["empty_queues"] == 3, st
    _, stc = SC.walk_conv(c, K)
    assert 64 < stc["max_fill"] < K["PGQ"], stc
    n = [[SC.in_wgrad_taps(c, hk)] for hk in SC.walk_win(c, K["SIW_WIN"])[0]]
    per_tap = torch.tensor(n).sum((0, 1)).tolist()
    if name == "one_class":     # taps (ky, kx) in {0, 2}^2; the other five waves write zero partials
        assert [t for t in range(9) if per_tap[t] == 0] == [1, 3, 4, 5, 7], per_tap
    else:
        assert [t for t in range(9) if per_tap[t] > 0] == [4], per_tap
    heads64 = SC.walk_win(c, 64)[1]["heads_per_window"]
    assert sum(h % 16 != 0 for h in heads64) >= 8 and heads64.count(64) >= 8, heads64


def test_border_is_the_border():
    c = SC.case("border")
    assert (c.B, c.H, c.W) == (2, 16, 24) and c.counts.tolist() == [76, 74]
    b, y, x = R.cells(c.heads, c.H, c.W)
    assert bool(((y == 0) | (y == c.H - 1) | (x == 0) | (x == c.W - 1)).all())
    corners = {(int(bb), int(yy), int(xx)) for bb, yy, xx in zip(b, y, x) if yy in (0, c.H - 1) and xx in (0, c.W - 1)}
    assert corners == {(0, 0, 0), (0, 0, 23), (0, 15, 0), (0, 15, 23), (1, 15, 0), (1, 15, 23)}
    # the stride-2 forms: oy = -1 (ky = 2 at y = 0) and ox = w2 (kx = 0 at x = W - 1) occur
    assert bool((y == 0).any()) and bool((x == c.W - 1).any())


@pytest.mark.parametrize("run", ["runs", "runs@engine"])
def test_runs_reaches_headless_windows(run):
    c = SC.case(run)
    assert c.counts.tolist() == [700, 0, 1, 70] and c.nblk == (2 if run == "runs" else 64)
    k0 = c.keys[:700].long()
    assert int((k0 == k0[300]).sum()) == 300 and k0[229] != k0[230] and k0[230] == k0[529] and k0[529] != k0[530]   # 230 .. 529
    assert k0[59] != k0[60] and k0[60] == k0[69] and k0[69] != k0[70]                                                  # straddles 64
    _, s64 = SC.walk_pig(c, K)
    _, s64c = SC.walk_conv(c, K)
    _, s256 = SC.walk_win(c, K["SW_WIN"])
    assert s64["empty_windows"] >= 1 and s64c["empty_windows"] >= 1 and s256["empty_windows"] >= 1, (s64, s64c, s256)
    assert s256["max_run"] > K["SW_WIN"]
    if run == "runs@engine":
        assert s256["idle"] >= 4 * 64 - 5


def test_idle_is_the_engines_launch():
    c = SC.case("idle")
    assert c.nblk == max(1, 256 // c.B) == 256 and c.keys.numel() == 37
    for st in (SC.walk_pig(c, K)[1], SC.walk_conv(c, K)[1], SC.walk_win(c, K["SW_WIN"])[1], SC.walk_win(c, K["SIW_WIN"])[1]):
        assert st["idle"] >= 250, st


def test_views_layouts():
    for name in ("views", "views_unaligned"):
        c = SC.case(name)
        assert c.counts.tolist() == [700, 0, 700] and c.nblk == 3
        lay = c.layout
        assert lay["x"][0] == 128 and lay["dy"][0] == 192 and lay["x"][1] % 4 == 0 and lay["dy"][1] % 4 == 0 and lay["y"][1] % 4 == 0
        assert lay["canvas"] == (64, 0) and lay["dcanvas"] == (64, 0)
        for k, (width, off) in lay.items():
            assert off + (32 if k in ("canvas", "dcanvas") else 64) <= width
    assert SC.LAYOUT["views"]["dskip"] == (128, 64)
    ld, off = SC.LAYOUT["views_unaligned"]["dskip"]
    assert ld == 66 and ld % 2 == 0 and (ld * 4) % 16 != 0          # rows are not 16-byte aligned: df_pillar_input_grad's fp32 form


# ---- the references ---------------------------------------------------------------------------------------------------------
def _close(a, b, tag):
    e = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
    assert e <= 1e-12, (tag, e)


@pytest.mark.parametrize("name", [n for n in SC.NAMES if n != "views_unaligned"])
def test_references_vs_float64_autograd(name):
    c = SC.case(name)
    _, r64 = SC.reference(name)
    t = {k: v.double() for k, v in c.t.items()}
    b, y, x = R.cells(c.heads, c.H, c.W)
    occ = c.occ().double()[..., None]
    for key, rnd in (("conv", lambda v: v), ("conv_bf16", lambda v: R.bf16_rne(v).double())):
        yd = nhwc(F.conv2d(nchw(rnd(c.t["x"].double())), rnd(c.t["w"].double()), t["bias"], padding=1))
        _close(r64[key], yd[b, y, x], key)
    w = t["w"].clone().requires_grad_(True)
    bias = t["bias"].clone().requires_grad_(True)
    nhwc(F.conv2d(nchw(t["x"]), w, bias, padding=1)).backward(t["dy"] * occ)
    _close(r64["wgrad"], w.grad, "wgrad")
    _close(r64["wgrad_bias"], bias.grad, "wgrad_bias")
    for g in (0, 1):
        sl = slice(32 * g, 32 * g + 32)
        canvas = (t["canvas"][..., sl] * occ).requires_grad_(True)
        w1 = t["w1"].clone().requires_grad_(True)
        y1 = nhwc(F.conv2d(nchw(canvas), w1, stride=2, padding=1))
        ys = nhwc(F.conv2d(nchw(canvas), t["w3"][:, sl]))
        (y1 * t["dy1"][g * c.B:(g + 1) * c.B]).sum().add((ys * t["dskip"]).sum()).backward()
        _close(r64[f"in_wgrad{g}"], w1.grad, f"in_wgrad{g}")
        _close(r64[f"pig{g}"], canvas.grad[b, y, x], f"pig{g}")


@pytest.mark.parametrize("run", SC.RUNS)
def test_restatements_equal_the_references(run):
    """the float64 rows of ref64 put through the walks give ref64's result: the faults below start from the exact computation"""
    c = SC.case(run)
    r32, r64 = SC.reference(run)
    _close(SC.conv_rows64(c, c.heads), r64["conv"], "conv rows")
    for queued in (True, False):
        _close(SC.percell64(c, SC.walk_conv(c, K, queued=queued)[0], r64["conv"], None, False), r64["conv"], "conv")
        old = R.cells(c.heads, c.H, c.W)
        dold = c.t["dold"][old[0], old[1], old[2]][:, :32].double()
        _close(SC.percell64(c, SC.walk_pig(c, K, queued=queued)[0], r64["pig0"], dold, True), dold + r64["pig0"], "pig acc")
        _close(SC.percell64(c, SC.walk_pig(c, K, queued=queued)[0], r64["pig0"], dold, False), r64["pig0"], "pig")
    ws = SC.partials64(c, SC.walk_win(c, K["SW_WIN"])[0], lambda hk: R.sparse_wgrad3x3(c.t["x"], c.t["dy"], hk)[0], (64, 64, 3, 3))
    _close(ws.sum(0), r64["wgrad"], "wgrad partials")
    ws = SC.partials64(c, SC.walk_win(c, K["SIW_WIN"])[0],
                       lambda hk: R.sparse_in_wgrad(c.t["canvas"][..., 32:], c.t["dy1"][c.B:], hk), (64, 32, 3, 3))
    _close(ws.sum(0), r64["in_wgrad1"], "in_wgrad partials")


@pytest.mark.parametrize("run", SC.RUNS)
def test_fp32_reference_error_is_finite_and_small(run):
    """the yardstick of the GPU bounds: the ref64 functions in float32 on the CPU.  Printed per case; nowhere above 1e-5, so that no bound
    of the GPU test is wider than a few times its floor"""
    r32, r64 = SC.reference(run)
    for k in r64:
        e = R.errors(r32[k], r64[k], SC.ch_dim(k))
        print(f"[sparse cases] {run} {k}: ref64 in fp32 vs float64 max {e['max']:.2e} rms {e['rms']:.2e} ch {e['ch']:.2e}")
        assert r32[k].dtype == torch.float32 and e["finite"] and e["max"] <= 1e-5 and e["rms"] <= 1e-5, (k, e)


# ---- the faults ----------------------------------------------------------------------------------------------------------------
def _over(got, key, run, floor):
    r32, r64 = SC.reference(run)
    return SC.excess(R.errors(got, r64[key], SC.ch_dim(key)), SC.bounds(floor, r32[key], r64[key], SC.ch_dim(key)))


def _dold(c):
    b, y, x = R.cells(c.heads, c.H, c.W)
    return c.t["dold"][b, y, x][:, :32].double()


def test_fault_head_dropped_at_the_wrap():
    c = SC.case("wrap")
    _, r64 = SC.reference("wrap")
    visits, st = SC.walk_conv(c, K, fault="drop_at_wrap")
    assert st["dropped"] and len(visits) == c.heads.numel() - 1
    assert _over(SC.percell64(c, visits, r64["conv"], None, False), "conv", "wrap", SC.CONV32) >= 10
    visits, st = SC.walk_pig(c, K, fault="drop_at_wrap")
    assert st["dropped"] and len(visits) == c.heads.numel() - 1
    got = SC.percell64(c, visits, r64["pig0"], _dold(c), True) - _dold(c)
    assert _over(got, "pig0", "wrap", SC.CONV32) >= 10


def test_fault_out_of_image_tap_reads_the_neighbouring_row():
    c = SC.case("border")
    assert _over(SC.conv_rows64(c, c.heads), "conv", "border", SC.CONV32) <= 1e-3
    assert _over(SC.conv_rows64(c, c.heads, fault="oob_tap"), "conv", "border", SC.CONV32) >= 10


def test_fault_duplicate_run_processed_twice():
    c = SC.case("runs")
    _, r64 = SC.reference("runs")
    got = SC.percell64(c, SC.walk_pig(c, K)[0], r64["pig0"], _dold(c), True, fault="twice") - _dold(c)
    assert _over(got, "pig0", "runs", SC.CONV32) >= 10


def test_fault_accumulate_ignored():
    c = SC.case("views")
    _, r64 = SC.reference("views")
    for g in (0, 1):
        b, y, x = R.cells(c.heads, c.H, c.W)
        old = c.t["dold"][b, y, x][:, 32 * g:32 * g + 32].double()
        got = SC.percell64(c, SC.walk_pig(c, K)[0], r64[f"pig{g}"], old, False, fault="ignore_accumulate")
        assert _over(got, f"pig{g}", "views", SC.CONV32) >= 10


def test_fault_idle_partial_left_unwritten():
    c = SC.case("idle")
    fn = lambda hk: R.sparse_wgrad3x3(c.t["x"], c.t["dy"], hk)[0]        # noqa: E731
    good = SC.partials64(c, SC.walk_win(c, K["SW_WIN"])[0], fn, (64, 64, 3, 3)).sum(0)
    bad = SC.partials64(c, SC.walk_win(c, K["SW_WIN"])[0], fn, (64, 64, 3, 3), fault="idle_unwritten").sum(0)
    assert _over(good, "wgrad", "idle", SC.CONV32) <= 1e-3
    assert _over(bad, "wgrad", "idle", SC.CONV32) >= 10 and _over(bad, "wgrad", "idle", SC.X2) >= 10
    fn = lambda hk: R.sparse_in_wgrad(c.t["canvas"][..., :32], c.t["dy1"][:c.B], hk)        # noqa: E731
    bad = SC.partials64(c, SC.walk_win(c, K["SIW_WIN"])[0], fn, (64, 32, 3, 3), fault="idle_unwritten").sum(0)
    assert _over(bad, "in_wgrad0", "idle", SC.CONV32) >= 10
