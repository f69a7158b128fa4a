"""GPU: the sparse kernels at the UNet's two ends (csrc/pillarize.hip) against float64 at the cases of tests/helpers/sparse_cases.py, through
the C entry points: df_pillar_input_grad (the bf16x3 queue form; its fp32-MFMA fallback in `views_unaligned`), df_sparse_conv3x3 / _h2 /
_bf16, df_sparse_wgrad3x3 / _x2 and df_sparse_in_wgrad -- every case through every form.

Bounds (none taken from the code under test): max(floor, 4 x the error of the same ref64 function evaluated in float32 on the CPU), in the
three norms of ref64.errors.  Floors: CONV32 of the layer census (2e-6 / 2e-6 / 2e-5 per channel) for pillar_input_grad, sparse_in_wgrad,
sparse_conv3x3, _h2, sparse_wgrad3x3 and for _bf16 against the convolution of the bf16-rounded operands (their products are exact in
fp32: the rule of test_conv_bf16_operand_mode), the fp32 form's bias sums included; max 2e-5 / rms 1e-5 / bias 2e-6 of
test_sparse_wgrad3x3_x2_vs_float64 for _x2.  tests/test_sparse_cases_cpu.py shows that the cases reach what they were built for and that
the faults they were built for breach these bounds tenfold.

Beyond the error bound: the per-cell kernels' outputs (and, in `views`, the channels outside the slice) hold a sentinel or the old gradient
and must come back bit-unchanged wherever no cell is listed; accumulate = 0 starts from NaN at the listed cells and must give a finite
result; the weight-gradient workspaces are NaN-filled and their float64 sum must be finite; every launch runs twice and must repeat to
the bit.  Inputs a kernel has no business reading (dy, dskip and the canvas away from the listed cells, the channels outside an input
slice) hold NaN.

The last test is the guard of the packed coordinates y << 16 | x (df_sparse_wgrad3x3_x2, df_sparse_in_wgrad): a 32770 x 2 grid.

Measured on an MI355X, worst over the cases, max / rms of max |reference| (every bound sat at its floor; the references' own fp32 error
is <= 3.8e-7):
  pillar_input_grad   bf16x3 7.2e-7 / 2.7e-7 (runs, one_class)    fp32 MFMA 7.0e-7 / 2.8e-7 (views_unaligned)
  sparse_conv3x3      fp32 9.8e-7 / 4.3e-7 (one_class, wrap)      h2 3.5e-7 / 1.8e-7      bf16 4.1e-7 / 1.4e-7 (wrap)
  sparse_wgrad3x3     fp32 3.8e-7 / 3.0e-7, bias 1.3e-6           x2 6.2e-6 / 4.6e-6 (idle, wrap), bias 1.2e-6
  sparse_in_wgrad     1.6e-6 / 8.4e-7 (wrap: one fp32 chain over ~2 250 cells per tap)
  32770 x 2           sparse_wgrad3x3 4.8e-7 / 2.4e-7
`wrap` found sparse_wgrad3x3_kernel at 4.1e-6 / 1.7e-6 (one fp32 chain over the 9 000 pixels of its single workgroup); the kernel now sums
a window at a time into a second accumulator.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import parity  # noqa: E402
import ref64 as R  # noqa: E402
import sparse_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def ohwi(w):
    return w.permute(0, 2, 3, 1).contiguous()


def bits(t):
    return t.contiguous().view(torch.int32)


def buffer(t, lay, fill, dev, keep=None):
    """t [B,H,W,C] placed at channel offset `off` of a [B,H,W,width] buffer holding `fill` elsewhere; keep [B,H,W] bool: the cells of t
    that stay, the others become `fill` too"""
    width, off = lay
    buf = torch.full(t.shape[:3] + (width,), fill, dtype=torch.float32)
    buf[..., off:off + t.shape[3]] = t if keep is None else torch.where(keep[..., None], t, torch.full_like(t, fill))
    return buf.to(dev)


class Figures:
    """every figure is printed and recorded before the first assertion"""

    def __init__(self, test):
        self.test, self.bad = test, []

    def add(self, run, key, form, got, floor, ref_key=None, plus=None):
        """plus: the old value an accumulating kernel adds to (fp32): the reference is the ref64 result + plus, in float64 and in float32"""
        r32, r64 = SC.reference(run)
        rk = ref_key or key
        dim = SC.ch_dim(rk)
        a32, a64 = (r32[rk], r64[rk]) if plus is None else (r32[rk] + plus.float(), r64[rk] + plus.double())
        e, e32, b = R.errors(got, a64, dim), R.errors(a32, a64, dim), SC.bounds(floor, a32, a64, dim)
        ok = b.ok(e)
        print(f"[parity] sparse case {run} {form} {key}: vs fp64 max {e['max']:.2e} rms {e['rms']:.2e} ch {e['ch']:.2e} | ref64 in fp32 max "
              f"{e32['max']:.2e} rms {e32['rms']:.2e} ch {e32['ch']:.2e} | bounds {b.max:.1e} / {b.rms:.1e} / {b.ch:.1e}")
        parity.record(self.test, f"{run} {form} {key}", err_hip_vs_fp64=e["max"], rms_hip=e["rms"], ch_hip=e["ch"], err_ref32_vs_fp64=e32["max"],
                      rms_ref32=e32["rms"], bound=b.max, rms_bound=b.rms, ch_bound=b.ch, ok=ok)
        if not ok:
            self.bad.append((run, form, key, {k: e[k] for k in ("max", "rms", "ch")}, b))

    def note(self, cond, msg):
        if not cond:
            self.bad.append(msg)

    def done(self):
        assert not self.bad, self.bad


def _gpu_keys(c, dev):
    return c.keys.to(dev), c.counts.to(dev)


def _listed(c):
    """(occ [B,H,W] bool, (b, y, x) of the listed cells in the references' row order)"""
    return c.occ(), R.cells(c.heads, c.H, c.W)


# ------------------------------------------------------------------------------------------------------------ pillar_input_grad ----
@pytest.mark.parametrize("run", SC.RUNS)
def test_pillar_input_grad_case(dev, run):
    """both clouds, accumulate = 1 and 0; the default form everywhere except `views_unaligned` (skip-gradient rows of 264 bytes: the entry
    point takes the fp32-MFMA form)"""
    from deflow_amd._lib import call, img, ptr, stream
    assert os.environ.get("DF_PIG_X3") is None, "DF_PIG_X3 is set: the entry point would not choose the form by alignment"
    c = SC.case(run)
    lay, t = c.layout, c.t
    occ, (b, y, x) = _listed(c)
    keys, counts = _gpu_keys(c, dev)
    dy1, w1, w3 = t["dy1"].to(dev), ohwi(t["w1"]).to(dev), t["w3"].reshape(64, 64).contiguous().to(dev)
    dskip = buffer(t["dskip"], lay["dskip"], NAN, dev, keep=occ)
    dsk = img(dskip, 64, lay["dskip"][1])
    fig = Figures("sparse_cases pillar_input_grad")
    form = "fp32" if (lay["dskip"][0] * 4) % 16 else "x3"
    for g in (0, 1):
        sl = slice(32 * g, 32 * g + 32)
        for acc in (1, 0):
            old = t["dold"].clone()
            if not acc:
                old[..., sl][occ] = NAN                 # accumulate = 0 must not read what is there
            outs = []
            for _ in range(2):
                dc = old.to(dev)
                call("df_pillar_input_grad", ptr(keys), ptr(counts), c.B, c.H, c.W, g, ptr(dy1), ptr(w1), dsk, ptr(w3), img(dc, 32, 32 * g),
                     acc, c.nblk, stream())
                torch.cuda.synchronize()
                outs.append(dc.cpu())
            got = outs[0]
            fig.note(torch.equal(bits(outs[0]), bits(outs[1])), f"{run} cloud {g} accumulate {acc}: the second launch differs")
            rest = torch.ones_like(got, dtype=torch.bool)
            rest[..., sl][occ] = False
            fig.note(torch.equal(bits(got[rest]), bits(old[rest])), f"{run} cloud {g} accumulate {acc}: an element outside the listed cells changed")
            rows = got[b, y, x][:, sl].double()
            fig.note(bool(torch.isfinite(rows).all()), f"{run} cloud {g} accumulate {acc}: non-finite result")
            fig.add(run, f"cloud{g} acc{acc}", form, rows, SC.CONV32, ref_key=f"pig{g}", plus=t["dold"][b, y, x][:, sl] if acc else None)
    fig.done()


# ---------------------------------------------------------------------------------------------------------------- sparse conv ----
@pytest.mark.parametrize("form", ["fp32", "h2", "bf16"])
@pytest.mark.parametrize("run", SC.RUNS)
def test_sparse_conv3x3_case(dev, run, form):
    from deflow_amd._lib import call, img, ptr, stream
    c = SC.case(run)
    lay, t = c.layout, c.t
    occ, (b, y, x) = _listed(c)
    keys, counts = _gpu_keys(c, dev)
    xb = buffer(t["x"], lay["x"], NAN, dev)
    xi = img(xb, 64, lay["x"][1])
    w, bias = ohwi(t["w"]).to(dev), t["bias"].to(dev)
    if form == "h2":
        xa, wa = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
        call("df_absmax", xi, ptr(xa), stream())
        call("df_absmax", img(w.reshape(1, 1, -1, 64)), ptr(wa), stream())
        w2 = torch.empty(2 * w.numel(), dtype=torch.float16, device=dev)
        call("df_split_h2", ptr(w), ptr(wa), ptr(w2), w.numel(), stream())
    width, off = lay["y"]
    outs = []
    for _ in range(2):
        yb = torch.full((c.B, c.H, c.W, width), SC.SENTINEL, device=dev)
        yi = img(yb, 64, off)
        if form == "fp32":
            call("df_sparse_conv3x3", ptr(keys), ptr(counts), c.B, xi, ptr(w), ptr(bias), yi, c.nblk, stream())
        elif form == "h2":
            call("df_sparse_conv3x3_h2", ptr(keys), ptr(counts), c.B, xi, ptr(w2), ptr(xa), ptr(wa), ptr(bias), yi, c.nblk, stream())
        else:
            call("df_sparse_conv3x3_bf16", ptr(keys), ptr(counts), c.B, xi, ptr(w), ptr(bias), yi, c.nblk, stream())
        torch.cuda.synchronize()
        outs.append(yb.cpu())
    got = outs[0]
    fig = Figures("sparse_cases sparse_conv3x3")
    fig.note(torch.equal(bits(outs[0]), bits(outs[1])), f"{run} {form}: the second launch differs")
    rest = torch.ones_like(got, dtype=torch.bool)
    rest[..., off:off + 64][occ] = False
    fig.note(bool((got[rest] == SC.SENTINEL).all()), f"{run} {form}: an element outside the listed cells was written")
    fig.add(run, "y", form, got[b, y, x][:, off:off + 64], SC.CONV32, ref_key="conv_bf16" if form == "bf16" else "conv")
    fig.done()


# --------------------------------------------------------------------------------------------------------------- sparse wgrad ----
@pytest.mark.parametrize("form", ["fp32", "x2"])
@pytest.mark.parametrize("run", SC.RUNS)
def test_sparse_wgrad3x3_case(dev, run, form):
    from deflow_amd._lib import call, img, ptr, stream
    c = SC.case(run)
    lay, t = c.layout, c.t
    occ, _ = _listed(c)
    keys, counts = _gpu_keys(c, dev)
    xb = buffer(t["x"], lay["x"], NAN, dev)
    dyb = buffer(t["dy"], lay["dy"], NAN, dev, keep=occ)
    name = "df_sparse_wgrad3x3" + ("_x2" if form == "x2" else "")
    outs = []
    for _ in range(2):
        ws = torch.full((c.nblk * c.B, 64 * 9 * 64), NAN, device=dev)
        bws = torch.full((c.nblk * c.B, 64), NAN, device=dev)
        call(name, ptr(keys), ptr(counts), c.B, img(xb, 64, lay["x"][1]), img(dyb, 64, lay["dy"][1]), ptr(ws), ptr(bws), c.nblk, stream())
        torch.cuda.synchronize()
        outs.append((ws.cpu(), bws.cpu()))
    ws, bws = outs[0]
    fig = Figures("sparse_cases sparse_wgrad3x3")
    fig.note(torch.equal(bits(ws), bits(outs[1][0])) and torch.equal(bits(bws), bits(outs[1][1])), f"{run} {form}: the second launch differs")
    dw = ws.double().sum(0).view(64, 3, 3, 64).permute(0, 3, 1, 2)          # [O,kh,kw,I] partials -> logical [O,I,kh,kw]
    db = bws.double().sum(0)
    fig.note(bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), f"{run} {form}: a partial row was left unwritten (NaN)")
    fig.add(run, "wgrad", form, dw, SC.X2 if form == "x2" else SC.CONV32)
    fig.add(run, "wgrad_bias", form, db, SC.X2_BIAS if form == "x2" else SC.CONV32)
    fig.done()


@pytest.mark.parametrize("run", SC.RUNS)
def test_sparse_in_wgrad_case(dev, run):
    from deflow_amd._lib import call, img, ptr, stream
    c = SC.case(run)
    lay, t = c.layout, c.t
    occ, _ = _listed(c)
    keys, counts = _gpu_keys(c, dev)
    cv = buffer(t["canvas"], lay["canvas"], NAN, dev, keep=occ)
    dy1 = t["dy1"].to(dev)
    fig = Figures("sparse_cases sparse_in_wgrad")
    for g in (0, 1):
        outs = []
        for _ in range(2):
            ws = torch.full((c.nblk * c.B, 64 * 9 * 32), NAN, device=dev)
            call("df_sparse_in_wgrad", ptr(keys), ptr(counts), c.B, c.H, c.W, g, ptr(dy1), img(cv, 32, 32 * g), ptr(ws), c.nblk, stream())
            torch.cuda.synchronize()
            outs.append(ws.cpu())
        fig.note(torch.equal(bits(outs[0]), bits(outs[1])), f"{run} cloud {g}: the second launch differs")
        dw = outs[0].double().sum(0).view(64, 3, 3, 32).permute(0, 3, 1, 2)
        fig.note(bool(torch.isfinite(dw).all()), f"{run} cloud {g}: a partial row was left unwritten (NaN)")
        fig.add(run, f"in_wgrad{g}", "fp32", dw, SC.CONV32)
    fig.done()


# ------------------------------------------------------------------------------------------------- the packed coordinates ----
def test_packed_coordinates_are_guarded(dev):
    """y << 16 | x in an int holds rows below 32768: on a 32770 x 2 grid with listed cells at rows >= 32768, df_sparse_wgrad3x3_x2 and
    df_sparse_in_wgrad refuse (DF_E_SHAPE, workspace untouched) and df_sparse_wgrad3x3, which does not pack, meets its bound"""
    from deflow_amd import _lib
    from deflow_amd._lib import img, ptr, stream
    lib = _lib.load()
    E_SHAPE = next(k for k, v in _lib._ERR.items() if v == "DF_E_SHAPE")
    H, W, nblk = 32770, 2, 3
    g = torch.Generator().manual_seed(77)
    rows = torch.cat([torch.randperm(32768, generator=g)[:600], torch.tensor([32768, 32769])])
    cells = torch.cat([rows * W, rows[-300:] * W + 1, torch.tensor([32767 * W + 1, 32768 * W, 32768 * W])])      # incl. duplicates
    keys = torch.sort(cells)[0].to(torch.int32)
    heads = torch.unique_consecutive(keys.long())
    assert int((heads // W >= 32768).sum()) == 4
    counts = torch.tensor([keys.numel()], dtype=torch.int32)
    x, dy = torch.randn(1, H, W, 64, generator=g), torch.randn(1, H, W, 64, generator=g)
    canvas, dy1 = torch.randn(1, H, W, 64, generator=g), torch.randn(2, H // 2, W // 2, 64, generator=g)
    kd, cd, xd, dyd, cvd, dy1d = (v.to(dev) for v in (keys, counts, x, dy, canvas, dy1))
    ws = torch.full((nblk, 64 * 9 * 64), SC.SENTINEL, device=dev)
    bws = torch.full((nblk, 64), SC.SENTINEL, device=dev)
    rc = lib.df_sparse_wgrad3x3_x2(ptr(kd), ptr(cd), 1, img(xd), img(dyd), ptr(ws), ptr(bws), nblk, stream())
    rc1 = lib.df_sparse_in_wgrad(ptr(kd), ptr(cd), 1, H, W, 0, ptr(dy1d), img(cvd, 32, 0), ptr(ws), nblk, stream())
    torch.cuda.synchronize()
    assert rc == E_SHAPE and rc1 == E_SHAPE, (rc, rc1, E_SHAPE)
    assert bool((ws == SC.SENTINEL).all()) and bool((bws == SC.SENTINEL).all()), "a refused call wrote its workspace"
    ws.fill_(NAN)
    bws.fill_(NAN)
    _lib.call("df_sparse_wgrad3x3", ptr(kd), ptr(cd), 1, img(xd), img(dyd), ptr(ws), ptr(bws), nblk, stream())
    torch.cuda.synchronize()
    dw = ws.double().sum(0).view(64, 3, 3, 64).permute(0, 3, 1, 2).cpu()
    r64, r32 = R.sparse_wgrad3x3(x, dy, heads), R.sparse_wgrad3x3(x, dy, heads, dtype=torch.float32)
    fails = []
    for key, got, a, b64, floor, dim in (("wgrad", dw, r32[0], r64[0], SC.CONV32, 0), ("wgrad_bias", bws.double().sum(0).cpu(), r32[1], r64[1], SC.CONV32, -1)):
        e, bnd = R.errors(got, b64, dim), SC.bounds(floor, a, b64, dim)
        print(f"[parity] sparse case 32770x2 fp32 {key}: vs fp64 max {e['max']:.2e} rms {e['rms']:.2e} ch {e['ch']:.2e} | bounds {bnd.max:.1e} / {bnd.rms:.1e} / {bnd.ch:.1e}")
        parity.record("sparse_cases packed coordinates", key, err_hip_vs_fp64=e["max"], rms_hip=e["rms"], bound=bnd.max, rms_bound=bnd.rms, ok=bnd.ok(e))
        if not bnd.ok(e):
            fails.append((key, e, bnd))
    assert not fails, fails
