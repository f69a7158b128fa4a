"""GPU: the dense convolution kernels (csrc/conv.hip, conv_common.h, conv_wgrad.hip) against float64 at the cases of
tests/helpers/conv_cases.py, through the C entry points -- every case through every form the library offers for it: forward and data
gradient (df_conv2d_mp with fp32 and bf16 operands, _amax, _h2f, _h2f_wp, _x3, _h2, _w16, _yh2, and a bf16 output), weight gradient
(df_conv2d_wgrad_mp, _x3, _h2, df_conv2d_wgrad1_h2, df_conv2d_wgrad_s2_h2, df_conv2d_wgrad_bf16, each ending in df_conv2d_wgrad_reduce /
_reduce_bias), and the two reductions on a workspace of known content.

Bounds (none taken from the code under test): max(floor, 4 x the error of the same ref64 function evaluated in float32 on the CPU), in the
three norms of ref64.errors.  Floors: CONV32 of the layer census (2e-6 / 2e-6 / 2e-5 per channel) for every fp32-tensor form, for the
bf16-operand forms against the reference on bf16-rounded operands (the rule of test_conv_bf16_operand_mode), and for the pre-split output
after df_h2_unpack; BIAS32 (1e-5) for the bias sums; one bf16 ulp above BF16_FLOOR for the bf16-stored output; 2e-5 per statistics table.
The reductions: the weights within 4 x the error of the same sum as one sequential float32 chain, the bias within one fp32 ulp of the
float64 sum.  tests/test_conv_cases_cpu.py shows that the cases reach what they were built for and that the faults they were built for
breach these bounds tenfold.

Beyond the error bound: every output buffer is a sentinel with at least one 128-row tile of guard rows before its first and after its last
image row (and, in `views`, around the channel slice); the written elements start from NaN, or from seeded old values where the launch
accumulates; everything else must come back bit-unchanged.  Inputs are surrounded by NaN.  Split-K and bias workspaces are NaN-filled and
must be finite afterwards -- also where the split count leaves a trailing split without chunks.  Every launch runs twice and must repeat to
the bit.  *y_amax (from zero) must equal max |y| of the stored result exactly.  Every row of a statistics table is checked, the zero rows
of the 256-pixel tiles too.  A refused call returns its documented code and leaves the output untouched.

Measured on an MI355X, worst over the cases, max / rms of max |reference| (case); every bound sat at its floor -- the references' own
fp32 error is <= 3.0e-7 (convolutions) and <= 5.2e-7 (weight gradients) -- and the sequential-chain bound of conv_cases.chain32 was not needed:
  forward / data gradient   mp, amax, h2f, h2fwp 1.6e-6 / 6.0e-7 (halo_odd 128 -> 128: 1152 fp32 terms per element; tail128)
                            x3 1.4e-6 / 5.2e-7    h2 5.5e-7 / 2.3e-7    mpbf16 5.5e-7 / 2.0e-7    w16 5.9e-7 / 2.0e-7 (halo_odd)
                            yh2 after df_h2_unpack 1.4e-6 / 6.0e-7 (tail128)    ybf16 0.51 bf16 ulp    statistics per tile 5.1e-7
  weight gradient           mp 9.9e-7 / 6.0e-7 (w_two_seg), bias 4.2e-7    mpbf16 4.8e-7 / 1.9e-7    x3 5.5e-7 / 2.6e-7    h2 2.5e-7 / 1.4e-7
                            w1h2 2.3e-7 / 1.3e-7    w1bf16 2.2e-7 / 7.0e-8    s2h2 2.5e-7 / 1.5e-7    s2bf16 2.3e-7 / 9.4e-8    bf16 2.2e-7 / 9.4e-8
  reductions                1.3e-7 / 8.5e-8 (never above the sequential chain's own error); bias 0.5 ulp
Every kernel family zero-fills the workspace of a split without chunks.  `s2_odd`, `s2_even_ragged` and `views` found conv_kernel (the
register-staged kernel the generic stride-2 data gradient runs on) ignoring mfma_bf16: 1.9e-3 - 2.2e-3 from the reference on bf16-rounded
operands, i.e. fp32 products; it now rounds both operands on their way into LDS (<= 1.9e-7 at the same cases).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import conv_cases as CC  # noqa: E402
import parity  # noqa: E402
import ref64 as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Buf:
    """a tensor placed in a flat buffer through a conv_cases.Lay: `fill` everywhere else (guards, gaps, channels outside the slice)"""

    def __init__(self, shape, lay, fill, dtype=torch.float32):
        self.shape, self.lay, self.dtype = shape, lay, dtype
        self.idx = CC.index(lay, shape)
        self.host = torch.full((lay.total,), fill, dtype=dtype)
        self.rest = torch.ones(lay.total, dtype=torch.bool)
        self.rest[self.idx.reshape(-1)] = False

    def put(self, t):
        self.host[self.idx] = t.to(self.dtype)
        return self

    def upload(self, dev):
        self.dev = self.host.to(dev)
        return self

    def desc(self, elt=None):
        from deflow_amd._lib import DfImg
        n, h, w, c = self.shape
        lay = self.lay
        e = (1 if self.dtype == torch.bfloat16 else 0) if elt is None else elt
        return DfImg(self.dev.data_ptr() + self.dev.element_size() * (lay.lead + lay.off), n, h, w, c, lay.ld, lay.grp_size, lay.img_stride,
                     lay.grp_off, e, 0)

    def read(self):
        """-> (the tensor, did everything around it stay bit-unchanged)"""
        back = self.dev.cpu()
        return back[self.idx], torch.equal(bits(back[self.rest]), bits(self.host[self.rest])), back


class Figures:
    """every figure is printed and recorded before the first assertion"""

    def __init__(self, test):
        self.test, self.bad = test, []

    def add(self, name, got, r32, r64, floor, dim=-1):
        e, e32, b = R.errors(got, r64, dim), R.errors(r32, r64, dim), CC.bounds(floor, r32, r64, dim)
        ok = b.ok(e)
        print(f"[parity] conv case {name}: vs fp64 max {e['max']:.2e} rms {e['rms']:.2e} ch {e['ch']:.2e} | ref64 in fp32 max {e32['max']:.2e} "
              f"rms {e32['rms']:.2e} ch {e32['ch']:.2e} | bounds {b.max:.1e} / {b.rms:.1e} / {b.ch:.1e}")
        parity.record(self.test, name, err_hip_vs_fp64=e["max"], rms_hip=e["rms"], ch_hip=e["ch"], err_ref32_vs_fp64=e32["max"],
                      rms_ref32=e32["rms"], bound=b.max, rms_bound=b.rms, ch_bound=b.ch, ok=ok)
        if not ok:
            self.bad.append((name, {k: e[k] for k in ("max", "rms", "ch")}, b))

    def scalar(self, name, value, bound):
        ok = value <= bound
        print(f"[parity] conv case {name}: {value:.2e} (bound {bound:.1e})")
        parity.record(self.test, name, value=value, bound=bound, ok=ok)
        if not ok:
            self.bad.append((name, value, bound))

    def note(self, cond, msg):
        if not cond:
            self.bad.append(msg)

    def done(self):
        assert not self.bad, self.bad


def _absmax(d, dev):
    from deflow_amd._lib import call, ptr, stream
    a = torch.zeros(1, device=dev)
    call("df_absmax", d, ptr(a), stream())
    return a


def _flat_img(t):
    """[rows, c] device tensor as a one-image df_img (df_absmax of a weight tensor)"""
    from deflow_amd._lib import img
    return img(t.reshape(1, 1, -1, t.shape[-1]))


# ------------------------------------------------------------------------------------------------ forward / data gradient ----
def _operands(p, form, dev):
    """what both launches of a problem share: the input in its NaN-surrounded buffer, the weights in the form's format, the bounds"""
    from deflow_amd._lib import call, ptr, stream
    t = CC.tensors(p)
    o = dict(xb=Buf(p.in_shape, CC.layout(p.in_shape, p.grp, p.views, "x"), NAN).put(t["x"]).upload(dev), w=CC.kernel_weights(p).to(dev),
             bias=None if t["bias"] is None else t["bias"].to(dev), scale=t["scale"].to(dev), shift=t["shift"].to(dev))
    o["x"] = o["xb"].desc()
    w = o["w"]
    if form in ("h2f", "h2fwp", "h2"):
        o["xa"], o["wa"] = _absmax(o["x"], dev), _absmax(_flat_img(w), dev)
    if form in ("h2fwp", "h2"):
        o["w2"] = torch.empty(2 * w.numel(), dtype=torch.float16, device=dev)
        call("df_split_h2", ptr(w), ptr(o["wa"]), ptr(o["w2"]), w.numel(), stream())
    if form == "x3":
        o["w3"] = torch.empty(3 * w.numel(), dtype=torch.bfloat16, device=dev)
        call("df_split_bf16x3", ptr(w), ptr(o["w3"]), w.numel(), stream())
    if form == "w16":
        o["w16"] = torch.empty(w.numel(), dtype=torch.bfloat16, device=dev)
        call("df_cast_bf16", ptr(w), ptr(o["w16"]), w.numel() // w.shape[-1], w.shape[-1], w.shape[-1], w.shape[-1], stream())
    return o


def _launch(p, form, o, y, stats, amax, ybound):
    """one call of the form's entry point -> its return code"""
    from deflow_amd import _lib
    from deflow_amd._lib import ptr, stream
    lib = _lib.load()
    mode = CC.FWD if p.mode == "fwd" else CC.DGRAD
    tail = (p.k, p.stride, p.k // 2, mode, CC.EPI[p.epi], ptr(o["scale"]), ptr(o["shift"]), ptr(stats), int(p.acc))
    x, w, b = o["x"], ptr(o["w"]), ptr(o["bias"])
    if form in ("mp", "mpbf16", "ybf16"):
        return lib.df_conv2d_mp(x, w, b, y, *tail, int(form == "mpbf16"), stream())
    if form == "amax":
        return lib.df_conv2d_amax(x, w, b, y, *tail, ptr(amax), stream())
    if form == "h2f":
        return lib.df_conv2d_h2f(x, w, ptr(o["xa"]), ptr(o["wa"]), b, y, *tail, ptr(amax), stream())
    if form == "h2fwp":
        return lib.df_conv2d_h2f_wp(x, w, ptr(o["w2"]), ptr(o["xa"]), ptr(o["wa"]), b, y, None, *tail, ptr(amax), stream())
    if form == "x3":
        return lib.df_conv2d_x3(x, ptr(o["w3"]), b, y, *tail, stream())
    if form == "h2":
        return lib.df_conv2d_h2(x, ptr(o["w2"]), ptr(o["xa"]), ptr(o["wa"]), b, y, *tail, ptr(amax), stream())
    if form == "w16":
        return lib.df_conv2d_w16(x, ptr(o["w16"]), b, y, *tail, stream())
    if form == "yh2":
        return lib.df_conv2d_yh2(x, w, None, None, b, y, ptr(ybound), *tail, stream())
    raise KeyError(form)


def _offered(p, form, o, y):
    """the conditional forms: what the library's own query answers for these descriptors"""
    from deflow_amd._lib import call
    mode = CC.FWD if p.mode == "fwd" else CC.DGRAD
    if form in ("x3", "h2"):
        return call("df_conv2d_x3_ok", o["x"], y, p.k, p.stride, mode, CC.EPI[p.epi]) == 1
    if form == "w16":
        return call("df_conv2d_w16_ok", o["x"], y, p.k, p.stride, mode, CC.EPI[p.epi]) == 1
    return True


CASE_FORMS = [(c, f) for c in CC.NAMES for f in CC.forms(c)]


@pytest.mark.parametrize("case,form", CASE_FORMS, ids=[f"{c}-{f}" for c, f in CASE_FORMS])
def test_conv_case(dev, case, form):
    from deflow_amd._lib import call, img, ptr, stream
    fig = Figures("conv_cases " + case)
    for p in CC.PROBS[case]:
        name = f"{p.pid} {form}"
        t = CC.tensors(p)
        o = _operands(p, form, dev)
        ydt = torch.bfloat16 if form == "ybf16" else torch.float32
        ylay = CC.layout(p.out_shape, p.grp, p.views, "y")
        old = t["old"].to(ydt).float() if p.acc else None            # (a bf16 output accumulates onto bf16 values)
        key = "bf16" if form in CC.BF16_OPERAND_FORMS else "plain"
        r32, r64 = CC.reference(p)[key]
        if p.acc and form == "ybf16":
            r32, r64 = r32 - t["old"] + old, r64 - t["old"].double() + old.double()
        ybound = (r64.abs().max() * 1.5).float().reshape(1).to(dev) if form == "yh2" else None
        srows, smul = CC.stats_layout(p, form) if p.epi == "stats" else (0, 0)
        code = CC.refused(p, form)
        runs = []
        for _ in range(2):
            yb = Buf(p.out_shape, ylay, CC.SENTINEL, ydt).put(old if p.acc else torch.full(p.out_shape, NAN)).upload(dev)
            y = yb.desc(2 if form == "yh2" else None)
            if code is None and not _offered(p, form, o, y):
                code = CC.E_SHAPE
            stats = torch.full((p.M // srows * smul, p.out_shape[3], 2), NAN, device=dev) if srows else None
            amax = torch.zeros(1, device=dev) if form in ("amax", "h2f", "h2fwp", "h2") else None
            rc = _launch(p, form, o, y, stats, amax, ybound)
            torch.cuda.synchronize()
            if code is not None:
                break
            fig.note(rc == 0, f"{name}: return code {rc}")
            got, clean, whole = yb.read()
            if form == "yh2":
                yu = torch.full(p.out_shape, NAN, device=dev)
                call("df_h2_unpack", y, ptr(ybound), img(yu), stream())
                torch.cuda.synchronize()
                got = yu.cpu()
            runs.append(dict(got=got.float(), clean=clean, whole=whole, stats=None if stats is None else stats.cpu(),
                             amax=None if amax is None else float(amax)))
        if code is not None:
            fig.note(rc == code, f"{name}: return code {rc}, documented {code}")
            fig.note(torch.equal(bits(yb.dev.cpu()), bits(yb.host)), f"{name}: a refused call wrote its output")
            print(f"[parity] conv case {name}: refused with {rc}")
            continue
        a, b = runs
        fig.note(torch.equal(bits(a["whole"]), bits(b["whole"])), f"{name}: the second launch differs")
        fig.note(a["clean"], f"{name}: an element outside the written tensor changed (guard rows, gaps or channels outside the slice)")
        got = a["got"]
        fig.note(bool(torch.isfinite(got).all()), f"{name}: non-finite result")
        if form == "ybf16":
            fig.scalar(name + " bf16 ulps", R.bf16_excess(got, r64, CC.BF16_FLOOR), 1.0)
        else:
            fig.add(name, got, r32, r64, CC.CONV32)
        if a["amax"] is not None:
            fig.note(a["amax"] == float(got.abs().max()), f"{name}: *y_amax = {a['amax']!r}, max |y| = {float(got.abs().max())!r}")
            fig.note(a["amax"] == b["amax"], f"{name}: *y_amax differs in the second launch")
        if srows:
            tab, want = a["stats"].double(), CC.stats64(p, r64, form)
            fig.note(torch.equal(bits(a["stats"]), bits(b["stats"])), f"{name}: the statistics differ in the second launch")
            fig.note(bool(torch.isfinite(tab).all()), f"{name}: a statistics row was left unwritten")
            for j, what in enumerate(("sum", "sumsq")):
                e = float((tab[..., j] - want[..., j]).abs().max() / want[..., j].abs().max()) if bool(torch.isfinite(tab).all()) else float("inf")
                fig.scalar(f"{name} stats {what} per tile", e, CC.STATS_TOL)
            if smul == 2:
                fig.note(bool((tab.view(-1, 2, *tab.shape[1:])[:, 1] == 0).all()), f"{name}: the second table row of a 256-pixel tile is not zero")
    fig.done()


# ---------------------------------------------------------------------------------------------------------- weight gradient ----
def _wlaunch(p, form, x, dy, o, ws, splits, bws):
    from deflow_amd import _lib
    from deflow_amd._lib import ptr, stream
    lib = _lib.load()
    pad = p.k // 2
    if form in ("mp", "mpbf16"):
        return lib.df_conv2d_wgrad_mp(x, dy, p.k, p.stride, pad, ptr(ws), splits, ptr(o.get("counts")), p.rows_per_seg, ptr(bws),
                                      int(form == "mpbf16"), stream())
    if form == "x3":
        return lib.df_conv2d_wgrad_x3(x, dy, p.k, p.stride, pad, ptr(ws), splits, ptr(bws), stream())
    if form == "h2":
        return lib.df_conv2d_wgrad_h2(x, dy, ptr(o["xa"]), ptr(o["da"]), p.k, p.stride, pad, ptr(ws), splits, ptr(bws), stream())
    if form in ("w1h2", "w1bf16"):
        return lib.df_conv2d_wgrad1_h2(x, dy, ptr(o.get("xa")), ptr(o.get("da")), ptr(ws), splits, ptr(bws), stream())
    if form in ("s2h2", "s2bf16"):
        return lib.df_conv2d_wgrad_s2_h2(x, dy, ptr(o.get("xa")), ptr(o.get("da")), ptr(ws), splits, ptr(bws), stream())
    if form == "bf16":
        return lib.df_conv2d_wgrad_bf16(o["x16"], o["dy16"], p.k, p.stride, pad, ptr(ws), splits, ptr(bws), stream())
    raise KeyError(form)


def _w_ok(p, form, x, dy):
    from deflow_amd._lib import call
    if form in ("x3", "h2", "bf16"):
        return call("df_conv2d_wgrad_x3_ok", x, dy, p.k, p.stride) == 1
    if form.startswith("w1"):
        return call("df_conv2d_wgrad1_h2_ok", x, dy) == 1
    if form.startswith("s2"):
        return call("df_conv2d_wgrad_s2_h2_ok", x, dy) == 1
    return True


WCASE_FORMS = [(c, f) for c in CC.WNAMES for f in CC.wforms(c)]
# (ids: the case w_x3 is spelled w_3x, so that a -k "not x3" -- test_alternate_kernel_paths -- drops its x3 form and keeps its fp32-MFMA one)


@pytest.mark.parametrize("case,form", WCASE_FORMS, ids=[f"{c.replace('w_x3', 'w_3x')}-{f}" for c, f in WCASE_FORMS])
def test_conv_wgrad_case(dev, case, form):
    from deflow_amd._lib import DfImg, call, ptr, stream
    fig = Figures("conv_cases " + case)
    for p in CC.WPROBS[case]:
        if form not in CC.wforms(case, p):
            continue
        t = CC.wtensors(p)
        xs, ds = (p.n, p.h, p.w, p.cin), (p.n, p.ho, p.wo, p.cout)
        xt, dt = t["x"].clone(), t["dy"].clone()
        if p.row_counts is not None:             # pixels past a segment's count: nobody's business
            bad = ~CC.row_ok(p)
            xt[:, :, bad], dt[:, :, bad] = NAN, NAN
        xb = Buf(xs, CC.layout(xs, p.grp, p.views, "x"), NAN).put(xt).upload(dev)
        db_ = Buf(ds, CC.layout(ds, p.grp, p.views, "y"), NAN).put(dt).upload(dev)
        x, dy = xb.desc(), db_.desc()
        fig.note(_w_ok(p, form, x, dy), f"{p.pid} {form}: the form's _ok query says no")
        o = {}
        if p.row_counts is not None:
            o["counts"] = torch.tensor(p.row_counts, dtype=torch.int32, device=dev)
        if form in ("h2", "w1h2", "s2h2"):
            o["xa"], o["da"] = _absmax(x, dev), _absmax(dy, dev)
        if form == "bf16":
            x16 = torch.empty(xs, dtype=torch.bfloat16, device=dev)
            d16 = torch.empty(ds, dtype=torch.bfloat16, device=dev)
            call("df_cast_bf16", ptr(t["x"].to(dev)), ptr(x16), p.n * p.h * p.w, p.cin, p.cin, p.cin, stream())
            call("df_cast_bf16", ptr(t["dy"].to(dev)), ptr(d16), p.n * p.ho * p.wo, p.cout, p.cout, p.cout, stream())
            o["x16"] = DfImg(x16.data_ptr(), *xs, p.cin, p.n, p.h * p.w * p.cin, 0, 1, 0)
            o["dy16"] = DfImg(d16.data_ptr(), *ds, p.cout, p.n, p.ho * p.wo * p.cout, 0, 1, 0)
            o["keep"] = (x16, d16)
        one_plane = form in ("w1bf16", "s2bf16", "bf16")
        (dw32, db32), (dw64, db64) = CC.wreference(p)["bf16" if (one_plane or form == "mpbf16") else "plain"]
        if form == "mpbf16":                     # (the bias sums of the fp32-tensor kernels add dy as stored)
            db32, db64 = CC.wreference(p)["plain"][0][1], CC.wreference(p)["plain"][1][1]
        taps, row = p.k * p.k, p.k * p.k * p.cin
        ld_co, dw_off = (row + 20, 12) if p.views else (row, 0)
        guard = 128 * ld_co
        oldm = t["old"].permute(0, 2, 3, 1).reshape(p.cout, row)          # [O, taps * I] as stored
        cols = guard + dw_off + torch.arange(p.cout)[:, None] * ld_co + torch.arange(row)[None, :]
        for splits in CC.wsplits(p, form, x, dy):
            for acc in ((0, 1) if p.views else (0,)):
                for with_bias in (True, False):
                    name = f"{p.pid} {form} splits {splits} acc {acc} {'bias' if with_bias else 'nobias'}"
                    outs = []
                    for _ in range(2):
                        ws = torch.full((splits, p.cout * row), NAN, device=dev)
                        bws = torch.full((splits, p.cout), NAN, device=dev) if with_bias else None
                        rc = _wlaunch(p, form, x, dy, o, ws, splits, bws)
                        host = torch.full((2 * guard + p.cout * ld_co + 32,), CC.SENTINEL)
                        host[cols] = oldm if acc else torch.full_like(oldm, NAN)
                        dwb = host.to(dev)
                        dbv = torch.full((p.cout + 64,), CC.SENTINEL, device=dev)
                        if with_bias:
                            rc2 = call("df_conv2d_wgrad_reduce_bias", ptr(ws), splits, p.cout, taps, p.cin, dwb.data_ptr() + 4 * (guard + dw_off), ld_co,
                                       acc, ptr(bws), dbv.data_ptr() + 4 * 32, stream())
                        else:
                            rc2 = call("df_conv2d_wgrad_reduce", ptr(ws), splits, p.cout, taps, p.cin, dwb.data_ptr() + 4 * (guard + dw_off), ld_co, acc,
                                       stream())
                        torch.cuda.synchronize()
                        fig.note(rc == 0 and rc2 == 0, f"{name}: return codes {rc}, {rc2}")
                        outs.append((ws.cpu(), None if bws is None else bws.cpu(), dwb.cpu(), dbv.cpu(), host))
                    (ws, bws, dwb, dbv, host), second = outs
                    fig.note(all(torch.equal(bits(u), bits(v)) for u, v in zip(outs[0][:4], second[:4]) if u is not None), f"{name}: the second launch differs")
                    fig.note(bool(torch.isfinite(ws).all()) and (bws is None or bool(torch.isfinite(bws).all())),
                             f"{name}: a split's workspace was left unwritten (NaN)")
                    rest = torch.ones_like(host, dtype=torch.bool)
                    rest[cols.reshape(-1)] = False
                    fig.note(bool((dwb[rest] == CC.SENTINEL).all()), f"{name}: the reduction wrote between or around the rows of dw")
                    got = dwb[cols].view(p.cout, p.k, p.k, p.cin).permute(0, 3, 1, 2)
                    plus32, plus64 = (t["old"], t["old"].double()) if acc else (0.0, 0.0)
                    fig.add(name + " dw", got, dw32 + plus32, dw64 + plus64, CC.CONV32, dim=0)
                    if with_bias:
                        fig.note(bool((dbv[:32] == CC.SENTINEL).all()) and bool((dbv[32 + p.cout:] == CC.SENTINEL).all()), f"{name}: db written out of range")
                        fig.add(name + " db", dbv[32:32 + p.cout], db32, db64, CC.BIAS32)
    fig.done()


# ----------------------------------------------------------------------------------------- the reductions on their own ----
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("cout", CC.REDUCE_COUTS)
@pytest.mark.parametrize("splits", CC.REDUCE_SPLITS)
def test_conv_wgrad_reduce_alone(dev, splits, cout, acc):
    """df_conv2d_wgrad_reduce and df_conv2d_wgrad_reduce_bias on a seeded workspace: the 4-way unrolled loop's remainders, the bias part's
    k + 24 < splits and stride-8 tails, ld_co wider than a row, accumulate; 64 output channels (whole 256-thread blocks) and 65 (a ragged
    last block, a bias block with one column)"""
    from deflow_amd._lib import call, ptr, stream
    S = CC.REDUCE_SHAPE
    taps, cin, row = S["taps"], S["cin"], S["taps"] * S["cin"]
    ld_co = row + S["pad"]
    ws, bws, old = CC.reduce_case(splits, cout)
    r32, r64 = CC.reduce_refs(ws, old if acc else None)
    b64 = bws.double().sum(0)
    wsd, bwsd = ws.to(dev), bws.to(dev)
    guard = 128 * ld_co
    cols = guard + torch.arange(cout)[:, None] * ld_co + torch.arange(row)[None, :]
    host = torch.full((2 * guard + cout * ld_co,), CC.SENTINEL)
    host[cols] = old if acc else torch.full_like(old, NAN)
    rest = torch.ones_like(host, dtype=torch.bool)
    rest[cols.reshape(-1)] = False
    fig = Figures("conv_cases reduce")
    for entry in ("df_conv2d_wgrad_reduce", "df_conv2d_wgrad_reduce_bias"):
        outs = []
        for _ in range(2):
            dw = host.to(dev)
            db = torch.full((cout + 64,), CC.SENTINEL, device=dev)
            if entry.endswith("bias"):
                call(entry, ptr(wsd), splits, cout, taps, cin, dw.data_ptr() + 4 * guard, ld_co, acc, ptr(bwsd), db.data_ptr() + 4 * 32, stream())
            else:
                call(entry, ptr(wsd), splits, cout, taps, cin, dw.data_ptr() + 4 * guard, ld_co, acc, stream())
            torch.cuda.synchronize()
            outs.append((dw.cpu(), db.cpu()))
        (dw, db), (dw2, db2) = outs
        name = f"{entry} cout {cout} splits {splits} acc {acc}"
        fig.note(torch.equal(bits(dw), bits(dw2)) and torch.equal(bits(db), bits(db2)), f"{name}: the second launch differs")
        fig.note(torch.equal(bits(dw[rest]), bits(host[rest])), f"{name}: an element between the rows of dw changed")
        got = dw[cols]
        fig.note(bool(torch.isfinite(got).all()), f"{name}: non-finite result")
        e, e32 = R.errors(got, r64, 0), R.errors(r32, r64, 0)
        print(f"[parity] conv case {name}: vs fp64 max {e['max']:.2e} rms {e['rms']:.2e} | sequential fp32 chain max {e32['max']:.2e} rms {e32['rms']:.2e}")
        ok = e["finite"] and e["max"] <= 4 * e32["max"] and e["rms"] <= 4 * e32["rms"]
        parity.record("conv_cases reduce", name, err_hip_vs_fp64=e["max"], rms_hip=e["rms"], err_ref32_vs_fp64=e32["max"], rms_ref32=e32["rms"], ok=ok)
        fig.note(ok, (name, e, e32))
        if entry.endswith("bias"):
            dbg = db[32:32 + cout].double()
            ulps = float(((dbg - b64).abs() / CC.ulp32(b64)).max())
            fig.scalar(name + " db in fp32 ulps of the float64 sum", ulps, 1.0)
            fig.note(bool((db[:32] == CC.SENTINEL).all()) and bool((db[32 + cout:] == CC.SENTINEL).all()), f"{name}: db written out of range")
        else:
            fig.note(bool((db == CC.SENTINEL).all()), f"{name}: db written without being asked for")
    fig.done()
