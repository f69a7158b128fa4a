"""GPU: the layer census -- every UNet layer call of a real step, at its real shape, checked on its own right after it ran against
the float64 reference of the same operation (tests/helpers/ref64.py) on the inputs the call actually read.

The kernel tests pin each kernel form on iid operands at hand-picked shapes; the model tests compare end results against a 1e-4
floor.  In between, an error one launch makes (one tile, one image of the 2B pair images, one channel slice of a concatenation) can
hide below a parameter gradient's floor, and a model test that fails names a parameter, not the launch.  Here the seams of the
engine are intercepted (ops.conv2d / conv2d_wgrad / conv1x1_up_fused / upsample2x(_bwd) / bn_finalize / bn_gelu_apply / bn_gelu_bwd,
the sparse edge kernels' call sites in unet and autograd); each call is synchronised (the bf16 mode runs weight gradients on a side
stream), its operands are read back through the descriptors it was given (a registry of the tensors behind every _lib.img /
img_pair descriptor; pre-split tensors through df_h2_unpack), and the output is compared.  Rows carry the kernel form and layer tag
ops.KernelProfiler records.  Every df_* entry point a run invokes is seen by a recording proxy of _lib.load: it must have been
called inside a checked seam, or be on ALLOW below with the exact test that pins it.

Runs (each after two Adam steps at lr 2e-4, so that weights and BatchNorm running statistics are not at their init):
  A  configs[2] fp32 training step: B = 16, 512 x 512, 80 000 points, Trainer eagerly as bench.py steps it
  B  configs[1] forward: B = 1, 512 x 512, eval, DeFlow.forward_padded as the bench times it; + its flow against the CPU oracle
  C  bf16 training mode: Trainer(dtype="bf16"), B = 16, 256 x 256, 20 000 points (the bs16_256 shape); references on the bf16
     values the kernels read: fp32-stored outputs to fp32 summation accuracy, bf16-stored outputs within one bf16 ulp
  D  run A's body on a rectangular grid: B = 16, [H, W] = [320, 512] (range +-51.2 m in x, +-32 m in y), 50 000 points -- the smallest
     rectangular shape on which every form run A reaches is selected (tests/helpers/rect_cases.py), with h = 160 / 80 / 40 and every
     h * w no power of two: the elementwise kernels decode their indices by real division, which A, B and C never do
  E  run C's body on [H, W] = [192, 256] (range +-25.6 m in x, +-19.2 m in y), B = 16, 20 000 points: bf16-tile forms at h = 96 / 48
Each run prints its wall time; D (0.625 of A's pixels) and E (0.75 of C's) stay below A and C.
"""
import math
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ref64 as R  # noqa: E402
import rect_cases as RC  # noqa: E402

pytestmark = pytest.mark.gpu

# ---- bounds -------------------------------------------------------------------------------------------------------------------
# fp32 mode: what the kernel tests assert for the same forms (test_conv_big_tiles, test_conv_h2f_fragments, test_wgrad_*_fp32_accurate:
# 2e-6 of max |ref| for the fp16x2 / x3 convolutions and weight gradients), the same figure for the rms-relative error, and 2e-5
# per output channel (a channel holding >= 1e-3 of the tensor's norm: tests/test_ref64.py shows 1e-4 on one channel is flagged)
CONV32 = R.Bounds(max=2e-6, rms=2e-6, ch=2e-5)
BIAS32 = R.Bounds(max=1e-5, rms=1e-5, ch=math.inf)          # bias column sums
BNBWD = R.Bounds(max=2e-5, rms=2e-5, ch=2e-4)                # BatchNorm + GELU backward: dy, dgamma, dbeta
ELEM = R.Bounds(max=2e-6, rms=2e-6, ch=2e-5)                 # BatchNorm + GELU apply, bilinear x2 and its backward
STATS = 1e-5                                                 # BatchNorm mean (in units of the std) and invstd, running statistics
# bf16 mode: fp32-stored outputs of bf16 x bf16 products (exact in fp32) accumulated in fp32 are held to the same figures (summation-
# order accuracy; measured at most 5.7e-7 of max |ref|), against references on the bf16-rounded operands
BF16_FLOOR = 2.0 ** -8          # bf16-stored outputs: within one ulp of max(|ref|, 2^-8 max|ref|) (test_conv_w16_bf16_storage's rule)
SLACK_MAX = 2.0 ** 12           # pre-split bound / max|x|: the stale-scale limit of test_h2_pack_unpack_round_trip
DBIAS_SHADOW = 1e-6             # conv bias under a training BatchNorm: exact gradient 0, |dbias| <= 1e-6 sum |dy| (parity.py)

# entry points invoked outside the census' seams, each with the exact test that pins it
ALLOW = {
    # pillar stage -> tests/test_gpu_kernels.py::test_pillar_bands_vs_oracle, ::test_pillarize_backward
    **{k: "test_gpu_kernels.py::test_pillar_bands_vs_oracle, ::test_pillarize_backward" for k in (
        "df_pillar2_hist", "df_pillar2_scan", "df_pillar2_scatter", "df_pillar2_band", "df_pillar2_band_sp", "df_pfn_bn_finalize",
        "df_pfn_bn_finalize2", "df_cell_sort")},
    # the feature net's backward trio: both reductions, train / eval, the trainer's two-call accumulating form and the launch geometry
    # (tests/helpers/pfn_cases.py), against float64 at a 2e-5 floor
    **{k: "test_gpu_pfn_cases.py::test_pfn_case_vs_float64" for k in ("df_pfn_bwd_stats", "df_pfn_bwd_finalize", "df_pfn_bwd_weights")},
    # GRU trio (and the decoder's bias-sum / weight-plane helpers): one golden input (B = 3, rows 333 / 0 / 1) at 1 - 16 iterations, and
    # the cases built for the row tiles and split-K walks (tests/helpers/decoder_cases.py), lean / lean_fp32 / full forms
    # bf16 mode (runs C and E): the lean trio and the full form's forward against the float64 emulation of their own rounding points
    # (tests/helpers/decoder_bf16_ref.py); the full form's bf16 backward stays on the 2e-2 rule of test_decoder_case_bf16_operand_mode
    **{k: "test_gpu_kernels.py::test_gru_decoder_golden, test_gpu_decoder_cases.py::test_decoder_case_vs_float64" for k in (
        "df_gru_decoder_bwd_mp", "df_gru_wgrad_mp", "df_gru_head_wgrad", "df_split_bf16x2_rows")},
    **{k: "test_gpu_kernels.py::test_gru_decoder_golden, test_gpu_decoder_cases.py::test_decoder_case_vs_float64; bf16 mode: "
          "test_gpu_decoder_bf16_cases.py::test_bf16_mode_step_vs_float64, ::test_mode1_equals_mode2, ::test_wave_forms_bit_identical"
       for k in ("df_gru_xtab", "df_gru_lean_fwd", "df_gru_lean_bwd", "df_gru_lean_wgrad", "df_gru_lean_head_wgrad", "df_gru_lean_finalize")},
    "df_gru_decoder_fwd_mp": "test_gpu_kernels.py::test_gru_decoder_golden, test_gpu_decoder_cases.py::test_decoder_case_vs_float64; bf16 mode: "
                             "test_gpu_decoder_bf16_cases.py::test_bf16_mode_forward_vs_float64",
    # the split-K reduction: behind the decoder's weight gradients, and on a workspace of known content (every loop remainder, ld_co wider
    # than a row, accumulate)
    "df_conv2d_wgrad_reduce": "test_gpu_kernels.py::test_gru_decoder_golden, test_gpu_decoder_cases.py::test_decoder_case_vs_float64, "
                              "test_gpu_conv_cases.py::test_conv_wgrad_reduce_alone",
    # the column sum that ends the decoder's bias sums and the feature net's dW (the latter also with accumulate = 1)
    "df_colsum_finalize": "test_gpu_kernels.py::test_gru_decoder_golden, test_gpu_decoder_cases.py::test_decoder_case_vs_float64, "
                          "test_gpu_pfn_cases.py::test_pfn_case_vs_float64",
    # the two-stage column sum runs from B ceil(N / 64) >= 2048 only: the `blocks` case
    "df_colsum_stage": "test_gpu_decoder_cases.py::test_decoder_case_vs_float64[blocks-*]",
    # the segmented gather backward: against float64 above, and to the bit against the sequential fp32 sum (both lane forms, accumulate,
    # the measured maximum)
    **{k: "test_gpu_decoder_cases.py::test_gather_backward_forms_bit_exact, ::test_decoder_case_vs_float64" for k in (
        "df_gather_bwd", "df_gather_bwd_m")},
    # the fp32 C-ABI wrappers of the _mp entries (thin forwarders with mfma_bf16 = 0; no Python caller)
    **{k: "test_gpu_model.py::test_alternate_kernel_paths (through the _mp entry)" for k in (
        "df_gru_decoder_fwd", "df_gru_decoder_bwd", "df_gru_wgrad")},
    # the bf16 inference forward of the head (DeFlow.inference_dtype = "bf16")
    "df_gru_decoder_fwd_bf16": "test_gpu_decoder_bf16_cases.py::test_inference_kernel_vs_float64, "
                               "test_gpu_model.py::test_bf16_inference_path_vs_oracle",
    # ego-motion transform, deflowLoss through DeflowLossFn, host-step Adam at n = 4096
    **{k: "test_gpu_kernels.py::test_ego_transform_loss_adam" for k in ("df_ego_transform", "df_adam_step")},
    # the loss trios, the ground-truth gather and the device-step Adam, each against a float64 restatement
    **{k: "test_gpu_loss_optim_kernels.py::test_deflow_loss_kernels_vs_float64, test_gpu_kernels.py::test_ego_transform_loss_adam" for k in (
        "df_deflow_loss_fwd", "df_deflow_loss_finalize", "df_deflow_loss_bwd")},
    **{k: "test_gpu_loss_optim_kernels.py::test_wloss_kernels_vs_float64" for k in ("df_wloss_fwd", "df_wloss_finalize", "df_wloss_bwd")},
    "df_gather_gt": "test_gpu_loss_optim_kernels.py::test_gather_gt_exact",
    "df_adam_step_dev": "test_gpu_loss_optim_kernels.py::test_adam_step_dev_matches_host_step_form",
}
# entries outside the seams whose products every checked layer reads: the step's weight forms (transposes, fp16 planes, row L1
# norms: each convolution check runs on the fp32 weights the forms were made from) and the weight arena's max |w| (the planes' scale)
THROUGH = {"df_weight_prep": "every conv / data-gradient check (its planes and transposes are the kernels' weights)",
           "df_split_h2": "the fp16x2 conv checks (weight planes split outside a trainer step: the sparse last conv)",
           "df_absmax": "every fp16x2 conv check (the operands' scales)"}


class Census:
    """install() the seams; rows collect one dict per check; entries / seams record which df_* entry ran inside which seam"""

    def __init__(self, run: str, mp, dev):
        from deflow_amd import ops
        self.run, self.mp, self.dev, self.ops = run, mp, dev, ops
        self.rows, self.entries, self.checked_seams = [], {}, set()
        self.stack, self.recording, self.n = [], True, 0
        self.last_stats_y = None
        self.prof = None
        self.held = {}

    # ---- plumbing -------------------------------------------------------------------------------------------------------------
    def install(self):
        from deflow_amd import _lib, ops, unet, autograd
        orig_load, census = _lib.load, self

        class Proxy:
            def __getattr__(self, name):
                if census.recording and name.startswith("df_"):
                    census.entries.setdefault(name, set()).add(census.stack[-1] if census.stack else None)
                return getattr(orig_load(), name)

        proxy = Proxy()
        self.mp.setattr(_lib, "load", lambda: proxy)
        oimg, opair = _lib.img, _lib.img_pair

        def img(t, *a, **k):
            d = oimg(t, *a, **k)
            d._base = t
            return d

        def img_pair(t, c):
            d = opair(t, c)
            d._base = t
            return d

        for mod in [m for n, m in list(sys.modules.items()) if n == "deflow_amd" or n.startswith("deflow_amd.")]:
            if getattr(mod, "img", None) is oimg:
                self.mp.setattr(mod, "img", img)
            if getattr(mod, "img_pair", None) is opair:
                self.mp.setattr(mod, "img_pair", img_pair)
        self.img = img
        for name in ("conv2d", "conv2d_wgrad", "conv1x1_up_fused", "upsample2x", "upsample2x_bwd", "bn_finalize", "bn_gelu_apply",
                     "bn_gelu_bwd", "weight_transpose", "conv_out_bound", "h2_bound"):
            self.mp.setattr(ops, name, self._seam(name, getattr(ops, name), getattr(self, "_chk_" + name, None)))
        ucall = unet.call

        def unet_call(name, *a):
            seam = "sparse_fwd" if name.startswith("df_sparse_conv3x3") else "sparse_bwd" if name in (
                "df_sparse_wgrad3x3_x2", "df_sparse_wgrad3x3", "df_conv2d_wgrad_reduce_bias") else None
            if seam is None:
                return ucall(name, *a)
            self.stack.append(seam)
            try:
                return ucall(name, *a)
            finally:
                self.stack.pop()
        self.mp.setattr(unet, "call", unet_call)
        acall = autograd.call

        def autograd_call(name, *a):
            if name not in ("df_sparse_in_wgrad", "df_conv2d_wgrad_reduce", "df_pillar_input_grad"):
                return acall(name, *a)
            self.stack.append("canvas_grad")
            try:
                return acall(name, *a)
            finally:
                self.stack.pop()
        self.mp.setattr(autograd, "call", autograd_call)
        FU = unet.FastFlow3DUNet
        orun, ous, orb = FU.run, FU._upsample_skip, FU.run_backward

        def run(m, bstar, train, tape, out_cells=None):
            v = orun(m, bstar, train, tape, out_cells)
            if out_cells is not None:
                self.guarded("sparse_fwd", self._chk_sparse_fwd, m, bstar, v)
            self.held["bstar"] = bstar
            return v

        def upsample_skip(net, m, a, b, tape, train=False):
            u = ous(net, m, a, b, tape, train)
            self.held["u"] = u
            return u

        def run_backward(m, bstar, tape, dv, dbstar, grads, phase=None, sparse_input_grad=False, dv_cells=None):
            self.held.update(xu=tape[-1][2], dv=dv, m4=tape[-1][1])
            return orb(m, bstar, tape, dv, dbstar, grads, phase, sparse_input_grad, dv_cells)
        self.mp.setattr(FU, "run", run)
        self.mp.setattr(FU, "_upsample_skip", upsample_skip)
        self.mp.setattr(FU, "run_backward", run_backward)

        def tap(stage, **t):
            if stage == "head":
                torch.cuda.synchronize()
                self.held["dbstar_head"] = t["dbstar"].clone()
            elif stage == "canvas_grad":
                self.held.update(dy1=t["dy1"], dbstar_canvas=t["dbstar"], dskip=t["dskip"])
        self.mp.setattr(autograd, "TAP", tap)
        self.prof = ops.KernelProfiler()
        self.mp.setattr(ops, "PROFILER", self.prof)

    def _seam(self, name, fn, chk):
        def wrapped(*a, **k):
            torch.cuda.synchronize()
            pre = self._pre(name, a, k)
            n0 = len(self.prof.records)
            self.stack.append(name if name not in ("conv_out_bound", "h2_bound") else "bound")
            try:
                out = fn(*a, **k)
            finally:
                self.stack.pop()
            if chk is not None and not self.stack:
                torch.cuda.synchronize()
                self.recording = False
                try:
                    chk(a, k, out, pre, self.prof.records[n0:])
                except Exception as e:      # noqa: BLE001  (a check that cannot run is a failed row, and the census goes on)
                    self.row(name, "?", "", f"check raised {type(e).__name__}: {e}"[:200], ok=False)
                finally:
                    self.recording = True
                self.checked_seams.add(name)
            return out
        return wrapped

    def _pre(self, name, a, k):
        """what a check needs from BEFORE the call: the output of an accumulating convolution, the running statistics"""
        if self.stack:
            return None
        if name == "conv2d" and k.get("accumulate"):
            self.recording = False
            try:
                return self.tensor(a[3]).clone()
            finally:
                self.recording = True
        if name == "bn_finalize":
            return a[9].detach().clone(), a[10].detach().clone()
        return None

    def tensor(self, d) -> torch.Tensor:
        """the [n,h,w,c] tensor a descriptor addresses (fp32 values of a pre-split one)"""
        from deflow_amd._lib import call, ptr, stream
        if d.elt == 2:
            out = torch.empty(d.n, d.h, d.w, d.c, dtype=torch.float32, device=self.dev)
            call("df_h2_unpack", d, ptr(d._amax), self.img(out), stream())
            torch.cuda.synchronize()
            return out
        t = d._base
        off = (d.ptr - t.untyped_storage().data_ptr()) // t.element_size()
        g = d.n // d.grp_size
        v = t.as_strided((g, d.grp_size, d.h, d.w, d.c), (d.grp_off, d.img_stride, d.w * d.ld, d.ld, 1), off)
        return v.reshape(d.n, d.h, d.w, d.c)

    def guarded(self, name, fn, *a):
        try:
            fn(*a)
        except Exception as e:      # noqa: BLE001  (a check that cannot run is a failed row, and the census goes on)
            self.recording = True
            self.row(name, "?", "", f"check raised {type(e).__name__}: {e}"[:200], ok=False)

    def label(self, recs, fallback):
        if recs:
            return recs[-1][0], recs[-1][4]
        return fallback, ""

    def row(self, layer, form, tag, what, e=None, bounds=None, ok=None, **extra):
        self.n += 1
        if e is not None and ok is None:
            ok = bounds.ok(e)
        r = dict(run=self.run, i=self.n, layer=layer, form=form, tag=tag, check=what, ok=bool(ok), **extra)
        if e is not None:
            r.update(max=e["max"], rms=e["rms"], ch=e["ch"], ch_idx=e["ch_idx"])
            if bounds is not None:
                r.update(bound_max=bounds.max, bound_rms=bounds.rms, bound_ch=bounds.ch)
        self.rows.append(r)
        import parity
        parity.record(f"census_{self.run}", f"{self.n:03d} {layer} {what}", **{k: v for k, v in r.items() if k not in ("run", "layer", "check")})
        return ok

    def out_check(self, layer, form, tag, what, got_d, ref, bounds, ch_dim=-1):
        """an output as stored: fp32 -> bounds; bf16 -> the one-ulp rule; pre-split -> bounds + its scale bound"""
        got = self.tensor(got_d) if not torch.is_tensor(got_d) else got_d
        if got.dtype == torch.bfloat16:
            ex = R.bf16_excess(got, ref, BF16_FLOOR)
            e = R.errors(got, ref, ch_dim)
            self.row(layer, form, tag, what + " [bf16 ulps]", e, None, ok=ex <= 1.0, ulps=ex, bound_ulps=1.0)
        else:
            self.row(layer, form, tag, what, R.errors(got, ref, ch_dim), bounds)
        if not torch.is_tensor(got_d) and got_d.elt == 2:
            self.bound_check(layer, form, tag, what, got, got_d._amax)

    def bound_check(self, layer, form, tag, what, x, bound):
        m = float(x.abs().max())
        b = float(bound.reshape(-1)[0])
        slack = b / m if m > 0 else 1.0
        ok = bool(torch.isfinite(x).all()) and b >= m and slack <= SLACK_MAX
        self.row(layer, form, tag, what + " pre-split bound", ok=ok, bound_value=b, amax=m, slack=slack)

    def rnd(self):
        return R.bf16_rne if self.ops.MFMA_BF16 else None

    def conv_bounds(self):
        return CONV32

    # ---- checks -------------------------------------------------------------------------------------------------------------
    def _chk_conv2d(self, a, k, out, pre, recs):
        ops = self.ops
        names = ("x", "w_ohwi", "bias", "y", "ks", "stride", "mode", "epi", "scale", "shift", "stats", "accumulate")
        p = dict(zip(names, a), **k)
        p.setdefault("stride", 1); p.setdefault("mode", ops.CONV_FWD); p.setdefault("epi", ops.EPI_BIAS)
        x, w, y = self.tensor(p["x"]), p["w_ohwi"], p["y"]
        form, tag = self.label(recs, "conv2d")
        if p["mode"] == ops.CONV_FWD:
            ref = R.conv2d(x, w.permute(0, 3, 1, 2), p.get("bias"), p["stride"], self.rnd())
            if p["epi"] == ops.EPI_BN_GELU:
                ref = R.bn_gelu(ref, p["scale"], p["shift"])
            if p["epi"] == ops.EPI_STATS:
                self.last_stats_y = (p["y"], self.tensor(p["y"]))
        else:       # data gradient: x is dy, w the transposed weights wt[ci][tap][co] = w[co][tap][ci]
            ref = R.conv2d_dgrad(x, w.permute(3, 0, 1, 2), (y.h, y.w), p["stride"], self.rnd())
        if pre is not None:
            ref = ref + pre.double()
        self.out_check(tag or "conv", form, tag, "fwd" if p["mode"] == ops.CONV_FWD else "dgrad", y, ref, self.conv_bounds())

    def _chk_conv2d_wgrad(self, a, k, out, pre, recs):
        names = ("x", "dy", "ks", "stride", "dw", "ld_co", "accumulate", "row_counts", "rows_per_seg", "dw_off", "want_bias")
        p = dict(zip(names, a), **k)
        form, tag = self.label(recs, "conv2d_wgrad")
        assert p.get("ld_co") is None and not p.get("accumulate") and p.get("row_counts") is None and not p.get("dw_off"), \
            "census: a weight gradient into a strided / accumulated buffer (not covered)"
        x, dy = self.tensor(p["x"]), self.tensor(p["dy"])
        dw, db = R.conv2d_wgrad(x, dy, p["ks"], p.get("stride", 1), self.rnd())
        self.row(tag, form, tag, "wgrad", R.errors(p["dw"].permute(0, 3, 1, 2), dw, 0), self.conv_bounds())
        if out is not None:
            # the column sums of the dy the kernel read: in the bf16 mode the one-plane 1x1 form (wgrad1_h2_kernel) sums the bf16-rounded
            # dy, 2e-8 from that sum and up to 3.3e-5 from the sum of the fp32 dy in memory (recorded as max_vs_fp32_dy)
            self.row(tag, form, tag, "wgrad bias", R.errors(out, db), BIAS32, max_vs_fp32_dy=R.errors(out, R.operand(dy).sum((0, 1, 2)))["max"])

    def _chk_weight_transpose(self, a, k, out, pre, recs):
        w = a[0]
        co, kh, kw, ci = w.shape
        tag = f"weight transpose {co}x{kh}x{kw}x{ci}"
        self.row(tag, "df_weight_transpose" if self.ops.WPREP is None else "df_weight_prep", tag, "transpose (bit-exact)",
                 ok=torch.equal(out, w.permute(3, 1, 2, 0)), max=float((out - w.permute(3, 1, 2, 0)).abs().max()), bound_max=0.0)

    def _chk_conv1x1_up_fused(self, a, k, out, pre, recs):
        if not out:
            return
        xd, w, bias, yd, td, ac = a[:6]
        form, tag = self.label(recs, "conv1x1_up_fused")
        cat = self.ops.h2_unpack(yd._base)
        torch.cuda.synchronize()
        lat = yd.c
        self.row(tag, form, tag, "fwd 1x1 half", R.errors(cat[..., lat:], R.conv2d(self.tensor(xd), w.permute(0, 3, 1, 2), bias)), CONV32)
        self.row(tag, form, tag, "bilinear half", R.errors(cat[..., :lat], R.upsample2x(self.tensor(td), ac)), ELEM)
        self.bound_check(tag, form, tag, "concatenation", cat, yd._base._df_h2)

    def _chk_upsample2x(self, a, k, out, pre, recs):
        xd, yd, ac = a[:3]
        tag = f"bilinear x2 {xd.c} ch @{yd.h}x{yd.w} x{yd.n} ac={int(ac)}"
        self.out_check(tag, "df_upsample2x" + ("_h2" if yd.elt == 2 else ""), tag, "upsample2x", yd, R.upsample2x(self.tensor(xd), ac), ELEM)

    def _chk_upsample2x_bwd(self, a, k, out, pre, recs):
        dyd, dxd, ac = a[:3]
        tag = f"bilinear x2 bwd {dxd.c} ch @{dyd.h}x{dyd.w} x{dyd.n} ac={int(ac)}"
        self.out_check(tag, "df_upsample2x_bwd", tag, "upsample2x_bwd", dxd, R.upsample2x_bwd(self.tensor(dyd), ac), ELEM)

    def _chk_bn_finalize(self, a, k, out, pre, recs):
        partial, tiles_pg, groups, C, count, gamma, beta, eps, momentum, rmean, rvar, bn_ss = a[:12]
        yd, y = self.last_stats_y
        tag = f"bn stats {C} ch @{yd.h}x{yd.w} x{yd.n} groups={groups}"
        mean, var = R.bn_stats(y, groups)
        ss = bn_ss.view(groups, 4, C).double()
        inv_ref = torch.rsqrt(var + eps)
        e_mean = float(((ss[:, 2] - mean).abs() * inv_ref).max())
        e_inv = float((ss[:, 3] / inv_ref - 1).abs().max())
        self.row(tag, "df_bn_finalize2", tag, "mean / invstd", ok=e_mean <= STATS and e_inv <= STATS, max=max(e_mean, e_inv),
                 mean_err_in_std=e_mean, invstd_rel_err=e_inv, bound_max=STATS)
        if rmean is not None:
            rm, rv = R.bn_running_update(pre[0], pre[1], mean, var, count, momentum)
            em, ev = R.errors(rmean, rm)["max"], R.errors(rvar, rv)["max"]
            self.row(tag, "df_bn_finalize2", tag, "running stats", ok=em <= STATS and ev <= STATS, max=max(em, ev), bound_max=STATS)

    def _chk_bn_gelu_apply(self, a, k, out, pre, recs):
        y, bn_ss, ipg, zd = a[:4]
        groups = y.shape[0] // ipg
        ss = bn_ss.view(groups, 4, -1)
        tag = f"bn+gelu {y.shape[3]} ch @{zd.h}x{zd.w} x{zd.n} groups={groups}"
        self.out_check(tag, "bn_gelu_apply", tag, "z", zd, R.bn_gelu(y, ss[:, 0], ss[:, 1], groups), ELEM)

    def _chk_bn_gelu_bwd(self, a, k, out, pre, recs):
        names = ("dz", "y", "bn_ss", "imgs_per_group", "groups", "gamma_grad", "frozen")
        p = dict(zip(names, a), **k)
        dzd, y, groups, frozen = p["dz"], p["y"], p["groups"], p.get("frozen", False)
        ss = p["bn_ss"].view(groups, 4, -1)
        dy_got, dgamma, dbeta, dbias = out
        tag = f"bn+gelu bwd {y.shape[3]} ch @{dzd.h}x{dzd.w} x{dzd.n} groups={groups}"
        dy, dg, db = R.bn_gelu_bwd(self.tensor(dzd), y, ss[:, 0], ss[:, 1], ss[:, 2], ss[:, 3], groups, frozen)
        got = self.ops.h2_unpack(dy_got) if getattr(dy_got, "_df_h2", None) is not None else dy_got
        torch.cuda.synchronize()
        if got.dtype == torch.bfloat16:
            ex = R.bf16_excess(got, dy, BF16_FLOOR)
            self.row(tag, "bn_gelu_bwd", tag, "dy [bf16 ulps]", R.errors(got, dy), None, ok=ex <= 1.0, ulps=ex, bound_ulps=1.0)
        else:
            self.row(tag, "bn_gelu_bwd", tag, "dy", R.errors(got, dy), BNBWD)
        if getattr(dy_got, "_df_h2", None) is not None:
            self.bound_check(tag, "bn_gelu_bwd", tag, "dy", got, dy_got._df_h2)
        self.row(tag, "bn_gelu_bwd", tag, "dgamma", R.errors(dgamma, dg), BNBWD)
        self.row(tag, "bn_gelu_bwd", tag, "dbeta", R.errors(dbeta, db), BNBWD)
        s_abs = float(got.double().abs().sum())
        if frozen:
            self.row(tag, "bn_gelu_bwd", tag, "dbias", R.errors(dbias, got.double().sum((0, 1, 2))), BIAS32)
        else:
            g = float(dbias.abs().max())
            self.row(tag, "bn_gelu_bwd", tag, "dbias (exact 0)", ok=g <= DBIAS_SHADOW * s_abs, max=g / max(s_abs, 1e-300),
                     bound_max=DBIAS_SHADOW)

    def _chk_sparse_fwd(self, m, bstar, v):
        """the last conv evaluated at the occupied cells of cloud 0 (df_sparse_conv3x3_h2 / _bf16): the canvas' non-zero pixels"""
        torch.cuda.synchronize()
        self.recording = False
        try:
            u = self.held["u"]
            occ = (bstar[..., :32] != 0).any(-1)
            w = m.decoder_step4.weight
            ref = R.conv2d(u, w, m.decoder_step4.bias, 1, self.rnd())[occ]
            tag = f"sparse conv3x3 64->64 @{u.shape[1]}x{u.shape[2]} x{u.shape[0]} ({int(occ.sum())} cells)"
            self.row(tag, "df_sparse_conv3x3" + ("_bf16" if self.ops.MFMA_BF16 else "_h2"), tag, "fwd at cells", R.errors(v[occ], ref),
                     self.conv_bounds())
        finally:
            self.recording = True
        self.checked_seams.add("sparse_fwd")

    def check_after_backward(self, model):
        """weight gradients of the two sparse edge kernels and the canvas gradient at the occupied cells, read from the gradient arena
        once the step's backward is complete (Trainer.reduce_gradients)"""
        torch.cuda.synchronize()
        self.recording = False
        try:
            bb = model.backbone
            h = self.held
            m4 = bb.decoder_step4
            dw, db = R.conv2d_wgrad(h["xu"], h["dv"], 3, 1)       # dv is zero outside cloud 0's cells: the dense sum is the sparse one
            tag = f"sparse wgrad3x3 64->64 @{h['dv'].shape[1]}x{h['dv'].shape[2]} x{h['dv'].shape[0]}"
            self.row(tag, "df_sparse_wgrad3x3_x2", tag, "wgrad", R.errors(m4.weight.grad, dw, 0), CONV32)
            self.row(tag, "df_sparse_wgrad3x3_x2", tag, "wgrad bias", R.errors(m4.bias.grad, db), BIAS32)
            self.checked_seams.add("sparse_bwd")
            bstar, dy1 = h["bstar"], h["dy1"]
            B = bstar.shape[0]
            pair = torch.cat([bstar[..., :32], bstar[..., 32:]], 0)
            w1 = bb.encoder_step_1[0].conv.weight
            tag = f"sparse in wgrad 3x3 s2 32->64 @{dy1.shape[1]}x{dy1.shape[2]} x{dy1.shape[0]}"
            self.row(tag, "df_sparse_in_wgrad", tag, "wgrad", R.errors(w1.grad, R.conv2d_wgrad(pair, dy1, 3, 2)[0], 0), CONV32)
            w3 = bb.decoder_step3.u3.weight
            dskip = R.conv2d_dgrad(self.held["dskip"], w3, bstar.shape[1:3], 1) if "dskip" in self.held else None
            head, after = h["dbstar_head"], h["dbstar_canvas"]
            for cloud in (0, 1):
                sl = slice(32 * cloud, 32 * cloud + 32)
                occ = (bstar[..., sl] != 0).any(-1)
                ref = head[..., sl].double() + R.conv2d_dgrad(dy1[cloud * B:(cloud + 1) * B], w1, bstar.shape[1:3], 2)
                if dskip is not None:
                    ref = ref + dskip[..., sl]
                tag = f"pillar input grad cloud {cloud} @{bstar.shape[1]}x{bstar.shape[2]} x{B} ({int(occ.sum())} cells)"
                self.row(tag, "df_pillar_input_grad", tag, "d(canvas) at cells", R.errors(after[..., sl][occ], ref[occ]), CONV32)
            self.checked_seams.add("canvas_grad")
        finally:
            self.recording = True

    # ---- verdict ------------------------------------------------------------------------------------------------------------
    def coverage(self):
        """-> list of (entry, why it is not covered)"""
        from deflow_amd import _lib
        bad = []
        for name, seams in sorted(self.entries.items()):
            if name in _lib._RAW:
                continue            # shape / tile queries: nothing launched
            for s in seams:
                if s is None and (name in ALLOW or name in THROUGH):
                    continue
                if s == "bound":        # a-priori bounds of pre-split tensors: checked where each such tensor is written
                    if any("pre-split bound" in r["check"] for r in self.rows):
                        continue
                if s is not None and s != "bound" and s in self.checked_seams:
                    continue
                bad.append((name, s))
        return bad

    def report(self, wall):
        rows = self.rows
        print(f"\n[census {self.run}] {len(rows)} checks in {wall:.1f} s")
        print(f"{'#':>4s} {'ok':3s} {'check':28s} {'max':>9s} {'rms':>9s} {'ch':>9s} {'bound':>8s}  {'form':44s} layer")
        for r in rows:
            err = r.get("max", r.get("slack", 0.0))
            b = r.get("bound_max", r.get("bound_ulps", SLACK_MAX if "slack" in r else float("nan")))
            extra = f" ulps {r['ulps']:.2f}" if "ulps" in r else f" slack {r['slack']:.1f}" if "slack" in r else ""
            print(f"{r['i']:4d} {'ok' if r['ok'] else 'BAD':3s} {r['check'][:28]:28s} {err:9.2e} {r.get('rms', float('nan')):9.2e} "
                  f"{r.get('ch', float('nan')):9.2e} {b:8.1e}  {str(r['form'])[:44]:44s} {r['layer']}{extra}")
        errs = [r for r in rows if "max" in r and "[bf16" not in r["check"]]
        if errs:
            w = max(errs, key=lambda r: r["max"] / r["bound_max"] if r.get("bound_max") else 0)
            print(f"[census {self.run}] worst row (error / bound): #{w['i']} {w['check']} max {w['max']:.3e} (bound {w.get('bound_max', 0):.1e}) "
                  f"{w['form']} {w['layer']}")
        u = [r for r in rows if "ulps" in r]
        if u:
            w = max(u, key=lambda r: r["ulps"])
            print(f"[census {self.run}] worst bf16-stored row: #{w['i']} {w['check']} {w['ulps']:.2f} ulps {w['form']} {w['layer']}")


def _two_adam_steps_then(tr, batch):
    for _ in range(2):
        tr.step(batch)
    torch.cuda.synchronize()


def _census_step(run, tr, model, batch, dev):
    census = Census(run, None, dev)
    with pytest.MonkeyPatch.context() as mp:
        census.mp = mp
        census.install()
        orig = tr.reduce_gradients

        def reduce_gradients(*a, **k):
            census.guarded("after_backward", census.check_after_backward, model)
            return orig(*a, **k)
        mp.setattr(tr, "reduce_gradients", reduce_gradients)
        t0 = time.perf_counter()
        tr.step(batch)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    return census, wall


def _verdict(census, wall):
    census.report(wall)
    bad_rows = [r for r in census.rows if not r["ok"]]
    bad_cov = census.coverage()
    assert census.rows, "the census saw no layer"
    assert not bad_cov, f"entry points run outside a checked seam and not on ALLOW: {bad_cov}"
    assert not bad_rows, f"{len(bad_rows)} layer checks failed, first: " + "; ".join(
        f"#{r['i']} {r['check']} {r['form']} {r['layer']} max {r.get('max', float('nan')):.3e}" for r in bad_rows[:6])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the layer census needs an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def test_census_A_configs2_fp32_step(dev):
    """configs[2]: B = 16, 512 x 512, 80 000 points, fp32 training step through the Trainer (eager)"""
    import deflow_amd
    from deflow_amd.optim import Trainer
    from deflow_amd.synth import synth_batch
    torch.manual_seed(0)
    model = deflow_amd.DeFlow(grid_feature_size=[512, 512], num_iters=4).to(dev).train()
    tr = Trainer(model, lr=2e-4)
    batch = synth_batch(16, 80000, seed=Trainer.shard_seed(20240116, 0, 16), device=dev)
    _two_adam_steps_then(tr, batch)
    census, wall = _census_step("A", tr, model, batch, dev)
    _verdict(census, wall)


def test_census_C_bf16_training_mode(dev):
    """Trainer(dtype="bf16") at the bs16_256 shape: B = 16, 256 x 256 (0.2 m voxels), 20 000 points"""
    import deflow_amd
    from deflow_amd.optim import Trainer
    from deflow_amd.synth import synth_batch
    torch.manual_seed(4242)
    cfg = dict(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-25.6, -25.6, -3, 25.6, 25.6, 3], grid_feature_size=[256, 256])
    model = deflow_amd.DeFlow(**cfg).to(dev).train()
    tr = Trainer(model, lr=2e-4, dtype="bf16")
    batch = synth_batch(16, 20000, seed=4242, grid_hw=(256, 256), device=dev)
    _two_adam_steps_then(tr, batch)
    census, wall = _census_step("C", tr, model, batch, dev)
    _verdict(census, wall)


def test_census_B_configs1_forward_and_oracle(dev):
    """configs[1]: B = 1, 512 x 512, eval-mode DeFlow.forward_padded (BatchNorm folded into the conv epilogue); and its flow against the
    CPU oracle at 1e-4 with non-trivial BatchNorm state (two Adam steps from scattered gamma / beta / running statistics)"""
    import deflow_amd
    from oracle import ref_torch as O
    from deflow_amd.optim import Trainer
    from deflow_amd.synth import synth_batch
    torch.manual_seed(44)
    ref = O.DeFlow()
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.uniform_(0.6, 1.4); m.bias.uniform_(-0.2, 0.2)
                m.running_mean.uniform_(-0.3, 0.3); m.running_var.uniform_(0.6, 1.5)
    mine = deflow_amd.DeFlow()
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(dev).train()
    tr = Trainer(mine, lr=2e-4)
    _two_adam_steps_then(tr, synth_batch(1, 80000, seed=7, device=dev))
    mine.eval()
    b1 = synth_batch(1, 80000, seed=20240116, device=dev)
    with torch.no_grad():
        mine.forward_padded(b1)           # warm (weight planes, folded BatchNorm caches), as the bench's untimed calls
    torch.cuda.synchronize()
    census = Census("B", None, dev)
    with pytest.MonkeyPatch.context() as mp:
        census.mp = mp
        census.install()
        t0 = time.perf_counter()
        with torch.no_grad():
            mine.forward_padded(b1)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    # the flow of this forward against the CPU oracle carrying the same (trained) state
    ref.load_state_dict({k: v.detach().cpu() for k, v in mine.state_dict().items()})
    ref.eval()
    cpu = {k: v.cpu() for k, v in b1.items()}
    with torch.no_grad():
        want = ref(cpu)
        got = mine(b1)
    f_got, f_want = got["flow"][0].detach().double().cpu(), want["flow"][0].detach().double()
    assert f_got.shape == f_want.shape
    e = float((f_got - f_want).abs().max() / f_want.abs().max())
    import parity
    parity.record("census_B", "flow vs oracle", err=e, bound=1e-4, ok=e <= 1e-4)
    print(f"[census B] configs[1] eval forward flow vs CPU oracle: max err / max|flow| = {e:.3e} (bound 1e-4)")
    _verdict(census, wall)
    assert e <= 1e-4


def test_census_D_rectangular_fp32_step(dev):
    """run A's body on [320, 512]: B = 16, 50 000 points, fp32 training step through the Trainer (eager)"""
    import deflow_amd
    from deflow_amd.optim import Trainer
    from deflow_amd.synth import synth_batch
    c = RC.case("320x512")
    assert (c.grid, c.point_cloud_range, c.B, c.N) == ([320, 512], [-51.2, -32, -3, 51.2, 32, 3], 16, 50000)
    torch.manual_seed(0)
    model = deflow_amd.DeFlow(**c.cfg, num_iters=4).to(dev).train()
    tr = Trainer(model, lr=2e-4)
    batch = synth_batch(c.B, c.N, seed=Trainer.shard_seed(c.seed, 0, c.B), grid_hw=(512, 512), device=dev)
    _two_adam_steps_then(tr, batch)
    census, wall = _census_step("D", tr, model, batch, dev)
    _verdict(census, wall)
    forms = {r["form"] for r in census.rows}
    assert any(str(f).endswith(",xp>") for f in forms) and "wgrad3_h2p_kernel<4>" in forms, sorted(map(str, forms))   # the pre-split forms ran


def test_census_E_rectangular_bf16_training_mode(dev):
    """run C's body on [192, 256]: Trainer(dtype="bf16"), B = 16, 20 000 points"""
    import deflow_amd
    from deflow_amd.optim import Trainer
    from deflow_amd.synth import synth_batch
    c = RC.case("192x256")
    assert (c.grid, c.point_cloud_range, c.B, c.N) == ([192, 256], [-25.6, -19.2, -3, 25.6, 19.2, 3], 16, 20000)
    torch.manual_seed(4242)
    model = deflow_amd.DeFlow(**c.cfg).to(dev).train()
    tr = Trainer(model, lr=2e-4, dtype="bf16")
    batch = synth_batch(c.B, c.N, seed=c.seed, grid_hw=(256, 256), device=dev)
    _two_adam_steps_then(tr, batch)
    census, wall = _census_step("E", tr, model, batch, dev)
    _verdict(census, wall)
    assert any("ulps" in r for r in census.rows) and "wgrad3_tr_kernel<4>/bf16" in {r["form"] for r in census.rows}      # the bf16-tile stages ran
