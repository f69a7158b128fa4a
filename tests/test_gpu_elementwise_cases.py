"""GPU: the elementwise family of csrc/elementwise.hip -- BatchNorm + GELU apply and backward, the two BatchNorm finalisations, the
bilinear x2 and its backward, the column sums -- kernel by kernel against the float64 restatements of tests/helpers/ref64.py, at
the shapes where these kernels take another path: h*w, w, h and C/4 (C/8) that are no powers of two (df_udiv's real-division
branch; the model tests and the census' runs A - C only ever take the shift), single rows and columns, totals past the 4096-block
grid cap (the grid-stride loop, and the second unrolled element group of bn_gelu_apply8_kernel both real and clamped), statistic
groups, one- and two-stage reductions with uneven splits, channel slices of wider buffers, every storage type.

Bounds are the layer census' (tests/test_gpu_layer_census.py): ELEM, BNBWD, STATS, BIAS32, the one-ulp rule for bf16-stored outputs,
|dbias| <= 1e-6 sum |dy| under batch statistics; pre-split outputs against the fp32 form of the same kernel by the 2^-21 x bound
rule of tests/test_gpu_h2p.py.  Every output written into a view has the rest of its buffer compared bit-exact with a sentinel.
The four-channel forms (DF_UP8=0, DF_BN_X8=0) are recomputed in one child process and must equal the default forms to the bit.
"""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import elementwise_cases as EC  # noqa: E402
import parity  # noqa: E402
import ref64 as R  # noqa: E402
from test_gpu_layer_census import BF16_FLOOR, BIAS32, BNBWD, DBIAS_SHADOW, ELEM, STATS  # noqa: E402

pytestmark = pytest.mark.gpu
H2_REL = 2.0 ** -21         # a pre-split value against the fp32 one: 22 significant bits of the bound's scale (test_gpu_h2p.py)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the elementwise case tests need an MI355X"
    from deflow_amd import _lib
    _lib.load()
    return torch.device("cuda")


def _within(tag, what, got, ref, bounds):
    e = R.errors(got, ref)
    ok = bounds.ok(e)
    parity.record("elementwise_" + tag, what, max=e["max"], rms=e["rms"], ch=e["ch"], bound_max=bounds.max, ok=ok)
    print(f"[elementwise] {tag} {what}: max {e['max']:.2e} rms {e['rms']:.2e} ch {e['ch']:.2e} (bounds {bounds.max:.0e} / {bounds.rms:.0e} / {bounds.ch:.0e})")
    assert ok, f"{tag} {what}: {e} vs {bounds}"


def _one_ulp(tag, what, got, ref):
    ex = R.bf16_excess(got, ref, BF16_FLOOR)
    parity.record("elementwise_" + tag, what + " [bf16 ulps]", ulps=ex, bound_ulps=1.0, ok=ex <= 1.0)
    print(f"[elementwise] {tag} {what}: {ex:.3f} bf16 ulps (bound 1)")
    assert ex <= 1.0, f"{tag} {what}: {ex} ulps"


def _untouched(buf, lo, hi, what):
    """channels outside [lo, hi) of a buffer that was filled with the sentinel hold it to the bit"""
    h2 = getattr(buf, "_df_h2", None) is not None      # (a pre-split pixel keeps channel chunk k in floats [32 k, 32 k + 32) of its row)
    raw, want = (buf.view(torch.int32), EC.SENTINEL_BITS) if h2 else (buf, EC.SENTINEL)
    rest = torch.cat([raw[..., :lo], raw[..., hi:]], -1)
    assert bool((rest == want).all()), f"{what}: the buffer outside channels [{lo}, {hi}) was written"


def _h2_values(buf):
    from deflow_amd import ops
    out = ops.h2_unpack(buf)
    torch.cuda.synchronize()
    return out


# ---- BatchNorm + GELU apply ---------------------------------------------------------------------------------------------------------
APPLY = [  # n, h, w, C, groups, storage of y and z, (buffer width, channel offset) of z
    (3, 5, 7, 4, 1, torch.float32, None),            # one four-channel group per pixel, h*w = 35
    (2, 3, 11, 12, 2, torch.float32, None),          # C/4 = 3
    (4, 6, 10, 64, 2, torch.float32, None),
    (2, 1, 1, 1024, 2, torch.float32, None),         # one pixel per image
    (4, 6, 10, 64, 2, torch.float32, (128, 64)),     # the upper channel half of a 2C-wide buffer (the skip concatenation)
    (2, 3, 11, 12, 2, torch.bfloat16, (32, 16)),     # bf16 storage, three 8-byte groups per pixel, into a view
    (3, 250, 177, 36, 3, torch.float32, None),       # n*h*w*C/4 = 1 194 750 > 4096 * 256: the capped grid loops; h*w and C/4 no powers of two
]


@pytest.mark.parametrize("n,h,w,C,groups,dt,view", APPLY, ids=[f"{a[0]}x{a[1]}x{a[2]}x{a[3]}-g{a[4]}-{'bf16' if a[5] == torch.bfloat16 else 'f32'}{'-view' if a[6] else ''}" for a in APPLY])
def test_bn_gelu_apply(dev, n, h, w, C, groups, dt, view):
    from deflow_amd import ops
    from deflow_amd._lib import img
    y, _, _, bn_ss = EC.bn_inputs(n, h, w, C, groups, dev, 17 + C + w, dt)
    width, off = view or (C, 0)
    buf = torch.full((n, h, w, width), EC.SENTINEL, dtype=dt, device=dev)
    ops.bn_gelu_apply(y, bn_ss, n // groups, img(buf, C, off))
    torch.cuda.synchronize()
    ref = R.bn_gelu(y, bn_ss[:, 0], bn_ss[:, 1], groups)
    tag = f"apply_{n}x{h}x{w}x{C}_g{groups}"
    if dt == torch.bfloat16:
        _one_ulp(tag, "z", buf[..., off:off + C], ref)
    else:
        _within(tag, "z", buf[..., off:off + C], ref, ELEM)
    _untouched(buf, off, off + C, tag)


@pytest.fixture(scope="module")
def presplit(dev):
    """the pre-split apply cases of tests/helpers/elementwise_cases.py, computed once in this process (eight-channel form)"""
    return {name: EC.presplit_apply(name, dev) for name in EC.PRESPLIT_APPLY}


@pytest.mark.parametrize("name", list(EC.PRESPLIT_APPLY))
def test_bn_gelu_apply_presplit(dev, presplit, name):
    """z written as fp16 planes (bn_gelu_apply8_kernel): against the fp32 form of the same pass by the 2^-21 x bound rule, the fp32
    form against float64 within ELEM, the bound a bound"""
    from deflow_amd import ops
    from deflow_amd._lib import img
    p = presplit[name]
    y, C, off = p["y"], p["C"], p["c_off"]
    z32 = torch.empty(y.shape, device=dev)
    ops.bn_gelu_apply(y, p["bn_ss"], p["ipg"], img(z32))
    zz = _h2_values(p["buf"])[..., off:off + C]
    bound, zmax = float(p["bound"]), float(z32.abs().max())
    d = float((zz - z32).abs().max())
    parity.record("elementwise_apply_presplit_" + name, "z vs fp32 form", max_abs=d, bound=H2_REL * bound, ok=d <= H2_REL * bound)
    print(f"[elementwise] apply_presplit_{name}: |z(h2) - z(fp32)| max {d:.3e} (bound 2^-21 x {bound:.3f} = {H2_REL * bound:.3e}); bound / max|z| = {bound / zmax:.2f}")
    assert zmax <= bound <= 1024 * zmax
    assert d <= H2_REL * bound
    _within("apply_presplit_" + name, "z (fp32 form)", z32, R.bn_gelu(y, p["bn_ss"][:, 0], p["bn_ss"][:, 1], p["groups"]), ELEM)
    _untouched(p["buf"], off, off + C, name)


# ---- ops.bn_finalize ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [36, 64])
@pytest.mark.parametrize("tiles", [7, 200, 4097])       # one-stage; 3 splits of 66 / 67 / 67 tiles; 64 splits of 64 or 65 tiles
def test_bn_finalize(dev, tiles, C):
    """per-tile partials (sum, sum of squares) made by torch, three statistic groups, one channel with mean 30 and std 0.5 (its variance
    is a cancellation of two sums near 900): mean in units of the std, invstd, scale, shift and the running statistics within STATS of
    float64 sums of the same fp32 partials"""
    from deflow_amd import ops
    groups, rows = 3, 8
    g = EC.gen(dev, tiles + C)
    yt = EC.randn((groups, tiles, rows, C), g, dev) * (0.5 + torch.rand(C, generator=g, device=dev)) + EC.randn((C,), g, dev)
    yt[..., 5] = 30.0 + 0.5 * EC.randn((groups, tiles, rows), g, dev)
    partial = torch.stack([yt.sum(2), (yt * yt).sum(2)], dim=-1).reshape(groups * tiles, C, 2).contiguous()
    gamma, beta = torch.rand(C, generator=g, device=dev) + 0.5, EC.randn((C,), g, dev) * 0.3
    rm0, rv0 = EC.randn((C,), g, dev) * 0.3, torch.rand(C, generator=g, device=dev) + 0.6
    rm, rv = rm0.clone(), rv0.clone()
    count, eps, mom = tiles * rows, 1e-5, 0.1
    bn_ss = torch.full((groups, 4, C), EC.SENTINEL, device=dev)
    ops.bn_finalize(partial, tiles, groups, C, count, gamma, beta, eps, mom, rm, rv, bn_ss)
    torch.cuda.synchronize()
    s = partial.view(groups, tiles, C, 2).double().sum(1)
    mean = s[..., 0] / count
    var = (s[..., 1] / count - mean * mean).clamp_min(0.0)
    scale, shift, invstd = R.bn_fold_train(mean, var, gamma, beta, eps)
    ss = bn_ss.double()
    e_mean = float(((ss[:, 2] - mean).abs() * invstd).max())
    e_inv = float((ss[:, 3] / invstd - 1).abs().max())
    e_scale, e_shift = R.errors(ss[:, 0], scale)["max"], R.errors(ss[:, 1], shift)["max"]
    rmr, rvr = R.bn_running_update(rm0, rv0, mean, var, count, mom)
    e_rm, e_rv = R.errors(rm, rmr)["max"], R.errors(rv, rvr)["max"]
    fig = dict(mean_err_in_std=e_mean, invstd_rel_err=e_inv, scale=e_scale, shift=e_shift, running_mean=e_rm, running_var=e_rv)
    parity.record(f"elementwise_bn_finalize_t{tiles}_C{C}", "statistics", bound=STATS, ok=max(fig.values()) <= STATS, **fig)
    print(f"[elementwise] bn_finalize tiles {tiles} C {C}: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()) + f" (bound {STATS:.0e})")
    assert float(ss[:, 3, 5].min()) > 1.5       # the narrow channel: invstd about 2
    assert max(fig.values()) <= STATS, fig


# ---- ops.bn_gelu_bwd ------------------------------------------------------------------------------------------------------------
BWD = [  # n, h, w, C, groups, frozen, (y, dz, dy) storage, dz as a channel slice
    (2, 5, 7, 8, 2, False, "fff", False),           # 35 rows per group and block over 128 row lanes
    (4, 6, 10, 64, 2, False, "fff", False),         # 30 rows per block over 16 row lanes: uneven lanes, the odd tail of the two-row unroll
    (2, 3, 5, 1024, 2, False, "fff", False),        # one row lane
    (2, 9, 9, 4, 2, False, "fff", False),           # 256 row lanes, 81 rows
    (2, 5, 7, 8, 2, True, "fff", False),            # frozen statistics
    (2, 5, 7, 8, 2, False, "ffb", False),           # bf16 dy
    (4, 6, 10, 64, 2, False, "bbb", False),         # bf16 everywhere (a bf16-storage stage)
    (4, 6, 10, 64, 2, False, "fff", True),          # dz = channels [64, 128) of a 192-wide buffer
]
_DT = {"f": torch.float32, "b": torch.bfloat16}


@pytest.mark.parametrize("n,h,w,C,groups,frozen,types,sliced", BWD,
                         ids=[f"{a[0]}x{a[1]}x{a[2]}x{a[3]}-{a[6]}{'-frozen' if a[5] else ''}{'-slice' if a[7] else ''}" for a in BWD])
def test_bn_gelu_bwd(dev, n, h, w, C, groups, frozen, types, sliced):
    from deflow_amd import ops
    from deflow_amd._lib import img
    ye, ge, de = (_DT[t] for t in types)
    y, _, _, bn_ss = EC.bn_inputs(n, h, w, C, groups, dev, 31 + C + h, ye)
    g = EC.gen(dev, 5 + C)
    width, off = (3 * C, C) if sliced else (C, 0)
    dzbuf = (EC.randn((n, h, w, width), g, dev) * 1e-2).to(ge)
    dz = dzbuf[..., off:off + C]
    dy, dgamma, dbeta, dbias = ops.bn_gelu_bwd(img(dzbuf, C, off), y, bn_ss, n // groups, groups, frozen=frozen, dy_dtype=de)
    torch.cuda.synchronize()
    dy_ref, dg_ref, db_ref = R.bn_gelu_bwd(dz, y, bn_ss[:, 0], bn_ss[:, 1], bn_ss[:, 2], bn_ss[:, 3], groups, frozen)
    tag = f"bn_bwd_{n}x{h}x{w}x{C}_{types}{'_frozen' if frozen else ''}{'_slice' if sliced else ''}"
    assert dy.dtype == de and tuple(dy.shape) == (n, h, w, C)
    if de == torch.bfloat16:
        _one_ulp(tag, "dy", dy, dy_ref)
    else:
        _within(tag, "dy", dy, dy_ref, BNBWD)
    _within(tag, "dgamma", dgamma, dg_ref, BNBWD)
    _within(tag, "dbeta", dbeta, db_ref, BNBWD)
    stored = dy.double()
    if frozen:
        _within(tag, "dbias", dbias, stored.sum((0, 1, 2)), BIAS32)
    else:       # exact value 0 (the batch statistics cancel a conv bias): against sum |dy| of the stored values
        # (a bf16-stored dy is summed as stored: each value carries its own rounding, at most 2^-9 of itself, and those do not cancel)
        s_abs, gmax = float(stored.abs().sum()), float(dbias.abs().max())
        bound = DBIAS_SHADOW + (2.0 ** -9 if de == torch.bfloat16 else 0.0)
        print(f"[elementwise] {tag} dbias: max |dbias| / sum |dy| = {gmax / s_abs:.2e} (bound {bound:.1e})")
        assert gmax <= bound * s_abs
        # ... and it IS the column sum of the stored dy
        assert float((dbias.double() - stored.sum((0, 1, 2))).abs().max()) <= 2e-5 * float(stored.abs().sum((0, 1, 2)).max())


@pytest.mark.parametrize("nblk", [1, 129, 513, 640])      # one lane; the 128-stride tail; one four-deep pass + tail; one pass + two tail rounds
def test_bn_bwd_finalize(dev, nblk):
    """df_bn_bwd_finalize on synthesized per-block partials, C = 12 (two channel blocks, the second half empty), three groups: the
    group means (coef) and dgamma / dbeta against float64 sums of the same fp32 partials"""
    from deflow_amd._lib import call, ptr, stream
    groups, C, count = 3, 12, 1000 * nblk
    g = EC.gen(dev, nblk)
    partial = (EC.randn((groups, nblk, C, 2), g, dev) + 0.3).contiguous()
    dgamma, dbeta = torch.full((C,), EC.SENTINEL, device=dev), torch.full((C,), EC.SENTINEL, device=dev)
    coef = torch.full((groups, 2, C), EC.SENTINEL, device=dev)
    call("df_bn_bwd_finalize", ptr(partial), nblk, groups, C, count, ptr(dgamma), ptr(dbeta), ptr(coef), stream())
    torch.cuda.synchronize()
    s = partial.double().sum(1)          # [groups, C, 2]
    tag = f"bn_bwd_finalize_{nblk}"
    _within(tag, "coef", coef, (s / count).permute(0, 2, 1), BNBWD)
    _within(tag, "dbeta", dbeta, s[..., 0].sum(0), BNBWD)
    _within(tag, "dgamma", dgamma, s[..., 1].sum(0), BNBWD)


# ---- bilinear x2 ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bilinear(dev):
    """every bilinear case of tests/helpers/elementwise_cases.py computed once in this process: what the tests below check against
    float64 is what the four-channel child is compared with"""
    return EC.bilinear_outputs(dev)


@pytest.mark.parametrize("ac", [False, True])
@pytest.mark.parametrize("shape", EC.BILINEAR_SHAPES, ids=EC.shape_key)
def test_upsample2x_fwd_bwd(dev, shape, ac):
    x, y, dy, dx = EC.bilinear_plain(shape, ac, dev)
    tag = f"up_{EC.shape_key(shape)}_ac{int(ac)}"
    _within(tag, "upsample2x", y, R.upsample2x(x, ac), ELEM)
    _within(tag, "upsample2x_bwd", dx, R.upsample2x_bwd(dy, ac), ELEM)


@pytest.mark.parametrize("ac", [False, True])
def test_upsample2x_views_and_types(dev, ac):
    """a concatenation view whose rows are 4- but not 8-aligned (forward into it, backward from one into one), bfloat16 output into a
    view, pre-split output at C = 32 and C = 96, and the bf16 inference kernel df_upsample2x_bf16"""
    from deflow_amd import ops
    from deflow_amd._lib import call, img, stream
    x, ycat, dycat, dxcat = EC.bilinear_ld20(ac, dev)
    tag = f"up_views_ac{int(ac)}"
    _within(tag, "ld20 upsample2x", ycat[..., 12:], R.upsample2x(x, ac), ELEM)
    _untouched(ycat, 12, 20, tag + " ld20 fwd")
    _within(tag, "ld20 upsample2x_bwd", dxcat[..., 12:], R.upsample2x_bwd(dycat[..., 12:], ac), ELEM)
    _untouched(dxcat, 12, 20, tag + " ld20 bwd")
    x, y16 = EC.bilinear_bf16_out(ac, dev)
    _one_ulp(tag, "bf16 output", y16[..., 8:], R.upsample2x(x, ac))
    _untouched(y16, 8, 48, tag + " bf16 out")
    for name in EC.BILINEAR_H2:
        x, buf, off, C = EC.bilinear_h2(name, ac, dev)
        n, h, w, _ = x.shape
        y32 = torch.empty(n, 2 * h, 2 * w, C, device=dev)
        ops.upsample2x(img(x), img(y32), ac)
        got = _h2_values(buf)[..., off:off + C]
        bound = float(buf._df_h2)
        d = float((got - y32).abs().max())
        print(f"[elementwise] {tag} {name}: |y(h2) - y(fp32)| max {d:.3e} (bound 2^-21 x {bound:.3f})")
        assert d <= H2_REL * bound
        _within(tag, f"{name} (fp32 form)", y32, R.upsample2x(x, ac), ELEM)
        _untouched(buf, off, off + C, f"{tag} {name}")
    # bf16 in, bf16 out (DeFlow.inference_dtype = "bf16"): 16 channels at offset 8 of a 32-wide buffer
    xb = EC.bilinear_input((2, 5, 9, 16), dev).to(torch.bfloat16)
    yb = torch.full((2, 10, 18, 32), EC.SENTINEL, dtype=torch.bfloat16, device=dev)
    call("df_upsample2x_bf16", img(xb), img(yb, 16, 8), int(ac), stream())
    torch.cuda.synchronize()
    _one_ulp(tag, "df_upsample2x_bf16", yb[..., 8:24], R.upsample2x(xb, ac))
    _untouched(yb, 8, 24, tag + " df_upsample2x_bf16")


# ---- ops.colsum -----------------------------------------------------------------------------------------------------------------
def test_colsum_uneven_blocks_on_views(dev):
    """rows that the block count does not divide: a pair view (270 rows over 4 blocks of 68) and a channel slice (364 rows over 5
    blocks of 73)"""
    from deflow_amd import ops
    from deflow_amd._lib import img, img_pair
    g = EC.gen(dev, 3)
    t = EC.randn((3, 5, 9, 16), g, dev) + 0.2
    got = ops.colsum(img_pair(t, 8), dev)
    torch.cuda.synchronize()
    _within("colsum", "pair view", got, t.double()[..., :8].sum((0, 1, 2)) + t.double()[..., 8:].sum((0, 1, 2)), BIAS32)
    t = EC.randn((4, 7, 13, 16), g, dev) + 0.2
    got = ops.colsum(img(t, 8, 4), dev)
    torch.cuda.synchronize()
    _within("colsum", "slice view", got, t.double()[..., 4:12].sum((0, 1, 2)), BIAS32)


# ---- the four-channel forms -----------------------------------------------------------------------------------------------------
def test_four_channel_forms_are_bit_identical(dev, tmp_path, presplit, bilinear):
    """DF_UP8=0 DF_BN_X8=0 (read once per process: one fresh child): the pre-split apply cases and every bilinear case recomputed by the
    four-channel kernels equal this process' outputs to the bit"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "four_channel.pt")
    env = dict(os.environ, DF_UP8="0", DF_BN_X8="0")
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "helpers", "elementwise_cases.py"), out], cwd=root, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    four = torch.load(out)
    mine = dict(bilinear)
    mine.update({f"apply_{k}": p["buf"].view(torch.int32).cpu() for k, p in presplit.items()})
    assert set(four) == set(mine) and len(mine) > 30
    diff = [k for k in sorted(mine) if not torch.equal(four[k], mine[k])]
    assert not diff, f"the four-channel forms differ from the eight-channel ones: {diff}"
