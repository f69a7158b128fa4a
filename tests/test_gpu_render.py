"""GPU: the bird's-eye-view rasteriser (csrc/render.hip, deflow_amd/render.py, ``python -m deflow_amd.vis``) against the numpy restatement
in tests/helpers/render_ref.py.  Every floating-point step of the definition is one correctly rounded fp32 operation and what a pixel
shows is an integer maximum, so every comparison is exact: torch.equal on the bytes."""
import json
import os
import shutil
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import render_ref as RR  # noqa: E402
import sweep_flow_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], grid_feature_size=[64, 64])   # tests/test_gpu_save.py's
F = np.float32
B = 3
SHAPES = {"48x40": ((48, 40), (-12.0, -10.0, 2.0)),                      # lines of 1 + 3W = 145 bytes: they start at every alignment; cells of exactly 0.5
          "37x53": ((37, 53), (-5.55, -7.95, 1.0 / 0.3))}                # odd sides, lines of 112 bytes, cells whose size is no fp32 number
# (a total that is no multiple of 4 bytes, the resolve kernel's byte-wise tail: test_special_rows_show_their_colours, 3 lines of 49)
VMAX = 1.5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def same(got: torch.Tensor, want: np.ndarray, what: str):
    w = torch.from_numpy(np.ascontiguousarray(want))
    g = got.detach().cpu()
    assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, g.dtype, tuple(g.shape), w.dtype, tuple(w.shape))
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} bytes differ"


def special_rows(size, view):
    """(x, y, z, vx, vy, vz, cls): rows on all four borders and corners (a radius is clipped there), the edge, skip and colour cases of
    tests/test_render_cpu.py"""
    (W, H), (xmin, ymin, inv) = size, (F(v) for v in view)
    res = F(1) / inv
    cx = lambda i: float(xmin + (F(i) + F(0.5)) * res)               # the middle of column i / line (counted from the bottom) j
    cy = lambda j: float(ymin + (F(j) + F(0.5)) * res)
    nan, inf = float("nan"), float("inf")
    rows = []
    for i, j in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)):
        rows.append((cx(i), cy(j), 3.0 + i, 1.0, -1.0, 0.0, 1))
    rows += [(float(xmin), float(ymin), 9.0, 0.0, 1.0, 0.0, 1),                      # x == xmin, y == ymin: drawn
             (float(xmin + F(W) * res), cy(3), 9.0, 1.0, 0.0, 0.0, 1),               # one cell past the last: skipped
             (cx(3), float(ymin + F(H) * res), 9.0, 1.0, 0.0, 0.0, 1),
             (float(np.nextafter(xmin, F(-1e9))), cy(3), 9.0, 1.0, 0.0, 0.0, 1),
             (nan, cy(5), 0.0, 1.0, 0.0, 0.0, 1), (cx(5), inf, 0.0, 1.0, 0.0, 0.0, 1), (cx(5), cy(5), -inf, 1.0, 0.0, 0.0, 1),
             (cx(5), cy(5), 0.0, nan, 0.0, 0.0, 1), (cx(5), cy(5), 0.0, 0.0, 0.0, inf, 2), (cx(5), cy(5), 50.0, 1.0, 0.0, 0.0, 0),
             (3e38, -3e38, 0.0, 1.0, 0.0, 0.0, 1), (cx(6), cy(6), 0.0, 3e38, 3e38, 0.0, 1)]
    for k, (vx, vy) in enumerate([(1.5, 0.0), (0.0, 1.5), (-1.5, 0.0), (0.0, -1.5), (1.5, -0.0), (-0.0, 1.5), (-1.5, -0.0), (-0.0, -1.5),
                                  (0.0, 0.0), (-0.0, -0.0), (1e-40, 0.0), (-1e-40, 1e-40), (0.75, 0.0), (5.0, 0.0), (0.9, 1.2), (-1.0, -3.0),
                                  (1.0, -1e-30)]):
        rows.append((cx(8 + k), cy(8 + k % 7), 40.0, vx, vy, 0.25, 1))               # above everything random: these colours are seen
    # priority: coloured under a higher grey row; a higher coloured row; equal heights decided by the colour bits; -0.0 below +0.0
    rows += [(cx(2), cy(9), 41.0, 1.0, 0.0, 0.0, 1), (cx(2), cy(9), 99.0, 1.0, 0.0, 0.0, 2),
             (cx(3), cy(9), 41.0, 1.0, 0.0, 0.0, 1), (cx(3), cy(9), 42.0, -1.0, 0.0, 0.0, 1),
             (cx(4), cy(9), 41.0, -1.0, 0.0, 0.0, 1), (cx(4), cy(9), 41.0, 1.0, 0.0, 0.0, 1),
             (cx(5), cy(9), 41.0, 1.0, 0.0, 0.0, 2), (cx(5), cy(9), 43.0, 1.0, 0.0, 0.0, 200)]
    return rows


def make_case(N, size, view, seed):
    """B = 3 samples of N rows, counts (N, 0, most of N).  Half of the random rows fall into a patch of a few cells and z takes few
    values: many rows per pixel, many of equal height -- the atomic's outcome matters.  The special rows are spread over the samples'
    leading rows as far as N allows; rows behind count hold drawable garbage."""
    rng = np.random.default_rng(seed)
    (W, H), (xmin, ymin, inv) = size, view
    ext = np.array([W / inv, H / inv])
    pts = np.empty((B, N, 3), dtype=F)
    pts[..., :2] = (np.array([xmin, ymin]) + rng.uniform(-0.1, 1.1, (B, N, 2)) * ext).astype(F)
    patch = rng.random((B, N)) < 0.5
    pts[..., :2][patch] = (np.array([xmin, ymin]) + (0.45 + 0.08 * rng.random((int(patch.sum()), 2))) * ext).astype(F)
    pts[..., 2] = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 0.25, 1.0, 2.0], dtype=F), size=(B, N))
    vec = (rng.standard_normal((B, N, 3)) * 0.8).astype(F)
    vec[rng.random((B, N)) < 0.1] = 0.0
    cls = rng.choice(np.array([0, 1, 1, 1, 2, 2, 7], dtype=np.uint8), size=(B, N))
    sp = special_rows(size, view)
    for k, row in enumerate(sp[: 2 * N]):
        b, i = (0, k) if k < N else (2, k - N)
        pts[b, i], vec[b, i], cls[b, i] = row[:3], row[3:6], row[6]
    count = np.array([N, 0, max(N - 7, 1)], dtype=np.int32)
    return pts, count, vec, cls


def poison(dev, *nbytes):
    """fill blocks of the given sizes with 0x5A and hand them back to the caching allocator: the next allocations of those sizes get
    poisoned memory -- an image that is not zeroed, or an output byte that is not written, shows"""
    t = [torch.full((n,), 0x5A, dtype=torch.uint8, device=dev) for n in nbytes]
    torch.cuda.synchronize()
    del t


def entries_poisoned(dev, pts, count, vec, cls, view, size, vmax, radius, bg, legend):
    """df_render_splat / df_render_resolve through the binding on buffers of this test's own: the output 0x5A beforehand"""
    from deflow_amd._lib import call, ptr, stream
    d = lambda a: torch.from_numpy(a).to(dev)
    (W, H), Bn, N = size, pts.shape[0], pts.shape[1]
    image = torch.zeros(Bn, H, W, dtype=torch.int64, device=dev)
    out = torch.full((Bn, H, 1 + 3 * W), 0x5A, dtype=torch.uint8, device=dev)
    args = [d(a) for a in (pts, vec, cls, count)]
    call("df_render_splat", *(ptr(a) for a in args), Bn, N, view[0], view[1], view[2], W, H, vmax, radius, ptr(image), stream())
    call("df_render_resolve", ptr(image), Bn, W, H, (bg[0] << 16) | (bg[1] << 8) | bg[2], legend, ptr(out), stream())
    return out, image


# ---- the kernels against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_render_equals_the_restatement(dev, N, shape):
    from deflow_amd import render
    size, view = SHAPES[shape]
    W, H = size
    pts, count, vec, cls = make_case(N, size, view, seed=N * 7 + W)
    d = lambda a: torch.from_numpy(a).to(dev)
    args = (d(pts), d(count), d(vec), d(cls))
    bg = (24, 24, 24)
    for radius in (0, 1, 2, 4):
        imgs = [RR.splat(pts[b], vec[b], cls[b], count[b], view, size, VMAX, radius) for b in range(B)]
        if N >= 256:
            ok, px, py, _ = RR.rows(pts[0], vec[0], cls[0], count[0], view, size, VMAX)
            per_pixel = np.bincount((py[ok] * W + px[ok]))
            assert per_pixel.max() >= 4 and not imgs[1].any() and imgs[0].any()            # many rows per pixel; the empty sample is empty
        for legend in (0, 7):
            want = np.stack([RR.resolve(im, bg, legend) for im in imgs])
            poison(dev, B * H * W * 8, B * H * (1 + 3 * W))
            got = render.render_rows(*args, view=view, size=size, vmax=VMAX, radius=radius, bg=bg, legend=legend)
            again = render.render_rows(*args, view=view, size=size, vmax=VMAX, radius=radius, bg=bg, legend=legend)
            same(got, want, f"render_rows N={N} {shape} r={radius} legend={legend}")
            assert torch.equal(got, again), "a second call differs"
        out, image = entries_poisoned(dev, pts, count, vec, cls, view, size, VMAX, radius, (1, 2, 3), 0)
        same(out, np.stack([RR.resolve(im, (1, 2, 3), 0) for im in imgs]), f"entries N={N} {shape} r={radius}")
        same(image, np.stack(imgs).view(np.int64), f"image words N={N} {shape} r={radius}")
    if N == 1000:
        px = RR.pixels(want)
        print(f"[render] N = {N}, {shape}: {int((px[0] != 24).any(axis=2).sum())} of {W * H} pixels drawn in sample 0, r = 4 with legend")


def test_special_rows_show_their_colours(dev):
    """the rows of the CPU list, alone in an image: the kernel's colours are the stated bytes, not merely the restatement's"""
    from deflow_amd import render
    size, view = (16, 3), (0.0, 0.0, 1.0)
    vecs = [(2, 0), (0, 2), (-2, 0), (0, -2), (2, -0.0), (-0.0, 2), (-2, -0.0), (-0.0, -2), (0, 0), (1e-40, 0), (1, 0), (5, 0), (3, 4), (-1, -3)]
    wants = [(255, 0, 0), (128, 255, 0), (0, 255, 255), (128, 0, 255)] * 2 + [(255, 255, 255), (255, 255, 255), (255, 128, 128), (255, 0, 0)]
    wants += [tuple(int(v) for v in RR.colour(F(3), F(4), 2.0)), tuple(int(v) for v in RR.colour(F(-1), F(-3), 2.0))]
    assert wants[-2] == (255, 219, 0)                                    # |v| = 5 > vmax = 2: the hue of test_render_cpu's (3, 4, 5) case
    pts = np.array([[(k + 0.5, 1.5, 0.0) for k in range(len(vecs))]], dtype=F)
    vec = np.array([[(vx, vy, 0.0) for vx, vy in vecs]], dtype=F)
    cls = np.ones((1, len(vecs)), dtype=np.uint8)
    d = lambda a: torch.from_numpy(a).to(dev)
    got = render.render_rows(d(pts), torch.tensor([len(vecs)], dtype=torch.int32, device=dev), d(vec), d(cls), view=view, size=size, vmax=2.0,
                             radius=0)
    px = RR.pixels(got.cpu().numpy())[0]
    assert [tuple(int(v) for v in p) for p in px[1, : len(vecs)]] == wants
    assert (px[0] == 24).all() and (px[2] == 24).all() and (px[1, len(vecs):] == 24).all()


# ---- no host reads: captured in a graph -------------------------------------------------------------------------------------------------------
def test_graph_replay_on_overwritten_inputs(dev):
    from deflow_amd import render
    size, view = SHAPES["37x53"]
    N = 300
    cases = [make_case(N, size, view, seed=s) for s in (1, 2)]
    d = lambda a: torch.from_numpy(a).to(dev)
    static = [d(a) for a in cases[0]]
    kw = dict(view=view, size=size, vmax=VMAX, radius=2, legend=5)
    render.render_rows(*static, **kw)                                    # eager first
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                            # one stream, a linear chain: memset, splat, resolve
        out = render.render_rows(*static, **kw)
    for case in (cases[1], cases[0]):
        for s, a in zip(static, case):
            s.copy_(d(a))
        out.fill_(0x5A)
        g.replay()
        torch.cuda.synchronize()
        same(out, RR.render_rows(*case, view, size, VMAX, radius=2, legend=5), "replay")


# ---- guards -----------------------------------------------------------------------------------------------------------------------------------
def test_guards_refuse_and_leave_the_outputs_alone(dev):
    from deflow_amd import render
    from deflow_amd._lib import call, ptr
    N, (W, H) = 16, (16, 12)
    pts = torch.zeros(2, N, 3, device=dev)
    vec = torch.ones(2, N, 3, device=dev)
    cls = torch.ones(2, N, dtype=torch.uint8, device=dev)
    cnt = torch.full((2,), N, dtype=torch.int32, device=dev)
    kw = dict(view=(-1.0, -1.0, 4.0), size=(W, H), vmax=1.0)
    assert tuple(render.render_rows(pts, cnt, vec, cls, **kw).shape) == (2, H, 1 + 3 * W)
    for bad, exc, what in ((dict(points=pts.cpu()), TypeError, "points must be a CUDA tensor"), (dict(vec=vec.cpu()), TypeError, "vec must be a CUDA"),
                           (dict(cls=cls.cpu()), TypeError, "cls must be a CUDA"), (dict(count=cnt.cpu()), TypeError, "count must be a CUDA"),
                           (dict(points=pts.double()), ValueError, "points must be torch.float32"), (dict(points=pts[:, :0]), ValueError, "N >= 1"),
                           (dict(vec=vec[:, :-1]), ValueError, "vec must be"), (dict(cls=cls.int()), ValueError, "cls must be torch.uint8"),
                           (dict(count=cnt.long()), ValueError, "count must be torch.int32"), (dict(count=cnt[:1]), ValueError, "count must be"),
                           (dict(size=(0, H)), ValueError, "size: 1 <= W, H <= 4096"), (dict(size=(W, 4097)), ValueError, "size: 1 <= W, H <= 4096"),
                           (dict(size=(W,)), ValueError, "size must be"), (dict(size=(W, 12.0)), ValueError, "size must be"),
                           (dict(radius=5), ValueError, "radius must be"), (dict(radius=-1), ValueError, "radius must be"),
                           (dict(vmax=0.0), ValueError, "vmax must be positive"), (dict(vmax=float("nan")), ValueError, "vmax must be"),
                           (dict(view=(-1.0, -1.0, 0.0)), ValueError, "inv_res"), (dict(view=(float("inf"), 0.0, 1.0)), ValueError, "xmin"),
                           (dict(view=(0.0, 1.0)), ValueError, "view must be"), (dict(bg=(1, 2, 256)), ValueError, "bg must be"),
                           (dict(legend=4), ValueError, "legend must be"), (dict(legend=-1), ValueError, "legend must be")):
        a = dict(points=pts, count=cnt, vec=vec, cls=cls, **kw)
        a.update(bad)
        with pytest.raises(exc, match=what):
            render.render_rows(a.pop("points"), a.pop("count"), a.pop("vec"), a.pop("cls"), **a)
    with pytest.raises(ValueError, match=r"B \* H \* \(1 \+ 3 W\) < 2\^31"):
        render.check_image(60, (4096, 4096))
    assert render.check_image(2, (W, H), legend=3) == (W, H, 0x181818)               # 2 L + 5 = 11 <= 12
    # the entry points' own guards: a negative status, no launch -- the poisoned output and the zeroed image stay as they were
    image = torch.zeros(2, H, W, dtype=torch.int64, device=dev)
    out = torch.full((2, H, 1 + 3 * W), 0x5A, dtype=torch.uint8, device=dev)
    sp = lambda **k: call("df_render_splat", ptr(pts), ptr(vec), ptr(cls), ptr(cnt), k.get("B", 2), k.get("N", N), -1.0, -1.0, k.get("inv", 4.0),
                          k.get("W", W), k.get("H", H), k.get("vmax", 1.0), k.get("r", 1), k.get("image", ptr(image)), None)
    rs = lambda **k: call("df_render_resolve", k.get("image", ptr(image)), k.get("B", 2), k.get("W", W), k.get("H", H), k.get("bg", 0), k.get("L", 0),
                          k.get("out", ptr(out)), None)
    for fn, k, code in ((sp, dict(B=0), "SHAPE"), (sp, dict(B=65536), "SHAPE"), (sp, dict(N=0), "SHAPE"), (sp, dict(W=0), "SHAPE"), (sp, dict(H=4097), "SHAPE"),
                        (sp, dict(B=60, W=4096, H=4096), "SHAPE"), (sp, dict(B=65535, N=40000), "SHAPE"), (sp, dict(r=5), "ARG"), (sp, dict(r=-1), "ARG"),
                        (sp, dict(vmax=0.0), "ARG"), (sp, dict(inv=-1.0), "ARG"), (sp, dict(image=None), "ARG"), (sp, dict(image=ptr(image) + 4), "ALIGN"),
                        (rs, dict(B=0), "SHAPE"), (rs, dict(W=4097), "SHAPE"), (rs, dict(bg=1 << 24), "ARG"), (rs, dict(L=4), "ARG"), (rs, dict(L=-1), "ARG"),
                        (rs, dict(out=None), "ARG"), (rs, dict(out=ptr(out) + 1), "ALIGN")):
        with pytest.raises(RuntimeError, match="DF_E_" + code):
            fn(**k)
    torch.cuda.synchronize()
    assert not bool(image.any()) and bool((out == 0x5A).all())
    sp()
    rs()
    torch.cuda.synchronize()
    assert bool(image.any()) and not bool((out[:, :, 1:] == 0x5A).all())              # the same closures do draw when nothing is wrong


# ---- flow_vectors -----------------------------------------------------------------------------------------------------------------------------
def test_flow_vectors(dev):
    from deflow_amd import render, sweeps
    rng = np.random.default_rng(5)
    N = 700
    raw = (rng.standard_normal((B, N, 3)) * (20.0, 20.0, 1.5)).astype(F)
    raw[0, 5, 1] = np.nan
    raw[2, 9, 0] = np.inf
    count = np.array([N, N - 50, 1], dtype=np.int32)
    raw[1, count[1]:] = np.nan
    drop = (rng.random((B, N)) < 0.3).astype(np.uint8)
    T = np.tile(np.eye(4, dtype=F), (B, 1, 1))
    for b in range(B):
        a = 0.02 * (b + 1)
        T[b, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[b, :3, 3] = rng.standard_normal(3) * (1.0, 0.3, 0.05)
    d = lambda a: torch.from_numpy(a).to(dev)
    raw_d, count_d, T_d = d(raw), d(count), d(T)
    pc, row_of, pos_of, kept = sweeps.compact_rows(raw_d, count_d, d(drop))
    kept_h = kept.cpu().numpy()
    flow = (rng.standard_normal((B, N, 3)) * 0.3).astype(F)
    idx_c = np.zeros((B, N), dtype=np.int64)
    counts = np.zeros(B, dtype=np.int32)
    for b in range(B):                                                    # the "model" decoded half of the kept rows
        m = int(kept_h[b]) // 2
        counts[b] = m
        idx_c[b, :m] = rng.permutation(int(kept_h[b]))[:m]
    est, _ = sweeps.compose_flow(raw_d, count_d, T_d, pos_of, d(flow), d(idx_c), d(counts))
    vec = render.flow_vectors(raw_d, count_d, est, T_d).cpu().numpy()
    est_h, pos_h = est.cpu().numpy(), pos_of.cpu().numpy()
    zero_rows = decoded_rows = 0
    for b in range(B):
        fin = np.isfinite(raw[b]).all(axis=1) & (np.arange(N) < count[b])
        with np.errstate(all="ignore"):
            want = est_h[b][fin] - SR.pose_flow(raw[b][fin], T[b])       # section 6f's formula, then one fsub
        assert want.dtype == F
        assert np.array_equal(vec[b][fin].view(np.int32), want.view(np.int32)), f"sample {b}"
        decoded = np.zeros(N, dtype=bool)
        inv = set(idx_c[b, : counts[b]].tolist())
        decoded[np.array([r for r in np.nonzero(fin)[0] if pos_h[b, r] in inv], dtype=np.int64)] = True
        others = fin & ~decoded                                           # ground and undecoded rows: compose_flow gave them the pose flow
        assert (vec[b][others].view(np.int32) == 0).all(), "a pose-flow row is not exactly +0.0"
        zero_rows += int(others.sum())
        decoded_rows += int(decoded.sum())
        assert not np.isfinite(vec[b][~np.isfinite(raw[b]).all(axis=1)]).all(axis=1).any()      # non-finite rows stay non-finite
    assert zero_rows > 300 and decoded_rows > 200
    gt = d((rng.standard_normal((B, N, 3)) * 0.3).astype(F))
    v2 = render.flow_vectors(raw_d, count_d, gt, T_d)
    assert v2.shape == est.shape and v2.dtype == torch.float32
    with pytest.raises(TypeError, match="flow must be a CUDA"):
        render.flow_vectors(raw_d, count_d, est.cpu(), T_d)
    with pytest.raises(ValueError, match="T must be"):
        render.flow_vectors(raw_d, count_d, est, T_d[:, :3])
    with pytest.raises(ValueError, match="flow must be torch.float32"):
        render.flow_vectors(raw_d, count_d, est.half(), T_d)


# ---- the command ------------------------------------------------------------------------------------------------------------------------------
def reference_composite(directory, sid, ts, est, panels, opt, ground=None):
    """the PNG's pixels [H, W len(panels), 3] from the flow file's array and the scene file alone, in numpy (``ground``: a mask to use
    instead of the scene file's)"""
    from deflow_amd import save
    pairs = save.ScenePairs(directory, sid)
    it = pairs[[str(t) for _, t in pairs.data_index].index(str(ts))]
    raw = it["pc0"][:, :3].float().numpy()
    n = raw.shape[0]
    T = it["ego_motion"].float().numpy()
    cls = np.where((it["gm0"].numpy().reshape(-1) if ground is None else ground) != 0, 2, 1).astype(np.uint8)
    valid = it["flow_is_valid"].numpy().reshape(-1) != 0
    gt = it["flow"].float().numpy()
    with np.errstate(all="ignore"):
        pf = SR.pose_flow(raw, T) if n else np.zeros((0, 3), dtype=F)
        vecs = {"est": (est - pf, cls, opt["vmax"]), "gt": (gt - pf, np.where(valid, cls, 0).astype(np.uint8), opt["vmax"]),
                "err": (est - gt, np.where(valid, cls, 0).astype(np.uint8), opt["vmax_err"])}
    out = []
    for p in panels:
        v, c, vmax = vecs[p]
        if n == 0:                                                        # the collate pads an empty sweep to one NaN row
            raw_p, v, c = np.full((1, 3), np.nan, dtype=F), np.zeros((1, 3), dtype=F), np.zeros(1, dtype=np.uint8)
        else:
            raw_p = raw
        img = RR.splat(raw_p, v.astype(F), c, n, opt["view"], opt["size"], vmax, opt["radius"])
        out.append(RR.pixels(RR.resolve(img, (24, 24, 24), opt["legend"])))
    return np.concatenate(out, axis=1)


def test_vis_command(dev, tmp_path, golden_dir, capsys):
    import deflow_amd
    from deflow_amd import png, save, train, vis
    from deflow_amd.h5scene import H5File
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "scene_val.h5"), tmp_path / "scene_val.h5")      # never written under tests/golden
    shutil.copy(os.path.join(golden_dir, "av2_mini", "train", "scene_chunked.h5"), tmp_path / "scene_chunked.h5")
    torch.manual_seed(47)
    model = deflow_amd.DeFlow(**SMALL, num_iters=2).to(dev).eval()
    cfg = dict(train.DEFAULTS)
    cfg.update({"voxel_size": SMALL["voxel_size"], "point_cloud_range": SMALL["point_cloud_range"], "model.target.num_iters": 2, "batch_size": 4})
    ckpt = str(tmp_path / "small_best.ckpt")
    train.save_checkpoint(ckpt, model, types.SimpleNamespace(opt=types.SimpleNamespace(state_dict=lambda: {})), cfg, 0, 0)
    assert save.main([f"checkpoint={ckpt}", f"dataset_path={tmp_path}"]) == 0
    capsys.readouterr()
    view = ["range=25.6", "res=0.4", "legend=6", "vmax=0.4", "vmax_err=0.3"]
    base = [f"dataset_path={tmp_path}", "res_name=small_best"] + view
    lines_of = lambda: [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    sweeps_of = {}
    for sid in ("scene_chunked", "scene_val"):
        with H5File(str(tmp_path / (sid + ".h5"))) as f:
            sweeps_of[sid] = sorted(f.keys(), key=int)[:-1]               # every sweep but the scene's last
    runs = {"three": (base + [f"out_dir={tmp_path / 'three'}"], ["est", "gt", "err"]),           # the default: the files carry flow
            "est": (base + ["panels=est", f"out_dir={tmp_path / 'est'}"], ["est"])}
    for name, (argv, panels) in runs.items():
        assert vis.main(argv) == 0
        lines = lines_of()
        opt = vis.parse_args(argv)
        assert opt["size"] == (128, 128)
        assert [x["scene"] for x in lines] == ["scene_chunked", "scene_val"]
        drawn = 0
        for x in lines:
            sid = x["scene"]
            assert x["images"] == len(sweeps_of[sid]) and x["skipped"] == 0 and x["panels"] == panels and x["size"] == [128 * len(panels), 128]
            assert sorted(os.listdir(tmp_path / name / sid)) == sorted(t + ".png" for t in sweeps_of[sid])
            flows = save.read_flow(save.flow_path(str(tmp_path), sid, "small_best"))
            for ts in sweeps_of[sid]:
                got = png.read_png(vis.image_path(str(tmp_path / name), sid, ts))
                want = reference_composite(str(tmp_path), sid, ts, flows[ts][0], panels, opt)
                assert got.shape == want.shape == (128, 128 * len(panels), 3)
                assert np.array_equal(got, want), f"{name} {sid} {ts}: {int((got != want).any(axis=2).sum())} pixels differ"
                drawn += int((got != 24).any(axis=2).sum())
        print(f"[vis] panels={','.join(panels)}: {drawn} pixels drawn over {sum(len(v) for v in sweeps_of.values())} images")
        assert drawn > 2000
    # a second run without overwrite writes nothing
    stamp = {p: os.path.getmtime(p) for sid in sweeps_of for p in [vis.image_path(str(tmp_path / "est"), sid, t) for t in sweeps_of[sid]]}
    assert vis.main(runs["est"][0]) == 0
    lines = lines_of()
    assert all(x["images"] == 0 and x["skipped"] == len(sweeps_of[x["scene"]]) for x in lines) and len(lines) == 2
    assert all(os.path.getmtime(p) == t for p, t in stamp.items())
    # flow_source=model: the same bytes as flow_source=file at the same batch size (the checkpoint's 4, which save ran at)
    argv = [f"dataset_path={tmp_path}", "flow_source=model", f"checkpoint={ckpt}", "panels=est", f"out_dir={tmp_path / 'model'}"] + view
    assert vis.main(argv) == 0
    lines = lines_of()
    assert [x["images"] for x in lines] == [len(sweeps_of["scene_chunked"]), len(sweeps_of["scene_val"])]
    for sid, tss in sweeps_of.items():
        for ts in tss:
            a = open(vis.image_path(str(tmp_path / "model"), sid, ts), "rb").read()
            assert a == open(vis.image_path(str(tmp_path / "est"), sid, ts), "rb").read(), f"model / file differ: {sid} {ts}"
    # every=2 and overwrite=true on one scene: every second sweep is rewritten with the same bytes, nothing else appears
    assert vis.main(runs["est"][0] + ["every=2", "overwrite=true", "scenes=scene_val"]) == 0
    lines = lines_of()
    assert len(lines) == 1 and lines[0]["images"] == (len(sweeps_of["scene_val"]) + 1) // 2 and lines[0]["skipped"] == 0
    assert sorted(os.listdir(tmp_path / "est" / "scene_val")) == sorted(t + ".png" for t in sweeps_of["scene_val"])
    with pytest.raises(SystemExit, match="not found"):
        vis.main([f"dataset_path={tmp_path}", "res_name=nothing_saved"] + view)
    # ground_source=online: the grey rows come from a segmenter on the GPU, no mask is read from the files
    from deflow_amd.ground import GroundSegmenter
    from deflow_amd.sweeps import collate_raw_pad
    assert vis.main(base + ["panels=est", "ground_source=online", "scenes=scene_val", f"out_dir={tmp_path / 'online'}"]) == 0
    assert lines_of()[0]["images"] == len(sweeps_of["scene_val"])
    opt = vis.parse_args(base)
    pairs = save.ScenePairs(str(tmp_path), "scene_val", "online")
    items = [pairs[i] for i in range(len(pairs))]
    flows = save.read_flow(save.flow_path(str(tmp_path), "scene_val", "small_best"))
    differ = 0
    for k in range(0, len(items), 4):
        hb = collate_raw_pad(items[k:k + 4])
        masks = GroundSegmenter(len(hb["timestamp"]), device=dev).segment(hb["raw0"].to(dev), hb["n0"].to(dev)).cpu().numpy()
        assert masks.any() and not masks.all()
        for i, (ts, n) in enumerate(zip(hb["timestamp"], hb["n0"].tolist())):
            got = png.read_png(vis.image_path(str(tmp_path / "online"), "scene_val", ts))
            want = reference_composite(str(tmp_path), "scene_val", ts, flows[str(ts)][0], ["est"], opt, ground=masks[i, :n])
            assert np.array_equal(got, want), f"online scene_val {ts}"
            differ += int((got != png.read_png(vis.image_path(str(tmp_path / "est"), "scene_val", ts))).any())
    print(f"[vis] ground_source=online: {differ} of {len(items)} images differ from the ones drawn with the files' masks")
