"""Cases for the sparse kernels at the UNet's two ends (csrc/pillarize.hip: df_pillar_input_grad in its bf16x3 queue form and its
fp32-MFMA fallback, df_sparse_in_wgrad, df_sparse_conv3x3 / _h2 / _bf16, df_sparse_wgrad3x3 / _x2): sorted key lists built to reach
one piece of each kernel's walk, the tensors the kernels read, and a restatement of the walks in plain Python.

  case             content                                                         what it reaches
  wrap             B = 1, 96 x 104, 9000 distinct cells + 1000 duplicate points,   a wave sees >= 8 windows; a queue head passes PGQ = 128 and
                   nblk = 1                                                        wraps (per parity class in pillar_input_grad_x3, the single
                                                                                   queue of the conv forms); tails carry into the next window
  one_class        B = 1, 64 x 72, 2100 points, all in cells with odd row and      64 heads of one class on top of a left-over tail: queue fill
                   odd column, the duplicates in the first 500 cells, nblk = 1     > 64; three class queues stay empty; five of the nine tap
                                                                                   waves of sparse_in_wgrad have n = 0 (zero partials)
  single_tap       the same with even row and even column                          the one-tap class of the stride-2 data gradient
  border           B = 2, 16 x 24, exactly the border cells; sample 1 without the  every cell has out-of-image taps (stride 2: oy = -1, ox =
                   two top corners, nblk = 2                                       w2); nothing leaks in from a neighbouring row or sample
  runs             B = 4, counts [700, 0, 1, 70]; sample 0: a 300-point pillar at  windows without a head (64 and 256 points), a run longer
                   sorted positions 230 .. 529, a 10-point run at 60 .. 69;        than SW_WIN, an empty sample inside sample_range, cnt = 1, a
                   nblk = 2, and 64 = max(1, 256 // B) as `runs@engine`            head at i == sr.off; the engine's launch at B = 4
  idle             B = 1, 16 x 24, 37 points, nblk = 256                           the engine's B = 1 launch: >= 250 workgroups without a
                                                                                   window (zero partials over NaN, no per-cell write)
  views            B = 3, 32 x 40, 700 points, sample 1 empty; every tensor a      every ld, img_stride and channel offset; accumulate 0 and 1
                   channel slice of a wider buffer (LAYOUT), nblk = 3
  views_unaligned  views with the skip gradient in a buffer of ld = 66             the fp32-MFMA fallback of df_pillar_input_grad, in process

Tensors (fp32, seeded, finite everywhere; NHWC; weights LOGICAL [O,I,kh,kw], which the GPU test hands over as [O,kh,kw,I] memory):
x, w, bias, dy of the last conv (3x3, 64 -> 64); canvas [B,H,W,64] (cloud g = channels 32 g ..), dy1 [2B,H/2,W/2,64] (image g B + b), w1
[64,32,3,3], dskip [B,H,W,64], w3 [64,64,1,1] and the old d(canvas) `dold` [B,H,W,64] of the canvas gradient.  Both clouds use the same
key list.  LAYOUT[name] = (buffer width, channel offset) of each tensor the kernels address through a df_img.

reference(name) holds, per kernel, the ref64 function's result in float64 and the same function evaluated in float32 on the CPU
(their dtype argument): bounds(...) is parity.three_way's rule, max(floor, 4 x that fp32 error), per norm of ref64.errors.  Cached per process,
never modified by its readers.

walk_pig / walk_conv / walk_win restate the kernels' iteration (which wave of which workgroup sees which window, what its queues hold) and
visit the pillar heads in the kernels' order; percell64 / partials64 put the float64 rows of ref64 through that walk.  With fault=None
they equal ref64; they take the faults tests/test_sparse_cases_cpu.py injects (never into a kernel).
"""
import math
import os
import re
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

import ref64 as R

if os.path.dirname(os.path.dirname(os.path.abspath(__file__))) not in sys.path:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from test_gpu_layer_census import CONV32  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAMES = ["wrap", "one_class", "single_tap", "border", "runs", "idle", "views", "views_unaligned"]
RUNS = NAMES[:5] + ["runs@engine"] + NAMES[5:]          # what the tests are parametrised over: every case, `runs` twice
SEEDS = {n: 31 + i for i, n in enumerate(NAMES)}
SENTINEL = -512.0                                       # exact in every format the kernels use

# floors: the project's own figures.  CONV32 of the layer census (imported: one figure, one place), also for the fp32 form's bias sums, and
# the figures tests/test_gpu_kernels.py::test_sparse_wgrad3x3_x2_vs_float64 asserts for the bf16x2 form (no per-channel figure there)
X2 = R.Bounds(max=2e-5, rms=1e-5, ch=math.inf)
X2_BIAS = R.Bounds(max=2e-6, rms=math.inf, ch=math.inf)
FACTOR = 4.0

PLAIN = dict(x=(64, 0), y=(64, 0), dy=(64, 0), canvas=(64, 0), dcanvas=(64, 0), dskip=(64, 0))
VIEWS = dict(x=(128, 36), y=(128, 60), dy=(192, 100), canvas=(64, 0), dcanvas=(64, 0), dskip=(128, 64))
LAYOUT = {n: PLAIN for n in NAMES}
LAYOUT["views"] = VIEWS
LAYOUT["views_unaligned"] = dict(VIEWS, dskip=(66, 2))


def constants() -> Dict[str, int]:
    """PGQ, SW_WIN, SIW_WIN, PG_THREADS as csrc/pillarize.hip defines them"""
    src = open(os.path.join(ROOT, "deflow_amd", "csrc", "pillarize.hip")).read()
    out = {}
    for k in ("PGQ", "SW_WIN", "SIW_WIN", "PG_THREADS"):
        m = re.findall(r"^constexpr\s+int\s+" + k + r"\s*=\s*(\d+)\s*;", src, re.M)
        assert len(m) == 1, (k, m)
        out[k] = int(m[0])
    return out


@dataclass
class Case:
    name: str
    B: int
    H: int
    W: int
    nblk: int
    keys: torch.Tensor                   # [sum counts] int32, sorted: b H W + cell, one entry per POINT
    counts: torch.Tensor                 # [B] int32
    t: Dict[str, torch.Tensor] = field(default_factory=dict)

    @property
    def heads(self) -> torch.Tensor:
        """the listed cells once each (int64, sorted): what the references take"""
        return torch.unique_consecutive(self.keys.long())

    @property
    def layout(self):
        return LAYOUT[self.name]

    def occ(self) -> torch.Tensor:
        o = torch.zeros(self.B * self.H * self.W, dtype=torch.bool)
        o[self.heads] = True
        return o.view(self.B, self.H, self.W)


def _with_dups(cells: torch.Tensor, ndup: int, among: int, g) -> torch.Tensor:
    """cells once each + ndup more points drawn from the first `among` of them (sorted)"""
    cells = torch.sort(cells)[0]
    extra = cells[torch.randint(0, among, (ndup,), generator=g)]
    return torch.sort(torch.cat([cells, extra]))[0]


def _samples(name: str, g):
    """-> (H, W, nblk, [per sample: sorted cells, one per point])"""
    if name == "wrap":
        H, W = 96, 104
        cells = torch.randperm(H * W, generator=g)[:9000]
        return H, W, 1, [_with_dups(cells, 1000, 9000, g)]
    if name in ("one_class", "single_tap"):
        H, W = 64, 72
        par = 1 if name == "one_class" else 0
        yy, xx = torch.meshgrid(torch.arange(par, H, 2), torch.arange(par, W, 2), indexing="ij")
        cells = (yy * W + xx).reshape(-1)                       # 1152 cells of one parity class
        return H, W, 1, [_with_dups(cells, 948, 500, g)]
    if name == "border":
        H, W = 16, 24
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        edge = ((yy == 0) | (yy == H - 1) | (xx == 0) | (xx == W - 1)).reshape(-1)
        c0 = torch.nonzero(edge).squeeze(1)
        c1 = c0[(c0 != 0) & (c0 != W - 1)]                      # without the two top corners
        return H, W, 2, [c0, c1]
    if name == "runs":
        H, W = 32, 40
        d = torch.sort(torch.randperm(H * W, generator=g)[:392])[0]       # 60 cells | the 10-run | 160 cells | the 300-run | 170 cells
        s0 = torch.cat([d[:60], d[60:61].repeat(10), d[61:221], d[221:222].repeat(300), d[222:392]])
        s3 = _with_dups(torch.randperm(H * W, generator=g)[:50], 20, 50, g)
        return H, W, 2, [s0, d[:0], torch.tensor([517]), s3]
    if name == "idle":
        H, W = 16, 24
        return H, W, 256, [_with_dups(torch.randperm(H * W, generator=g)[:30], 7, 30, g)]
    if name in ("views", "views_unaligned"):
        H, W = 32, 40
        out = []
        for b in range(3):
            out.append(torch.zeros(0, dtype=torch.long) if b == 1 else _with_dups(torch.randperm(H * W, generator=g)[:525], 175, 525, g))
        return H, W, 3, out
    raise KeyError(name)


_CASES: Dict[str, Case] = {}


def case(run: str) -> Case:
    """run = a case name, or `runs@engine`: `runs` launched with max(1, 256 // B) workgroups per sample"""
    if run in _CASES:
        return _CASES[run]
    name = run.split("@")[0]
    seed = SEEDS["views" if name == "views_unaligned" else name]
    g = torch.Generator().manual_seed(seed)
    H, W, nblk, samples = _samples(name, g)
    B = len(samples)
    if run.endswith("@engine"):
        nblk = max(1, 256 // B)
    keys = torch.cat([s.long() + b * H * W for b, s in enumerate(samples)]).to(torch.int32)
    counts = torch.tensor([s.numel() for s in samples], dtype=torch.int32)
    rn = lambda *shape, s=1.0: torch.randn(*shape, generator=g) * s      # noqa: E731
    t = dict(x=rn(B, H, W, 64), w=rn(64, 64, 3, 3, s=0.05), bias=rn(64, s=0.1), dy=rn(B, H, W, 64),
             canvas=rn(B, H, W, 64), dy1=rn(2 * B, H // 2, W // 2, 64), w1=rn(64, 32, 3, 3, s=0.08),
             dskip=rn(B, H, W, 64), w3=rn(64, 64, 1, 1, s=0.1), dold=rn(B, H, W, 64))
    c = Case(name, B, H, W, nblk, keys, counts, t)
    _CASES[run] = c
    return c


# ---- references -------------------------------------------------------------------------------------------------------------
def _all_refs(c: Case, dtype: torch.dtype) -> Dict[str, object]:
    t, k, B = c.t, c.heads, c.B
    out = {"conv": R.sparse_conv3x3(t["x"], t["w"], t["bias"], k, dtype=dtype),
           "conv_bf16": R.sparse_conv3x3(t["x"], t["w"], t["bias"], k, rnd=R.bf16_rne, dtype=dtype)}
    out["wgrad"], out["wgrad_bias"] = R.sparse_wgrad3x3(t["x"], t["dy"], k, dtype=dtype)
    for g in (0, 1):
        sl = slice(32 * g, 32 * g + 32)
        out[f"in_wgrad{g}"] = R.sparse_in_wgrad(t["canvas"][..., sl], t["dy1"][g * B:(g + 1) * B], k, dtype=dtype)
        out[f"pig{g}"] = R.pillar_input_grad(t["dy1"][g * B:(g + 1) * B], t["w1"], t["dskip"], t["w3"][:, sl], k, dtype=dtype)
    return out


_REFS: Dict[str, tuple] = {}


def reference(run: str):
    """-> (fp32 results, float64 results): dicts conv, conv_bf16 [ncells,64]; wgrad [64,64,3,3], wgrad_bias [64]; in_wgrad{g} [64,32,3,3];
    pig{g} [ncells,32] (row j = cell heads[j])"""
    name = run.split("@")[0]
    name = "views" if name == "views_unaligned" else name       # (the same keys and tensors)
    if name not in _REFS:
        c = case(name)
        _REFS[name] = (_all_refs(c, torch.float32), _all_refs(c, torch.float64))
    return _REFS[name]


def ch_dim(key: str) -> int:
    return 0 if key.startswith(("wgrad", "in_wgrad")) else -1


def bounds(floor: R.Bounds, r32: torch.Tensor, r64: torch.Tensor, dim: int) -> R.Bounds:
    """max(floor, FACTOR x the reference's own fp32 error), per norm"""
    e = R.errors(r32, r64, dim)
    return R.Bounds(max=max(floor.max, FACTOR * e["max"]), rms=max(floor.rms, FACTOR * e["rms"]), ch=max(floor.ch, FACTOR * e["ch"]))


def excess(e: dict, b: R.Bounds) -> float:
    """the largest error / bound over the three norms (<= 1 passes)"""
    if not e["finite"]:
        return math.inf
    return max(e["max"] / b.max, e["rms"] / b.rms, e["ch"] / b.ch)


# ---- the walks ----------------------------------------------------------------------------------------------------------------
def _sample_ranges(c: Case):
    off = 0
    for b in range(c.B):
        cnt = int(c.counts[b])
        yield b, off, off + cnt
        off += cnt


def _is_head(c: Case) -> torch.Tensor:
    """head[i]: i == sr.off or key[i - 1] != key[i] (a sample's first key differs from the previous sample's last: b H W + cell)"""
    k = c.keys.long()
    h = torch.ones(k.numel(), dtype=torch.bool)
    h[1:] = k[1:] != k[:-1]
    return h


def _queue(stats, visits, cells, q, cap, fault, tag):
    """push the window's heads `cells` into the circular queue q = dict(h, n, pushed), pop full batches of 16"""
    for cell in cells:
        slot = q["pushed"]
        q["pushed"] += 1
        q["n"] += 1
        if fault == "drop_at_wrap" and slot == cap and not stats.get("dropped"):
            stats["dropped"] = (tag, cell)          # the first head written past the end of the array is lost
            q["lost"] = q.get("lost", []) + [slot]
        q.setdefault("slots", []).append(cell)
    stats["max_fill"] = max(stats["max_fill"], q["n"])
    while q["n"] >= 16:
        _pop(visits, q, 16)
        if q["h"] >= cap:
            stats["head_wraps"] += 1
            if tag[0] == "pig":
                stats["wraps_by_class"][tag[-1]] += 1
            q["h"] -= cap


def _pop(visits, q, n):
    first = q["popped"]
    for s in range(first, first + n):
        if s not in q.get("lost", ()):
            visits.append(q["slots"][s])
    q["popped"] += n
    q["h"] += n
    q["n"] -= n


def _new_q():
    return dict(h=0, n=0, pushed=0, popped=0)


def _new_stats():
    return dict(wraps_by_class=[0, 0, 0, 0], max_fill=0, head_wraps=0, max_windows=0, max_pushed=0, idle=0, carried=0, empty_windows=0, empty_queues=0)


def walk_pig(c: Case, k: Dict[str, int], fault: Optional[str] = None, queued: bool = True):
    """df_pillar_input_grad: workgroup (bx, b) has PG_THREADS / 64 waves; wave wv scans the 64-point windows at sr.off + (bx nw + wv) 64,
    stride nblk nw 64.  queued (the x3 form): four class queues of PGQ per wave, full batches of 16, the tails at the end of the wave's
    range; else (the fp32 form) every window is multiplied by itself.  -> (visits: keys in processing order, stats)"""
    nw, cap = k["PG_THREADS"] // 64, k["PGQ"]
    head, keys = _is_head(c), c.keys.long()
    visits, st = [], _new_stats()
    for b, off, end in _sample_ranges(c):
        ncell = c.H * c.W
        for bx in range(c.nblk):
            nwin_wg = 0
            for wv in range(nw):
                qs = [_new_q() for _ in range(4)]
                nwin = 0
                for base in range(off + (bx * nw + wv) * 64, end, c.nblk * nw * 64):
                    nwin += 1
                    i = torch.arange(base, min(base + 64, end))
                    hk = keys[i][head[i]]
                    cell = hk - b * ncell
                    cls = (((cell // c.W + 1) & 1) << 1) | ((cell % c.W + 1) & 1)
                    if hk.numel() == 0:
                        st["empty_windows"] += 1
                    if any(q["n"] > 0 for q in qs) and hk.numel() > 0:
                        st["carried"] += 1
                    for cl in range(4):
                        sel = hk[cls == cl].tolist()
                        if queued:
                            _queue(st, visits, sel, qs[cl], cap, fault, ("pig", b, bx, wv, cl))
                        else:
                            visits.extend(sel)
                for q in qs:
                    if q["n"] > 0:
                        _pop(visits, q, q["n"])
                    st["max_pushed"] = max(st["max_pushed"], q["pushed"])
                if nwin:
                    st["empty_queues"] = max(st["empty_queues"], sum(q["pushed"] == 0 for q in qs))
                st["max_windows"] = max(st["max_windows"], nwin)
                nwin_wg += nwin
            st["idle"] += nwin_wg == 0
    return visits, st


def walk_conv(c: Case, k: Dict[str, int], fault: Optional[str] = None, queued: bool = True):
    """df_sparse_conv3x3 / _h2 / _bf16: a sample's 64-point chunks are split into nblk contiguous ranges; the waves of workgroup bx take the
    chunks of its range in turn.  queued (_h2, _bf16): one queue of PGQ per wave.  -> (visits, stats)"""
    nw, cap = k["PG_THREADS"] // 64, k["PGQ"]
    head, keys = _is_head(c), c.keys.long()
    visits, st = [], _new_stats()
    for b, off, end in _sample_ranges(c):
        nchunk = (end - off + 63) // 64
        per = (nchunk + c.nblk - 1) // c.nblk
        for bx in range(c.nblk):
            c_lo, c_hi = bx * per, min(bx * per + per, nchunk)
            st["idle"] += c_lo >= c_hi
            for wv in range(nw):
                q, nwin = _new_q(), 0
                for base in range(off + (c_lo + wv) * 64, off + c_hi * 64, nw * 64):
                    nwin += 1
                    i = torch.arange(base, min(base + 64, end))
                    hk = keys[i][head[i]].tolist()
                    if not hk:
                        st["empty_windows"] += 1
                    if q["n"] > 0 and hk:
                        st["carried"] += 1
                    if queued:
                        _queue(st, visits, hk, q, cap, fault, ("conv", b, bx, wv))
                    else:
                        visits.extend(hk)
                if q["n"] > 0:
                    _pop(visits, q, q["n"])
                st["max_pushed"] = max(st["max_pushed"], q["pushed"])
                st["max_windows"] = max(st["max_windows"], nwin)
    return visits, st


def walk_win(c: Case, win: int):
    """df_sparse_wgrad3x3 / _x2 (win = SW_WIN) and df_sparse_in_wgrad (SIW_WIN): workgroup (bx, b) scans the windows at sr.off + bx win, stride
    nblk win; one wave per tap, all nine see the same windows.  -> (per workgroup b nblk + bx: the head keys of its windows, stats)"""
    head, keys = _is_head(c), c.keys.long()
    groups, st = [], _new_stats()
    st["max_run"] = int(torch.unique_consecutive(keys, return_counts=True)[1].max())
    for b, off, end in _sample_ranges(c):
        for bx in range(c.nblk):
            mine, nwin = [], 0
            for base in range(off + bx * win, end, c.nblk * win):
                nwin += 1
                i = torch.arange(base, min(base + win, end))
                hk = keys[i][head[i]]
                st["empty_windows"] += hk.numel() == 0
                st.setdefault("heads_per_window", []).append(int(hk.numel()))
                mine.append(hk)
            st["idle"] += nwin == 0
            st["max_windows"] = max(st["max_windows"], nwin)
            groups.append(torch.cat(mine) if mine else keys[:0])
    return groups, st


def in_wgrad_taps(c: Case, hk: torch.Tensor) -> List[int]:
    """per tap of df_sparse_in_wgrad: how many of the heads hk it keeps (parity and range of (q + 1 - k) / 2)"""
    cell = hk % (c.H * c.W)
    y, x = cell // c.W, cell % c.W
    n = []
    for ky in range(3):
        for kx in range(3):
            ty, tx = y + 1 - ky, x + 1 - kx
            ok = (ty % 2 == 0) & (tx % 2 == 0) & (ty >= 0) & (ty // 2 < c.H // 2) & (tx >= 0) & (tx // 2 < c.W // 2)
            n.append(int(ok.sum()))
    return n


# ---- float64 restatements that go through the walks --------------------------------------------------------------------------------
def conv_rows64(c: Case, heads: torch.Tensor, fault: Optional[str] = None) -> torch.Tensor:
    """the last conv at `heads`, tap by tap over the flattened image as the kernels address it: row (qy W + qx) of sample b, zero where
    (qy, qx) is outside the image.  fault `oob_tap`: tap (ky, kx) = (1, 0) at x = 0 reads the address it computes -- the last pixel of the
    row above -- instead of zero"""
    x, w = c.t["x"].double().reshape(c.B, c.H * c.W, 64), c.t["w"].double()
    b, y, xx = R.cells(heads, c.H, c.W)
    out = c.t["bias"].double().expand(heads.numel(), 64).clone()
    for ky in range(3):
        for kx in range(3):
            qy, qx = y + ky - 1, xx + kx - 1
            ok = (qy >= 0) & (qy < c.H) & (qx >= 0) & (qx < c.W)
            flat = qy * c.W + qx
            if fault == "oob_tap" and (ky, kx) == (1, 0):
                ok = ok | ((qx < 0) & (flat >= 0))
            rows = x[b, flat.clamp(0, c.H * c.W - 1)] * ok[:, None]
            out += rows @ w[:, :, ky, kx].T
    return out


def percell64(c: Case, visits: List[int], rows: torch.Tensor, old: Optional[torch.Tensor], accumulate: bool,
              fault: Optional[str] = None) -> torch.Tensor:
    """a per-cell kernel's output at the listed cells: every visit writes (accumulate ? what is there : 0) + its row over `old` (None: the
    sentinel).  faults: `twice` -- every pillar of more than 200 points is visited a second time; `ignore_accumulate` -- the old value is
    added whatever `accumulate` says"""
    heads = c.heads
    pos = {int(h): j for j, h in enumerate(heads.tolist())}
    out = torch.full_like(rows, SENTINEL) if old is None else old.double().clone()
    if fault == "twice":
        k, n = torch.unique_consecutive(c.keys.long(), return_counts=True)
        visits = list(visits) + k[n > 200].tolist()
        assert len(visits) > heads.numel()
    for v in visits:
        j = pos[v]
        out[j] = (out[j] if (accumulate or fault == "ignore_accumulate") else 0.0) + rows[j]
    return out


def partials64(c: Case, groups: List[torch.Tensor], fn, shape, fault: Optional[str] = None) -> torch.Tensor:
    """a weight-gradient kernel's partial rows [nblk B, *shape] over a NaN-filled workspace: workgroup j writes fn(its heads), zeros if it
    has none.  fault `idle_unwritten`: a workgroup without a window returns before it writes"""
    ws = torch.full((len(groups),) + tuple(shape), float("nan"), dtype=torch.float64)
    for j, hk in enumerate(groups):
        if hk.numel() == 0:
            if fault != "idle_unwritten":
                ws[j] = 0.0
            continue
        ws[j] = fn(hk)
    return ws
