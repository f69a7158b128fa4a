"""Decoder cases for the GRU head's kernel tests: inputs built to reach one launch mechanism each, and their CPU reference.

The reference is oracle.ref_torch.ConvGRUDecoder on the CPU in fp32 and as its .double() twin, carrying the `w.*` weights of
tests/golden/g2_grudecoder_it4.npz (the reference's own initialisation).  Images are randn under a seeded generator, offsets uniform in
+-0.1, the flow cotangent randn per row.  reference(name) is cached per process: every kernel form of a case shares one run.

  case    counts per sample                                            image    T   what it reaches
  edges   0 1 15 16 17 63 64 65 0 0 127 128 129 191 192 193 0          23 x 41  2   every row-tile tail (16 nwv rows per workgroup: 64 /
                                                                                    128 / 192), empty first / middle / last samples, 943
                                                                                    cells (no multiple of the gather's 32 / 64 cell passes)
  walk    1700 0 2300 2047 1                                           23 x 41  4   380 stages x 4 iterations over 170 gate splits (~9 per
                                                                                    split: the four-deep ring wraps; splits straddle sample
                                                                                    and iteration boundaries and the empty sample)
  blocks  40000 0 37001 40000                                          64 x 96  1   B ceil(N / 64) = 2500 >= 2048 (df_colsum_stage); 7313
                                                                                    stages over 1024 head splits (~7 per split, ring depth 3)

Cell placement (all cases): a sample with at least 100 rows puts HEAVY_ROWS = 70 rows into one cell (more than a wavefront, and its
neighbours in the gather backward's four-cell lane group -- the cells 8 k or 16 k further on -- and 48 cells either side stay empty), one
row in each corner cell (the last cell of the image among them), and the rest on a small pool of random cells (about three rows per
cell); smaller samples fill the corners last-first and then the pool.  Row order is shuffled, so a cell's rows are not adjacent.
"""
import os
from dataclasses import dataclass, field
from typing import Dict, List

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN_W = os.path.join(ROOT, "tests", "golden", "g2_grudecoder_it4.npz")
WP = 16                 # rows per stage of the weight-gradient kernels (csrc/decoder_wgrad.hip)
HEAVY_ROWS = 70
HEAVY_CLEAR = 48        # cells either side of the heavy cell that stay empty (4-cell lane groups: +-8 k, +-16 k, k <= 3)

SPECS = {
    "edges": dict(counts=[0, 1, 15, 16, 17, 63, 64, 65, 0, 0, 127, 128, 129, 191, 192, 193, 0], H=23, W=41, iters=2, seed=101),
    "walk": dict(counts=[1700, 0, 2300, 2047, 1], H=23, W=41, iters=4, seed=202),
    "blocks": dict(counts=[40000, 0, 37001, 40000], H=64, W=96, iters=1, seed=303),
}


@dataclass
class Case:
    name: str
    counts: List[int]
    H: int
    W: int
    iters: int
    before: torch.Tensor                 # [B,64,H,W] fp32
    after: torch.Tensor
    coords: List[torch.Tensor]           # per sample [n,3] int32 (z, y, x)
    offs: List[torch.Tensor]             # per sample [n,3] fp32
    cot: List[torch.Tensor]              # per sample [n,3] fp32: the flow cotangent
    heavy: Dict[int, int] = field(default_factory=dict)     # sample -> linear index of its 70-row cell

    @property
    def B(self):
        return len(self.counts)

    @property
    def N(self):
        return max(1, max(self.counts))

    def infos(self):
        return [{"voxel_coords": c, "point_offsets": o} for c, o in zip(self.coords, self.offs)]

    def cells(self, b):
        """linear cell index y W + x of every row of sample b"""
        return self.coords[b][:, 1].long() * self.W + self.coords[b][:, 2].long()


def _place(n, H, W, g):
    """-> ([n] linear cell index, heavy cell or None)"""
    ncell = H * W
    corners = [ncell - 1, 0, W - 1, (H - 1) * W]           # the image's last cell first: a one-row sample lands there
    cells, heavy = [], None
    if n >= 100:
        heavy = (H // 2) * W + W // 2
        cells += [heavy] * HEAVY_ROWS
    cells += corners[:max(0, min(4, n - len(cells)))]
    rest = n - len(cells)
    if rest > 0:
        ok = torch.ones(ncell, dtype=torch.bool)
        if heavy is not None:
            ok[max(0, heavy - HEAVY_CLEAR):heavy + HEAVY_CLEAR + 1] = False
        allowed = ok.nonzero().squeeze(1)
        pool = allowed[torch.randint(0, allowed.numel(), (max(1, rest // 3),), generator=g)]
        cells += pool[torch.randint(0, pool.numel(), (rest,), generator=g)].tolist()
    cells = torch.tensor(cells, dtype=torch.int64)
    return cells[torch.randperm(n, generator=g)] if n else cells, heavy


_CASES: Dict[str, Case] = {}


def case(name: str) -> Case:
    if name in _CASES:
        return _CASES[name]
    s = SPECS[name]
    g = torch.Generator().manual_seed(s["seed"])
    H, W, B = s["H"], s["W"], len(s["counts"])
    before, after = torch.randn(B, 64, H, W, generator=g), torch.randn(B, 64, H, W, generator=g)
    c = Case(name, list(s["counts"]), H, W, s["iters"], before, after, [], [], [])
    for b, n in enumerate(c.counts):
        cells, heavy = _place(n, H, W, g)
        if heavy is not None:
            c.heavy[b] = heavy
        c.coords.append(torch.stack([torch.zeros_like(cells), cells // W, cells % W], 1).to(torch.int32).reshape(n, 3))
        c.offs.append(torch.rand(n, 3, generator=g) * 0.2 - 0.1)
        c.cot.append(torch.randn(n, 3, generator=g))
    _CASES[name] = c
    return c


def weights() -> Dict[str, torch.Tensor]:
    g = np.load(GOLDEN_W)
    return {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w.")}


def oracle_head(iters: int, double: bool = False):
    from oracle import ref_torch as O
    m = O.ConvGRUDecoder(num_iters=iters)
    m.load_state_dict(weights())
    return m.double() if double else m


def _oracle_run(c: Case, double: bool):
    """forward + backward of the oracle on its own leaf copies -> dict(flow=[...], gbefore, gafter, gw={name: grad})"""
    m = oracle_head(c.iters, double)
    dt = torch.float64 if double else torch.float32
    before = c.before.to(dt).clone().requires_grad_(True)
    after = c.after.to(dt).clone().requires_grad_(True)
    infos = [{"voxel_coords": vc, "point_offsets": o.to(dt)} for vc, o in zip(c.coords, c.offs)]
    flows = m(before, after, infos)
    sum((f * ct.to(dt)).sum() for f, ct in zip(flows, c.cot)).backward()
    return dict(flow=[f.detach() for f in flows], gbefore=before.grad, gafter=after.grad,
                gw={k: p.grad for k, p in m.named_parameters()})


_REFS: Dict[str, tuple] = {}


def reference(name: str):
    """-> (fp32 result, float64 result) of _oracle_run; computed once per process and never modified by its readers"""
    if name not in _REFS:
        c = case(name)
        _REFS[name] = (_oracle_run(c, False), _oracle_run(c, True))
    return _REFS[name]


def rows_contribution(c: Case, b: int, rows: slice):
    """float64: what rows `rows` of sample b add to (d(before)[b], d(after)[b], {name: parameter gradient}).  The loss is a sum
    over rows and a row touches nothing but its own cell and the shared weights, so this is a forward + backward of those rows alone."""
    m = oracle_head(c.iters, True)
    before = c.before[b].double().clone().requires_grad_(True)
    after = c.after[b].double().clone().requires_grad_(True)
    flow = m.forward_single(before, after, c.offs[b][rows].double(), c.coords[b][rows])
    (flow * c.cot[b][rows].double()).sum().backward()
    return before.grad, after.grad, {k: p.grad for k, p in m.named_parameters()}


# ---- structure of the split-K walks, from the counts (csrc/decoder_wgrad.hip: gru_wgrad4_kernel / gru_head_wgrad4_kernel) -------------
def stages_per_sample(counts):
    return [(n + WP - 1) // WP for n in counts]


def split_ranges(total: int, nsplit: int):
    """[w0, w1) of every split: w0 = total * split / nsplit as the kernels compute it"""
    return [(total * s // nsplit, total * (s + 1) // nsplit) for s in range(nsplit)]


def stage_owner(counts, iters):
    """-> list over the S * iters stages of a gate walk of (iteration, sample)"""
    per = [b for b, k in enumerate(stages_per_sample(counts)) for _ in range(k)]
    return [(t, b) for t in range(iters) for b in per]


def segsum_ascending(rows: torch.Tensor, cell: torch.Tensor, ncell: int) -> torch.Tensor:
    """[n,C] fp32 rows -> [ncell,C]: per cell 0 + row_1 + row_2 + ... in ascending row index, every add one fp32 add -- the order the
    gather backward promises (csrc/decoder_bwd.hip)"""
    assert rows.dtype == torch.float32 and rows.device.type == "cpu"
    order = torch.argsort(cell, stable=True)
    r = rows[order]
    cnt = torch.bincount(cell, minlength=ncell)
    start = torch.cumsum(cnt, 0) - cnt
    out = torch.zeros(ncell, rows.shape[1], dtype=torch.float32)
    for j in range(int(cnt.max()) if cell.numel() else 0):
        sel = (cnt > j).nonzero().squeeze(1)
        out[sel] = out[sel] + r[start[sel] + j]
    return out
