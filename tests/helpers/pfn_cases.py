"""Cases for the pillar feature net's backward kernels (csrc/pillarize.hip: pfn_bwd_stats / finalize / weights, driven by
DynamicEmbedder.pillarize_bwd): clouds built to reach one launch path each, and their CPU references.

The reference is oracle.ref_torch.DynamicEmbedder (feature_net.mode set) on the CPU in fp32 and as its copy.deepcopy(...).double() twin
on pts.double(); a case with two clouds calls the same module twice, so the parameter gradients of both calls are summed.  Parameters:
the module's own seeded initialisation with the BatchNorm weight, bias and running statistics moved off their init.  The upstream
gradient is randn [B,32,H,W] per cloud under a seeded generator.  reference(name, mode, train) is cached per process and never
modified by its readers.

  case        content                                                              what it reaches (nbs = max(1, min(256, ceil(N / 32))))
  tiny        B = 2, N = 20, 16 / 14 valid points, a three-point pillar            nbs = 1
  stride      B = 3, N = 9000, gaussian cloud (NaN tail, corner points, five       nbs capped at 256, a second grid-stride pass (sorted
              points in one pillar), z inside the range; in sample 1 a 40-point    positions >= 8192), the finalize lane loops past 32,
              pillar across sorted position 8192                                   a run that straddles the stride
  degenerate  S = 4, N = 6000: 5000 points in one cell + 600 spread | 3000 in      an empty sample in the middle of sample_range, runs far
              one row | all NaN | two points (eval mode: one point)                longer than a 32-position block, cnt = 2
  rect_far    B = 3, N = 5000, 40 x 72 cells over +-51.2 m, uniform cloud          gx != gy, a width that is no power of two, fp32
                                                                                   cancellation in p - mean at 50 m
  pair        two clouds, B = 2, N = 700 each: the trainer's form -- the two       ld = 64 channel halves, accumulate, no read of a dead
              32-channel halves of one [B,H,W,64] gradient buffer, the second      cell (the GPU test fills them with NaN)
              call accumulating into the first's result

`pair` also holds, in cloud 0, (i) three exact copies of one point next to a fourth point of the same pillar -- in max mode a tie between
duplicates must be counted once -- and (ii) a pillar of two points that differ in x only.  Channel TIE_CH of pair's Linear has its three
x-weights (columns 0, 3, 6) set to zero, so both points of (ii) give the SAME positive feature there (bit-equal in every arithmetic)
while their input features differ: the only way a tie between different points can carry gradient.  Ties at the ReLU's zero -- pillar
(ii) has those too, in the channels where both points are non-positive -- carry none under either rule, since the ReLU masks them.
The upstream gradient of that pillar in channel TIE_CH is TIE_GRAD = 8 instead of a randn draw, so that the one tie weighs more than
the bound in a dW that sums 1 200 points.

pfn_backward64() restates the backward in float64 the way the kernels walk it (sorted runs, per-sample sums, coefficients, du (x) f);
with fault=None it equals the oracle's autograd, and it takes the faults the CPU test injects (never into a kernel).
"""
import copy
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

FLOOR, FACTOR = 2e-5, 4.0       # parity.three_way's arguments for every comparison of these cases (BNBWD of the layer census)
NAMES = ["tiny", "stride", "degenerate", "rect_far", "pair"]
MODES = ["avg", "max"]
# (case, mode, train): all five in both modes in training mode; tiny / degenerate / pair also in eval mode
PARAMS = [(n, m, True) for n in NAMES for m in MODES] + [(n, m, False) for n in ("tiny", "degenerate", "pair") for m in MODES]
TIE_CH = 5
GRADS = ("dW", "dgamma", "dbeta")

SMALL = dict(vs=[0.2, 0.2, 6], rng=[-6.4, -6.4, -3, 6.4, 6.4, 3], dims=[64, 64])
FAR = dict(vs=[102.4 / 72, 102.4 / 40, 6], rng=[-51.2, -51.2, -3, 51.2, 51.2, 3], dims=[40, 72])
SEEDS = {"tiny": 11, "stride": 12, "degenerate": 13, "rect_far": 14, "pair": 15}


@dataclass
class Case:
    name: str
    mode: str
    train: bool
    clouds: List[torch.Tensor]           # one or two [B,N,3] fp32
    vs: List[float]
    rng: List[float]
    dims: List[int]                      # [H, W]
    state: Dict[str, torch.Tensor]       # state_dict of oracle.ref_torch.DynamicEmbedder
    gout: List[torch.Tensor]             # per cloud [B,32,H,W] fp32, finite everywhere

    @property
    def B(self):
        return self.clouds[0].shape[0]

    @property
    def N(self):
        return self.clouds[0].shape[1]

    @property
    def nbs(self):
        return max(1, min(256, (self.N + 31) // 32))      # deflow_amd/encoder.py: pillarize_bwd


def gaussian_cloud(B, N, seed, extent, zspan=6.6):
    """_cloud of tests/test_gpu_kernels.py (zspan = 6.6: a tenth of the points leave the +-3 m of the range)"""
    g = torch.Generator().manual_seed(seed)
    pts = torch.cat([torch.randn(B, N, 2, generator=g) * extent * 0.4, (torch.rand(B, N, 1, generator=g) - 0.5) * zspan], 2)
    pts[:, -N // 50:] = float("nan")
    pts[0, 5] = torch.tensor([-extent, -extent, -3.0])        # exactly on the lower corner
    pts[0, 6] = torch.tensor([extent, 0.0, 0.0])              # exactly on the (exclusive) upper bound
    pts[0, 7:12] = torch.tensor([0.31, 0.47, 0.1])            # five points in one pillar
    return pts


def _clouds(name: str, train: bool):
    from oracle import ref_torch as O
    seed = SEEDS[name]
    g = torch.Generator().manual_seed(seed)
    if name == "tiny":
        pts = torch.cat([torch.randn(2, 20, 2, generator=g) * 2.5, torch.rand(2, 20, 1, generator=g) * 5.0 - 2.5], 2)
        pts[0, 3:6] = torch.tensor([[1.23, -0.55, 0.4], [1.27, -0.51, -1.1], [1.38, -0.42, 2.0]])     # one pillar, three points
        pts[0, 16:] = float("nan")
        pts[1, :3] = float("nan")
        pts[1, 17:] = float("nan")
        return [pts]
    if name == "stride":
        # _cloud's z span would leave about 7 850 valid points of 9 000, short of the 8 192 sorted positions one grid-stride pass
        # covers: z stays inside the range here, so that only the NaN tail and the gaussian's far points go (about 8 600 stay)
        pts = gaussian_cloud(3, 9000, 1000 + seed, 6.4, zspan=5.8)
        # sample 1: a 40-point pillar whose run starts below sorted position 8192 and ends above it
        rows = slice(100, 100 + STRADDLE)
        pts[1, rows] = float("nan")
        vc = O.DynamicVoxelizer(SMALL["vs"], SMALL["rng"])(pts[1:2])[0]["voxel_coords"].long()
        k = int(torch.sort(vc[:, 1] * 64 + vc[:, 2]).values[8192 - STRADDLE // 2])
        lo = torch.tensor([-6.4 + 0.2 * (k % 64), -6.4 + 0.2 * (k // 64), -2.5])
        pts[1, rows] = lo + torch.tensor([0.02, 0.02, 0.0]) + torch.rand(STRADDLE, 3, generator=g) * torch.tensor([0.16, 0.16, 5.0])
        return [pts]
    if name == "degenerate":            # the clouds of test_pillar_bands_degenerate_clouds, the 5000 points moved 0.1 m in y: there
        S, N = 4, 6000                  # they lie across the cell border at y = -2.0 (3291 + 1709); here they share ONE cell
        pts = torch.full((S, N, 3), float("nan"))
        pts[0, :5000] = torch.tensor([1.01, -2.13, 0.5]) + torch.rand(5000, 3, generator=g) * torch.tensor([0.09, 0.09, 1.0])
        pts[0, 5000:5600] = torch.rand(600, 3, generator=g) * torch.tensor([12.0, 12.0, 5.0]) - torch.tensor([6.0, 6.0, 2.5])
        pts[1, :3000, 0] = torch.rand(3000, generator=g) * 12.6 - 6.3
        pts[1, :3000, 1] = 0.05
        pts[1, :3000, 2] = 0.0
        pts[3, 17] = torch.tensor([0.1, 0.1, 0.1])
        if train:                       # the reference's BatchNorm1d refuses a one-point sample in training mode
            pts[3, 4000] = torch.tensor([-3.3, 2.2, -1.0])
        return [pts]
    if name == "rect_far":
        B, N = 3, 5000
        pts = torch.cat([(torch.rand(B, N, 2, generator=g) - 0.5) * 2.02 * 51.2, torch.rand(B, N, 1, generator=g) * 6.6 - 3.3], 2)
        pts[:, -N // 40:] = float("nan")
        return [pts]
    if name == "pair":
        a, b = gaussian_cloud(2, 700, 2000 + seed, 6.4), gaussian_cloud(2, 700, 3000 + seed, 6.4)
        a[1, 30:33] = torch.tensor([-2.13, 3.31, 0.7])            # three exact copies ...
        a[1, 33] = torch.tensor([-2.07, 3.25, -1.6])              # ... and a fourth, different point of the same pillar
        a[0, 40] = torch.tensor([4.41, -5.13, 1.9])               # two points that differ in x only (one pillar)
        a[0, 41] = torch.tensor([4.59, -5.13, 1.9])
        return [a, b]
    raise KeyError(name)


STRADDLE = 40                   # stride, sample 1: points of the pillar whose run crosses sorted position 8192
TIE_POINTS = (0, 40, 41)        # pair, cloud 0: sample, the two input rows of pillar (ii)
TIE_CELL, TIE_GRAD = (6, 54), 8.0   # its cell (y, x) and the upstream gradient there in channel TIE_CH
DUP_POINTS = (1, 30, 33)        # pair, cloud 0: sample, first duplicate, the different point


def oracle(c: Case, double: bool = False):
    from oracle import ref_torch as O
    m = O.DynamicEmbedder(c.vs, c.dims, c.rng, 32)
    m.load_state_dict(c.state)
    m.feature_net.mode = c.mode
    m.train(c.train)
    return m.double() if double else m


_CASES: Dict[tuple, Case] = {}


def case(name: str, mode: str, train: bool) -> Case:
    key = (name, mode, train)
    if key in _CASES:
        return _CASES[key]
    from oracle import ref_torch as O
    geo = FAR if name == "rect_far" else SMALL
    seed = SEEDS[name]
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        m = O.DynamicEmbedder(geo["vs"], geo["dims"], geo["rng"], 32)
    g = torch.Generator().manual_seed(100 + seed)
    lin, bn = m.feature_net.pfn_layers[0][0], m.feature_net.pfn_layers[0][1]
    with torch.no_grad():
        bn.weight.copy_(torch.rand(32, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(32, generator=g) * 0.4 - 0.2)
        bn.running_mean.copy_(torch.rand(32, generator=g) * 2 - 1)
        bn.running_var.copy_(torch.rand(32, generator=g) * 1.5 + 0.5)
        if name == "pair":
            lin.weight[TIE_CH, [0, 3, 6]] = 0.0
    clouds = _clouds(name, train)
    H, W = geo["dims"]
    gout = [torch.randn(cl.shape[0], 32, H, W, generator=g) for cl in clouds]
    if name == "pair":      # a plain randn gradient leaves the tie's share of dW (a sum over 1 200 points at |x| <= 6.4) under the bound
        gout[0][TIE_POINTS[0], TIE_CH, TIE_CELL[0], TIE_CELL[1]] = TIE_GRAD
    c = Case(name, mode, train, clouds, geo["vs"], geo["rng"], geo["dims"], copy.deepcopy(m.state_dict()), gout)
    _CASES[key] = c
    return c


def _params(m):
    p = dict(m.feature_net.pfn_layers[0].named_parameters())
    return {"dW": p["0.weight"], "dgamma": p["1.weight"], "dbeta": p["1.bias"]}


def _oracle_run(c: Case, double: bool):
    """-> dict(canvas=[per cloud [B,32,H,W]], coords=[per cloud [per sample [n,3] int32]], grads={dW, dgamma, dbeta})"""
    m = oracle(c, double)
    canvas, coords = [], []
    for pts, go in zip(c.clouds, c.gout):
        out, infos = m(pts.double() if double else pts)
        out.backward(go.double() if double else go)
        canvas.append(out.detach())
        coords.append([i["voxel_coords"] for i in infos])
    return dict(canvas=canvas, coords=coords, grads={k: p.grad.clone() for k, p in _params(m).items()})


_REFS: Dict[tuple, tuple] = {}


def reference(name: str, mode: str, train: bool):
    """-> (fp32 result, float64 result) of _oracle_run"""
    key = (name, mode, train)
    if key not in _REFS:
        c = case(name, mode, train)
        _REFS[key] = (_oracle_run(c, False), _oracle_run(c, True))
    return _REFS[key]


def occupied(c: Case, cloud: int) -> torch.Tensor:
    """[B,H,W] bool: the cells cloud `cloud` occupies (all the backward may read of its gradient image)"""
    H, W = c.dims
    occ = torch.zeros(c.B, H, W, dtype=torch.bool)
    for b, vc in enumerate(reference(c.name, c.mode, c.train)[1]["coords"][cloud]):
        occ[b, vc[:, 1].long(), vc[:, 2].long()] = True
    return occ


# ---- float64 restatement of the backward, the way the kernels walk it ---------------------------------------------------------------
def sorted_sample(c: Case, cloud: int, b: int):
    """valid points of sample b in the kernels' order (stable sort by cell y W + x) -> (points [M,3] float64, cell [M] int64)"""
    from oracle import ref_torch as O
    info = O.DynamicVoxelizer(c.vs, c.rng)(c.clouds[cloud][b:b + 1])[0]
    vc = info["voxel_coords"].long()
    cell = vc[:, 1] * c.dims[1] + vc[:, 2]
    order = torch.sort(cell, stable=True).indices
    return info["points"][order].double(), cell[order]


def pfn_backward64(c: Case, fault: Optional[str] = None, **fk) -> Dict[str, torch.Tensor]:
    """float64 (dW, dgamma, dbeta) of the case.  fault (None = the exact computation):
      drop_last_pillar  sample=b                the last pillar of sample b (cloud 0) is not visited
      drop_block        sample=b, start=i       pillars whose head lies at sorted positions [i, i + 32) of sample b are not visited
      coef_prev                                 the batch-statistic coefficients of sample b are those of sample (b - 1) mod B
      overwrite                                 the second cloud's result replaces the first's
      last_max                                  max mode: the gradient goes to the LAST point that attains the maximum
      swap_gxgy                                 the pillar centre's (cx, cy) come from cell / gy instead of cell / gx
      no_inv            sample=b, pillar=k      avg mode: pillar k (in sorted order) of sample b keeps its gradient undivided by its length"""
    H, W = c.dims
    W64 = c.state["feature_net.pfn_layers.0.0.weight"].double()
    bn = {k: c.state["feature_net.pfn_layers.0.1." + k].double() for k in ("weight", "bias", "running_mean", "running_var")}
    eps = 1e-3
    vx, vy, vz = [float(v) for v in c.vs]
    off = [vx / 2 + c.rng[0], vy / 2 + c.rng[1], vz / 2 + c.rng[2]]
    total = None
    for ci in range(len(c.clouds)):
        samples = []
        for b in range(c.B):
            p, cell = sorted_sample(c, ci, b)
            M = p.shape[0]
            if M == 0:
                samples.append(None)
                continue
            uc, pid, n = torch.unique_consecutive(cell, return_inverse=True, return_counts=True)
            P = uc.shape[0]
            start = torch.cumsum(n, 0) - n
            mean = torch.zeros(P, 3, dtype=torch.float64).index_add_(0, pid, p) / n[:, None]
            gx = H if fault == "swap_gxgy" else W
            cy = uc // gx
            cx = uc - cy * gx
            ctr = torch.stack([cx.double() * vx + off[0], cy.double() * vy + off[1], torch.zeros(P, dtype=torch.float64) + off[2]], 1)
            f = torch.cat([p, p - mean[pid], p - ctr[pid]], 1)
            u = f @ W64.t()
            if c.train:
                mu, var = u.mean(0), u.var(0, unbiased=False)
            else:
                mu, var = bn["running_mean"], bn["running_var"]
            istd = 1.0 / torch.sqrt(var + eps)
            xh = (u - mu) * istd
            y = xh * bn["weight"] + bn["bias"]
            pos = y > 0
            gcell = c.gout[ci][b].double().reshape(32, H * W)[:, uc].t()      # [P,32]
            if c.mode == "avg":
                inv = 1.0 / n.double()
                if fault == "no_inv" and ci == 0 and b == fk["sample"]:
                    inv[fk["pillar"]] = 1.0
                gh = gcell[pid] * inv[pid][:, None] * pos
            else:
                v = torch.relu(y)
                idx = pid[:, None].expand(M, 32)
                vmax = torch.full((P, 32), -float("inf"), dtype=torch.float64).scatter_reduce(0, idx, v, "amax")
                order = torch.arange(M)[:, None].expand(M, 32)
                if fault == "last_max":
                    cand = torch.where(v == vmax[pid], order, torch.full_like(order, -1))
                    pick = torch.full((P, 32), -1, dtype=torch.long).scatter_reduce(0, idx, cand, "amax")
                else:
                    cand = torch.where(v == vmax[pid], order, torch.full_like(order, M))
                    pick = torch.full((P, 32), M, dtype=torch.long).scatter_reduce(0, idx, cand, "amin")
                gh = torch.zeros(M, 32, dtype=torch.float64).scatter_(0, pick, gcell) * pos
            act = torch.ones(M, dtype=torch.bool)           # points of visited pillars
            if fault == "drop_last_pillar" and ci == 0 and b == fk["sample"]:
                act[start[-1]:] = False
            if fault == "drop_block" and ci == 0 and b == fk["sample"]:
                heads = start[(start >= fk["start"]) & (start < fk["start"] + 32)]
                assert heads.numel() > 0
                for k in (start.unsqueeze(1) == heads.unsqueeze(0)).any(1).nonzero().squeeze(1).tolist():
                    act[start[k]:start[k] + n[k]] = False
            gh = gh * act[:, None]
            s1, s2 = gh.sum(0), (gh * xh).sum(0)
            samples.append(dict(f=f, xh=xh, gh=gh, act=act, istd=istd, s1=s1, s2=s2, M=M))
        dW, dgamma, dbeta = torch.zeros(32, 9, dtype=torch.float64), torch.zeros(32, dtype=torch.float64), torch.zeros(32, dtype=torch.float64)
        zero = torch.zeros(32, dtype=torch.float64)
        coefs = [(zero, zero) if s is None or not c.train else (s["s1"] / s["M"], s["s2"] / s["M"]) for s in samples]
        for b, s in enumerate(samples):
            if s is None:
                continue
            dbeta += s["s1"]
            dgamma += s["s2"]
            c1, c2 = coefs[(b - 1) % c.B] if fault == "coef_prev" else coefs[b]
            du = bn["weight"] * s["istd"] * (s["gh"] - c1 - s["xh"] * c2) * s["act"][:, None]
            dW += du.t() @ s["f"]
        res = {"dW": dW, "dgamma": dgamma, "dbeta": dbeta}
        total = res if total is None or fault == "overwrite" else {k: total[k] + res[k] for k in res}
    return total
