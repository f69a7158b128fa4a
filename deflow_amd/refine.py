"""Per-cluster rigid snap of any model's flow on the GPU (``python -m deflow_amd.refine save|eval ...``): the rows of one body move
together, so the first sweep is clustered, one robust yaw + translation per cluster is fitted to the flow the model produced, the result is
checked against the second sweep, and every row of an accepted cluster gets the cluster's motion.  It sits BEHIND the models -- the
trained networks and the checkpoint-free ones of ``pairflow.TABLE`` alike -- and is no model of its own.

UNPINNED: the recipe is the rigid refinement of Chodosh et al., "Re-evaluating LiDAR scene flow" (WACV'24), but no upstream source was
read and every choice here is this project's own.  The definition is in DESIGN.md section 6p and include/deflow_amd.h;
tests/helpers/refine_ref.py restates it in numpy.  The clusters come from ``cluster.dbscan``, their ordered row lists from
df_rigid_segments, the nearest-neighbour distances of the check from df_nn_grid_build / df_chamfer_nn; the fit, the check's score and the
apply run on csrc/refine.hip.

``python -m deflow_amd.refine save <the save command's arguments> [refine_*=]`` writes ``<scene_id>.<res_name>.flow.npz`` with the refined
flow (``res_name`` defaults to what ``save`` would choose plus ``+rigid``); ``python -m deflow_amd.refine eval <the eval command's
arguments> [refine_*=]`` prints the same tables for the refined flow.

CUDA tensors only, like the rest of the library: there is no CPU fallback.  Nothing here reads a device value back."""
from __future__ import annotations

import functools
import sys
from typing import Dict, List, Optional, Sequence

import torch

from . import pairflow, rigid
from ._lib import call, ptr, stream
from .args import cloud, flag, integer, merged, nonneg, positive
from .args import tensor as _tensor
from .chamfer import CELL, GRID_RANGE, RowGrid

STATUS_NAMES = {0: "empty", 1: "snapped", 2: "too few rows", 3: "too large", 4: "inlier fraction", 5: "yaw / displacement", 6: "static",
                7: "worse against the second sweep"}
TABLE_COLS = 12          # theta, tx, ty, tz, inlier_frac, rms, rows used, status, c_before, c_after, 0, 0 (csrc/refine.hip: RF_COLS)
MAX_ITERS = 64

# every default of section 6p; all of them are arguments of rigid_refine and Refined, and `refine_<name>=` keys of the command
DEFAULTS: Dict[str, object] = {"eps": 0.7, "min_points": 4, "min_cluster_size": 20, "min_rows": 8, "max_cluster_points": 8192, "iters": 4,
                               "delta": 0.1, "inlier_dist": 0.2, "min_inlier_frac": 0.5, "max_yaw": 0.35, "max_disp": 3.4,
                               "static_disp": 0.05, "static_yaw": 0.02, "check": True, "check_trunc": 2.0, "check_tol": 0.05}
COMMAND_KEYS: Dict[str, str] = {"refine_" + k: k for k in DEFAULTS}
# what pairflow's command helpers want to know about a family of keys; NOT a line of pairflow.TABLE: this is no model
ENTRY = pairflow.Entry("refine", "refine", "Refined", "refine", "6p", "")
COMMANDS = ("save", "eval")
_show = lambda v: str(v).lower() if isinstance(v, bool) else repr(v)
USAGE = ("usage: python -m deflow_amd.refine save|eval <that command's arguments> " +
         " ".join(f"[{k}={_show(DEFAULTS[n])}]" for k, n in COMMAND_KEYS.items()))


def check_params(p: Dict[str, object]) -> Dict[str, object]:
    """validated copy of a parameter dict (ValueError naming the argument); launches nothing"""
    fn = "rigid_refine"
    out = merged(fn, DEFAULTS, p)
    integer(fn, out, "iters", 0, MAX_ITERS, finite=True)
    for k in ("min_points", "min_cluster_size", "min_rows", "max_cluster_points"):
        integer(fn, out, k, 1, 1 << 30, finite=True)
    for k in ("eps", "delta", "inlier_dist", "check_trunc"):
        positive(fn, out, k, finite=True)
    for k in ("min_inlier_frac", "max_yaw", "max_disp", "static_disp", "static_yaw", "check_tol"):
        nonneg(fn, out, k, finite=True)
    flag(fn, out, "check")
    return out


def params_from_command(given: Dict[str, str]) -> Dict[str, object]:
    """{refine_<name>: value as typed} -> validated parameters; a bad value ends the command (SystemExit)"""
    return pairflow.params_from_command(ENTRY, given)


def kcap(Nc: int, min_cluster_size: int) -> int:
    """cluster slots per sample: every cluster has at least min_cluster_size rows, so no more than this many exist"""
    return max(int(Nc) // int(min_cluster_size), 1)


_rows = functools.partial(cloud, "rigid_refine", rows_limit=3)


def _slots(name: str, K, Nc: int) -> int:
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= Nc:
        raise ValueError(f"rigid_refine: {name} must be an integer in [1, {Nc}], got {K!r}")
    return K


def segments(labels: torch.Tensor, count: torch.Tensor, K: int, status: Optional[torch.Tensor] = None):
    """labels [B,Nc] i32, count [B] i32 -> (labels with the rows behind the count set to 0, seg_off [B, 2K + 1] i32, seg_rows [B, Nc + 1]
    i32): ``rigid.segments``, with the arguments checked."""
    fn = "rigid_refine"
    _tensor(fn, "labels", labels, torch.int32)
    if labels.dim() != 2:
        raise ValueError(f"{fn}: labels must be torch.int32 of shape (B, Nc), got {tuple(labels.shape)}")
    B, Nc = int(labels.shape[0]), int(labels.shape[1])
    dev = labels.device
    _tensor(fn, "count", count, torch.int32, (B,), dev)
    _slots("kcap", K, Nc)
    return rigid.segments(fn, "labels", labels, count, K, status)


def _lists(fn: str, B: int, Nc: int, K: int, dev, seg_off, seg_rows):
    _tensor(fn, "seg_off", seg_off, torch.int32, (B, 2 * K + 1), dev, "x is")
    _tensor(fn, "seg_rows", seg_rows, torch.int32, (B, Nc + 1), dev, "x is")
    return seg_off.contiguous(), seg_rows.contiguous()


def refine_fit(x: torch.Tensor, count: torch.Tensor, flow: torch.Tensor, seg_off: torch.Tensor, seg_rows: torch.Tensor, **params):
    """x, flow [B,Nc,3] f32, count [B] i32, the lists of ``segments`` -> table [B,K,12] f32 (theta, tx, ty, tz, inlier_frac, rms, rows used,
    status, 0, 0, 0, 0) and anchor [B,K] i32 (section 6p b-d).  K is read off seg_off.  Two calls are bit-identical; no host
    synchronisation."""
    fn = "rigid_refine"
    B, Nc = _rows("x", x)
    dev = x.device
    _tensor(fn, "flow", flow, torch.float32, (B, Nc, 3), dev, "x is")
    _tensor(fn, "count", count, torch.int32, (B,), dev, "x is")
    p = check_params(params)
    if not isinstance(seg_off, torch.Tensor) or seg_off.dim() != 2 or seg_off.shape[1] < 3 or seg_off.shape[1] % 2 == 0:
        raise ValueError(f"{fn}: seg_off must be torch.int32 of shape (B, 2 K + 1)")
    K = _slots("kcap", (int(seg_off.shape[1]) - 1) // 2, Nc)
    seg_off, seg_rows = _lists(fn, B, Nc, K, dev, seg_off, seg_rows)
    table = torch.empty(B, K, TABLE_COLS, dtype=torch.float32, device=dev)
    anchor = torch.empty(B, K, dtype=torch.int32, device=dev)
    call("df_refine_fit", ptr(x.detach().contiguous()), ptr(flow.detach().contiguous()), ptr(count.contiguous()), ptr(seg_off), ptr(seg_rows),
         B, Nc, K, p["min_rows"], p["max_cluster_points"], p["iters"], p["delta"], p["inlier_dist"], p["min_inlier_frac"], p["max_yaw"],
         p["max_disp"], p["static_disp"], p["static_yaw"], ptr(table), ptr(anchor), stream())
    return table, anchor


def refine_score(x: torch.Tensor, count: torch.Tensor, flow: torch.Tensor, count1: torch.Tensor, seg_off: torch.Tensor,
                 seg_rows: torch.Tensor, d2_before: torch.Tensor, d2_after: torch.Tensor, table: torch.Tensor, *, check_trunc: float = 2.0,
                 check_tol: float = 0.05) -> torch.Tensor:
    """d2_before / d2_after [B,Nc] f32 (squared nearest-neighbour distances of x + f and x + f' to the second sweep; inf without a
    neighbour) -> ``table`` with c_before, c_after filled and the status of a worsened slot turned into 7 (section 6p e), IN PLACE; it is
    returned too.  A sample with count1 <= 0 passes everything."""
    fn = "rigid_refine"
    B, Nc = _rows("x", x)
    dev = x.device
    _tensor(fn, "flow", flow, torch.float32, (B, Nc, 3), dev, "x is")
    for name, c in (("count", count), ("count1", count1)):
        _tensor(fn, name, c, torch.int32, (B,), dev, "x is")
    for name, d in (("d2_before", d2_before), ("d2_after", d2_after)):
        _tensor(fn, name, d, torch.float32, (B, Nc), dev, "x is")
    p = check_params({"check_trunc": check_trunc, "check_tol": check_tol})
    _tensor(fn, "table", table, torch.float32, None, dev, "x is")
    if table.dim() != 3 or table.shape[0] != B or table.shape[2] != TABLE_COLS or not table.is_contiguous():
        raise ValueError(f"{fn}: table must be contiguous torch.float32 of shape ({B}, K, {TABLE_COLS}), got {tuple(table.shape)}")
    K = _slots("kcap", int(table.shape[1]), Nc)
    seg_off, seg_rows = _lists(fn, B, Nc, K, dev, seg_off, seg_rows)
    call("df_refine_score", ptr(x.detach().contiguous()), ptr(flow.detach().contiguous()), ptr(count.contiguous()), ptr(count1.contiguous()),
         ptr(seg_off), ptr(seg_rows), ptr(d2_before.contiguous()), ptr(d2_after.contiguous()), B, Nc, K, p["check_trunc"], p["check_tol"],
         ptr(table), stream())
    return table


def refine_apply(x: torch.Tensor, count: torch.Tensor, flow: torch.Tensor, labels: torch.Tensor, table: torch.Tensor, anchor: torch.Tensor):
    """-> flow_out [B,Nc,3] f32, rigid_id [B,Nc] i32 (section 6p f): the cluster's motion for the participating rows of a status 1 / 6 slot,
    the bits of ``flow`` for every other row.  Every element is written."""
    fn = "rigid_refine"
    B, Nc = _rows("x", x)
    dev = x.device
    _tensor(fn, "flow", flow, torch.float32, (B, Nc, 3), dev, "x is")
    _tensor(fn, "count", count, torch.int32, (B,), dev, "x is")
    _tensor(fn, "labels", labels, torch.int32, (B, Nc), dev, "x is")
    _tensor(fn, "table", table, torch.float32, None, dev, "x is")
    if table.dim() != 3 or table.shape[0] != B or table.shape[2] != TABLE_COLS or not table.is_contiguous():
        raise ValueError(f"{fn}: table must be contiguous torch.float32 of shape ({B}, K, {TABLE_COLS}), got {tuple(table.shape)}")
    K = _slots("kcap", int(table.shape[1]), Nc)
    _tensor(fn, "anchor", anchor, torch.int32, (B, K), dev, "x is")
    flow_out = torch.empty(B, Nc, 3, dtype=torch.float32, device=dev)
    rigid_id = torch.empty(B, Nc, dtype=torch.int32, device=dev)
    call("df_refine_apply", ptr(x.detach().contiguous()), ptr(flow.detach().contiguous()), ptr(count.contiguous()), ptr(labels.contiguous()),
         ptr(table), ptr(anchor.contiguous()), B, Nc, K, ptr(flow_out), ptr(rigid_id), stream())
    return flow_out, rigid_id


def _nn_d2(queries: Sequence[torch.Tensor], count: torch.Tensor, ref: torch.Tensor, rcount: torch.Tensor, max_dist2: float,
           grid_range: Optional[Sequence[float]]):
    """squared distance of every row of each query cloud to its nearest row of ``ref``: ONE df_nn_grid_build, one df_chamfer_nn per query"""
    grid = RowGrid(int(ref.shape[0]), GRID_RANGE if grid_range is None else grid_range, CELL, ref.device)
    filed = grid.file(ref, rcount)
    return [grid.nn(q, count, None, filed, max_dist2)[0] for q in queries]


def rigid_refine(x: torch.Tensor, count: torch.Tensor, flow: torch.Tensor, pc1: torch.Tensor, count1: torch.Tensor, *,
                 labels: Optional[torch.Tensor] = None, grid_range: Optional[Sequence[float]] = None, **params):
    """x [B,Nc,3] f32 (the decoded rows of the ego-compensated first sweep, compacted) with count [B] i32 valid leading rows, flow [B,Nc,3]
    f32 (the model's residual flow of those rows), pc1 [B,N1,3] f32 with count1 [B] i32 (the second sweep's decoded rows).
    -> flow_out [B,Nc,3] f32 and info: table [B,Kcap,12] f32 (theta, tx, ty, tz, inlier_frac, rms, rows used, status, c_before, c_after, 0,
    0), rigid_id [B,Nc] i32 (the label of a row that got its cluster's motion, else 0), labels [B,Nc] i32 (0 behind the count), anchor
    [B,Kcap] i32, cluster_status i32[1] (dbscan's and the lists' status word, 0 on a sane input).  Kcap = max(Nc // min_cluster_size, 1).
    labels: the cluster labels of x when the caller has them (else ``cluster.dbscan``); grid_range (xmin, ymin, xmax, ymax) as in dbscan:
    it decides only the speed.  Keywords: DEFAULTS.  Rows that get no motion keep ``flow`` bit for bit.  No host synchronisation;
    workspaces come from torch's allocator; two calls are bit-identical."""
    fn = "rigid_refine"
    B, Nc = _rows("x", x)
    dev = x.device
    _tensor(fn, "count", count, torch.int32, (B,), dev, "x is")
    _tensor(fn, "flow", flow, torch.float32, (B, Nc, 3), dev, "x is")
    B1, N1 = _rows("pc1", pc1)
    if B1 != B or pc1.device != dev:
        raise ValueError(f"{fn}: pc1 must have the batch size ({B}) and device of x, got {tuple(pc1.shape)} on {pc1.device}")
    _tensor(fn, "count1", count1, torch.int32, (B,), dev, "x is")
    if labels is not None:
        _tensor(fn, "labels", labels, torch.int32, (B, Nc), dev, "x is")
    p = check_params(params)
    K = kcap(Nc, p["min_cluster_size"])
    with torch.no_grad():
        x, flow, pc1 = x.detach().contiguous(), flow.detach().contiguous(), pc1.detach().contiguous()
        count, count1 = count.contiguous(), count1.contiguous()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        if labels is None:
            from .cluster import dbscan
            labels, _ = dbscan(x, count, eps=p["eps"], min_points=p["min_points"], min_cluster_size=p["min_cluster_size"],
                               grid_range=grid_range, status=status)
        labels, seg_off, seg_rows = segments(labels, count, K, status)
        fit = {k: p[k] for k in ("min_rows", "max_cluster_points", "iters", "delta", "inlier_dist", "min_inlier_frac", "max_yaw", "max_disp",
                                 "static_disp", "static_yaw")}
        table, anchor = refine_fit(x, count, flow, seg_off, seg_rows, **fit)
        if p["check"]:
            provisional, _ = refine_apply(x, count, flow, labels, table, anchor)
            d2_before, d2_after = _nn_d2([x + flow, x + provisional], count, pc1, count1, p["check_trunc"] ** 2, grid_range)
            refine_score(x, count, flow, count1, seg_off, seg_rows, d2_before, d2_after, table, check_trunc=p["check_trunc"],
                         check_tol=p["check_tol"])
        flow_out, rigid_id = refine_apply(x, count, flow, labels, table, anchor)
    return flow_out, {"table": table, "rigid_id": rigid_id, "labels": labels, "anchor": anchor, "cluster_status": status}


class Refined:
    """Any model that has ``forward_padded`` -- ``DeFlow`` and every ``PairFlowModel`` -- with its flow snapped per cluster:
    ``forward_padded`` calls the inner one, takes the compact decoded rows and replaces ``st["flow"]``; every other key stays, ``rigid_id``
    and ``refine_table`` are added.  ``sweeps.SweepFlow``, ``metrics.evaluate_batch`` and ``metrics_device.evaluate_batch_device`` take it as
    they take the model.  Every keyword is one of DEFAULTS."""

    def __init__(self, model, **params):
        if not callable(getattr(model, "forward_padded", None)):
            raise TypeError(f"Refined: {type(model).__name__} has no forward_padded")
        self.model = model
        self.params = check_params(params)
        self.last_state: Optional[dict] = None

    # (the commands treat the model as an nn.Module)
    def eval(self):
        self.model.eval()
        return self

    def to(self, *a, **k):
        self.model = self.model.to(*a, **k)
        return self

    def parameters(self):
        return self.model.parameters()

    def __getattr__(self, name):            # whatever else a caller asks the model (point_cloud_range, inference_dtype, timer ...)
        if name == "model":
            raise AttributeError(name)
        return getattr(self.model, name)

    def _sweeps(self, st: dict):
        """(x, count, second sweep, its count, idx_c1) of a forward_padded result: a pair model carries the compact rows, DeFlow's are
        gathered from pc0s by idx_c0 and read from its second pillar state"""
        if "points_c0" in st:
            return st["points_c0"], st["counts0"], st["points_c1"], st["counts1"], st["idx_c1"]
        # (DeFlow's idx_c0 is written for the decoded rows only: behind the count it is whatever the allocator held, so it is not an index)
        idx, N = st["idx_c0"], st["pc0s"].shape[1]
        counted = torch.arange(idx.shape[1], device=idx.device)[None] < st["counts0"][:, None]
        idx = torch.where(counted, idx, torch.zeros_like(idx)).clamp_(0, N - 1)
        x = torch.gather(st["pc0s"], 1, idx[..., None].expand(-1, -1, 3))
        p1 = st["p1"]
        return x, st["counts0"], p1.points_c, p1.counts, p1.idx_c

    def forward_padded(self, batch: Dict[str, torch.Tensor]) -> dict:
        """the inner model's result with flow [B,N,3] refined: row i < counts0[b] is the flow of input row idx_c0[b,i].  Reads nothing back."""
        st = dict(self.model.forward_padded(batch))
        x, count, pc1, count1, _ = self._sweeps(st)
        r = getattr(self.model, "point_cloud_range", None)
        rng = (r[0], r[1], r[3], r[4]) if r is not None and len(r) == 6 else None
        flow, info = rigid_refine(x, count, st["flow"].detach(), pc1, count1, grid_range=rng, **self.params)
        st.update({"flow": flow, "rigid_id": info["rigid_id"], "refine_table": info["table"]})
        self.last_state = st
        return st

    def forward(self, batch: Dict[str, torch.Tensor]):
        """the dict of lists ``DeFlow.forward`` returns (one host read: the per-sample counts)"""
        st = self.forward_padded(batch)
        x, count, pc1, count1, idx_c1 = self._sweeps(st)
        B = st["flow"].shape[0]
        m = torch.stack([count, count1]).tolist()
        m0, m1 = m[0], m[1]
        return {
            "flow": [st["flow"][b, :m0[b]] for b in range(B)],
            "pose_flow": [st["pose_flow"][b] for b in range(B)],
            "pc0_valid_point_idxes": [st["idx_c0"][b, :m0[b]] for b in range(B)],
            "pc0_points_lst": [x[b, :m0[b]] for b in range(B)],
            "pc1_valid_point_idxes": [idx_c1[b, :m1[b]] for b in range(B)],
            "pc1_points_lst": [pc1[b, :m1[b]] for b in range(B)],
        }

    def __call__(self, batch):
        return self.forward(batch)


# ---- the command ------------------------------------------------------------------------------------------------------------------------
class Wrap:
    """what ``save.main`` / ``eval.main`` take as ``wrap=``: called with the finished model (and, by save, the flow file's meta, which it
    amends) it returns the model to run"""

    def __init__(self, params: Dict[str, object]):
        self.params = dict(params)

    def __call__(self, model, meta: Optional[dict] = None):
        if meta is not None:
            meta["refine"] = dict(self.params)
            meta["definition"] = meta["definition"].replace(" (UNPINNED)", ", 6p (UNPINNED)")      # "DESIGN.md 6f[, 6x], 6p (UNPINNED)"
        return Refined(model, **self.params)


def split_args(argv: List[str]):
    """the command's arguments -> (the refine_* keys {key: value as typed}, the rest as typed, in order).  Needs no GPU."""
    own: Dict[str, str] = {}
    rest: List[str] = []
    for a in argv:
        k = a.split("=", 1)[0].lstrip("+")
        if "=" in a and k.startswith("refine_"):
            if k not in COMMAND_KEYS:
                raise SystemExit(f"unknown key {k!r}; the refine_* keys: {', '.join(COMMAND_KEYS)}")
            own[k] = a.split("=", 1)[1]
        else:
            rest.append(a)
    return own, rest


def parse_command(argv: List[str]):
    """argv -> (command, validated parameters, the wrapped command's arguments).  For ``save`` a ``res_name=`` is appended when none was
    given: what save would choose, plus ``+rigid``.  ``eval av2_mode=test`` is refused.  Needs no GPU and reads no file."""
    if not argv or argv[0] not in COMMANDS:
        raise SystemExit(USAGE)
    cmd = argv[0]
    own, rest = split_args(list(argv[1:]))
    params = params_from_command(own)
    given = {a.split("=", 1)[0].lstrip("+"): a for a in rest if "=" in a}
    if cmd == "eval" and given.get("av2_mode", "av2_mode=val") == "av2_mode=test":
        raise SystemExit("the refined flow writes no leaderboard submission (av2_mode=test is out of its scope): av2_mode=val prints its "
                         "metrics, python -m deflow_amd.refine save writes its flow")
    if cmd == "save" and "res_name" not in given:
        from . import save
        rest = rest + [f"res_name={save.parse_args(rest)['res_name']}+rigid"]
    return cmd, params, rest


def main(argv=None):
    cmd, params, rest = parse_command(list(sys.argv[1:] if argv is None else argv))
    if cmd == "save":
        from . import save
        return save.main(rest, wrap=Wrap(params))
    from . import eval as eval_
    return eval_.main(rest, wrap=Wrap(params))


if __name__ == "__main__":
    r = main()
    sys.exit(r if isinstance(r, int) else 0)
