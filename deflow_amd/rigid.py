"""Training-free rigid cluster flow on the GPU (``model=icpflow``): the flow of the first sweep's rows from a per-cluster rigid
registration onto the second sweep, with no weights and no checkpoint.

UNPINNED: the recipe is ICP-Flow's (Lin & Caesar, CVPR'24) -- ego-compensate, cluster both sweeps together, register every cluster
rigidly, read the flow off the transform -- but upstream's source is absent, and every choice here is this project's own.  The definition
is in include/deflow_amd.h and DESIGN.md section 6j; tests/helpers/rigid_ref.py restates it in numpy.  Joint clusters come from
``cluster.dbscan`` over the concatenated rows; csrc/rigid.hip builds the ordered row lists per cluster, votes for a translation over all
point pairs (integer counters: exact), refines yaw + translation by a fixed number of ICP iterations and writes the per-row flow.

CUDA tensors only, like the rest of the library: there is no CPU fallback.  Nothing here reads a device value back."""
from __future__ import annotations

import functools
import math
from typing import Dict, Optional, Sequence

import torch

from . import pairflow
from ._lib import call, ptr, stream
from .args import cloud, integer, merged, nonneg, positive, tensor, workspace
from .pairflow import PairFlowModel  # noqa: F401  (rigid.PairFlowModel stays importable)

STATUS_NAMES = {0: "empty", 1: "registered", 2: "one-sided", 3: "too large", 4: "inlier fraction", 5: "no vote / yaw / displacement"}
R_MAX = 64

# every default of section 6j; all of them are arguments of rigid_cluster_flow and IcpFlow, and `icp_<name>=` keys of the commands
DEFAULTS: Dict[str, object] = {"eps": 0.7, "min_points": 4, "min_cluster_size": 20, "min_side": 8, "max_cluster_points": 8192,
                               "vote_cap": 1024, "vote_bin": 0.2, "max_disp": 3.4, "icp_cap": 2048, "icp_iters": 8, "icp_max_dist": 0.5,
                               "min_inlier_frac": 0.6, "max_yaw": 0.35}


# the commands' keys (save, eval): icp_<name>, the three names that start with icp_ already as they are
COMMAND_KEYS: Dict[str, str] = {(k if k.startswith("icp_") else "icp_" + k): k for k in DEFAULTS}
COMMAND_BATCH_SIZE = None   # the commands' batch_size has no default of this model's own


def params_from_command(given: Dict[str, str]) -> Dict[str, object]:
    return pairflow.params_from_command(pairflow.entry("icpflow"), given)


def vote_radius(max_disp: float, vote_bin: float) -> int:
    """R = ceil(max_disp / vote_bin) with both rounded to fp32 first and the quotient taken in double (3.4 / 0.2: 17)"""
    import numpy as np
    q = float(np.float32(max_disp)) / float(np.float32(vote_bin))
    return int(math.ceil(q - 1e-6))


def check_params(p: Dict[str, object]) -> Dict[str, object]:
    """validated copy of a parameter dict (ValueError naming the argument); launches nothing"""
    fn = "rigid_cluster_flow"
    out = merged(fn, DEFAULTS, p)
    for k in ("min_points", "min_cluster_size", "min_side", "max_cluster_points"):
        integer(fn, out, k, 1, 1 << 30)
    for k in ("vote_cap", "icp_cap"):
        integer(fn, out, k, 1, 1 << 20)
    integer(fn, out, "icp_iters", 0, 1024)
    for k in ("eps", "vote_bin", "icp_max_dist"):
        positive(fn, out, k)
    for k in ("max_disp", "max_yaw", "min_inlier_frac"):
        nonneg(fn, out, k)
    if vote_radius(out["max_disp"], out["vote_bin"]) > R_MAX:
        raise ValueError(f"rigid_cluster_flow: max_disp / vote_bin must be at most {R_MAX} bins, got max_disp = {out['max_disp']}, "
                         f"vote_bin = {out['vote_bin']}")
    return out


_check = functools.partial(tensor, "rigid_cluster_flow", other="pc0s is")


def segments(fn: str, name: str, labels: torch.Tensor, count: torch.Tensor, K: int, status: Optional[torch.Tensor] = None):
    """The ordered row lists of ONE cloud's clusters: labels [B,N] i32 (checked by the caller; 0: no cluster, 1..K), count [B] i32 ->
    (labels with the rows behind the count set to 0, seg_off [B, 2K + 1] i32, seg_rows [B, N + 1] i32): df_rigid_segments with N0 = N,
    N1 = 1 on the labels followed by one zero column.  status: i32[1] that is added to for a label outside [0, K].  fn / name: the
    function and the argument a refusal names."""
    B, N = int(labels.shape[0]), int(labels.shape[1])
    dev = labels.device
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    counted = torch.arange(N, device=dev)[None] < count.clamp(0, N)[:, None]
    lab = torch.where(counted, labels, torch.zeros_like(labels)).contiguous()
    ext = torch.zeros(B, N + 1, dtype=torch.int32, device=dev)
    ext[:, :N] = lab
    ws = workspace("df_rigid_segments_ws_bytes", (B, N, 1, K), dev,
                   f"{fn}: {name}: df_rigid_segments_ws_bytes refused B = {B}, N = {N}, kcap = {K}")
    seg_off = torch.empty(B, 2 * K + 1, dtype=torch.int32, device=dev)
    seg_rows = torch.empty(B, N + 1, dtype=torch.int32, device=dev)
    call("df_rigid_segments", ptr(ext), B, N, 1, K, ptr(seg_off), ptr(seg_rows), ptr(status), ptr(ws), stream())
    return lab, seg_off, seg_rows


def kcap(N0: int, N1: int, min_cluster_size: int) -> int:
    """cluster slots per sample: every cluster has at least min_cluster_size rows, so no more than this many exist"""
    return max((N0 + N1) // int(min_cluster_size), 1)


def joint_labels(pc0s: torch.Tensor, count0: torch.Tensor, pc1: torch.Tensor, count1: torch.Tensor, *, eps: float, min_points: int,
                 min_cluster_size: int, grid_range: Optional[Sequence[float]] = None, status: Optional[torch.Tensor] = None):
    """DBSCAN labels [B,N0+N1] i32 of the concatenation (pc0s rows, then pc1 rows); rows behind either count take no part"""
    from .cluster import dbscan
    B, N0, N1 = pc0s.shape[0], pc0s.shape[1], pc1.shape[1]
    dev = pc0s.device
    pts = torch.cat([pc0s, pc1], dim=1)
    r0 = torch.arange(N0, device=dev, dtype=torch.int32)
    r1 = torch.arange(N1, device=dev, dtype=torch.int32)
    mask = torch.cat([r0[None, :] < count0[:, None], r1[None, :] < count1[:, None]], dim=1)
    full = torch.full((B,), N0 + N1, dtype=torch.int32, device=dev)
    labels, _ = dbscan(pts, full, mask, eps=eps, min_points=min_points, min_cluster_size=min_cluster_size, grid_range=grid_range,
                       status=status)
    return labels


def rigid_cluster_flow(pc0s: torch.Tensor, count0: torch.Tensor, pc1: torch.Tensor, count1: torch.Tensor, *, eps: float = 0.7,
                       min_points: int = 4, min_cluster_size: int = 20, min_side: int = 8, max_cluster_points: int = 8192,
                       vote_cap: int = 1024, vote_bin: float = 0.2, max_disp: float = 3.4, icp_cap: int = 2048, icp_iters: int = 8,
                       icp_max_dist: float = 0.5, min_inlier_frac: float = 0.6, max_yaw: float = 0.35,
                       grid_range: Optional[Sequence[float]] = None, labels: Optional[torch.Tensor] = None, return_hist: bool = False):
    """pc0s [B,N0,3] f32 (first sweep, ground removed, in the second sweep's frame) with count0 [B] i32 valid leading rows; pc1 [B,N1,3],
    count1 alike.  -> flow [B,N0,3] f32 (the residual flow on top of the pose flow; 0 for rows of no registered cluster), rigid_id [B,N0] i32
    (the cluster slot 1..Kcap of a registered row, else 0), table [B,Kcap,8] f32 (theta, tx, ty, tz, inlier_frac, n_src, n_dst, status),
    vote [B,Kcap,3] i32 (ix, iy, count), status i32[1] (0 unless a bounded loop hit its bound); with return_hist also the whole vote
    histogram [B,Kcap,2R+1,2R+1] i32 as a sixth value.  Kcap = max((N0+N1) // min_cluster_size, 1).
    labels: the joint labels [B,N0+N1] i32 when the caller has them already (else cluster.dbscan computes them); grid_range as in dbscan.
    No host synchronisation; workspaces come from torch's allocator; two calls are bit-identical."""
    (B, N0), (_, N1) = cloud("rigid_cluster_flow", "pc0s", pc0s), cloud("rigid_cluster_flow", "pc1", pc1)
    dev = pc0s.device
    if pc1.shape[0] != B:
        raise ValueError(f"rigid_cluster_flow: pc1 must have the batch size of pc0s ({B}), got {tuple(pc1.shape)}")
    if pc1.device != dev:
        raise ValueError(f"rigid_cluster_flow: pc1 is on {pc1.device}, pc0s is on {dev}")
    _check("count0", count0, torch.int32, (B,), dev)
    _check("count1", count1, torch.int32, (B,), dev)
    p = check_params({"eps": eps, "min_points": min_points, "min_cluster_size": min_cluster_size, "min_side": min_side,
                      "max_cluster_points": max_cluster_points, "vote_cap": vote_cap, "vote_bin": vote_bin, "max_disp": max_disp,
                      "icp_cap": icp_cap, "icp_iters": icp_iters, "icp_max_dist": icp_max_dist, "min_inlier_frac": min_inlier_frac,
                      "max_yaw": max_yaw})
    N = N0 + N1
    if B > 65535 or B * N >= 2 ** 31:
        raise ValueError(f"rigid_cluster_flow: 1 <= B <= 65535 and B * (N0 + N1) < 2^31 expected, got B = {B}, N0 = {N0}, N1 = {N1}")
    K = kcap(N0, N1, p["min_cluster_size"])
    R = vote_radius(p["max_disp"], p["vote_bin"])
    if labels is not None:
        _check("labels", labels, torch.int32, (B, N), dev)
    pc0s, pc1 = pc0s.detach().contiguous(), pc1.detach().contiguous()
    count0, count1 = count0.contiguous(), count1.contiguous()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if labels is None:
        labels = joint_labels(pc0s, count0, pc1, count1, eps=p["eps"], min_points=p["min_points"],
                              min_cluster_size=p["min_cluster_size"], grid_range=grid_range, status=status)
    labels = labels.contiguous()

    ws = lambda entry, *a: workspace(entry, a, dev, f"rigid_cluster_flow: {entry} refused B = {B}, N0 = {N0}, N1 = {N1}")
    seg_ws, icp_ws = ws("df_rigid_segments_ws_bytes", B, N0, N1, K), ws("df_rigid_icp_ws_bytes", B, N0, N1)
    seg_off = torch.empty(B, 2 * K + 1, dtype=torch.int32, device=dev)
    seg_rows = torch.empty(B, N, dtype=torch.int32, device=dev)
    vote = torch.empty(B, K, 3, dtype=torch.int32, device=dev)
    hist = torch.empty(B, K, 2 * R + 1, 2 * R + 1, dtype=torch.int32, device=dev) if return_hist else None
    table = torch.empty(B, K, 8, dtype=torch.float32, device=dev)
    flow = torch.empty(B, N0, 3, dtype=torch.float32, device=dev)
    rigid_id = torch.empty(B, N0, dtype=torch.int32, device=dev)
    s = stream()
    call("df_rigid_segments", ptr(labels), B, N0, N1, K, ptr(seg_off), ptr(seg_rows), ptr(status), ptr(seg_ws), s)
    call("df_rigid_vote", ptr(pc0s), ptr(pc1), ptr(seg_off), ptr(seg_rows), B, N0, N1, K, p["min_side"], p["max_cluster_points"],
         p["vote_cap"], p["vote_bin"], R, ptr(vote), ptr(hist), s)
    call("df_rigid_icp", ptr(pc0s), ptr(pc1), ptr(seg_off), ptr(seg_rows), ptr(vote), B, N0, N1, K, p["min_side"], p["max_cluster_points"],
         p["icp_cap"], p["icp_iters"], p["vote_bin"], p["icp_max_dist"], p["min_inlier_frac"], p["max_yaw"], p["max_disp"], ptr(table),
         ptr(icp_ws), s)
    call("df_rigid_apply", ptr(pc0s), ptr(count0), ptr(labels), ptr(seg_off), ptr(seg_rows), ptr(table), B, N0, N1, K, ptr(flow),
         ptr(rigid_id), s)
    if return_hist:
        return flow, rigid_id, table, vote, status, hist
    return flow, rigid_id, table, vote, status


class IcpFlow(PairFlowModel):
    """``model=icpflow``: an object with the two methods of ``DeFlow`` the commands use -- ``forward_padded`` and ``forward`` -- and no
    weights.  ``sweeps.SweepFlow``, ``metrics.evaluate_batch`` and ``metrics_device.evaluate_batch_device`` take it as they take the model.
    point_cloud_range / voxel_size decide which rows count as decoded, by the voxeliser's rule (floor((p - min) / voxel) inside the grid on
    all three axes, on the ego-compensated rows); every other keyword is a parameter of ``rigid_cluster_flow``."""

    def __init__(self, point_cloud_range=(-51.2, -51.2, -3, 51.2, 51.2, 3), voxel_size=(0.2, 0.2, 6), **params):
        super().__init__(point_cloud_range, voxel_size)
        self.params = check_params(params)

    def forward_padded(self, batch: Dict[str, torch.Tensor]) -> dict:
        """flow [B,N,3]: row i < counts0[b] is the flow of input row idx_c0[b,i] (the decoded rows in ascending order), 0 behind them;
        pose_flow [B,N,3] of every input row; pc0s the ego-compensated rows.  Reads nothing back."""
        st = self._pair(batch)
        r = self.point_cloud_range
        flow, rigid_id, table, vote, status = rigid_cluster_flow(st["points_c0"], st["counts0"], st["points_c1"], st["counts1"],
                                                                 grid_range=(r[0], r[1], r[3], r[4]), **self.params)
        st.update({"flow": flow, "rigid_id": rigid_id, "table": table, "vote": vote, "status": status})
        self.last_state = st
        return st
