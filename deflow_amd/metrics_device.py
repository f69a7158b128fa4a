"""The validation metrics of deflow_amd/metrics.py accumulated on the GPU (csrc/metrics.hip; definition: include/deflow_amd.h and
DESIGN.md section 6e): ``DeviceMetrics`` is fed a whole padded batch per call -- what ``DeFlow.forward_padded`` leaves on the device plus
the batch's labels -- and reads nothing back until ``result()`` / ``summary()`` / ``table()``.  It produces the tables of
``OfficialMetrics`` (both leaderboard versions) and the range-free summary ``eval.py`` prints as ``metrics``.

Not the same bits as the host path: the host's summary (``epe_metrics``) works in fp32 and ``torch.norm`` rounds differently from the
fixed sequence used here, so a row sitting on a threshold can fall on the other side; the float64 restatement in
tests/helpers/metrics_batch_ref.py is what the kernels are pinned to.  CUDA tensors only: there is no CPU fallback."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ._lib import call, ptr, stream
from .args import tensor, ws_bytes
from .metrics import BUCKET_WIDTH, META_CLASSES, N_BUCKETS, N_CATEGORIES, OfficialMetrics

SUMMARY_KEYS = ("EPE", "AccS", "AccR", "n", "EPE_FD", "EPE_FS", "EPE_BS", "EPE_3way")
_NC = len(META_CLASSES) * N_BUCKETS
_NV1 = len(OfficialMetrics.V1_KEYS)
# the state's layout (include/deflow_amd.h): doubles v1_sum, err_sum, speed_sum, tot; int64 v1_cnt, n, count, wsum
_NF = _NV1 + 2 * _NC + len(SUMMARY_KEYS)
_NI = _NV1 + 1 + _NC + len(SUMMARY_KEYS)


def rows_per_block() -> int:
    """compact rows one block of df_metrics_rows walks (tests straddle it)"""
    return int(call("df_metrics_rows_per_block"))


def _tensor(name: str, t, device) -> torch.Tensor:
    return tensor("DeviceMetrics", name, t, device=device, other="the accumulator is")


def _rows3(name: str, t, B: int, N: int, device) -> torch.Tensor:
    t = _tensor(name, t, device)
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != B or t.shape[1] != N or t.shape[2] < 3 or (name != "pc0" and t.shape[2] != 3):
        raise ValueError(f"DeviceMetrics: {name} must be torch.float32 of shape ({B}, {N}, 3), got {t.dtype} {tuple(t.shape)}")
    return t.detach()[..., :3].contiguous()


def _u8(name: str, t, shape, device, clamp: Optional[int] = None) -> Optional[torch.Tensor]:
    """optional per-point (or per-sample) mask / label -> u8 on the device; bool and integer dtypes only"""
    if t is None:
        return None
    t = _tensor(name, t, device)
    if tuple(t.shape) != tuple(shape) or t.dtype.is_floating_point or t.dtype.is_complex:
        raise ValueError(f"DeviceMetrics: {name} must be a bool or integer tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    if t.dtype == torch.bool:
        return t.contiguous().view(torch.uint8)
    if clamp is not None:                       # labels: clamped BEFORE they are narrowed
        return t.contiguous() if t.dtype == torch.uint8 else t.clamp(0, clamp).to(torch.uint8).contiguous()
    return t.contiguous() if t.dtype == torch.uint8 else (t != 0).view(torch.uint8)


class DeviceMetrics:
    """Device-resident accumulator of the Argoverse-2 validation tables and the range-free summary; all state is sums and counts."""

    V1_KEYS = OfficialMetrics.V1_KEYS

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise TypeError("DeviceMetrics: device must be a CUDA device (deflow_amd has no CPU fallback)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else device
        self.device = device
        # one buffer, so that result() is one read: _NF doubles, then _NI int64
        self._state = torch.zeros(_NF + _NI, dtype=torch.int64, device=device)
        self._sf = self._state[:_NF].view(torch.float64)
        self._si = self._state[_NF:]
        self._status = torch.zeros(1, dtype=torch.int32, device=device)
        self._edges = torch.from_numpy(np.arange(1, N_BUCKETS, dtype=np.float64) * BUCKET_WIDTH).to(device)    # k * 2.0 / 50, k = 1 .. 50
        self._ws: Optional[torch.Tensor] = None

    # ---- feeding ------------------------------------------------------------------------------------------------------------------------
    def reserve(self, B: int, N: int) -> None:
        """make the workspace large enough for [B, N] batches (update() does it itself, but never inside a stream capture)"""
        need = ws_bytes("df_metrics_ws_bytes", (int(B), int(N)),
                        f"DeviceMetrics: 1 <= B <= 65535, N >= 1 and B * N < 2^31 expected, got B = {B}, N = {N}")
        if self._ws is None or self._ws.numel() * 8 < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DeviceMetrics: the workspace would have to grow inside a stream capture; call reserve(B, N) or one "
                                   "eager update() of this shape first")
            self._ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=self.device)

    def update(self, flow: torch.Tensor, pose_flow: torch.Tensor, pc0: torch.Tensor, gt_flow: torch.Tensor, idx_c: torch.Tensor,
               counts: torch.Tensor, *, is_valid: Optional[torch.Tensor] = None, eval_mask: Optional[torch.Tensor] = None,
               categories: Optional[torch.Tensor] = None, has_eval_mask: Optional[torch.Tensor] = None) -> None:
        """One padded batch: flow [B,N,3] f32 whose rows i < counts[b] are the model's flow of the points idx_c[b,i] (i64 [B,N]);
        pose_flow, pc0 (sensor frame of the first sweep, untransformed; further columns are ignored), gt_flow [B,N,3] f32 and the optional
        is_valid, eval_mask (bool / integer, != 0 counts) and categories (integer, clamped to 0..30) [B,N] are indexed by point; counts [B]
        i32; has_eval_mask [B] as collate_fn_pad writes it.  Reads nothing back."""
        flow = _tensor("flow", flow, self.device)
        if flow.dim() != 3:
            raise ValueError(f"DeviceMetrics: flow must be torch.float32 of shape (B, N, 3), got {tuple(flow.shape)}")
        B, N = int(flow.shape[0]), int(flow.shape[1])
        flow = _rows3("flow", flow, B, N, self.device)
        pose_flow = _rows3("pose_flow", pose_flow, B, N, self.device)
        pc0 = _rows3("pc0", pc0, B, N, self.device)
        gt_flow = _rows3("gt_flow", gt_flow, B, N, self.device)
        idx_c = _tensor("idx_c", idx_c, self.device)
        if idx_c.dtype != torch.int64 or tuple(idx_c.shape) != (B, N):
            raise ValueError(f"DeviceMetrics: idx_c must be torch.int64 of shape ({B}, {N}), got {idx_c.dtype} {tuple(idx_c.shape)}")
        counts = _tensor("counts", counts, self.device)
        if counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
            raise ValueError(f"DeviceMetrics: counts must be torch.int32 of shape ({B},), got {counts.dtype} {tuple(counts.shape)}")
        is_valid = _u8("is_valid", is_valid, (B, N), self.device)
        eval_mask = _u8("eval_mask", eval_mask, (B, N), self.device)
        categories = _u8("categories", categories, (B, N), self.device, clamp=N_CATEGORIES - 1)
        has_eval_mask = _u8("has_eval_mask", has_eval_mask, (B,), self.device)
        self.reserve(B, N)
        idx_c, counts = idx_c.contiguous(), counts.contiguous()
        s = stream()
        call("df_metrics_rows", ptr(flow), ptr(pose_flow), ptr(pc0), ptr(gt_flow), ptr(idx_c), ptr(counts), ptr(is_valid), ptr(eval_mask),
             ptr(categories), B, N, ptr(self._edges), ptr(self._ws), ptr(self._status), s)
        call("df_metrics_accumulate", ptr(counts), ptr(has_eval_mask), B, N, ptr(self._ws), ptr(self._sf), ptr(self._si), s)

    # ---- state --------------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _views(sf: torch.Tensor, si: torch.Tensor) -> Dict[str, torch.Tensor]:
        nb = len(META_CLASSES)
        return {"v1_sum": sf[:_NV1], "err_sum": sf[_NV1:_NV1 + _NC].view(nb, N_BUCKETS),
                "speed_sum": sf[_NV1 + _NC:_NV1 + 2 * _NC].view(nb, N_BUCKETS), "tot": sf[_NV1 + 2 * _NC:],
                "v1_cnt": si[:_NV1], "n": si[_NV1:_NV1 + 1], "count": si[_NV1 + 1:_NV1 + 1 + _NC].view(nb, N_BUCKETS),
                "wsum": si[_NV1 + 1 + _NC:]}

    def state(self) -> Dict[str, torch.Tensor]:
        """the raw device tensors (views of one buffer): v1_sum / v1_cnt [8] in V1_KEYS order, n [1], err_sum / speed_sum / count [5,51],
        tot / wsum [8] in SUMMARY_KEYS order"""
        return self._views(self._sf, self._si)

    @property
    def status(self) -> torch.Tensor:
        """i32[1] on the device: the number of rows dropped because their idx_c entry was outside [0, N)"""
        return self._status

    def reset(self) -> None:
        self._state.zero_()
        self._status.zero_()

    def merge_(self, other: "DeviceMetrics") -> "DeviceMetrics":
        """add another accumulator's sums and counts to this one"""
        if not isinstance(other, DeviceMetrics):
            raise TypeError("DeviceMetrics: merge_ takes another DeviceMetrics")
        self._sf += other._sf.to(self.device)
        self._si += other._si.to(self.device)
        self._status += other._status.to(self.device)
        return self

    def _host(self) -> Dict[str, torch.Tensor]:
        h = self._state.cpu()                   # the one read
        return self._views(h[:_NF].view(torch.float64), h[_NF:])

    def _official(self) -> OfficialMetrics:
        """the host accumulator holding this state: its result() / table() are the final arithmetic and the formats"""
        h = self._host()
        om = OfficialMetrics()
        om.v1_sum = {k: float(h["v1_sum"][i]) for i, k in enumerate(self.V1_KEYS)}
        om.v1_cnt = {k: int(h["v1_cnt"][i]) for i, k in enumerate(self.V1_KEYS)}
        om.n = int(h["n"][0])
        om.err_sum, om.speed_sum, om.count = h["err_sum"].clone(), h["speed_sum"].clone(), h["count"].clone()
        return om

    def result(self, leaderboard_version: int = 1) -> Dict[str, float]:
        return self._official().result(leaderboard_version)

    def table(self, leaderboard_version: int = 1) -> str:
        return self._official().table(leaderboard_version)

    def summary(self) -> Dict[str, float]:
        """the range-free summary over everything fed so far, weighted by batch size as eval.py weights evaluate_batch's returns: per
        update() the mean of each key over the samples that have it, times B; a key no sample ever had is absent"""
        h = self._host()
        return {k: float(h["tot"][i]) / int(h["wsum"][i]) for i, k in enumerate(SUMMARY_KEYS) if int(h["wsum"][i]) > 0}


def evaluate_batch_device(model, batch: dict, dm: DeviceMetrics) -> None:
    """One validation iteration without a host sync: ``model.forward_padded(batch)`` under no_grad, then ``dm.update`` from its
    ``last_state`` and the batch's labels (``flow``; ``flow_is_valid``, ``eval_mask``, ``flow_category_indices``, ``has_eval_mask`` when
    present) -- the device counterpart of ``evaluate_batch(model(batch), batch, official)``."""
    with torch.no_grad():
        st = model.forward_padded(batch)
        dm.update(st["flow"].detach(), st["pose_flow"], batch["pc0"].float(), batch["flow"].float(), st["idx_c0"], st["counts0"],
                  is_valid=batch.get("flow_is_valid"), eval_mask=batch.get("eval_mask"), categories=batch.get("flow_category_indices"),
                  has_eval_mask=batch.get("has_eval_mask"))
