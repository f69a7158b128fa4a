"""The flow of every row of a raw sweep, put together on the GPU (csrc/sweep.hip; definition: include/deflow_amd.h and DESIGN.md section
6f, UNPINNED): the step after the model that ``python -m deflow_amd.save`` is built on.

``DeFlow.forward`` answers for the rows the model decoded -- not ground, finite, inside the range -- of a batch whose ground rows
``collate_fn_pad`` removed on the CPU, so the way back to the rows of ``lidar`` is lost.  Here the raw sweep goes to the device once:

* ``compact_rows``: the ground rows are removed there (stable; the same bits as ``collate_fn_pad``'s ``pc0``), and both index maps stay;
* ``compose_flow``: pose flow + the model's flow for the decoded rows, the pose flow alone for every other finite row, zeros for
  non-finite and padded rows, and a dynamic flag from the model's flow;
* ``SweepFlow``: compaction of both sweeps, ``model.forward_padded``, composition -- without a ``.tolist()``, ``.item()`` or ``.cpu()``;
* ``collate_raw_pad``: ``HDF5Dataset`` items -> the NaN-padded raw batch ``SweepFlow.infer`` takes.

CUDA tensors only: there is no CPU fallback (tests/helpers/sweep_flow_ref.py restates the definition in numpy)."""
from __future__ import annotations

import functools
from typing import Dict, List, Optional

import torch

from ._lib import call, ptr, stream
from .args import cloud, tensor, workspace


def rows_per_block() -> int:
    """raw rows one block of df_sweep_compact walks (tests straddle it)"""
    return int(call("df_sweep_rows_per_block"))


_check = functools.partial(tensor, "sweeps", other="raw is")
_raw = functools.partial(cloud, "sweeps", "raw")


def _mask(name: str, t, shape, device) -> torch.Tensor:
    """bool or uint8 [B,N] -> u8 (non-zero = set)"""
    t = _check(name, t, (torch.bool, torch.uint8), shape, device).contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def _workspace(entry: str, B: int, N: int, device) -> torch.Tensor:
    return workspace(entry + "_ws_bytes", (B, N), device, f"sweeps: 1 <= B <= 65535, N >= 1 and B * N < 2^31 expected, got B = {B}, N = {N}")


def compact_rows(raw: torch.Tensor, count_raw: torch.Tensor, drop: torch.Tensor):
    """raw [B,N,3] f32, count_raw [B] i32 valid leading rows, drop [B,N] bool / u8 (non-zero = ground) ->
    pc [B,N,3] f32: the kept rows (r < count_raw[b], not dropped) first, in order, then NaN rows -- ``collate_fn_pad``'s ``pc0``, bit for bit;
    row_of [B,N] i32: the raw row of each kept row, -1 in the padding; pos_of [B,N] i32: the compact position of each raw row, -1 for
    dropped and padded rows; kept [B] i32.  Reads nothing back."""
    B, N = _raw(raw)
    dev = raw.device
    _check("count_raw", count_raw, torch.int32, (B,), dev)
    drop = _mask("drop", drop, (B, N), dev)
    raw, count_raw = raw.detach().contiguous(), count_raw.contiguous()
    ws = _workspace("df_sweep_compact", B, N, dev)
    pc = torch.empty_like(raw)
    row_of = torch.empty(B, N, dtype=torch.int32, device=dev)
    pos_of = torch.empty(B, N, dtype=torch.int32, device=dev)
    kept = torch.empty(B, dtype=torch.int32, device=dev)
    call("df_sweep_compact", ptr(raw), ptr(count_raw), ptr(drop), B, N, ptr(ws), ptr(pc), ptr(row_of), ptr(pos_of), ptr(kept), stream())
    return pc, row_of, pos_of, kept


def compose_flow(raw: torch.Tensor, count_raw: torch.Tensor, T: torch.Tensor, pos_of: torch.Tensor, flow: torch.Tensor,
                 idx_c: torch.Tensor, counts: torch.Tensor, half: bool = False):
    """raw, count_raw, pos_of as in ``compact_rows``; T [B,4,4] f32; the forward's flow [B,Nc,3] f32, idx_c [B,Nc] i64 (compact position of
    decoded row i) and counts [B] i32 -> flow_est [B,N,3] f32 (f16 with ``half``), dynamic [B,N] u8, every element written.  Reads nothing
    back; two calls are bit-identical."""
    B, N = _raw(raw)
    dev = raw.device
    _check("count_raw", count_raw, torch.int32, (B,), dev)
    _check("T", T, torch.float32, (B, 4, 4), dev)
    _check("pos_of", pos_of, torch.int32, (B, N), dev)
    _check("flow", flow)
    if flow.dim() != 3 or flow.shape[0] != B or flow.shape[1] < 1 or flow.shape[2] != 3:
        raise ValueError(f"sweeps: flow must be torch.float32 of shape ({B}, Nc, 3) with Nc >= 1, got {flow.dtype} {tuple(flow.shape)}")
    Nc = int(flow.shape[1])
    _check("flow", flow, torch.float32, (B, Nc, 3), dev)
    _check("idx_c", idx_c, torch.int64, (B, Nc), dev)
    _check("counts", counts, torch.int32, (B,), dev)
    raw, flow = raw.detach().contiguous(), flow.detach().contiguous()
    count_raw, T, pos_of, idx_c, counts = count_raw.contiguous(), T.contiguous(), pos_of.contiguous(), idx_c.contiguous(), counts.contiguous()
    ws = _workspace("df_flow_compose", B, N, dev)
    flow_est = torch.empty(B, N, 3, dtype=torch.float16 if half else torch.float32, device=dev)
    dynamic = torch.empty(B, N, dtype=torch.uint8, device=dev)
    call("df_flow_compose", ptr(raw), ptr(count_raw), ptr(T), ptr(pos_of), ptr(flow), ptr(idx_c), ptr(counts), B, N, Nc, int(bool(half)),
         ptr(ws), ptr(flow_est), ptr(dynamic), stream())
    return flow_est, dynamic


class SweepFlow:
    """The flow of all rows of raw sweeps: compaction, ``model.forward_padded``, composition.  ``ground``: a ``GroundSegmenter`` of the
    batch size; with one, ``drop0`` / ``drop1`` may be None and the masks come from ``segment()`` on the raw rows (first sweep, then second),
    which needs no mask on disk."""

    def __init__(self, model, ground=None):
        self.model, self.ground = model, ground

    def _drop(self, name: str, raw: torch.Tensor, n: torch.Tensor, drop: Optional[torch.Tensor]) -> torch.Tensor:
        if drop is not None:
            return drop
        if self.ground is None:
            raise ValueError(f"SweepFlow: {name} is None and there is no ground segmenter to compute it (SweepFlow(model, ground=...))")
        return self.ground.segment(raw, n)

    def infer(self, raw0: torch.Tensor, n0: torch.Tensor, drop0: Optional[torch.Tensor], raw1: torch.Tensor, n1: torch.Tensor,
              drop1: Optional[torch.Tensor], pose0: torch.Tensor, pose1: torch.Tensor, ego_motion: Optional[torch.Tensor] = None,
              half: bool = False):
        """raw0 / raw1 [B,N0,3] / [B,N1,3] f32 with n0 / n1 [B] i32 valid leading rows and drop0 / drop1 [B,N] ground masks; pose0, pose1
        (and ego_motion, which wins) [B,4,4] -> flow_est [B,N0,3], dynamic [B,N0] u8 of the first sweep's rows."""
        from .deflow import batch_transform
        _raw(raw0), _raw(raw1)
        pc0, _, pos0, _ = compact_rows(raw0, n0, self._drop("drop0", raw0, n0, drop0))
        pc1, _, _, _ = compact_rows(raw1, n1, self._drop("drop1", raw1, n1, drop1))
        poses = {"pose0": pose0, "pose1": pose1}
        if ego_motion is not None:
            poses["ego_motion"] = ego_motion
        # the transform is formed once, by the function forward_padded forms it with, and handed to the model as the batch's ego_motion
        # (which forward_padded takes as it is): the model's pose flow and the composed one come from the same 16 floats per sample
        T = batch_transform(poses, raw0.device)
        with torch.no_grad():
            st = self.model.forward_padded({"pc0": pc0, "pc1": pc1, **poses, "ego_motion": T})
            return compose_flow(raw0, n0, T, pos0, st["flow"].detach(), st["idx_c0"], st["counts0"], half=half)


def collate_raw_pad(items: List[Dict[str, object]]) -> Dict[str, object]:
    """``HDF5Dataset`` items (which carry the unfiltered ``pc0 gm0 pc1 gm1``) -> ``raw0`` / ``raw1`` [B,N,3] f32 padded with NaN rows to
    max(longest, 1), ``drop0`` / ``drop1`` [B,N] u8 padded with 0, ``n0`` / ``n1`` [B] i32, ``pose0`` / ``pose1`` (``ego_motion`` when the
    items have it) [B,4,4] f32, ``scene_id``, ``timestamp``.  Nothing is removed: ``SweepFlow`` does that on the device."""
    res: Dict[str, object] = {}
    for g in ("0", "1"):
        rows = [int(b["pc" + g].shape[0]) for b in items]
        n = max(max(rows), 1)
        raw = torch.full((len(items), n, 3), float("nan"), dtype=torch.float32)
        drop = torch.zeros(len(items), n, dtype=torch.uint8)
        for i, b in enumerate(items):
            raw[i, : rows[i]] = b["pc" + g][:, :3].float()
            drop[i, : rows[i]] = (b["gm" + g].reshape(-1) != 0).to(torch.uint8)
        res["raw" + g], res["drop" + g], res["n" + g] = raw, drop, torch.tensor(rows, dtype=torch.int32)
    res["pose0"] = torch.stack([b["pose0"].float() for b in items])
    res["pose1"] = torch.stack([b["pose1"].float() for b in items])
    if "ego_motion" in items[0]:
        res["ego_motion"] = torch.stack([b["ego_motion"].float() for b in items])
    res["scene_id"] = [b["scene_id"] for b in items]
    res["timestamp"] = [b["timestamp"] for b in items]
    return res
