"""Leaderboard submission bodies, packed on the GPU (csrc/submit.hip; definition: include/deflow_amd.h and DESIGN.md section 6g, UNPINNED):
the step after ``sweeps.SweepFlow`` that ``python -m deflow_amd.eval av2_mode=test`` is built on.

``SweepFlow.infer`` gives the flow of every raw row of a sweep and the 0.05 m dynamic flag.  A submission file holds the benchmark's rows
only (``eval_mask``), as fp16, in Arrow's column layout with the boolean column bit-packed:

* ``pack_rows``: ``df_sweep_compact`` with ``drop = (eval_mask == 0)`` selects the rows, ``df_submit_pack`` gathers through its ``row_of``
  and writes the record-batch body of every sample byte for byte; ``feather.feather_file`` only wraps metadata around it on the host;
* ``SubmitFlow``: ``SweepFlow.infer`` (fp32) followed by ``pack_rows`` -- without a ``.tolist()``, ``.item()`` or ``.cpu()``;
* ``collate_submit_pad``: ``sweeps.collate_raw_pad`` plus ``eval0``, the first sweep's ``eval_mask``;
* ``submission_frames``: the frames of a directory's index that go into a submission;
* ``SubmissionZip``: the zip of ``<scene_id>/<timestamp>.feather`` members, byte-identical from run to run.

CUDA tensors only: there is no CPU fallback (tests/helpers/submit_ref.py restates the body layout in numpy)."""
from __future__ import annotations

import functools
import os
import zipfile
from typing import Dict, List, Optional, Tuple

import torch

from . import sweeps
from ._lib import call, ptr, stream
from .args import cloud, tensor
from .data import HDF5Dataset
from .feather import COLUMNS

ZIP_DATE_TIME = (1980, 1, 1, 0, 0, 0)      # every member's time stamp: the zip format's epoch, so that two runs give the same bytes


def body_stride(N: int) -> int:
    """bytes between two samples' bodies in ``pack_rows``' output: the body length at M = N, rounded up to 64"""
    S = int(call("df_submit_body_stride", int(N)))
    if S < 0:
        raise ValueError(f"submit: N >= 1 expected, got N = {N}")
    return S


_cuda = functools.partial(tensor, "submit", other="flow_est is")


def pack_rows(flow_est: torch.Tensor, dynamic: torch.Tensor, eval_mask: torch.Tensor, count_raw: torch.Tensor, version: int):
    """flow_est [B,N,3] f32 and dynamic [B,N] u8 as ``SweepFlow.infer`` returns them (``half=False``), eval_mask [B,N] bool / u8 (non-zero =
    a row of the benchmark), count_raw [B] i32 valid leading rows, version 1 or 2 -> body [B,S] u8 with S = ``body_stride(N)``, kept [B]
    i32.  Sample b's first ``feather.body_len(kept[b])`` bytes are the record-batch body of its selected rows, in raw order; the bytes
    behind them are not written.  Reads nothing back; two calls are bit-identical."""
    if version not in COLUMNS:
        raise ValueError(f"submit: version must be 1 or 2, got {version!r}")
    B, N = cloud("submit", "flow_est", flow_est)
    dev = flow_est.device
    flow_est = flow_est.detach().contiguous()
    dynamic = _cuda("dynamic", dynamic, (torch.uint8, torch.bool), (B, N), dev).contiguous()
    eval_mask = _cuda("eval_mask", eval_mask, (torch.bool, torch.uint8), (B, N), dev).contiguous()
    count_raw = _cuda("count_raw", count_raw, torch.int32, (B,), dev).contiguous()
    if dynamic.dtype == torch.bool:
        dynamic = dynamic.view(torch.uint8)
    S = body_stride(N)
    if B > 65535 or B * S >= 2 ** 31:
        raise ValueError(f"submit: 1 <= B <= 65535 and B * body_stride(N) < 2^31 expected, got B = {B}, N = {N}")
    # allocated before the compaction's temporaries: under a graph capture no other kernel of the graph then shares its memory, and the
    # bytes behind each sample's L(M) stay as the caller left them on every replay
    body = torch.empty(B, S, dtype=torch.uint8, device=dev)
    _, row_of, _, kept = sweeps.compact_rows(flow_est, count_raw, eval_mask == 0)
    call("df_submit_pack", ptr(flow_est), ptr(dynamic), ptr(row_of), ptr(kept), B, N, int(version), ptr(body), stream())
    return body, kept


class SubmitFlow:
    """Submission bodies of raw sweeps: ``SweepFlow(model, ground).infer`` in fp32, then ``pack_rows``."""

    def __init__(self, model, ground=None):
        self.sweep_flow = sweeps.SweepFlow(model, ground=ground)

    def infer(self, raw0: torch.Tensor, n0: torch.Tensor, drop0: Optional[torch.Tensor], raw1: torch.Tensor, n1: torch.Tensor,
              drop1: Optional[torch.Tensor], pose0: torch.Tensor, pose1: torch.Tensor, eval0: torch.Tensor,
              ego_motion: Optional[torch.Tensor] = None, version: int = 1):
        """the arguments of ``SweepFlow.infer`` and eval0 [B,N0] bool / u8, the first sweep's ``eval_mask`` -> body [B,S] u8, kept [B] i32"""
        flow_est, dynamic = self.sweep_flow.infer(raw0, n0, drop0, raw1, n1, drop1, pose0, pose1, ego_motion=ego_motion, half=False)
        return pack_rows(flow_est, dynamic, eval0, n0, version)


def collate_submit_pad(items: List[Dict[str, object]]) -> Dict[str, object]:
    """``sweeps.collate_raw_pad``'s batch and ``eval0`` [B,N0] u8: each item's ``eval_mask`` (non-zero -> 1), padded with 0.  Every item
    must carry one."""
    res = sweeps.collate_raw_pad(items)
    n = int(res["raw0"].shape[1])
    eval0 = torch.zeros(len(items), n, dtype=torch.uint8)
    for i, b in enumerate(items):
        if "eval_mask" not in b:
            raise KeyError(f"collate_submit_pad: {b.get('scene_id')} {b.get('timestamp')} has no eval_mask")
        m = torch.as_tensor(b["eval_mask"]).reshape(-1)
        if m.shape[0] != int(res["n0"][i]):
            raise ValueError(f"collate_submit_pad: {b.get('scene_id')} {b.get('timestamp')}: {m.shape[0]} eval_mask entries for "
                             f"{int(res['n0'][i])} rows")
        eval0[i, : m.shape[0]] = (m != 0).to(torch.uint8)
    res["eval0"] = eval0
    return res


class SubmissionFrames(HDF5Dataset):
    """``HDF5Dataset(directory, eval=True)`` whose ``ground_source`` may also be "online": the items then carry all-False masks and the
    caller computes them on the GPU"""

    def __init__(self, directory: str, ground_source: str = "auto"):
        super().__init__(directory, eval=True, ground_source="auto" if ground_source == "online" else ground_source)
        self.online = ground_source == "online"

    def _ground(self, scene_id, ts, group, rows):
        if self.online:
            return torch.zeros(rows, dtype=torch.bool)
        return super()._ground(scene_id, ts, group, rows)


def submission_frames(directory: str, ground_source: str = "auto"):
    """-> (dataset, skipped): the frames of ``HDF5Dataset(directory, eval=True)``'s index that go into a submission, once each and sorted
    by scene and timestamp.  A frame without ``eval_mask`` and a frame whose sweep has no successor are left out and counted (the file is
    named by the timestamp, so such a frame is not stepped back to its predecessor as the training reader does)."""
    ds = SubmissionFrames(directory, ground_source)
    unique = sorted({(str(e[0]), int(e[1])) for e in ds.data_index})
    skipped = {"duplicate": len(ds.data_index) - len(unique), "no_eval_mask": 0, "no_successor": 0}
    frames = []
    for scene_id, ts in unique:
        f = ds._file(scene_id)
        if f.sweeps.index(str(ts)) + 1 >= len(f.sweeps):
            skipped["no_successor"] += 1
        elif "eval_mask" not in f[str(ts)]:
            skipped["no_eval_mask"] += 1
        else:
            frames.append([scene_id, str(ts)])
    ds.data_index = frames
    return ds, skipped


class SubmissionZip:
    """The submission archive: ``add(scene_id, timestamp, data)`` writes ``<scene_id>/<timestamp>.feather``.  Members must arrive in sorted
    (scene_id, timestamp) order and once each; every member carries the same fixed time stamp and mode, so two runs over the same frames
    give byte-identical files.  Written to a temporary file beside ``path`` and moved into place on a clean exit."""

    def __init__(self, path: str):
        self.path = path
        self._tmp = path + ".tmp"
        self._last: Optional[Tuple[str, int]] = None
        self.members = 0

    def __enter__(self):
        self._zip = zipfile.ZipFile(self._tmp, "w", compression=zipfile.ZIP_DEFLATED)
        return self

    def add(self, scene_id: str, timestamp, data: bytes) -> str:
        key = (str(scene_id), int(timestamp))
        if not key[0] or "/" in key[0] or os.sep in key[0]:
            raise ValueError(f"SubmissionZip: bad scene id {scene_id!r}")
        if self._last is not None and key <= self._last:
            raise ValueError(f"SubmissionZip: {key} after {self._last}: members must be added once each, in sorted order")
        self._last = key
        info = zipfile.ZipInfo(f"{key[0]}/{key[1]}.feather", date_time=ZIP_DATE_TIME)
        info.compress_type = zipfile.ZIP_DEFLATED
        info.create_system = 3                     # the same header whatever platform writes it
        info.external_attr = 0o644 << 16
        self._zip.writestr(info, data)
        self.members += 1
        return info.filename

    def __exit__(self, exc_type, exc, tb):
        self._zip.close()
        if exc_type is None:
            os.replace(self._tmp, self.path)
        else:
            os.remove(self._tmp)
        return False
