"""Training augmentation on the GPU: flip, yaw, height, jitter and point dropout of a padded device batch in one launch
(csrc/augment.hip; the definition is in include/deflow_amd.h and DESIGN.md section 6h).

UNPINNED: upstream's later releases ship ``RandomFlip`` / ``RandomHeight`` / ``RandomJitter`` dataset transforms.  The names are recalled;
their magnitudes, probabilities and distributions are not, which is why every one is an argument here.  The jitter bell and the random
stream are this project's own.  Parity with upstream's transforms is not claimed.

Everything is a pure function of (seed, epoch, sample id, row): it does not depend on the batch a sample lands in, on its position there, on
the world size or on the number of reader workers, so a resumed run repeats exactly.  Nothing is read back to the host, and the batch that
comes in is not modified: ``Augmenter.__call__`` returns a new dict whose ``pc0`` / ``pc1`` / ``flow`` / ``ego_motion`` / ``pose0`` / ``pose1``
are new tensors and whose every other entry is the input's own object.  A dropped row is three NaNs in place -- an invalid point to the
pillariser, like the padding -- so the per-row keys aligned to pc0 / pc1 stay aligned."""
from __future__ import annotations

import math
from typing import Any, Dict, Sequence, Union

import torch

from ._lib import call, ptr, stream

Ids = Union[torch.Tensor, Sequence[int]]


class Augmenter:
    """seed: the key's first word (with the epoch of each call).  flip_x_p / flip_y_p: the probability of negating x / y; yaw_deg: the yaw
    is uniform in +-yaw_deg degrees; height: the z shift is uniform in +-height metres; jitter_sigma: the standard deviation in metres of
    the per-row, per-axis bell (bounded by 3.46 sigma); drop_p: the probability that a row is dropped."""

    def __init__(self, seed: int, flip_x_p: float = 0.5, flip_y_p: float = 0.5, yaw_deg: float = 0.0, height: float = 0.2,
                 jitter_sigma: float = 0.01, drop_p: float = 0.0):
        if int(seed) != seed:
            raise ValueError(f"Augmenter: seed must be an integer, got {seed!r}")
        for name, v in (("flip_x_p", flip_x_p), ("flip_y_p", flip_y_p), ("drop_p", drop_p)):
            if not (isinstance(v, (int, float)) and not isinstance(v, bool) and 0.0 <= v <= 1.0):    # (False for NaN)
                raise ValueError(f"Augmenter: {name} must be a probability in [0, 1], got {v!r}")
        for name, v in (("yaw_deg", yaw_deg), ("height", height), ("jitter_sigma", jitter_sigma)):
            if not (isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and 0.0 <= v <= 3.0e38):
                raise ValueError(f"Augmenter: {name} must be a finite magnitude >= 0, got {v!r}")
        self.seed = int(seed)
        self.flip_x_p, self.flip_y_p, self.yaw_deg = float(flip_x_p), float(flip_y_p), float(yaw_deg)
        self.height, self.jitter_sigma, self.drop_p = float(height), float(jitter_sigma), float(drop_p)

    def config(self) -> Dict[str, Any]:
        """every argument, as plain values"""
        return {"seed": self.seed, "flip_x_p": self.flip_x_p, "flip_y_p": self.flip_y_p, "yaw_deg": self.yaw_deg, "height": self.height,
                "jitter_sigma": self.jitter_sigma, "drop_p": self.drop_p}

    def _draw_args(self, epoch: int):
        return (self.seed, int(epoch), self.flip_x_p, self.flip_y_p, math.radians(self.yaw_deg), self.height, self.jitter_sigma, self.drop_p)

    @staticmethod
    def sample_ids_of(batch: Dict[str, Any], device=None) -> torch.Tensor:
        """the batch's ``timestamp`` list (what the scene reader's collate carries) as an int64 tensor, uploaded non-blocking"""
        if "timestamp" not in batch:
            raise KeyError("Augmenter.sample_ids_of: the batch has no 'timestamp' (scene-file batches carry one per sample)")
        ids = torch.tensor([int(t) for t in batch["timestamp"]], dtype=torch.int64)
        device = batch["pc0"].device if device is None else device
        if torch.device(device).type == "cuda":
            ids = ids.pin_memory()
        return ids.to(device, non_blocking=True)

    @staticmethod
    def _ids(sample_ids: Ids, B: int, device) -> torch.Tensor:
        if not isinstance(sample_ids, torch.Tensor):
            sample_ids = torch.tensor([int(i) for i in sample_ids], dtype=torch.int64)
        if sample_ids.dtype != torch.int64 or tuple(sample_ids.shape) != (B,):
            raise ValueError(f"Augmenter: sample_ids must be int64 of shape ({B},), got {sample_ids.dtype} {tuple(sample_ids.shape)}")
        return sample_ids.to(device, non_blocking=True).contiguous()

    @staticmethod
    def _rows(name: str, t, B=None, N=None) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise TypeError(f"Augmenter: batch[{name!r}] must be a CUDA tensor (deflow_amd has no CPU fallback)")
        if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1 or (B is not None and t.shape[0] != B) or \
                (N is not None and t.shape[1] != N):
            want = f"[{'B' if B is None else B},{'N' if N is None else N},3]"
            raise ValueError(f"Augmenter: batch[{name!r}] must be {want} with B, N >= 1, got {tuple(t.shape)}")
        return t.detach().float().contiguous()

    def params(self, sample_ids: Ids, epoch: int) -> torch.Tensor:
        """[B, 8] f32 on the device: (sx, sy, c, s, dz, theta, 0, 0) of each sample's draw"""
        if isinstance(sample_ids, torch.Tensor) and not sample_ids.is_cuda:
            raise TypeError("Augmenter.params: sample_ids must be a CUDA tensor or a sequence of integers")
        dev = sample_ids.device if isinstance(sample_ids, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        B = len(sample_ids)
        ids = self._ids(sample_ids, B, dev)
        out = torch.empty(B, 8, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("df_augment_params", ptr(ids), B, *self._draw_args(epoch), ptr(out), stream())
        return out

    def __call__(self, batch: Dict[str, Any], sample_ids: Ids, epoch: int) -> Dict[str, Any]:
        from .deflow import batch_transform
        pc0 = self._rows("pc0", batch.get("pc0"))
        B, N0, _ = pc0.shape
        dev = pc0.device
        pc1 = self._rows("pc1", batch.get("pc1"), B)
        N1 = pc1.shape[1]
        flow = self._rows("flow", batch["flow"], B, N0) if "flow" in batch else None
        ids = self._ids(sample_ids, B, dev)
        has_T = "ego_motion" in batch or ("pose0" in batch and "pose1" in batch)
        T = batch_transform(batch, dev) if has_T else None
        poses = {k: batch[k].detach().to(device=dev, dtype=torch.float32).contiguous() for k in ("pose0", "pose1") if k in batch}
        for k, m in (("ego_motion", T), *poses.items()):
            if m is not None and tuple(m.shape) != (B, 4, 4):
                raise ValueError(f"Augmenter: batch[{k!r}] must be [{B},4,4], got {tuple(m.shape)}")
        new = lambda t: None if t is None else torch.empty_like(t)
        out0, out1, oflow, oT = new(pc0), new(pc1), new(flow), new(T)
        oposes = {k: new(v) for k, v in poses.items()}
        with torch.cuda.device(dev):
            call("df_augment", ptr(pc0), ptr(pc1), ptr(flow), ptr(ids), B, N0, N1, *self._draw_args(epoch), ptr(T), ptr(poses.get("pose0")),
                 ptr(poses.get("pose1")), ptr(out0), ptr(out1), ptr(oflow), ptr(oT), ptr(oposes.get("pose0")), ptr(oposes.get("pose1")),
                 stream())
        res = dict(batch)
        res["pc0"], res["pc1"] = out0, out1
        if oflow is not None:
            res["flow"] = oflow
        if oT is not None:
            res["ego_motion"] = oT
        res.update(oposes)
        return res
