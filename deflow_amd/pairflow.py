"""The checkpoint-free pair models (``model=icpflow|nsfp|fastnsf|mbnsf|floxels``) as the commands see them: one table, and what the
models share -- their base class, the commands' configuration and key refusals, and the parameter checks.

``TABLE`` has one line per model with what differs between them; the rest (``COMMAND_KEYS``, ``DEFAULTS``, ``COMMAND_BATCH_SIZE``,
``check_params``) is read from the model's own module, imported on first use.  ``deflow_amd.eval`` and ``deflow_amd.save`` name these
models through the table only: one more model is its own module and one more line here.  Nothing here needs a GPU
but ``PairFlowModel._pair``."""
from __future__ import annotations

import ast
import importlib
from typing import Dict, Iterable, NamedTuple, Optional, Tuple

import torch

from ._lib import call, ptr, stream
from .args import flag, integer, merged, nonneg, positive  # noqa: F401


class Entry(NamedTuple):
    name: str      # the model= value, and the default res_name
    module: str    # deflow_amd.<module>
    cls: str       # the model class in it
    prefix: str    # the commands' keys are <prefix>_<parameter>
    section: str   # DESIGN.md section, for the flow file's meta["definition"]
    memory: str    # the note that ends the save command's usage text


TABLE: Tuple[Entry, ...] = (
    Entry("icpflow", "rigid", "IcpFlow", "icp", "6j", ""),
    Entry("nsfp", "nsfp", "Nsfp", "nsfp", "6k",
          "batch_size defaults to 2: the saved activations are (nsfp_depth + 1) x N x 512 bytes per net evaluation and sample"),
    Entry("fastnsf", "fastnsf", "FastNsf", "fastnsf", "6l",
          "batch_size defaults to 4: per sample the distance-transform grid (2 bytes per voxel of point_cloud_range / fastnsf_cell, twice "
          "while it is built) and the saved activations, (fastnsf_depth + 1) x N x 512 bytes, twice during the backward"),
    Entry("mbnsf", "mbnsf", "MbNsf", "mbnsf", "6m",
          "batch_size defaults to 4: model=fastnsf's memory per sample plus the neighbour table, N x 2 mbnsf_rigid_pairs x 8 bytes"),
    Entry("floxels", "floxels", "Floxels", "floxels", "6n",
          "batch_size defaults to 4: per sample the distance-transform grid (2 bytes per voxel of point_cloud_range / floxels_cell, twice "
          "while it is built); the field and its five companions are 12 bytes per node of point_cloud_range / floxels_voxel each"),
)


def entry(name: Optional[str]) -> Optional[Entry]:
    return next((e for e in TABLE if e.name == name), None)


def module(e: Entry):
    return importlib.import_module("." + e.module, __package__)


def selected(given: Dict[str, str], keys=("model",)) -> Optional[Entry]:
    """the entry that ``model=`` names in {key: "key=value"}, or None (save passes keys=("model", "model.name"))"""
    return next((e for k in keys for e in TABLE if given.get(k) == f"{k}={e.name}"), None)


def owner(key: str) -> Optional[Entry]:
    """the entry whose command key this is, or None"""
    return next((e for e in TABLE if key in module(e).COMMAND_KEYS), None)


def foreign_keys(given: Iterable[str], e: Optional[Entry]):
    """(owner, message) for the first family, in table order, that has keys among ``given`` without being the selected model ``e``'s;
    None when there is none"""
    for o in TABLE:
        wrong = sorted(k for k in given if o is not e and k in module(o).COMMAND_KEYS)
        if wrong:
            return o, f"{', '.join(wrong)}: the {o.prefix}_* keys belong to model={o.name}"
    return None


def params_from_command(e: Entry, given: Dict[str, str]) -> Dict[str, object]:
    """{command key: value as typed} -> validated parameters; a bad value ends the command (SystemExit) before anything runs"""
    m = module(e)
    # true / false are read as Python's only by a model that has a flag: for the others they stay the bad values they are
    flags = any(isinstance(v, bool) for v in m.DEFAULTS.values())
    p: Dict[str, object] = {}
    for k, v in given.items():
        try:
            p[m.COMMAND_KEYS[k]] = ast.literal_eval(v.capitalize() if flags and v.lower() in ("true", "false") else v)
        except (ValueError, SyntaxError):
            raise SystemExit(f"bad value for {k}: {v!r}")
    try:
        return m.check_params(p)
    except (ValueError, TypeError) as err:
        raise SystemExit(f"bad value among the {e.prefix}_* keys: {err}")


def config(e: Entry, given: Dict[str, str]):
    """(configuration, parameters) of a checkpoint-free model from the command line alone -- the defaults of deflow_amd.train under the keys
    as typed ({key: "key=value"}), the model's own keys validated by its module; batch_size defaults to the module's COMMAND_BATCH_SIZE
    when it has one.  Another model's keys are refused.  Needs no GPU and reads no file."""
    from .train import parse_overrides
    m = module(e)
    for k in ("checkpoint", "inference_dtype"):
        if k in given:
            raise SystemExit(f"model={e.name} has no weights: it takes no {k}=")
    wrong = foreign_keys(given, e)
    if wrong:
        raise SystemExit(wrong[1])
    own = {k: a.split("=", 1)[1] for k, a in given.items() if k in m.COMMAND_KEYS}
    cfg = parse_overrides([a for k, a in given.items() if k not in m.COMMAND_KEYS and k != "model"])
    cfg["model"] = e.name
    if m.COMMAND_BATCH_SIZE is not None and "batch_size" not in given:
        cfg["batch_size"] = m.COMMAND_BATCH_SIZE
    return cfg, params_from_command(e, own)


def build(e: Entry, cfg: dict, params: Dict[str, object]):
    return getattr(module(e), e.cls)(point_cloud_range=cfg["point_cloud_range"], voxel_size=cfg["voxel_size"], **params)


def usage(e: Entry) -> str:
    """the save command's usage text for this model: its keys with their defaults, then its memory note"""
    m = module(e)
    show = lambda v: "" if v is None else str(v).lower() if isinstance(v, bool) else repr(v)
    own = " ".join(f"[{k}={show(m.DEFAULTS[name])}]" for k, name in m.COMMAND_KEYS.items())
    return (f"usage: python -m deflow_amd.save model={e.name} dataset_path=<dir of .h5 files> [res_name={e.name}] [scenes=a,b] "
            f"[batch_size={show(m.COMMAND_BATCH_SIZE)}] [num_workers=] [ground_source=auto|file|sidecar|online] [half=false] "
            f"[overwrite=false] [voxel_size=] [point_cloud_range=] {own}" + ("\n" + e.memory if e.memory else ""))


# ---- the parameter checks of the models' check_params are deflow_amd.args' (imported above: pairflow.integer and the rest resolve) ----------
def whole_cells(fn: str, out: dict, r_max: int) -> None:
    """trunc is 1 to r_max cells (the distance transform's radius, deflow_amd.fastnsf)"""
    R = int(round(out["trunc"] / out["cell"]))
    if not 1 <= R <= r_max or abs(R * out["cell"] - out["trunc"]) > 1e-6 * out["trunc"]:
        raise ValueError(f"{fn}: trunc must be a whole number of cells, 1 to {r_max} of them, got trunc = {out['trunc']}, "
                         f"cell = {out['cell']}")


# ---- the models' base ------------------------------------------------------------------------------------------------------------------
class PairFlowModel:
    """What the weight-free estimators (the classes of ``TABLE``) share: an object with the two methods of ``DeFlow`` the commands use --
    ``forward_padded`` and ``forward`` -- and no weights.  point_cloud_range / voxel_size decide which rows count as decoded, by the
    voxeliser's rule (floor((p - min) / voxel) inside the grid on all three axes, on the ego-compensated rows)."""

    def __init__(self, point_cloud_range=(-51.2, -51.2, -3, 51.2, 51.2, 3), voxel_size=(0.2, 0.2, 6)):
        name = type(self).__name__
        if len(point_cloud_range) != 6 or len(voxel_size) != 3:
            raise ValueError(f"{name}: point_cloud_range has 6 values and voxel_size 3")
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_size = [float(v) for v in voxel_size]
        if not all(v > 0 for v in self.voxel_size):
            raise ValueError(f"{name}: voxel_size must be positive, got {voxel_size}")
        self.grid = [int(round((self.point_cloud_range[3 + i] - self.point_cloud_range[i]) / self.voxel_size[i])) for i in range(3)]
        if not all(g >= 1 for g in self.grid):
            raise ValueError(f"{name}: empty point_cloud_range {point_cloud_range}")
        self.training = False
        self.last_state: Optional[dict] = None

    # (the commands treat the model as an nn.Module)
    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def parameters(self):
        return iter(())

    def _decoded(self, pts: torch.Tensor) -> torch.Tensor:
        """[B,N] bool: the rows the voxeliser would keep (csrc/pillar_common.h: NaN rows and rows outside the grid are not decoded)"""
        ok = ~torch.isnan(pts).any(dim=2)
        for i in range(3):
            f = torch.floor((pts[..., i] - self.point_cloud_range[i]) / self.voxel_size[i])
            ok &= (f >= 0) & (f < float(self.grid[i]))
        return ok

    @staticmethod
    def _compact(valid: torch.Tensor):
        """stable: idx [B,N] i64 with the valid rows first in ascending order, counts [B] i32"""
        idx = torch.argsort((~valid).to(torch.uint8), dim=1, stable=True)
        return idx, valid.sum(dim=1).to(torch.int32)

    def _pair(self, batch: Dict[str, torch.Tensor]) -> dict:
        """the ego-compensated first sweep, the pose flow of every input row, and both sweeps' decoded rows compacted (stable)"""
        from .deflow import batch_transform
        pc0 = batch["pc0"].contiguous().float()
        pc1 = batch["pc1"].contiguous().float()
        if not pc0.is_cuda or not pc1.is_cuda:
            raise TypeError(f"{type(self).__name__}: pc0 and pc1 must be CUDA tensors (deflow_amd has no CPU fallback)")
        B, N, _ = pc0.shape
        T = batch_transform(batch, pc0.device)
        pc0s = torch.empty_like(pc0)
        pose_flow = torch.empty_like(pc0)
        call("df_ego_transform", ptr(pc0), ptr(T), B, N, ptr(pc0s), ptr(pose_flow), stream())
        v0, v1 = self._decoded(pc0s), self._decoded(pc1)
        idx0, counts0 = self._compact(v0)
        idx1, counts1 = self._compact(v1)
        g0 = torch.gather(pc0s, 1, idx0[..., None].expand(-1, -1, 3))
        g1 = torch.gather(pc1, 1, idx1[..., None].expand(-1, -1, 3))
        return {"pose_flow": pose_flow, "counts0": counts0, "counts1": counts1, "idx_c0": idx0, "idx_c1": idx1, "pc0s": pc0s,
                "points_c0": g0, "points_c1": g1}

    def forward_padded(self, batch: Dict[str, torch.Tensor]) -> dict:
        raise NotImplementedError

    def forward(self, batch: Dict[str, torch.Tensor]):
        """the dict of lists ``DeFlow.forward`` returns (one host read: the per-sample counts)"""
        st = self.forward_padded(batch)
        B = st["flow"].shape[0]
        m = torch.stack([st["counts0"], st["counts1"]]).tolist()
        m0, m1 = m[0], m[1]
        return {
            "flow": [st["flow"][b, :m0[b]] for b in range(B)],
            "pose_flow": [st["pose_flow"][b] for b in range(B)],
            "pc0_valid_point_idxes": [st["idx_c0"][b, :m0[b]] for b in range(B)],
            "pc0_points_lst": [st["points_c0"][b, :m0[b]] for b in range(B)],
            "pc1_valid_point_idxes": [st["idx_c1"][b, :m1[b]] for b in range(B)],
            "pc1_points_lst": [st["points_c1"][b, :m1[b]] for b in range(B)],
        }

    def __call__(self, batch):
        return self.forward(batch)
