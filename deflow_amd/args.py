"""What every point-cloud op checks and allocates before it launches, in one place: the tensor and cloud checks, the workspace of an
entry that has a ``*_ws_bytes`` query, and the parameter checks of the ``check_params`` functions.  The row grid is ``chamfer.RowGrid``
and the segment lists are ``rigid.segments``.  An op module may bind its own ``fn`` and ``other`` with
``functools.partial``; it does not restate a check.  Nothing here needs a GPU but the allocation in ``workspace``."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from ._lib import call, ptr  # noqa: F401  (both names, as in the op modules: tests/helpers/guarded.py patches the modules that hold the pair)


# ---- tensors -----------------------------------------------------------------------------------------------------------------------------
def tensor(fn: str, name: str, t, dtype=None, shape=None, device=None, other: str = "not"):
    """t, a CUDA tensor of that dtype (one, or a tuple of allowed ones; None: any) and shape, on that device -- or an error of ``fn``
    naming the argument; other: how the message names the device it compares with ("raw is", "the map is")"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{fn}: {name} must be a CUDA tensor (deflow_amd has no CPU fallback)")
    if device is not None and t.device != device:
        raise ValueError(f"{fn}: {name} is on {t.device}, {other} on {device}")
    dtypes = () if dtype is None else dtype if isinstance(dtype, tuple) else (dtype,)
    if (dtypes and t.dtype not in dtypes) or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{fn}: {name} must be {' or '.join(str(d) for d in dtypes) or 'a tensor'}" +
                         (f" of shape {tuple(shape)}" if shape is not None else "") + f", got {t.dtype} {tuple(t.shape)}")
    return t


def cloud(fn: str, name: str, t, rows_limit: Optional[int] = None) -> Tuple[int, int]:
    """(B, N) of a CUDA float32 cloud [B,N,3], or an error of ``fn`` naming the argument.  rows_limit k (1: the rows are indexed, 3: their
    components are) also asks for B <= 65535 and k * B * N < 2^31; None asks for neither."""
    tensor(fn, name, t)
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{fn}: {name} must be torch.float32 of shape (B, N, 3) with B >= 1 and N >= 1, got {t.dtype} {tuple(t.shape)}")
    B, N = int(t.shape[0]), int(t.shape[1])
    if rows_limit is not None and (B > 65535 or rows_limit * B * N >= 2 ** 31):
        raise ValueError(f"{fn}: {name}: 1 <= B <= 65535 and {'' if rows_limit == 1 else f'{rows_limit} * '}B * N < 2^31 expected, "
                         f"got B = {B}, N = {N}")
    return B, N


def labels(fn: str, name: str, t, shape, wrong: str, device=None) -> Optional[torch.Tensor]:
    """an optional integer / bool row label as the int32 tensor the search reads (label > 0 takes part); wrong: the caller's finished
    sentence for anything else"""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (device is not None and t.device != device) or \
            tuple(t.shape) != tuple(shape) or t.dtype.is_floating_point:
        raise ValueError(f"{fn}: {name} {wrong}")
    return t.to(torch.int32).contiguous()


# ---- workspaces --------------------------------------------------------------------------------------------------------------------------
def ws_bytes(query: str, dims, refused: str) -> int:
    """what the entry's ``*_ws_bytes`` query answers for these dimensions; a negative answer is ValueError(refused), the caller's sentence"""
    need = int(call(query, *dims))
    if need < 0:
        raise ValueError(refused)
    return need


def workspace(query: str, dims, device, refused: str) -> torch.Tensor:
    """the entry's scratch, at least ws_bytes(...) bytes as int32, from torch's caching allocator like the outputs: safe across streams,
    and under a stream capture it comes from the graph's own pool"""
    return torch.empty(max((ws_bytes(query, dims, refused) + 3) // 4, 1), dtype=torch.int32, device=device)


# ---- the parameter checks of the check_params functions ---------------------------------------------------------------------------------
# fn: the function the message names; out: the parameter dict, checked and converted in place.  finite=True (mbnsf, floxels, refine): a
# value that is no finite number is reported as such, whatever else the key asks for.
def merged(fn: str, defaults: Dict[str, object], p: Dict[str, object]) -> Dict[str, object]:
    out = dict(defaults)
    for k, v in p.items():
        if k not in defaults:
            raise ValueError(f"{fn}: unknown parameter {k!r}; known: {', '.join(sorted(defaults))}")
        out[k] = v
    return out


def _number(v) -> bool:
    return not isinstance(v, bool) and isinstance(v, (int, float))


def _finite(fn: str, k: str, v) -> None:
    if not _number(v) or not math.isfinite(v):
        raise ValueError(f"{fn}: {k} must be a finite number, got {v!r}")


def integer(fn: str, out: dict, k: str, lo: int, hi: int, finite: bool = False) -> None:
    v = out[k]
    if finite:
        _finite(fn, k, v)
    if not _number(v) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f"{fn}: {k} must be an integer in [{lo}, {hi}], got {v!r}")
    out[k] = int(v)


def positive(fn: str, out: dict, k: str, finite: bool = False) -> None:
    v = out[k]
    if finite:
        _finite(fn, k, v)
    if not _number(v) or not (math.isfinite(v) and v > 0):
        raise ValueError(f"{fn}: {k} must be positive and finite, got {v!r}")
    out[k] = float(v)


def nonneg(fn: str, out: dict, k: str, finite: bool = False) -> None:
    v = out[k]
    if finite:
        _finite(fn, k, v)
    if not _number(v) or not (math.isfinite(v) and v >= 0):
        raise ValueError(f"{fn}: {k} must be finite and >= 0, got {v!r}")
    out[k] = float(v)


def flag(fn: str, out: dict, k: str) -> None:
    if not isinstance(out[k], bool):
        raise ValueError(f"{fn}: {k} must be True or False, got {out[k]!r}")
