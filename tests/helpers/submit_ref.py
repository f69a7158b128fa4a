"""Numpy restatement of the submission body (include/deflow_amd.h): what deflow_amd/submit.py packs on the GPU, per
sample -- the rows with eval_mask != 0 among the first ``count``, in raw order; ``astype(float16)`` per column; the flag column through
``np.packbits(..., bitorder="little")``; every buffer padded with zeros to 8 bytes; L(M) bytes in all."""
import numpy as np

# version -> the columns in file order (restated here on purpose: the tests compare deflow_amd.feather.COLUMNS with it)
ORDER = {1: ("flow_tx_m", "flow_ty_m", "flow_tz_m", "is_dynamic"), 2: ("is_valid", "flow_tx_m", "flow_ty_m", "flow_tz_m")}
FLAGS = ("is_dynamic", "is_valid")


def pad8(n):
    return (int(n) + 7) // 8 * 8


def body_len(M):
    """L(M) = 3 P + Q with P = pad8(2 M), Q = pad8(ceil(M / 8))"""
    return 3 * pad8(2 * M) + pad8((M + 7) // 8)


def select(eval_mask, count):
    """the raw rows of the benchmark, in raw order"""
    eval_mask = np.asarray(eval_mask).reshape(-1)
    N = eval_mask.shape[0]
    count = min(max(int(count), 0), N)
    return np.nonzero((np.arange(N) < count) & (eval_mask != 0))[0]


def columns(flow_est, dynamic, eval_mask, count):
    """one sample -> {column name: array of M values} for both versions' columns"""
    rows = select(eval_mask, count)
    sel = np.asarray(flow_est, dtype=np.float32)[rows]
    with np.errstate(all="ignore"):
        half = [sel[:, i].astype(np.float16) for i in range(3)]       # three strided column copies, overflow to inf
    return {"flow_tx_m": half[0], "flow_ty_m": half[1], "flow_tz_m": half[2], "is_dynamic": np.asarray(dynamic).reshape(-1)[rows] != 0,
            "is_valid": np.ones(rows.shape[0], dtype=bool)}


def _padded(raw: bytes) -> bytes:
    return raw + bytes(pad8(len(raw)) - len(raw))


def body(flow_est, dynamic, eval_mask, count, version):
    """one sample -> (uint8 [L(M)], M)"""
    cols = columns(flow_est, dynamic, eval_mask, count)
    M = int(cols["is_valid"].shape[0])
    out = b""
    for name in ORDER[version]:
        if name in FLAGS:
            out += _padded(np.packbits(cols[name], bitorder="little").tobytes())
        else:
            out += _padded(cols[name].astype("<f2").tobytes())
    assert len(out) == body_len(M)
    return np.frombuffer(out, dtype=np.uint8), M


def body_batch(flow_est, dynamic, eval_mask, count, version):
    return [body(flow_est[b], dynamic[b], eval_mask[b], count[b], version) for b in range(flow_est.shape[0])]
