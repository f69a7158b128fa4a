"""Numpy restatement of the whole-sweep flow (include/deflow_amd.h): what deflow_amd/sweeps.py computes on the GPU,
per sample, with one fp32 rounding per operation -- compaction by boolean indexing, the pose flow in df_ego_transform's operation order,
the composition, the squared-norm flag and the fp16 cast."""
import numpy as np

F = np.float32
DYN2 = F(0.0025)
NAN_BITS = np.uint32(0x7FC00000)          # float("nan") as fp32: what collate_fn_pad pads with


def compact(raw, count, drop):
    """one sample: raw [N,3] f32, count valid leading rows, drop [N] (non-zero = ground) -> pc [N,3], row_of [N], pos_of [N], kept"""
    raw = np.ascontiguousarray(raw, dtype=F)
    N = raw.shape[0]
    count = min(max(int(count), 0), N)
    keep = (np.arange(N) < count) & (np.asarray(drop).reshape(-1) == 0)
    rows = np.nonzero(keep)[0]
    kept = int(rows.shape[0])
    pc = np.full((N, 3), NAN_BITS, dtype=np.uint32)
    pc[:kept] = raw.view(np.uint32)[rows]
    row_of = np.full(N, -1, dtype=np.int32)
    row_of[:kept] = rows
    pos_of = np.full(N, -1, dtype=np.int32)
    pos_of[rows] = np.arange(kept, dtype=np.int32)
    return pc.view(F), row_of, pos_of, kept


def compact_batch(raw, count, drop):
    out = [compact(raw[b], count[b], drop[b]) for b in range(raw.shape[0])]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.array([o[3] for o in out], dtype=np.int32))


def pose_flow(p, T):
    """p [N,3] f32, T [4,4] f32 -> [N,3] f32: a = x T[i][0]; a += y T[i][1]; a += z T[i][2]; a += T[i][3]; a - p[i], each rounded to fp32"""
    p, T = np.asarray(p, dtype=F), np.asarray(T, dtype=F)
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for i in range(3):
            a = p[:, 0] * T[i, 0]
            a = a + p[:, 1] * T[i, 1]
            a = a + p[:, 2] * T[i, 2]
            a = a + T[i, 3]
            out[:, i] = a - p[:, i]
    assert out.dtype == F
    return out


def sq_norm(f):
    """(fx fx + fy fy) + fz fz in fp32, one rounding per operation"""
    f = np.asarray(f, dtype=F)
    with np.errstate(all="ignore"):
        return (f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2]


def compose(raw, count, T, pos_of, flow, idx_c, counts, half=False):
    """one sample -> flow_est [N,3] (f32, or f16 with half), dynamic u8 [N]"""
    raw = np.asarray(raw, dtype=F)
    N = raw.shape[0]
    count = min(max(int(count), 0), N)
    est = np.zeros((N, 3), dtype=F)
    dyn = np.zeros(N, dtype=np.uint8)
    fin = np.isfinite(raw).all(axis=1) & (np.arange(N) < count)
    est[fin] = pose_flow(raw[fin], T)
    m = min(max(int(counts), 0), flow.shape[0])
    inv = np.full(N, -1, dtype=np.int64)                   # compact position -> decoded index
    idx = np.asarray(idx_c[:m], dtype=np.int64)
    ok = (idx >= 0) & (idx < N)
    inv[idx[ok]] = np.nonzero(ok)[0]
    for r in np.nonzero(fin)[0]:
        q = pos_of[r]
        i = inv[q] if 0 <= q < N else -1
        if i >= 0:
            f = np.asarray(flow[i], dtype=F)
            with np.errstate(all="ignore"):
                est[r] = est[r] + f
            dyn[r] = 1 if sq_norm(f) >= DYN2 else 0
    if half:
        with np.errstate(all="ignore"):
            est = est.astype(np.float16)
    return est, dyn


def compose_batch(raw, count, T, pos_of, flow, idx_c, counts, half=False):
    out = [compose(raw[b], count[b], T[b], pos_of[b], flow[b], idx_c[b], counts[b], half) for b in range(raw.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def threshold_flows():
    """flow rows whose fp32 squared norm is the float below 0.0025f, 0.0025f itself and the float above it: fx = 2^-5 (its square is
    exact), fy found by walking the fp32 neighbours of sqrt(0.0025 - fx^2), and where that walk steps over a value, fz = 2^-16, whose
    square is exactly one ulp of 0.0025f, added to the row one ulp lower -> {"below": row, "at": row, "above": row}"""
    t = DYN2
    want = {"below": np.nextafter(t, F(0)), "at": t, "above": np.nextafter(t, F(1))}
    fx = F(2.0 ** -5)
    fy = F(np.sqrt(np.float64(t) - np.float64(fx) ** 2))
    out = {}
    for step in range(-64, 65):
        y = fy
        for _ in range(abs(step)):
            y = np.nextafter(y, F(1) if step > 0 else F(0))
        row = np.array([fx, y, 0.0], dtype=F)
        s = sq_norm(row)
        for k, v in want.items():
            if s == v and k not in out:
                out[k] = row
    for lo, hi in (("below", "at"), ("at", "above")):
        if hi not in out and lo in out:
            out[hi] = np.array([out[lo][0], out[lo][1], 2.0 ** -16], dtype=F)
    for k, v in want.items():
        assert k in out and sq_norm(out[k]) == v, k
    assert sorted(out) == sorted(want), sorted(out)
    return out
