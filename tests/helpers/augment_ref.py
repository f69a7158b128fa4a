"""numpy restatement of the training augmentation (include/deflow_amd.h "training augmentation"): Python-integer
Philox4x32-10 and float64 geometry.  ``apply`` evaluates the transform in float64 (``dtype=np.float64``, the reference the device's fp32
arithmetic is bounded against) or operation by operation in fp32 (``dtype=np.float32``: what the device computes bit for bit on the paths
without a multiply-add pair -- flips, height, dropout)."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
SAMPLE_ROW = 0xFFFFFFFF
BELL_STD = 147.8           # sqrt(4 (256^2 - 1) / 12): the standard deviation of the sum of four bytes
F = np.float32


def philox(ctr, key):
    """Philox4x32-10: ctr four and key two Python integers -> four words"""
    c0, c1, c2, c3 = (int(c) & MASK for c in ctr)
    k0, k1 = (int(k) & MASK for k in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
    return c0, c1, c2, c3


def philox_rows(id_, rows, purpose, key):
    """the four words of every row in ``rows`` (uint array) of one sample, vectorised: -> uint64 [len(rows), 4] holding u32 values"""
    id_ = int(id_) & 0xFFFFFFFFFFFFFFFF
    n = len(rows)
    c0 = np.full(n, id_ & MASK, dtype=np.uint64)
    c1 = np.full(n, id_ >> 32, dtype=np.uint64)
    c2 = np.asarray(rows, dtype=np.uint64).copy()
    c3 = np.full(n, purpose, dtype=np.uint64)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # (u32 x u32 fits u64)
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
    return np.stack([c0, c1, c2, c3], 1)


def u01(w):
    """(w >> 8) 2^-24: exact in fp32 and in float64"""
    return (np.asarray(w, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def bell(w):
    """the sum of the four bytes of w minus 510, as float64 integers"""
    w = np.asarray(w, dtype=np.uint64)
    b = sum((w >> np.uint64(s)) & np.uint64(255) for s in (0, 8, 16, 24))
    return b.astype(np.float64) - 510.0


def key_of(seed, epoch):
    return int(seed) & MASK, int(epoch) & MASK


class Config:
    """the op's arguments as the device takes them: every magnitude rounded to fp32 (the C ABI passes floats), yaw in radians"""

    def __init__(self, seed, flip_x_p=0.5, flip_y_p=0.5, yaw_deg=0.0, height=0.2, jitter_sigma=0.01, drop_p=0.0):
        self.seed = int(seed)
        self.flip_x_p, self.flip_y_p, self.drop_p = (float(F(v)) for v in (flip_x_p, flip_y_p, drop_p))
        self.yaw_max = float(F(math.radians(float(yaw_deg))))
        self.height_max, self.sigma = float(F(height)), float(F(jitter_sigma))
        self.sj = float(F(self.sigma / BELL_STD))            # fp32(sigma / 147.8), the quotient in double


def sample_draw(cfg, id_, epoch):
    """-> dict sx, sy, theta (float64), c, s (float64 cos / sin of theta), dz (the fp32 value, as float64)"""
    w = philox((int(id_) & MASK, (int(id_) >> 32) & MASK, SAMPLE_ROW, 0), key_of(cfg.seed, epoch))
    u = [float(u01(x)) for x in w]
    theta = (2.0 * u[2] - 1.0) * cfg.yaw_max
    dz = float(F(F(2.0 * u[3] - 1.0) * F(cfg.height_max)))
    return {"sx": -1.0 if u[0] < cfg.flip_x_p else 1.0, "sy": -1.0 if u[1] < cfg.flip_y_p else 1.0, "theta": theta,
            "c": float(np.cos(theta)) if cfg.yaw_max != 0 else 1.0, "s": float(np.sin(theta)) if cfg.yaw_max != 0 else 0.0, "dz": dz}


def params(cfg, ids, epoch):
    """float64 [B, 8]: sx, sy, c, s, dz, theta, 0, 0"""
    out = np.zeros((len(ids), 8))
    for b, i in enumerate(ids):
        d = sample_draw(cfg, i, epoch)
        out[b, :6] = d["sx"], d["sy"], d["c"], d["s"], d["dz"], d["theta"]
    return out


def matrices(d):
    """A and A^-1 as float64 4x4"""
    sx, sy, c, s, dz = d["sx"], d["sy"], d["c"], d["s"], d["dz"]
    A = np.array([[c * sx, -s * sy, 0, 0], [s * sx, c * sy, 0, 0], [0, 0, 1, dz], [0, 0, 0, 1.0]])
    Ai = np.array([[sx * c, sx * s, 0, 0], [-sy * s, sy * c, 0, 0], [0, 0, 1, -dz], [0, 0, 0, 1.0]])
    return A, Ai


def linear(d, v, dtype=np.float64):
    """L v on rows [n, 3]: flip, then rotation, in the device's order"""
    t = dtype
    x1, y1 = t(d["sx"]) * v[:, 0].astype(t), t(d["sy"]) * v[:, 1].astype(t)
    if d["s"] == 0.0 and d["c"] == 1.0:
        return np.stack([x1, y1, v[:, 2].astype(t)], 1)
    c, s = t(d["c"]), t(d["s"])
    return np.stack([c * x1 - s * y1, s * x1 + c * y1, v[:, 2].astype(t)], 1)


def cloud(cfg, d, id_, epoch, pc, purpose, dtype=np.float64):
    """one sample's cloud [n, 3] -> augmented [n, 3] of ``dtype`` and the dropped-row mask.  dtype=np.float32 rounds after every operation."""
    t = dtype
    with np.errstate(invalid="ignore"):
        out = linear(d, pc, t)
        out[:, 2] = out[:, 2] + t(d["dz"])
        dropped = np.zeros(len(pc), dtype=bool)
        if cfg.sj > 0 or cfg.drop_p > 0:
            w = philox_rows(id_, np.arange(len(pc)), purpose, key_of(cfg.seed, epoch))
            if cfg.sj > 0:
                for k in range(3):
                    out[:, k] = out[:, k] + (bell(w[:, k]) * cfg.sj).astype(t)
            dropped = u01(w[:, 3]) < cfg.drop_p
            out[dropped] = np.nan
    return out, dropped


def apply(cfg, ids, epoch, pc0, pc1, flow=None, T=None, pose0=None, pose1=None, dtype=np.float64):
    """the whole op on numpy arrays [B, N, 3] / [B, 4, 4] -> dict of the outputs that have inputs (matrices always float64)"""
    out = {"pc0": [], "pc1": [], "flow": [], "T": [], "pose0": [], "pose1": [], "drop0": [], "drop1": []}
    for b, i in enumerate(ids):
        d = sample_draw(cfg, i, epoch)
        for name, pc, purpose in (("0", pc0, 1), ("1", pc1, 2)):
            p, dr = cloud(cfg, d, i, epoch, pc[b], purpose, dtype)
            out["pc" + name].append(p)
            out["drop" + name].append(dr)
        A, Ai = matrices(d)
        if flow is not None:
            with np.errstate(invalid="ignore"):
                out["flow"].append(linear(d, flow[b], dtype))
        if T is not None:
            out["T"].append(A @ T[b].astype(np.float64) @ Ai)
        if pose0 is not None:
            out["pose0"].append(pose0[b].astype(np.float64) @ Ai)
        if pose1 is not None:
            out["pose1"].append(pose1[b].astype(np.float64) @ Ai)
    return {k: np.stack(v) for k, v in out.items() if v}
