"""Numpy restatement of the bird's-eye-view rasteriser (include/deflow_amd.h): what csrc/render.hip computes on the
GPU -- the pixel of a row, the colour of its vector, the 64-bit word, the atomic maximum over the (2r+1)^2 square, the scanlines and the
legend disc -- with one fp32 rounding per operation (numpy float32 arithmetic rounds every operation on its own)."""
import numpy as np

F = np.float32
GREY = (128, 128, 128)


def colour(vx, vy, vmax):
    """vx, vy f32 arrays (finite), vmax > 0 -> u8 [..., 3]: HSV with V = 1, S = min(|v| / vmax, 1), H = the diamond angle"""
    vx, vy, vmax = np.asarray(vx, dtype=F), np.asarray(vy, dtype=F), F(vmax)
    with np.errstate(all="ignore"):
        m = np.sqrt(vx * vx + vy * vy)
        s = np.minimum(m / vmax, F(1))
        a = np.abs(vx) + np.abs(vy)
        safe = np.where(a != 0, a, F(1))
        t = np.where(vy >= 0,
                     np.where(vx >= 0, vy / safe, F(1) + (-vx) / safe),
                     np.where(vx >= 0, F(3) + vx / safe, F(2) + (-vy) / safe)).astype(F)
        t = np.where(a != 0, t, F(0)).astype(F)
        h6 = F(1.5) * t
        fl = np.floor(h6)
        f = h6 - fl
        k = fl.astype(np.int32)
        k = np.where(k > 5, 0, k)
        p = F(1) - s
        q = F(1) - s * f
        u = F(1) - s * (F(1) - f)
        assert all(v.dtype == F for v in (m, s, a, t, h6, f, p, q, u))
        byte = lambda c: np.floor(c * F(255) + F(0.5)).astype(np.int64)
        P, Q, U, V = byte(p), byte(q), byte(u), np.full(p.shape, 255, dtype=np.int64)
    table = [(V, U, P), (Q, V, P), (P, V, U), (P, Q, V), (U, P, V), (V, P, Q)]
    out = np.zeros(p.shape + (3,), dtype=np.int64)
    for sector, chans in enumerate(table):
        for c in range(3):
            out[..., c] = np.where(k == sector, chans[c], out[..., c])
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= 255
    return out.astype(np.uint8)


def z_key(z):
    """the order-preserving unsigned form of fp32 bits"""
    b = np.asarray(z, dtype=F).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def rows(points, vec, cls, count, view, size, vmax):
    """one sample: -> drawn [N] bool, px, py [N] int, word [N] u64 (px, py, word meaningful where drawn)"""
    points, vec, cls = np.asarray(points, dtype=F), np.asarray(vec, dtype=F), np.asarray(cls, dtype=np.uint8).reshape(-1)
    N = points.shape[0]
    (xmin, ymin, inv_res), (W, H) = (F(v) for v in view), size
    count = min(max(int(count), 0), N)
    ok = (np.arange(N) < count) & (cls != 0) & np.isfinite(points).all(axis=1) & np.isfinite(vec).all(axis=1)
    with np.errstate(all="ignore"):
        fx = np.floor((points[:, 0] - xmin) * inv_res)
        fy = np.floor((points[:, 1] - ymin) * inv_res)
        assert fx.dtype == F and fy.dtype == F
        ok &= (fx >= 0) & (fx < F(W)) & (fy >= 0) & (fy < F(H))
    px = np.where(ok, fx, 0).astype(np.int64)
    py = H - 1 - np.where(ok, fy, 0).astype(np.int64)
    v = np.where(ok[:, None], vec, F(0))
    rgb = colour(v[:, 0], v[:, 1], vmax).astype(np.uint64)
    rgb = np.where((cls == 1)[:, None], rgb, np.array(GREY, dtype=np.uint64))
    key = (z_key(np.where(ok, points[:, 2], F(0))) >> np.uint32(1)).astype(np.uint64)
    word = ((cls == 1).astype(np.uint64) << np.uint64(63)) | (key << np.uint64(32)) | (rgb[:, 0] << np.uint64(24)) | \
           (rgb[:, 1] << np.uint64(16)) | (rgb[:, 2] << np.uint64(8)) | np.uint64(0xFF)
    return ok, px, py, word


def splat(points, vec, cls, count, view, size, vmax, radius):
    """one sample -> image u64 [H, W] (0 = empty)"""
    W, H = size
    ok, px, py, word = rows(points, vec, cls, count, view, size, vmax)
    px, py, word = px[ok], py[ok], word[ok]
    img = np.zeros((H, W), dtype=np.uint64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            xx, yy = px + dx, py + dy
            m = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            np.maximum.at(img, (yy[m], xx[m]), word[m])
    return img


def resolve(img, bg=(24, 24, 24), legend=0):
    """image u64 [H, W] -> scanlines u8 [H, 1 + 3W]"""
    H, W = img.shape
    rgb = np.stack([(img >> np.uint64(s)).astype(np.uint8) for s in (24, 16, 8)], axis=-1)      # astype keeps the low byte
    rgb = np.where((img == 0)[..., None], np.array(bg, dtype=np.uint8), rgb)
    L = int(legend)
    if L > 0:
        assert 2 * L + 5 <= min(W, H)
        yy, xx = np.mgrid[0:H, 0:W]
        dx, dy = xx - (W - 3 - L), yy - (L + 2)
        disc = dx * dx + dy * dy <= L * L
        wheel = colour(dx.astype(F), (-dy).astype(F), F(L))
        rgb = np.where(disc[..., None], wheel, rgb)
    out = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    out[:, 1:] = rgb.reshape(H, 3 * W)
    return out


def render_rows(points, count, vec, cls, view, size, vmax, radius=1, bg=(24, 24, 24), legend=0):
    """[B,N,3], [B], [B,N,3], [B,N] -> scanlines u8 [B, H, 1 + 3W]"""
    return np.stack([resolve(splat(points[b], vec[b], cls[b], count[b], view, size, vmax, radius), bg, legend)
                     for b in range(points.shape[0])])


def pixels(scanlines):
    """scanlines [..., H, 1 + 3W] -> [..., H, W, 3]"""
    s = np.asarray(scanlines)
    assert (s[..., 0] == 0).all()
    return s[..., 1:].reshape(s.shape[:-1] + ((s.shape[-1] - 1) // 3, 3))
