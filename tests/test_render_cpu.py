"""CPU: the numpy restatement of the bird's-eye-view rasteriser (tests/helpers/render_ref.py) pinned to hand-made cases
whose expected bytes are stated here, the PNG writer / reader (deflow_amd/png.py), the vis command's argument parsing and the entry points'
guards (which return before any launch).  tests/test_gpu_render.py compares the kernels with the same restatement."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import render_ref as RR  # noqa: E402

F = np.float32
WHITE, RED, YGREEN, CYAN, VIOLET, GREY, BG = (255, 255, 255), (255, 0, 0), (128, 255, 0), (0, 255, 255), (128, 0, 255), (128, 128, 128), (24, 24, 24)


# ---- colour ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vx, vy, vmax, want", [
    (2.0, 0.0, 2.0, RED), (0.0, 2.0, 2.0, YGREEN), (-2.0, 0.0, 2.0, CYAN), (0.0, -2.0, 2.0, VIOLET),            # the four axes, |v| = vmax
    (2.0, -0.0, 2.0, RED), (-0.0, 2.0, 2.0, YGREEN), (-2.0, -0.0, 2.0, CYAN), (-0.0, -2.0, 2.0, VIOLET),        # -0.0 >= 0 holds
    (0.0, 0.0, 2.0, WHITE), (-0.0, -0.0, 2.0, WHITE),                                                           # a == 0: t = 0, s = 0
    (1e-40, 0.0, 2.0, WHITE), (-1e-40, 1e-40, 2.0, WHITE),                                                      # denormal: vx vx underflows, s = 0
    (1.0, 0.0, 2.0, (255, 128, 128)),                                                                           # s = 0.5: p = u = 0.5 -> floor(128.0)
    (5.0, 0.0, 2.0, RED), (0.0, -1e30, 2.0, VIOLET), (3e38, 0.0, 2.0, RED),                                     # |v| > vmax, and vx vx = inf: s = 1
    (3.0, 4.0, 5.0, (255, 219, 0)),           # m = 5, s = 1, t = 4/7, h6 = 0.857: sector 0, u = f -> floor(218.57 + 0.5)
    (-1.0, -3.0, 4.0, (79, 53, 255)),         # s = sqrt(10)/4 = 0.79057, t = 2.75, h6 = 4.125: sector 4, f = 0.125: u = 0.30825, p = 0.20943
    (-3.0, 1.0, 8.0, (154, 255, 217)),       # s = 0.39528, t = 1.75, h6 = 2.625: sector 2 (p, 1, u), f = 0.625: p = 0.60472, u = 1 - s 0.375 = 0.85177
])
def test_colour_cases(vx, vy, vmax, want):
    got = tuple(int(v) for v in RR.colour(F(vx), F(vy), vmax))
    assert got == want, (vx, vy, vmax, got, want)


def test_colour_is_continuous_across_the_wrap_and_stays_in_range():
    # h6 -> 6 from below is the red of h6 = 0; a ring of directions never leaves [0, 255] and is fully saturated at |v| = vmax
    assert tuple(RR.colour(F(1.0), F(-1e-30), 1.0)) == RED
    ang = np.linspace(0, 2 * np.pi, 721)
    c = RR.colour(np.cos(ang).astype(F) * F(3), np.sin(ang).astype(F) * F(3), 2.0)
    assert (c.max(axis=1) == 255).all() and (c.min(axis=1) == 0).all()
    step = np.abs(np.diff(c.astype(int), axis=0)).max()
    assert step <= 6, step                                   # 0.5 degree steps: the hue moves, never jumps


def test_z_key_orders_like_the_floats():
    z = np.array([-np.inf, -3e38, -2.0, -1.0, -1e-40, -0.0, 0.0, 1e-40, 1.0, 2.0, 3e38, np.inf], dtype=F)
    k = RR.z_key(z)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert int(RR.z_key(F(0.0))) == 0x80000000 and int(RR.z_key(F(-0.0))) == 0x7FFFFFFF


# ---- words, priority, edges -----------------------------------------------------------------------------------------------------------------
def draw(rows, size, view=(0.0, 0.0, 1.0), vmax=1.0, radius=0, count=None, **kw):
    """rows: (x, y, z, vx, vy, vz, cls) -> pixels [H, W, 3]"""
    a = np.array([r[:6] for r in rows], dtype=F).reshape(-1, 6)
    cls = np.array([r[6] for r in rows], dtype=np.uint8)
    img = RR.splat(a[:, :3], a[:, 3:], cls, len(rows) if count is None else count, view, size, vmax, radius)
    return RR.pixels(RR.resolve(img, **kw)), img


def test_word_layout():
    _, img = draw([(1.5, 0.5, 2.0, 1.0, 0.0, 9.0, 1), (2.5, 0.5, -2.0, 0.0, 0.0, 0.0, 2)], (4, 1))
    # z = 2.0 = 0x40000000 -> key 0xC0000000 -> 31 bits 0x60000000; red; coloured bit set
    assert int(img[0, 1]) == (1 << 63) | (0x60000000 << 32) | (0xFF0000 << 8) | 0xFF
    # z = -2.0 = 0xC0000000 -> key 0x3FFFFFFF -> 0x1FFFFFFF; grey; coloured bit clear
    assert int(img[0, 2]) == (0x1FFFFFFF << 32) | (0x808080 << 8) | 0xFF
    assert int(img[0, 0]) == 0 and int(img[0, 3]) == 0


def test_priority():
    red, cyan = (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)
    px, _ = draw([(0.5, 0.5, 0.0) + red + (1,), (0.5, 0.5, 5.0) + red + (2,),                  # coloured under a higher grey row: coloured wins
                  (1.5, 0.5, 1.0) + red + (1,), (1.5, 0.5, 2.0) + cyan + (1,),                 # within a class the higher z wins
                  (2.5, 0.5, -1.0) + cyan + (1,), (2.5, 0.5, -2.0) + red + (1,),               # ... among negative heights too
                  (3.5, 0.5, 1.0) + cyan + (1,), (3.5, 0.5, 1.0) + red + (1,),                 # equal z: 0xFF0000 > 0x00FFFF
                  (4.5, 0.5, 1.0) + red + (2,), (4.5, 0.5, 3.0) + cyan + (7,),                 # any other non-zero class is grey
                  (5.5, 0.5, 9.0) + red + (0,)], (7, 1))                                        # class 0 is not drawn
    assert [tuple(int(v) for v in p) for p in px[0]] == [RED, CYAN, CYAN, RED, GREY, BG, BG]


def test_edges_and_skipped_rows():
    nan, inf = float("nan"), float("inf")
    v = (1.0, 0.0, 0.0)
    view, size = (-1.0, -2.0, 2.0), (4, 3)                     # res = 0.5: x in [-1, 1), y in [-2, -0.5)
    rows = [(-1.0, -2.0, 0.0) + v + (1,),                       # x == xmin, y == ymin: drawn at column 0 of the BOTTOM line
            (1.0, -2.0, 0.0) + v + (1,),                        # x == xmin + W res: skipped
            (-1.0, -0.5, 0.0) + v + (1,),                       # y == ymin + H res: skipped
            (0.75, -0.75, 0.0) + v + (1,),                      # the last cell on both axes: column 3 of the top line
            (np.nextafter(F(1.0), F(0)), -0.75, 0.0) + v + (1,),   # fp32(x - xmin) rounds up to 2.0: column 4, skipped -- the definition's own rounding
            (np.nextafter(F(-1.0), F(-2)), -2.0, 0.0) + v + (1,),                             # just outside on the left: skipped
            (nan, -1.0, 0.0) + v + (1,), (0.0, inf, 0.0) + v + (1,), (0.0, -1.0, -inf) + v + (1,),
            (0.0, -1.0, 0.0, nan, 0.0, 0.0, 1), (0.0, -1.0, 0.0, 0.0, 0.0, inf, 2),           # a non-finite vector skips grey rows too
            (0.0, -1.0, 0.0) + v + (0,),
            (0.0, -1.25, 0.0) + v + (1,)]                       # behind count: padded
    px, img = draw(rows, size, view=view, count=len(rows) - 1)
    want = np.full((3, 4, 3), 24, dtype=np.uint8)
    want[2, 0] = RED
    want[0, 3] = RED
    assert np.array_equal(px, want)
    assert int((img != 0).sum()) == 2
    px, _ = draw(rows, size, view=view)                         # with the last row counted it lands at column 2 of the middle line
    want[1, 2] = RED
    assert np.array_equal(px, want)


def test_radius_is_clipped_to_the_image():
    v = (0.0, 0.0, 0.0)
    px, _ = draw([(0.5, 4.5, 0.0) + v + (1,), (5.5, 0.5, 1.0) + v + (2,)], (6, 5), radius=1)
    want = np.full((5, 6, 3), 24, dtype=np.uint8)
    want[0:2, 0:2] = WHITE                                      # the top left corner: a 2 x 2 remainder of the 3 x 3 square
    want[3:5, 4:6] = GREY                                       # the bottom right corner
    assert np.array_equal(px, want)
    px, _ = draw([(2.5, 2.5, 0.0) + v + (1,)], (6, 5), radius=4)
    assert (px == 255).all()                                    # 9 x 9 around the middle covers all of 6 x 5


def test_resolve_and_legend():
    img = np.zeros((9, 9), dtype=np.uint64)
    img[8, 0] = np.uint64((0x123456 << 8) | 0xFF)
    s = RR.resolve(img, bg=(1, 2, 3), legend=0)
    assert s.shape == (9, 28) and s.dtype == np.uint8 and not s[:, 0].any()
    assert s[8, 1:4].tolist() == [0x12, 0x34, 0x56] and s[8, 4:7].tolist() == [1, 2, 3] and s[0, 1:4].tolist() == [1, 2, 3]
    img[4, 4] = img[8, 0]                                       # the legend overrides what lies under it
    px = RR.pixels(RR.resolve(img, bg=(1, 2, 3), legend=2))     # centre (W - 3 - L, L + 2) = (4, 4)
    t = lambda y, x: tuple(int(v) for v in px[y, x])
    assert t(4, 4) == WHITE and t(4, 6) == RED and t(2, 4) == YGREEN and t(4, 2) == CYAN and t(6, 4) == VIOLET      # dy points up
    assert t(5, 5) == tuple(int(v) for v in RR.colour(F(1), F(-1), 2.0)) and t(5, 5) != (1, 2, 3)
    assert t(5, 6) == (1, 2, 3) and t(1, 4) == (1, 2, 3) and t(8, 0) == (0x12, 0x34, 0x56)
    assert int((px != np.array([1, 2, 3])).any(axis=2).sum()) == 13 + 1                                              # 13 lattice points within radius 2
    with pytest.raises(AssertionError):
        RR.resolve(np.zeros((8, 9), dtype=np.uint64), legend=2)      # 2 L + 5 = 9 > 8


# ---- png ------------------------------------------------------------------------------------------------------------------------------------
def chunks(data):
    at, out = 8, []
    while at < len(data):
        n = struct.unpack(">I", data[at:at + 4])[0]
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n], struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0]))
        at += 12 + n
    return out


@pytest.mark.parametrize("W", [1, 37, 48])
def test_png_round_trip(tmp_path, W):
    from deflow_amd import png
    H = 5
    rng = np.random.default_rng(W)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    lines = np.zeros((H, 1 + 3 * W), dtype=np.uint8)
    lines[:, 1:] = rgb.reshape(H, 3 * W)
    a, b = str(tmp_path / "a.png"), str(tmp_path / "b.png")
    assert png.write_png(a, lines, W, H) == a
    assert np.array_equal(png.read_png(a), rgb)
    import torch
    png.write_png(b, torch.from_numpy(lines).numpy(), W, H)
    data = open(a, "rb").read()
    assert data == open(b, "rb").read(), "two writes differ"
    assert sorted(os.listdir(tmp_path)) == ["a.png", "b.png"]                    # no temporary file is left
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    cs = chunks(data)
    assert [c[0] for c in cs] == [b"IHDR", b"IDAT", b"IEND"]
    for kind, body, crc in cs:
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
    assert cs[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0) and cs[2][1] == b""
    assert zlib.decompress(cs[1][1]) == lines.tobytes()
    assert png.encode_png(lines.tobytes(), W, H) == data
    assert np.array_equal(png.decode_png(png.encode_png(lines, W, H, level=0)), rgb)


def test_png_refusals():
    from deflow_amd import png
    lines = np.zeros((2, 7), dtype=np.uint8)
    good = png.encode_png(lines, 2, 2)

    def with_ihdr(body):
        return png.SIGNATURE + png._chunk(b"IHDR", body) + good[8 + 25:]

    with pytest.raises(ValueError, match="interlaced"):
        png.decode_png(with_ihdr(struct.pack(">IIBBBBB", 2, 2, 8, 2, 0, 0, 1)))
    with pytest.raises(ValueError, match="only 8-bit RGB"):
        png.decode_png(with_ihdr(struct.pack(">IIBBBBB", 2, 2, 16, 2, 0, 0, 0)))
    with pytest.raises(ValueError, match="only 8-bit RGB"):
        png.decode_png(with_ihdr(struct.pack(">IIBBBBB", 2, 2, 8, 6, 0, 0, 0)))
    with pytest.raises(ValueError, match="bad signature"):
        png.decode_png(b"GIF89a" + good)
    broken = bytearray(good)
    broken[-5] ^= 1
    with pytest.raises(ValueError, match="bad CRC"):
        png.decode_png(bytes(broken))
    with pytest.raises(ValueError, match="truncated"):
        png.decode_png(good[:-3])
    filtered = png.SIGNATURE + png._chunk(b"IHDR", struct.pack(">IIBBBBB", 2, 2, 8, 2, 0, 0, 0)) + \
        png._chunk(b"IDAT", zlib.compress(bytes([1] + [0] * 6) * 2)) + png._chunk(b"IEND", b"")
    with pytest.raises(ValueError, match="filter type 0"):
        png.decode_png(filtered)
    with pytest.raises(ValueError, match="scanlines must be uint8"):
        png.encode_png(lines, 3, 2)
    bad = lines.copy()
    bad[1, 0] = 4
    with pytest.raises(ValueError, match="filter byte 0"):
        png.encode_png(bad, 2, 2)


# ---- the command's arguments ----------------------------------------------------------------------------------------------------------------
def test_vis_argument_parsing():
    from deflow_amd import vis
    o = vis.parse_args(["dataset_path=/d", "res_name=run"])
    assert o["flow_source"] == "file" and o["panels"] is None and o["size"] == (1024, 1024) and o["legend"] == 32 and o["radius"] == 1
    assert o["view"] == (-51.2, -51.2, 10.0) and o["out_dir"] == os.path.join("/d", "vis_run") and o["every"] == 1 and not o["overwrite"]
    o = vis.parse_args(["dataset_path=/d", "flow_source=model", "checkpoint=/c/best.ckpt", "panels=est,err", "range=6.4", "res=0.2",
                        "legend=0", "every=3", "batch_size=2", "overwrite=true", "vmax=0.5", "vmax_err=0.25", "radius=0", "out_dir=/o",
                        "scenes=a,b", "ground_source=online", "num_workers=0"])
    assert o["res_name"] == "best" and o["panels"] == ["est", "err"] and o["size"] == (64, 64) and o["legend"] == 0 and o["every"] == 3
    assert o["batch_size"] == 2 and o["overwrite"] and o["out_dir"] == "/o" and o["scenes"] == ["a", "b"] and o["_rest"] == {"num_workers": "num_workers=0"}
    assert vis.parse_args(["dataset_path=/d", "res_name=r", "range=1.0", "res=0.1"])["legend"] == 7           # (20 - 5) // 2
    for bad, what in ((["dataset_path=/d", "res_name=r", "colour=hot"], "unknown key 'colour'"),
                      (["dataset_path=/d", "res_name=r", "panels=est,flow"], "bad value for panels"),
                      (["dataset_path=/d", "res_name=r", "panels=est,est"], "bad value for panels"),
                      (["dataset_path=/d", "res_name=r", "panels="], "bad value for panels"),
                      (["dataset_path=/d", "flow_source=model"], "flow_source=model needs checkpoint"),
                      (["dataset_path=/d", "res_name=r", "checkpoint=/c.ckpt"], "only read with flow_source=model"),
                      (["dataset_path=/d"], "bad value for res_name"),
                      (["res_name=r"], "usage"),
                      (["dataset_path=/d", "res_name=r", "radius=5"], "bad value for radius"),
                      (["dataset_path=/d", "res_name=r", "vmax=0"], "bad value for vmax"),
                      (["dataset_path=/d", "res_name=r", "res=0.01"], "pixels per side"),
                      (["dataset_path=/d", "res_name=r", "range=1.0", "legend=9"], "bad value for legend"),
                      (["dataset_path=/d", "res_name=r", "every=0"], "bad value for every"),
                      (["dataset_path=/d", "res_name=r", "flow_source=npz"], "bad value for flow_source"),
                      (["dataset_path=/d", "res_name=r", "overwrite"], "expected key=value")):
        with pytest.raises(SystemExit) as e:
            vis.parse_args(bad)
        assert what in str(e.value), (bad, str(e.value))


# ---- the entry points' guards return before any launch: no GPU needed -----------------------------------------------------------------------
def test_entry_point_guards():
    from deflow_amd import build
    from deflow_amd._lib import load
    build.build()
    lib = load()
    P, SHAPE, ARG, ALIGN = C.c_void_p, -1, -3, -2
    p = P(0x1000)

    def splat(B=1, N=8, inv=10.0, W=16, H=16, vmax=1.0, r=1, points=p, image=p, xmin=0.0):
        return lib.df_render_splat(points, p, p, p, B, N, xmin, 0.0, inv, W, H, vmax, r, image, P(0))

    def resolve(B=1, W=16, H=16, bg=0, L=0, image=p, out=p):
        return lib.df_render_resolve(image, B, W, H, bg, L, out, P(0))

    assert splat(B=0) == SHAPE and splat(B=65536) == SHAPE and splat(N=0) == SHAPE and splat(B=65535, N=40000) == SHAPE
    assert splat(W=0) == SHAPE and splat(W=4097) == SHAPE and splat(H=0) == SHAPE and splat(H=4097) == SHAPE
    assert splat(B=60, W=4096, H=4096) == SHAPE                                   # B H (1 + 3W) >= 2^31
    assert splat(r=-1) == ARG and splat(r=5) == ARG and splat(vmax=0.0) == ARG and splat(vmax=-1.0) == ARG and splat(inv=0.0) == ARG
    assert splat(vmax=float("nan")) == ARG and splat(inv=float("inf")) == ARG and splat(xmin=float("nan")) == ARG
    assert splat(points=P(0)) == ARG and splat(image=P(0)) == ARG and splat(image=P(0x1004)) == ALIGN
    assert resolve(B=0) == SHAPE and resolve(W=4097) == SHAPE and resolve(B=60, W=4096, H=4096) == SHAPE
    assert resolve(bg=-1) == ARG and resolve(bg=1 << 24) == ARG and resolve(L=-1) == ARG and resolve(L=6) == ARG      # 2 L + 5 = 17 > 16
    assert resolve(W=40, H=16, L=6) == ARG and resolve(image=P(0)) == ARG and resolve(out=P(0)) == ARG
    assert resolve(out=P(0x1002)) == ALIGN and resolve(image=P(0x1004)) == ALIGN
