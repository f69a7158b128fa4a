"""A PNG writer and reader for exactly what ``deflow_amd.vis`` produces: 8-bit RGB, non-interlaced, every scanline with filter type 0
(None) -- the layout ``render.render_rows`` leaves on the device, so the host only deflates and frames it.  stdlib ``zlib`` alone (in-tree
like ``h5scene.py`` and ``feather.py``: no imaging library is a dependency).  No time stamp or other ancillary chunk is written: the same
scanlines give the same bytes."""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def encode_png(scanlines, W: int, H: int, level: int = 6) -> bytes:
    """scanlines: uint8 [H, 1 + 3W] (numpy array, CPU tensor or bytes), each line a 0 filter byte and W RGB pixels -> the file's bytes"""
    W, H = int(W), int(H)
    if W < 1 or H < 1:
        raise ValueError(f"png: W and H must be >= 1, got {W} x {H}")
    if isinstance(scanlines, (bytes, bytearray, memoryview)):
        a = np.frombuffer(scanlines, dtype=np.uint8)
    else:
        a = np.asarray(scanlines)
    if a.dtype != np.uint8 or a.size != H * (1 + 3 * W):
        raise ValueError(f"png: scanlines must be uint8 with H (1 + 3 W) = {H * (1 + 3 * W)} bytes, got {a.dtype} with {a.size}")
    a = np.ascontiguousarray(a).reshape(H, 1 + 3 * W)
    if a[:, 0].any():
        raise ValueError("png: every scanline must start with filter byte 0")
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)          # 8 bits, colour type 2 (RGB), deflate, adaptive filtering, no interlace
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(a.tobytes(), int(level))) + _chunk(b"IEND", b"")


def write_png(path: str, scanlines, W: int, H: int, level: int = 6) -> str:
    """``encode_png`` into ``path``, through a temporary file and ``os.replace``"""
    data = encode_png(scanlines, W, H, level)
    tmp = f"{path}.tmp.{os.getpid()}"
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)
    return path


def decode_png(data: bytes) -> np.ndarray:
    """the subset ``encode_png`` writes -> uint8 [H, W, 3]; anything else is a ValueError saying what"""
    if data[:8] != SIGNATURE:
        raise ValueError("png: not a PNG file (bad signature)")
    at, chunks = 8, []
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError("png: truncated chunk")
        (n,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        if len(body) != n or at + 12 + n > len(data):
            raise ValueError(f"png: truncated {kind!r} chunk")
        if struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError(f"png: bad CRC in the {kind!r} chunk")
        chunks.append((kind, body))
        at += 12 + n
        if kind == b"IEND":
            break
    if not chunks or chunks[0][0] != b"IHDR" or len(chunks[0][1]) != 13 or chunks[-1][0] != b"IEND":
        raise ValueError("png: IHDR first and IEND last expected")
    W, H, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    if depth != 8 or ctype != 2:
        raise ValueError(f"png: only 8-bit RGB is read (bit depth {depth}, colour type {ctype})")
    if lace != 0:
        raise ValueError("png: interlaced files are not read")
    if comp != 0 or flt != 0 or W < 1 or H < 1:
        raise ValueError("png: bad IHDR")
    for kind, _ in chunks[1:-1]:
        if kind != b"IDAT" and not (kind[0] & 0x20):          # an unknown critical chunk (upper-case first letter)
            raise ValueError(f"png: critical chunk {kind!r} is not read")
    raw = zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT"))
    if len(raw) != H * (1 + 3 * W):
        raise ValueError(f"png: {len(raw)} bytes of image data, {H * (1 + 3 * W)} expected")
    a = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + 3 * W)
    if a[:, 0].any():
        raise ValueError("png: only filter type 0 (None) is read")
    return a[:, 1:].reshape(H, W, 3).copy()


def read_png(path: str) -> np.ndarray:
    with open(path, "rb") as f:
        return decode_png(f.read())
