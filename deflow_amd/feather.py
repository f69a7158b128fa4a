"""The feather files of an Argoverse-2 scene-flow submission, written in-tree (pyarrow is not a dependency, as h5py is not one of
``h5scene.py``): ``feather_file(version, M, body_bytes)`` wraps a record-batch body -- what ``df_submit_pack`` writes on the GPU, DESIGN.md
section 6g -- into an uncompressed Arrow IPC file (Feather V2) with one record batch.

A feather file of a fixed four-column schema is a few hundred bytes of metadata around a body of plain column buffers:

    "ARROW1\\0\\0" | Schema message | RecordBatch message | body | end-of-stream marker | Footer | int32 footer length | "ARROW1"

Each message is ``0xFFFFFFFF``, an int32 metadata length, and a flatbuffer (Message.fbs / Schema.fbs / File.fbs of the Arrow format, whose
table layouts are restated below as slot numbers) padded to 8 bytes.  ``_Builder`` is the small flatbuffer emitter for the three tables.

UNPINNED: the column names, order and types in ``COLUMNS`` are recalled from av2's and OpenSceneFlow's ``write_output_file``; this table is
the one place to correct them.  The body layout follows from it: the buffers of the columns in order, each padded to 8 bytes."""
from __future__ import annotations

import struct
from typing import List, Sequence, Tuple

# version -> ((column name, "float16" | "bool"), ...), in file order
COLUMNS = {
    1: (("flow_tx_m", "float16"), ("flow_ty_m", "float16"), ("flow_tz_m", "float16"), ("is_dynamic", "bool")),
    2: (("is_valid", "bool"), ("flow_tx_m", "float16"), ("flow_ty_m", "float16"), ("flow_tz_m", "float16")),
}

MAGIC = b"ARROW1"
_CONTINUATION = 0xFFFFFFFF
_V5 = 4                                      # MetadataVersion.V5
_TYPE_FLOATING_POINT, _TYPE_BOOL = 3, 6      # the Type union of Schema.fbs
_HEADER_SCHEMA, _HEADER_RECORD_BATCH = 1, 3  # the MessageHeader union of Message.fbs


def _pad8(n: int) -> int:
    return (n + 7) & ~7


def buffer_lengths(version: int, M: int) -> List[int]:
    """the unpadded byte length of each column's data buffer at M rows, in file order"""
    if version not in COLUMNS:
        raise ValueError(f"feather: version must be 1 or 2, got {version!r}")
    if int(M) != M or M < 0:
        raise ValueError(f"feather: M must be a non-negative integer, got {M!r}")
    return [2 * M if t == "float16" else (M + 7) // 8 for _, t in COLUMNS[version]]


def body_len(M: int, version: int = 1) -> int:
    """L(M) = 3 pad8(2 M) + pad8(ceil(M / 8)): the length of a record-batch body of M rows (the same for both versions)"""
    return sum(_pad8(n) for n in buffer_lengths(version, M))


# ---- a minimal flatbuffer emitter ---------------------------------------------------------------------------------------------------------
class _Builder:
    """Builds a flatbuffer back to front, as the format's own builders do: children first, and every reference is an unsigned offset
    forward to a child.  Positions are kept as distances from the END of the buffer, which stay valid while the front grows; alignment is
    kept relative to the end, and ``finish`` pads the front so that it also holds relative to the start."""

    def __init__(self):
        self.b = bytearray()
        self.minalign = 1
        self._slots = None
        self._object_end = 0

    def _prep(self, size: int, extra: int = 0):
        """pad so that after ``extra`` more bytes the front is aligned to ``size``"""
        self.minalign = max(self.minalign, size)
        self.b[0:0] = bytes(-(len(self.b) + extra) % size)

    def _put(self, fmt: str, v):
        self.b[0:0] = struct.pack("<" + fmt, v)

    def _scalar(self, fmt: str, v):
        self._prep(struct.calcsize(fmt))
        self._put(fmt, v)

    def _uoffset(self, target: int):
        self._prep(4)
        self._put("I", len(self.b) + 4 - target)

    def string(self, s: str) -> int:
        raw = s.encode("utf-8")
        self._prep(4, len(raw) + 1)
        self.b[0:0] = raw + b"\0"
        self._put("I", len(raw))
        return len(self.b)

    def struct_vector(self, fmt: str, rows: Sequence[Tuple], align: int) -> int:
        """a vector of structs; ``fmt`` packs one of them (its padding spelled out)"""
        size = struct.calcsize("<" + fmt) * len(rows)
        self._prep(4, size)
        self._prep(align, size)
        for row in reversed(rows):
            self.b[0:0] = struct.pack("<" + fmt, *row)
        self._put("I", len(rows))
        return len(self.b)

    def offset_vector(self, targets: Sequence[int]) -> int:
        self._prep(4, 4 * len(targets))
        for t in reversed(targets):
            self._uoffset(t)
        self._put("I", len(targets))
        return len(self.b)

    def table(self, nslots: int, fields: Sequence[Tuple]) -> int:
        """``fields``: (slot, kind, value) with kind a struct format character for a scalar or "o" for a reference to a child built
        before.  Absent slots read as the schema's defaults.  Larger fields are laid down first, so that no padding is needed between."""
        object_end = len(self.b)
        slots = [0] * nslots
        order = sorted(fields, key=lambda f: -(4 if f[1] == "o" else struct.calcsize(f[1])))
        for slot, kind, value in order:
            if kind == "o":
                self._uoffset(value)
            else:
                self._scalar(kind, value)
            slots[slot] = len(self.b)
        self._prep(4)
        self._put("i", 0)                                    # the table's signed offset to its vtable, patched below
        table = len(self.b)
        for at in reversed(slots):
            self._put("H", table - at if at else 0)
        self._put("H", table - object_end)
        self._put("H", 2 * (nslots + 2))
        struct.pack_into("<i", self.b, len(self.b) - table, len(self.b) - table)    # the vtable lies before the table: positive
        return table

    def finish(self, root: int) -> bytes:
        self._prep(self.minalign, 4)
        self._uoffset(root)
        return bytes(self.b)


# ---- the three tables ---------------------------------------------------------------------------------------------------------------------
def _schema(fb: _Builder, version: int) -> int:
    """Schema {0 endianness (Little), 1 fields}; Field {0 name, 1 nullable, 2 type_type, 3 type, 5 children}; FloatingPoint {0 precision:
    HALF = 0, the default}; Bool {}"""
    fields = []
    for name, t in COLUMNS[version]:
        children = fb.offset_vector([])
        type_table = fb.table(1 if t == "float16" else 0, [])
        name_at = fb.string(name)
        fields.append(fb.table(7, [(0, "o", name_at), (1, "B", 1), (2, "B", _TYPE_FLOATING_POINT if t == "float16" else _TYPE_BOOL),
                                   (3, "o", type_table), (5, "o", children)]))
    return fb.table(4, [(1, "o", fb.offset_vector(fields))])


def _message(header_type: int, header, body_length: int) -> bytes:
    """Message {0 version, 1 header_type, 2 header, 3 bodyLength}, framed: continuation marker, metadata length, flatbuffer, padding"""
    fb = _Builder()
    fields = [(0, "h", _V5), (1, "B", header_type), (2, "o", header(fb))]
    if body_length:
        fields.append((3, "q", body_length))
    meta = fb.finish(fb.table(5, fields))
    meta += bytes(_pad8(len(meta)) - len(meta))
    return struct.pack("<Ii", _CONTINUATION, len(meta)) + meta


def _record_batch(fb: _Builder, version: int, M: int) -> int:
    """RecordBatch {0 length, 1 nodes: [FieldNode {length, null_count}], 2 buffers: [Buffer {offset, length}]}: per column a validity
    buffer of length 0 (no nulls) and the data buffer"""
    buffers, at = [], 0
    for n in buffer_lengths(version, M):
        buffers += [(at, 0), (at, n)]
        at += _pad8(n)
    buffers_at = fb.struct_vector("qq", buffers, 8)
    nodes_at = fb.struct_vector("qq", [(M, 0)] * len(COLUMNS[version]), 8)
    return fb.table(5, [(0, "q", M), (1, "o", nodes_at), (2, "o", buffers_at)])


def _footer(version: int, block: Tuple[int, int, int]) -> bytes:
    """Footer {0 version, 1 schema, 2 dictionaries: [Block], 3 recordBatches: [Block {offset, metaDataLength, 4 bytes of padding,
    bodyLength}]}"""
    fb = _Builder()
    batches = fb.struct_vector("qi4xq", [block], 8)
    dictionaries = fb.struct_vector("qi4xq", [], 8)
    schema = _schema(fb, version)
    return fb.finish(fb.table(5, [(0, "h", _V5), (1, "o", schema), (2, "o", dictionaries), (3, "o", batches)]))


def feather_file(version: int, M: int, body_bytes) -> bytes:
    """The file of M rows whose record-batch body is ``body_bytes`` (bytes, memoryview or a uint8 array of exactly ``body_len(M)`` bytes,
    laid out as DESIGN.md section 6g says).  M = 0 gives a valid empty file."""
    body = bytes(body_bytes)
    M = int(M)
    want = body_len(M, version)
    if len(body) != want:
        raise ValueError(f"feather: a body of {M} rows has {want} bytes, got {len(body)}")
    head = MAGIC + b"\0\0"
    schema = _message(_HEADER_SCHEMA, lambda fb: _schema(fb, version), 0)
    batch = _message(_HEADER_RECORD_BATCH, lambda fb: _record_batch(fb, version, M), len(body))
    footer = _footer(version, (len(head) + len(schema), len(batch), len(body)))
    return b"".join((head, schema, batch, body, struct.pack("<Ii", _CONTINUATION, 0), footer, struct.pack("<i", len(footer)), MAGIC))
