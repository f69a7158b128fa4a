"""CPU: the numpy restatement of the submission body (tests/helpers/submit_ref.py) on hand-made rows, the in-tree
feather writer read back by pyarrow and pandas, and the host side of ``python -m deflow_amd.eval av2_mode=test``: the argument parser, the
collate, the frame selection and the zip.  Every comparison is exact."""
import io
import os
import pickle
import shutil
import sys
import zipfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import submit_ref as UR  # noqa: E402

F = np.float32
# fp32 value -> its fp16 bits, written down by hand: past the range (inf), the tie at 65520 (to even: inf), the largest finite, signed
# zero, a value that rounds (0.1), the smallest subnormal and the tie below it (to even: zero)
SPECIAL = [(7e4, 0x7C00), (-1e5, 0xFC00), (65520.0, 0x7C00), (65519.0, 0x7BFF), (-65504.0, 0xFBFF), (-0.0, 0x8000), (0.0, 0x0000),
           (1.0, 0x3C00), (0.1, 0x2E66), (2.0 ** -24, 0x0001), (2.0 ** -25, 0x0000), (-1.5, 0xBE00)]
MS = (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65)


def hand_rows(M, seed):
    """M selected rows among N = M + 9 raw ones (unselected rows in between and behind count hold values that must not appear):
    -> flow_est [N,3], dynamic [N], eval_mask [N] (non-zero values 1, 2, 255), count, and the selected values / flags"""
    rng = np.random.default_rng(seed)
    N = M + 9
    count = N - 2
    mask = np.zeros(N, dtype=np.uint8)
    rows = np.sort(rng.choice(count, size=M, replace=False))
    mask[rows] = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=M)
    mask[count:] = 1                                                     # set, but behind count: not selected
    flow = np.full((N, 3), 777.0, dtype=F)
    vals = (rng.standard_normal((M, 3)) * 3).astype(F)
    for i in range(M):
        vals[i, i % 3] = SPECIAL[i % len(SPECIAL)][0]
    flow[rows] = vals
    dyn = np.ones(N, dtype=np.uint8)
    flags = rng.random(M) < 0.5
    dyn[rows] = np.where(flags, rng.choice(np.array([1, 255], dtype=np.uint8), size=M), 0)
    return flow, dyn, mask, count, vals, flags


def half_bits(v):
    for s, bits in SPECIAL:
        if np.float32(s).tobytes() == np.float32(v).tobytes():
            return bits
    with np.errstate(all="ignore"):
        return int(np.float32(v).astype(np.float16).view(np.uint16))


def by_hand(M, version, vals, flags):
    """the body stated byte by byte, without packbits or array casts of whole columns"""
    P = -(-2 * M // 8) * 8
    Q = -(-(-(-M // 8)) // 8) * 8
    out = bytearray(3 * P + Q)
    cols, bits = (0, 3 * P) if version == 1 else (Q, 0)
    for p in range(M):
        for c in range(3):
            h = half_bits(vals[p, c])
            out[cols + c * P + 2 * p] = h & 0xFF
            out[cols + c * P + 2 * p + 1] = h >> 8
        if version == 2 or flags[p]:
            out[bits + (p >> 3)] |= 1 << (p & 7)
    return bytes(out)


def test_special_values_round_as_written():
    with np.errstate(all="ignore"):
        for v, bits in SPECIAL:
            assert int(np.float32(v).astype(np.float16).view(np.uint16)) == bits, v


def test_three_rows_written_out():
    flow = np.array([[1.0, -1.5, 7e4], [9, 9, 9], [0.1, 0.0, -0.0], [-1e5, 65519.0, 1.0], [5, 5, 5]], dtype=F)
    dyn = np.array([1, 1, 0, 255, 1], dtype=np.uint8)
    mask = np.array([2, 0, 1, 255, 1], dtype=np.uint8)
    b1, M = UR.body(flow, dyn, mask, 4, 1)                               # row 4 lies behind count
    assert M == 3 and UR.body_len(3) == 32
    assert b1.tobytes() == bytes([0x00, 0x3C, 0x66, 0x2E, 0x00, 0xFC, 0, 0,            # tx: 1.0, 0.1, -inf, padding
                                  0x00, 0xBE, 0x00, 0x00, 0xFF, 0x7B, 0, 0,            # ty: -1.5, 0.0, 65504
                                  0x00, 0x7C, 0x00, 0x80, 0x00, 0x3C, 0, 0,            # tz: +inf, -0.0, 1.0
                                  0b101, 0, 0, 0, 0, 0, 0, 0])                         # is_dynamic: rows 0 and 3
    b2, _ = UR.body(flow, dyn, mask, 4, 2)
    assert b2.tobytes() == bytes([0b111, 0, 0, 0, 0, 0, 0, 0]) + b1.tobytes()[:24]     # is_valid first, then the same columns


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("M", MS)
def test_restatement_on_hand_made_rows(M, version):
    flow, dyn, mask, count, vals, flags = hand_rows(M, seed=M + 100 * version)
    if M >= 3:
        with np.errstate(all="ignore"):
            assert np.isinf(vals.astype(np.float16)).any() and not np.isinf(vals).any()    # a value past the fp16 range
    assert np.array_equal(UR.select(mask, count), np.nonzero(mask[:count])[0])
    got, m = UR.body(flow, dyn, mask, count, version)
    assert m == M and got.dtype == np.uint8 and got.shape == (UR.body_len(M),)
    assert UR.body_len(M) == 3 * (-(-2 * M // 8) * 8) + -(-(-(-M // 8)) // 8) * 8
    assert got.tobytes() == by_hand(M, version, vals, flags)
    assert UR.body_len(13) == 104 and UR.pad8(26) == 32                              # 13 rows: columns at +0, +32, +64, bits at +96


# ---- the feather writer -------------------------------------------------------------------------------------------------------------------
def test_column_table():
    from deflow_amd import feather
    assert {v: tuple(n for n, _ in c) for v, c in feather.COLUMNS.items()} == UR.ORDER
    for v, c in feather.COLUMNS.items():
        assert sorted(t for _, t in c) == ["bool", "float16", "float16", "float16"]
        assert all((t == "bool") == (n in UR.FLAGS) for n, t in c)
    for M in MS + (13, 1000):
        assert feather.body_len(M, 1) == feather.body_len(M, 2) == UR.body_len(M)


def test_file_framing():
    """the container, without pyarrow: magic at both ends, the footer length in front of the trailing magic, 8-byte alignment of every
    part, the body where the framing says, and the end-of-stream marker behind it"""
    import struct
    from deflow_amd import feather
    flow, dyn, mask, count, _, _ = hand_rows(13, seed=1)
    for version in (1, 2):
        body, M = UR.body(flow, dyn, mask, count, version)
        data = feather.feather_file(version, M, body)
        assert data[:8] == b"ARROW1\0\0" and data[-6:] == b"ARROW1" and isinstance(data, bytes)
        at = 8
        lens = []
        for _ in range(2):                                               # Schema, RecordBatch
            cont, n = struct.unpack_from("<Ii", data, at)
            assert cont == 0xFFFFFFFF and n > 0 and n % 8 == 0 and at % 8 == 0
            lens.append(n)
            at += 8 + n
        assert data[at: at + len(body)] == body.tobytes()
        at += len(body)
        assert struct.unpack_from("<Ii", data, at) == (0xFFFFFFFF, 0)
        at += 8
        (flen,) = struct.unpack_from("<i", data, len(data) - 10)
        assert at % 8 == 0 and at + flen == len(data) - 10
        assert feather.feather_file(version, M, body.tobytes()) == data == feather.feather_file(version, M, memoryview(body))


@pytest.mark.parametrize("version", [1, 2])
def test_wrong_body_length_is_rejected(version):
    from deflow_amd import feather
    for M, n in ((0, 8), (1, 0), (13, 96), (13, 112), (8, UR.body_len(9))):
        with pytest.raises(ValueError, match=f"a body of {M} rows has {UR.body_len(M)} bytes, got {n}"):
            feather.feather_file(version, M, bytes(n))
    with pytest.raises(ValueError, match="version must be 1 or 2"):
        feather.feather_file(3, 0, b"")
    with pytest.raises(ValueError, match="M must be"):
        feather.body_len(-1)


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("M", [0, 1, 7, 8, 9, 13, 64, 65, 1000])
def test_pyarrow_reads_the_file(M, version):
    pa = pytest.importorskip("pyarrow")
    import pyarrow.ipc
    import pandas as pd
    from deflow_amd import feather
    flow, dyn, mask, count, vals, flags = hand_rows(M, seed=7 * M + version)
    body, m = UR.body(flow, dyn, mask, count, version)
    data = feather.feather_file(version, m, body)
    reader = pa.ipc.open_file(pa.BufferReader(data))
    assert reader.num_record_batches == 1
    table = reader.read_all()
    table.validate(full=True)
    assert table.schema.names == list(UR.ORDER[version])
    for name, field in zip(UR.ORDER[version], table.schema):
        assert field.type == (pa.bool_() if name in UR.FLAGS else pa.float16()), (name, field.type)
    assert table.num_rows == M and all(col.null_count == 0 for col in table.columns)
    want = UR.columns(flow, dyn, mask, count)
    with np.errstate(all="ignore"):
        assert np.array_equal(want["flow_tx_m"].view(np.uint16), vals[:, 0].astype(np.float16).view(np.uint16))
    assert np.array_equal(want["is_dynamic"], flags)
    expected = pa.table({name: pa.array(want[name]) for name in UR.ORDER[version]})
    assert table.schema.equals(expected.schema) and table.equals(expected)
    for name in UR.ORDER[version]:                                       # and bit for bit: -0.0 and inf included
        got = table.column(name).to_numpy()
        assert got.dtype == want[name].dtype and got.tobytes() == want[name].tobytes(), name
    frame = pd.read_feather(io.BytesIO(data))
    assert list(frame.columns) == list(UR.ORDER[version]) and frame.equals(expected.to_pandas())


# ---- the command's host side --------------------------------------------------------------------------------------------------------------
def test_parser_accepts_the_reference_command_lines():
    from deflow_amd import eval as E
    # [REF README.md:90-91]
    for v in (1, 2):
        o = E.parse_test_args(["checkpoint=/home/kin/deflow_best.ckpt", "av2_mode=test", f"leaderboard_version={v}"])
        assert o["version"] == v and o["checkpoint"] == "/home/kin/deflow_best.ckpt" and o["test_dir"] is None
        assert o["output"] == f"/home/kin/deflow_best.av2_submit_v{v}.zip" and o["ground_source"] == "auto" and o["inference_dtype"] is None
    # [REF assets/slurm/2_eval.sh:28-30]
    o = E.parse_test_args(["wandb_mode=online", "dataset_path=/scratch/local/av2/sensor", "av2_mode=test", "save_res=True", "checkpoint=a.ckpt"])
    assert o["version"] == 1 and o["test_dir"] == "/scratch/local/av2/sensor/test" and o["output"] == "a.av2_submit_v1.zip"
    o = E.parse_test_args(["checkpoint=a.ckpt", "av2_mode=test", "dataset_path=/d", "test_data=/t", "output=/o/x.zip", "ground_source=online",
                           "batch_size=4", "num_workers=2", "inference_dtype=bf16", "leaderboard_version=2"])
    assert o["test_dir"] == "/t" and o["output"] == "/o/x.zip" and o["ground_source"] == "online" and o["inference_dtype"] == "bf16"
    assert o["_given"]["batch_size"] == "batch_size=4" and set(E.TEST_OWN_KEYS) <= set(o["_given"])
    for bad in ("leaderboard_version=3", "leaderboard_version=x"):
        with pytest.raises(SystemExit, match="leaderboard_version must be"):
            E.parse_test_args(["checkpoint=a.ckpt", "av2_mode=test", bad])
    for bad in ("ground_source=lidar", "batch_size=0", "num_workers=-1", "inference_dtype=fp8", "output=", "test_data="):
        with pytest.raises(SystemExit, match="bad value for " + bad.split("=")[0]):
            E.parse_test_args(["checkpoint=a.ckpt", "av2_mode=test", bad])
    with pytest.raises(SystemExit, match="expected key=value"):
        E.parse_test_args(["checkpoint=a.ckpt", "av2_mode=test", "verbose"])
    with pytest.raises(SystemExit, match="usage"):
        E.parse_test_args(["av2_mode=test"])
    # no data named: the command stops before it touches a GPU
    with pytest.raises(SystemExit, match="needs the data"):
        E.main(["checkpoint=a.ckpt", "av2_mode=test"])
    with pytest.raises(SystemExit, match="unknown av2_mode=train"):
        E.main(["checkpoint=a.ckpt", "av2_mode=train"])


def test_save_points_at_the_command():
    from deflow_amd import save
    with pytest.raises(SystemExit, match=r"feather.*deflow_amd\.eval.*av2_mode=test"):
        save.parse_args(["checkpoint=a.ckpt", "dataset_path=d", "av2_mode=test"])


def test_collate_and_frames(golden_dir, tmp_path):
    from deflow_amd import submit, sweeps
    src = os.path.join(golden_dir, "av2_mini", "val")
    ds, skipped = submit.submission_frames(src)
    assert skipped == {"duplicate": 0, "no_eval_mask": 0, "no_successor": 0} and len(ds) == 10
    items = [ds[i] for i in range(3)]
    got, base = submit.collate_submit_pad(items), sweeps.collate_raw_pad(items)
    assert set(got) == set(base) | {"eval0"}                             # collate_raw_pad's keys are unchanged
    for k, v in base.items():
        assert torch.equal(got[k].view(torch.int32), v.view(torch.int32)) if isinstance(v, torch.Tensor) and v.dtype == torch.float32 \
            else (torch.equal(got[k], v) if isinstance(v, torch.Tensor) else got[k] == v)
    e = got["eval0"]
    assert e.dtype == torch.uint8 and tuple(e.shape) == tuple(got["drop0"].shape)
    for i, it in enumerate(items):
        n = int(it["pc0"].shape[0])
        assert torch.equal(e[i, :n] != 0, it["eval_mask"]) and not bool(e[i, n:].any()) and bool(it["eval_mask"].any())
    with pytest.raises(KeyError, match="has no eval_mask"):
        submit.collate_submit_pad([{k: v for k, v in items[0].items() if k != "eval_mask"}])
    # an index that lists the scene's last sweep, a frame twice and (from the training split) frames without a mask
    d = tmp_path / "test"
    shutil.copytree(src, d)
    shutil.copy(os.path.join(golden_dir, "av2_mini", "train", "scene_a.h5"), d / "scene_a.h5")
    with open(d / "index_total.pkl", "rb") as f:
        index = pickle.load(f)
    from deflow_amd.h5scene import H5File
    with H5File(str(d / "scene_val.h5")) as f:
        last = sorted(f.keys(), key=int)[-1]
    with H5File(str(d / "scene_a.h5")) as f:
        a_sweeps = sorted(f.keys(), key=int)
        assert "eval_mask" not in f[a_sweeps[0]]
    with open(d / "index_eval.pkl", "wb") as f:
        pickle.dump([index[3], ["scene_val", last], index[0], index[3], ["scene_a", a_sweeps[0]], ["scene_a", a_sweeps[1]]], f)
    ds, skipped = submit.submission_frames(str(d), ground_source="online")
    assert ds.index_file == "index_eval.pkl" and skipped == {"duplicate": 1, "no_eval_mask": 2, "no_successor": 1}
    assert ds.data_index == [["scene_val", str(index[0][1])], ["scene_val", str(index[3][1])]]
    it = ds[1]
    assert it["timestamp"] == int(index[3][1]) and not bool(it["gm0"].any()) and "eval_mask" in it     # online: all-False ground masks


def test_zip_assembly(tmp_path):
    from deflow_amd import feather, submit
    members = []
    for k, (sid, ts, M) in enumerate((("scene_a", 315970000000000000, 5), ("scene_a", 315970000100000000, 0), ("scene_b", 7, 64))):
        flow, dyn, mask, count, _, _ = hand_rows(M, seed=k)
        body, m = UR.body(flow, dyn, mask, count, 1)
        members.append((sid, ts, feather.feather_file(1, m, body)))
    paths = [str(tmp_path / "a.zip"), str(tmp_path / "b.zip")]
    for p in paths:
        with submit.SubmissionZip(p) as z:
            names = [z.add(*m) for m in members]
        assert z.members == 3
    assert names == ["scene_a/315970000000000000.feather", "scene_a/315970000100000000.feather", "scene_b/7.feather"]
    assert sorted(os.listdir(tmp_path)) == ["a.zip", "b.zip"]            # the temporary files are gone
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read()
    with zipfile.ZipFile(paths[0]) as z:
        assert z.namelist() == names and z.testzip() is None
        assert all(i.date_time == (1980, 1, 1, 0, 0, 0) for i in z.infolist())
        for name, (_, _, data) in zip(names, members):
            assert z.read(name) == data
    with pytest.raises(ValueError, match="sorted order"):
        with submit.SubmissionZip(str(tmp_path / "c.zip")) as z:
            z.add("scene_b", 7, b"x")
            z.add("scene_a", 8, b"x")
    with pytest.raises(ValueError, match="sorted order"):
        with submit.SubmissionZip(str(tmp_path / "c.zip")) as z:
            z.add("scene_b", 7, b"x")
            z.add("scene_b", "7", b"x")                                  # the same frame twice
    assert sorted(os.listdir(tmp_path)) == ["a.zip", "b.zip"]            # a failed assembly leaves nothing behind
