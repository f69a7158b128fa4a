"""GPU: the submission bodies (csrc/submit.hip, deflow_amd/submit.py, ``python -m deflow_amd.eval av2_mode=test``) against the numpy
restatement in tests/helpers/submit_ref.py.  Selection moves rows, the fp16 rounding is numpy's ``astype(float16)`` and the flag column is a
bit packing, so every comparison is exact: bytes against bytes."""
import json
import os
import pickle
import shutil
import sys
import types
import zipfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import submit_ref as UR  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], grid_feature_size=[64, 64])   # tests/test_gpu_save.py's
F = np.float32
B = 3
POISON = 0x5A
# fp32 values on and around fp16's edges: past the range, the tie at 65520, the largest finite, signed zeros, the subnormal edge
EDGE = np.array([7e4, -1e5, 65520.0, 65519.0, -65504.0, -0.0, 0.0, 2.0 ** -24, 2.0 ** -25, -(2.0 ** -25) * 1.5, 6.1e-5, 3e38], dtype=F)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


@pytest.fixture(scope="module")
def R():
    from deflow_amd import sweeps
    return sweeps.rows_per_block()


def make_rows(Bn, N, seed):
    """flow_est / dynamic as df_flow_compose writes them: finite fp32 (no NaN), flags 0 / 1 -- with fp16's edge values sprinkled in"""
    rng = np.random.default_rng(seed)
    flow = (rng.standard_normal((Bn, N, 3)) * (2.0, 0.5, 0.05)).astype(F)
    at = rng.random((Bn, N, 3)) < 0.05
    flow[at] = rng.choice(EDGE, size=int(at.sum()))
    dyn = (rng.random((Bn, N)) < 0.3).astype(np.uint8)
    return flow, dyn


def make_mask(Bn, N, mode, seed):
    rng = np.random.default_rng(seed + 1000)
    values = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=(Bn, N))
    if mode == "none":
        return np.zeros((Bn, N), dtype=np.uint8)
    if mode == "all":
        return values
    return np.where(rng.random((Bn, N)) < 0.4, values, 0).astype(np.uint8)


_CASES = {}


def case(N, mode):
    """inputs and both versions' reference bodies of one (N, mask) case, computed once and shared"""
    key = (N, mode)
    if key not in _CASES:
        flow, dyn = make_rows(B, N, seed=N * 7 + len(mode))
        mask = make_mask(B, N, mode, seed=N)
        count = np.array([N, N - 7, N // 2], dtype=np.int32)
        want = {v: UR.body_batch(flow, dyn, mask, count, v) for v in (1, 2)}
        for a in (flow, dyn, mask, count):
            a.setflags(write=False)
        _CASES[key] = (flow, dyn, mask, count, want)
    return _CASES[key]


def pack_poisoned(dev, flow, dyn, mask, count, version):
    """df_sweep_compact + df_submit_pack through the binding on a body of this test's own, every byte 0x5A beforehand"""
    from deflow_amd import submit, sweeps
    from deflow_amd._lib import call, ptr, stream
    Bn, N, _ = flow.shape
    d = lambda a: torch.from_numpy(np.array(a)).to(dev)
    flow_d, dyn_d, mask_d, count_d = d(flow), d(dyn), d(mask), d(count)
    _, row_of, _, kept = sweeps.compact_rows(flow_d, count_d, mask_d == 0)
    S = submit.body_stride(N)
    assert S % 64 == 0 and UR.body_len(N) <= S < UR.body_len(N) + 64
    body = torch.full((Bn, S), POISON, dtype=torch.uint8, device=dev)
    call("df_submit_pack", ptr(flow_d), ptr(dyn_d), ptr(row_of), ptr(kept), Bn, N, version, ptr(body), stream())
    return body, kept


def check_bodies(body, kept, want, what, poisoned):
    body, kept = body.cpu().numpy(), kept.cpu().numpy()
    assert body.dtype == np.uint8 and kept.dtype == np.int32
    assert kept.tolist() == [m for _, m in want], (what, kept.tolist())
    for b, (w, M) in enumerate(want):
        L = UR.body_len(M)
        got = body[b, :L]
        assert got.tobytes() == w.tobytes(), f"{what}: sample {b} (M = {M}): {int((got != w).sum())} of {L} bytes differ, first at {int(np.argmax(got != w))}"
        if poisoned:
            assert (body[b, L:] == POISON).all(), f"{what}: sample {b} (M = {M}): bytes behind L(M) = {L} were written"


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("mode", ["none", "all", "random"])
@pytest.mark.parametrize("which", ["R-1", "R", "R+1", "2R+3"])
def test_pack_rows(dev, R, which, mode, version):
    from deflow_amd import submit
    N = {"R-1": R - 1, "R": R, "R+1": R + 1, "2R+3": 2 * R + 3}[which]
    flow, dyn, mask, count, want = case(N, mode)
    print(f"[submit] N = {N}, {mode}, v{version}: counts {count.tolist()}, M {[m for _, m in want[version]]}")
    if mode == "none":
        assert [m for _, m in want[version]] == [0, 0, 0]
    if mode == "all":
        assert [m for _, m in want[version]] == count.tolist()
    body, kept = pack_poisoned(dev, flow, dyn, mask, count, version)
    check_bodies(body, kept, want[version], "df_submit_pack", poisoned=True)
    d = lambda a: torch.from_numpy(np.array(a)).to(dev)
    args = (d(flow), d(dyn), d(mask), d(count))
    a = submit.pack_rows(*args, version)
    assert tuple(a[0].shape) == (B, submit.body_stride(N)) and a[0].dtype == torch.uint8 and a[1].dtype == torch.int32
    check_bodies(*a, want[version], "pack_rows", poisoned=False)
    b = submit.pack_rows(args[0], args[1] != 0, args[2] != 0, args[3], version)          # bool flags and a bool mask are the same
    check_bodies(*b, want[version], "pack_rows(bool)", poisoned=False)
    if mode != "none":
        w = np.concatenate([x for x, _ in want[version]])
        assert (w == 0x7C).any() and (w == 0xFC).any()                   # the rows past the fp16 range became inf


@pytest.mark.parametrize("version", [1, 2])
def test_row_counts_around_the_byte_and_word_edges(dev, version):
    """M = 7, 8, 9, 63, 64, 65, 66 and 0: every residue mod 4 (the fp16 columns' padding), both sides of a flag byte and of a wave's 8 flag
    bytes, chosen rows scattered over N = 200 raw ones"""
    Ms = [7, 8, 9, 63, 64, 65, 66, 0]
    assert {m % 4 for m in Ms} == {0, 1, 2, 3}
    N, Bn = 200, len(Ms)
    rng = np.random.default_rng(77)
    flow, dyn = make_rows(Bn, N, seed=5)
    count = np.full(Bn, N - 3, dtype=np.int32)
    mask = np.zeros((Bn, N), dtype=np.uint8)
    for b, M in enumerate(Ms):
        mask[b, rng.choice(N - 3, size=M, replace=False)] = rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=M)
    mask[:, N - 3:] = 1                                                  # set, but behind count
    want = UR.body_batch(flow, dyn, mask, count, version)
    assert [m for _, m in want] == Ms
    body, kept = pack_poisoned(dev, flow, dyn, mask, count, version)
    check_bodies(body, kept, want, "df_submit_pack", poisoned=True)


def test_guards_return_their_codes_without_a_launch(dev):
    from deflow_amd import submit
    from deflow_amd._lib import call, ptr
    N = 16
    flow = torch.zeros(2, N, 3, device=dev)
    dyn = torch.zeros(2, N, dtype=torch.uint8, device=dev)
    row_of = torch.zeros(2, N, dtype=torch.int32, device=dev)
    kept = torch.zeros(2, dtype=torch.int32, device=dev)
    body = torch.full((2, submit.body_stride(N) + 8), POISON, dtype=torch.uint8, device=dev)
    ok = lambda **kw: [kw.get("flow", ptr(flow)), kw.get("dyn", ptr(dyn)), kw.get("row_of", ptr(row_of)), kw.get("kept", ptr(kept)),
                       kw.get("B", 2), kw.get("N", N), kw.get("version", 1), kw.get("body", ptr(body)), None]
    assert int(call("df_submit_body_stride", 0)) < 0 and int(call("df_submit_body_stride", -5)) < 0
    assert int(call("df_submit_body_stride", 1)) == 64 and int(call("df_submit_body_stride", 13)) == 128      # L(1) = 32, L(13) = 104
    assert int(call("df_submit_body_stride", 2 ** 31 - 1)) > 2 ** 33                                         # no 32-bit overflow
    for kw in (dict(B=0), dict(B=65536), dict(N=0), dict(N=-1), dict(B=65535, N=40000)):                     # the last: B S >= 2^31
        with pytest.raises(RuntimeError, match="DF_E_SHAPE"):
            call("df_submit_pack", *ok(**kw))
    for kw in (dict(flow=None), dict(dyn=None), dict(row_of=None), dict(kept=None), dict(body=None), dict(version=0), dict(version=3)):
        with pytest.raises(RuntimeError, match="DF_E_ARG"):
            call("df_submit_pack", *ok(**kw))
    with pytest.raises(RuntimeError, match="DF_E_ALIGN"):
        call("df_submit_pack", *ok(body=ptr(body) + 4))
    torch.cuda.synchronize()
    assert bool((body == POISON).all())                                  # nothing was launched
    # the Python layer names the argument
    cnt = torch.full((2,), N, dtype=torch.int32, device=dev)
    mask = torch.ones(2, N, dtype=torch.uint8, device=dev)
    submit.pack_rows(flow, dyn, mask, cnt, 1)
    with pytest.raises(TypeError, match="flow_est must be a CUDA tensor"):
        submit.pack_rows(flow.cpu(), dyn, mask, cnt, 1)
    with pytest.raises(TypeError, match="eval_mask must be a CUDA tensor"):
        submit.pack_rows(flow, dyn, mask.cpu(), cnt, 1)
    with pytest.raises(ValueError, match="flow_est must be torch.float32"):
        submit.pack_rows(flow.half(), dyn, mask, cnt, 1)
    with pytest.raises(ValueError, match="N >= 1"):
        submit.pack_rows(flow[:, :0], dyn[:, :0], mask[:, :0], cnt, 1)
    with pytest.raises(ValueError, match="dynamic must be"):
        submit.pack_rows(flow, dyn.int(), mask, cnt, 1)
    with pytest.raises(ValueError, match="eval_mask must be"):
        submit.pack_rows(flow, dyn, mask[:, :-1], cnt, 1)
    with pytest.raises(ValueError, match="count_raw must be torch.int32"):
        submit.pack_rows(flow, dyn, mask, cnt.long(), 1)
    with pytest.raises(ValueError, match="version must be 1 or 2"):
        submit.pack_rows(flow, dyn, mask, cnt, 3)


def test_graph_replay_on_overwritten_inputs(dev, R):
    from deflow_amd import submit
    N = R + 37
    d = lambda a: torch.from_numpy(np.array(a)).to(dev)
    cases = []
    for seed in (1, 2):
        flow, dyn = make_rows(B, N, seed=seed)
        mask = make_mask(B, N, "random", seed=seed)
        count = np.array([N, N - 7 * seed, N // 2], dtype=np.int32)
        cases.append((flow, dyn, mask, count, UR.body_batch(flow, dyn, mask, count, 1)))
    static = [d(a) for a in cases[0][:4]]
    submit.pack_rows(*static, 1)                                         # eager first: sizes everything
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                            # one stream, a linear chain
        body, kept = submit.pack_rows(*static, 1)
    for c in (cases[1], cases[0]):
        for s, a in zip(static, c[:4]):
            s.copy_(d(a))
        body.fill_(POISON)
        kept.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        check_bodies(body, kept, c[4], "replay", poisoned=True)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def small_model(dev, seed=31):
    import deflow_amd
    torch.manual_seed(seed)
    return deflow_amd.DeFlow(**SMALL, num_iters=2).to(dev).eval()


def street(N, seed):
    """a B = 2 cloud around the SMALL range: rows outside +-6.4 m, a ground plane near z = -0.33, NaN rows (tests/test_gpu_save.py's)"""
    rng = np.random.default_rng(seed)
    raw = np.empty((2, N, 3), dtype=F)
    raw[..., :2] = rng.uniform(-8.0, 8.0, (2, N, 2))
    raw[..., 2] = rng.uniform(-0.2, 2.0, (2, N))
    plane = rng.random((2, N)) < 0.3
    raw[..., 2][plane] = (-0.33 + 0.02 * rng.standard_normal(int(plane.sum()))).astype(F)
    raw[0, rng.choice(N, 5, replace=False), 0] = np.nan
    raw[1, rng.choice(N, 5, replace=False), 2] = np.nan
    count = np.array([N, N - N // 4], dtype=np.int32)
    raw[1, count[1]:] = np.nan
    return raw, count, plane.astype(np.uint8)


@pytest.mark.parametrize("version", [1, 2])
def test_submit_flow_against_host_filtering(dev, version):
    from deflow_amd import submit, sweeps
    model = small_model(dev)
    raw0, n0, drop0 = street(700, 3)
    raw1, n1, drop1 = street(640, 4)
    pose0 = np.tile(np.eye(4, dtype=F), (2, 1, 1))
    pose1 = pose0.copy()
    pose1[:, :3, 3] = (0.4, 0.02, 0.003)
    rng = np.random.default_rng(version)
    eval0 = np.where(rng.random((2, 700)) < 0.6, rng.choice(np.array([1, 255], dtype=np.uint8), size=(2, 700)), 0).astype(np.uint8)
    d = lambda a: torch.from_numpy(a).to(dev)
    args = (d(raw0), d(n0), d(drop0), d(raw1), d(n1), d(drop1), d(pose0), d(pose1))
    est, dyn = sweeps.SweepFlow(model).infer(*args)
    sf = submit.SubmitFlow(model)
    body, kept = sf.infer(*args, d(eval0), version=version)
    body2, kept2 = sf.infer(*args, d(eval0) != 0, version=version)
    # host filtering of SweepFlow.infer's output: boolean indexing, astype(float16) per column, packbits
    want = UR.body_batch(est.cpu().numpy(), dyn.cpu().numpy(), eval0, n0, version)
    assert dyn.any() and not dyn.all() and all(0 < m < 700 for _, m in want)
    check_bodies(body, kept, want, "SubmitFlow.infer", poisoned=False)
    check_bodies(body2, kept2, want, "SubmitFlow.infer (bool mask)", poisoned=False)


# ---- the command ----------------------------------------------------------------------------------------------------------------------------
def test_submission_command(dev, tmp_path, golden_dir, capsys):
    from deflow_amd import eval as E
    from deflow_amd import feather, submit, sweeps, train
    from deflow_amd.h5scene import H5File
    test_dir = tmp_path / "sensor" / "test"
    shutil.copytree(os.path.join(golden_dir, "av2_mini", "val"), test_dir)                 # never written under tests/golden
    model = small_model(dev, seed=47)
    cfg = dict(train.DEFAULTS)
    cfg.update({"voxel_size": SMALL["voxel_size"], "point_cloud_range": SMALL["point_cloud_range"], "model.target.num_iters": 2, "batch_size": 4})
    ckpt = str(tmp_path / "small_best.ckpt")
    train.save_checkpoint(ckpt, model, types.SimpleNamespace(opt=types.SimpleNamespace(state_dict=lambda: {})), cfg, 0, 0)
    with H5File(str(test_dir / "scene_val.h5")) as f:
        all_sweeps = sorted(f.keys(), key=int)
    with open(test_dir / "index_total.pkl", "rb") as f:
        index = [(str(s), str(t)) for s, t in pickle.load(f)]
    frames = [(s, t) for s, t in index if t != all_sweeps[-1]]                             # every indexed frame with a successor
    assert len(frames) >= 8
    # the expected members: SweepFlow on the same batches of 4, the restatement under the fixture's eval_mask
    ds, _ = submit.submission_frames(str(test_dir))
    items = [ds[i] for i in range(len(ds))]
    assert [(it["scene_id"], str(it["timestamp"])) for it in items] == sorted(frames, key=lambda e: (e[0], int(e[1])))
    sf = sweeps.SweepFlow(model)
    expected = {}
    for k in range(0, len(items), 4):
        hb = submit.collate_submit_pad(items[k:k + 4])
        db = {key: v.to(dev) for key, v in hb.items() if isinstance(v, torch.Tensor)}
        est, dyn = sf.infer(db["raw0"], db["n0"], db["drop0"], db["raw1"], db["n1"], db["drop1"], db["pose0"], db["pose1"],
                            ego_motion=db.get("ego_motion"))
        est, dyn = est.cpu().numpy(), dyn.cpu().numpy()
        for i, it in enumerate(items[k:k + 4]):
            n = int(it["pc0"].shape[0])
            expected[f"{it['scene_id']}/{it['timestamp']}.feather"] = (est[i, :n], dyn[i, :n], it["eval_mask"].numpy())
    try:
        import pyarrow as pa
        import pyarrow.ipc
    except ImportError:
        pa = None
    for version in (1, 2):
        argv = [f"checkpoint={ckpt}", "av2_mode=test", f"dataset_path={tmp_path / 'sensor'}", f"leaderboard_version={version}", "num_workers=0"]
        out = E.main(argv)
        cap = capsys.readouterr()
        line = json.loads([x for x in cap.out.splitlines() if x.startswith("{")][-1])
        path = str(tmp_path / f"small_best.av2_submit_v{version}.zip")
        assert line["zip"] == path == out["zip"] and os.path.isabs(path) and path in cap.err
        assert sorted(os.listdir(tmp_path)) == sorted(["sensor", "small_best.ckpt"] + [f"small_best.av2_submit_v{v}.zip" for v in range(1, version + 1)])
        with zipfile.ZipFile(path) as z:
            assert z.namelist() == sorted(expected) and z.testzip() is None
            rows = 0
            for name, (est, dyn, mask) in expected.items():
                data = z.read(name)
                w, M = UR.body(est, dyn, mask, est.shape[0], version)
                assert M == int(mask.sum()) and M > 0
                rows += M
                whole = feather.feather_file(version, M, w)
                assert len(data) == len(whole) and data == whole, f"{name}: the member differs from the restatement's file"
                assert w.tobytes() in data                                                 # the body itself, byte for byte
                if pa is not None:
                    t = pa.ipc.open_file(pa.BufferReader(data)).read_all()
                    cols = UR.columns(est, dyn, mask, est.shape[0])
                    assert t.num_rows == M and t.schema.names == list(UR.ORDER[version])
                    for c in UR.ORDER[version]:
                        assert t.column(c).to_numpy().tobytes() == cols[c].tobytes(), (name, c)
        assert line["frames"] == len(expected) == len(frames) and line["rows"] == rows and line["leaderboard_version"] == version
        assert line["skipped"] == {"duplicate": 0, "no_eval_mask": 0, "no_successor": len(index) - len(frames)}
        first = open(path, "rb").read()
        E.main(argv + ["output=" + str(tmp_path / "again.zip")])                           # a second run: the same bytes
        capsys.readouterr()
        assert open(tmp_path / "again.zip", "rb").read() == first
        os.remove(tmp_path / "again.zip")
    # an index that names the scene's last sweep and one frame twice: both are left out and counted; test_data= names the directory
    with open(test_dir / "index_eval.pkl", "wb") as f:
        pickle.dump([list(frames[2]), ["scene_val", all_sweeps[-1]], list(frames[0]), list(frames[2])], f)
    out = E.main([f"checkpoint={ckpt}", "av2_mode=test", f"test_data={test_dir}", "output=" + str(tmp_path / "two.zip"), "ground_source=online"])
    capsys.readouterr()
    assert out["frames"] == 2 and out["skipped"] == {"duplicate": 1, "no_eval_mask": 0, "no_successor": 1}
    with zipfile.ZipFile(tmp_path / "two.zip") as z:
        assert z.namelist() == [f"{frames[0][0]}/{frames[0][1]}.feather", f"{frames[2][0]}/{frames[2][1]}.feather"]
