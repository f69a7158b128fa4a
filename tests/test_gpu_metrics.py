"""GPU: the device-resident metrics accumulator (csrc/metrics.hip, deflow_amd/metrics_device.py) against the float64 restatement of the
batched semantics in tests/helpers/metrics_batch_ref.py (itself pinned to evaluate_batch + OfficialMetrics by
tests/test_metrics_device_cpu.py).  Every integer -- n, the 5 x 51 counts, how many frames had each value, the summary's weights, and
through them IoU's tp / fp / fn -- must be exactly equal; floats within 1e-9 relative and absolute (reordering a sum of at most 1e5
non-negative doubles moves it by at most n 2^-53 ~ 1e-11; the 100 x margin is the one tests/test_metrics.py uses); Angle within 1e-7
(arccos at 1, see that file)."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import metrics_batch_ref as MB  # noqa: E402

pytestmark = pytest.mark.gpu
POS = ("flow", "pose_flow", "pc0", "gt_flow", "idx_c", "counts")
VAL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "av2_mini", "val")
SMALL = dict(voxel_size=[0.4, 0.4, 6], point_cloud_range=[-51.2, -51.2, -3, 51.2, 51.2, 3], grid_feature_size=[256, 256],
             decoder_option="gru", num_iters=2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def rpb():
    from deflow_amd.metrics_device import rows_per_block
    return rows_per_block()


@pytest.fixture(scope="module")
def main_batches(rpb):
    """the three main batches and their reference, computed once and left unchanged"""
    batches = [MB.make_batch(s, rpb) for s in MB.SEEDS]
    ref = MB.BatchRef()
    for nb in batches:
        ref.update(nb)
    return batches, ref


def args_of(nb, dev, **dtypes):
    t = lambda k: torch.from_numpy(np.ascontiguousarray(nb[k] if k not in dtypes else nb[k].astype(dtypes[k]))).to(dev)
    return [t(k) for k in POS], {k: t(k) for k in MB.MASK_KEYS if nb.get(k) is not None}


def feed(dm, nb, dev, **dtypes):
    pos, kw = args_of(nb, dev, **dtypes)
    dm.update(*pos, **kw)


def check(dm, ref):
    st = {k: v.cpu() for k, v in dm.state().items()}
    for k, want in ref.integers().items():
        got = st[k].numpy().reshape(want.shape)
        assert np.array_equal(got, want), (k, np.argwhere(got != want)[:8].tolist(), got[got != want][:8], want[got != want][:8])
    MB.same(ref.result(1), dm.result(1))
    MB.same(ref.result(2), dm.result(2))
    MB.same(ref.summary(), dm.summary())
    assert int(dm.status.cpu()) == ref.dropped


def test_three_batches_match_the_float64_restatement(dev, rpb, main_batches):
    """B = 6, N = 2 R + 40, counts {0, 1, R - 1, R, R + 1, 2 R + 7}, random injective idx_c, NaN rows in each input, every meta-class and an
    unevaluated category, both sides of 35 m, every speed regime"""
    from deflow_amd.metrics_device import DeviceMetrics, SUMMARY_KEYS
    batches, ref = main_batches
    assert batches[0]["flow"].shape == (6, 2 * rpb + 40, 3) and sorted(batches[0]["counts"]) == [0, 1, rpb - 1, rpb, rpb + 1, 2 * rpb + 7]
    dm = DeviceMetrics(dev)
    for nb in batches:
        feed(dm, nb, dev)
    check(dm, ref)
    assert tuple(MB.SUMMARY_KEYS) == tuple(SUMMARY_KEYS) and tuple(MB.V1_KEYS) == tuple(dm.V1_KEYS)
    assert set(dm.summary()) == set(SUMMARY_KEYS) and dm.result(1)["n"] > 3 * rpb
    assert "Three-way" in dm.table(1) and "WHEELED_VRU" in dm.table(2)
    dm.reset()
    assert all(int(v.abs().sum()) == 0 for v in dm.state().values()) and dm.summary() == {}


def test_boundaries_cell_by_cell(dev):
    """fp32 values on every threshold (box and radius 35 m, bucket edges 1.0 and 2.0, the 0.05 m dynamic threshold from both sides, an error
    of exactly 0.5 at |gt| = 5), every intermediate exact: the counts cell by cell"""
    from deflow_amd.metrics_device import DeviceMetrics
    nb = MB.boundary_batch()
    ref = MB.BatchRef()
    ref.update(nb)
    dm = DeviceMetrics(dev)
    feed(dm, nb, dev)
    got, want = dm.state()["count"].cpu().numpy(), ref.integers()["count"]
    for ci in range(5):
        for bi in range(51):
            assert got[ci, bi] == want[ci, bi], (ci, bi, got[ci, bi], want[ci, bi])
    assert got[1, 25] == 1 and got[3, 50] == 1 and got[4, 49] == 1 and got[2, 1] == 2 and int(dm.state()["n"].cpu()) == 11
    check(dm, ref)
    r1 = dm.result(1)
    # tp: the rows with speeds 1, 1, 2, 2-, fp32(0.05), 5, 0.5; fp: errors 0.25 and fp32(0.05) on static rows; fn: the row built as one
    assert r1["IoU"] == pytest.approx(7 / 10)
    # strictly accurate: the six rows without error; relaxed adds 0.5 at |gt| = 5 (relative) and the two errors of fp32(0.05) (absolute)
    assert r1["AccS"] == pytest.approx(6 / 11) and r1["AccR"] == pytest.approx(9 / 11)


@pytest.mark.parametrize("masks", [(), ("is_valid",), ("eval_mask",), ("categories",), ("is_valid", "eval_mask"), ("is_valid", "categories"),
                                   ("eval_mask", "categories"), ("is_valid", "eval_mask", "categories")])
def test_mask_combinations(dev, rpb, masks):
    """each of is_valid, eval_mask and categories absent and present (absent categories: all background in the tables, all foreground in the
    summary, as on the host); integer dtypes are converted on the device, labels clamped to 0..30 before they are narrowed"""
    from deflow_amd.metrics_device import DeviceMetrics
    nb = MB.make_batch(7, rpb, masks=masks, has=None)
    dtypes = {}
    if "categories" in masks:
        cats = nb["categories"].astype(np.int64)
        cats[0, :50], cats[1, :50] = 300, -4          # clamped to 30 (WHEELED_RIDER) and 0, never wrapped
        nb["categories"] = cats
    if "eval_mask" in masks:
        nb["eval_mask"] = nb["eval_mask"].astype(np.int32) * 256      # != 0 counts; a narrowing cast would make these 0
    if "is_valid" in masks and "eval_mask" in masks:
        dtypes["is_valid"] = np.uint8
    ref = MB.BatchRef()
    ref.update(nb)
    dm = DeviceMetrics(dev)
    feed(dm, nb, dev, **dtypes)
    check(dm, ref)


@pytest.mark.parametrize("has", ["mixed", "all", "none", None])
def test_skip_rule(dev, rpb, has):
    """a frame without has_eval_mask is skipped iff some frame of the batch has one; the summary's weight is the whole batch"""
    from deflow_amd.metrics_device import DeviceMetrics
    nb = MB.make_batch(9, rpb, has=has)
    ref = MB.BatchRef()
    ref.update(nb)
    dm = DeviceMetrics(dev)
    feed(dm, nb, dev)
    check(dm, ref)
    assert int(dm.state()["wsum"][3].cpu()) == 6


def test_status_word_counts_dropped_rows(dev, rpb):
    from deflow_amd.metrics_device import DeviceMetrics
    nb = MB.make_batch(5, rpb)
    big = int(np.argmax(nb["counts"]))
    nb["idx_c"][big, 3] = nb["flow"].shape[1]           # one past the end
    nb["idx_c"][big, rpb + 9] = -1
    nb["idx_c"][big, 2 * rpb + 1] = 2 ** 40
    ref = MB.BatchRef()
    ref.update(nb)
    assert ref.dropped == 3
    dm = DeviceMetrics(dev)
    assert int(dm.status.cpu()) == 0
    feed(dm, nb, dev)
    check(dm, ref)
    assert dm.status.dtype == torch.int32 and tuple(dm.status.shape) == (1,) and int(dm.status.cpu()) == 3


def test_two_runs_are_bit_identical_and_merge_adds(dev, main_batches):
    from deflow_amd.metrics_device import DeviceMetrics
    batches, ref = main_batches
    a, b, h0, h1 = (DeviceMetrics(dev) for _ in range(4))
    for nb in batches:
        feed(a, nb, dev)
        feed(b, nb, dev)
    for k, v in a.state().items():
        assert torch.equal(v, b.state()[k]), k
    feed(h0, batches[0], dev)
    for nb in batches[1:]:
        feed(h1, nb, dev)
    assert h0.merge_(h1) is h0
    for k, v in a.state().items():
        m = h0.state()[k]
        if v.dtype == torch.int64:
            assert torch.equal(v, m), k
        else:
            assert bool(((v - m).abs() <= 1e-12 * v.abs()).all()), (k, float((v - m).abs().max()))
    check(h0, ref)


def test_update_reads_nothing_back_and_replays_in_a_graph(dev, main_batches):
    """update() under torch's sync debug mode; update() captured once in a graph (one stream) and replayed on new contents of the same
    buffers gives the eager state bit for bit"""
    from deflow_amd.metrics_device import DeviceMetrics
    batches, _ = main_batches
    eager, strict, graphed = DeviceMetrics(dev), DeviceMetrics(dev), DeviceMetrics(dev)
    for nb in batches[:2]:
        feed(eager, nb, dev)
    staged = [args_of(nb, dev) for nb in batches[:2]]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for pos, kw in staged:
            strict.update(*pos, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k, v in eager.state().items():
        assert torch.equal(v, strict.state()[k]), k
    pos, kw = args_of(batches[2], dev)                  # the buffers the graph reads; a warm-up run sizes the workspace outside the capture
    graphed.update(*pos, **kw)
    graphed.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.update(*pos, **kw)
    for p2, k2 in staged:
        for dst, src in zip(pos, p2):
            dst.copy_(src)
        for k in kw:
            kw[k].copy_(k2[k])
        g.replay()
    torch.cuda.synchronize()
    for k, v in eager.state().items():
        assert torch.equal(v, graphed.state()[k]), k


def test_update_names_the_bad_argument(dev, rpb):
    from deflow_amd.metrics_device import DeviceMetrics
    nb = MB.make_batch(3, rpb)
    pos, kw = args_of(nb, dev)
    dm = DeviceMetrics(dev)
    for i, name in enumerate(POS):
        bad = list(pos)
        bad[i] = pos[i].cpu()
        with pytest.raises(TypeError, match=name):
            dm.update(*bad, **kw)
        bad[i] = pos[i].double() if pos[i].is_floating_point() else pos[i].to(torch.int16)
        with pytest.raises(ValueError, match=name):
            dm.update(*bad, **kw)
    for name in kw:
        with pytest.raises(ValueError, match=name):
            dm.update(*pos, **{**kw, name: kw[name][..., :-1]})
        with pytest.raises(ValueError, match=name):
            dm.update(*pos, **{**kw, name: kw[name].float()})
        with pytest.raises(TypeError, match=name):
            dm.update(*pos, **{**kw, name: kw[name].cpu()})
    assert all(int(v.abs().sum()) == 0 for v in dm.state().values())          # nothing was accumulated by the rejected calls


def _val_batch(dev, n=4):
    from deflow_amd.data import HDF5Dataset, collate_fn_pad
    ds = HDF5Dataset(VAL, eval=True)
    batch = collate_fn_pad([ds[i] for i in range(min(n, len(ds)))])
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def test_evaluate_batch_device_matches_evaluate_batch(dev):
    """one validation iteration on a small model (grid 256 x 256, 2 iterations): evaluate_batch_device against evaluate_batch on
    model(batch).  The tables: integers equal, floats 1e-9 (Angle 1e-7).  The host's summary is computed in fp32, so only its integer
    (n) is compared with it; the summary's floats are checked at 1e-9 against the float64 restatement fed the same padded tensors"""
    import deflow_amd
    from deflow_amd.metrics import OfficialMetrics, evaluate_batch
    from deflow_amd.metrics_device import DeviceMetrics, evaluate_batch_device
    torch.manual_seed(77)
    model = deflow_amd.DeFlow(**SMALL).to(dev).eval()
    batch = _val_batch(dev)
    assert "eval_mask" in batch and "flow_category_indices" in batch and "flow_is_valid" in batch
    om = OfficialMetrics()
    with torch.no_grad():
        m = evaluate_batch(model(batch), batch, om)
    dm = DeviceMetrics(dev)
    evaluate_batch_device(model, batch, dm)
    st = {k: v.cpu() for k, v in dm.state().items()}
    assert int(st["n"]) == om.n and om.n > 500 and torch.equal(st["count"], om.count)
    assert st["v1_cnt"].tolist() == [om.v1_cnt[k] for k in om.V1_KEYS]
    MB.same(om.result(1), dm.result(1))
    MB.same(om.result(2), dm.result(2))
    s = dm.summary()
    assert set(s) == set(m) and s["n"] == m["n"]
    ls = model.last_state
    nb = {"flow": ls["flow"], "pose_flow": ls["pose_flow"], "pc0": batch["pc0"], "gt_flow": batch["flow"], "idx_c": ls["idx_c0"],
          "counts": ls["counts0"], "is_valid": batch["flow_is_valid"], "eval_mask": batch["eval_mask"],
          "categories": batch["flow_category_indices"], "has_eval_mask": batch.get("has_eval_mask")}
    ref = MB.BatchRef()
    ref.update({k: (v.detach().cpu().numpy() if v is not None else None) for k, v in nb.items()})
    MB.same(ref.summary(), s)
    for k in ("EPE", "EPE_FD", "EPE_FS", "EPE_BS"):     # and the fp32 host line is the same quantity
        assert abs(s[k] - m[k]) <= 1e-4 * max(1.0, abs(m[k])), (k, s[k], m[k])


@pytest.mark.parametrize("version", [1, 2])
def test_eval_cli_device_matches_host(dev, tmp_path, capsys, version):
    """python -m deflow_amd.eval ... metrics_impl=device against metrics_impl=host on tests/golden/av2_mini/val: the leaderboard and its n
    (the host's `metrics` line is fp32 arithmetic; the device summary is pinned to float64 above), the same keys in the JSON line, the
    same table"""
    from deflow_amd import eval as E
    from oracle import ref_torch as O
    val = tmp_path / "sensor" / "val"
    shutil.copytree(VAL, val)
    torch.manual_seed(77)
    ref = O.DeFlow(**SMALL).eval()
    with torch.no_grad():
        for mod in ref.modules():
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                mod.weight.uniform_(0.6, 1.4); mod.bias.uniform_(-0.2, 0.2)
                mod.running_mean.uniform_(-0.3, 0.3); mod.running_var.uniform_(0.6, 1.5)
    ck = tmp_path / "model.ckpt"
    torch.save({"state_dict": {"model." + k: v for k, v in ref.state_dict().items()},
                "hyper_parameters": {"cfg": {"model": {"name": "deflow", "target": {"num_iters": 2, "decoder_option": "gru"}},
                                             "voxel_size": [0.4, 0.4, 6], "point_cloud_range": SMALL["point_cloud_range"], "batch_size": 4}}}, ck)
    lines, tables = {}, {}
    for impl in ("host", "device"):
        out = E.main([f"checkpoint={ck}", "av2_mode=val", f"dataset_path={tmp_path / 'sensor'}", "num_workers=0", "batch_size=4",
                      f"leaderboard_version={version}", f"metrics_impl={impl}"])
        cap = capsys.readouterr()
        lines[impl] = json.loads([l for l in cap.out.splitlines() if l.startswith("{")][-1])
        heads = ("Three-way", "class", "mean") + tuple(MB.META)
        tables[impl] = [l for l in cap.err.splitlines() if l.startswith(heads)]
        assert out["leaderboard"] == lines[impl]["leaderboard"] or version == 2      # (NaN cells do not compare equal)
    h, d = lines["host"], lines["device"]
    assert set(h) == set(d) and set(h["metrics"]) == set(d["metrics"]) and "metrics_impl" not in d
    MB.same(h["leaderboard"], d["leaderboard"])
    if version == 1:
        assert d["leaderboard"]["n"] == h["leaderboard"]["n"] > 1000
    assert d["metrics"]["n"] == h["metrics"]["n"]
    assert tables["host"] == tables["device"] and len(tables["host"]) == (1 if version == 1 else 7)


def test_train_cli_validation_line_device_matches_host(dev, tmp_path, capsys):
    """python -m deflow_amd.train ... metrics_impl=device: the per-epoch validation line is DeviceMetrics.summary(); with one validation
    batch it is the host's line (the host works in fp32: the integer equal, the floats to fp32 accuracy), and the key is not saved"""
    from deflow_amd import train as T
    vals = {}
    for impl in ("host", "device"):
        ck = tmp_path / f"{impl}.ckpt"
        T.main(["model=deflow", "lr=2e-4", "epochs=1", "batch_size=2", "loss_fn=deflowLoss", "model.target.num_iters=2",
                "voxel_size=[0.2, 0.2, 6]", "point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3]", "pairs_per_epoch=4",
                "points_per_cloud=1200", f"save_checkpoint={ck}", f"metrics_impl={impl}"])
        lines = [json.loads(l) for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        vals[impl] = [l for l in lines if "val" in l][-1]["val"]
        hp = torch.load(ck, map_location="cpu", weights_only=False)["hyper_parameters"]["cfg"]
        assert "metrics_impl" not in hp
    h, d = vals["host"], vals["device"]
    assert set(h) == set(d) and d["n"] == h["n"] > 0
    for k in h:
        assert abs(d[k] - h[k]) <= 1e-4 * max(1.0, abs(h[k])), (k, d[k], h[k])
