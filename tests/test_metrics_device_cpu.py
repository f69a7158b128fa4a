"""CPU: (1) the float64 restatement of the BATCHED metric semantics (tests/helpers/metrics_batch_ref.py: gather by idx_c, masks, skip rule,
per-frame accumulation, summary weighting) pinned to the existing host code -- evaluate_batch + OfficialMetrics -- on the same padded
batches, and, on the seeds the GPU test uses, every integer of the two equal (no random row sits on a threshold; the host's torch.norm and
the restatement's sequential norm differ in the last bit, which matters only there -- if a seed fails that, change the seed);
(2) the new C entries reject NULL buffers and bad sizes with DF_E_* before any launch (the pattern of tests/test_abi.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import metrics_batch_ref as MB  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from deflow_amd import build
    from deflow_amd._lib import load
    build.build()
    return load()


@pytest.fixture(scope="module")
def rpb(lib):
    r = int(lib.df_metrics_rows_per_block())
    assert r >= 64 and r % 64 == 0
    return r


def host_product(batches):
    """evaluate_batch + OfficialMetrics + eval.py's weighting on float64 copies of the padded batches.  The model's flow is handed over as
    float64(est) - float64(pose_flow) with est the fp32 sum: the difference of two fp32 values is exact in double, so the host's
    pose_flow + flow is that est again"""
    from deflow_amd.metrics import OfficialMetrics, evaluate_batch
    om, tot, wsum = OfficialMetrics(), {}, {}
    t = torch.from_numpy
    for nb in batches:
        B = nb["flow"].shape[0]
        res = {"flow": [], "pc0_valid_point_idxes": [], "pose_flow": []}
        for b in range(B):
            c = int(nb["counts"][b])
            vi = nb["idx_c"][b, :c]
            with np.errstate(all="ignore"):
                est = (nb["pose_flow"][b, vi] + nb["flow"][b, :c]).astype(np.float32)
                res["flow"].append(t(est.astype(np.float64) - nb["pose_flow"][b, vi].astype(np.float64)))
            res["pc0_valid_point_idxes"].append(t(vi))
            res["pose_flow"].append(t(nb["pose_flow"][b].astype(np.float64)))
        batch = {"pc0": t(nb["pc0"].astype(np.float64)), "flow": t(nb["gt_flow"].astype(np.float64)), "pose0": [None] * B}
        for src, dst in (("is_valid", "flow_is_valid"), ("eval_mask", "eval_mask"), ("categories", "flow_category_indices"),
                         ("has_eval_mask", "has_eval_mask")):
            if nb.get(src) is not None:
                batch[dst] = t(np.ascontiguousarray(nb[src]))
        m = evaluate_batch(res, batch, om)
        for k, v in m.items():
            tot[k] = tot.get(k, 0.0) + v * B
            wsum[k] = wsum.get(k, 0) + B
    return om, {k: tot[k] / wsum[k] for k in tot}, wsum


def check_against_host(batches):
    ref = MB.BatchRef()
    for nb in batches:
        ref.update(nb)
    om, summary, wsum = host_product(batches)
    MB.same(ref.result(1), om.result(1))
    MB.same(ref.result(2), om.result(2))
    MB.same(ref.summary(), summary)
    ints = ref.integers()
    assert int(ints["n"][0]) == om.n
    assert np.array_equal(ints["count"], om.count.numpy())
    assert ints["v1_cnt"].tolist() == [om.v1_cnt[k] for k in MB.V1_KEYS]
    assert ints["wsum"].tolist() == [wsum.get(k, 0) for k in MB.SUMMARY_KEYS]
    return ref


def test_helper_matches_the_host_code_on_the_gpu_tests_seeds(rpb):
    ref = check_against_host([MB.make_batch(s, rpb) for s in MB.SEEDS])
    ints = ref.integers()
    # the batches do what the GPU test needs them to: every meta-class, the static bucket, the open bucket, all eight version-1 values
    assert (ints["count"].sum(1) > 0).all() and (ints["count"][:, 0] > 0).all() and ints["count"][:, 50].sum() > 0
    assert (ints["v1_cnt"] > 0).all() and (ints["wsum"] > 0).all() and ref.dropped == 0


@pytest.mark.parametrize("masks", [(), ("is_valid",), ("eval_mask",), ("categories",), ("is_valid", "categories"), ("eval_mask", "categories"),
                                   ("is_valid", "eval_mask")])
def test_helper_matches_the_host_code_without_some_masks(rpb, masks):
    check_against_host([MB.make_batch(7, rpb, masks=masks, has=None)])


@pytest.mark.parametrize("has", ["mixed", "all", "none", None])
def test_helper_skip_rule(rpb, has):
    ref = check_against_host([MB.make_batch(9, rpb, has=has)])
    assert ref.integers()["wsum"][3] == 6          # ("n" always exists) the weight is the whole batch, skipped samples included


def test_helper_boundaries():
    ref = check_against_host([MB.boundary_batch()])
    c = ref.integers()["count"]
    # CAR: speed 1.0 is edge 25 -> bucket 25 (the point at radius exactly 35 and the |gt| = 5 row's speed 5 -> open bucket)
    assert c[1, 25] == 1 and c[1, 50] == 1 and c[3, 50] == 1 and c[4, 49] == 1 and c[2, 1] == 2 and c[0, 0] == 2 and c[4, 1] == 1
    assert int(c.sum()) == 9 and ref.n == 11       # all rows but the one a hair outside the box


def test_helper_counts_dropped_rows(rpb):
    nb = MB.make_batch(5, rpb)
    big = int(np.argmax(nb["counts"]))
    full = MB.BatchRef()
    full.update(nb)
    nb["idx_c"][big, 3] = nb["flow"].shape[1]
    nb["idx_c"][big, 9] = -1
    cut = MB.BatchRef()
    cut.update(nb)
    assert cut.dropped == 2 and full.dropped == 0 and cut.n <= full.n


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------
def test_metrics_entries_reject_bad_arguments_without_launching(lib, rpb):
    P = C.c_void_p
    ok = P(0x1000)
    rows = lambda B, N, **kw: lib.df_metrics_rows(*[kw.get(k, ok) for k in ("flow", "pose_flow", "pc0", "gt_flow", "idx_c", "counts")],
                                                  P(0), P(0), P(0), B, N, kw.get("edges", ok), kw.get("ws", ok), P(0), P(0))
    acc = lambda B, N, **kw: lib.df_metrics_accumulate(kw.get("counts", ok), P(0), B, N, kw.get("ws", ok), kw.get("state_f", ok),
                                                       kw.get("state_i", ok), P(0))
    for k in ("flow", "pose_flow", "pc0", "gt_flow", "idx_c", "counts", "edges", "ws"):
        assert rows(2, 100, **{k: P(0)}) == -3, k                              # DF_E_ARG
    for k in ("counts", "ws", "state_f", "state_i"):
        assert acc(2, 100, **{k: P(0)}) == -3, k
    for B, N in ((0, 100), (-1, 100), (65536, 100), (2, 0), (2, -5), (65535, 32769), (2, 2 ** 30)):      # B * N >= 2^31
        assert rows(B, N) == -1 and acc(B, N) == -1, (B, N)                   # DF_E_SHAPE
        assert lib.df_metrics_ws_bytes(B, N) < 0
    assert rows(2, 100, ws=P(0x1004)) == -2 and acc(2, 100, ws=P(0x1004)) == -2            # DF_E_ALIGN
    # the workspace: per block and per frame 519 doubles + 270 counts
    per = 519 * 8 + 270 * 4
    assert lib.df_metrics_ws_bytes(1, 1) == 2 * per and lib.df_metrics_ws_bytes(3, rpb) == 6 * per
    assert lib.df_metrics_ws_bytes(3, rpb + 1) == 9 * per and lib.df_metrics_ws_bytes(65535, 32768) > 2 ** 31


def test_device_metrics_needs_a_cuda_device():
    from deflow_amd.metrics_device import DeviceMetrics
    with pytest.raises(TypeError, match="CUDA device"):
        DeviceMetrics("cpu")


def test_metrics_impl_is_validated_and_never_a_hyper_parameter():
    from deflow_amd import eval as E
    from deflow_amd import train as T
    with pytest.raises(SystemExit, match="metrics_impl"):
        E.main(["checkpoint=/nonexistent.ckpt", "metrics_impl=fast"])
    with pytest.raises(SystemExit, match="metrics_impl"):
        T.main(["metrics_impl=fast"])
    assert "metrics_impl" not in T.DEFAULTS
    assert T.split_metrics_impl(["lr=1e-4", "metrics_impl=device"]) == ("device", ["lr=1e-4"])
    assert T.split_metrics_impl(["lr=1e-4"]) == ("host", ["lr=1e-4"])
