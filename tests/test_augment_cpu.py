"""CPU: the training augmentation's definition (tests/helpers/augment_ref.py, the numpy restatement of include/deflow_amd.h's section) and
its configuration plumbing.  The device kernel is compared against the same restatement in tests/test_gpu_augment.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import augment_ref as AR  # noqa: E402

KEY = (20240116, 3)


# ---- Philox4x32-10: the published Random123 known answers -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    assert " ".join("%08x" % w for w in AR.philox(ctr, key)) == want


def test_vectorised_philox_equals_the_integer_one():
    for id_ in (0, -7, (1 << 32) + 5, 315969904359876000):
        rows = np.array([0, 1, 255, 65536, 2 ** 31 - 2], dtype=np.uint64)
        w = AR.philox_rows(id_, rows, 2, KEY)
        for i, r in enumerate(rows):
            assert tuple(int(x) for x in w[i]) == AR.philox((id_ & AR.MASK, (id_ >> 32) & AR.MASK, int(r), 2), KEY)


def test_uniform_and_bell_ranges():
    assert float(AR.u01(0)) == 0.0 and float(AR.u01(0xffffffff)) == 1.0 - 2.0 ** -24 and float(AR.u01(0x100)) == 2.0 ** -24
    assert float(AR.bell(0)) == -510.0 and float(AR.bell(0xffffffff)) == 510.0 and float(AR.bell(0x01020304)) == 10.0 - 510.0
    # the bound quoted everywhere: 510 / 147.8 standard deviations, and 147.8 is the standard deviation of four uniform bytes
    assert 510.0 / AR.BELL_STD <= 3.46 and abs(AR.BELL_STD - np.sqrt(4 * (256 ** 2 - 1) / 12.0)) < 0.01


# ---- draw statistics (deterministic: key (20240116, 3)) ----------------------------------------------------------------------------------------
def test_flip_rates():
    cfg = AR.Config(KEY[0], flip_x_p=0.5, flip_y_p=0.5)
    d = [AR.sample_draw(cfg, i, KEY[1]) for i in range(4096)]
    fx, fy = np.mean([x["sx"] < 0 for x in d]), np.mean([x["sy"] < 0 for x in d])
    print("flip rates", fx, fy)
    assert abs(fx - 0.5) <= 0.04 and abs(fy - 0.5) <= 0.04


def test_jitter_and_drop_statistics():
    w = AR.philox_rows(0, np.arange(20000), 1, KEY)
    unit = AR.bell(w[:, :3]) / AR.BELL_STD
    print("jitter std", unit.std(), "max", np.abs(unit).max())
    assert abs(unit.std() - 1.0) <= 0.02
    assert np.abs(unit).max() <= 3.46
    rate = np.mean(AR.u01(w[:, 3]) < 0.1)
    print("drop rate", rate)
    assert abs(rate - 0.1) <= 0.01


def test_sample_draw_ranges_and_purity():
    cfg = AR.Config(7, flip_x_p=0.3, flip_y_p=0.7, yaw_deg=45.0, height=0.5)
    for i in (0, -1, 1 << 40):
        d = AR.sample_draw(cfg, i, 2)
        assert d == AR.sample_draw(cfg, i, 2)
        assert abs(d["theta"]) <= cfg.yaw_max and abs(d["dz"]) <= cfg.height_max and abs(d["c"] ** 2 + d["s"] ** 2 - 1) < 1e-15
        assert d != AR.sample_draw(cfg, i, 3) and d != AR.sample_draw(AR.Config(8, 0.3, 0.7, 45.0, 0.5), i, 2)


# ---- algebra -------------------------------------------------------------------------------------------------------------------------------
def _rigid(rng):
    a = rng.uniform(-0.05, 0.05)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = rng.uniform(-1.5, 1.5, 3)
    return T


def test_inverse_and_flow_identity():
    rng = np.random.default_rng(0)
    cfg = AR.Config(11, yaw_deg=180.0, height=1.0, jitter_sigma=0.0)
    for i in range(8):
        d = AR.sample_draw(cfg, i, 0)
        A, Ai = AR.matrices(d)
        assert np.abs(Ai @ A - np.eye(4)).max() < 1e-15 and np.abs(A @ Ai - np.eye(4)).max() < 1e-15
        T = _rigid(rng)
        p = rng.uniform(-60, 60, (50, 3))
        flow = rng.standard_normal((50, 3))
        pose_flow = p @ T[:3, :3].T + T[:3, 3] - p
        p2, _ = AR.cloud(cfg, d, i, 0, p, 1)
        T2 = A @ T @ Ai
        pose_flow2 = p2 @ T2[:3, :3].T + T2[:3, 3] - p2
        flow2 = AR.linear(d, flow)
        L = A[:3, :3]
        assert np.abs((flow2 - pose_flow2) - (flow - pose_flow) @ L.T).max() < 1e-12
        # the poses: pose' p' = pose p for every point
        pose = _rigid(rng)
        assert np.abs((p2 @ (pose @ Ai)[:3, :3].T + (pose @ Ai)[:3, 3]) - (p @ pose[:3, :3].T + pose[:3, 3])).max() < 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_all_zero_configuration_is_the_identity(dtype):
    rng = np.random.default_rng(1)
    cfg = AR.Config(5, flip_x_p=0.0, flip_y_p=0.0, yaw_deg=0.0, height=0.0, jitter_sigma=0.0, drop_p=0.0)
    pc0 = rng.uniform(-60, 60, (2, 40, 3)).astype(np.float32)
    pc0[0, 5] = np.nan
    pc1 = rng.uniform(-60, 60, (2, 30, 3)).astype(np.float32)
    flow = rng.standard_normal((2, 40, 3)).astype(np.float32)
    T = np.stack([_rigid(rng), _rigid(rng)]).astype(np.float32)
    out = AR.apply(cfg, [3, -4], 9, pc0, pc1, flow, T, T, T, dtype=dtype)
    assert np.array_equal(out["pc0"], pc0.astype(dtype), equal_nan=True) and np.array_equal(out["pc1"], pc1.astype(dtype))
    assert np.array_equal(out["flow"], flow.astype(dtype))
    assert np.array_equal(out["T"], T.astype(np.float64)) and np.array_equal(out["pose0"], T.astype(np.float64))
    assert not out["drop0"].any() and not out["drop1"].any()


def test_dropped_rows_are_nan_in_place_and_input_nan_stays():
    rng = np.random.default_rng(2)
    cfg = AR.Config(5, 0.0, 0.0, 0.0, 0.0, 0.0, drop_p=0.25)
    pc = rng.uniform(-60, 60, (1, 400, 3)).astype(np.float32)
    pc[0, 17] = np.nan
    out = AR.apply(cfg, [1], 0, pc, pc)
    d0 = out["drop0"][0]
    assert 60 <= d0.sum() <= 140 and not np.array_equal(d0, out["drop1"][0])      # pc0 and pc1 rows draw their own words
    assert np.isnan(out["pc0"][0][d0]).all() and np.isnan(out["pc0"][0, 17]).all()
    keep = ~d0 & ~np.isnan(pc[0]).any(1)
    assert np.array_equal(out["pc0"][0][keep], pc[0][keep].astype(np.float64))


# ---- configuration ---------------------------------------------------------------------------------------------------------------------------
AUG_DEFAULTS = {"augment": False, "aug_flip_x_p": 0.5, "aug_flip_y_p": 0.5, "aug_yaw_deg": 0.0, "aug_height": 0.2, "aug_jitter_sigma": 0.01,
                "aug_drop_p": 0.0}


def test_parse_overrides_knows_the_keys_and_keeps_the_defaults(capsys):
    from deflow_amd import train
    cfg = train.parse_overrides([])
    assert {k: cfg[k] for k in AUG_DEFAULTS} == AUG_DEFAULTS and train.augmenter_from(cfg) is None
    cfg = train.parse_overrides(["augment=true", "aug_yaw_deg=30", "aug_drop_p=0.05", "aug_flip_y_p=0"])
    assert "unknown override" not in capsys.readouterr().err
    assert cfg["augment"] is True and cfg["aug_yaw_deg"] == 30 and cfg["aug_drop_p"] == 0.05 and cfg["aug_height"] == 0.2
    a = train.augmenter_from(cfg)
    assert a.config() == {"seed": 20240116, "flip_x_p": 0.5, "flip_y_p": 0.0, "yaw_deg": 30.0, "height": 0.2, "jitter_sigma": 0.01,
                          "drop_p": 0.05}
    for bad in ("aug_flip_x_p=1.5", "aug_drop_p=-0.1", "aug_height=-1", "aug_jitter_sigma=nan", "aug_yaw_deg=inf", "aug_height=abc"):
        with pytest.raises(SystemExit):
            train.parse_overrides(["augment=true", bad])
    with pytest.raises(SystemExit):
        train.parse_overrides(["augment=maybe"])


def test_augmenter_rejects_bad_arguments():
    from deflow_amd.augment import Augmenter
    Augmenter(0, 0.0, 1.0, 180.0, 0.0, 0.0, 1.0)
    for kw in ({"flip_x_p": 1.01}, {"flip_y_p": -0.5}, {"drop_p": float("nan")}, {"yaw_deg": -1.0}, {"height": float("inf")},
               {"jitter_sigma": float("nan")}, {"jitter_sigma": -0.01}):
        with pytest.raises(ValueError):
            Augmenter(0, **kw)
    with pytest.raises(KeyError):
        Augmenter.sample_ids_of({"pc0": torch.zeros(1, 1, 3)})
    ids = Augmenter.sample_ids_of({"pc0": torch.zeros(2, 1, 3), "timestamp": [315969904359876000, -3]})
    assert ids.dtype == torch.int64 and ids.tolist() == [315969904359876000, -3]


def test_checkpoint_config_with_the_keys_loads(tmp_path):
    """what save_checkpoint writes for an augmented run reads back through ckpt.py's reader, and eval's resolve_config keeps the keys"""
    from deflow_amd import train
    from deflow_amd.ckpt import flatten, load_checkpoint, plain
    from deflow_amd.eval import resolve_config
    cfg = train.parse_overrides(["augment=true", "aug_yaw_deg=15.5", "aug_drop_p=0.1"])
    saved = {k: v for k, v in cfg.items() if not k.startswith("_")}
    path = str(tmp_path / "a.ckpt")
    torch.save({"state_dict": {}, "hyper_parameters": {"cfg": saved}, "epoch": 0, "global_step": 1}, path)
    back = flatten(plain(load_checkpoint(path)["hyper_parameters"])["cfg"])
    assert back["augment"] is True and back["aug_yaw_deg"] == 15.5 and back["aug_drop_p"] == 0.1 and back["aug_height"] == 0.2
    res = resolve_config(path, {})
    assert res["augment"] is True and res["aug_yaw_deg"] == 15.5 and res["aug_flip_x_p"] == 0.5


def test_c_entry_points_reject_bad_arguments_without_launching():
    """validation precedes any launch, so it runs without a GPU: DF_E_ARG = -3, DF_E_SHAPE = -1"""
    import ctypes as C
    from deflow_amd import build
    from deflow_amd._lib import load
    build.build()
    lib = load()
    P, F = C.c_void_p, C.c_float
    a, b = 0x1000, 0x2000

    def aug(pc0=a, pc1=a, flow=0, ids=a, B=2, N0=8, N1=8, p=(0.5, 0.5, 0.1, 0.2, 0.01, 0.0), T=0, T_out=0, o0=b, o1=b, oflow=0):
        return lib.df_augment(P(pc0), P(pc1), P(flow), P(ids), B, N0, N1, 1, 0, *(F(v) for v in p), P(T), P(0), P(0), P(o0), P(o1), P(oflow),
                              P(T_out), P(0), P(0), P(0))

    assert aug(pc0=0) == -3 and aug(ids=0) == -3 and aug(o1=0) == -3
    assert aug(flow=a) == -3 and aug(oflow=b) == -3 and aug(T=a) == -3                 # an optional buffer without its partner
    assert aug(o0=a) == -3                                                              # in place
    assert aug(B=0) == -1 and aug(N0=0) == -1 and aug(N1=-1) == -1 and aug(B=65536) == -1 and aug(B=3, N0=2 ** 30) == -1
    for bad in ((1.5, 0.5, 0, 0, 0, 0), (0.5, -0.1, 0, 0, 0, 0), (0.5, 0.5, -1, 0, 0, 0), (0.5, 0.5, 0, float("inf"), 0, 0),
                (0.5, 0.5, 0, 0, float("nan"), 0), (0.5, 0.5, 0, 0, 0, 2.0)):
        assert aug(p=bad) == -3, bad
        assert lib.df_augment_params(P(a), 2, 1, 0, *(F(v) for v in bad), P(b), P(0)) == -3
    assert lib.df_augment_params(P(0), 2, 1, 0, *(F(0) for _ in range(6)), P(b), P(0)) == -3
    assert lib.df_augment_params(P(a), 0, 1, 0, *(F(0) for _ in range(6)), P(b), P(0)) == -1
