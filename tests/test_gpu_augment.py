"""GPU: the training augmentation (csrc/augment.hip, deflow_amd/augment.py) against the numpy restatement in tests/helpers/augment_ref.py.

Bounds (u = 2^-24, one fp32 rounding; none of them is fitted to what the kernel gives):

* flips, height, dropout: no multiply-add pair is evaluated -- sx x is exact, z + dz is one rounding of the same two fp32 values on both
  sides -- so the device is compared BIT FOR BIT with the restatement evaluated operation by operation in fp32.
* yaw / jitter, per coordinate of a row, against the float64 restatement (which uses the double cos / sin and the exact product n sj):
  x' = fma(n, sj, fma(c, x1, -fl(s y1))).  fl(s y1) errs by <= u |y|; the inner FMA's rounding by <= u (|x| + |y|); c and s are fp32 roundings
  of the double values: <= u |x| + u |y|; the outer FMA's rounding <= u (|x| + |y| + 3.46 sigma); sj = fp32(sigma / 147.8) moves the jitter
  by <= u 3.46 sigma.  Sum <= u (3 |x| + 4 |y| + 2 * 3.46 sigma).  z' = fma(n, sj, fl(z + dz)): <= u (2 |z| + 2 |dz| + 2 * 3.46 sigma).  So
  every coordinate is within  4 u M,  M = |x| + |y| + |z| + |dz| + 3.46 sigma  of the row (second-order terms: the factor 1 + 2^-20).
  The flow gets the linear part only: 4 u (|fx| + |fy|).
* T', pose0', pose1', df_augment_params: composed in double and rounded once: |got - want| <= u |want| (1 + 1e-6) + 1e-13 max|inputs| (the
  second term: the double sums' own rounding, which matters only where an entry cancels to nothing).
* df_ego_transform on the augmented batch, pose_flow' against L pose_flow in float64: the augmented points carry <= 4 u M, which enters
  through T' - I only (< 1 in norm); T' is rounded to fp32: <= u S', S' = |x'| + |y'| + |z'| + |t'|; df_ego_transform rounds three products,
  three sums and one difference, each of magnitude <= S': <= 7 u S'.  A rotation grows |x| + |y| by at most sqrt 2, so S' <= sqrt 2 (M + |t|)
  and the sum is (4 + 8 sqrt 2) u (M + |t|) < 16 u (M + |t|)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import augment_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL = dict(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], grid_feature_size=[64, 64])
F = np.float32
U = 2.0 ** -24
B = 3
# a negative id, one above 2^32 (both counter words), a nanosecond timestamp; at (SEED, EPOCH) the first draws flip x and the second flip y
IDS = [-5, (1 << 32) + 2, 315969904359876000]
EPOCH = 3
SIZES = [(1000, 1000), (1003, 997), (257, 64), (3, 1)]  # aligned 16-byte path; scalar path; its tail; fewer rows than one lane's four
CONFIGS = {
    "flips": dict(flip_x_p=0.5, flip_y_p=0.5, yaw_deg=0.0, height=0.0, jitter_sigma=0.0, drop_p=0.0),
    "flips_height": dict(flip_x_p=0.5, flip_y_p=0.5, yaw_deg=0.0, height=0.3, jitter_sigma=0.0, drop_p=0.0),
    "drop": dict(flip_x_p=0.0, flip_y_p=0.0, yaw_deg=0.0, height=0.0, jitter_sigma=0.0, drop_p=0.3),
    "yaw": dict(flip_x_p=0.5, flip_y_p=0.5, yaw_deg=180.0, height=0.0, jitter_sigma=0.0, drop_p=0.0),
    "jitter": dict(flip_x_p=0.0, flip_y_p=0.0, yaw_deg=0.0, height=0.0, jitter_sigma=0.02, drop_p=0.0),
    "all": dict(flip_x_p=0.5, flip_y_p=0.5, yaw_deg=45.0, height=0.3, jitter_sigma=0.02, drop_p=0.1),
}
EXACT = ("flips", "flips_height", "drop")
SEED = 20240116


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda")


def _pose(rng, far):
    a = rng.uniform(-math.pi, math.pi) if far else rng.uniform(-0.04, 0.04)
    T = np.eye(4)
    T[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    T[:3, 3] = rng.uniform(-3000, 3000, 3) if far else rng.uniform(-1.5, 1.5, 3)      # city coordinates / one frame's motion
    return T.astype(F)


_DATA = {}


def data(N0, N1):
    """one batch of numpy inputs per size, made once and never written again"""
    key = (N0, N1)
    if key not in _DATA:
        rng = np.random.default_rng(N0 * 1009 + N1)
        d = {}
        for name, N in (("pc0", N0), ("pc1", N1)):
            pc = rng.uniform(-60, 60, (B, N, 3)).astype(F)            # +-60 m: some rows outside the +-51.2 m range
            if N >= 3:
                pc[:, N - max(N // 10, 1):] = np.nan                    # the NaN tail
                pc[:, N // 2] = np.nan                                  # NaN rows in the middle
                pc[0, N // 3, 1] = np.nan                               # ... and a row with one NaN coordinate
            pc[2] = np.nan                                              # one sample entirely NaN
            d[name] = pc
        d["flow"] = rng.standard_normal((B, N0, 3)).astype(F)
        d["flow"][np.isnan(d["pc0"]).any(-1)] = np.nan
        d["ego_motion"] = np.stack([_pose(rng, False) for _ in range(B)])
        d["pose0"] = np.stack([_pose(rng, True) for _ in range(B)])
        d["pose1"] = np.stack([_pose(rng, True) for _ in range(B)])
        for a in d.values():
            a.setflags(write=False)
        _DATA[key] = d
    return _DATA[key]


_REF = {}


def reference(N0, N1, name, dtype):
    key = (N0, N1, name, dtype)
    if key not in _REF:
        d = data(N0, N1)
        _REF[key] = AR.apply(AR.Config(SEED, **CONFIGS[name]), IDS, EPOCH, d["pc0"], d["pc1"], d["flow"], d["ego_motion"], d["pose0"],
                             d["pose1"], dtype=dtype)
    return _REF[key]


def to_dev(d, dev, keys=None):
    return {k: torch.from_numpy(np.array(v)).to(dev) for k, v in d.items() if keys is None or k in keys}


def augmenter(name, seed=SEED):
    from deflow_amd.augment import Augmenter
    return Augmenter(seed, **CONFIGS[name])


def bits_equal(got, want):
    """same NaN pattern and bit-identical values elsewhere (a NaN's sign and payload are not part of the definition)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn)) and bool(np.array_equal(got[~gn].view(np.int32), want[~wn].view(np.int32)))


def one_rounding(got, want, scale):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want) - (U * np.abs(want) * (1 + 1e-6) + 1e-13 * scale)
    return float(err.max())


def row_bound(pc, dzs, sigma):
    """4 u M per row, M = |x| + |y| + |z| + |dz| + 3.46 sigma: [B, N, 1]"""
    M = np.abs(pc.astype(np.float64)).sum(-1) + np.abs(dzs)[:, None] + 3.46 * sigma
    return (4 * U * (1 + 2.0 ** -20) * M)[..., None]


# ---- the device against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N0, N1", SIZES)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_clouds_flow_and_matrices_match_the_restatement(dev, name, N0, N1):
    d = data(N0, N1)
    out = augmenter(name)(to_dev(d, dev), torch.tensor(IDS, device=dev), EPOCH)
    got = {k: out[k].cpu().numpy() for k in ("pc0", "pc1", "flow", "ego_motion", "pose0", "pose1")}
    want = reference(N0, N1, name, np.float64)
    cfg = AR.Config(SEED, **CONFIGS[name])
    # dropped rows: the NaN pattern is exactly the restatement's (input NaN rows included), whatever the arithmetic
    for k in ("pc0", "pc1"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), k
    assert np.array_equal(np.isnan(got["flow"]), np.isnan(want["flow"]))
    if name in EXACT:
        w32 = reference(N0, N1, name, np.float32)
        for k in ("pc0", "pc1", "flow"):
            assert bits_equal(got[k], w32[k]), k
    else:
        dzs = np.array([AR.sample_draw(cfg, i, EPOCH)["dz"] for i in IDS])
        for k in ("pc0", "pc1"):
            with np.errstate(invalid="ignore"):
                over = np.abs(got[k].astype(np.float64) - want[k]) - row_bound(d[k], dzs, cfg.sigma)
            worst = np.nanmax(over) if np.isfinite(over).any() else -1.0
            print(f"[augment] {name} {k} N={got[k].shape[1]}: error - bound, worst {worst:.3e}")
            assert not (over > 0).any(), (k, worst)
        with np.errstate(invalid="ignore"):
            fb = 4 * U * (1 + 2.0 ** -20) * np.abs(d["flow"][..., :2].astype(np.float64)).sum(-1, keepdims=True)
            over = np.abs(got["flow"].astype(np.float64) - want["flow"]) - fb
        assert not (over > 0).any()
    if N0 > 3:      # something must have happened: flips / drops / jitter change the rows of the finite samples
        assert not bits_equal(got["pc0"], d["pc0"])
    for k, src in (("ego_motion", "T"), ("pose0", "pose0"), ("pose1", "pose1")):
        scale = max(float(np.abs(d[k]).max()), 1.0)
        over = one_rounding(got[k], want[src], scale)
        print(f"[augment] {name} {k}: error - one rounding, worst {over:.3e}")
        assert over <= 0, (k, over)


@pytest.mark.parametrize("name", ["flips_height", "all"])
def test_params_match_the_restatement(dev, name):
    a = augmenter(name)
    ids = list(range(-40, 40)) + IDS                    # 83 samples: more than one block of the params kernel
    got = a.params(torch.tensor(ids, device=dev), EPOCH).cpu().numpy()
    want = AR.params(AR.Config(SEED, **CONFIGS[name]), ids, EPOCH)
    assert got.shape == (len(ids), 8) and got.dtype == np.float32
    assert np.array_equal(got[:, :2], want[:, :2]) and np.array_equal(got[:, 6:], np.zeros((len(ids), 2)))
    assert np.array_equal(got[:, 4], want[:, 4].astype(F))                       # dz: the same fp32 product
    assert one_rounding(got[:, [2, 3, 5]], want[:, [2, 3, 5]], 1.0) <= 0        # c, s, theta: double values rounded once
    assert set(np.unique(got[:, 0])) == {-1.0, 1.0} and set(np.unique(got[:, 1])) == {-1.0, 1.0}
    assert np.array_equal(got[-3:], a.params(IDS, EPOCH).cpu().numpy())          # a plain list of ids


def test_absent_flow_and_poses(dev):
    """flow, ego_motion and the poses are optional, alone and together; without ego_motion T is inv(pose1) pose0 as the model forms it"""
    from deflow_amd.deflow import batch_transform
    N0, N1 = 257, 64
    d = data(N0, N1)
    a = augmenter("all")
    ids = torch.tensor(IDS, device=dev)
    full = a(to_dev(d, dev), ids, EPOCH)
    bare = a(to_dev(d, dev, ("pc0", "pc1")), ids, EPOCH)
    assert sorted(bare) == ["pc0", "pc1"]
    assert bits_equal(bare["pc0"].cpu().numpy(), full["pc0"].cpu().numpy()) and bits_equal(bare["pc1"].cpu().numpy(), full["pc1"].cpu().numpy())
    noflow = a(to_dev(d, dev, ("pc0", "pc1", "ego_motion")), ids, EPOCH)
    assert sorted(noflow) == ["ego_motion", "pc0", "pc1"] and torch.equal(noflow["ego_motion"], full["ego_motion"])
    # poses only, and poses that compose well (one frame apart): T = inv(pose1) pose0 in the model's own bits
    rng = np.random.default_rng(5)
    pose0 = d["pose0"]
    pose1 = np.stack([(pose0[b].astype(np.float64) @ np.linalg.inv(_pose(rng, False).astype(np.float64))).astype(F) for b in range(B)])
    pb = {**to_dev(d, dev, ("pc0", "pc1", "flow")), "pose0": torch.from_numpy(pose0.copy()).to(dev), "pose1": torch.from_numpy(pose1).to(dev)}
    T_in = batch_transform(pb, dev).cpu().numpy()
    out = a(pb, ids, EPOCH)
    assert "ego_motion" not in pb and sorted(out) == ["ego_motion", "flow", "pc0", "pc1", "pose0", "pose1"]
    want = AR.apply(AR.Config(SEED, **CONFIGS["all"]), IDS, EPOCH, d["pc0"], d["pc1"], None, T_in, pose0, pose1)
    assert one_rounding(out["ego_motion"].cpu().numpy(), want["T"], max(float(np.abs(T_in).max()), 1.0)) <= 0
    assert one_rounding(out["pose1"].cpu().numpy(), want["pose1"], float(np.abs(pose1).max())) <= 0
    assert bits_equal(out["flow"].cpu().numpy(), full["flow"].cpu().numpy())


def test_unaligned_buffers_take_the_scalar_path_with_the_same_bits(dev):
    """N % 4 == 0 but the buffers start 4 bytes past a 16-byte boundary: the 4-byte path, and the same values"""
    N0 = N1 = 1000
    d = data(N0, N1)
    a = augmenter("all")
    ids = torch.tensor(IDS, device=dev)
    want = a(to_dev(d, dev), ids, EPOCH)

    def shifted(x):
        buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=dev)
        v = buf[1:].view(x.shape)
        v.copy_(x)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    got = a({k: (shifted(v) if k in ("pc0", "pc1", "flow") else v) for k, v in to_dev(d, dev).items()}, ids, EPOCH)
    for k in ("pc0", "pc1", "flow"):
        assert bits_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), k


# ---- purity ---------------------------------------------------------------------------------------------------------------------------------
def test_rows_depend_on_seed_epoch_sample_and_row_only(dev):
    N0, N1 = 1003, 997
    d = data(N0, N1)
    a = augmenter("all")
    batch = to_dev(d, dev)
    before = {k: v.clone() for k, v in batch.items()}
    full = a(batch, torch.tensor(IDS, device=dev), EPOCH)
    for k, v in batch.items():                                    # the input batch: bit-unchanged, and none of its tensors handed back
        assert torch.equal(v.view(torch.int32), before[k].view(torch.int32)), k
        assert full[k].data_ptr() != v.data_ptr()
    keys = ("pc0", "pc1", "flow", "ego_motion", "pose0", "pose1")
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
    perm = [2, 0, 1]
    p = a({k: v[perm] for k, v in batch.items()}, torch.tensor([IDS[i] for i in perm], device=dev), EPOCH)
    for k in keys:
        assert same(p[k], full[k][perm]), k
    for lo, hi in ((0, 1), (1, 3)):                               # B = 1, and the rest in a second call
        part = a({k: v[lo:hi] for k, v in batch.items()}, IDS[lo:hi], EPOCH)
        for k in keys:
            assert same(part[k], full[k][lo:hi]), k
    again = a(batch, torch.tensor(IDS, device=dev), EPOCH)
    assert all(same(again[k], full[k]) for k in keys)
    other_epoch = a(batch, torch.tensor(IDS, device=dev), EPOCH + 1)
    other_seed = augmenter("all", seed=SEED + 1)(batch, torch.tensor(IDS, device=dev), EPOCH)
    other_ids = a(batch, torch.tensor([i + 1 for i in IDS], device=dev), EPOCH)
    for o in (other_epoch, other_seed, other_ids):
        assert not same(o["pc0"][:2], full["pc0"][:2]) and not same(o["pc1"][:2], full["pc1"][:2])
        assert not same(o["ego_motion"], full["ego_motion"])


def test_aligned_keys_pass_through_by_reference(dev):
    d = data(257, 64)
    batch = to_dev(d, dev)
    extra = {"flow_is_valid": torch.ones(B, 257, dtype=torch.bool, device=dev), "flow_category_indices": torch.zeros(B, 257, dtype=torch.uint8, device=dev),
             "pc0_dynamic": torch.zeros(B, 257, dtype=torch.int64, device=dev), "pc1_dynamic": torch.zeros(B, 64, dtype=torch.int64, device=dev),
             "pc0_dufo": torch.zeros(B, 257, dtype=torch.int64, device=dev), "pc1_dufo": torch.zeros(B, 64, dtype=torch.int64, device=dev),
             "eval_mask": torch.ones(B, 257, dtype=torch.bool, device=dev), "timestamp": list(IDS), "scene_id": ["a", "b", "c"]}
    batch.update(extra)
    from deflow_amd.augment import Augmenter
    ids = Augmenter.sample_ids_of(batch)
    assert ids.is_cuda and ids.tolist() == IDS
    out = augmenter("all")(batch, ids, EPOCH)
    assert sorted(out) == sorted(batch)
    for k, v in extra.items():
        assert out[k] is v, k


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(dev):
    d = data(257, 64)
    batch = to_dev(d, dev)
    a = augmenter("all")
    ids = torch.tensor(IDS, device=dev)
    with pytest.raises(TypeError):
        a({**batch, "pc0": batch["pc0"].cpu()}, ids, EPOCH)
    with pytest.raises(TypeError):
        a({k: v for k, v in batch.items() if k != "pc1"}, ids, EPOCH)
    with pytest.raises(ValueError):
        a({**batch, "pc1": batch["pc1"][:2]}, ids, EPOCH)
    with pytest.raises(ValueError):
        a({**batch, "flow": batch["flow"][:, :100]}, ids, EPOCH)
    with pytest.raises(ValueError):
        a({**batch, "pc0": batch["pc0"][..., :2]}, ids, EPOCH)
    with pytest.raises(ValueError):
        a({**batch, "ego_motion": batch["ego_motion"][:, :3]}, ids, EPOCH)
    with pytest.raises(ValueError):
        a(batch, ids[:2], EPOCH)
    with pytest.raises(ValueError):
        a(batch, ids.int(), EPOCH)
    from deflow_amd._lib import call, ptr, stream
    o = torch.empty_like(batch["pc0"])
    with pytest.raises(RuntimeError, match="DF_E_ARG"):       # in place: refused before any launch
        call("df_augment", ptr(batch["pc0"]), ptr(batch["pc1"]), None, ptr(ids), B, 257, 64, 1, 0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0, None, None, None,
             ptr(batch["pc0"]), ptr(torch.empty_like(batch["pc1"])), None, None, None, None, stream())
    with pytest.raises(RuntimeError, match="DF_E_ARG"):
        call("df_augment", ptr(batch["pc0"]), ptr(batch["pc1"]), None, ptr(ids), B, 257, 64, 1, 0, 0.5, 1.5, 0.0, 0.0, 0.0, 0.0, None, None, None,
             ptr(o), ptr(torch.empty_like(batch["pc1"])), None, None, None, None, stream())
    with pytest.raises(RuntimeError, match="DF_E_SHAPE"):
        call("df_augment_params", ptr(ids), 0, 1, 0, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0, ptr(o), stream())


# ---- dropout rests on the engine taking NaN rows anywhere ---------------------------------------------------------------------------------
def small_model(dev, seed=3):
    import deflow_amd
    torch.manual_seed(seed)
    return deflow_amd.DeFlow(**SMALL, num_iters=2).to(dev)


def test_engine_takes_dropped_rows_in_place(dev):
    """a batch with rows dropped in place against the same batch with those rows physically removed on the host (the survivors in order,
    NaN padding behind them): the eval forward's flow of the surviving rows is expected bit-equal -- a dropped row is skipped like padding
    and the pillar sort is stable, so every survivor meets the same neighbours in the same order."""
    from deflow_amd.augment import Augmenter
    from deflow_amd.synth import synth_batch
    Bn, N = 2, 2000
    sb = synth_batch(Bn, N, seed=31, grid_hw=(64, 64), device=dev)
    a = Augmenter(SEED, flip_x_p=0.0, flip_y_p=0.0, yaw_deg=0.0, height=0.0, jitter_sigma=0.0, drop_p=0.3)
    dropped = a(sb, [31, 32], 0)
    assert torch.equal(dropped["ego_motion"], sb["ego_motion"])
    removed = {k: v for k, v in dropped.items()}
    keep_rows = {}
    for key in ("pc0", "pc1"):
        pc = dropped[key].cpu()
        out = torch.full_like(pc, float("nan"))
        for b in range(Bn):
            keep = torch.isfinite(pc[b]).all(-1)
            rows = torch.nonzero(keep)[:, 0]
            assert 0.55 * N < len(rows) < 0.8 * N                 # ~30 % dropped (and the 2 % NaN tail)
            assert bool((~keep[: int(0.9 * N)]).any())            # ... in the middle of the cloud, not only at its end
            out[b, : len(rows)] = pc[b, rows]
            keep_rows[key, b] = rows
        removed[key] = out.to(dev)
    m = small_model(dev).eval()
    with torch.no_grad():
        r_drop = m(dropped)
        flow_d = [f.clone() for f in r_drop["flow"]]
        idx_d = [i.clone() for i in r_drop["pc0_valid_point_idxes"]]
        r_rem = m(removed)
    for b in range(Bn):
        rows = keep_rows["pc0", b].to(dev)
        assert torch.equal(idx_d[b], rows[r_rem["pc0_valid_point_idxes"][b]])          # the same survivors, in the same order
        diff = float((flow_d[b] - r_rem["flow"][b]).abs().max())
        print(f"[augment] dropped in place vs removed, sample {b}: {len(idx_d[b])} rows, max |flow difference| {diff:.3e}")
        assert torch.isfinite(flow_d[b]).all() and len(idx_d[b]) > 500
        assert torch.equal(flow_d[b], r_rem["flow"][b])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_fn", ["deflowLoss", "seflowLoss"])
def test_trainer_step_on_an_augmented_batch(dev, loss_fn):
    from deflow_amd.augment import Augmenter
    from deflow_amd.optim import Trainer
    from deflow_amd.synth import synth_batch, synth_cluster_labels
    sb = synth_batch(2, 2000, seed=77, grid_hw=(64, 64), device=dev)
    if loss_fn == "seflowLoss":
        sb["pc0_dynamic"], sb["pc1_dynamic"] = synth_cluster_labels(sb)
    a = Augmenter(SEED, flip_x_p=0.5, flip_y_p=0.5, yaw_deg=45.0, height=0.2, jitter_sigma=0.01, drop_p=0.1)
    ab = a(sb, torch.arange(2, device=dev) + 77, 1)
    m = small_model(dev).train()
    t = Trainer(m, lr=1e-3, loss_fn=loss_fn)
    before = t.flat.param.clone()
    loss = t.step(ab)
    assert math.isfinite(float(loss)) and float(loss) > 0
    assert bool(torch.isfinite(t.flat.grad).all()) and float(t.flat.grad.abs().max()) > 0
    assert bool(torch.isfinite(t.flat.param).all()) and not torch.equal(before, t.flat.param)


@pytest.mark.parametrize("sigma", [0.0, 0.01])
def test_pose_flow_of_the_augmented_batch_is_the_rotated_pose_flow(dev, sigma):
    """df_ego_transform(pc0', T') - pc0' = L (T q - q), q = A^-1 pc0' the point the augmented row is the image of: what keeps
    flow' - pose_flow' = L (flow - pose_flow) for df_gather_gt.  Without jitter q is the input row itself and the right-hand side is
    L pose_flow of the input batch, literally; both are asserted then.  With jitter j the augmented row is the image of p + L^-1 j, a
    slightly different point with a slightly different pose flow -- L pose_flow(p) + (R' - I) j, up to |ego yaw per frame| 3.46 sigma away
    from L pose_flow(p), far above rounding -- so the comparison is made at q (from the float64 restatement's augmented rows).  The labels
    do not follow the jitter: it is noise on the points."""
    from deflow_amd._lib import call, ptr, stream
    from deflow_amd.augment import Augmenter
    from deflow_amd.synth import synth_batch
    sb = synth_batch(2, 2000, seed=77, grid_hw=(64, 64), device=dev)
    kw = dict(flip_x_p=0.5, flip_y_p=0.5, yaw_deg=45.0, height=0.2, jitter_sigma=sigma, drop_p=0.1)
    ids = [77, 78]
    ab = Augmenter(SEED, **kw)(sb, ids, 1)
    pc, T = ab["pc0"].contiguous(), ab["ego_motion"].contiguous()
    moved, pose_flow = torch.empty_like(pc), torch.empty_like(pc)
    call("df_ego_transform", ptr(pc), ptr(T), 2, 2000, ptr(moved), ptr(pose_flow), stream())
    got = pose_flow.cpu().numpy().astype(np.float64)
    cfg = AR.Config(SEED, **kw)
    p0, T0 = sb["pc0"].cpu().numpy(), sb["ego_motion"].cpu().numpy().astype(np.float64)
    checked = 0
    for b in range(2):
        d = AR.sample_draw(cfg, ids[b], 1)
        A, Ai = AR.matrices(d)
        L = A[:3, :3]
        pose_flow_of = lambda q: q @ T0[b][:3, :3].T + T0[b][:3, 3] - q
        with np.errstate(invalid="ignore"):
            aug64, _ = AR.cloud(cfg, d, ids[b], 1, p0[b], 1)
            q = aug64 @ Ai[:3, :3].T + Ai[:3, 3]
            want = pose_flow_of(q) @ L.T
            M = np.abs(p0[b].astype(np.float64)).sum(-1) + abs(d["dz"]) + 3.46 * cfg.sigma + np.abs(T0[b][:3, 3]).sum()
            over = np.abs(got[b] - want) - (16 * U * M)[:, None]
            literal = np.abs(got[b] - pose_flow_of(p0[b].astype(np.float64)) @ L.T) - (16 * U * M)[:, None]
        live = ~np.isnan(got[b]).any(-1)
        assert 1500 < live.sum() < 1900 and np.isfinite(want[live]).all()
        print(f"[augment] pose flow sigma {sigma} sample {b}: error - bound, worst {over[live].max():.3e}; against L pose_flow(p) {literal[live].max():.3e}")
        assert (over[live] <= 0).all()
        if sigma == 0.0:
            assert (literal[live] <= 0).all()
        checked += int(live.sum())
    assert checked > 3000
