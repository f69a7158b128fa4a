"""CPU: the seflowLoss plumbing -- command line, Trainer construction, the new C-ABI entries' argument checks, losses.seflow_loss against
the naive float64 restatement (tests/helpers/seflow_ref.py) with a brute-force search injected, the synthetic cluster labels and the
collate of scene-file labels."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from seflow_ref import brute_nn_fn, seflow_ref  # noqa: E402


def test_command_line_accepts_seflow_loss():
    from deflow_amd.train import parse_overrides
    assert parse_overrides(["loss_fn=seflowLoss"])["loss_fn"] == "seflowLoss"
    with pytest.raises(SystemExit):
        parse_overrides(["loss_fn=chamferLoss"])


def test_trainer_constructs_with_seflow_loss():
    import deflow_amd
    from deflow_amd.optim import Trainer
    m = deflow_amd.DeFlow(voxel_size=[0.2, 0.2, 6], point_cloud_range=[-6.4, -6.4, -3, 6.4, 6.4, 3], grid_feature_size=[64, 64], num_iters=2)
    t = Trainer(m, loss_fn="seflowLoss", loss_args=dict(min_dynamic=8, weights=(1, 1, 1, 0.5), truncate_dist=2.0))
    assert t.loss_fn == "seflowLoss" and t.last_loss_terms is None and t.loss_args["min_dynamic"] == 8
    with pytest.raises(ValueError):
        Trainer(m, loss_fn="seflowLoss", loss_args=dict(min_dynamics=8))
    with pytest.raises(ValueError):
        Trainer(m, loss_fn="deflowLoss", loss_args=dict(min_dynamic=8))


def test_new_entries_reject_bad_arguments_without_launching():
    """NULL buffers, B <= 0, a missing counts pointer, sizes past the 32-bit key range: negative DF_E_* codes, no launch (no GPU here)"""
    from deflow_amd import build
    from deflow_amd._lib import load
    build.build()
    lib = load()
    P, F = C.c_void_p, C.c_float
    ok = P(0x1000)
    inf = F(math.inf)
    # df_nn_grid_build(ref, rcount, rlabel, B, Nr, minx, miny, cell, G, cell_rng, sorted, ws, stream)
    grid = lambda ref=ok, cnt=ok, B=2, Nr=100, cell=0.5, G=16, rng=ok, srt=ok, ws=ok: lib.df_nn_grid_build(
        ref, cnt, P(0), B, Nr, F(-4.0), F(-4.0), F(cell), G, rng, srt, ws, P(0))
    assert grid(ref=P(0)) < 0 and grid(cnt=P(0)) < 0 and grid(rng=P(0)) < 0 and grid(srt=P(0)) < 0 and grid(ws=P(0)) < 0
    assert grid(B=0) < 0 and grid(B=-1) < 0 and grid(Nr=0) < 0 and grid(G=0) < 0 and grid(G=5000) < 0
    assert grid(cell=0.0) < 0 and grid(cell=float("nan")) < 0
    assert grid(B=40000, Nr=80000) < 0 and grid(B=64, G=4096) < 0            # B * Nr, B * G * G past 2^30
    assert grid(srt=P(0x1004)) < 0                                            # unaligned rows
    # df_chamfer_nn(query, qcount, qlabel, B, Nq, cell_rng, sorted, minx, miny, cell, G, max_dist2, d2, idx, far_count, stream)
    nn = lambda q=ok, cnt=ok, B=2, Nq=100, rng=ok, srt=ok, G=16, md=inf, d2=ok, idx=ok: lib.df_chamfer_nn(
        q, cnt, P(0), B, Nq, rng, srt, F(-4.0), F(-4.0), F(0.5), G, md, d2, idx, P(0), P(0))
    assert nn(q=P(0)) < 0 and nn(cnt=P(0)) < 0 and nn(rng=P(0)) < 0 and nn(srt=P(0)) < 0 and nn(d2=P(0)) < 0 and nn(idx=P(0)) < 0
    assert nn(B=0) < 0 and nn(Nq=0) < 0 and nn(G=-3) < 0 and nn(md=F(-1.0)) < 0 and nn(md=F(float("nan"))) < 0
    assert nn(B=40000, Nq=80000) < 0
    # df_chamfer_bwd(query, ref, idx, g, B, Nq, Nr, dquery, dref, ws, stream)
    bwd = lambda q=ok, r=ok, idx=ok, g=ok, B=2, Nq=100, Nr=100, dq=ok, dr=ok, ws=ok: lib.df_chamfer_bwd(q, r, idx, g, B, Nq, Nr, dq, dr, ws, P(0))
    assert bwd(q=P(0)) < 0 and bwd(r=P(0)) < 0 and bwd(idx=P(0)) < 0 and bwd(g=P(0)) < 0
    assert bwd(dq=P(0), dr=P(0)) < 0 and bwd(ws=P(0)) < 0                    # nothing to write; the scatter needs its workspace
    assert bwd(B=0) < 0 and bwd(Nq=0) < 0 and bwd(Nr=-1) < 0 and bwd(B=40000, Nr=80000) < 0
    lib.df_nn_grid_ws_bytes.restype = lib.df_chamfer_bwd_ws_bytes.restype = C.c_int64
    assert lib.df_nn_grid_ws_bytes(2, 100, 16) > 0 and lib.df_nn_grid_ws_bytes(0, 100, 16) == 0
    assert lib.df_chamfer_bwd_ws_bytes(2, 100, 50) > 0 and lib.df_chamfer_bwd_ws_bytes(2, 0, 50) == 0


def test_chamfer_api_has_no_cpu_fallback():
    from deflow_amd.chamfer import ChamferDis, chamfer_nn
    a = torch.zeros(1, 4, 3)
    n = torch.full((1,), 4, dtype=torch.int32)
    with pytest.raises(TypeError, match="CUDA"):
        chamfer_nn(a, n, a, n)
    with pytest.raises(TypeError, match="CUDA"):
        ChamferDis.apply(a[0], a[0])


# ---- losses.seflow_loss against the helper, float64 on both sides ------------------------------------------------------------------------
def make_case(kind: str):
    """pc0, pc1, flow [B,N,3] float64, counts, labels.  kinds: 'dynamic' every sample has > 256 dynamic rows in both clouds; 'below' one
    sample below the threshold; 'fallback' every dynamic cluster's neighbours are static (term 3's fallback branch); 'empty' one sample
    with zero valid points"""
    from deflow_amd.synth import synth_batch, synth_cluster_labels
    b = synth_batch(2, 4000, seed=60, grid_hw=(64, 64))
    l0, l1 = synth_cluster_labels(b)
    ok = torch.isfinite(b["pc0"]).all(-1) & torch.isfinite(b["pc1"]).all(-1)
    n = int(ok.sum(1).min())
    pc0, pc1 = b["pc0"][:, :n].double(), b["pc1"][:, :n].double()
    pc0 = pc0 @ b["ego_motion"].double()[:, :3, :3].transpose(1, 2) + b["ego_motion"].double()[:, None, :3, 3]   # ego-compensated
    l0, l1 = l0[:, :n].clone(), l1[:, :n].clone()
    c0, c1 = torch.tensor([n, n - 150], dtype=torch.int32), torch.tensor([n - 70, n], dtype=torch.int32)
    g = torch.Generator().manual_seed(7)
    flow = (torch.randn(2, n, 3, generator=g) * 0.2).double()
    flow[0, 5] = 0.0                                    # |v| at v = 0: a zero gradient, not NaN
    if kind == "below":
        l0[1, 200:] = 0                                 # sample 1: fewer than 256 dynamic rows in pc0
    elif kind == "fallback":
        # pc1's dynamic rows moved far away from every pc0 row: each dynamic pc0 row's neighbour is a static pc1 row
        far = l1 > 0
        pc1 = torch.where(far[..., None], pc1 + torch.tensor([0.0, 0.0, 40.0], dtype=torch.float64), pc1)
    elif kind == "empty":
        c0[1] = 0
        c1[1] = 0
    return pc0, pc1, flow, c0, c1, l0, l1


@pytest.mark.parametrize("kind", ["dynamic", "below", "fallback", "empty"])
def test_seflow_loss_matches_the_helper(kind):
    from deflow_amd.losses import seflow_loss
    pc0, pc1, flow, c0, c1, l0, l1 = make_case(kind)
    f1 = flow.clone().requires_grad_(True)
    stats = {}
    loss, terms = seflow_loss(pc0, pc1, f1, c0, c1, l0, l1, nn_fn=brute_nn_fn, stats=stats)
    g1, = torch.autograd.grad(loss, f1)
    f2 = flow.clone().requires_grad_(True)
    want, wterms = seflow_ref(pc0, pc1, f2, c0, c1, l0, l1)
    g2, = torch.autograd.grad(want, f2)
    print(kind, float(loss), terms.tolist())
    assert terms.shape == (2, 4) and torch.isfinite(g1).all()
    assert abs(float(loss) - float(want)) <= 1e-10 * abs(float(want))
    assert float((terms - wterms).abs().max()) <= 1e-10 * float(wterms.abs().max())
    assert float((g1 - g2).abs().max()) <= 1e-10 * float(g2.abs().max())
    assert int(stats["label_overflow"]) == 0
    dyn = [(int((l0[b, : int(c0[b])] > 0).sum()), int((l1[b, : int(c1[b])] > 0).sum())) for b in range(2)]
    if kind == "dynamic":
        assert all(min(d) > 256 for d in dyn) and bool((terms > 0).all())
    if kind == "below":
        assert dyn[1][0] <= 256 and float(terms[1, 1]) == 0.0 and float(terms[1, 3]) == 0.0 and float(terms[0, 3]) > 0
    if kind == "fallback":
        # the fallback value: the truncated chamfer distance of the RAW clouds, a constant (no gradient from term 3)
        assert all(min(d) > 256 for d in dyn) and bool((terms[:, 3] > 0).all())
        f3 = flow.clone().requires_grad_(True)
        only3 = seflow_loss(pc0, pc1, f3, c0, c1, l0, l1, weights=(0, 0, 0, 1), nn_fn=brute_nn_fn)[0]
        assert float(torch.autograd.grad(only3, f3, allow_unused=True)[0].abs().max()) == 0.0
    if kind == "empty":
        assert bool((terms[1] == 0).all()) and bool((g1[1] == 0).all())


def test_seflow_loss_weights_threshold_and_label_overflow():
    from deflow_amd.losses import seflow_loss
    pc0, pc1, flow, c0, c1, l0, l1 = make_case("dynamic")
    _, terms = seflow_loss(pc0, pc1, flow, c0, c1, l0, l1, nn_fn=brute_nn_fn)
    loss, _ = seflow_loss(pc0, pc1, flow, c0, c1, l0, l1, weights=(1.0, 0.5, 2.0, 0.25), nn_fn=brute_nn_fn)
    want = (terms * torch.tensor([1.0, 0.5, 2.0, 0.25], dtype=torch.float64)).sum()
    assert abs(float(loss) - float(want)) <= 1e-12 * float(want)
    _, hi = seflow_loss(pc0, pc1, flow, c0, c1, l0, l1, min_dynamic=10 ** 6, nn_fn=brute_nn_fn)
    assert bool((hi[:, 1] == 0).all()) and bool((hi[:, 3] == 0).all()) and torch.equal(hi[:, [0, 2]], terms[:, [0, 2]])
    # a table too small for the labels: the rows are counted, not silently dropped
    stats = {}
    cut = int(l0.max()) - 1
    seflow_loss(pc0, pc1, flow, c0, c1, l0, l1, nn_fn=brute_nn_fn, max_label=cut, stats=stats)
    valid = torch.arange(l0.shape[1])[None, :] < c0[:, None]
    assert int(stats["label_overflow"]) == int(((l0 > cut) & valid).sum()) > 0
    with pytest.raises(ValueError):
        seflow_loss(pc0, pc1, flow, c0, c1, l0, l1, weights=(1, 1, 1), nn_fn=brute_nn_fn)


# ---- labels ----------------------------------------------------------------------------------------------------------------------------
def test_synth_cluster_labels():
    from deflow_amd.synth import synth_batch, synth_cluster_labels, synth_max_label
    b = synth_batch(2, 6000, seed=123, grid_hw=(64, 64))
    l0, l1 = synth_cluster_labels(b)
    again = synth_cluster_labels(synth_batch(2, 6000, seed=123, grid_hw=(64, 64)))
    assert torch.equal(l0, again[0]) and torch.equal(l1, again[1]) and torch.equal(l0, l1)
    assert not torch.equal(l0, synth_cluster_labels(synth_batch(2, 6000, seed=124, grid_hw=(64, 64)))[0])
    assert l0.shape == (2, 6000) and not l0.dtype.is_floating_point and int(l0.min()) == 0 and int(l0.max()) <= synth_max_label()
    nan = ~torch.isfinite(b["pc0"]).all(-1)
    assert int(nan.sum()) > 0 and bool((l0[nan] == 0).all())
    # in range of the 64 x 64 grid the small GPU tests use (+-6.4 m, |z| < 3): > 256 dynamic rows per cloud
    for pc, lab in ((b["pc0"], l0), (b["pc1"], l1)):
        inr = (pc[..., :2].abs() < 6.4).all(-1) & (pc[..., 2].abs() < 3.0)
        per = ((lab > 0) & inr).sum(1)
        print("in-range rows", inr.sum(1).tolist(), "dynamic", per.tolist())
        assert int(per.min()) > 256
    # dynamic = the ground-truth flow minus the ego motion's share is longer than 5 cm
    T = b["ego_motion"]
    resid = b["flow"] - ((b["pc0"] @ T[:, :3, :3].transpose(1, 2) + T[:, None, :3, 3]) - b["pc0"])
    moving = torch.nan_to_num(resid.norm(dim=-1), nan=0.0) > 0.05
    assert torch.equal(l0 > 0, moving)
    assert len(torch.unique(l0[l0 > 0])) >= 2          # tiles: more than one cluster


def test_collate_labels():
    from deflow_amd.data import collate_fn_pad

    def item(n0, n1, labelled, seed):
        g = torch.Generator().manual_seed(seed)
        it = {"scene_id": "s", "timestamp": seed, "pc0": torch.randn(n0, 3, generator=g), "pc1": torch.randn(n1, 3, generator=g),
              "gm0": torch.rand(n0, generator=g) < 0.3, "gm1": torch.rand(n1, generator=g) < 0.3, "pose0": torch.eye(4), "pose1": torch.eye(4)}
        if labelled:
            it["label0"] = torch.randint(0, 9, (n0,), generator=g)
            it["label1"] = torch.randint(0, 12, (n1,), generator=g)
        return it

    items = [item(50, 60, True, 1), item(80, 40, True, 2)]
    res = collate_fn_pad(items)
    assert res["pc0_dynamic"].shape == res["pc0"].shape[:2] and res["pc1_dynamic"].shape == res["pc1"].shape[:2]
    assert not res["pc0_dynamic"].dtype.is_floating_point
    for b, it in enumerate(items):
        for key, lab, gm in (("pc0_dynamic", "label0", "gm0"), ("pc1_dynamic", "label1", "gm1")):
            kept = it[lab][~it[gm]]
            assert torch.equal(res[key][b, : kept.numel()], kept) and bool((res[key][b, kept.numel():] == 0).all())
    assert isinstance(res["max_label"], int)
    assert res["max_label"] == max(int(res["pc0_dynamic"].max()), int(res["pc1_dynamic"].max()))
    plain = collate_fn_pad([item(50, 60, False, 1), item(80, 40, False, 2)])
    assert "pc0_dynamic" not in plain and "pc1_dynamic" not in plain and "max_label" not in plain
    mixed = collate_fn_pad([item(50, 60, True, 1), item(80, 40, False, 2)])
    assert "pc0_dynamic" not in mixed
