"""No GPU: what the per-pair optimisers share (deflow_amd/pairopt.py) -- the snapshot / freeze / early-stop rule of
the loop on host tensors against the pure-Python rule the GPU tests use (tests/helpers/nsfp_ref.replay), the per-sample reductions
against float64, and the refusals of the shared argument checks under each optimiser's name."""
import numpy as np
import pytest
import torch

from helpers import nsfp_ref as nr

ITERS, PATIENCE, MIN_DELTA = 60, 5, 3e-3
STATE = ("best", "best_flow", "stalled", "frozen", "last", "history", "t_dev")


def _histories():
    """[60, 3] fp32: sample 0 decays with noise and stalls late, sample 1 falls for ten iterations and then jitters about a plateau,
    sample 2 falls by ten times min_delta per iteration and never freezes"""
    rng = np.random.default_rng(5)
    t = np.arange(ITERS)
    a = 1 / (1 + 0.2 * t) + 0.02 * rng.standard_normal(ITERS)
    b = np.where(t < 10, 1 - 0.05 * t, 0.5 + 0.01 * rng.standard_normal(ITERS))
    return torch.from_numpy(np.stack([a, b, 2 - 0.03 * t], axis=1).astype(np.float32))


def _run(losses, check_every):
    """the loop fed these losses; F of iteration t is the constant t, so best_flow names the snapshot's iteration"""
    from deflow_amd import pairopt
    B = losses.shape[1]
    p = dict(iters=ITERS, patience=PATIENCE, min_delta=MIN_DELTA, check_every=check_every, graph=False, lr=1e-3)
    loop = pairopt.Loop(torch.zeros(4), torch.zeros(B, 2, 3), p)

    def iteration():
        t = int(loop.t_dev)
        loop.snapshot(losses[t], torch.full((B, 2, 3), float(t)))

    return loop, loop.run(iteration)


def test_snapshot_freeze_and_history_are_the_replayed_rule():
    losses = _histories()
    loop, ran = _run(losses, 0)
    assert ran == ITERS == loop.ran and int(loop.t_dev) == ITERS
    flow, info = loop.result(torch.tensor([[True, False]] * 3), extra=7)
    hist = info["loss_history"].numpy()
    assert set(info) == {"best_loss", "loss_history", "stalled", "frozen", "grads", "iters_run", "extra"} and info["iters_run"] == ITERS
    assert info["grads"] is loop.grads and info["grads"].shape == (4,) and hist.shape == (ITERS, 3)
    assert loop.best_flow[:, 0, 0].tolist() == [47.0, 15.0, 59.0], "the best iterates"
    assert info["stalled"].tolist() == [5, 5, 0] and info["frozen"].tolist() == [True, True, False]
    assert torch.equal(flow[:, 0], loop.best_flow[:, 0]) and not flow[:, 1].any(), "the flow is the best iterate's, 0 outside m0"
    for b in range(3):
        best, stalled, frozen, arg = nr.replay(hist[:, b], PATIENCE, MIN_DELTA)
        assert np.float32(info["best_loss"][b].item()) == best and int(info["stalled"][b]) == stalled and bool(info["frozen"][b]) == frozen
        assert float(loop.best_flow[b, 0, 0]) == arg
        if frozen:                                        # entries after a freeze repeat the last value; before it they are the losses fed
            t = arg + PATIENCE
            assert (hist[t:, b] == hist[t, b]).all() and np.array_equal(hist[:t + 1, b], losses[:t + 1, b].numpy())
        else:
            assert np.array_equal(hist[:, b], losses[:, b].numpy())


def test_early_stop_changes_no_state():
    losses = _histories()[:, :2]
    whole, ran = _run(losses, 0)
    assert ran == ITERS and bool(whole.frozen.all())
    early, ran = _run(losses, 7)
    assert ran == 56 == early.ran, "both samples are frozen from iteration 53 on: the read after 56 iterations stops the loop"
    for k in STATE[:-1]:
        assert torch.equal(getattr(early, k), getattr(whole, k)), k
    assert int(early.t_dev) == 56 and _run(losses, 59)[1] == 59 and _run(losses, 60)[1] == 60 and _run(losses[:, :1], 7)[1] == 56


def test_sample_sum_and_mean_and_weight():
    from deflow_amd import pairopt
    gen = torch.Generator().manual_seed(3)
    d = torch.rand(3, 1001, generator=gen) * 4
    d[0, ::3], d[2] = float("inf"), float("inf")                     # rows left out; a sample without any row
    mean, weight = pairopt.mean_and_weight(d)
    keep = torch.isfinite(d)
    n = keep.sum(1)
    want = torch.where(keep, d, torch.zeros(())).double().sum(1) / n.clamp_min(1)
    # the error of an fp32 sum of n terms in [0, 4) in any order is below n eps times the sum of the magnitudes; the division adds one rounding
    assert float((mean.double() - want).abs().max()) <= 1001 * 2.0 ** -24 * float(want.max()) and float(mean[2]) == 0.0 and float(mean[1]) > 1
    assert torch.equal(weight, keep.float() / n.clamp_min(1).float()[:, None]) and not weight[2].any()
    v = torch.randn(2, 37, 5, generator=gen)
    assert float((pairopt.sample_sum(v).double() - v.double().sum((1, 2))).abs().max()) <= 185 * 2.0 ** -24 * float(v.abs().sum((1, 2)).max())
    # a row's result does not depend on its batch: alone, and as the second of three rows of another padded width
    row = d[1]
    wide = torch.full((3, 1400), float("inf"))
    wide[0, :700], wide[1, :1001], wide[2, :1300] = d[0, :700], row, 1.5
    m1, w1 = pairopt.mean_and_weight(row[None])
    m3, w3 = pairopt.mean_and_weight(wide)
    assert torch.equal(m1[0], m3[1]) and torch.equal(m1[0], mean[1]) and torch.equal(w1[0], w3[1, :1001]) and not w3[1, 1001:].any()
    s1, s3 = pairopt.sample_sum(row[None]), pairopt.sample_sum(torch.stack([d[2].nan_to_num(posinf=0.0), row, d[1].flip(0)]))
    assert torch.equal(s1[0], s3[1])


class _OnDevice(torch.Tensor):
    """a host tensor that says it is on the GPU: the argument checks run before anything is launched"""
    is_cuda = property(lambda self: True)


@pytest.mark.parametrize("fn", ["nsfp_optimize", "fastnsf_optimize", "mbnsf_optimize", "floxels_optimize"])
def test_pair_clouds_refuses_by_argument_name(fn):
    from deflow_amd import pairopt
    x, c = torch.zeros(2, 4, 3), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TypeError, match=f"{fn}: pc0s must be a CUDA tensor"):
        pairopt.pair_clouds(fn, x, c, x, c)
    dev = lambda t: t.as_subclass(_OnDevice)
    xg, cg = dev(x), dev(c)
    assert xg.is_cuda and not x.is_cuda
    for args, exc, what in (((xg, cg, x, cg), TypeError, "pc1 must be a CUDA tensor"), ((xg, c, xg, cg), TypeError, "count0 must be a CUDA tensor"),
                            ((xg, cg, dev(x[:1]), cg), ValueError, r"pc1 must have the batch size \(2\)"),
                            ((xg, cg, xg, dev(c.long())), ValueError, "count1 must be torch.int32"),
                            ((xg, dev(c[:1]), xg, cg), ValueError, "count0 must be torch.int32 of shape"),
                            ((dev(x.double()), cg, xg, cg), ValueError, "pc0s must be torch.float32"),
                            ((xg, cg, dev(x[:, :, :2]), cg), ValueError, "pc1 must be torch.float32 of shape")):
        with pytest.raises(exc, match=f"{fn}: {what}"):
            pairopt.pair_clouds(fn, *args)
    # the four optimisers themselves report through it
    from deflow_amd import fastnsf, floxels, mbnsf, nsfp
    opt = {"nsfp_optimize": nsfp.nsfp_optimize, "fastnsf_optimize": fastnsf.fastnsf_optimize, "mbnsf_optimize": mbnsf.mbnsf_optimize,
           "floxels_optimize": floxels.floxels_optimize}[fn]
    with pytest.raises(ValueError, match=f"{fn}: count1 must be torch.int32"):
        opt(xg, cg, xg, dev(c.long()), grid_range=(-1, -1, -1, 1, 1, 1))
