"""GPU: the per-pair neural flow prior (csrc/mlp.hip, deflow_amd/nsfp.py) against tests/helpers/nsfp_ref.py.

Bound of every floating-point comparison: max(1e-4 of the compared tensor's largest magnitude, 4 x the fp32 helper's own difference
from the float64 helper on that case).  Conditions that make a case well-posed are asserted on the INPUT."""
import math

import numpy as np
import pytest
import torch

from helpers import nsfp_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 64            # nsfp.ROW_TILE (asserted below)
SPLIT = 1024      # nsfp.WGRAD_SPLIT_ROWS


def _bound(ref64, ref32):
    return max(1e-4 * float(ref64.abs().max()), 4 * float((ref32.double() - ref64).abs().max()))


def _close(got, ref64, ref32, what):
    err, tol = float((got.double().cpu() - ref64).abs().max()), _bound(ref64, ref32)
    print(f"{what}: err {err:.3e} bound {tol:.3e} (max |ref| {float(ref64.abs().max()):.3e})")
    assert err <= tol, (what, err, tol)


def _case(N, depth, seed):
    """B = 3 nets with different parameters, counts {N, N // 2, 0}, NaN rows behind the counts"""
    gen = torch.Generator().manual_seed(seed)
    counts = [N, N // 2, 0]
    x = (torch.rand(3, N, 3, generator=gen, dtype=torch.float64) * 2 - 1) * torch.tensor([30.0, 30.0, 2.0], dtype=torch.float64)
    x = x.float()
    dy = (torch.rand(3, N, 3, generator=gen, dtype=torch.float64) * 2 - 1).float()
    for b, c in enumerate(counts):
        x[b, c:] = float("nan")
        dy[b, c:] = float("nan")
    P = nr.num_params(depth)
    S = (P + 3) // 4 * 4
    params = torch.zeros(3, S, dtype=torch.float32)
    for b in range(3):
        params[b, :P] = nr.xavier_params(depth, gen, torch.float32, scale=1.5 if b else 1.0, bias=0.3)
    params[:, 0:384] *= 0.1                         # |W_in x| of the order of 1 at coordinates of tens of metres
    return x, dy, params, counts, P


# ---- 1. forward and backward against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [0, 1, 7])
@pytest.mark.parametrize("N", [1, T - 1, T, T + 1, 3 * T + 5, SPLIT + 37])
def test_mlp_forward_backward_against_float64(N, depth):
    """tile edges of the row tile (1, T - 1, T, T + 1, 3 T + 5: one weight-gradient split) and SPLIT + 37 (two splits, the last ragged)"""
    from deflow_amd import nsfp
    assert nsfp.ROW_TILE == T and nsfp.WGRAD_SPLIT_ROWS == SPLIT
    x, dy, params, counts, P = _case(N, depth, 1000 * depth + N)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    xg, pg, dyg = x.to(DEV), params.to(DEV), dy.to(DEV)
    y, acts = nsfp.mlp_forward(xg, cnt, pg, depth)
    dp, dx = nsfp.mlp_backward(xg, cnt, pg, depth, acts, dyg)
    torch.cuda.synchronize()
    y, acts, dp, dx = y.cpu(), acts.cpu(), dp.cpu(), dx.cpu()
    assert acts.shape == (3, depth + 1, N, 128) and dp.shape == (3, params.shape[1]) and dx.shape == x.shape
    for b, c in enumerate(counts):
        assert not y[b, c:].any() and not dx[b, c:].any(), "zeros behind the counts"
        assert not dp[b, P:].any()
        if c == 0:
            assert not dp[b].any()
            continue
        x64, x32 = x[b, :c].double(), x[b, :c]
        y64, z64, a64 = nr.mlp_forward(x64, params[b, :P].double(), depth)
        y32, _, a32 = nr.mlp_forward(x32, params[b, :P], depth)
        _close(y[b, :c], y64, y32, f"y[{b}]")
        masks = []
        for l in range(depth + 1):
            _close(acts[b, l, :c], a64[l], a32[l], f"a_{l}[{b}]")
            m = acts[b, l, :c] > 0
            sure = z64[l].abs() > _bound(a64[l], a32[l])
            assert torch.equal(m[sure], (z64[l] > 0)[sure]), f"ReLU masks of layer {l}"
            masks.append(m)
        g64, dx64 = nr.mlp_backward(x64, params[b, :P].double(), depth, dy[b, :c].double(), masks)
        g32, dx32 = nr.mlp_backward(x32, params[b, :P], depth, dy[b, :c], masks)
        _close(dx[b, :c], dx64, dx32, f"dx[{b}]")
        o = 0
        for l, (W, bias) in enumerate(nr.unpack(params[b, :P], depth)):
            for t in (W, bias):
                n = t.numel()
                _close(dp[b, o:o + n], g64[o:o + n], g32[o:o + n], f"dparams[{b}] layer {l} {'W' if t is W else 'b'}")
                o += n


# ---- 2. exact layout ------------------------------------------------------------------------------------------------------------------
def test_mlp_layout_is_exact_on_small_integers():
    """small-integer weights, biases, inputs and output gradients with asymmetric matrices: every product and partial sum is an integer
    below 2^24 (asserted on the inputs through absolute-value bounds), so fp32 is exact in any order and y and all gradients must EQUAL
    float64's.  A transposed or permuted fragment cannot pass."""
    from deflow_amd import nsfp
    depth, N, counts = 2, T + 6, [T + 6, 33]
    gen = torch.Generator().manual_seed(5)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).double()
    P = nr.num_params(depth)
    S = (P + 3) // 4 * 4
    params = torch.zeros(2, S, dtype=torch.float64)
    for b in range(2):
        layers = []
        for rows, cols in [(128, 3)] + [(128, 128)] * depth + [(3, 128)]:
            W = ri(-2, 2, rows, cols) * (torch.rand(rows, cols, generator=gen) < (1.0 if cols == 3 else 0.125))
            layers.append((W, ri(-3, 3, rows)))
        params[b, :P] = nr.pack(layers)
    x, dy = ri(-3, 3, 2, N, 3), ri(-2, 2, 2, N, 3)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    y, acts = nsfp.mlp_forward(x.float().to(DEV), cnt, params.float().to(DEV), depth)
    dp, dx = nsfp.mlp_backward(x.float().to(DEV), cnt, params.float().to(DEV), depth, acts, dy.float().to(DEV))
    torch.cuda.synchronize()
    for b, c in enumerate(counts):
        flat = params[b, :P]
        layers = nr.unpack(flat, depth)
        # the bound on every partial sum, any order: the same network with absolute values
        a, big = x[b, :c].abs(), 0.0
        for W, bias in layers:
            a = a @ W.abs().T + bias.abs()
            big = max(big, float(a.max()))
        y64, z64, a64 = nr.mlp_forward(x[b, :c], flat, depth)
        masks = [z > 0 for z in z64]
        g64, dx64 = nr.mlp_backward(x[b, :c], flat, depth, dy[b, :c], masks)
        d = dy[b, :c].abs()
        big = max(big, float((d.T @ a64[-1].abs()).max()))
        d = d @ layers[-1][0].abs()
        for l in range(depth, -1, -1):
            prev = a64[l - 1].abs() if l else x[b, :c].abs()
            big = max(big, float((d.T @ prev).max()), float(d.sum(0).max()))
            d = d @ layers[l][0].abs()
            big = max(big, float(d.max()))
        assert big < 2 ** 24, big
        assert torch.equal(y[b, :c].cpu().double(), y64)
        for l in range(depth + 1):
            assert torch.equal(acts[b, l, :c].cpu().double(), a64[l]), l
        assert torch.equal(dx[b, :c].cpu().double(), dx64)
        assert torch.equal(dp[b, :P].cpu().double(), g64)
        assert float(g64.abs().max()) > 100 and float(y64.abs().max()) > 100        # not a degenerate all-zero case


# ---- 3. contract ----------------------------------------------------------------------------------------------------------------------
def _dirty(value):
    """leave `value` in freed blocks of the caching allocator, so that an output element the kernels skip shows it"""
    junk = [torch.full((n,), value, dtype=torch.float32, device=DEV) for n in (1 << 22, 1 << 20, 1 << 18, 1 << 16, 4096, 512)]
    torch.cuda.synchronize()
    del junk


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_mlp_contract():
    from deflow_amd import nsfp
    depth, N = 3, SPLIT + T + 3
    x, dy, params, counts, P = _case(N, depth, 77)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    xg, pg, dyg = x.to(DEV), params.to(DEV), dy.to(DEV)
    outs = []
    for fill in (float("nan"), 1.0e30):
        _dirty(fill)
        y, acts = nsfp.mlp_forward(xg, cnt, pg, depth)
        dp, dx = nsfp.mlp_backward(xg, cnt, pg, depth, acts, dyg)
        torch.cuda.synchronize()
        outs.append((y.cpu(), dp.cpu(), dx.cpu()))
    for a, b in zip(*outs):
        assert torch.isfinite(a).all(), "every element written"
        assert torch.equal(_bits(a), _bits(b)), "two calls are bit-identical"
    # a sample alone equals the sample inside the batch, at equal padded N
    for b in range(3):
        y1, a1 = nsfp.mlp_forward(xg[b:b + 1].contiguous(), cnt[b:b + 1], pg[b:b + 1], depth)
        dp1, dx1 = nsfp.mlp_backward(xg[b:b + 1].contiguous(), cnt[b:b + 1], pg[b:b + 1], depth, a1, dyg[b:b + 1].contiguous())
        for got, want in zip((y1, dp1, dx1), outs[0]):
            assert torch.equal(_bits(got.cpu()), _bits(want[b:b + 1])), b
    # inference: no saved activations, the same y
    y2, none = nsfp.mlp_forward(xg, cnt, pg, depth, save=False)
    assert none is None and torch.equal(_bits(y2.cpu()), _bits(outs[0][0]))
    # the autograd function on top
    xr, pr = torch.nan_to_num(xg).requires_grad_(True), pg.clone().requires_grad_(True)
    yy = nsfp.FlowMLPFn.apply(xr, cnt, pr, depth)
    (yy * torch.nan_to_num(dyg)).sum().backward()
    assert torch.equal(_bits(pr.grad.cpu()), _bits(outs[0][1])) and torch.equal(_bits(xr.grad.cpu()), _bits(outs[0][2]))
    # bad arguments raise and name the argument
    with pytest.raises(TypeError, match="x"):
        nsfp.mlp_forward(x, cnt, pg, depth)
    with pytest.raises(ValueError, match="depth"):
        nsfp.mlp_forward(xg, cnt, pg, 16)
    with pytest.raises(ValueError, match="count"):
        nsfp.mlp_forward(xg, cnt.long(), pg, depth)
    with pytest.raises(ValueError, match="params"):
        nsfp.mlp_forward(xg, cnt, pg[:, :100], depth)
    with pytest.raises(ValueError, match="x"):
        nsfp.mlp_forward(xg[:, :, :2], cnt, pg, depth)
    with pytest.raises(ValueError, match="dy"):
        nsfp.mlp_backward(xg, cnt, pg, depth, acts, dyg[:, :5])
    with pytest.raises(ValueError, match="acts"):
        nsfp.mlp_backward(xg, cnt, pg, depth, acts[:, :2], dyg)
    from deflow_amd._lib import load
    lib = load()
    assert lib.df_mlp_ws_bytes(1, 0, 3) < 0 and lib.df_mlp_ws_bytes(1, 8, 16) < 0 and lib.df_mlp_ws_bytes(1, 8, -1) < 0
    assert lib.df_mlp_fwd(None, None, None, 0, 1, 8, 3, None, None, None) < 0
    assert lib.df_mlp_bwd(None, None, None, 0, None, None, 1, 8, 3, None, None, None, None) < 0


# ---- 4. one iteration of nsfp_optimize ------------------------------------------------------------------------------------------------
def _pad_pair(samples, pad0=5, pad1=9):
    """[(P0, P1)] -> pc0s, count0, pc1, count1 on the device, NaN rows behind the counts"""
    n0, n1 = max(len(s[0]) for s in samples) + pad0, max(len(s[1]) for s in samples) + pad1
    a = np.full((len(samples), n0, 3), np.nan, np.float32)
    b = np.full((len(samples), n1, 3), np.nan, np.float32)
    for i, (P0, P1) in enumerate(samples):
        a[i, :len(P0)], b[i, :len(P1)] = P0, P1
    c0 = torch.tensor([len(s[0]) for s in samples], dtype=torch.int32, device=DEV)
    c1 = torch.tensor([len(s[1]) for s in samples], dtype=torch.int32, device=DEV)
    return torch.from_numpy(a).to(DEV), c0, torch.from_numpy(b).to(DEV), c1


def test_one_iteration_against_float64():
    """iters = 1, B = 2 (210 + 150 rows), depth 2, a start whose ReLUs are decided (helpers.decided_params): the loss of the start and
    the parameters after the Adam step against the float64 helper fed the op's own neighbour rows.  Well-posed by the helper's report:
    no near-tie between neighbours, no d2 near the truncation, no pre-activation inside the forward bound -- asserted."""
    from deflow_amd import nsfp
    depth, trunc = 2, 4.0
    P, S = nsfp.num_params(depth), nsfp.param_stride(depth)
    gen = torch.Generator().manual_seed(42)
    init = torch.zeros(2, S)
    init[0, :P], init[1, :P] = nr.decided_params(depth, gen).float(), nr.decided_params(depth, gen).float()
    samples = [nr.planted_blobs(2, blobs=3, per_blob=70)[:2], nr.planted_blobs(7, blobs=3, per_blob=50)[:2]]
    pc0s, c0, pc1, c1 = _pad_pair(samples)
    flow, info = nsfp.nsfp_optimize(pc0s, c0, pc1, c1, init=init, depth=depth, iters=1, trunc_d2=trunc)
    torch.cuda.synchronize()
    assert info["iters_run"] == 1 and info["loss_history"].shape == (1, 2)
    for b, (P0, P1) in enumerate(samples):
        P0t, P1t = torch.from_numpy(P0), torch.from_numpy(P1)
        wp = nr.wellposed(P0t, P1t, init[0, :P], init[1, :P], depth, trunc)
        print(b, wp)
        assert wp["min_gap"] > 1e-5 and wp["min_trunc_edge"] > 1e-3 and wp["small_z"] == 0, wp
        n0, n1 = len(P0), len(P1)
        i_w1, i_1w, i_c0, i_0c = (t[b].cpu().long() for t in info["nn"])
        nn = (i_w1[:n0], i_1w[:n1], i_c0[:n0], i_0c[:n0])
        for t, n in ((i_w1, n0), (i_1w, n1), (i_c0, n0), (i_0c, n0)):
            assert bool((t[n:] == -1).all()), "rows behind the counts find nothing"
        res = {}
        for dt in (torch.float64, torch.float32):
            f, g = init[0, :P].to(dt), init[1, :P].to(dt)
            loss, F, df, dg, nn_all = nr.iteration(P0t.to(dt), P1t.to(dt), f, g, depth, trunc, nn=nn)
            z = torch.zeros_like(f)
            res[dt] = (loss, F, df, dg, nr.adam_step(f, df, z, z, 1)[0], nr.adam_step(g, dg, z, z, 1)[0])
        free = nr.iteration(P0t.double(), P1t.double(), init[0, :P].double(), init[1, :P].double(), depth, trunc)[4]
        assert all(torch.equal(a, b_) for a, b_ in zip(nn, free)), "the op's neighbour rows are the all-pairs rows"
        r64, r32 = res[torch.float64], res[torch.float32]
        _close(info["loss_history"][0, b].reshape(1), r64[0].reshape(1), r32[0].reshape(1), f"loss[{b}]")
        _close(info["best_loss"][b].reshape(1), r64[0].reshape(1), r32[0].reshape(1), f"best_loss[{b}]")
        _close(flow[b, :n0], r64[1], r32[1], f"flow[{b}] (the start's F: the only iterate)")
        assert not flow[b, n0:].any()
        _close(info["grads"][b, 0, :P], r64[2], r32[2], f"df[{b}]")
        _close(info["grads"][b, 1, :P], r64[3], r32[3], f"dg[{b}]")
        _close(info["params"][b, 0, :P], r64[4], r32[4], f"f after the step [{b}]")
        _close(info["params"][b, 1, :P], r64[5], r32[5], f"g after the step [{b}]")


# ---- 5. loop logic --------------------------------------------------------------------------------------------------------------------
def test_loop_logic_is_exact():
    """snapshot / freeze from the op's own loss history, in a pure-Python replay; early stop, check_every and the graph change nothing"""
    from deflow_amd import nsfp
    samples = [nr.planted_blobs(2, blobs=3, per_blob=40, spacing=2.5, size=(1.2, 0.8, 0.6))[:2],
               nr.planted_blobs(3, blobs=2, per_blob=50, spacing=2.5, size=(1.2, 0.8, 0.6))[:2]]
    pc0s, c0, pc1, c1 = _pad_pair(samples)
    kw = dict(depth=1, iters=40, patience=4, min_delta=1e-3, seed=3)
    flow, info = nsfp.nsfp_optimize(pc0s, c0, pc1, c1, check_every=0, **kw)
    hist = info["loss_history"].cpu().numpy()
    assert info["iters_run"] == 40 and hist.shape == (40, 2) and np.isfinite(hist).all()
    args = []
    for b in range(2):
        best, stalled, frozen, arg = nr.replay(hist[:, b], kw["patience"], kw["min_delta"])
        print(b, "best", best, "stalled", stalled, "frozen", frozen, "argmin", arg)
        assert np.float32(info["best_loss"][b].item()) == best and int(info["stalled"][b]) == stalled and bool(info["frozen"][b]) == frozen
        args.append(arg)
        if frozen:                       # entries after the freeze keep the last value
            t = arg + kw["patience"]
            assert (hist[t:, b] == hist[t, b]).all()
    assert bool(info["frozen"].any()), "the case freezes at least one sample inside the budget"
    assert min(args) >= 1, "the best iterate is not the start"
    for b in range(2):
        f2, i2 = nsfp.nsfp_optimize(pc0s, c0, pc1, c1, check_every=0, **dict(kw, iters=args[b] + 1))
        assert torch.equal(_bits(f2[b]), _bits(flow[b])), "the flow is the best iterate's"
        assert torch.equal(_bits(i2["loss_history"][:, b]), _bits(info["loss_history"][:args[b] + 1, b]))
    # a sample alone: the same result as inside the batch (equal padded N)
    f1, i1 = nsfp.nsfp_optimize(pc0s[1:], c0[1:], pc1[1:], c1[1:], check_every=0, **kw)
    assert torch.equal(_bits(f1[0]), _bits(flow[1])) and torch.equal(_bits(i1["loss_history"][:, 0]), _bits(info["loss_history"][:, 1]))
    for other in (dict(check_every=5), dict(check_every=0, graph=True), dict(check_every=5, graph=True)):
        f3, i3 = nsfp.nsfp_optimize(pc0s, c0, pc1, c1, **dict(kw, **other))
        assert torch.equal(_bits(f3), _bits(flow)), other
        for k in ("best_loss", "loss_history", "stalled"):
            assert torch.equal(_bits(i3[k].float() if k == "stalled" else i3[k]), _bits(info[k].float() if k == "stalled" else info[k])), (other, k)
        assert torch.equal(i3["frozen"], info["frozen"])
        if other.get("check_every") and bool(info["frozen"].all()):
            assert i3["iters_run"] < 40


# ---- 6. planted motion ----------------------------------------------------------------------------------------------------------------
def test_planted_motion():
    """four rigid blobs of 60 rows (1.2 x 0.8 x 0.6 m, 2.5 m apart), the second sweep independently re-sampled and moved by 0.6 m each;
    depth 2, 120 iterations, seed 0, every other parameter at its default.  Chosen on the CPU with the helper: zero-flow EPE 0.600 m,
    float64 helper 0.0815 m, float32 helper 0.0813 m (a quarter of the zero-flow EPE is 0.150; the two agree within a factor 2).  The op
    must reach at most twice the float64 helper's EPE."""
    from deflow_amd import nsfp
    P0, P1, truth = nr.planted_blobs(2, blobs=4, per_blob=60, shift=0.6, spacing=2.5, size=(1.2, 0.8, 0.6))
    ref64 = 0.08150229483963692
    assert abs(float(np.linalg.norm(truth, axis=1).mean()) - 0.6) < 1e-6 and ref64 <= 0.6 / 4
    pc0s, c0, pc1, c1 = _pad_pair([(P0, P1)])
    flow, info = nsfp.nsfp_optimize(pc0s, c0, pc1, c1, depth=2, iters=120, seed=0)
    epe = float(np.linalg.norm(flow[0, :len(P0)].cpu().numpy() - truth, axis=1).mean())
    print("EPE", epe, "best_loss", float(info["best_loss"][0]), "helper float64", ref64)
    assert epe <= 2 * ref64


# ---- 7. through the stack -------------------------------------------------------------------------------------------------------------
def test_nsfp_inside_sweepflow_and_metrics():
    from helpers import rigid_ref as rr
    from helpers import sweep_flow_ref as SR
    from deflow_amd import metrics, nsfp, sweeps
    from deflow_amd.deflow import batch_transform
    rng = np.random.default_rng(9)
    host = {}
    scenes = [rr.planted_sample(4, n_vehicles=2, n_static=1, n_one=0, pad0=0, pad1=0), rr.planted_sample(5, n_vehicles=2, n_static=1, n_one=0, pad0=0, pad1=0)]
    for g, key in (("0", "pc0s"), ("1", "pc1")):
        raws, drops = [], []
        for s in scenes:
            ground = np.stack([rng.uniform(-45, 45, 60), rng.uniform(-45, 45, 60), rng.normal(-1.6, 0.02, 60)], axis=1).astype(np.float32)
            far = np.stack([rng.uniform(52, 60, 20), rng.uniform(-10, 10, 20), rng.uniform(0, 1, 20)], axis=1).astype(np.float32)
            raw = np.concatenate([s[key], ground, far, np.full((1, 3), np.nan, np.float32)])
            drop = np.concatenate([np.zeros(len(s[key])), np.ones(60), np.zeros(21)]).astype(np.uint8)
            p = rng.permutation(len(raw))
            raws.append(raw[p]), drops.append(drop[p])
        n = max(len(r) for r in raws) + 3
        host["raw" + g] = np.full((2, n, 3), np.nan, np.float32)
        host["drop" + g] = np.zeros((2, n), np.uint8)
        for b in range(2):
            host["raw" + g][b, :len(raws[b])], host["drop" + g][b, :len(raws[b])] = raws[b], drops[b]
        host["n" + g] = np.array([len(r) for r in raws], dtype=np.int32)
    pose0 = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1))
    pose1 = pose0.copy()
    pose1[:, :3, 3] = (0.3, -0.02, 0.004)
    d = lambda a: torch.from_numpy(a).to(DEV)
    model = nsfp.Nsfp(depth=1, iters=4, check_every=0)
    sf = sweeps.SweepFlow(model)
    args = (d(host["raw0"]), d(host["n0"]), d(host["drop0"]), d(host["raw1"]), d(host["n1"]), d(host["drop1"]), d(pose0), d(pose1))
    with torch.no_grad():
        est, dyn = sf.infer(*args)
        st = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in model.last_state.items()}
        est2, dyn2 = sf.infer(*args)
    assert torch.equal(est.view(torch.int32), est2.view(torch.int32)) and torch.equal(dyn, dyn2)
    est, dyn = est.cpu().numpy(), dyn.cpu().numpy()
    T = batch_transform({"pose0": d(pose0), "pose1": d(pose1)}, DEV).cpu().numpy()
    _, _, pos_of, kept = SR.compact_batch(host["raw0"], host["n0"], host["drop0"])
    want, want_dyn = SR.compose_batch(host["raw0"], host["n0"], T, pos_of, st["flow"], st["idx_c0"], st["counts0"])
    assert np.array_equal(est.view(np.int32), want.view(np.int32)) and np.array_equal(dyn, want_dyn)
    for b in range(2):
        c0 = int(st["counts0"][b])
        assert c0 == int(kept[b]) - 21 and np.isfinite(st["flow"][b]).all() and st["flow"][b][:c0].any() and not st["flow"][b][c0:].any()
    assert st["loss_history"].shape == (4, 2) and np.isfinite(st["best_loss"]).all()
    # forward()'s dict of lists into evaluate_batch, host and device
    keep0 = [(np.arange(host["raw0"].shape[1]) < host["n0"][b]) & (host["drop0"][b] == 0) for b in range(2)]
    batch = {"pc0": d(np.stack([np.concatenate([host["raw0"][b][keep0[b]], np.full((st["pc0s"].shape[1] - keep0[b].sum(), 3), np.nan, np.float32)])
                                for b in range(2)])),
             "pc1": d(st["points_c1"]), "pose0": d(pose0), "pose1": d(pose1)}
    batch["flow"] = torch.zeros_like(batch["pc0"])
    batch["flow_is_valid"] = torch.ones(batch["pc0"].shape[:2], dtype=torch.bool, device=DEV)
    batch["flow_category_indices"] = torch.ones(batch["pc0"].shape[:2], dtype=torch.uint8, device=DEV)
    with torch.no_grad():
        res = model(batch)
    assert sorted(res) == ["flow", "pc0_points_lst", "pc0_valid_point_idxes", "pc1_points_lst", "pc1_valid_point_idxes", "pose_flow"]
    assert [int(f.shape[0]) for f in res["flow"]] == st["counts0"].tolist()
    m = metrics.evaluate_batch(res, batch)
    assert {"EPE", "AccS", "AccR"} <= set(m) and all(np.isfinite(v) for v in m.values())
    from deflow_amd.metrics_device import DeviceMetrics, evaluate_batch_device
    dm = DeviceMetrics(torch.device(DEV))
    with torch.no_grad():
        evaluate_batch_device(model, batch, dm)
    assert abs(dm.summary()["EPE"] - m["EPE"]) < 1e-4


def test_save_vis_and_eval_commands(tmp_path, golden_dir, capsys):
    import json
    import os
    import shutil
    from deflow_amd import nsfp, save, vis
    from deflow_amd.h5scene import H5File
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "scene_val.h5"), tmp_path / "scene_val.h5")      # never written under tests/golden
    argv = ["model=nsfp", f"dataset_path={tmp_path}", "nsfp_iters=3", "nsfp_depth=1", "nsfp_check_every=0",
            "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"]
    assert save.main(argv) == 0
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert [x["scene"] for x in lines] == ["scene_val"] and lines[0]["sweeps"] >= 2
    path = save.flow_path(str(tmp_path), "scene_val", "nsfp")
    assert os.path.basename(path) == "scene_val.nsfp.flow.npz"
    got, meta = save.read_flow(path), save.read_meta(path)
    assert meta == {"res_name": "nsfp", "checkpoint": None, "model": "nsfp", "voxel_size": [0.2, 0.2, 6.0],
                    "point_cloud_range": [-6.4, -6.4, -3.0, 6.4, 6.4, 3.0], "ground_source": "auto", "half": False,
                    "params": dict(nsfp.DEFAULTS, iters=3, depth=1, check_every=0), "definition": "DESIGN.md 6f, 6k (UNPINNED)"}
    with H5File(str(tmp_path / "scene_val.h5")) as f:
        ts = sorted(f.keys(), key=int)
        rows = {t: int(f[t]["lidar"].read().shape[0]) for t in ts}
    assert list(got) == ts[:-1]
    for t in ts[:-1]:
        assert got[t][0].dtype == np.float32 and got[t][0].shape == (rows[t], 3) and np.isfinite(got[t][0]).all()
    out_dir = tmp_path / "png"
    assert vis.main([f"dataset_path={tmp_path}", "res_name=nsfp", "scenes=scene_val", f"out_dir={out_dir}", "range=6.4", "res=0.2",
                     "panels=est"]) == 0
    line = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")][0]
    assert line["scene"] == "scene_val" and line["images"] >= 2 and len(os.listdir(out_dir / "scene_val")) == line["images"]
    from deflow_amd import eval as ev
    shutil.copy(os.path.join(golden_dir, "av2_mini", "val", "index_total.pkl"), tmp_path / "index_total.pkl")
    out = ev.main(["model=nsfp", f"val_data={tmp_path}", "nsfp_iters=3", "nsfp_depth=1", "point_cloud_range=[-6.4,-6.4,-3,6.4,6.4,3]"])
    result = json.loads([x for x in capsys.readouterr().out.splitlines() if x.startswith("{")][-1])
    assert result["model"] == "nsfp" and result["checkpoint"] is None and "EPE" in result["metrics"] and "leaderboard" in out
