"""Bit-reproducibility soaks beside a concurrent neighbour (round 5; were tools/archive/grad_repro_probe.py / tools/archive/pfn_bwd_stress.py runs
recorded in profiles/r04_pfn_race_probe.txt).  History: the pillar feature net's backward kernels returned wrong sums in ~4 % of
their launches while the GRU decoder's forward kernel ran on another stream driven by another host thread -- with the SLP-vectorised
(packed-fp32) build of csrc/pillarize.hip only; the library builds that file with -fno-slp-vectorize (deflow_amd/build.py) and the cause
below the ISA was never identified.  These tests fence that state: the shipped library must be bit-reproducible

  * for the pillar feature net's backward on fixed inputs,
  * for the sparse kernels at the UNet's ends on fixed inputs (sparse_wgrad3x3_x2_kernel emits a packed fp32 subtraction on purpose), and
  * for the whole training step (fp32 and bf16, weight gradients on the side stream),

while a second host thread of this process keeps the GRU decoder's forward kernel -- the one neighbour that triggered it -- running on
its own stream (both generations: the lean kernel the engine runs now, and the round-3/4 kernel that was the original trigger).
Sized to a few seconds each."""
import os
import sys
import threading
import time

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


class GruNeighbour:
    """a host thread that keeps df_gru_* forward launches in flight on its own stream until stopped"""

    def __init__(self, dev, lean: bool):
        from test_gpu_model import build_pair
        self.dev, self.lean = dev, lean
        _, model = build_pair(dev, 43, decoder_option="gru", num_iters=2)
        self.head = model.eval().head
        self.stop, self.count, self.err = threading.Event(), 0, None
        self.th = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        try:
            torch.cuda.set_device(self.dev)
            if not self.lean:
                os.environ["DF_GRU_LEAN"] = "0"          # (read per call: this thread's launches only matter)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s), torch.no_grad():
                B, H, W = 2, 64, 64
                before = torch.randn(B, H, W, 64, device=self.dev)
                after = torch.randn(B, H, W, 64, device=self.dev)
                from deflow_amd._lib import img
                from deflow_amd.decoder import PointSet
                N = 1500
                coords = torch.zeros(B, N, 3, dtype=torch.int32, device=self.dev)
                coords[..., 1:] = torch.randint(0, H, (B, N, 2), device=self.dev, dtype=torch.int32)
                offs = (torch.rand(B, N, 3, device=self.dev) - 0.5) * 0.2
                counts = torch.full((B,), N - 100, dtype=torch.int32, device=self.dev)
                ps = PointSet(coords, offs, counts)
                while not self.stop.is_set():
                    for _ in range(8):
                        self.head.run(img(before), img(after), ps, False)
                    self.count += 8
                    s.synchronize()
        except Exception as e:      # noqa: BLE001
            self.err = e

    def __enter__(self):
        self.th.start()
        t0 = time.time()
        while self.count < 64 and self.err is None and time.time() - t0 < 60:
            time.sleep(0.05)
        assert self.err is None, self.err
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.th.join(30.0)
        os.environ.pop("DF_GRU_LEAN", None)
        assert self.err is None, self.err
        return False


@pytest.mark.parametrize("lean", [True, False], ids=["gru_fwd4", "gru_fwd3"])
def test_pfn_backward_is_bit_reproducible_beside_the_gru_forward(dev, lean):
    """df_pfn_bwd_stats / _finalize / _weights + the column sum on FIXED inputs, 1500 repetitions beside the neighbour"""
    from test_gpu_model import build_pair, make_batch, to_dev
    from deflow_amd._lib import img
    _, model = build_pair(dev, 41, decoder_option="gru", num_iters=2)
    model.train()
    batch = to_dev(make_batch(2, 1500, 7000), dev)
    with torch.no_grad():
        st = model.forward_padded(batch, engine_tape=True)["engine"]
    emb = model.embedder
    dbstar = torch.randn(2, 64, 64, 64, generator=torch.Generator().manual_seed(3)).to(dev)
    torch.cuda.synchronize()
    first, nbad, worst = None, 0, 0.0
    with GruNeighbour(dev, lean) as nb:
        t0 = time.time()
        reps = 0
        while reps < 1500 and time.time() - t0 < 12:
            g = emb.pillarize_bwd(st["p0"], img(dbstar, 32, 0), None)
            g = emb.pillarize_bwd(st["p1"], img(dbstar, 32, 32), g)
            cur = torch.cat([t.reshape(-1) for t in g]).clone()
            torch.cuda.synchronize()
            if first is None:
                first = cur
            elif not torch.equal(cur, first):
                nbad += 1
                worst = max(worst, float((cur - first).abs().max() / first.abs().max()))
            reps += 1
        ran = nb.count
    assert reps >= 300 and ran >= 64, (reps, ran)
    assert nbad == 0, f"{nbad} of {reps} repetitions differ from the first (worst rel {worst:.2e}) beside {ran} neighbour launches"


@pytest.mark.parametrize("lean", [True, False], ids=["gru_fwd4", "gru_fwd3"])
def test_sparse_edge_kernels_are_bit_reproducible_beside_the_gru_forward(dev, lean):
    """df_pillar_input_grad, df_sparse_conv3x3_h2, df_sparse_wgrad3x3_x2 (whose residual split is ONE packed fp32 subtraction per pair, in a
    file otherwise built without the SLP vectoriser), df_sparse_in_wgrad and the fp32-MFMA form df_sparse_wgrad3x3 (the engine's choice
    outside the packed-coordinate bound and with DF_GRU_X2=0) on the FIXED inputs of the `wrap` case of
    tests/helpers/sparse_cases.py, beside the neighbour: every repetition bit-equal to the first"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
    import sparse_cases as SC
    from deflow_amd._lib import call, img, ptr, stream
    c = SC.case("wrap")
    B, H, W, nblk = c.B, c.H, c.W, c.nblk
    t = {k: v.to(dev) for k, v in c.t.items()}
    keys, counts = c.keys.to(dev), c.counts.to(dev)
    w = t["w"].permute(0, 2, 3, 1).contiguous()
    w1 = t["w1"].permute(0, 2, 3, 1).contiguous()
    w3 = t["w3"].reshape(64, 64).contiguous()
    xa, wa = torch.zeros(1, device=dev), torch.zeros(1, device=dev)
    call("df_absmax", img(t["x"]), ptr(xa), stream())
    call("df_absmax", img(w.reshape(1, 1, -1, 64)), ptr(wa), stream())
    w2 = torch.empty(2 * w.numel(), dtype=torch.float16, device=dev)
    call("df_split_h2", ptr(w), ptr(wa), ptr(w2), w.numel(), stream())
    dc = torch.zeros(B, H, W, 64, device=dev)
    y = torch.zeros(B, H, W, 64, device=dev)
    ws = torch.zeros(nblk * B, 64 * 9 * 64, device=dev)
    bws = torch.zeros(nblk * B, 64, device=dev)
    ws1 = torch.zeros(nblk * B, 64 * 9 * 32, device=dev)
    ws0, bws0 = torch.zeros_like(ws), torch.zeros_like(bws)
    torch.cuda.synchronize()
    first, nbad, worst = None, 0, 0.0
    with GruNeighbour(dev, lean) as nb:
        t0 = time.time()
        reps = 0
        while reps < 1500 and time.time() - t0 < 12:
            for g in (0, 1):
                call("df_pillar_input_grad", ptr(keys), ptr(counts), B, H, W, g, ptr(t["dy1"]), ptr(w1), img(t["dskip"]), ptr(w3),
                     img(dc, 32, 32 * g), 0, nblk, stream())
            call("df_sparse_conv3x3_h2", ptr(keys), ptr(counts), B, img(t["x"]), ptr(w2), ptr(xa), ptr(wa), ptr(t["bias"]), img(y), nblk, stream())
            call("df_sparse_wgrad3x3_x2", ptr(keys), ptr(counts), B, img(t["x"]), img(t["dy"]), ptr(ws), ptr(bws), nblk, stream())
            call("df_sparse_wgrad3x3", ptr(keys), ptr(counts), B, img(t["x"]), img(t["dy"]), ptr(ws0), ptr(bws0), nblk, stream())
            call("df_sparse_in_wgrad", ptr(keys), ptr(counts), B, H, W, 1, ptr(t["dy1"]), img(t["canvas"], 32, 32), ptr(ws1), nblk, stream())
            cur = torch.cat([v.reshape(-1) for v in (dc, y, ws, bws, ws1, ws0, bws0)])
            torch.cuda.synchronize()
            if first is None:
                first = cur
            elif not torch.equal(cur, first):
                nbad += 1
                worst = max(worst, float((cur - first).abs().max() / first.abs().max()))
            reps += 1
        ran = nb.count
    print(f"[soak] sparse edge kernels: {reps} repetitions, {nbad} differ, beside {ran} neighbour launches")
    assert reps >= 300 and ran >= 64, (reps, ran)
    assert nbad == 0, f"{nbad} of {reps} repetitions differ from the first (worst rel {worst:.2e}) beside {ran} neighbour launches"


@pytest.mark.slow
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_training_step_is_bit_reproducible_beside_the_gru_forward(dev, dtype, monkeypatch):
    """the whole step (lr = 0: the same problem every time), weight gradients on the side stream, gradient arena compared bit for bit"""
    from test_gpu_model import build_pair, make_batch, to_dev
    from deflow_amd.optim import Trainer
    monkeypatch.setenv("DF_SIDE_STREAM", "1")
    _, model = build_pair(dev, 41, decoder_option="gru", num_iters=2)
    model.train()
    batch = to_dev(make_batch(2, 1500, 7000), dev)
    tr = Trainer(model, lr=0.0, dtype=dtype)
    for _ in range(2):
        tr.step(batch)
    torch.cuda.synchronize()
    first, bad = None, []
    with GruNeighbour(dev, True) as nb:
        t0 = time.time()
        reps = 0
        while reps < 600 and time.time() - t0 < 12:
            tr.step(batch)
            cur = tr.flat.grad.clone()
            torch.cuda.synchronize()
            if first is None:
                first = cur
            elif not torch.equal(cur, first):
                d = (cur - first).abs()
                names = [n for n, p in tr.flat.named if float(d[tr.flat.slots[n][0]: tr.flat.slots[n][0] + tr.flat.slots[n][1]].max()) > 0]
                bad.append((reps, names[:4]))
            reps += 1
        ran = nb.count
    assert reps >= 100 and ran >= 64, (reps, ran)
    assert not bad, f"{len(bad)} of {reps} steps differ from the first, e.g. {bad[:3]} (beside {ran} neighbour launches)"
