"""Measure model=nsfp's optimisation loop on one pair of 80 000 + 80 000 synthetic rows (B = 1) and write profiles/nsfp_flow.json:
ms per iteration, eager and as a replayed HIP graph, and the split of one iteration over the MLP forward, the MLP backward, the searches
and grid builds, the loss reductions with the point gradients, and Adam.  Medians of 10, by device events.  For the MLP kernels the
algorithmic TFLOP/s against the roof of the product form they use (fp32 MFMA: 157 TFLOP/s).  No thresholds: the numbers are written
down with the box they came from.

    python tools/nsfp_bench.py [--rows 80000] [--depth 7] [--out profiles/nsfp_flow.json]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deflow_amd import chamfer, nsfp, pairopt  # noqa: E402
from deflow_amd._lib import call, ptr, stream  # noqa: E402
from deflow_amd.chamfer import chamfer_bwd  # noqa: E402

ROOF_FP32_MFMA = 157.0     # TFLOP/s, v_mfma_f32_16x16x4_f32 (a three-MFMA split form would be measured against 2500 / 3)


def median_ms(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--depth", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nsfp_flow.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    N, depth = a.rows, a.depth
    gen = torch.Generator().manual_seed(0)
    scale = torch.tensor([50.0, 50.0, 2.0])
    p0 = ((torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale).to(dev)
    p1 = ((torch.rand(1, N, 3, generator=gen) * 2 - 1) * scale + torch.tensor([0.4, 0.1, 0.0])).to(dev)
    cnt = torch.full((1,), N, dtype=torch.int32, device=dev)

    def loop(iters, graph):
        return lambda: nsfp.nsfp_optimize(p0, cnt, p1, cnt, depth=depth, iters=iters, check_every=0, graph=graph)

    res = {"shape": {"batch": 1, "rows_pc0": N, "rows_pc1": N, "depth": depth, "width": nsfp.WIDTH},
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "method": "device events, median of 10"}
    lo, hi = 3, 13
    for name, graph in (("eager", False), ("graph", True)):
        t_lo, t_hi = median_ms(loop(lo, graph)), median_ms(loop(hi, graph))
        res[f"ms_per_iteration_{name}"] = round((t_hi - t_lo) / (hi - lo), 4)
        res[f"ms_{name}_{lo}_iterations"], res[f"ms_{name}_{hi}_iterations"] = round(t_lo, 3), round(t_hi, 3)

    # the split of one iteration, every part timed alone on the tensors the loop hands it
    S = nsfp.param_stride(depth)
    arena = nsfp.init_params(depth, 0).to(dev)[None].contiguous()
    par = arena[:, 0]
    y, acts = nsfp.mlp_forward(p0, cnt, par, depth)
    dy = torch.randn_like(y)
    W = p0 + y
    lab = torch.ones(1, N, dtype=torch.int32, device=dev)
    search = chamfer.RowGrid(1, chamfer.GRID_RANGE, chamfer.CELL, dev)
    grid1 = search.file(p1, cnt, lab)
    d2, idx = search.nn(W, cnt, lab, grid1, 4.0)
    g = pairopt.mean_and_weight(d2)[1]
    buf = torch.zeros_like(W)
    grads, m, v = torch.zeros_like(arena), torch.zeros_like(arena), torch.zeros_like(arena)
    step = torch.ones(1, dtype=torch.int32, device=dev)
    ms_fwd = median_ms(lambda: nsfp.mlp_forward(p0, cnt, par, depth))
    ms_bwd = median_ms(lambda: nsfp.mlp_backward(p0, cnt, par, depth, acts, dy, need_dx=True))
    ms_nn = median_ms(lambda: search.nn(W, cnt, lab, grid1, 4.0))
    ms_build = median_ms(lambda: search.file(W, cnt, lab))
    ms_red = median_ms(lambda: pairopt.mean_and_weight(d2))
    ms_cq = median_ms(lambda: chamfer_bwd(W, p1, idx, g, buf, None))
    ms_cr = median_ms(lambda: chamfer_bwd(W, p1, idx, g, None, buf))
    ms_adam = median_ms(lambda: call("df_adam_step_dev", ptr(arena), ptr(grads), ptr(m), ptr(v), arena.numel(), 8e-3, *pairopt.BETAS, pairopt.EPS,
                                     ptr(step), 1.0, stream()))
    hid = depth * 128 * 128
    flop_fwd = 2.0 * N * (3 * 128 + hid + 128 * 3)
    flop_bwd = 2.0 * N * (128 * 3 + hid + 128 * 3) + 2.0 * N * (3 * 128 + hid + 128 * 3)
    res["split_ms"] = {
        "mlp_forward (x2 per iteration)": round(ms_fwd, 4), "mlp_backward with dx (x2 per iteration, one without dx)": round(ms_bwd, 4),
        "search (x4 per iteration)": round(ms_nn, 4), "grid_build (x2 per iteration)": round(ms_build, 4),
        "loss_reduction (x4 per iteration)": round(ms_red, 4), "point_gradient to queries (x2)": round(ms_cq, 4),
        "point_gradient to references (x2)": round(ms_cr, 4), "adam (x1, both nets)": round(ms_adam, 4)}
    res["split_ms_per_iteration_estimate"] = {
        "mlp_forward": round(2 * ms_fwd, 4), "mlp_backward": round(2 * ms_bwd, 4), "searches_and_grid_builds": round(4 * ms_nn + 2 * ms_build, 4),
        "loss_reductions_and_point_gradients": round(4 * ms_red + 2 * ms_cq + 2 * ms_cr, 4), "adam": round(ms_adam, 4)}
    res["mlp_tflops"] = {"product_form": "v_mfma_f32_16x16x4_f32 (fp32 operands)", "roof_tflops": ROOF_FP32_MFMA,
                         "forward_gflop": round(flop_fwd / 1e9, 3), "forward_tflops": round(flop_fwd / ms_fwd / 1e9, 2),
                         "forward_fraction_of_roof": round(flop_fwd / ms_fwd / 1e9 / ROOF_FP32_MFMA, 4),
                         "backward_gflop": round(flop_bwd / 1e9, 3), "backward_tflops": round(flop_bwd / ms_bwd / 1e9, 2),
                         "backward_fraction_of_roof": round(flop_bwd / ms_bwd / 1e9 / ROOF_FP32_MFMA, 4)}
    res["unexamined"] = ("no hardware counters were collected: where the MLP kernels' time goes (L2 weight streaming, LDS, MFMA issue, the "
                         "activation writes to HBM) is not examined; the search times are those of uniformly random rows, not of a real sweep")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
