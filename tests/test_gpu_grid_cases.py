"""GPU: the two searches over the xy row grid of df_nn_grid_build held to their references at cell edges, exact radii and ring ties -- the
cases of tests/helpers/grid_cases.py, whose input conditions and wrong variants tests/test_grid_cases_cpu.py checks without a GPU.

The ring walk (csrc/nn_search.h: nn_ring_search), per search case:
  df_chamfer_nn      idx equals float64 all pairs on EVERY participating row (no near-tie exemption: the rows that test_gpu_seflow.py's
                     check_nn would exempt -- best and second-best within 1e-5 relative -- are only the exact ties of the dyadic cases
                     and the eight binade queries of beyond_square, asserted here; on all other rows that share is 0), +inf / -1 exactly
                     where the header says, d2 bit-equal to float64's on the dyadic cases and within 1e-6 relative elsewhere, far_count
                     equal to the number of queries whose restated walk scans a ring >= 2, a repeated call bit-identical
  df_reg_accumulate  identity T, the case's gate (1e30 where the case has none; not run at max_dist2 = 0, which the entry refuses): idx_out
                     and d2_out bit-equal to df_chamfer_nn's, q_out the query itself, w_out > 0 on exactly the gated rows
The fixed-radius window (csrc/cluster.hip), per DBSCAN case: labels and n_clusters equal dbscan_ref's, status 0, a repeated call
bit-identical -- through cluster.dbscan (cell = 1.0025 eps) and, for binade_abi and exact_eps, through the three C entries on a grid with
cell == eps, where a 3 x 3 window gives two clusters for one.  Freed allocator blocks are poisoned before every call.

Shapes: N <= 1331 rows, B <= 2, grids of 1 to 4096 cells a side (the 4096 one with B = 1: its cell ranges take 134 MB).

Measured on an MI355X: 0 wrong neighbours on all 14 search cases (2 655 participating queries), d2 error 0 on the four dyadic cases and
at most 1.88e-7 relative elsewhere (single_ref; g4096 1.45e-7, outside 1.43e-7), far_count equal to the restated walk's on every case
(88, 88, 2, 24, 0, 0, 0, 0, 1, 324, 200, 250, 225, 225 in the order of gc.SEARCH_NAMES), df_reg_accumulate bit-equal throughout; every
DBSCAN case equal to the reference with status 0 both ways.  With the 3 x 3 window the stages had before (that cluster.hip built on its
own), binade_abi through the C entries at cell == eps gives 10 clusters for 6: every linked pair of groups split, both lone members
noise, 56 of 62 labels off.  The 32 tests take 3.1 s together, references included."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import grid_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
NO_GATE = 1e30                       # the finite gate df_reg_accumulate gets where the case has none (every d2 is below 1e9)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def _dirty(dev, value):
    """leave `value` in freed blocks of the caching allocator, so that an output element the kernels skip shows it"""
    junk = [torch.full((n,), value, dtype=torch.int16, device=dev) for n in (1 << 22, 1 << 20, 1 << 18, 1 << 16, 4096, 512)]
    torch.cuda.synchronize()
    del junk


def bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _dev(a, dev, dtype=None):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, device=dev)       # (a copy: the cases' arrays are read-only)


# ---- the ring walk ----------------------------------------------------------------------------------------------------------------------
def run_chamfer(c, dev):
    from deflow_amd.chamfer import chamfer_nn
    q, r = _dev(c.query, dev), _dev(c.refs, dev)
    qc, rc = _dev(c.qcount, dev, torch.int32), _dev(c.rcount, dev, torch.int32)
    ql, rl = _dev(c.qlabel, dev), _dev(c.rlabel, dev)
    outs = []
    for fill in (0x7fc0, 0x3039):                                   # NaN-ish / 12345-ish patterns in whatever the outputs land on
        _dirty(dev, fill)
        far = torch.zeros(1, dtype=torch.int32, device=dev)
        d2, idx = chamfer_nn(q, qc, r, rc, ql, rl, c.max_dist2, grid_range=c.xy_range, cell=c.cell, far_count=far)
        torch.cuda.synchronize()
        outs.append((d2, idx, far))
    assert all(bits(a) == bits(b) for a, b in zip(*outs)), f"{c.name}: a repeated call differs"
    return outs[0]


def run_accumulate(c, dev, gate):
    """both clouds filed under the case's grid, then ONE df_reg_accumulate at T = identity on poisoned per-row outputs"""
    from deflow_amd._lib import call, ptr, stream
    from deflow_amd.chamfer import RowGrid
    q, r = _dev(c.query, dev), _dev(c.refs, dev)
    B, Ns = q.shape[:2]
    grid = RowGrid(B, c.xy_range, c.cell, dev)
    assert grid.G == c.G
    s_rng, s_rows = grid.file(q, _dev(c.qcount, dev, torch.int32), _dev(c.qlabel, dev))
    d_rng, d_rows = grid.file(r, _dev(c.rcount, dev, torch.int32), _dev(c.rlabel, dev))
    T = torch.eye(4, dtype=torch.float64, device=dev).reshape(1, 16).repeat(B, 1).contiguous()
    nblk = (Ns + 255) // 256
    _dirty(dev, 0x7fc0)
    partial = torch.full((B, nblk, 32), float("nan"), dtype=torch.float64, device=dev)
    qo = torch.full((B, Ns, 3), float("nan"), dtype=torch.float32, device=dev)
    idx = torch.full((B, Ns), 12345, dtype=torch.int32, device=dev)
    d2 = torch.full((B, Ns), float("nan"), dtype=torch.float32, device=dev)
    w = torch.full((B, Ns), float("nan"), dtype=torch.float32, device=dev)
    call("df_reg_accumulate", ptr(s_rng), ptr(s_rows), grid.G, ptr(d_rng), ptr(d_rows), grid.minx, grid.miny, grid.cell, grid.G, B, Ns, 1,
         ptr(T), float(gate), float(gate) / 9.0, ptr(partial), ptr(qo), ptr(idx), ptr(d2), ptr(w), stream())
    torch.cuda.synchronize()
    return qo, idx, d2, w, partial


@pytest.mark.parametrize("name", gc.SEARCH_NAMES)
def test_search_case(dev, name):
    c, ref = gc.search_case(name), gc.search_ref(name)
    part, want = ref["part"], ref["idx"]
    d2, idx, far = run_chamfer(c, dev)
    d2_h, idx_h = d2.cpu().numpy(), idx.cpu().numpy()
    assert d2_h.shape == part.shape and idx_h.dtype == np.int32 and d2_h.dtype == np.float32
    hit = part & (want >= 0)
    wrong = np.argwhere(idx_h != want)
    rel = np.abs(d2_h[hit].astype(np.float64) - ref["d2"][hit]) / np.maximum(ref["d2"][hit], 1e-30)
    rel = np.where(ref["d2"][hit] == 0, d2_h[hit], rel)
    # the rows check_nn's near-tie rule would exempt: only exact ties and the designated narrow rows
    with np.errstate(invalid="ignore"):                                              # (inf - inf where nothing takes part)
        near_tie = hit & ~((ref["d2nd"] - ref["d2"]) > 1e-5 * ref["d2"])
    exact_tie = hit & (ref["d2nd"] == ref["d2"])
    narrow = np.zeros_like(hit)
    narrow[0, list(c.narrow)] = True
    other = near_tie & ~exact_tie & ~narrow
    walked = gc.walk(name)[1]
    print(f"[{name}] G {c.G}: {int(hit.sum())} neighbours of {int(part.sum())} queries, {len(wrong)} idx differ, max rel d2 error "
          f"{float(rel.max()) if rel.size else 0:.3g}, exact ties {int(exact_tie.sum())}, narrow {int(narrow.sum())}, other near-ties "
          f"{int(other.sum())}, far_count {int(far)} (restated walk: {int((walked >= 2).sum())})")
    assert other.sum() == 0 and (exact_tie.sum() == 0 or c.dyadic)
    assert len(wrong) == 0, wrong[:10]                                               # every row, the non-participating ones (-1) included
    assert np.all(np.isposinf(d2_h[~hit])) and np.all(idx_h[~hit] == -1)             # +inf / -1 exactly where the header says
    if c.dyadic:
        assert np.array_equal(d2_h[hit].astype(np.float64), ref["d2"][hit])          # bit-equal: every difference, square and sum is exact
    else:
        assert rel.size == 0 or rel.max() <= 1e-6
    assert int(far) == int((walked >= 2).sum())
    if c.max_dist2 > 0:
        gate = c.max_dist2 if np.isfinite(c.max_dist2) else NO_GATE
        assert np.isfinite(c.max_dist2) or ref["d2"][hit].max() < 1e9
        qo, ridx, rd2, w, partial = run_accumulate(c, dev, gate)
        assert bits(ridx) == bits(idx) and bits(rd2) == bits(d2)                     # ONE body: bit for bit at these edges
        w_h, qo_h = w.cpu().numpy(), qo.cpu().numpy()
        assert np.array_equal(w_h > 0, hit) and np.all(w_h[~hit] == 0)
        assert np.array_equal(qo_h[part], c.query[part]) and np.all(qo_h[~part] == 0)
        assert torch.isfinite(partial).all() and np.array_equal(partial[:, :, 29].sum(1).cpu().numpy(), hit.sum(1).astype(np.float64))


# ---- DBSCAN -----------------------------------------------------------------------------------------------------------------------------
def through_the_wrapper(c, dev):
    from deflow_amd.cluster import dbscan
    p, n = _dev(c.points, dev), _dev(c.count, dev, torch.int32)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lab, k = dbscan(p, n, eps=c.eps, min_points=c.min_points, min_cluster_size=c.min_cluster_size, grid_range=c.xy_range, status=status)
    return lab, k, status


def through_the_entries(c, dev, cell, lib_call=None):
    """df_dbscan_core / _link / _finish on a grid with the given cell (the documented C contract: cell >= eps).  lib_call(name, *args):
    another build's entries (default: this library's)"""
    from deflow_amd._lib import call, ptr, stream
    from deflow_amd.chamfer import RowGrid
    lib_call = lib_call or call
    p, n = _dev(c.points, dev), _dev(c.count, dev, torch.int32)
    B, N = p.shape[:2]
    grid = RowGrid(B, c.xy_range, cell, dev)
    cell_rng, rows = grid.file(p, n)
    ws = torch.empty(call("df_dbscan_ws_bytes", B, N), dtype=torch.uint8, device=dev)
    lab = torch.full((B, N), 12345, dtype=torch.int32, device=dev)
    k = torch.full((B,), 12345, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    a = (grid.minx, grid.miny, grid.cell, grid.G, c.eps)
    lib_call("df_dbscan_core", ptr(cell_rng), ptr(rows), B, N, *a, c.min_points, ptr(ws), stream())
    lib_call("df_dbscan_link", ptr(cell_rng), B, N, *a, ptr(status), ptr(ws), stream())
    lib_call("df_dbscan_finish", ptr(cell_rng), None, B, N, *a, c.min_cluster_size, 0.0, ptr(lab), ptr(k), ptr(status), ptr(ws), stream())
    return lab, k, status


def hold_to_reference(name, dev, run, what):
    want, wantk, _ = gc.dbscan_want(name)
    outs = []
    for fill in (0x7fc0, 0x3039):
        _dirty(dev, fill)
        lab, k, status = run()
        torch.cuda.synchronize()
        outs.append((lab, k, status))
    lab, k, status = outs[0]
    differ = int((lab.cpu().long() != want).sum())
    print(f"[{name}] {what}: clusters {wantk.tolist()} (op {k.tolist()}), {differ} labels differ, status {int(status)}")
    assert all(bits(a) == bits(b) for a, b in zip(*outs)), f"{name}: a repeated call differs"
    assert int(status) == 0 and lab.dtype == torch.int32 and k.dtype == torch.int32
    assert torch.equal(k.cpu().long(), wantk) and differ == 0
    return lab.cpu().numpy()


@pytest.mark.parametrize("name", gc.DBSCAN_NAMES)
def test_dbscan_case(dev, name):
    c = gc.dbscan_case(name)
    hold_to_reference(name, dev, lambda: through_the_wrapper(c, dev), "cluster.dbscan, cell 1.0025 eps")


@pytest.mark.parametrize("name", [n for n in gc.DBSCAN_NAMES if n.startswith(("binade_abi", "exact_eps"))])
def test_dbscan_entries_at_cell_equal_eps(dev, name):
    """the C contract says cell >= eps: at cell == eps the pairs of binade_abi are filed two cells apart, and the window must still hold
    them -- one cluster per linked pair of groups (the 3 x 3 window: two), the lone member a border row of its partner's cluster"""
    c = gc.dbscan_case(name)
    lab = hold_to_reference(name, dev, lambda: through_the_entries(c, dev, c.eps), "the C entries, cell == eps")
    for i, j, _ in getattr(c, "links", []) + getattr(c, "borders", []):
        assert lab[0, i] == lab[0, j] > 0
