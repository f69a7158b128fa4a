"""CPU: the conditions that make tests/test_gpu_decoder_cases.py meaningful, decided without a GPU.

  * the oracle's own fp32-vs-float64 error on every case and tensor is at most 2.5e-5, so parity.three_way's bound
    max(1e-4, 4 x that) is the project's 1e-4 floor and nothing wider;
  * one 16-row stage of the weight-gradient walks (rows 32-47 of the first sample with at least 48 rows) carries at least 1e-3 of
    every parameter gradient in both norms -- a dropped or doubled stage shows at ten times the floor -- and so does one row of a
    70-row cell in d(after);
  * the counts really give the split-K walks what the cases were built for (stages per split, splits across a sample / an iteration
    boundary, the two-stage column sum's threshold, the row-tile edges).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import decoder_cases as DC  # noqa: E402
import parity  # noqa: E402

CASES = ["edges", "walk", "blocks"]
ORACLE_ERR_MAX = 2.5e-5
SHARE_MIN = 1e-3


def _tensors(r):
    out = {f"flow[{b}]": f for b, f in enumerate(r["flow"]) if f.numel()}
    out.update({"d(before)": r["gbefore"], "d(after)": r["gafter"]})
    out.update({"grad " + k: v for k, v in r["gw"].items()})
    return out


@pytest.mark.parametrize("name", CASES)
def test_oracle_fp32_error_leaves_the_floor(name):
    r32, r64 = DC.reference(name)
    t32, t64 = _tensors(r32), _tensors(r64)
    worst = 0.0
    for k in t64:
        e, r = parity.rel_err(t32[k], t64[k]), parity.rms_rel(t32[k], t64[k])
        worst = max(worst, e, r)
        assert e <= ORACLE_ERR_MAX and r <= ORACLE_ERR_MAX, f"{name} {k}: oracle fp32 vs float64 max {e:.3e} rms {r:.3e}"
    print(f"[decoder cases] {name}: worst oracle fp32-vs-float64 error over {len(t64)} tensors: {worst:.2e} (limit {ORACLE_ERR_MAX:.1e})")


def _share(part, whole):
    return float(part.abs().max() / whole.abs().max()), float(part.norm() / whole.norm())


@pytest.mark.parametrize("name", ["walk", "blocks"])
def test_one_stage_is_visible_in_every_parameter_gradient(name):
    c = DC.case(name)
    _, r64 = DC.reference(name)
    b = next(i for i, n in enumerate(c.counts) if n >= 48)
    _, _, gw = DC.rows_contribution(c, b, slice(32, 48))
    worst = min(min(_share(g, r64["gw"][k])) for k, g in gw.items())
    for k, g in gw.items():
        m, r = _share(g, r64["gw"][k])
        assert m >= SHARE_MIN and r >= SHARE_MIN, f"{name} grad {k}: rows 32-47 of sample {b} carry max {m:.2e} rms {r:.2e} of it"
    print(f"[decoder cases] {name}: stage rows 32-47 of sample {b}: smallest share of a parameter gradient {worst:.2e} (needs {SHARE_MIN:.0e})")


@pytest.mark.parametrize("name", CASES)
def test_one_row_of_the_heavy_cell_is_visible_in_d_after(name):
    c = DC.case(name)
    _, r64 = DC.reference(name)
    b, cell = next(iter(c.heavy.items()))
    rows = (c.cells(b) == cell).nonzero().squeeze(1)
    assert rows.numel() == DC.HEAVY_ROWS >= 70
    i = int(rows[DC.HEAVY_ROWS // 2])
    _, ga, _ = DC.rows_contribution(c, b, slice(i, i + 1))
    m, r = _share(ga, r64["gafter"])
    print(f"[decoder cases] {name}: row {i} of the {DC.HEAVY_ROWS}-row cell of sample {b}: share of d(after) max {m:.2e} rms {r:.2e}")
    assert m >= SHARE_MIN and r >= SHARE_MIN


def _splits():
    from deflow_amd._lib import call
    return call("df_gru_wgrad_splits"), int(os.environ.get("DF_GRU_HEAD_SPLITS", "1024"))


def test_walk_structure():
    c = DC.case("walk")
    nsplit, _ = _splits()
    owner = DC.stage_owner(c.counts, c.iters)
    S = sum(DC.stages_per_sample(c.counts))
    assert len(owner) == S * c.iters
    rng = DC.split_ranges(len(owner), nsplit)
    per = [w1 - w0 for w0, w1 in rng]
    cross_sample = sum(1 for w0, w1 in rng if w1 > w0 and owner[w0][1] != owner[w1 - 1][1] and owner[w0][0] == owner[w1 - 1][0])
    cross_iter = sum(1 for w0, w1 in rng if w1 > w0 and owner[w0][0] != owner[w1 - 1][0])
    # a split that walks from the 1700-row sample into the 2300-row one skips the empty sample between them
    over_empty = sum(1 for w0, w1 in rng if w1 > w0 and owner[w0] == (owner[w0][0], 0) and owner[w1 - 1] == (owner[w0][0], 2))
    print(f"[decoder cases] walk: {S} stages x {c.iters} iterations over {nsplit} gate splits: {min(per)}-{max(per)} per split; "
          f"{cross_sample} splits cross a sample boundary, {cross_iter} an iteration boundary, {over_empty} the empty sample")
    assert min(per) >= 6                      # the four-deep ring turns over in every split
    assert cross_sample >= 1 and cross_iter >= 1 and over_empty >= 1
    # the head's walk: 1024 splits over one iteration's stages -- mostly empty, none above one stage
    hper = [w1 - w0 for w0, w1 in DC.split_ranges(S, _splits()[1])]
    print(f"[decoder cases] walk: head splits with no stage: {sum(1 for k in hper if k == 0)} of {len(hper)}")
    assert sum(1 for k in hper if k == 0) > len(hper) // 2


def test_blocks_structure():
    c = DC.case("blocks")
    nsplit, nhead = _splits()
    S = sum(DC.stages_per_sample(c.counts))
    hper = [w1 - w0 for w0, w1 in DC.split_ranges(S, nhead)]
    gper = [w1 - w0 for w0, w1 in DC.split_ranges(S * c.iters, nsplit)]
    print(f"[decoder cases] blocks: {S} stages: {min(hper)}-{max(hper)} per head split ({nhead}), {min(gper)}-{max(gper)} per gate split "
          f"({nsplit}); B ceil(N / 64) = {c.B * ((c.N + 63) // 64)}")
    assert min(hper) >= 5                     # the three-deep ring turns over in every head split
    assert c.B * ((c.N + 63) // 64) >= 2048   # deflow_amd/decoder.py: the two-stage column sum (df_colsum_stage)


def test_edges_structure():
    c = DC.case("edges")
    assert c.N == 193
    for k in (1, 4, 8, 12):
        for n in (16 * k - 1, 16 * k, 16 * k + 1):
            if n <= c.N:
                assert n in c.counts, n
    assert c.counts[0] == 0 and c.counts[-1] == 0 and 0 in c.counts[1:-1]
    assert (c.H * c.W) % 32 != 0 and (c.H * c.W) % 64 != 0


@pytest.mark.parametrize("name", CASES)
def test_cell_placement(name):
    c = DC.case(name)
    ncell = c.H * c.W
    assert c.heavy
    for b, n in enumerate(c.counts):
        cells = c.cells(b)
        assert cells.numel() == n and (n == 0 or (0 <= int(cells.min()) and int(cells.max()) < ncell))
        cnt = torch.bincount(cells, minlength=ncell)
        if b in c.heavy:
            h = c.heavy[b]
            assert int(cnt[h]) == DC.HEAVY_ROWS
            near = cnt[max(0, h - DC.HEAVY_CLEAR):h + DC.HEAVY_CLEAR + 1].clone()
            near[min(h, DC.HEAVY_CLEAR)] = 0
            assert int(near.sum()) == 0                     # its neighbours in either four-cell lane group are empty
            assert all(int(cnt[k]) >= 1 for k in (0, c.W - 1, ncell - c.W, ncell - 1))
            assert int((cnt > 1).sum()) > 1                 # duplicates beyond the heavy cell
            rows = (cells == h).nonzero().squeeze(1)
            assert int(rows[-1] - rows[0]) > DC.HEAVY_ROWS - 1  # shuffled: the cell's rows are not one adjacent run
        elif n == 1:
            assert int(cells[0]) == ncell - 1               # the image's last cell (the ragged tail of the gather's last pass)


def test_segsum_ascending_is_the_sequential_sum():
    g = torch.Generator().manual_seed(1)
    rows = torch.randn(50, 4, generator=g) * torch.logspace(-3, 3, 50)[:, None]
    cell = torch.randint(0, 5, (50,), generator=g)
    got = DC.segsum_ascending(rows, cell, 7)
    for k in range(7):
        a = torch.zeros(4)
        for i in range(50):
            if int(cell[i]) == k:
                a = a + rows[i]
        assert torch.equal(got[k], a)
