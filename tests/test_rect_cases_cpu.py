"""CPU: the conditions that make tests/test_gpu_rect_grids.py and the census runs D / E meaningful, decided without a GPU.

  * the oracle accepts every model-sized case in the order grid_feature_size = [H, W] = [ny, nx] (and rejects the swapped range);
  * every sample of every cloud keeps at least half of its finite rows and loses at least 5 % of them to the range -- the cloud
    overfills the short axis, so rows leave on one axis only and the kept index lists depend on which axis the engine calls H;
  * the library's host-side selection queries answer, per case and encoder stage, what tests/helpers/rect_cases.py SELECTION says
    (which kernel forms a case reaches), the statistic tile is 64 rows at stage 3 of 64x96 / 96x64, and 40x72 with B = 2 breaks the
    training tile rule while every training case keeps it.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rect_cases as RC  # noqa: E402

MODEL_CASES = [n for n, c in RC.CASES.items() if c.oracle]
KEEP_MIN, LOSE_MIN = 0.5, 0.05


def test_ranges_are_the_grids_at_02m_in_ny_nx_order():
    from deflow_amd.train import grid_from
    for c in RC.CASES.values():
        assert grid_from(c.cfg) == c.grid, c.name
        assert c.H % 8 == 0 and c.W % 8 == 0 and c.H != c.W
    assert RC.case("64x96").point_cloud_range == [-9.6, -6.4, -3, 9.6, 6.4, 3]
    assert RC.case("320x512").point_cloud_range == [-51.2, -32, -3, 51.2, 32, 3]
    assert RC.case("192x256").point_cloud_range == [-25.6, -19.2, -3, 25.6, 19.2, 3]


@pytest.mark.parametrize("name", MODEL_CASES)
def test_oracle_runs_and_the_range_cuts_one_axis(name):
    c = RC.case(name)
    batch = RC.make_batch(c)
    ref = RC.oracle(c, 1, decoder_option="gru", num_iters=2).eval()
    with torch.no_grad():
        res = ref(batch)
    finite = int(torch.isfinite(batch["pc0"][0]).all(1).sum())
    assert finite == c.N - int(c.N * 0.02)
    long_is_x = c.W > c.H
    for b in range(c.B):
        assert tuple(res["flow"][b].shape) == (len(res["pc0_valid_point_idxes"][b]), 3) and bool(torch.isfinite(res["flow"][b]).all())
        for cloud in ("pc0", "pc1"):
            kept = len(res[f"{cloud}_valid_point_idxes"][b])
            print(f"[rect cases] {name} sample {b} {cloud}: kept {kept} of {finite} finite rows")
            assert kept >= KEEP_MIN * finite, (name, b, cloud, kept, finite)
            assert kept <= (1.0 - LOSE_MIN) * finite, (name, b, cloud, kept, finite)
        # the rows that left did so on the short axis (or in z): no kept point lies outside the short half-extent, and the cloud
        # itself reaches past it
        p = batch["pc1"][b]
        p = p[torch.isfinite(p).all(1)]
        r = c.point_cloud_range
        short_half, short = (r[4], p[:, 1]) if long_is_x else (r[3], p[:, 0])
        assert float((short.abs() > short_half).float().mean()) >= LOSE_MIN
        kept_pts = res["pc1_points_lst"][b]
        assert float(kept_pts[:, 1 if long_is_x else 0].abs().max()) <= short_half


def test_oracle_rejects_the_swapped_range():
    c = RC.case("64x96")
    from oracle import ref_torch as O
    r = c.point_cloud_range
    swapped = dict(c.cfg, point_cloud_range=[r[1], r[0], r[2], r[4], r[3], r[5]])
    ref = O.DeFlow(**swapped, decoder_option="linear").eval()
    with pytest.raises((IndexError, RuntimeError, AssertionError)), torch.no_grad():
        ref(RC.make_batch(c))


@pytest.mark.parametrize("key", sorted(RC.SELECTION), ids=lambda k: f"{k[0]}-stage{k[1]}")
def test_library_selects_the_forms_the_case_was_built_for(key):
    name, k = key
    got = RC.selection(RC.case(name), k)
    print(f"[rect cases] {name} stage {k}: tile_m, h2p (fwd, dgrad, wgrad), w16 (fwd+stats, dgrad), x3 = {got}")
    assert got == RC.SELECTION[key]


def test_rectangular_census_shape_selects_what_the_square_one_does():
    """320x512 at B = 16 answers all nine queries per stage as configs[2]'s 512 x 512 at B = 16 does"""
    sq = RC.Case("512x512", 512, 512, 16, 80000, 0, "configs[2]", oracle=False)
    for k in (1, 2, 3):
        assert RC.selection(RC.case("320x512"), k) == RC.selection(sq, k), k


@pytest.mark.parametrize("name", ["64x96", "96x64"])
def test_stage3_statistic_tile_is_64_rows_and_straddles_images(name):
    c = RC.case(name)
    tile_m = RC.selection(c, 3)[0]
    h, w = c.stage_hw(3)
    assert tile_m == 64 and c.rows_pg(3) % tile_m == 0 and (h * w) % tile_m != 0


def test_training_tile_rule():
    from deflow_amd.unet import check_tile_rule
    c = RC.case("40x72")
    assert c.rows_pg(3) == 90
    with pytest.raises(ValueError, match=r"B = 2, H = 40, W = 72.*multiple of df_conv2d_tile_m.*k = 1, 2, 3"):
        check_tile_rule(c.B, c.H, c.W)
    for name in ("64x96", "96x64", "96x256", "256x96", "320x512", "192x256"):
        t = RC.case(name)
        check_tile_rule(t.B, t.H, t.W)
