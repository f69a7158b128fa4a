"""CPU: the nearest-first eviction of the local map (UNPINNED) -- the restatement of tests/helpers/map_evict_ref.py
("the rings that fit, then a budget") against the other statement of the definition ("the first cap kept candidates under the order
(ring, sorted position), emitted in sorted position") written with numpy's lexsort, the ABI rows of df_map_compact_near, its argument
errors, the wrappers' and the command's errors, and the conditions of the loop scene under overflow that
tests/test_gpu_localmap_evict.py registers on the GPU, on the float64 reference alone.

The loop scene under overflow: map_ref's loop scene (17 sweeps of 489 rows, levels ((1.0, 6), (0.5, 6)), map voxel 0.5 m, K = 1) at a
capacity every update overflows.  Measured on the reference, evict="near": seed 3, capacity 450: smallest nearest / second-nearest
margin 1.27e-4 m, every status 0, every update overflows (by 39, then by 206 .. 241 rows), closing pose off the truth by 3.2e-4,
intermediate poses by 2.6e-3.  Seed 2 (map_ref.LOOP_SEED), capacity 500: margin 3.9e-5, which is why this scene does not take it; seed
8, capacity 650: 1.07e-4.  evict="order" on the same inputs: closing pose 1.2e-4 (seed 3), 5.4e-8 (seed 2), 6.3e-5 (seed 8) -- on this
scene nearest-first is NOT more accurate than the sorted-order cut: the closing sweep is a copy of sweep 0, and in a scene 1.4 m across
the sorted-order cut happens never to evict sweep 0's rows.  The scene shows that the loop works under eviction and matches its
definition, not that poses improve; whether nearest-first helps on real sweeps is unmeasured."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import map_evict_ref  # noqa: E402
import map_ref  # noqa: E402


# ---- the restatement against the lexsort statement --------------------------------------------------------------------------------------
def first_cap_by_ring(key, keep, drop, cap, W):
    """numpy, no dict: the kept candidates in sorted order, the first cap of them under (ring, sorted position), back in sorted position
    -> (surviving candidates, ring of every kept candidate)"""
    S = 2 * W + 1
    rows = np.flatnonzero((key < drop) & (keep > 0))
    kept = rows[np.lexsort((rows, key[rows]))]
    ring = np.maximum(np.abs(key[kept] % S - W), np.abs(key[kept] // S % S - W))
    first = np.lexsort((np.arange(len(kept)), ring))[:cap]
    return kept[np.sort(first)], ring


def random_case(rng, W, n, cap_rule):
    S = 2 * W + 1
    spread = rng.choice((1, 2, W + 1))                                   # some cases crowd the inner rings
    d = np.clip(np.rint(rng.normal(W, spread, size=(n, 2))).astype(np.int64), -2, S + 1)
    inside = ((d >= 0) & (d < S)).all(axis=1)
    key = np.where(inside, d[:, 1] * S + d[:, 0], S * S)
    keep = ((rng.uniform(size=n) < 0.7) & inside).astype(np.int32)
    cand = rng.normal(size=(n, 3))
    return cand, key, keep, cap_rule(int(keep.sum()))


@pytest.mark.parametrize("seed", range(4))
def test_restatement_agrees_with_the_lexsort_statement(seed):
    rng = np.random.default_rng(seed)
    seen = {"fits": 0, "one": 0, "budget0": 0, "R0": 0, "cases": 0}
    rules = (lambda k: k + 3, lambda k: k, lambda k: max(k - 1, 1), lambda k: max(k // 2, 1), lambda k: max(k // 7, 1), lambda k: 1)
    for trial in range(150):
        W = int(rng.choice((1, 2, 5, 8)))
        n = int(rng.integers(5, 120))
        cand, key, keep, cap = random_case(rng, W, n, rules[trial % len(rules)])
        drop = (2 * W + 1) ** 2
        out, cnt, stat, cut = map_evict_ref.compact_near(cand, key, keep, drop, cap, W)
        want, ring = first_cap_by_ring(key, keep, drop, cap, W)
        kept = len(ring)
        assert cnt == min(kept, cap) == len(want) and stat[1] == kept and stat[3] == max(0, kept - cap)
        assert np.array_equal(out[:cnt].view(np.int64), cand[want].view(np.int64)) and np.isnan(out[cnt:]).all()
        base = map_ref.compact(cand, key, keep, drop, cap)
        assert stat == base[2] and cnt == base[1]                     # stat keeps df_map_compact's four meanings
        if kept <= cap:
            assert cut == (W + 1, 0) and np.array_equal(out.view(np.int64), base[0].view(np.int64))
            seen["fits"] += 1
        else:
            R, budget = cut
            h = np.bincount(ring, minlength=W + 1)
            assert 0 <= R <= W and h[:R].sum() <= cap and 0 <= budget == cap - h[:R].sum() < h[R]
            assert R == W or h[:R + 1].sum() > cap
            seen["one"] += kept == cap + 1
            seen["budget0"] += budget == 0
            seen["R0"] += R == 0
        seen["cases"] += 1
    print(seen)
    assert seen["cases"] == 150 and all(seen[k] >= 3 for k in ("fits", "one", "budget0", "R0")), seen


def test_restatement_on_hand_made_cuts():
    W, S = 3, 7
    cols = [(3, 3)] * 4 + [(2, 3), (4, 4), (3, 2)] + [(1, 1), (5, 3), (3, 5), (1, 4)] + [(0, 0), (6, 2)]      # rings 0 x4, 1 x3, 2 x4, 3 x2
    key = np.array([dy * S + dx for dx, dy in cols], dtype=np.int64)
    keep = np.ones(len(key), dtype=np.int32)
    cand = np.arange(3 * len(key), dtype=np.float64).reshape(-1, 3)
    order = map_ref.sorted_order(key, S * S)
    ring = [map_evict_ref.ring_of(key[c], W) for c in order]

    def rows(cap):
        out, cnt, stat, cut = map_evict_ref.compact_near(cand, key, keep, S * S, cap, W)
        return [int(r[0]) // 3 for r in out[:cnt]], cut, stat

    assert rows(13) == ([int(c) for c in order], (W + 1, 0), (13, 13, 0, 0))          # kept == cap: nothing goes
    got, cut, stat = rows(12)                                          # cap + 1 = kept: the last row of the outermost ring goes
    last_outer = [c for c, r in zip(order, ring) if r == 3][-1]
    assert cut == (3, 1) and got == [c for c in order if c != last_outer] and stat[3] == 1
    got, cut, _ = rows(11)                                             # the inner rings sum to exactly cap
    assert cut == (3, 0) and got == [c for c, r in zip(order, ring) if r < 3]
    got, cut, _ = rows(7)
    assert cut == (2, 0) and got == [c for c, r in zip(order, ring) if r < 2]
    got, cut, _ = rows(9)                                              # two of ring 2, the first two in sorted order
    part = [c for c, r in zip(order, ring) if r == 2][:2]
    assert cut == (2, 2) and got == [c for c, r in zip(order, ring) if r < 2 or c in part]
    got, cut, _ = rows(3)                                              # R = 0: the anchor column alone overflows
    assert cut == (0, 3) and got == [0, 1, 2]


# ---- the ABI rows -----------------------------------------------------------------------------------------------------------------------
def test_bindings_of_the_near_entries_match_the_header():
    import abi_sizes
    from deflow_amd import _lib
    protos = abi_sizes.header_prototypes()
    names = list(_lib._SIGS)
    at = names.index("df_map_near_ws_bytes")
    assert names[at - 1] == "df_map_drop" and names[at + 1:at + 3] == ["df_map_compact_near", "df_reg_ws_bytes"]      # where 6u put its four
    assert [p.name for p in protos["df_map_near_ws_bytes"]] == ["B", "cap", "N", "W"]
    assert [p.name for p in protos["df_map_compact_near"]] == ["cand", "key", "idx_sorted", "cell_rng", "keep", "B", "cap", "N", "W", "map_out",
                                                               "count_out", "stat", "cut", "ws", "stream"]
    for n in ("df_map_near_ws_bytes", "df_map_compact_near"):
        assert len(_lib._SIGS[n]) == len(protos[n])
        for t, p in zip(_lib._SIGS[n], protos[n]):
            assert (t is _lib.P) == p.pointer and not p.nullable, (n, p.name)
    assert [p.name for p in protos["df_map_compact_near"] if p.const] == ["cand", "key", "idx_sorted", "cell_rng", "keep"]
    assert "df_map_near_ws_bytes" in _lib._RAW and _lib._RESTYPE["df_map_near_ws_bytes"] is _lib.C.c_int64
    assert "df_map_compact_near" not in _lib._RAW


def test_near_entry_rejects_bad_arguments_without_launching():
    """every check fails before the launch: fake (aligned, never dereferenced) addresses do on a machine without a GPU"""
    import ctypes as C
    from deflow_amd import _lib, build
    build.build()
    lib = _lib.load()
    P, a = C.c_void_p, 0x10000
    names = ["cand", "key", "idx_sorted", "cell_rng", "keep", "map_out", "count_out", "stat", "cut", "ws"]

    def near(B=2, cap=700, N=600, W=8, **ptrs):
        p = {k: a for k in names}
        p["map_out"] = 2 * a
        p.update(ptrs)
        return lib.df_map_compact_near(P(p["cand"]), P(p["key"]), P(p["idx_sorted"]), P(p["cell_rng"]), P(p["keep"]), B, cap, N, W,
                                       P(p["map_out"]), P(p["count_out"]), P(p["stat"]), P(p["cut"]), P(p["ws"]), P(0))

    for k in names:                                                    # none is nullable: cut and key included
        assert near(**{k: 0}) == -3, k
    assert near(map_out=a) == -3                                       # map_out == cand
    assert near(cand=a + 4) == -2 and near(map_out=2 * a + 4) == -2 and near(ws=a + 2) == -2
    assert near(W=2048) == -1 and near(W=0) == -1 and near(B=0) == -1 and near(B=65536) == -1 and near(cap=0) == -1 and near(N=0) == -1
    assert near(B=2, cap=2 ** 29, N=1) == -1 and near(B=65535, W=64) == -1                          # B n, B S S >= 2^30
    q = lambda *v: _lib.call("df_map_near_ws_bytes", *v)                # noqa: E731
    assert q(3, 700, 600, 8) == 4 * 3 * (9 + 4 * 6) and q(1, 700, 600, 2047) == 4 * (2048 + 4 * 6) and q(1, 1, 1, 1) == 4 * (2 + 4)
    assert q(0, 700, 600, 8) == -1 and q(3, 700, 600, 2048) == -1 and q(3, 700, 0, 8) == -1 and q(3, 700, 600, 0) == -1


# ---- the wrappers and the command --------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_evict_arguments_before_the_gpu():
    from deflow_amd.localmap import LocalMap
    from deflow_amd.odometry import register_sweeps
    with pytest.raises(ValueError, match="LocalMap: evict must be 'order' or 'near', got 'far'"):
        LocalMap(1, 8, voxel=0.5, max_per_voxel=1, max_range=5.0, device="cpu", evict="far")
    with pytest.raises(TypeError, match="device must be a CUDA device"):
        LocalMap(1, 8, voxel=0.5, max_per_voxel=1, max_range=5.0, device="cpu", evict="near")
    with pytest.raises(ValueError, match="register_sweeps: map_evict must be 'order' or 'near', got 'far'"):
        register_sweeps([np.zeros((4, 3))], target="map", map_evict="far")
    with pytest.raises(ValueError, match="map_evict='near' needs target='map'"):
        register_sweeps([np.zeros((4, 3))], map_evict="near")
    with pytest.raises(TypeError, match="device must be a CUDA device"):
        register_sweeps([np.zeros((4, 3))], target="map", map_evict="near", device="cpu")


def test_command_parser_takes_the_evict_key():
    from deflow_amd.odometry import CLI_DEFAULTS, MAP_CARVE_DEFAULTS, MAP_DEFAULTS, MAP_EVICT_DEFAULTS, USAGE, parse_args
    assert MAP_EVICT_DEFAULTS == {"map_evict": "order"} and "map_evict" not in MAP_DEFAULTS and "map_evict" not in MAP_CARVE_DEFAULTS
    assert parse_args(["data_dir=/d"])["map_evict"] == "order" and CLI_DEFAULTS["map_evict"] == "order"
    cfg = parse_args(["data_dir=/d", "target=map", "map_evict=near"])
    assert cfg["map_evict"] == "near"
    assert {k: v for k, v in cfg.items() if k not in ("data_dir", "target", "map_evict")} == \
        {k: v for k, v in CLI_DEFAULTS.items() if k not in ("data_dir", "target", "map_evict")}
    assert parse_args(["data_dir=/d", "target=map", "map_evict=order"])["map_evict"] == "order"
    assert parse_args(["data_dir=/d", "map_evict=order"])["target"] == "scan"
    for bad in (["map_evict=far"], ["map_evict="], ["map_evict=near"], ["map_evict=near", "target=scan"]):
        with pytest.raises(SystemExit):
            parse_args(["data_dir=/d", *bad])
    with pytest.raises(SystemExit, match="map_evict=near needs target=map"):
        parse_args(["data_dir=/d", "map_evict=near", "target=scan"])
    assert "[map_evict=order|near]" in USAGE


# ---- the loop scene under overflow, on the reference alone -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    return map_ref.loop_scene(map_evict_ref.EVICT_SEED, nodes=map_ref.LOOP_NODES)


def run(scene, evict):
    return map_evict_ref.register_sweeps_map(scene[0], map_ref.LOOP["levels"], voxel=map_ref.LOOP["voxel"], K=1, cap=map_evict_ref.EVICT_CAP,
                                             W=map_ref.LOOP_W, evict=evict, gaps=True)


def test_loop_scene_under_overflow_holds_the_condition_on_the_reference(scene):
    sweeps, truth = scene
    r = run(scene, "near")
    overflow = [m[2][3] for m in r["maps"]]
    closing = np.abs(r["poses"][-1] - truth[-1]).max()
    mid = max(np.abs(P - T).max() for P, T in zip(r["poses"][1:-1], truth[1:-1]))
    print("near: gap", min(r["gap"]), "overflow", overflow, "cuts", r["cuts"], "closing", closing, "intermediate", mid)
    assert len(sweeps) == 17 and all(len(s) == int(map_ref.LOOP["frac"] * map_ref.LOOP_NODES) for s in sweeps)
    assert r["status"] == [0] * 16 and min(overflow) > 0 and all(m[1] == map_evict_ref.EVICT_CAP for m in r["maps"])
    assert len(r["gap"]) == 16 and min(r["gap"]) >= 1e-4               # the condition the GPU comparison at 1e-4 rests on
    assert all(0 < R < map_ref.LOOP_W for R, _ in r["cuts"])
    assert closing <= 1e-2 and mid <= 1e-2                             # the loop works under eviction; no more is claimed


def test_loop_scene_makes_no_accuracy_claim_for_nearest_first(scene):
    """reported; the one assertion is that the reference does NOT show nearest-first better by a factor of 3 (it shows it no better at all:
    this file's docstring), so nothing may be claimed for it"""
    truth = scene[1]
    near, order = run(scene, "near"), run(scene, "order")
    cn, co = np.abs(near["poses"][-1] - truth[-1]).max(), np.abs(order["poses"][-1] - truth[-1]).max()
    print("closing pose off the truth: near", cn, "order", co, "order's gap", min(order["gap"]))
    assert order["status"] == [0] * 16 and not (co >= 3.0 * cn)
