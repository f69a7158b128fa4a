"""CPU: what makes every case of tests/helpers/rigid_cases.py well-posed, asserted on the INPUT with the helpers alone (never a tolerance on a
result): each case reaches the edge of csrc/rigid.hip its name says, the lattice votes are exact in both precisions, the ICP tie case's
result depends on the tie rule, no float case has a pair in the inlier band, and every accept-step case has its margin on the side it
claims.  tests/test_gpu_rigid_cases.py runs the same cases on the GPU."""
import numpy as np
import pytest

from helpers import rigid_cases as rc
from helpers import rigid_ref as rr


# ---- segments ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg_cases():
    return rc.segment_cases()


def _tiles(rows):
    return set(int(t) for t in np.asarray(rows) // rc.TILE)


def test_segments_ref_agrees_with_a_plain_loop():
    rng = np.random.default_rng(0)
    for N0, N1, Kcap in ((37, 20, 5), (1, 9, 3), (50, 1, 4)):
        labels = rng.integers(-2, Kcap + 3, N0 + N1)
        off, rows, bad = rc.segments_ref(labels, N0, Kcap)
        off2, rows2, bad2 = rc.segments_loop(labels, N0, Kcap)
        assert off.tolist() == off2 and rows.tolist() == rows2 and bad == bad2 and bad > 0
        assert off.dtype == np.int32 and rows.dtype == np.int32 and off[-1] == (rows >= 0).sum()
    c = rc.segment_cases()["bad_labels"]
    off, rows, bad = rc.segments_ref(c["labels"][1], c["N0"], c["Kcap"])
    assert (off.tolist(), rows.tolist(), bad) == rc.segments_loop(c["labels"][1], c["N0"], c["Kcap"])


def test_segment_cases_reach_their_edges(seg_cases):
    assert tuple(seg_cases) == rc.SEGMENT_CASE_NAMES
    for name, c in seg_cases.items():
        lab, N0, N1, K = c["labels"], c["N0"], c["N1"], c["Kcap"]
        assert lab.dtype == np.int32 and lab.shape[1] == N0 + N1 and N0 != N1 and 1 <= K <= N0 + N1 and N0 + N1 <= 3100, name
        off, rows, bad = rc.segments_ref(lab[0], N0, K)
        n = np.diff(off)
        # interleaved: a labelled row's successor carries another label nearly everywhere
        listed = lab[0][lab[0] > 0]
        assert (np.diff(listed) != 0).mean() > 0.4 or name == "full_middle_tile", name
        if name.startswith("kcap_"):
            assert K == int(name[5:]) and n[2 * K - 2] > 0 and n[2 * K - 1] > 0                       # the last slot, both lists
            edges = list(range(rc.CHUNK, 2 * K, rc.CHUNK))
            assert len(edges) == {127: 0, 128: 0, 129: 1, 300: 2}[K]
            for e in edges:                                                                           # both sides of every scan chunk
                assert (n[e - 2: e + 2] > 0).all() and off[e] > 0, (name, e)
        if name.startswith("n_"):
            assert N0 + N1 == int(name[2:])
        if name != "bad_labels":
            assert bad == 0, name
    assert sorted(c["N0"] + c["N1"] for k, c in seg_cases.items() if k.startswith("n_")) == [1023, 1024, 1025, 2 * 1024 + 7]
    # one list fills the whole middle tile and has nothing else
    c = seg_cases["full_middle_tile"]
    off, rows, _ = rc.segments_ref(c["labels"][0], c["N0"], c["Kcap"])
    lst = 2 * (rc.FULL_TILE_LABEL - 1) + 1
    assert rows[off[lst]: off[lst + 1]].tolist() == list(range(rc.TILE, 2 * rc.TILE)) and c["N0"] + c["N1"] > 2 * rc.TILE
    assert off[lst] - off[lst - 1] > 0                                                                # its source list is populated too
    # one list has rows in tiles 0 and 2, none in tile 1
    c = seg_cases["list_skips_tile_1"]
    off, rows, _ = rc.segments_ref(c["labels"][0], c["N0"], c["Kcap"])
    lst = 2 * (rc.SKIP_TILE_LABEL - 1)
    assert _tiles(rows[off[lst]: off[lst + 1]]) == {0, 2}
    assert sum(1 for k in range(2 * c["Kcap"]) if 1 in _tiles(rows[off[k]: off[k + 1]])) >= 5          # tile 1 is not empty
    # refine's and mbnsf's call
    c = seg_cases["n1_is_one_zero_column"]
    assert c["N1"] == 1 and c["labels"][0, -1] == 0 and (c["labels"][0] > 0).sum() > 1000
    c = seg_cases["b2_second_sample_unlabelled"]
    assert c["labels"].shape[0] == 2 and (c["labels"][0] > 0).any() and not c["labels"][1].any()
    c = seg_cases["bad_labels"]
    for b, planted in enumerate(rc.BAD_PLANTED):
        lab = c["labels"][b].astype(np.int64)
        assert ((lab == -1).sum(), (lab == c["Kcap"] + 1).sum(), (lab == rc.INT32_MIN).sum()) == planted
        assert rc.segments_ref(lab, c["N0"], c["Kcap"])[2] == sum(planted)
        bad_rows = np.nonzero((lab < 0) | (lab > c["Kcap"]))[0]
        assert (bad_rows < c["N0"]).any() and (bad_rows >= c["N0"]).any() or b == 1                   # on both sides (sample 0)


# ---- votes --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vote_a():
    return rc.vote_sample_a()


@pytest.fixture(scope="module")
def vote_b():
    return rc.vote_sample_b()


def _exact(sample, **over):
    r, q = rc.ref(sample, **over), rc.ref(sample, dtype=np.float32, **over)
    assert np.array_equal(r["hist"], q["hist"]) and np.array_equal(r["vote"], q["vote"])
    assert np.array_equal(r["table"][:, 5:8], q["table"][:, 5:8])
    return r


@pytest.mark.parametrize("vote_cap", [1024, 257, 256])
def test_vote_sample_a_is_exact_and_crosses_tiles(vote_a, vote_cap):
    s = vote_a
    assert rc.kcap_of(s) == 6 and len(s["labels"]) <= 3100
    r = _exact(s, vote_cap=vote_cap)
    assert r["R"] == 12 and r["hist"].shape == (6, 25, 25)
    st = r["table"][:, 7]
    assert st[rc.TOO_LARGE - 1] == 3 and st[rc.ONE_SIDED - 1] == 2 and st[5] == 0 and not np.isin(st[:3], (0, 2, 3)).any()
    assert not r["hist"][3:].any() and not r["vote"][3:].any() and (r["vote"][:3, 2] > 0).all()
    src, dst = rc.list_rows(s, rc.BIG)
    assert (len(src), len(dst)) == (300, 700)
    us, ud = min(300, vote_cap), min(700, vote_cap)
    if vote_cap == 1024:                                             # two and three tiles, both ragged
        assert (us - 1) // rc.CHUNK == 1 and (ud - 1) // rc.CHUNK == 2 and us % rc.CHUNK and ud % rc.CHUNK
    elif vote_cap == 257:                                            # the stride rule; the second tile holds one row
        assert us == ud == rc.CHUNK + 1 and len(set(rr._pick(src, 257))) == 257 and rr._pick(src, 257)[-1] != src[256]
    else:
        assert us == ud == rc.CHUNK
    assert 0 < r["hist"][rc.BIG - 1].sum() <= us * ud
    # NaN / inf rows at list positions 255 and 256 of both lists; at cap 1024 and 257 they are used rows
    src, dst = rc.list_rows(s, rc.NONFINITE)
    pts = np.concatenate([s["pc0s"], s["pc1"]])
    for lst in (src, dst):
        assert len(lst) == 300 and not np.isfinite(pts[lst[list(rc.NONFINITE_AT)]]).all(1).any()
        assert np.isfinite(pts[np.delete(lst, rc.NONFINITE_AT)]).all()
        if vote_cap != 256:
            assert set(lst[list(rc.NONFINITE_AT)]) & set(rr._pick(lst, vote_cap))


def test_edge_pairs_are_planted(vote_a, vote_b):
    for s, R, vbin in ((vote_a, 12, rc.VOTE_BIN), (vote_b, 64, 0.0625)):
        assert rr.vote_radius(s["params"]["max_disp"], vbin) == R
        qx, qy = rc.vote_quotients(s, rc.EDGE, 1024, vbin)
        for q, other in ((qx, qy), (qy, qx)):
            inside = np.abs(np.floor(other + 0.5)) <= R
            on, beyond, minus = ((q == v) & inside for v in (R, R + 0.5, -(R + 0.5)))
            assert on.sum() >= 10 and beyond.sum() >= 10 and minus.sum() >= 10
            assert (np.floor(q[on] + 0.5) == R).all() and (np.floor(q[beyond] + 0.5) == R + 1).all() and (np.floor(q[minus] + 0.5) == -R).all()
        r = rc.ref(s)
        h = r["hist"][rc.EDGE - 1]
        assert h[R, 2 * R] >= 10 and h[R, 0] >= 10 and h[2 * R, R] >= 10 and h[0, R] >= 10          # the outermost bins are hit


def test_vote_sample_b_radii(vote_b):
    s = vote_b
    assert rc.kcap_of(s) == 4
    r = _exact(s)
    assert r["R"] == 64 and r["hist"].shape == (4, 129, 129) and r["hist"].nbytes < 300 * 1024
    assert (r["vote"][:2, 2] > 0).all() and r["table"][2, 7] == 2 and r["table"][3, 7] == 0
    assert (4 * ((2 * 64 + 1) ** 2 + 2 * 256) + 8 * 256) > 48 * 1024                                  # bins, a target tile, the arg-max keys
    r17 = _exact(s, **rc.R17)
    assert r17["R"] == 17 and (r17["vote"][:2, 2] > 0).all()
    r0 = _exact(s, **rc.R0)
    assert r0["R"] == 0 and r0["hist"].shape == (4, 1, 1)
    qx, qy = rc.vote_quotients(s, rc.BIG, 1024, rc.VOTE_BIN)
    inside = (np.floor(qx + 0.5) == 0) & (np.floor(qy + 0.5) == 0)
    assert inside.sum() == r0["hist"][0, 0, 0] > 0 and (~inside).sum() > 0                            # pairs in the single bin and outside it
    assert r0["table"][0, 7] != 5 and r0["vote"][0].tolist() == [0, 0, int(inside.sum())]


# ---- the ICP tie ----------------------------------------------------------------------------------------------------------------------------
def test_tie_case_depends_on_the_tie_rule():
    got = {}
    for swapped in (False, True):
        s = rc.tie_sample(swapped)
        assert len(s["pc0s"]) == 40 and len(s["pc1"]) == 340 and rc.kcap_of(s) == 1 and (s["labels"] == 1).all()
        r, q = rc.ref(s), rc.ref(s, dtype=np.float32)
        assert r["vote"][0].tolist() == [0, 0, 1536] and r["runner_up"][0] < 1536
        assert r["table"][0, 0] == 0.0 and r["table"][0, 7] == 1 and r["table"][0, 4] == 1.0 and r["band_pairs"].sum() == 0
        assert r["table"][0, 1] == (-1 if swapped else 1) * rc.TIE_STEP and not r["table"][0, 2:4].any()
        own = max(np.abs(q["table"][:, :5] - r["table"][:, :5]).max(), np.abs(q["flow"] - r["flow"]).max())
        assert own == 0.0
        got[swapped] = (r["table"][0, 1], max(1e-4, 4 * own))
        # every source is equally far from its two copies, which sit in two LDS tiles; everything else is farther
        src, dst = s["pc0s"].astype(np.float64), s["pc1"].astype(np.float64)
        d2 = ((src[:, None] - dst[None]) ** 2).sum(-1)
        near = np.sort(np.argsort(d2, axis=1, kind="stable")[:, :2], axis=1)
        assert (near[:, 0] == np.arange(40)).all() and (near[:, 1] == 300 + np.arange(40)).all()
        assert near[:, 0].max() < rc.CHUNK <= near[:, 1].min()
        assert (d2[np.arange(40), near[:, 0]] == d2[np.arange(40), near[:, 1]]).all() and (np.sort(d2, axis=1)[:, 2] > 4 * rc.TIE_STEP ** 2).all()
        assert np.linalg.norm(dst[40:300, None, :2] - src[None, :, :2], axis=-1).min() >= 6.0
    assert abs(got[False][0] - got[True][0]) > 100 * max(got[False][1], got[True][1])


# ---- the accept step ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accept():
    cases = rc.accept_cases()
    assert tuple(cases) == rc.ACCEPT_CASE_NAMES
    return {k: (s, rc.ref(s), rc.ref(s, dtype=np.float32)) for k, s in cases.items()}


def _float_case_is_well_posed(s, r, q):
    assert r["band_pairs"].sum() == 0 and q["band_pairs"].sum() == 0
    voted = r["vote"][:, 2] > 0
    assert ((r["vote"][:, 2] - r["runner_up"])[voted] > r["edge_pairs"][voted]).all()               # the winning bin is fp32's too
    assert np.array_equal(q["vote"][:, :2], r["vote"][:, :2]) and np.array_equal(q["table"][:, 5:8], r["table"][:, 5:8])
    assert np.array_equal(q["rigid_id"], r["rigid_id"])
    for k in r["margins"]:                                           # no accept decision sits within 0.02 of its threshold
        assert min(abs(v) for v in r["margins"][k]) >= 0.02 and np.sign(r["margins"][k]).tolist() == np.sign(q["margins"][k]).tolist()


def test_accept_cases_have_their_margins(accept):
    for name, (s, r, q) in accept.items():
        assert rc.kcap_of(s) == 2 and (np.unique(s["labels"]) == [0, 1]).all(), name
        _float_case_is_well_posed(s, r, q)
    s, r, q = accept["icp_iters_0"]
    assert r["vote"][0, 2] > 0 and r["vote"][0, :2].any() and r["table"][0, 0] == 0 and r["table"][0, 7] == 1
    assert r["table"][0, 1:3].tolist() == (r["vote"][0, :2] * np.float64(np.float32(0.2))).tolist() and r["table"][0, 3] == 0
    s, r, q = accept["fewer_than_3_inliers"]
    for res, dt in ((r, np.float64), (q, np.float32)):
        assert rc.first_pass_inliers(s, 0, res, dt) < 3                                               # ... so in every pass
        assert res["table"][0, 7] == 4 and res["margins"][0][0] <= -0.05 and res["table"][0, 0] == 0 and res["vote"][0, 2] > 0
    assert 1 <= rc.first_pass_inliers(s, 0, r) and r["table"][0, 4] * 260 == rc.first_pass_inliers(s, 0, r)
    s, r, q = accept["yaw_over_max_yaw"]
    m = r["margins"][0]
    assert r["table"][0, 7] == 5 and r["vote"][0, 2] > 0 and m[0] >= 0.05 and m[1] <= -0.05 and m[2] >= 0.05
    s, r, q = accept["displacement_over_max_disp"]
    m = r["margins"][0]
    assert r["table"][0, 7] == 5 and r["vote"][0, 2] > 0 and m[0] >= 0.05 and m[1] >= 0.05 and m[2] <= -0.05


def test_apply_samples():
    samples = rc.apply_samples()
    want = (1, 4)
    for b, s in enumerate(samples):
        r, q = rc.ref(s), rc.ref(s, dtype=np.float32)
        _float_case_is_well_posed(s, r, q)
        assert (len(s["pc0s"]), len(s["pc1"])) == (300, 330) and rc.kcap_of(s) == 3
        assert r["table"][rc.APPLY_LABEL - 1, 7] == want[b] and r["table"][0, 7] == 1 and r["table"][2, 7] == 0
        c0 = rc.APPLY_COUNT0[b]
        lab0 = s["labels"][:300]
        assert (lab0[c0:] == rc.APPLY_LABEL).sum() >= 10 and (lab0[c0:] == 1).sum() >= 2              # labelled rows behind count0
        assert (s["nan_rows"] < c0).all() and np.isnan(s["pc0s"][s["nan_rows"]]).any(1).all() and not lab0[s["nan_rows"]].any()
        flow, rid = rc.apply_expected(r, c0)
        assert np.isfinite(flow).all() and not flow[c0:].any() and not rid[c0:].any()
        if b == 0:
            assert (rid[:c0] == rc.APPLY_LABEL).sum() >= 150 and np.abs(flow[rid == rc.APPLY_LABEL]).max() > 1.0
            assert (r["rigid_id"][c0:] == rc.APPLY_LABEL).any()                                       # count0 matters on this input
        else:
            assert not (rid == rc.APPLY_LABEL).any() and (rid == 1).any()
