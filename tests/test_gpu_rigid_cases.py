"""GPU: the four entry points of csrc/rigid.hip, each called on its own through deflow_amd._lib on labels written by hand, against
tests/helpers/rigid_cases.py (the row lists by a stable argsort) and tests/helpers/rigid_ref.py (all pairs, numpy).  What makes each case
well-posed, and that it reaches the edge its name says, is asserted on the input in tests/test_rigid_cases_cpu.py.

Integer results -- seg_off, seg_rows, the status word, whole histograms, votes, statuses, rigid_id -- are compared exactly; theta, t,
inlier_frac and flow within max(1e-4, 4 x the helper's own float32-vs-float64 difference on that case), the bound of test_gpu_rigid.py.
Every output buffer is pre-filled with a sentinel (0x7f7f7f7f or NaN) and every workspace with 0x7f bytes, so that an element a kernel skips
shows.  df_rigid_vote, df_rigid_icp and df_rigid_apply take their row lists from segments_ref, not from df_rigid_segments.

Measured on an MI355X (helper float32-vs-float64 / kernel against float64, table then flow; the tolerance is 1e-4 everywhere): the tie case
0 / 0 (tx = +-0.015625 exactly); icp_iters_0 1.0e-7 / 1.5e-8, 1.0e-7; fewer_than_3_inliers 1.5e-8 / 1.5e-8, 0; yaw_over_max_yaw 1.5e-6 /
7.1e-8, 0; displacement_over_max_disp 1.1e-6 / 1.4e-7, 0; apply 7.5e-7 / 1.3e-7, 3.7e-7 and 7.4e-7 / 9.8e-8, 2.7e-7."""
import numpy as np
import pytest
import torch

from helpers import rigid_cases as rc
from helpers import rigid_ref as rr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7F7F7F7F


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ints(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)


def _ws(entry, *dims):
    from deflow_amd._lib import call
    n = call(entry, *dims)
    assert n > 0
    return torch.full((n,), 0x7F, dtype=torch.uint8, device=DEV)


def run_segments(labels, N0, N1, Kcap):
    """labels [B,N] i32 numpy -> (seg_off [B,2 Kcap+1], seg_rows [B,N], status) numpy"""
    from deflow_amd._lib import call, ptr, stream
    B, N = labels.shape
    assert N == N0 + N1
    lab = _d(labels)
    seg_off, seg_rows = _ints(B, 2 * Kcap + 1), _ints(B, N)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = _ws("df_rigid_segments_ws_bytes", B, N0, N1, Kcap)
    call("df_rigid_segments", ptr(lab), B, N0, N1, Kcap, ptr(seg_off), ptr(seg_rows), ptr(status), ptr(ws), stream())
    torch.cuda.synchronize()
    assert torch.equal(lab.cpu(), torch.from_numpy(labels))                                            # the labels are an input
    return seg_off.cpu().numpy(), seg_rows.cpu().numpy(), int(status.item())


class Batch:
    """samples of rigid_cases (equal N0 and N1) on the device, with the row lists of segments_ref"""

    def __init__(self, samples, Kcap=None):
        self.samples = samples
        self.B, self.N0, self.N1 = len(samples), len(samples[0]["pc0s"]), len(samples[0]["pc1"])
        self.K = rc.kcap_of(samples[0]) if Kcap is None else Kcap
        assert all((len(s["pc0s"]), len(s["pc1"])) == (self.N0, self.N1) for s in samples)
        segs = [rc.segments_ref(s["labels"], self.N0, self.K) for s in samples]
        assert all(g[2] == 0 for g in segs)
        self.pc0s, self.pc1 = _d(np.stack([s["pc0s"] for s in samples])), _d(np.stack([s["pc1"] for s in samples]))
        self.labels = _d(np.stack([s["labels"] for s in samples]).astype(np.int32))
        self.seg_off, self.seg_rows = _d(np.stack([g[0] for g in segs])), _d(np.stack([g[1] for g in segs]))

    def params(self, over):
        p = dict(rr.DEFAULTS)
        p.update(self.samples[0]["params"])
        p.update(over)
        return p

    def vote(self, hist=True, **over):
        """-> (vote [B,K,3], hist [B,K,2R+1,2R+1]) numpy"""
        from deflow_amd._lib import call, ptr, stream
        p = self.params(over)
        R = rr.vote_radius(p["max_disp"], p["vote_bin"])
        vote = _ints(self.B, self.K, 3)
        h = _ints(self.B, self.K, 2 * R + 1, 2 * R + 1) if hist else None
        call("df_rigid_vote", ptr(self.pc0s), ptr(self.pc1), ptr(self.seg_off), ptr(self.seg_rows), self.B, self.N0, self.N1, self.K,
             p["min_side"], p["max_cluster_points"], p["vote_cap"], p["vote_bin"], R, ptr(vote), ptr(h), stream())
        torch.cuda.synchronize()
        self.vote_dev = vote
        return vote.cpu().numpy(), (h.cpu().numpy() if hist else None)

    def icp(self, **over):
        """after vote(): -> table [B,K,8] numpy"""
        from deflow_amd._lib import call, ptr, stream
        p = self.params(over)
        table = torch.full((self.B, self.K, 8), float("nan"), dtype=torch.float32, device=DEV)
        ws = _ws("df_rigid_icp_ws_bytes", self.B, self.N0, self.N1)
        call("df_rigid_icp", ptr(self.pc0s), ptr(self.pc1), ptr(self.seg_off), ptr(self.seg_rows), ptr(self.vote_dev), self.B, self.N0,
             self.N1, self.K, p["min_side"], p["max_cluster_points"], p["icp_cap"], p["icp_iters"], p["vote_bin"], p["icp_max_dist"],
             p["min_inlier_frac"], p["max_yaw"], p["max_disp"], ptr(table), ptr(ws), stream())
        torch.cuda.synchronize()
        self.table_dev = table
        return table.cpu().numpy()

    def apply(self, count0):
        """after icp(): -> (flow [B,N0,3], rigid_id [B,N0]) numpy"""
        from deflow_amd._lib import call, ptr, stream
        flow = torch.full((self.B, self.N0, 3), float("nan"), dtype=torch.float32, device=DEV)
        rid = _ints(self.B, self.N0)
        c0 = torch.tensor(list(count0), dtype=torch.int32, device=DEV)
        call("df_rigid_apply", ptr(self.pc0s), ptr(c0), ptr(self.labels), ptr(self.seg_off), ptr(self.seg_rows), ptr(self.table_dev), self.B,
             self.N0, self.N1, self.K, ptr(flow), ptr(rid), stream())
        torch.cuda.synchronize()
        return flow.cpu().numpy(), rid.cpu().numpy()


def _tolerance(r, q):
    own = max(np.abs(q["table"][:, :5] - r["table"][:, :5]).max(), np.abs(q["flow"] - r["flow"]).max())
    return own, max(1e-4, 4 * own)


# ---- 1. segments are exact --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seg_cases():
    return rc.segment_cases()


@pytest.mark.parametrize("name", rc.SEGMENT_CASE_NAMES)
def test_segments_are_exact(name, seg_cases):
    """seg_off (its last entry included), seg_rows (its -1 tail included) and the status word, element for element; two calls bit-identical"""
    c = seg_cases[name]
    want = [rc.segments_ref(lab, c["N0"], c["Kcap"]) for lab in c["labels"]]
    got = run_segments(c["labels"], c["N0"], c["N1"], c["Kcap"])
    again = run_segments(c["labels"], c["N0"], c["N1"], c["Kcap"])
    for b, (off, rows, _) in enumerate(want):
        assert np.array_equal(got[0][b], off), (name, b, np.nonzero(got[0][b] != off)[0][:8])
        assert np.array_equal(got[1][b], rows), (name, b, np.nonzero(got[1][b] != rows)[0][:8])
    bad = sum(w[2] for w in want)
    assert got[2] == bad and (bad > 0) == (name == "bad_labels")
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]) and got[2] == again[2]


# ---- 2. votes are exact across tiles, caps and radii ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vote_a():
    return Batch([rc.vote_sample_a()])


@pytest.fixture(scope="module")
def vote_b():
    return Batch([rc.vote_sample_b()])


def _vote_equals_helper(batch, **over):
    r = rc.ref(batch.samples[0], **over)
    vote, hist = batch.vote(**over)
    assert hist.shape[1:] == r["hist"].shape and np.array_equal(hist[0], r["hist"]), np.argwhere(hist[0] != r["hist"])[:8]
    assert np.array_equal(vote[0], r["vote"]), (vote[0], r["vote"])
    return r


@pytest.mark.parametrize("vote_cap", [1024, 257, 256])
def test_votes_are_exact_across_tiles_and_caps(vote_a, vote_cap):
    """a 300 x 700 cluster: two and three ragged LDS tiles at vote_cap = 1024, the stride rule with one row in the second tile at 257, one
    tile at 256; edge pairs on |q| = R and half a bin beyond it; NaN / inf rows at list positions 255 and 256; slots with status 0, 2 and 3
    get zeros"""
    r = _vote_equals_helper(vote_a, vote_cap=vote_cap)
    pre = r["table"][:, 7]
    assert (pre[3:] == (3, 2, 0)).all() and r["hist"][:3].any((1, 2)).all()


def test_vote_radius_0(vote_b):
    r = _vote_equals_helper(vote_b, **rc.R0)
    assert r["hist"].shape == (4, 1, 1) and r["vote"][0].tolist() == [0, 0, int(r["hist"][0, 0, 0])] and r["hist"][0, 0, 0] > 0


def test_vote_radius_64_between_two_radius_17_launches(vote_b):
    """R = 64 is the launch above 48 KB of dynamic LDS; the R = 17 launches before and after it still equal the helper"""
    assert _vote_equals_helper(vote_b, **rc.R17)["R"] == 17
    r = _vote_equals_helper(vote_b)
    assert r["R"] == 64 and r["hist"].shape == (4, 129, 129)
    assert _vote_equals_helper(vote_b, **rc.R17)["R"] == 17
    vote, _ = vote_b.vote(hist=False)                                                                  # hist = NULL: the same winners
    assert np.array_equal(vote[0], r["vote"])


# ---- 3. the ICP's tie rule, across two LDS tiles ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("swapped", [False, True])
def test_icp_lowest_row_wins_a_tie_across_tiles(swapped):
    """every source row is exactly as far from its copy at target position j < 256 as from the one at 300 + j: the lower position wins, so
    tx = +1/64 as written and -1/64 with the two blocks swapped"""
    s = rc.tie_sample(swapped)
    batch = Batch([s])
    r, q = rc.ref(s), rc.ref(s, dtype=np.float32)
    own, tol = _tolerance(r, q)
    vote, _ = batch.vote()
    assert np.array_equal(vote[0], r["vote"])
    table = batch.icp()[0]
    print(f"swapped {swapped}: helper fp32-vs-fp64 {own:.3e}, tolerance {tol:.3e}, table {table[0].tolist()}")
    assert np.array_equal(table[:, 5:8], r["table"][:, 5:8].astype(np.float32))
    assert r["table"][0, 1] == (-1 if swapped else 1) * rc.TIE_STEP
    assert np.abs(table[:, :5] - r["table"][:, :5]).max() <= tol


# ---- 4. the accept step and the short loops --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.ACCEPT_CASE_NAMES)
def test_accept_step_and_short_loops(name):
    s = rc.accept_cases()[name]
    batch = Batch([s])
    r, q = rc.ref(s), rc.ref(s, dtype=np.float32)
    own, tol = _tolerance(r, q)
    vote, _ = batch.vote()
    assert np.array_equal(vote[0][:, :2], r["vote"][:, :2]) and (np.abs(vote[0][:, 2] - r["vote"][:, 2]) <= r["edge_pairs"]).all()
    table = batch.icp()[0]
    flow, rid = batch.apply([batch.N0])
    err_t, err_f = np.abs(table[:, :5] - r["table"][:, :5]).max(), np.abs(flow[0] - r["flow"]).max()
    print(f"{name}: helper fp32-vs-fp64 {own:.3e}, tolerance {tol:.3e}, kernel table {err_t:.3e}, flow {err_f:.3e}, table {table[0].tolist()}")
    assert np.array_equal(table[:, 5:8], r["table"][:, 5:8].astype(np.float32))
    assert np.array_equal(rid[0], r["rigid_id"])
    assert err_t <= tol and err_f <= tol
    status = int(r["table"][0, 7])
    assert status == {"icp_iters_0": 1, "fewer_than_3_inliers": 4, "yaw_over_max_yaw": 5, "displacement_over_max_disp": 5}[name]
    if name in ("icp_iters_0", "fewer_than_3_inliers"):                                               # the vote's translation, bit for bit
        t0 = (vote[0][0, :2].astype(np.float32) * np.float32(batch.params({})["vote_bin"])).astype(np.float32)
        assert table[0, 0] == 0 and table[0, 3] == 0 and np.array_equal(table[0, 1:3].view(np.int32), t0.view(np.int32)) and t0.any()
    if status != 1:
        rows = rc.list_rows(s, 1)[0]
        assert len(rows) >= 200 and not flow[0][rows].any() and not rid[0][rows].any() and r["vote"][0, 2] > 0
    assert not table[1].any() and not flow[0][s["labels"][: batch.N0] == 0].any()                     # the empty slot, rows of no cluster


# ---- 5. apply -----------------------------------------------------------------------------------------------------------------------------
def test_apply_behind_count0_and_per_sample_status():
    """B = 2: label 2 is registered in sample 0 and rejected with status 4 in sample 1; labelled rows lie behind count0, NaN rows inside it"""
    samples = rc.apply_samples()
    batch = Batch(samples)
    vote, _ = batch.vote()
    table = batch.icp()
    flow, rid = batch.apply(rc.APPLY_COUNT0)
    assert np.array_equal(table[:, rc.APPLY_LABEL - 1, 7], (1, 4))
    assert not np.isnan(flow).any() and (rid != SENTINEL).all()                                        # every element is written
    for b, s in enumerate(samples):
        r, q = rc.ref(s), rc.ref(s, dtype=np.float32)
        own, tol = _tolerance(r, q)
        c0 = rc.APPLY_COUNT0[b]
        want_flow, want_rid = rc.apply_expected(r, c0)
        assert np.array_equal(vote[b][:, :2], r["vote"][:, :2])
        assert np.array_equal(table[b][:, 5:8], r["table"][:, 5:8].astype(np.float32))
        err_t, err_f = np.abs(table[b][:, :5] - r["table"][:, :5]).max(), np.abs(flow[b] - want_flow).max()
        print(f"sample {b}: helper fp32-vs-fp64 {own:.3e}, tolerance {tol:.3e}, kernel table {err_t:.3e}, flow {err_f:.3e}")
        assert np.array_equal(rid[b], want_rid)
        assert err_t <= tol and err_f <= tol
        assert np.array_equal(np.isfinite(flow[b]), np.isfinite(want_flow)) and np.isfinite(flow[b]).all()
        assert not flow[b][c0:].any() and not rid[b][c0:].any()                                        # behind count0: exactly zero
        assert not flow[b][s["nan_rows"]].any() and not rid[b][s["nan_rows"]].any()
        assert not flow[b][want_rid == 0].any()
    assert (rid[0] == rc.APPLY_LABEL).any() and not (rid[1] == rc.APPLY_LABEL).any() and (rid[1] == 1).any()
