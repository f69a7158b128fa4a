"""GPU: df_reg_solve (csrc/register.hip) on its own, on slabs written by hand, against a reference that shares no
formula with it: ``reg_ref.solve_ref`` = the Cholesky solve in np.longdouble, then torch.linalg.matrix_exp of the 4 x 4 twist in float64.
End-to-end registration cannot see an error in the exponential (ICP is a fixed-point iteration: as delta -> 0 the update is the identity
whatever A, B, C are, so a wrong one only slows convergence), and its lattice motions never leave the series branch; here every branch,
status, the pivot threshold, ``planar``, ``T = NULL``, the order of the sum over slab rows and the largest batch are run directly.

Base problem: H of ``reg_ref.base_sums()`` (cond 268); a wanted step delta is planted as g = -H delta.  Tolerance of every T comparison:
tol = max(2^-46 max(1, max|T_ref|), 4 own), own = max|se3_exp(reg_ref.solve(..)) T0 - T_ref| -- the helper's float64 pipeline against
solve_ref's on the same slab; 4 x is the project's rule (test_gpu_rigid.py), 64 ulp about the number of float64 roundings on the longest
path from the slab to an entry of T at this conditioning.  ``log`` is compared in fp32 within 2 ulp of the float64 value.  Every case
prints own, tol and the kernel's error.

Measured on an MI355X, the largest over each test's cases: exponential sweep own 2.3e-13, tol 1.0e-12, kernel error 2.3e-13 (at most
0.25 tol: the kernel and the float64 helper differ from the reference by the same amount, i.e. what is left is the reference's side);
statuses, the well-conditioned status-0 slabs: own 5.3e-15, kernel error 5.3e-15 against tol >= 1.3e-13 (the two 2e-9-pivot slabs,
status only: 1.4e-10 and 3.1e-12); planar: own 8.9e-16, kernel error 4.4e-16 against tol 1.6e-14."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import reg_ref  # noqa: E402

pytestmark = pytest.mark.gpu

ULP64 = 2.0 ** -46                                    # 64 ulp of 1.0
MIN_INLIERS = 50
ARBITRARY = reg_ref.se3_exp((0.3, -0.2, 0.1, 1.0, 2.0, 3.0))
FAR = reg_ref.se3_exp((-0.4, 0.25, 2.0, 0.0, 0.0, 0.0))
FAR[:3, 3] = (50.0, -50.0, 50.0)                      # a pose with 50 m translations
T0S = (np.eye(4), ARBITRARY, FAR)
AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.6, -0.48, 0.64))
THETAS = (0.0, 1e-9, 1e-3, 0.0099, 0.0101, 0.05, 0.3, 1.2, 3.03)
V = (0.3, -2.0, 11.0)
DELTA = np.array([0.02, -0.03, 0.05, 0.3, -2.0, 11.0])             # the step the status, order and NULL tests plant


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def base():
    H, g0, sw, swr, n = reg_ref.base_sums()
    cond = np.linalg.cond(H)
    print("base problem: cond(H)", cond, "diag", np.diag(H).tolist(), "n", n)
    assert cond <= 1e3 and n == 700                    # a condition on the INPUT
    return H, g0, sw, swr, n


def planted(base, delta, n=None, H=None):
    """the slab row whose solution is delta"""
    H0, _, sw, swr, n0 = base
    H = H0 if H is None else H
    return reg_ref.pack_slab(H, -H @ np.asarray(delta, dtype=np.float64), sw, swr, n0 if n is None else n)


def run_solve(dev, slab, min_inliers, planar, T0=None, status="buffer"):
    """one df_reg_solve.  slab [B,nblk,32] f64, T0 [B,4,4] f64 or None (T = NULL); status "buffer": prefilled with 77, None: NULL
    -> (T [B,4,4] or None, log [B,4] f32, status [B] i32 or None), numpy"""
    from deflow_amd._lib import call, ptr, stream
    slab = np.ascontiguousarray(slab, dtype=np.float64)
    B, nblk = slab.shape[:2]
    assert slab.shape == (B, nblk, 32)
    partial = torch.from_numpy(slab).to(dev)
    T = None if T0 is None else torch.from_numpy(np.ascontiguousarray(T0, dtype=np.float64).reshape(B, 16)).to(dev)
    log = torch.full((B, 4), float("nan"), dtype=torch.float32, device=dev)
    st = None if status is None else torch.full((B,), 77, dtype=torch.int32, device=dev)
    call("df_reg_solve", ptr(partial), B, nblk, int(min_inliers), int(planar), ptr(T), ptr(log), ptr(st), stream())
    torch.cuda.synchronize()
    assert torch.equal(partial.cpu(), torch.from_numpy(slab)) or np.isnan(slab).any()          # the slab is an input
    return (None if T is None else T.cpu().numpy().reshape(B, 4, 4), log.cpu().numpy(), None if st is None else st.cpu().numpy())


def reference(S, min_inliers, planar, T0):
    """-> (status, T_ref, log_ref, own, tol) of one summed slab row"""
    status, T_ref, log_ref = reg_ref.solve_ref(S, min_inliers, planar, T0)
    own = 0.0
    if status == 0:
        H, g, _, _, n = reg_ref.unpack_slab(S)
        st64, d64 = reg_ref.solve(H, g, n, min_inliers, planar)
        assert st64 == 0
        own = float(np.abs(reg_ref.se3_exp(d64) @ T0 - T_ref).max())
    return status, T_ref, log_ref, own, max(ULP64 * max(1.0, float(np.abs(T_ref).max())), 4.0 * own)


def check_log(log, log_ref, tol=0.0):
    """fp32, within 2 ulp of the float64 value (NaN where it is NaN).  tol: the case's tolerance on T, added for |omega| and |v| only --
    they are norms of the SOLVED step, which is uncertain by the solve's own error: where a component is planted as 0, what comes out is
    that error (1e-16 .. 1e-18), of which no ulp can be asked to agree.  At a planted norm it is 1e-6 of the two ulp."""
    for k in range(4):
        want = np.float32(log_ref[k])
        if np.isnan(want):
            assert np.isnan(log[k]), (k, log, log_ref)
        else:
            slack = 2.0 * np.float64(np.spacing(np.abs(want))) + (tol if k >= 2 else 0.0)
            assert abs(np.float64(log[k]) - np.float64(want)) <= slack, (k, log, log_ref)


# ---- a. the exponential ------------------------------------------------------------------------------------------------------------------
def sweep_cases():
    return [(th, ax, (0.0, 0.0, 0.0) if th in reg_ref.EXP_V0_THETAS else V) for th in THETAS for ax in AXES]


@pytest.fixture(scope="module")
def sweep(dev, base):
    """the exponential sweep's launch (B = 36, nblk = 1), shared with the limits test"""
    cases = sweep_cases()
    slab = np.stack([planted(base, np.concatenate((np.array(ax) * th, v))) for th, ax, v in cases])[:, None, :]
    T0 = np.stack([T0S[c % 3] for c in range(len(cases))])
    T, log, status = run_solve(dev, slab, MIN_INLIERS, 0, T0)
    return dict(cases=cases, slab=slab, T0=T0, T=T, log=log, status=status)


def test_exponential_sweep(sweep):
    """Thetas 0 .. 3.03 about x, y, z and (0.6, -0.48, 0.64), v = (0.3, -2, 11) (0 at theta = 0 and 0.3), T0 cycling through identity, an
    arbitrary pose and one with 50 m translations: status 0, log[2] = theta, the bottom row exactly (0, 0, 0, 1), T within tol of
    solve_ref; 20 cases take the closed form, 16 the series.
    What this cannot see: the theta^6 terms of the series -- below theta = 1e-2 they are under 1e-12 / 5040 of their coefficient, less
    than one ulp of A, B, C, so dropping them changes no bit that a 64 ulp bound can hold; and matrix_exp's own error (reg_ref.se3_exp_indep).
    Measured: largest own 2.3e-13 (theta = 0.0099 about z on the 50 m pose), largest tol 1.0e-12, largest kernel error 2.3e-13; the floor of
    64 ulp governs 35 of the 36 cases and the error is at most a quarter of tol."""
    cases, T, log, status = sweep["cases"], sweep["T"], sweep["log"], sweep["status"]
    assert status.tolist() == [0] * len(cases)
    worst = dict(own=0.0, tol=0.0, err=0.0, ratio=0.0)
    for c, (th, ax, v) in enumerate(cases):
        st, T_ref, log_ref, own, tol = reference(sweep["slab"][c, 0], MIN_INLIERS, False, sweep["T0"][c])
        err = float(np.abs(T[c] - T_ref).max())
        print(f"case {c} theta {th} axis {ax} v {v} T0 {c % 3}: own {own:.3e} tol {tol:.3e} err {err:.3e} log {log[c].tolist()}")
        assert st == 0 and abs(log_ref[2] - th) <= 1e-12 * max(th, 1e-3)
        assert np.array_equal(T[c, 3], [0.0, 0.0, 0.0, 1.0])
        check_log(log[c], log_ref, tol)
        assert err <= tol, (c, th, ax, err, tol)
        for k in worst:
            worst[k] = max(worst[k], dict(own=own, tol=tol, err=err, ratio=err / tol)[k])
    print("exponential sweep, largest:", worst)
    assert int((log[:, 2] >= 1e-2).sum()) >= 20 and int((log[:, 2] < 1e-2).sum()) >= 12          # both branches really ran


# ---- b. statuses -------------------------------------------------------------------------------------------------------------------------
def status_slabs(base):
    """-> slabs [12,32], ill-conditioned flags, the table [(sample, min_inliers, planar, status)]"""
    H = base[0]
    dmax = float(np.diag(H).max())
    L = np.linalg.cholesky(H)

    def with_pivot(row, ratio):
        Lp = L.copy()
        Lp[row, row] = np.sqrt(ratio * dmax)
        return Lp @ Lp.T

    def edited(col, value):
        S = planted(base, DELTA, n=MIN_INLIERS)
        S[col] = value
        return S

    slabs = [
        planted(base, DELTA, n=MIN_INLIERS),                       # 0  n == min_inliers
        planted(base, DELTA, n=MIN_INLIERS - 1),                   # 1  n == min_inliers - 1
        planted(base, DELTA, n=np.nan),                            # 2  n = NaN
        np.zeros(32),                                              # 3  all zero
        planted(base, DELTA, n=MIN_INLIERS, H=with_pivot(5, 0.5e-9)),   # 4  last pivot at 0.5e-9 dmax
        planted(base, DELTA, n=MIN_INLIERS, H=with_pivot(5, 2e-9)),     # 5  last pivot at 2e-9 dmax
        planted(base, DELTA, n=MIN_INLIERS, H=with_pivot(0, 2e-9)),     # 6  a 2e-9 pivot in row 0
        edited(0, 0.0),                                            # 7  H[0][0] = 0
        edited(0, 0.0),                                            # 8  the same, for the planar run
        edited(10, np.nan),                                        # 9  NaN in H[1][5]
        edited(25, np.inf),                                        # 10 +inf in g[4]
        edited(20, np.inf),                                        # 11 H[5][5] = +inf
    ]
    ill = [False] * 12
    ill[5] = ill[6] = True
    table = [(0, MIN_INLIERS, 0, 0), (1, MIN_INLIERS, 0, 2), (2, MIN_INLIERS, 0, 2), (3, 0, 0, 3), (4, MIN_INLIERS, 0, 3),
             (5, MIN_INLIERS, 0, 0), (6, MIN_INLIERS, 0, 0), (7, MIN_INLIERS, 0, 3), (8, MIN_INLIERS, 1, 0), (9, MIN_INLIERS, 0, 3),
             (10, MIN_INLIERS, 0, 3), (11, MIN_INLIERS, 0, 3)]
    return np.stack(slabs), ill, table


def test_statuses(dev, base):
    """The issue's twelve slabs as ONE batch, launched under each of the three settings its table names -- (min_inliers 50, 6 DoF), (0, 6
    DoF), (50, planar) -- because min_inliers and planar belong to a launch, not to a sample.  Every status of every launch is held
    against solve_ref's (the long-double elimination), the table's own entries against its literal values.  Status 2 / 3: T == T0 bit
    for bit (T0 carries a -0.0 and arbitrary mantissas), log[2:] == 0.  Status 0: the bottom row, finiteness, and -- except on the two
    slabs built with a 2e-9 pivot, whose condition number is 1e9 -- T within tol.  Every sample alone (B = 1) gives the batch's bytes.
    An input condition: no pivot ratio of any (slab, setting) lies in [0.9e-9, 1.1e-9] (rounding moves it by ~1e-7 relative)."""
    slabs, ill, table = status_slabs(base)
    nb = len(slabs)
    assert nb == 12 and np.isnan(reg_ref.unpack_slab(slabs[9])[0][[1, 5], [5, 1]]).all() and np.isposinf(reg_ref.unpack_slab(slabs[10])[1][4])
    T0 = np.stack([reg_ref.se3_exp_indep((0.3 + 0.1 * b, -0.2, 0.1 * b - 0.5, 1.0 + b, 2.0, 3.0 - b)) for b in range(nb)])
    T0[::2, 0, 3] = -0.0
    assert len({t.tobytes() for t in T0}) == nb and np.all(T0[:, 3] == [0, 0, 0, 1]) and np.signbit(T0[0, 0, 3])
    for b in (4, 5, 6):                                     # the pivots are where they were planted
        r = reg_ref.pivot_ratio(reg_ref.unpack_slab(slabs[b])[0])
        assert abs(r / (0.5e-9 if b == 4 else 2e-9) - 1) <= 1e-4, (b, r)
    seen = set()
    for min_inliers, planar in ((MIN_INLIERS, 0), (0, 0), (MIN_INLIERS, 1)):
        T, log, status = run_solve(dev, slabs[:, None, :], min_inliers, planar, T0)
        for b in range(nb):
            H = reg_ref.unpack_slab(slabs[b])[0]
            r = reg_ref.pivot_ratio(H, bool(planar))
            assert r is None or not 0.9e-9 <= r <= 1.1e-9, (b, planar, r)
            st, T_ref, log_ref, own, tol = reference(slabs[b], min_inliers, bool(planar), T0[b])
            err = float(np.abs(T[b] - T_ref).max()) if st == 0 else 0.0
            print(f"min_inliers {min_inliers} planar {planar} sample {b}: status {status[b]} (ref {st}) pivot ratio {r} own {own:.3e} "
                  f"tol {tol:.3e} err {err:.3e} log {log[b].tolist()}")
            assert status[b] == st, (b, min_inliers, planar, status[b], st)
            if (b, min_inliers, planar, st) in table:
                seen.add(b)
            assert not any(e[:3] == (b, min_inliers, planar) and e[3] != status[b] for e in table), (b, status[b])
            assert not np.isnan(T[b]).any()
            if st != 0:
                assert T[b].tobytes() == T0[b].tobytes()
                assert log[b, 2] == 0 and log[b, 3] == 0
                check_log(log[b], log_ref)
            else:
                assert np.isfinite(T[b]).all() and np.array_equal(T[b, 3], [0.0, 0.0, 0.0, 1.0])
                if not ill[b]:
                    check_log(log[b], log_ref, tol)
                    assert err <= tol, (b, min_inliers, planar, err, tol)
            Ta, la, sa = run_solve(dev, slabs[b:b + 1, None, :], min_inliers, planar, T0[b:b + 1])
            assert Ta.tobytes() == T[b].tobytes() and la.tobytes() == log[b].tobytes() and sa[0] == status[b]
    assert seen == set(range(nb))                          # every row of the table was met with its literal status


# ---- c. planar ---------------------------------------------------------------------------------------------------------------------------
def test_planar_discards_the_tilt_terms(dev, base):
    """A step planted with omega_x, omega_y = +-0.2 and g[0], g[1] = +-1e6, from a tilted T0 and from identity: the result is
    solve_ref(planar=True), which solves the 4 x 4 system left after the header's replacement; log[2] = |omega_z|; from identity the
    rotation stays about z exactly."""
    S = planted(base, (0.2, -0.2, 0.03, 0.1, -0.05, 0.02))
    S[21] += 1e6
    S[22] -= 1e6
    T0 = np.stack((reg_ref.se3_exp_indep((0.2, -0.15, 0.4, 3.0, -2.0, 1.0)), np.eye(4)))
    T, log, status = run_solve(dev, np.stack((S, S))[:, None, :], MIN_INLIERS, 1, T0)
    H, g, _, _, n = reg_ref.unpack_slab(S)
    st, delta = reg_ref.solve_hp(H, g, n, MIN_INLIERS, True)
    assert st == 0 and delta[0] == 0 and delta[1] == 0 and abs(float(delta[2])) > 1e-3
    for b in range(2):
        st, T_ref, log_ref, own, tol = reference(S, MIN_INLIERS, True, T0[b])
        err = float(np.abs(T[b] - T_ref).max())
        print(f"planar sample {b}: own {own:.3e} tol {tol:.3e} err {err:.3e} log {log[b].tolist()} omega_z {float(delta[2])}")
        assert status[b] == 0 and st == 0 and err <= tol
        check_log(log[b], log_ref, tol)
        assert abs(np.float64(log[b, 2]) - abs(float(delta[2]))) <= 2.0 * np.spacing(np.float32(abs(float(delta[2]))))
        assert np.array_equal(T[b, 3], [0.0, 0.0, 0.0, 1.0])
    assert np.all(T[1, 2, :2] == 0) and np.all(T[1, :2, 2] == 0) and T[1, 2, 2] == 1
    # the same slab in 6 DoF takes the tilt terms: the two runs differ where they must
    T6, _, s6 = run_solve(dev, np.stack((S, S))[:, None, :], MIN_INLIERS, 0, T0)
    assert s6.tolist() == [0, 0] and np.abs(T6[1, 2, :2]).max() > 1e-3


# ---- d. the order of the sum over slab rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk", [1, 2, 3, 4, 4097])
def test_slab_rows_are_added_in_ascending_order(dev, base, nblk):
    """split_slab spreads each sample's row over nblk rows with cancelling 2^40-scaled offsets: ascending sequential float64 addition
    gives one value, descending and pairwise addition others (asserted on the input).  T, log and status must be bit-identical to the
    nblk = 1 call on the row summed by numpy's left-to-right float64 loop."""
    rows = np.stack((reg_ref.split_slab(planted(base, DELTA), nblk, seed=0),
                     reg_ref.split_slab(planted(base, (-0.4, 0.1, 0.2, 1.0, 1.0, -1.0)), nblk, seed=1)))
    summed = np.stack([reg_ref.sum_rows(r) for r in rows])
    for b in range(2):
        if nblk >= 3:
            assert not np.array_equal(summed[b, :29], reg_ref.sum_rows(rows[b, ::-1])[:29])
        if nblk >= 4:
            assert not np.array_equal(summed[b, :29], reg_ref.sum_rows_pairwise(rows[b])[:29])
    T0 = np.stack((np.eye(4), ARBITRARY))
    T, log, status = run_solve(dev, rows, MIN_INLIERS, 0, T0)
    T1, log1, status1 = run_solve(dev, summed[:, None, :], MIN_INLIERS, 0, T0)
    print("nblk", nblk, "log", log.tolist(), "log of the summed row", log1.tolist())
    assert status.tolist() == [0, 0] and status1.tolist() == [0, 0]
    assert T.tobytes() == T1.tobytes() and log.tobytes() == log1.tobytes()


def test_inlier_column_is_added_in_ascending_order(dev):
    """column 29 = (2^53, 1, 1, -2^53), T = NULL, min_inliers = 0: ascending addition gives 0, pairwise 1, descending 2"""
    rows = np.zeros((1, 4, 32))
    rows[0, :, 29] = (2.0 ** 53, 1.0, 1.0, -2.0 ** 53)
    assert reg_ref.sum_rows(rows[0])[29] == 0 and reg_ref.sum_rows_pairwise(rows[0])[29] == 1 and reg_ref.sum_rows(rows[0, ::-1])[29] == 2
    _, log, _ = run_solve(dev, rows, 0, 0, None, status=None)
    print("log", log.tolist())
    assert log[0, 0] == 0.0 and np.all(log[0, 1:] == 0)


# ---- e. T = NULL -------------------------------------------------------------------------------------------------------------------------
def test_null_T_writes_the_log_only(dev, base):
    """T = NULL with status = NULL and with a status buffer, which must keep its 77s: log = (n, swr / sw, 0, 0), a mean of 0 at sw = 0;
    nothing is solved, so a slab that would give status 2 or 3 gives the same two numbers"""
    H, g0, sw, swr, n = base
    slabs = np.stack((reg_ref.pack_slab(H, g0, sw, swr, n), reg_ref.pack_slab(H, g0, 0.0, 5.0, 3), np.zeros(32),
                      reg_ref.pack_slab(H * np.nan, g0, 2.0, 0.5, 1e6)))
    rows = np.stack([reg_ref.split_slab(s, 2, scale=0.0) for s in slabs])
    want = np.array([[n, swr / sw, 0, 0], [3, 0, 0, 0], [0, 0, 0, 0], [1e6, 0.25, 0, 0]])
    for min_inliers in (MIN_INLIERS, 0):
        _, log_a, none = run_solve(dev, rows, min_inliers, 0, None, status=None)
        _, log_b, st = run_solve(dev, rows, min_inliers, 1, None, status="buffer")
        print("T = NULL: log", log_a.tolist())
        assert none is None and st.tolist() == [77] * 4 and log_a.tobytes() == log_b.tobytes()
        for b in range(4):
            S = reg_ref.sum_rows(rows[b])
            check_log(log_a[b], [S[29], S[28] / S[27] if S[27] > 0 else 0.0, 0.0, 0.0])
            check_log(log_a[b], want[b])
            assert log_a[b, 2] == 0 and log_a[b, 3] == 0


# ---- f. limits ---------------------------------------------------------------------------------------------------------------------------
def test_largest_batch(dev, sweep):
    """B = 65535 (the entry's limit, a 16 MB slab), sample b = case b % 36 of the exponential sweep: every status 0, every sample's T and
    log the bytes of the small batch (64 samples spread over the range one by one, then all of them)"""
    B, nc = 65535, len(sweep["cases"])
    pick = np.arange(B) % nc
    T, log, status = run_solve(dev, sweep["slab"][pick], MIN_INLIERS, 0, sweep["T0"][pick])
    assert status.shape == (B,) and np.all(status == 0)
    for b in np.linspace(0, B - 1, 64).astype(np.int64):
        assert T[b].tobytes() == sweep["T"][pick[b]].tobytes() and log[b].tobytes() == sweep["log"][pick[b]].tobytes(), b
    assert T.tobytes() == sweep["T"][pick].tobytes() and log.tobytes() == sweep["log"][pick].tobytes()
