"""CPU: the per-cluster rigid snap without a GPU -- tests/helpers/refine_ref.py on planted motions, the settings
of deflow_amd/refine.py and how its command splits and refuses arguments."""
import numpy as np
import pytest

from deflow_amd import refine
from helpers import refine_ref as rr


# ---- the helper ---------------------------------------------------------------------------------------------------------------------------
def test_helper_recovers_a_planted_motion_exactly():
    """noise-free flow of a yaw about an arbitrary centre plus a translation: the fit reproduces the flow of every row, in the first fit
    and after the re-weightings, whatever row is the anchor"""
    rng = np.random.default_rng(3)
    x = (rng.uniform(-1, 1, (50, 3)) * [2.0, 1.0, 0.7] + [12.0, -7.0, 0.3]).astype(np.float32)
    yaw, t = 0.21, (0.9, -1.4, 0.06)
    f = rr.rigid_motion(x, (11.0, -6.5, 0.0), yaw, t).astype(np.float32)
    lab = np.ones(50, dtype=np.int64)
    for iters in (0, 4):
        r = rr.refine_ref(x, f, lab, 50, check=False, iters=iters, min_cluster_size=50)
        assert r["table"][0, 7] == 1 and r["table"][0, 6] == 50 and r["table"][0, 4] == 1.0
        assert abs(r["table"][0, 0] - yaw) < 1e-6 and abs(r["table"][0, 3] - t[2]) < 1e-6
        assert np.abs(r["flow"] - f.astype(np.float64)).max() < 2e-6          # (f itself is rounded to fp32)
        assert r["rigid_id"].tolist() == [1] * 50 and r["moved"].all()
    # rows that do not take part keep their flow, bit for bit, and are not counted
    f2 = f.copy()
    f2[0], f2[7, 1] = np.nan, np.inf
    r = rr.refine_ref(x, f2, lab, 48, check=False, min_cluster_size=50)
    assert r["table"][0, 6] == 46 and r["anchor"][0] == 1 and r["rigid_id"][[0, 7, 48, 49]].tolist() == [0, 0, 0, 0]
    assert np.array_equal(r["flow"].astype(np.float32).view(np.int32)[~r["moved"]], f2.view(np.int32)[~r["moved"]])


def _kabsch_yaw(s, d):
    """plain least squares of d = Rz(theta) s + t by the 2 x 2 SVD, z by the mean: nothing of the helper's fit"""
    ms, md = s.mean(0), d.mean(0)
    H = (s[:, :2] - ms[:2]).T @ (d[:, :2] - md[:2])
    U, _, Vt = np.linalg.svd(H)
    R = Vt.T @ np.diag([1.0, np.linalg.det(Vt.T @ U.T)]) @ U.T
    theta = np.arctan2(R[1, 0], R[0, 0])
    t = np.array([*(md[:2] - R @ ms[:2]), md[2] - ms[2]])
    return theta, t


def test_iters_0_is_plain_least_squares():
    x, f, _, body = rr.planted_case()
    for b in (1, 2, 4):
        rows = np.nonzero(body == b)[0]
        s = x[rows].astype(np.float64) - x[rows[0]].astype(np.float64)
        d = s + f[rows].astype(np.float64)
        theta, t, _ = rr.irls(s, d, 0, 0.1)
        want_theta, want_t = _kabsch_yaw(s, d)
        assert abs(theta - want_theta) < 1e-12 and np.abs(t - want_t).max() < 1e-12


def test_planted_case_numbers():
    """DESIGN.md section 6p's planted case in float64: the mean end-point error of the input, of the plain least-squares fit applied to
    every body, and of the refinement with four re-weightings; the refined error is at most half of either"""
    x, f, truth, body = rr.planted_case()
    assert x.shape == (684, 3) and x.dtype == np.float32 and f.dtype == np.float32
    e_in = rr.epe(f, truth)
    ls = np.zeros_like(truth)
    for b in (1, 2, 3, 4):
        rows = np.nonzero(body == b)[0]
        s = x[rows].astype(np.float64) - x[rows[0]].astype(np.float64)
        theta, t, _ = rr.irls(s, s + f[rows].astype(np.float64), 0, 0.1)
        ls[rows] = rr.snap(s, theta, t)
    e_ls = rr.epe(ls, truth)
    r = rr.refine_ref(x, f, body, 684, check=False)
    e_ref = rr.epe(r["flow"], truth)
    print(f"planted case: input {e_in:.4f} m, least squares {e_ls:.4f} m, four re-weightings {e_ref:.4f} m")
    assert abs(e_in - 0.3234) < 5e-4 and abs(e_ls - 0.2487) < 5e-4 and abs(e_ref - 0.0346) < 5e-4          # the recorded figures
    assert e_ref <= 0.5 * e_in and e_ref <= 0.5 * e_ls
    tab = r["table"]
    assert tab[:4, 7].tolist() == [1, 1, 6, 1] and not tab[4:].any()
    assert ((tab[:4, 4] >= 0.72) & (tab[:4, 4] <= 0.78)).all()                 # inlier fractions at 0.2 m, clear of 0.5
    assert not tab[2, :4].any() and r["margins"][2]["static_disp"] > 0.5 and r["margins"][2]["static_yaw"] > 0.5   # body 3 is static
    for b, (yaw, t) in enumerate(rr.PLANTED_MOTION):
        if b != 2:
            assert abs(tab[b, 0] - yaw) < 5e-3
    # against the second sweep (the truth-moved rows) every snap passes, and the nearest-neighbour mean falls
    pc1 = (x.astype(np.float64) + truth).astype(np.float32)
    rc = rr.refine_ref(x, f, body, 684, pc1=pc1, count1=684)
    assert rc["table"][:4, 7].tolist() == [1, 1, 6, 1] and (rc["table"][:4, 9] < rc["table"][:4, 8]).all()
    assert np.array_equal(rc["flow"], r["flow"])
    # no second sweep: every cluster passes and the columns stay 0
    rn = rr.refine_ref(x, f, body, 684, pc1=pc1, count1=0)
    assert rn["table"][:4, 7].tolist() == [1, 1, 6, 1] and not rn["table"][:, 8:10].any()


def test_check_turns_a_worsening_snap_into_status_7():
    """a flow that is wrong for most rows of a body: the fit follows the majority and passes (d), but against the second sweep the
    snapped rows lie further from it than before, so the cluster is left alone"""
    rng = np.random.default_rng(5)
    a = (rng.uniform(-1, 1, (60, 3)) * [1.0, 1.0, 0.5] + [0.0, 0.0, 0.0]).astype(np.float32)
    f = np.tile(np.array([[1.5, 0.0, 0.0]], np.float32), (60, 1))
    pc1 = a + np.array([[-1.5, 0.0, 0.0]], np.float32)                       # the body really went the other way
    r = rr.refine_ref(a, f, np.ones(60, int), 60, pc1=pc1, count1=60, min_cluster_size=60, check_tol=0.05)
    assert r["table"][0, 7] == 1                                             # rigid in, rigid out: the snap changes nothing, so it passes
    # a fit that is accepted but lands the rows in empty space
    f2 = f.copy()
    f2[:15] = [-1.5, 0.0, 0.0]                                               # 15 rows right, 45 rows wrong: the fit follows the 45
    r2 = rr.refine_ref(a, f2, np.ones(60, int), 60, pc1=pc1, count1=60, min_cluster_size=60)
    assert r2["table"][0, 7] == 7 and r2["table"][0, 9] > r2["table"][0, 8] + 0.05
    assert np.array_equal(r2["flow"].astype(np.float32).view(np.int32), f2.view(np.int32)) and not r2["rigid_id"].any()


# ---- settings -----------------------------------------------------------------------------------------------------------------------------
def test_defaults_and_keys():
    assert refine.DEFAULTS == {"eps": 0.7, "min_points": 4, "min_cluster_size": 20, "min_rows": 8, "max_cluster_points": 8192, "iters": 4,
                               "delta": 0.1, "inlier_dist": 0.2, "min_inlier_frac": 0.5, "max_yaw": 0.35, "max_disp": 3.4,
                               "static_disp": 0.05, "static_yaw": 0.02, "check": True, "check_trunc": 2.0, "check_tol": 0.05}
    assert refine.COMMAND_KEYS == {"refine_" + k: k for k in refine.DEFAULTS}
    assert {k: v for k, v in refine.DEFAULTS.items() if k in rr.DEFAULTS} == rr.DEFAULTS      # the helper restates the same defaults
    assert refine.check_params({}) == refine.DEFAULTS
    p = refine.check_params({"iters": 2.0, "min_inlier_frac": 1.1, "check": False})
    assert p["iters"] == 2 and isinstance(p["iters"], int) and p["min_inlier_frac"] == 1.1 and p["check"] is False
    assert refine.kcap(9000, 20) == 450 and refine.kcap(7, 20) == 1
    # no line of the models' table: this is no model
    from deflow_amd import pairflow
    assert pairflow.entry("refine") is None and [e.name for e in pairflow.TABLE] == ["icpflow", "nsfp", "fastnsf", "mbnsf", "floxels"]


@pytest.mark.parametrize("bad, text", [
    ({"iters": -1}, "rigid_refine: iters must be an integer in [0, 64], got -1"),
    ({"iters": 65}, "rigid_refine: iters must be an integer in [0, 64], got 65"),
    ({"iters": 1.5}, "rigid_refine: iters must be an integer in [0, 64], got 1.5"),
    ({"min_rows": 0}, "rigid_refine: min_rows must be an integer in [1, 1073741824], got 0"),
    ({"max_cluster_points": True}, "rigid_refine: max_cluster_points must be a finite number, got True"),
    ({"delta": 0.0}, "rigid_refine: delta must be positive and finite, got 0.0"),
    ({"inlier_dist": -0.2}, "rigid_refine: inlier_dist must be positive and finite, got -0.2"),
    ({"check_trunc": float("inf")}, "rigid_refine: check_trunc must be a finite number, got inf"),
    ({"eps": float("nan")}, "rigid_refine: eps must be a finite number, got nan"),
    ({"max_yaw": -0.1}, "rigid_refine: max_yaw must be finite and >= 0, got -0.1"),
    ({"check_tol": "0.1"}, "rigid_refine: check_tol must be a finite number, got '0.1'"),
    ({"check": 1}, "rigid_refine: check must be True or False, got 1"),
])
def test_check_params_texts(bad, text):
    with pytest.raises(ValueError) as e:
        refine.check_params(bad)
    assert str(e.value) == text


def test_check_params_names_an_unknown_parameter():
    with pytest.raises(ValueError, match=r"^rigid_refine: unknown parameter 'icp_iters'; known: check, check_tol, "):
        refine.check_params({"icp_iters": 3})


# ---- the command --------------------------------------------------------------------------------------------------------------------------
def test_command_splits_its_own_keys_from_the_rest():
    own, rest = refine.split_args(["checkpoint=a.ckpt", "refine_iters=2", "dataset_path=/d", "+refine_check=false", "batch_size=2"])
    assert own == {"refine_iters": "2", "refine_check": "false"} and rest == ["checkpoint=a.ckpt", "dataset_path=/d", "batch_size=2"]
    cmd, params, rest = refine.parse_command(["save", "model=icpflow", "dataset_path=/d", "refine_iters=2", "refine_check=false", "icp_iters=3"])
    assert cmd == "save" and params == {**refine.DEFAULTS, "iters": 2, "check": False}
    assert rest == ["model=icpflow", "dataset_path=/d", "icp_iters=3", "res_name=icpflow+rigid"]        # what save would choose, + rigid
    assert refine.parse_command(["save", "checkpoint=/x/best.ckpt", "dataset_path=/d"])[2][-1] == "res_name=best+rigid"
    assert refine.parse_command(["save", "checkpoint=/x/best.ckpt", "dataset_path=/d", "res_name=mine"])[2][-1] == "res_name=mine"
    cmd, params, rest = refine.parse_command(["eval", "model=fastnsf", "val_data=synthetic", "refine_min_inlier_frac=1.1"])
    assert cmd == "eval" and params["min_inlier_frac"] == 1.1 and rest == ["model=fastnsf", "val_data=synthetic"]


def test_command_refusals():
    for argv in ([], ["vis"], ["refine_iters=2"]):
        with pytest.raises(SystemExit) as e:
            refine.parse_command(argv)
        assert str(e.value).startswith("usage: python -m deflow_amd.refine save|eval ") and "[refine_check=true]" in str(e.value)
    with pytest.raises(SystemExit) as e:
        refine.parse_command(["eval", "checkpoint=a.ckpt", "av2_mode=test", "dataset_path=/d"])
    assert "writes no leaderboard submission (av2_mode=test is out of its scope)" in str(e.value)
    with pytest.raises(SystemExit) as e:
        refine.parse_command(["save", "model=icpflow", "dataset_path=/d", "refine_itres=2"])
    assert str(e.value).startswith("unknown key 'refine_itres'; the refine_* keys: refine_eps, ")
    with pytest.raises(SystemExit) as e:
        refine.parse_command(["save", "model=icpflow", "dataset_path=/d", "refine_iters=many"])
    assert str(e.value) == "bad value for refine_iters: 'many'"
    with pytest.raises(SystemExit) as e:
        refine.parse_command(["eval", "model=icpflow", "refine_iters=65"])
    assert str(e.value) == "bad value among the refine_* keys: rigid_refine: iters must be an integer in [0, 64], got 65"
    # the wrapped command's own refusals come through: save needs its data
    with pytest.raises(SystemExit) as e:
        refine.parse_command(["save", "model=icpflow"])
    assert str(e.value).startswith("usage: python -m deflow_amd.save model=icpflow ")


def test_plain_save_still_refuses_a_refine_key():
    from deflow_amd import save
    with pytest.raises(SystemExit) as e:
        save.parse_args(["refine_iters=2", "checkpoint=a.ckpt", "dataset_path=/d"])
    assert str(e.value).startswith("unknown key 'refine_iters'; known: ")
    with pytest.raises(SystemExit) as e:
        save.main(["model=icpflow", "dataset_path=/d", "refine_iters=2"])
    assert str(e.value).startswith("unknown key 'refine_iters'; known: ")


def test_wrap_amends_the_meta_and_wraps_the_model():
    class Inner:
        point_cloud_range = [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0]
        inference_dtype = "bf16"

        def __init__(self):
            self.calls = []

        def forward_padded(self, batch):
            return {}

        def eval(self):
            self.calls.append("eval")
            return self

        def to(self, *a, **k):
            self.calls.append("to")
            return self

        def parameters(self):
            return iter((1, 2))

    w = refine.Wrap(refine.check_params({"iters": 2}))
    for before, after in (("DESIGN.md 6f, 6j (UNPINNED)", "DESIGN.md 6f, 6j, 6p (UNPINNED)"), ("DESIGN.md 6f (UNPINNED)", "DESIGN.md 6f, 6p (UNPINNED)")):
        meta = {"res_name": "x+rigid", "definition": before}
        inner = Inner()
        m = w(inner, meta)
        assert meta["definition"] == after and meta["refine"] == {**refine.DEFAULTS, "iters": 2}
        assert isinstance(m, refine.Refined) and m.model is inner and m.params["iters"] == 2
        assert m.eval() is m and m.to("cpu") is m and inner.calls == ["eval", "to"] and list(m.parameters()) == [1, 2]
        assert m.inference_dtype == "bf16" and m.point_cloud_range == inner.point_cloud_range
        with pytest.raises(AttributeError):
            m.no_such_attribute
    assert isinstance(w(Inner(), None), refine.Refined)
    with pytest.raises(TypeError, match="Refined: int has no forward_padded"):
        refine.Refined(3)
    with pytest.raises(ValueError, match="rigid_refine: unknown parameter 'depth'"):
        refine.Refined(Inner(), depth=3)


def test_ops_refuse_cpu_tensors_by_name():
    import torch
    x = torch.zeros(1, 40, 3)
    c = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(TypeError, match=r"rigid_refine: x must be a CUDA tensor \(deflow_amd has no CPU fallback\)"):
        refine.rigid_refine(x, c, x, x, c)
