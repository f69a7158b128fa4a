"""CPU: the odometry's float64 restatement (tests/helpers/reg_ref.py) against a known motion, the pose chain, the sidecar, the readers'
``pose_source``, the command's parser, and the argument checks of the three df_reg_* entries (which return before any launch)."""
import ctypes as C
import math
import os
import pickle
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi_sizes  # noqa: E402
import reg_ref  # noqa: E402


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", [False, True])
def test_restatement_recovers_the_lattice_motion(planar):
    """700 rows, three iterations from identity at max_dist 1.0: every row's nearest target is its true partner (<= 0.25 m against >= 0.35
    m), the fit is a well-conditioned least-squares problem on fp32-rounded targets.  Bound 1e-6; measured 1.4e-8 (6-DoF), 1.0e-8 (planar)."""
    T_true = reg_ref.se3_exp(reg_ref.MOTION_PLANAR if planar else reg_ref.MOTION)
    src = reg_ref.lattice(700)
    assert np.abs(src.astype(np.float64) @ T_true[:3, :3].T + T_true[:3, 3] - src).max() <= 0.25
    dst = reg_ref.moved(src, T_true)
    T, status = reg_ref.register(src, 700, dst, 700, [(1.0, 3)], planar=planar)
    err = np.abs(T - T_true).max()
    print("planar", planar, "|T - T_true|max", err)
    assert status == 0 and err <= 1e-6
    # 100 extra source rows 30 m above the cloud: beyond max_dist, weight 0
    far = reg_ref.lattice(100, seed=5) + np.array([0, 0, 30], dtype=np.float32)
    T2, status = reg_ref.register(np.concatenate((src, far)), 800, dst, 700, [(1.0, 3)], planar=planar)
    assert status == 0 and np.abs(T2 - T_true).max() <= 1e-6


def test_restatement_status_codes():
    src = reg_ref.lattice(60)
    dst = reg_ref.moved(src, np.eye(4))
    T, status = reg_ref.register(src, 60, dst, 60, [(1.0, 1)], min_inliers=61)
    assert status == 2 and np.array_equal(T, np.eye(4))
    line = np.zeros((60, 3), dtype=np.float32)          # every row at the origin: the rotation is not observable
    T, status = reg_ref.register(line, 60, line, 60, [(1.0, 1)])
    assert status == 3 and np.array_equal(T, np.eye(4))


def test_se3_exp_branches_agree():
    """the series below 1e-2 and the closed form above it meet: both against scipy-free Rodrigues in float64 at the threshold"""
    for th in (0.0, 1e-6, 0.99e-2, 1.01e-2, 0.3):
        w = np.array([0.6, -0.48, 0.64]) * th
        T = reg_ref.se3_exp(np.concatenate((w, [0.3, -0.2, 0.1])))
        R = T[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(R) - 1) < 1e-14
        if th:
            assert abs(math.acos(min(1.0, (np.trace(R) - 1) / 2)) - th) < 1e-9
    a, b = reg_ref.se3_exp([0.99999e-2, 0, 0, 1, 2, 3]), reg_ref.se3_exp([1.00001e-2, 0, 0, 1, 2, 3])
    assert np.abs(a - b).max() < 1e-6


# ---- the independent reference of df_reg_solve (tests/test_gpu_reg_solve.py) -----------------------------------------------------------
EXP_THETAS = (0.0, 1e-9, 1e-6, 1e-3, 0.0099, 0.0099999, 0.01, 0.0100001, 0.0101, 0.05, 0.3, 1.2, 3.03, 3.14159)
EXP_AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.6, -0.48, 0.64))


def test_slab_pack_round_trip():
    H, g, sw, swr, n = reg_ref.base_sums()
    S = reg_ref.pack_slab(H, g, sw, swr, n)
    assert S.shape == (32,) and S.dtype == np.float64 and S[30] == 0 and S[31] == 0
    assert S[0] == H[0, 0] and S[5] == H[0, 5] and S[6] == H[1, 1] and S[11] == H[2, 2] and S[20] == H[5, 5]      # row by row
    assert np.array_equal(S[21:27], g) and (S[27], S[28], S[29]) == (sw, swr, n) and n == 700
    H2, g2, sw2, swr2, n2 = reg_ref.unpack_slab(S)
    assert np.array_equal(H2, np.triu(H) + np.triu(H, 1).T) and np.array_equal(g2, g) and (sw2, swr2, n2) == (sw, swr, n)
    assert np.array_equal(reg_ref.pack_slab(H2, g2, sw2, swr2, n2), S)
    # split_slab: one row is the row; more rows sum to S within the bits the offsets cost, and the order of the additions shows
    assert np.array_equal(reg_ref.split_slab(S, 1), S[None])
    for nblk in (2, 3, 4, 4097):
        rows = reg_ref.split_slab(S, nblk)
        assert rows.shape == (nblk, 32) and np.all(rows[:, 30:] == 0)
        up = reg_ref.sum_rows(rows)
        assert np.abs(up - S).max() <= 2.0 ** -11 * np.abs(S).max() and np.all(np.abs(up - S) <= 2.0 ** -11 * np.abs(S))
        if nblk >= 3:
            assert not np.array_equal(up, reg_ref.sum_rows(rows[::-1]))
        if nblk >= 4:
            assert not np.array_equal(up, reg_ref.sum_rows_pairwise(rows))
    probe = np.array([2.0 ** 53, 1.0, 1.0, -2.0 ** 53])[:, None] * np.ones((1, 32))
    assert reg_ref.sum_rows(probe)[29] == 0 and reg_ref.sum_rows_pairwise(probe)[29] == 1 and reg_ref.sum_rows(probe[::-1])[29] == 2


def test_se3_exp_against_the_matrix_exponential():
    """The restated closed form / series against torch.linalg.matrix_exp of the 4 x 4 twist on the WHOLE matrix, translation column
    included, at every theta and axis of the GPU test's table and at the threshold, v = (0.3, -2, 11), and v = 0 at the two thetas where
    the GPU test has it.  Bound: 64 ulp of max(1, max|T|) = 2^-46 max(1, max|T|) = 1.6e-13 with this v.  Measured: largest difference
    3.4e-14 (theta = 3.14159).  Where the TWIST's norm is around 1e-2 -- v = 0 and theta = 0.0099 or 0.0101 -- matrix_exp itself is
    7.7e-14 and 8.6e-14 off (about a coordinate axis, where cos and sin give the exact answer and se3_exp is within 1 ulp at every
    theta; 1e-18 at 1e-3, 2e-16 at 0.05): with max|T| = 1 the reference would miss its own bound of 1.4e-14 there, so v = 0 is taken
    at theta = 0 and 0.3.  With |v| = 11 the norm is 11 at every theta and that regime is not entered."""
    worst = 0.0
    for th in EXP_THETAS:
        for ax in EXP_AXES:
            for vv in ((0.3, -2.0, 11.0),) + (((0.0, 0.0, 0.0),) if th in reg_ref.EXP_V0_THETAS else ()):
                d = np.concatenate((np.array(ax) * th, vv))
                A, Bm = reg_ref.se3_exp(d), reg_ref.se3_exp_indep(d)
                err, bound = np.abs(A - Bm).max(), 2.0 ** -46 * max(1.0, np.abs(Bm).max())
                worst = max(worst, err)
                assert err <= bound, (th, ax, vv, err, bound)
                assert np.array_equal(Bm[3], [0, 0, 0, 1])
    print("se3_exp against matrix_exp: largest difference", worst)
    for th in EXP_THETAS:                    # about x the exact answer is known: the restatement is the accurate one of the two
        T, c, s_ = reg_ref.se3_exp((th, 0, 0, 0, 0, 0)), math.cos(th), math.sin(th)
        assert np.abs(T[:3, :3] - np.array([[1, 0, 0], [0, c, -s_], [0, s_, c]])).max() <= 2.0 ** -52


def test_solve_ref_on_a_planted_step():
    """solve_hp returns the planted step, solve agrees with it, solve_ref puts the pieces together; the status rules"""
    H, _, sw, swr, n = reg_ref.base_sums()
    assert np.linalg.cond(H) <= 1e3
    delta = np.array([0.02, -0.03, 0.05, 0.3, -2.0, 11.0])
    S = reg_ref.pack_slab(H, -H @ delta, sw, swr, n)
    st, x = reg_ref.solve_hp(*reg_ref.unpack_slab(S)[:2], n, 50, False)
    assert st == 0 and x.dtype == np.longdouble and np.abs(x.astype(np.float64) - delta).max() <= 1e-12
    st64, x64 = reg_ref.solve(*reg_ref.unpack_slab(S)[:2], n, 50, False)
    assert st64 == 0 and np.abs(x64 - x.astype(np.float64)).max() <= 1e-12
    T0 = reg_ref.se3_exp((0.3, -0.2, 0.1, 1.0, 2.0, 3.0))
    st, T, log = reg_ref.solve_ref(S, 50, False, T0)
    assert st == 0 and np.abs(T - reg_ref.se3_exp(delta) @ T0).max() <= 2.0 ** -46 * np.abs(T).max()
    assert log[0] == 700 and log[1] == swr / sw
    assert abs(log[2] - np.linalg.norm(delta[:3])) <= 1e-13 and abs(log[3] - np.linalg.norm(delta[3:])) <= 1e-11
    # planar: the 4 x 4 system left after the replacement, whatever g[0], g[1] hold
    Sp = S.copy()
    Sp[21:23] = 1e6
    st, Tp, logp = reg_ref.solve_ref(Sp, 50, True, np.eye(4))
    Hs, gs = H[2:, 2:], (-H @ delta)[2:]
    xs = np.linalg.solve(Hs, -gs)
    assert st == 0 and np.abs(Tp - reg_ref.se3_exp(np.concatenate(([0, 0], xs)))).max() <= 1e-11 and abs(logp[2] - abs(xs[0])) <= 1e-13
    # statuses: T0 comes back, the last two log entries stay 0
    for kw, want in ((dict(min_inliers=701), 2), (dict(n=np.nan), 2), (dict(H55=np.inf), 3), (dict(g3=np.inf), 3), (dict(H01=np.nan), 3),
                     (dict(H00=0.0), 3)):
        Sb = S.copy()
        if "n" in kw:
            Sb[29] = kw["n"]
        if "H55" in kw:
            Sb[20] = kw["H55"]
        if "g3" in kw:
            Sb[24] = kw["g3"]
        if "H01" in kw:
            Sb[1] = kw["H01"]
        if "H00" in kw:
            Sb[0] = kw["H00"]
        st, Tb, lb = reg_ref.solve_ref(Sb, kw.get("min_inliers", 50), False, T0)
        assert st == want and Tb.tobytes() == T0.tobytes() and np.all(lb[2:] == 0), kw
        assert reg_ref.solve(*reg_ref.unpack_slab(Sb)[:2], Sb[29], kw.get("min_inliers", 50), False)[0] == want, kw
    assert reg_ref.solve_ref(np.zeros(32), 0, False, T0)[0] == 3 and reg_ref.solve_ref(np.zeros(32), 1, False, T0)[0] == 2
    Sz = S.copy()
    Sz[0] = 0.0                                          # H00 = 0: fatal in 6 DoF, replaced in the planar solve
    assert reg_ref.solve_ref(Sz, 50, True, T0)[0] == 0


# ---- chain and sidecar ------------------------------------------------------------------------------------------------------------------
def _poses(n, seed=3):
    rng = np.random.default_rng(seed)
    poses = [np.eye(4)]
    for _ in range(n - 1):
        poses.append(poses[-1] @ reg_ref.se3_exp(np.concatenate((rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.5, 0.5, 3)))))
    return poses


def test_pose_chain_reproduces_given_poses():
    from deflow_amd.odometry import chain_poses
    poses = _poses(12)
    rel = [np.linalg.inv(b) @ a for a, b in zip(poses, poses[1:])]          # sweep k into sweep k + 1's frame
    out = chain_poses(rel)
    assert len(out) == 12 and all(o.dtype == np.float64 for o in out)
    assert max(np.abs(o - p).max() for o, p in zip(out, poses)) <= 1e-12
    assert len(chain_poses([])) == 1


def test_sidecar_round_trips(tmp_path):
    from deflow_amd import odometry
    poses = {str(1000 + 7 * k): p for k, p in enumerate(_poses(5))}
    path = str(tmp_path / ("s" + odometry.SIDECAR_SUFFIX))
    odometry.write_sidecar(path, poses, {"stride": 4, "levels": (2.0, 1.0), "definition": "DESIGN.md 6r (UNPINNED)"})
    back = odometry.read_sidecar(path)
    assert sorted(back) == sorted(poses)
    for k in poses:
        assert back[k].dtype == np.float64 and back[k].shape == (4, 4) and np.array_equal(back[k], poses[k])
    with np.load(path, allow_pickle=False) as z:
        import json
        meta = json.loads(str(z["meta"]))
    assert meta["definition"] == "DESIGN.md 6r (UNPINNED)" and meta["levels"] == [2.0, 1.0]
    assert os.listdir(tmp_path) == ["s" + odometry.SIDECAR_SUFFIX]          # the temporary file was moved into place


# ---- the readers ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def scene_dir(tmp_path, golden_dir):
    """a copy of scene_a.h5 with an index of its own: nothing is ever written under tests/golden"""
    src = os.path.join(golden_dir, "av2_mini", "train")
    shutil.copy(os.path.join(src, "scene_a.h5"), tmp_path / "scene_a.h5")
    with open(os.path.join(src, "index_total.pkl"), "rb") as f:
        index = [e for e in pickle.load(f) if e[0] == "scene_a"]
    with open(tmp_path / "index_total.pkl", "wb") as f:
        pickle.dump(index, f)
    return str(tmp_path)


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and \
            a.numpy().tobytes() == b.numpy().tobytes()
    return a == b


def test_pose_source_auto_and_file_give_todays_items(golden_dir):
    from deflow_amd.data import HDF5Dataset
    from deflow_amd.h5scene import H5File
    d = os.path.join(golden_dir, "av2_mini", "train")
    auto, file_, plain = HDF5Dataset(d, pose_source="auto"), HDF5Dataset(d, pose_source="file"), HDF5Dataset(d)
    assert plain.pose_source == "auto"
    for i in (0, 3, len(auto) - 1):
        a, f, p = auto[i], file_[i], plain[i]
        assert sorted(a) == sorted(f) == sorted(p)
        assert all(_same(a[k], f[k]) and _same(a[k], p[k]) for k in a)
        with H5File(os.path.join(d, a["scene_id"] + ".h5")) as h:            # what the item held before pose_source existed
            ts = sorted(h.keys(), key=int)
            k = ts.index(str(a["timestamp"]))
            assert _same(a["pose0"], torch.from_numpy(h[ts[k]]["pose"].read()))
            assert _same(a["pose1"], torch.from_numpy(h[ts[k + 1]]["pose"].read()))
    with pytest.raises(ValueError, match="pose_source must be"):
        HDF5Dataset(d, pose_source="online")
    with pytest.raises(ValueError, match="needs a pose_sidecar"):
        HDF5Dataset(d, pose_source="sidecar", pose_sidecar="")


def test_pose_source_sidecar_returns_the_sidecars_poses(scene_dir):
    from deflow_amd import odometry
    from deflow_amd.data import HDF5Dataset, collate_fn_pad
    from deflow_amd.h5scene import H5File
    with H5File(os.path.join(scene_dir, "scene_a.h5")) as h:
        ts = sorted(h.keys(), key=int)
    poses = dict(zip(ts, _poses(len(ts), seed=9)))
    with pytest.raises(ValueError, match=r"scene_a\.pose\.npz does not exist; write it with  python -m deflow_amd\.odometry data_dir="):
        HDF5Dataset(scene_dir, pose_source="sidecar")[0]
    odometry.write_sidecar(os.path.join(scene_dir, "scene_a" + odometry.SIDECAR_SUFFIX), poses, {})
    ds, ref = HDF5Dataset(scene_dir, pose_source="sidecar"), HDF5Dataset(scene_dir)
    for i in (0, 5, len(ds) - 1):
        item, old = ds[i], ref[i]
        k = ts.index(str(item["timestamp"]))
        assert item["pose0"].dtype == torch.float64 and np.array_equal(item["pose0"].numpy(), poses[ts[k]])
        assert np.array_equal(item["pose1"].numpy(), poses[ts[k + 1]])
        assert all(_same(item[key], old[key]) for key in item if key not in ("pose0", "pose1"))
    batch = collate_fn_pad([ds[0], ds[1]])
    assert batch["pose0"].dtype == torch.float32 and batch["pose0"].shape == (2, 4, 4)
    # auto: the files hold ``pose``, so the sidecar is not looked at
    assert _same(HDF5Dataset(scene_dir, pose_source="auto")[0]["pose0"], ref[0]["pose0"])


def test_sidecar_missing_a_timestamp_raises(scene_dir):
    from deflow_amd import odometry
    from deflow_amd.data import HDF5Dataset
    from deflow_amd.h5scene import H5File
    with H5File(os.path.join(scene_dir, "scene_a.h5")) as h:
        ts = sorted(h.keys(), key=int)
    poses = dict(zip(ts, _poses(len(ts))))
    del poses[ts[1]]
    odometry.write_sidecar(os.path.join(scene_dir, "scene_a.pose.npz"), poses, {})
    ds = HDF5Dataset(scene_dir, pose_source="sidecar")
    with pytest.raises(ValueError, match=rf"has no entry for sweep {ts[1]}; write it with  python -m deflow_amd\.odometry"):
        ds[0]
    # the void map's labeller reads poses through the same helper: it fails the same way before it touches the GPU
    from deflow_amd.voidmap import label_scene
    with pytest.raises(ValueError, match=r"python -m deflow_amd\.odometry"):
        label_scene(os.path.join(scene_dir, "scene_a.h5"), pose_source="sidecar")
    with pytest.raises(ValueError, match="pose_source must be"):
        label_scene(os.path.join(scene_dir, "scene_a.h5"), pose_source="nowhere")


# ---- the commands' parsers --------------------------------------------------------------------------------------------------------------
def test_command_parser():
    from deflow_amd.odometry import CLI_DEFAULTS, parse_args
    cfg = parse_args(["data_dir=/d"])
    assert cfg == {**CLI_DEFAULTS, "data_dir": "/d"}
    assert cfg["stride"] == 4 and cfg["levels"] == [2.0, 1.0, 0.5] and cfg["iters"] == 8 and cfg["min_inliers"] == 50
    assert cfg["planar"] is False and cfg["min_range"] == 3.0 and cfg["max_range"] == 51.2 and cfg["ground_source"] == "auto"
    cfg = parse_args(["data_dir=/d", "scenes=a,b", "overwrite=true", "stride=2", "levels=1.5,0.5", "iters=3", "planar=true",
                      "ground_source=none", "init=identity", "min_range=1", "max_range=40", "cell=0.8", "min_inliers=10"])
    assert cfg["scenes"] == ["a", "b"] and cfg["overwrite"] is True and cfg["stride"] == 2 and cfg["levels"] == [1.5, 0.5]
    assert cfg["iters"] == 3 and cfg["planar"] is True and cfg["ground_source"] == "none" and cfg["init"] == "identity"
    assert (cfg["min_range"], cfg["max_range"], cfg["cell"], cfg["min_inliers"]) == (1.0, 40.0, 0.8, 10)
    for bad in (["stride=2"], ["data_dir=/d", "strid=2"], ["data_dir=/d", "stride=0"], ["data_dir=/d", "stride=1025"],
                ["data_dir=/d", "levels=1,-1"], ["data_dir=/d", "levels="], ["data_dir=/d", "levels=nan"], ["data_dir=/d", "iters=x"],
                ["data_dir=/d", "planar=maybe"], ["data_dir=/d", "ground_source=online"], ["data_dir=/d", "init=last"],
                ["data_dir=/d", "min_range=60"], ["data_dir=/d", "cell=0"], ["data_dir=/d", "xy_range=0,0,1"], ["data_dir"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_pose_source_key_of_the_other_commands():
    from deflow_amd import save, train, vis, voidmap
    assert train.split_pose_source(["lr=1e-3", "pose_source=sidecar", "epochs=1"]) == ("sidecar", ["lr=1e-3", "epochs=1"])
    assert train.split_pose_source(["lr=1e-3"]) == ("auto", ["lr=1e-3"])
    with pytest.raises(SystemExit, match="pose_source must be one of"):
        train.split_pose_source(["pose_source=online"])
    assert "pose_source" not in train.DEFAULTS                      # not a hyper-parameter: never saved with a checkpoint
    assert save.parse_args(["checkpoint=c.ckpt", "dataset_path=/d", "pose_source=sidecar"])["pose_source"] == "sidecar"
    assert save.parse_args(["checkpoint=c.ckpt", "dataset_path=/d"])["pose_source"] == "auto"
    assert vis.parse_args(["dataset_path=/d", "res_name=r", "pose_source=file"])["pose_source"] == "file"
    assert voidmap.parse_args(["data_dir=/d", "pose_source=sidecar"])["pose_source"] == "sidecar"
    for parse, argv in ((save.parse_args, ["checkpoint=c.ckpt", "dataset_path=/d"]), (vis.parse_args, ["dataset_path=/d", "res_name=r"]),
                        (voidmap.parse_args, ["data_dir=/d"])):
        with pytest.raises(SystemExit):
            parse(argv + ["pose_source=online"])


def test_register_names_the_function_and_the_argument():
    from deflow_amd.odometry import register, schedule
    x = torch.zeros(1, 8, 3)
    c = torch.full((1,), 8, dtype=torch.int32)
    with pytest.raises(TypeError, match="register: src must be a CUDA tensor"):
        register(x, c, x, c)
    with pytest.raises(ValueError, match=r"register: src \[B,Ns,3\] and dst \[B,Nd,3\] expected"):
        register(x[0], c, x, c)
    assert schedule((2.0, 1.0), 3) == [(2.0, 3), (1.0, 3)] and schedule(((1.0, 6),), 8) == [(1.0, 6)]
    for bad in ((), (0.0,), (float("inf"),), ((1.0, -1),), "ab"):
        with pytest.raises(ValueError, match="register: levels"):
            schedule(bad, 8)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deflow_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_reject_bad_arguments_without_launching(lib):
    """every check fails before the launch, so fake (aligned, never dereferenced) addresses do on a machine without a GPU"""
    P = C.c_void_p
    a = 0x10000
    inf, nan = float("inf"), float("nan")

    def acc(src_rng=a, src_sorted=a, Gs=8, dst_rng=a, dst_sorted=a, cell=1.0, G=8, B=2, Ns=300, stride=1, T=a, max_dist2=1.0, k2=0.1,
            partial=a):
        return lib.df_reg_accumulate(P(src_rng), P(src_sorted), Gs, P(dst_rng), P(dst_sorted), -4.0, -4.0, cell, G, B, Ns, stride, P(T),
                                     max_dist2, k2, P(partial), P(0), P(0), P(0), P(0), P(0))

    for name in ("src_rng", "src_sorted", "dst_rng", "dst_sorted", "T", "partial"):
        assert acc(**{name: 0}) == -3, name                          # DF_E_ARG
    assert acc(stride=0) == -3 and acc(stride=1025) == -3 and acc(stride=-1) == -3
    for v in (inf, nan, 0.0, -1.0):
        assert acc(max_dist2=v) == -3 and acc(k2=v) == -3 and acc(cell=v) == -3, v
    assert acc(B=0) == -1 and acc(B=65536) == -1 and acc(Ns=0) == -1 and acc(G=0) == -1 and acc(Gs=4097) == -1    # DF_E_SHAPE
    assert acc(B=4, Ns=1 << 28) == -1
    assert acc(src_sorted=a + 8) == -2 and acc(dst_sorted=a + 4) == -2 and acc(partial=a + 4) == -2 and acc(T=a + 4) == -2   # DF_E_ALIGN

    def solve(partial=a, B=2, nblk=2, min_inliers=50, T=a, log=a, status=a):
        return lib.df_reg_solve(P(partial), B, nblk, min_inliers, 0, P(T), P(log), P(status), P(0))

    assert solve(partial=0) == -3 and solve(log=0) == -3 and solve(status=0) == -3 and solve(min_inliers=-1) == -3
    assert solve(B=0) == -1 and solve(nblk=0) == -1 and solve(B=65536) == -1
    assert solve(partial=a + 4) == -2 and solve(T=a + 4) == -2 and solve(log=a + 2) == -2

    assert lib.df_reg_ws_bytes(3, 700) == 3 * 3 * 32 * 8 and lib.df_reg_ws_bytes(1, 256) == 256 and lib.df_reg_ws_bytes(1, 257) == 512
    assert lib.df_reg_ws_bytes(0, 700) == -1 and lib.df_reg_ws_bytes(3, 0) == -1 and lib.df_reg_ws_bytes(4, 1 << 28) == -1   # DF_E_SHAPE


def test_bindings_match_the_header(lib):
    from deflow_amd import _lib
    protos = abi_sizes.header_prototypes()
    assert sorted(_lib._SIGS) == sorted(protos)
    names = list(_lib._SIGS)
    for n in ("df_reg_ws_bytes", "df_reg_accumulate", "df_reg_solve"):
        assert names.index(n) > names.index("df_refine_apply")       # outside the range tests/helpers/abi_sizes.in_scope sizes
        assert len(_lib._SIGS[n]) == len(protos[n]) and hasattr(lib, n)
        for t, p in zip(_lib._SIGS[n], protos[n]):
            assert (t is C.c_void_p) == p.pointer, (n, p.name)
    assert [p.name for p in protos["df_reg_accumulate"] if p.nullable] == ["q_out", "idx_out", "d2_out", "w_out"]
    assert [p.name for p in protos["df_reg_solve"] if p.nullable] == ["T", "status"]
