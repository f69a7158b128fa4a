"""Hand-labelled cases that pin csrc/rigid.hip stage by stage (tests/test_gpu_rigid_cases.py runs them on the GPU, tests/test_rigid_cases_cpu.py
asserts on the INPUT that each case reaches the edge its name says), and the little reference code tests/helpers/rigid_ref.py lacks: the row
lists of df_rigid_segments by a stable argsort.  Nothing here is shared with rigid.hip: no tiles, no scans, no ranks.

Every builder is seeded and returns plain numpy.  A *sample* is dict(pc0s [N0,3] f32, pc1 [N1,3] f32, labels [N0+N1] i32 of the concatenation,
params: the keyword arguments of rigid_ref.rigid_ref for it); labels are written by hand, min_cluster_size only sets the number of slots
Kcap = (N0 + N1) // min_cluster_size, as in deflow_amd.rigid.kcap."""
import numpy as np

from helpers import rigid_ref as rr

TILE = 1024               # rows per tile of the scatter pass
CHUNK = 256               # counters per pass of the scan, rows per LDS tile of the vote and of the ICP
INT32_MIN = -2 ** 31


# ---- df_rigid_segments ----------------------------------------------------------------------------------------------------------------------
def segments_ref(labels, N0, Kcap):
    """one sample: labels [N] -> (seg_off [2 Kcap + 1] i32, seg_rows [N] i32, bad).  List 2 (label - 1) + (row >= N0) of every row with a label
    in [1, Kcap], rows of one list in ascending order (a stable sort on the list key); rows of no list are left out, the tail of seg_rows is
    -1; bad = the number of rows whose label is neither 0 nor in [1, Kcap]"""
    labels = np.asarray(labels).astype(np.int64)
    N = labels.shape[0]
    listed = (labels >= 1) & (labels <= Kcap)
    key = np.where(listed, 2 * (labels - 1) + (np.arange(N) >= N0), 2 * Kcap)
    order = np.argsort(key, kind="stable")
    n = int(listed.sum())
    seg_rows = np.full(N, -1, dtype=np.int32)
    seg_rows[:n] = order[:n]
    seg_off = np.zeros(2 * Kcap + 1, dtype=np.int32)
    seg_off[1:] = np.cumsum(np.bincount(key[listed], minlength=2 * Kcap)[: 2 * Kcap])
    return seg_off, seg_rows, int(((labels != 0) & ~listed).sum())


def segments_loop(labels, N0, Kcap):
    """the same by a plain Python loop over the rows (what segments_ref is checked against)"""
    lists = [[] for _ in range(2 * Kcap)]
    bad = 0
    for i, l in enumerate(int(v) for v in labels):
        if 1 <= l <= Kcap:
            lists[2 * (l - 1) + (1 if i >= N0 else 0)].append(i)
        elif l != 0:
            bad += 1
    off, rows = [0], []
    for lst in lists:
        rows += lst
        off.append(len(rows))
    return off, rows + [-1] * (len(labels) - len(rows)), bad


def _spread(rng, slots, rows, least=2):
    """{label: count}: about `rows` rows over the slots, at least `least` each"""
    slots = list(slots)
    extra = rng.multinomial(max(rows - least * len(slots), 0), np.ones(len(slots)) / len(slots))
    return {s + 1: least + int(e) for s, e in zip(slots, extra)}


def _shuffled(rng, n, counts):
    """n labels: counts[label] rows of every label, the rest 0, interleaved"""
    lab = np.zeros(n, dtype=np.int64)
    at = 0
    for l, c in counts.items():
        lab[at: at + c] = l
        at += c
    assert at <= n
    return rng.permutation(lab)


def _interleaved(rng, N0, N1, slots, fill=0.85):
    return np.concatenate([_shuffled(rng, N0, _spread(rng, slots, int(fill * N0))), _shuffled(rng, N1, _spread(rng, slots, int(fill * N1)))])


def chunk_edge_slots(Kcap):
    """the slots whose lists sit on both sides of every boundary between two 256-entry chunks of the 2 Kcap counters"""
    out = []
    for c in range(CHUNK, 2 * Kcap, CHUNK):
        out += [c // 2 - 1, c // 2]
    return out


def _kcap_case(Kcap, seed):
    rng = np.random.default_rng(seed)
    slots = sorted(set([0, 5, Kcap // 3, Kcap - 1] + chunk_edge_slots(Kcap) + [int(v) for v in rng.integers(0, Kcap, 6)]))
    return {"labels": _interleaved(rng, 700, 500, slots)[None], "N0": 700, "N1": 500, "Kcap": Kcap}


def _n_case(N0, N1, seed, Kcap=40):
    rng = np.random.default_rng(seed)
    slots = sorted(set([0, Kcap - 1] + [int(v) for v in rng.integers(0, Kcap, 14)]))
    return {"labels": _interleaved(rng, N0, N1, slots)[None], "N0": N0, "N1": N1, "Kcap": Kcap}


FULL_TILE_LABEL = 7       # full_middle_tile: the target list of this label is rows 1024 .. 2047 and nothing else
SKIP_TILE_LABEL = 5       # list_skips_tile_1: the source list of this label has rows in tiles 0 and 2 and none in tile 1


def _full_middle_tile():
    rng = np.random.default_rng(31)
    N0, N1, Kcap = 1000, 2 * TILE + 31, 30
    others = [s for s in range(0, Kcap, 2) if s + 1 != FULL_TILE_LABEL]
    lab = np.zeros(N0 + N1, dtype=np.int64)
    lab[:N0] = _shuffled(rng, N0, _spread(rng, others + [FULL_TILE_LABEL - 1], 850))
    rest = np.concatenate([np.arange(N0, TILE), np.arange(2 * TILE, N0 + N1)])
    lab[rest] = _shuffled(rng, len(rest), _spread(rng, others, int(0.85 * len(rest))))
    lab[TILE: 2 * TILE] = FULL_TILE_LABEL
    return {"labels": lab[None], "N0": N0, "N1": N1, "Kcap": Kcap}


def _list_skips_tile_1():
    rng = np.random.default_rng(32)
    N0, N1, Kcap = 2500, 579, 30
    others = [s for s in range(0, Kcap, 3) if s + 1 != SKIP_TILE_LABEL]
    lab = _interleaved(rng, N0, N1, others + [SKIP_TILE_LABEL - 1])
    lab[TILE: 2 * TILE] = _shuffled(rng, TILE, _spread(rng, others, 870))
    return {"labels": lab[None], "N0": N0, "N1": N1, "Kcap": Kcap}


def _n1_is_one_zero_column():
    rng = np.random.default_rng(33)
    N0, Kcap = 1500, 75
    lab = np.concatenate([_shuffled(rng, N0, _spread(rng, [0, 3, 17, 40, 41, 74], 1300)), [0]])
    return {"labels": lab[None], "N0": N0, "N1": 1, "Kcap": Kcap}


def _b2_second_sample_unlabelled():
    c = _n_case(600, 423, 34)
    c["labels"] = np.concatenate([c["labels"], np.zeros_like(c["labels"])])
    return c


BAD_PLANTED = ((3, 2, 1), (2, 1, 2))      # per sample: rows with label -1, Kcap + 1, INT32_MIN


def _bad_labels():
    rng = np.random.default_rng(35)
    N0, N1, Kcap = 600, 500, 40
    labs = []
    for n_bad in BAD_PLANTED:
        lab = _interleaved(rng, N0, N1, [0, 1, 9, 20, 38, 39])
        rows = rng.permutation(N0 + N1)[: sum(n_bad)]
        lab[rows] = np.repeat([-1, Kcap + 1, INT32_MIN], n_bad)
        labs.append(lab)
    return {"labels": np.stack(labs), "N0": N0, "N1": N1, "Kcap": Kcap}


def segment_cases():
    """name -> dict(labels [B,N] i32, N0, N1, Kcap); every case has interleaved labels"""
    cases = {f"kcap_{k}": _kcap_case(k, 20 + i) for i, k in enumerate((127, 128, 129, 300))}
    for i, (n0, n1) in enumerate(((600, 423), (500, 524), (513, 512), (1200, 2 * TILE + 7 - 1200))):
        cases[f"n_{n0 + n1}"] = _n_case(n0, n1, 40 + i)
    cases["full_middle_tile"] = _full_middle_tile()
    cases["list_skips_tile_1"] = _list_skips_tile_1()
    cases["n1_is_one_zero_column"] = _n1_is_one_zero_column()
    cases["b2_second_sample_unlabelled"] = _b2_second_sample_unlabelled()
    cases["bad_labels"] = _bad_labels()
    for c in cases.values():
        c["labels"] = np.ascontiguousarray(c["labels"], dtype=np.int32)
    return cases


SEGMENT_CASE_NAMES = ("kcap_127", "kcap_128", "kcap_129", "kcap_300", "n_1023", "n_1024", "n_1025", "n_2055", "full_middle_tile",
                      "list_skips_tile_1", "n1_is_one_zero_column", "b2_second_sample_unlabelled", "bad_labels")


# ---- samples with labels by hand -------------------------------------------------------------------------------------------------------
def hand_sample(rng, objects, noise0=0, noise1=0, shuffle=True):
    """objects: list of (src [n,3], dst [m,3]); object i gets label i + 1 on all of its rows.  noise rows (label 0) lie on the lattice 200 m
    away.  Rows are interleaved inside each sweep.  -> dict(pc0s, pc1, labels)"""
    far = lambda n: rr._lat(rng, n, (200.0, 200.0, 0.0), (230.0, 230.0, 2.0))
    src = np.concatenate([np.asarray(o[0], dtype=np.float32).reshape(-1, 3) for o in objects] + [far(noise0)])
    dst = np.concatenate([np.asarray(o[1], dtype=np.float32).reshape(-1, 3) for o in objects] + [far(noise1)])
    l0 = np.concatenate([np.full(len(o[0]), i + 1) for i, o in enumerate(objects)] + [np.zeros(noise0, dtype=np.int64)])
    l1 = np.concatenate([np.full(len(o[1]), i + 1) for i, o in enumerate(objects)] + [np.zeros(noise1, dtype=np.int64)])
    if shuffle:
        p0, p1 = rng.permutation(len(src)), rng.permutation(len(dst))
        src, l0, dst, l1 = src[p0], l0[p0], dst[p1], l1[p1]
    return {"pc0s": np.ascontiguousarray(src), "pc1": np.ascontiguousarray(dst), "labels": np.concatenate([l0, l1]).astype(np.int32)}


def kcap_of(sample):
    return max(len(sample["labels"]) // int(sample["params"]["min_cluster_size"]), 1)


def list_rows(sample, label):
    """(source rows, target rows) of a label, ascending: its two lists"""
    rows = np.nonzero(sample["labels"] == label)[0]
    n0 = len(sample["pc0s"])
    return rows[rows < n0], rows[rows >= n0]


def ref(sample, dtype=np.float64, **over):
    p = dict(sample["params"])
    p.update(over)
    with np.errstate(invalid="ignore"):
        return rr.rigid_ref(sample["pc0s"], sample["pc1"], sample["labels"], dtype=dtype, **p)


# ---- the vote on a lattice -------------------------------------------------------------------------------------------------------------
VOTE_BIN = 0.25
BIG, EDGE, NONFINITE, TOO_LARGE, ONE_SIDED = 1, 2, 3, 4, 5          # labels of vote_sample_a (slot 6 stays empty)
NONFINITE_AT = (255, 256)                                        # list positions: the last row of the first LDS tile, the first of the second


def _lat_pair(rng, centre, n0, n1, half=0.6):
    """n0 source and n1 target rows on the lattice around `centre`, the targets' box moved by a lattice vector"""
    c = np.asarray(centre, dtype=np.float64)
    e = np.array([half, half, 0.3])
    shift = np.array([26.0, -18.0, 0.0]) / rr.LATTICE
    return rr._lat(rng, n0, c - e, c + e), rr._lat(rng, n1, c - e + shift, c + e + shift)


def edge_offsets(R, vote_bin):
    """the three planted source-to-target offsets: on |q| = R (counted, in the outermost bin), half a bin beyond it (rounds to R + 1: not
    counted), and minus that (floor(q + 0.5) = -R: counted)"""
    return R * vote_bin, (R + 0.5) * vote_bin, -(R + 0.5) * vote_bin


def _edge_object(rng, centre, R, vote_bin):
    """10 sources in a 9 cm box; every one of them has a target at each of the three offsets, in x and in y"""
    c = np.asarray(centre, dtype=np.float64)
    src = rr._lat(rng, 10, c, c + 0.09)
    on, beyond, minus = (np.float32(v) for v in edge_offsets(R, vote_bin))
    dst = []
    for axis in (0, 1):
        for off in (on, beyond, minus):
            d = src.copy()
            d[:, axis] += off
            dst.append(d)
    return src, np.concatenate(dst)


def vote_sample_a():
    """six slots: a 300 x 700 cluster (two and three LDS tiles, both ragged), the edge pairs for R = 12, a 300 x 300 cluster with NaN / inf
    rows at list positions 255 and 256 of both lists, a 600 x 600 cluster over max_cluster_points = 1100 (status 3), a one-sided one
    (status 2) and an empty slot.  For df_rigid_vote only: a non-finite TARGET row inside a cluster is outside what DBSCAN ever labels, and
    past the vote the helper's np.argmin takes a NaN distance for the nearest one where the kernel's `<` skips it"""
    rng = np.random.default_rng(51)
    params = {"vote_bin": VOTE_BIN, "max_disp": 3.0, "max_cluster_points": 1100, "icp_iters": 0}
    R = rr.vote_radius(params["max_disp"], VOTE_BIN)
    objects = [_lat_pair(rng, (0.0, 0.0, 0.0), 300, 700), _edge_object(rng, (20.0, 0.0, 0.0), R, VOTE_BIN),
               _lat_pair(rng, (40.0, 0.0, 0.0), 300, 300), _lat_pair(rng, (60.0, 0.0, 0.0), 600, 600),
               (rr._lat(rng, 20, (80.0, 0.0, 0.0), (80.5, 0.5, 0.5)), np.zeros((0, 3), np.float32))]
    s = hand_sample(rng, objects, noise0=51, noise1=40)
    src, dst = list_rows(s, NONFINITE)
    n0 = len(s["pc0s"])
    s["pc0s"][src[NONFINITE_AT[0]]] = (np.nan, 1.0, 0.0)
    s["pc0s"][src[NONFINITE_AT[1]]] = (np.inf, 0.0, 0.0)
    s["pc1"][dst[NONFINITE_AT[0]] - n0] = (0.0, -np.inf, 0.0)
    s["pc1"][dst[NONFINITE_AT[1]] - n0] = (np.nan, np.nan, np.nan)
    params["min_cluster_size"] = len(s["labels"]) // 6
    s["params"] = params
    return s


def vote_sample_b():
    """four slots for the R = 64 launch (vote_bin = 1/16, max_disp = 4: a histogram of [4,129,129]): the 300 x 700 cluster, the edge pairs
    for R = 64, a one-sided cluster and an empty slot"""
    rng = np.random.default_rng(52)
    params = {"vote_bin": 0.0625, "max_disp": 4.0, "icp_iters": 0}
    objects = [_lat_pair(rng, (0.0, 0.0, 0.0), 300, 700), _edge_object(rng, (20.0, 0.0, 0.0), 64, 0.0625),
               (np.zeros((0, 3), np.float32), rr._lat(rng, 20, (80.0, 0.0, 0.0), (80.5, 0.5, 0.5)))]
    s = hand_sample(rng, objects, noise0=30, noise1=21)
    params["min_cluster_size"] = len(s["labels"]) // 4
    s["params"] = params
    return s


R17 = {"vote_bin": VOTE_BIN, "max_disp": 4.25}        # the launch before and after the R = 64 one
R0 = {"vote_bin": VOTE_BIN, "max_disp": 0.0}


def vote_quotients(sample, label, vote_cap, vote_bin):
    """(qx, qy) float64 [used sources, used targets] of a label's used pairs: (d - s) / vote_bin"""
    src, dst = list_rows(sample, label)
    pts = np.concatenate([sample["pc0s"], sample["pc1"]]).astype(np.float64)
    s, d = pts[rr._pick(src, vote_cap)], pts[rr._pick(dst, vote_cap)]
    with np.errstate(invalid="ignore"):
        return (d[None, :, 0] - s[:, None, 0]) / vote_bin, (d[None, :, 1] - s[:, None, 1]) / vote_bin


# ---- ICP: the tie rule across two LDS tiles -----------------------------------------------------------------------------------------------
TIE_STEP = 1.0 / 64.0
TIE_PARAMS = {"vote_bin": VOTE_BIN, "max_disp": 3.0, "icp_iters": 1, "min_cluster_size": 380}


def tie_sample(swapped=False):
    """40 sources on a 5 x 4 x 2 lattice of spacing 4/64 m; 340 targets: the sources moved by +1/64 m in x at list positions 0..39, 260 filler
    rows 10 m away, the sources moved by -1/64 m at positions 300..339 (`swapped`: the two blocks exchanged).  One label, rows NOT shuffled:
    every source is equally far from its two copies, one in the first LDS tile, one in the second"""
    rng = np.random.default_rng(61)
    g = np.stack(np.meshgrid(np.arange(5), np.arange(4), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3)
    src = (np.array([2.0, 1.0, 0.0]) + g * (4.0 / 64.0)).astype(np.float32)
    plus, minus = src.copy(), src.copy()
    plus[:, 0] += np.float32(TIE_STEP)
    minus[:, 0] -= np.float32(TIE_STEP)
    filler = rr._lat(rng, 260, (12.0, 1.0, 0.0), (13.0, 2.0, 0.5))
    dst = np.concatenate([minus, filler, plus] if swapped else [plus, filler, minus])
    return {"pc0s": src, "pc1": dst, "labels": np.ones(380, dtype=np.int32), "params": dict(TIE_PARAMS)}


# ---- the accept step and the short loops: continuous planted vehicles, one label ----------------------------------------------------------
def _vehicle_sample(seed, params, n0=260, n1=300, noise=(7, 4), heading=0.0, **motion):
    rng = np.random.default_rng(seed)
    src, dst, _ = rr.vehicle(rng, (3.0, -7.0, 0.0), heading, n0, n1, **motion)
    s = hand_sample(rng, [(src, dst)], noise0=noise[0], noise1=noise[1])
    s["params"] = dict(params, min_cluster_size=len(s["labels"]) // 2)          # two slots, the second one empty
    return s


def accept_cases():
    """name -> sample.  The cluster is label 1 (slot 0) in every case"""
    return {
        "icp_iters_0": _vehicle_sample(71, {"icp_iters": 0}, heading=0.6, yaw=0.05, forward=1.0),
        "fewer_than_3_inliers": _vehicle_sample(72, {"icp_max_dist": 0.02}, yaw=0.05, forward=1.0),
        "yaw_over_max_yaw": _vehicle_sample(73, {"icp_iters": 24, "icp_max_dist": 1.0}, yaw=0.5, forward=0.0),
        "displacement_over_max_disp": _vehicle_sample(74, {"max_disp": 1.7}, yaw=0.0, forward=2.0),
    }


ACCEPT_CASE_NAMES = ("icp_iters_0", "fewer_than_3_inliers", "yaw_over_max_yaw", "displacement_over_max_disp")


def first_pass_inliers(sample, slot, r, dtype=np.float64):
    """inliers of the FIRST nearest-neighbour pass of a slot (theta = 0, t = the vote's translation of the helper's result r).  With fewer
    than 3 the transform stays, the next pass is the same pass, and so on: then n_in < 3 holds in every pass"""
    dt = np.dtype(dtype).type
    P = dict(rr.DEFAULTS)
    P.update(sample["params"])
    src, dst = list_rows(sample, slot + 1)
    pts = np.concatenate([sample["pc0s"], sample["pc1"]]).astype(dt)
    a = pts[src[0]]
    su, du = pts[rr._pick(src, P["icp_cap"])] - a, pts[rr._pick(dst, P["icp_cap"])] - a
    vbin = dt(np.float32(P["vote_bin"]))
    t = np.array([dt(r["vote"][slot, 0]) * vbin, dt(r["vote"][slot, 1]) * vbin, dt(0)], dtype=dt)
    _, d2 = rr._nn(su + t, du)
    md = dt(np.float32(P["icp_max_dist"]))
    return int((d2 <= md * md).sum())


# ---- apply: B = 2, one slot with status 1 in sample 0 and status 4 in sample 1 --------------------------------------------------------------
APPLY_LABEL = 2
APPLY_COUNT0 = (250, 180)       # rows of pc0s that count, per sample


def apply_samples():
    """two samples of N0 = 300, N1 = 330 and three slots.  Label 2 is a planted vehicle in sample 0 (status 1); in sample 1 half of
    its source rows are a blob that the second sweep does not have (status 4: the inlier fraction); label 1 is a slow vehicle in both.  Rows are interleaved, so labelled rows lie behind count0, and NaN rows
    with label 0 are planted inside it"""
    out = []
    for b, seed in enumerate((81, 82)):
        rng = np.random.default_rng(seed)
        slow = rr.vehicle(rng, (-9.0, 5.0, 0.0), -1.1, 60, 70, yaw=-0.03, forward=0.5)[:2]
        if b == 0:
            obj = rr.vehicle(rng, (3.0, -7.0, 0.0), 0.4, 220, 250, yaw=0.06, forward=1.7)[:2]
        else:
            src, dst, _ = rr.vehicle(rng, (3.0, -7.0, 0.0), 0.4, 110, 250, yaw=0.06, forward=1.7)
            obj = (np.concatenate([src, (np.array([2.0, -2.0, 0.0]) + rng.random((110, 3)) * [1.2, 1.2, 0.8]).astype(np.float32)]), dst)
        s = hand_sample(rng, [slow, obj], noise0=20, noise1=10)
        free = np.nonzero(s["labels"][: APPLY_COUNT0[b]] == 0)[0]
        s["pc0s"][free[:3]] = np.nan
        s["pc0s"][free[3], 1] = np.nan
        s["nan_rows"] = free[:4]
        s["params"] = {"min_cluster_size": 210}
        out.append(s)
    return out


def apply_expected(r, count0):
    """the helper's flow and rigid_id with the rows behind count0 zeroed (section 6j f: every other row of pc0s gets zeros)"""
    flow, rid = r["flow"].copy(), r["rigid_id"].copy()
    flow[count0:] = 0
    rid[count0:] = 0
    return flow, rid
