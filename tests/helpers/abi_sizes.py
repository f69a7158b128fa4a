"""The byte size of every buffer of the point-cloud entry points, as include/deflow_amd.h states it.

One table, transcribed from the header's sentences and NOT from the Python wrappers: for every in-scope entry point the argument names in
the header's order, and for every pointer among them its role (input, output, in/out, workspace), whether it may be NULL, and its size in
bytes as an expression of the call's own scalar arguments.  tests/helpers/guarded.py carves its guarded regions from it, and
tests/test_abi_sizes_cpu.py holds it against the header's prototypes (names, order, const, nullable) and against _lib._SIGS, so that a
pointer added later fails there until it is sized here.  This is the place where a new entry point's buffer sizes are stated.

A workspace's size is what the matching df_*_ws_bytes function returns for the call's arguments: that is the promise under test.  Where an
input's extent cannot be derived from the call's own arguments the entry says so (RECORDED, with the reason) and the harness uses the
extent of the tensor the wrapper passed; that is never allowed for an output or a workspace.

In scope: df_cell_sort and every entry from df_nn_grid_build to df_refine_apply of _lib._SIGS that takes a pointer (the *_ws_bytes,
*_rows_per_block and df_submit_body_stride queries take none).  Out of scope: df_void_cast_probe, which serves only a tool."""
from __future__ import annotations

import os
import re
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "include", "deflow_amd.h")

IN, OUT, INOUT, WS = "in", "out", "inout", "ws"
OUT_OF_SCOPE = ("df_void_cast_probe",)


class Buf(NamedTuple):
    role: str
    size: Optional[str]            # bytes, a Python expression of the entry's scalar arguments; None: RECORDED (inputs only)
    nullable: bool = False
    ws_fn: Optional[str] = None    # workspaces: the df_*_ws_bytes symbol ...
    ws_args: Optional[str] = None  # ... and its arguments, an expression of the entry's scalar arguments
    why: str = ""                  # RECORDED: why the call's arguments do not give the extent


class Entry(NamedTuple):
    params: Tuple[str, ...]        # every argument in the header's order, the trailing stream excepted
    bufs: Dict[str, Buf]


def i(size: str, nullable: bool = False) -> Buf:
    return Buf(IN, size, nullable)


def o(size: str, nullable: bool = False) -> Buf:
    return Buf(OUT, size, nullable)


def io(size: str, nullable: bool = False) -> Buf:
    return Buf(INOUT, size, nullable)


def ws(fn: str, args: str, nullable: bool = False) -> Buf:
    return Buf(WS, None, nullable, fn, args)


def recorded(why: str) -> Buf:
    return Buf(IN, None, False, None, None, why)


def _e(_params: str, /, **bufs: Buf) -> Entry:
    names = tuple(_params.split())
    assert set(bufs) <= set(names), sorted(set(bufs) - set(names))
    return Entry(names, bufs)


# names the size expressions may use besides the scalar arguments
MLP_P = "(128 * 3 + 128 + depth * (128 * 128 + 128) + 3 * 128 + 3)"           # P of the header's MLP section
MLP_P4 = f"(({MLP_P} + 3) // 4 * 4)"
VOID_WORDS = "(Gx * Gy * Gz // 32)"
NV = "(VX * VY * VZ)"
NC = "((VX - 1) * (VY - 1) * (VZ - 1))"
_GRID = "minx miny cell G"

TABLE: Dict[str, Entry] = {
    # idx_sorted [n] u32, cell_rng [ncells, 2] i32
    "df_cell_sort": _e("key n ncells idx_sorted cell_rng ws",
                       key=i("4 * n"), idx_sorted=o("4 * n"), cell_rng=o("8 * ncells"), ws=ws("df_cell_sort_ws_bytes", "ncells")),
    # ---- chamfer: cell_rng [B*G*G, 2] i32, sorted [B*Nr, 4] f32
    "df_nn_grid_build": _e(f"ref rcount rlabel B Nr {_GRID} cell_rng sorted ws",
                           ref=i("12 * B * Nr"), rcount=i("4 * B"), rlabel=i("4 * B * Nr", True), cell_rng=o("8 * B * G * G"),
                           sorted=o("16 * B * Nr"), ws=ws("df_nn_grid_ws_bytes", "B, Nr, G")),
    "df_chamfer_nn": _e(f"query qcount qlabel B Nq cell_rng sorted {_GRID} max_dist2 d2 idx far_count",
                        query=i("12 * B * Nq"), qcount=i("4 * B"), qlabel=i("4 * B * Nq", True), cell_rng=i("8 * B * G * G"),
                        sorted=recorded("[B*Nr, 4] f32, and the entry does not receive Nr"),
                        d2=o("4 * B * Nq"), idx=o("4 * B * Nq"), far_count=io("4", True)),
    # "Either output may be NULL; ws (needed for dref)"
    "df_chamfer_bwd": _e("query ref idx g B Nq Nr dquery dref ws",
                         query=i("12 * B * Nq"), ref=i("12 * B * Nr"), idx=i("4 * B * Nq"), g=i("4 * B * Nq"),
                         dquery=io("12 * B * Nq", True), dref=io("12 * B * Nr", True),
                         ws=ws("df_chamfer_bwd_ws_bytes", "B, Nq, Nr", True)),
    # ---- DBSCAN: the grid was built with ref = points, so sorted is [B*N, 4]
    "df_dbscan_core": _e(f"cell_rng sorted B N {_GRID} eps min_points ws",
                         cell_rng=i("8 * B * G * G"), sorted=i("16 * B * N"), ws=ws("df_dbscan_ws_bytes", "B, N")),
    "df_dbscan_link": _e(f"cell_rng B N {_GRID} eps status ws",
                         cell_rng=i("8 * B * G * G"), status=io("4", True), ws=ws("df_dbscan_ws_bytes", "B, N")),
    "df_dbscan_finish": _e(f"cell_rng dynamic B N {_GRID} eps min_cluster_size min_dynamic_frac labels n_clusters status ws",
                           cell_rng=i("8 * B * G * G"), dynamic=i("4 * B * N", True), labels=o("4 * B * N"), n_clusters=o("4 * B"),
                           status=io("4", True), ws=ws("df_dbscan_ws_bytes", "B, N")),
    # ---- void map: F, O, V are [B, Gx*Gy*Gz/32] u32
    "df_void_cast": _e("points count origin B N gminx gminy gminz k Gx Gy Gz hit_margin R F O status",
                       points=i("12 * B * N"), count=i("4 * B"), origin=i("12 * B"), F=o(f"4 * B * {VOID_WORDS}"),
                       O=o(f"4 * B * {VOID_WORDS}"), status=io("4", True)),
    "df_void_merge": _e("F O V B Gx Gy Gz erode",
                        F=i(f"4 * B * {VOID_WORDS}"), O=i(f"4 * B * {VOID_WORDS}"), V=io(f"4 * B * {VOID_WORDS}")),
    "df_void_query": _e("points count B N gminx gminy gminz k Gx Gy Gz V flags",
                        points=i("12 * B * N"), count=i("4 * B"), V=i(f"4 * B * {VOID_WORDS}"), flags=o("4 * B * N")),
    # ---- ground: zmin, height i32 [B,Gy,Gx], observed u8 [B,Gy,Gx], mask u8 [B,N]
    "df_ground_cells": _e("points count B N xmin ymin kxy z_min kz Gx Gy H zmin",
                          points=i("12 * B * N"), count=i("4 * B"), zmin=o("4 * B * Gy * Gx")),
    "df_ground_height": _e("zmin B Gx Gy ox oy seed rise drop widen miss_cap height observed",
                           zmin=i("4 * B * Gy * Gx"), height=o("4 * B * Gy * Gx"), observed=o("B * Gy * Gx")),
    "df_ground_mask": _e("points count B N xmin ymin kxy z_min kz Gx Gy H height tol mask",
                         points=i("12 * B * N"), count=i("4 * B"), height=i("4 * B * Gy * Gx"), mask=o("B * N")),
    # ---- metrics: edges double[50], state_f double[526], state_i int64[272]
    "df_metrics_rows": _e("flow pose_flow pc0 gt_flow idx_c counts is_valid eval_mask cats B N edges ws status",
                          flow=i("12 * B * N"), pose_flow=i("12 * B * N"), pc0=i("12 * B * N"), gt_flow=i("12 * B * N"),
                          idx_c=i("8 * B * N"), counts=i("4 * B"), is_valid=i("B * N", True), eval_mask=i("B * N", True),
                          cats=i("B * N", True), edges=i("8 * 50"), ws=ws("df_metrics_ws_bytes", "B, N"), status=io("4", True)),
    "df_metrics_accumulate": _e("counts has_eval_mask B N ws state_f state_i",
                                counts=i("4 * B"), has_eval_mask=i("B", True), ws=ws("df_metrics_ws_bytes", "B, N"),
                                state_f=io("8 * 526"), state_i=io("8 * 272")),
    # ---- whole-sweep flow
    "df_sweep_compact": _e("raw count_raw drop B N ws pc row_of pos_of kept",
                           raw=i("12 * B * N"), count_raw=i("4 * B"), drop=i("B * N"), ws=ws("df_sweep_compact_ws_bytes", "B, N"),
                           pc=o("12 * B * N"), row_of=o("4 * B * N"), pos_of=o("4 * B * N"), kept=o("4 * B")),
    "df_flow_compose": _e("raw count_raw T pos_of flow idx_c counts B N Nc half ws flow_est dynamic",
                          raw=i("12 * B * N"), count_raw=i("4 * B"), T=i("64 * B"), pos_of=i("4 * B * N"), flow=i("12 * B * Nc"),
                          idx_c=i("8 * B * Nc"), counts=i("4 * B"), ws=ws("df_flow_compose_ws_bytes", "B, N"),
                          flow_est=o("(6 if half else 12) * B * N"), dynamic=o("B * N")),
    # ---- submission: body [B,S] u8, S = df_submit_body_stride(N)
    "df_submit_pack": _e("flow_est dynamic row_of kept B N version body",
                         flow_est=i("12 * B * N"), dynamic=i("B * N"), row_of=i("4 * B * N"), kept=i("4 * B"),
                         body=o("B * query('df_submit_body_stride', N)")),
    # ---- augmentation: flow, T and the poses are "nullable with their outputs"
    "df_augment": _e("pc0 pc1 flow sample_ids B N0 N1 seed epoch flip_x_p flip_y_p yaw_max height_max jitter_sigma drop_p T pose0 pose1 "
                     "pc0_out pc1_out flow_out T_out pose0_out pose1_out",
                     pc0=i("12 * B * N0"), pc1=i("12 * B * N1"), flow=i("12 * B * N0", True), sample_ids=i("8 * B"), T=i("64 * B", True),
                     pose0=i("64 * B", True), pose1=i("64 * B", True), pc0_out=o("12 * B * N0"), pc1_out=o("12 * B * N1"),
                     flow_out=o("12 * B * N0", True), T_out=o("64 * B", True), pose0_out=o("64 * B", True),
                     pose1_out=o("64 * B", True)),
    "df_augment_params": _e("sample_ids B seed epoch flip_x_p flip_y_p yaw_max height_max jitter_sigma drop_p params",
                            sample_ids=i("8 * B"), params=o("32 * B")),
    # ---- rendering: image u64 [B,H,W] (zeroed by the caller, raised by integer atomic max), scanlines u8 [B, H, 1 + 3W]
    "df_render_splat": _e("points vec cls count B N xmin ymin inv_res W H vmax radius image",
                          points=i("12 * B * N"), vec=i("12 * B * N"), cls=i("B * N"), count=i("4 * B"), image=io("8 * B * H * W")),
    "df_render_resolve": _e("image B W H bg_rgb legend scanlines",
                            image=i("8 * B * H * W"), scanlines=o("B * H * (1 + 3 * W)")),
    # ---- rigid cluster flow: N = N0 + N1
    "df_rigid_segments": _e("labels B N0 N1 Kcap seg_off seg_rows status ws",
                            labels=i("4 * B * (N0 + N1)"), seg_off=o("4 * B * (2 * Kcap + 1)"), seg_rows=o("4 * B * (N0 + N1)"),
                            status=io("4"), ws=ws("df_rigid_segments_ws_bytes", "B, N0, N1, Kcap")),
    "df_rigid_vote": _e("pc0s pc1 seg_off seg_rows B N0 N1 Kcap min_side max_cluster_points vote_cap vote_bin R vote hist",
                        pc0s=i("12 * B * N0"), pc1=i("12 * B * N1"), seg_off=i("4 * B * (2 * Kcap + 1)"),
                        seg_rows=i("4 * B * (N0 + N1)"), vote=o("12 * B * Kcap"),
                        hist=o("4 * B * Kcap * (2 * R + 1) * (2 * R + 1)", True)),
    "df_rigid_icp": _e("pc0s pc1 seg_off seg_rows vote B N0 N1 Kcap min_side max_cluster_points icp_cap icp_iters vote_bin icp_max_dist "
                       "min_inlier_frac max_yaw max_disp table ws",
                       pc0s=i("12 * B * N0"), pc1=i("12 * B * N1"), seg_off=i("4 * B * (2 * Kcap + 1)"),
                       seg_rows=i("4 * B * (N0 + N1)"), vote=i("12 * B * Kcap"), table=o("32 * B * Kcap"),
                       ws=ws("df_rigid_icp_ws_bytes", "B, N0, N1")),
    "df_rigid_apply": _e("pc0s count0 labels seg_off seg_rows table B N0 N1 Kcap flow rigid_id",
                         pc0s=i("12 * B * N0"), count0=i("4 * B"), labels=i("4 * B * (N0 + N1)"), seg_off=i("4 * B * (2 * Kcap + 1)"),
                         seg_rows=i("4 * B * (N0 + N1)"), table=i("32 * B * Kcap"), flow=o("12 * B * N0"), rigid_id=o("4 * B * N0")),
    # ---- MLP: sample b's parameters at params + b * param_stride, P of them; dparams: B blocks at param_stride, P rounded up to 4 written
    "df_mlp_fwd": _e("x count params param_stride B N depth y acts",
                     x=i("12 * B * N"), count=i("4 * B"), params=i(f"4 * ((B - 1) * param_stride + {MLP_P})"), y=o("12 * B * N"),
                     acts=o("4 * B * (depth + 1) * N * 128", True)),
    "df_mlp_bwd": _e("x count params param_stride acts dy B N depth dparams dx ws",
                     x=i("12 * B * N"), count=i("4 * B"), params=i(f"4 * ((B - 1) * param_stride + {MLP_P})"),
                     acts=i("4 * B * (depth + 1) * N * 128"), dy=i("12 * B * N"),
                     dparams=o(f"4 * ((B - 1) * param_stride + {MLP_P4})"), dx=o("12 * B * N", True),
                     ws=ws("df_mlp_ws_bytes", "B, N, depth")),
    # ---- distance transform: dt2 [B,GZ,GY,GX] u16
    "df_dt_build": _e("ref count B N ox oy oz cell GX GY GZ R dt2 ws",
                      ref=i("12 * B * N"), count=i("4 * B"), dt2=o("2 * B * GX * GY * GZ"), ws=ws("df_dt_ws_bytes", "B, GX, GY, GZ, R")),
    "df_dt_lookup": _e("query count dt2 B N ox oy oz cell GX GY GZ R d g cells clamped",
                       query=i("12 * B * N"), count=i("4 * B"), dt2=i("2 * B * GX * GY * GZ"), d=o("4 * B * N"), g=o("12 * B * N"),
                       cells=o("12 * B * N", True), clamped=o("B * N", True)),
    # ---- rigidity term: seg_rows [B, N + 1], nbr / r0 [B,N,2P]
    "df_iso_plan": _e("x count labels seg_off seg_rows B N Kcap P max_cluster_points nbr r0 pairs",
                      x=i("12 * B * N"), count=i("4 * B"), labels=i("4 * B * N"), seg_off=i("4 * B * (2 * Kcap + 1)"),
                      seg_rows=i("4 * B * (N + 1)"), nbr=o("4 * B * N * 2 * P"), r0=o("4 * B * N * 2 * P"), pairs=o("4 * B")),
    "df_iso_pairs": _e("w nbr r0 B N P delta v g",
                       w=i("12 * B * N"), nbr=i("4 * B * N * 2 * P"), r0=i("4 * B * N * 2 * P"), v=o("4 * B * N"), g=o("12 * B * N")),
    # ---- voxel flow: theta [B,NV,3], cell_rng [B NC, 2], active [B,NV] u8
    "df_vox_plan": _e("x count B N ox oy oz voxel VX VY VZ cell frac idx_sorted cell_rng active pairs ws",
                      x=i("12 * B * N"), count=i("4 * B"), cell=o("4 * B * N"), frac=o("12 * B * N"), idx_sorted=o("4 * B * N"),
                      cell_rng=o(f"8 * B * {NC}"), active=o(f"B * {NV}"), pairs=o("4 * B"),
                      ws=ws("df_vox_plan_ws_bytes", "B, N, VX, VY, VZ")),
    "df_vox_sample": _e("theta cell frac B N VX VY VZ F",
                        theta=i(f"12 * B * {NV}"), cell=i("4 * B * N"), frac=i("12 * B * N"), F=o("12 * B * N")),
    "df_vox_scatter": _e("dF frac idx_sorted cell_rng B N VX VY VZ dtheta",
                         dF=i("12 * B * N"), frac=i("12 * B * N"), idx_sorted=i("4 * B * N"), cell_rng=i(f"8 * B * {NC}"),
                         dtheta=o(f"12 * B * {NV}")),
    "df_vox_smooth": _e("theta active B VX VY VZ v g",
                        theta=i(f"12 * B * {NV}"), active=i(f"B * {NV}"), v=o(f"4 * B * {NV}"), g=o(f"12 * B * {NV}")),
    # ---- refine: seg_rows [B, Nc + 1], table [B,Kcap,12] f32, anchor [B,Kcap] i32
    "df_refine_fit": _e("x flow count seg_off seg_rows B Nc Kcap min_rows max_cluster_points iters delta inlier_dist min_inlier_frac max_yaw "
                        "max_disp static_disp static_yaw table anchor",
                        x=i("12 * B * Nc"), flow=i("12 * B * Nc"), count=i("4 * B"), seg_off=i("4 * B * (2 * Kcap + 1)"),
                        seg_rows=i("4 * B * (Nc + 1)"), table=o("48 * B * Kcap"), anchor=o("4 * B * Kcap")),
    "df_refine_score": _e("x flow count count1 seg_off seg_rows d2_before d2_after B Nc Kcap check_trunc check_tol table",
                          x=i("12 * B * Nc"), flow=i("12 * B * Nc"), count=i("4 * B"), count1=i("4 * B"),
                          seg_off=i("4 * B * (2 * Kcap + 1)"), seg_rows=i("4 * B * (Nc + 1)"), d2_before=i("4 * B * Nc"),
                          d2_after=i("4 * B * Nc"), table=io("48 * B * Kcap")),
    "df_refine_apply": _e("x flow count labels table anchor B Nc Kcap flow_out rigid_id",
                          x=i("12 * B * Nc"), flow=i("12 * B * Nc"), count=i("4 * B"), labels=i("4 * B * Nc"), table=i("48 * B * Kcap"),
                          anchor=i("4 * B * Kcap"), flow_out=o("12 * B * Nc"), rigid_id=o("4 * B * Nc")),
}

# pointers the header's prototype does not mark /*nullable*/ but whose section says in words that they may be NULL
NULLABLE_BY_TEXT = {
    "df_chamfer_bwd": {"dquery", "dref", "ws"},                                  # "Either output may be NULL; ws (needed for dref)"
    "df_augment": {"flow_out", "T_out", "pose0_out", "pose1_out"},               # "nullable with flow_out" / "with their outputs"
}
# non-const pointers that the entry also reads: the prototype cannot tell them from plain outputs, the section's text does
INOUT_BY_TEXT = {
    "df_chamfer_nn": {"far_count"}, "df_chamfer_bwd": {"dquery", "dref"}, "df_dbscan_link": {"status"}, "df_dbscan_finish": {"status"},
    "df_void_cast": {"status"}, "df_void_merge": {"V"}, "df_metrics_rows": {"status"}, "df_metrics_accumulate": {"state_f", "state_i"},
    "df_render_splat": {"image"}, "df_rigid_segments": {"status"}, "df_refine_score": {"table"},
}


def in_scope(sigs: Dict[str, list], pointer_type) -> List[str]:
    """df_cell_sort and every entry of _SIGS from df_nn_grid_build to df_refine_apply that takes a pointer besides the stream"""
    names = list(sigs)
    lo, hi = names.index("df_nn_grid_build"), names.index("df_refine_apply")
    out = ["df_cell_sort"]
    for n in names[lo:hi + 1]:
        if n not in OUT_OF_SCOPE and sum(1 for t in sigs[n] if t is pointer_type) > 1:
            out.append(n)
    return out


def ws_query(name: str, *args) -> int:
    """a df_*_ws_bytes (or df_submit_body_stride) value: host-only functions of the library, callable without a GPU"""
    from deflow_amd import _lib
    return int(_lib.call(name, *args))


def ws_cases() -> Dict[str, List[tuple]]:
    """the arguments every df_*_ws_bytes function gets in the scenarios of tests/test_gpu_guarded_ops.py (that module asserts that the
    workspace queries it saw are all listed here)"""
    nm = ws_query("df_metrics_rows_per_block") + 1
    ns = ws_query("df_sweep_rows_per_block") + 1
    return {
        "df_cell_sort_ws_bytes": [(1,), (2049,)],
        "df_nn_grid_ws_bytes": [(3, 513, 8), (3, 257, 12), (3, 387, 12), (3, 130, 17)],     # chamfer; DBSCAN, rigid, refine's check
        "df_chamfer_bwd_ws_bytes": [(3, 257, 513)],
        "df_dbscan_ws_bytes": [(3, 257), (3, 387)],
        "df_metrics_ws_bytes": [(3, nm)],
        "df_sweep_compact_ws_bytes": [(3, ns), (3, 257)],
        "df_flow_compose_ws_bytes": [(3, ns)],
        "df_rigid_segments_ws_bytes": [(3, 257, 130, 19), (3, 257, 1, 257), (3, 257, 1, 12)],   # rigid, iso, refine
        "df_rigid_icp_ws_bytes": [(3, 257, 130)],
        "df_mlp_ws_bytes": [(3, 65, 0), (3, 65, 1), (3, 1025, 1)],
        "df_dt_ws_bytes": [(3, 257, 3, 2, 2), (3, 5, 4, 3, 3)],
        "df_vox_plan_ws_bytes": [(3, 257, 2, 2, 2), (3, 257, 5, 4, 3)],
    }


def scalars_of(entry: Entry, args) -> Dict[str, object]:
    return {n: a for n, a in zip(entry.params, args) if n not in entry.bufs}


def size_of(name: str, pname: str, scalars: Dict[str, object], query: Callable[..., int] = ws_query) -> Optional[int]:
    """bytes the header states for parameter pname of entry `name` at these scalar arguments; None for a RECORDED input"""
    b = TABLE[name].bufs[pname]
    return eval_buf(b, scalars, query)


def eval_buf(b: Buf, scalars: Dict[str, object], query: Callable[..., int] = ws_query) -> Optional[int]:
    env = dict(scalars, query=query)
    if b.role == WS:
        a = eval("(" + b.ws_args + ",)", {"__builtins__": {}}, env)
        return int(query(b.ws_fn, *a))
    if b.size is None:
        return None
    return int(eval(b.size, {"__builtins__": {}}, env))


# ---- the header's prototypes ------------------------------------------------------------------------------------------------------------
class Param(NamedTuple):
    name: str
    pointer: bool
    const: bool
    nullable: bool


def header_prototypes(path: str = HEADER) -> Dict[str, List[Param]]:
    """name -> parameters of every `int df_*(...)` / `int64_t df_*(...)` prototype, read off the header's text"""
    src = open(path).read()
    src = re.sub(r"/\*\s*nullable[^*]*\*/", " __NULLABLE__ ", src)
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    out: Dict[str, List[Param]] = {}
    for m in re.finditer(r"\b(?:int|int64_t)\s+(df_[a-z0-9_]+)\s*\(([^;{]*)\)\s*;", src):
        params = []
        for p in m.group(2).split(","):
            p = p.strip()
            if not p or p == "void":
                continue
            nullable = "__NULLABLE__" in p
            p = p.replace("__NULLABLE__", " ").strip()
            pname = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1]
            params.append(Param(pname, "*" in p, bool(re.match(r"const\b", p)), nullable))
        out[m.group(1)] = params
    return out
