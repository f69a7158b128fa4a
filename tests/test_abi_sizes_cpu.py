"""CPU: the buffer-size table of tests/helpers/abi_sizes.py against include/deflow_amd.h and _lib._SIGS, and the guarded-call harness of
tests/helpers/guarded.py against a stand-in entry that overruns on purpose (host memory, inside the harness's own arena; no real kernel is
ever made to overrun)."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi_sizes  # noqa: E402
import guarded  # noqa: E402
from abi_sizes import IN, INOUT, OUT, WS, TABLE  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from deflow_amd import _lib, build
    build.build()
    return _lib


def _scope():
    from deflow_amd import _lib
    return abi_sizes.in_scope(_lib._SIGS, _lib.P)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def test_every_in_scope_entry_is_in_the_table_and_nothing_else():
    scope = _scope()
    assert len(scope) >= 39 and "df_cell_sort" in scope and "df_void_cast_probe" not in scope
    assert sorted(TABLE) == sorted(scope)


def test_one_entry_per_pointer_of_the_binding():
    """exactly one sized buffer for every P of _SIGS[name], the trailing stream excepted, at the position the binding has it"""
    from deflow_amd import _lib
    for name in _scope():
        sig, e = _lib._SIGS[name], TABLE[name]
        assert sig[-1] is _lib.P and len(sig) == len(e.params) + 1, name
        assert len(set(e.params)) == len(e.params), name
        for pos, pname in enumerate(e.params):
            assert (sig[pos] is _lib.P) == (pname in e.bufs), (name, pname)
        assert len(e.bufs) == sum(1 for t in sig[:-1] if t is _lib.P), name


def test_table_matches_the_headers_prototypes():
    """names and order, const <-> input, /*nullable*/ <-> nullable; what the prototype cannot say is listed with the section's words"""
    protos = abi_sizes.header_prototypes()
    for name, e in TABLE.items():
        ps = protos[name]
        assert ps[-1].name == "stream" and tuple(p.name for p in ps[:-1]) == e.params, name
        for p in ps[:-1]:
            assert p.pointer == (p.name in e.bufs), (name, p.name)
            if not p.pointer:
                continue
            b = e.bufs[p.name]
            assert (b.role == IN) == p.const, (name, p.name, b.role)
            assert b.nullable == (p.nullable or p.name in abi_sizes.NULLABLE_BY_TEXT.get(name, ())), (name, p.name)
            if not p.const and b.role != WS:
                assert (b.role == INOUT) == (p.name in abi_sizes.INOUT_BY_TEXT.get(name, ())), (name, p.name, b.role)
            if b.role == WS:
                assert p.name == "ws" and b.ws_fn in protos and b.size is None, (name, p.name)
                assert b.ws_args.replace(" ", "").split(",") == [q.name for q in protos[b.ws_fn]], (name, b.ws_fn)
            elif b.size is None:
                assert b.role == IN and b.why, (name, p.name)          # RECORDED: inputs only, and with the reason
            else:
                assert b.role in (IN, OUT, INOUT)
    for extra in (abi_sizes.NULLABLE_BY_TEXT, abi_sizes.INOUT_BY_TEXT):
        for name, ps in extra.items():
            assert ps <= set(TABLE[name].bufs), name


def test_only_the_documented_input_is_recorded():
    rec = [(n, p) for n, e in TABLE.items() for p, b in e.bufs.items() if b.role != WS and b.size is None]
    assert rec == [("df_chamfer_nn", "sorted")]


def test_size_expressions_evaluate(lib):
    """every expression evaluates to a positive integer at small arguments; spot values restate the header's shapes"""
    for name, e in TABLE.items():
        scal = {p: 2 for p in e.params if p not in e.bufs}
        if "param_stride" in scal:
            scal["param_stride"] = 20000
        if "Gx" in scal and "Gz" in scal:
            scal["Gx"] = 32
        for pname, b in e.bufs.items():
            if b.role == WS or b.size is None:
                continue
            n = abi_sizes.eval_buf(b, scal)
            assert isinstance(n, int) and n > 0, (name, pname, n)
    sz = abi_sizes.size_of
    assert sz("df_chamfer_nn", "d2", dict(B=3, Nq=257, G=8)) == 3 * 257 * 4
    assert sz("df_nn_grid_build", "sorted", dict(B=3, Nr=513, G=8)) == 3 * 513 * 16
    assert sz("df_void_cast", "F", dict(B=3, Gx=32, Gy=5, Gz=3)) == 3 * 15 * 4
    assert sz("df_flow_compose", "flow_est", dict(B=3, N=10, Nc=7, half=1)) == 3 * 10 * 3 * 2
    assert sz("df_flow_compose", "flow_est", dict(B=3, N=10, Nc=7, half=0)) == 3 * 10 * 3 * 4
    assert sz("df_submit_pack", "body", dict(B=2, N=13)) == 2 * 128                       # L(13) = 104 -> 128
    assert sz("df_render_resolve", "scanlines", dict(B=3, W=33, H=17)) == 3 * 17 * 100
    assert sz("df_rigid_vote", "hist", dict(B=3, Kcap=19, R=17)) == 3 * 19 * 35 * 35 * 4
    assert sz("df_mlp_fwd", "params", dict(B=3, param_stride=17412, depth=1)) == 4 * (2 * 17412 + 17411)
    assert sz("df_mlp_bwd", "dparams", dict(B=3, param_stride=17412, depth=1)) == 4 * 3 * 17412
    assert sz("df_mlp_bwd", "dparams", dict(B=1, param_stride=900, depth=0)) == 4 * 900    # P = 899 -> 900
    assert sz("df_dt_build", "dt2", dict(B=3, GX=257, GY=3, GZ=2)) == 3 * 257 * 6 * 2
    assert sz("df_vox_plan", "cell_rng", dict(B=3, VX=5, VY=4, VZ=3)) == 3 * 24 * 8
    assert sz("df_refine_fit", "table", dict(B=3, Kcap=12)) == 3 * 12 * 48


def test_every_workspace_resolves_to_an_exported_query_that_is_positive(lib):
    """at the arguments of the scenarios of tests/test_gpu_guarded_ops.py"""
    handle = lib.load()
    fns = {b.ws_fn for e in TABLE.values() for b in e.bufs.values() if b.role == WS}
    cases = abi_sizes.ws_cases()
    assert fns == set(cases), fns ^ set(cases)
    for fn, argsets in cases.items():
        assert hasattr(handle, fn) and fn in lib._SIGS and fn in lib._RAW, fn
        assert argsets, fn
        for a in argsets:
            assert len(a) == len(lib._SIGS[fn]), (fn, a)
            assert abi_sizes.ws_query(fn, *a) > 0, (fn, a)


# ---- the harness can fail ----------------------------------------------------------------------------------------------------------------
def _f32(address: int, n: int) -> torch.Tensor:
    return torch.frombuffer((C.c_uint8 * (4 * n)).from_address(address), dtype=torch.float32)


FAKE = {"df_standin": abi_sizes._e("x n y ws", x=abi_sizes.i("4 * n"), y=abi_sizes.o("4 * n"), ws=abi_sizes.ws("standin_ws_bytes", "n"))}


def _standin(mode: str):
    """y = 2 x through a workspace, in torch on host memory; the three planted faults stay inside the harness's arena"""
    def entry(name, x, n, y, ws, stream):
        assert name == "df_standin" and stream is None
        w = _f32(ws, n)
        w.copy_(_f32(x, n))
        _f32(y, n).copy_(w * 2)
        if mode == "past_output":
            _f32(y + 4 * n, 1)[0] = 1.0
        elif mode == "before_workspace":
            _f32(ws - 4, 1)[0] = 1.0
        elif mode == "reads_past_input":
            _f32(y + 4 * (n - 1), 1)[0] += _f32(x + 4 * n, 1)[0]
        return 0
    return entry


def _run(mode: str, fill: int, n: int = 7, y_elems=None, record=True):
    g = guarded.Guard(fill, _standin(mode), table=FAKE, query=lambda fn, n_: {"standin_ws_bytes": 4 * n_}[fn])
    x = torch.arange(1, n + 1, dtype=torch.float32)
    y = torch.full((n if y_elems is None else y_elems,), -1.0)
    ws = torch.zeros(4 * n, dtype=torch.uint8)
    g.call("df_standin", g.ptr(x), n, g.ptr(y) if record else y.data_ptr(), g.ptr(ws), None)
    return g, x, y


@pytest.mark.parametrize("fill", [0xA5, 0x7F])
def test_harness_passes_a_clean_entry_and_lays_the_arena_out_as_stated(fill):
    g, x, y = _run("clean", fill)
    assert torch.equal(y, 2 * x) and g.seen == ["df_standin"]
    base, total = g.arena_span
    assert [p for p, _, _ in g.layout] == ["x", "y", "ws"] and [s for _, _, s in g.layout] == [28, 28, 28]
    prev_end = base
    for _, addr, size in g.layout:
        assert addr % 32 == 16 and addr - prev_end >= guarded.PAD
        prev_end = addr + size
    assert base + total - prev_end >= guarded.TAIL == 1 << 20 and guarded.PAD == 4096
    # a call the table does not hold goes straight through
    assert guarded.Guard(fill, lambda name, *a: (name, a), table=FAKE).call("df_other", 1, 2) == ("df_other", (1, 2))


def test_harness_reports_a_write_past_an_output():
    with pytest.raises(guarded.GuardError, match=r"df_standin: y \(out, 28 bytes\): 4 damaged bytes starting 0 bytes past its end"):
        _run("past_output", 0xA5)


def test_harness_reports_a_write_before_a_workspace():
    with pytest.raises(guarded.GuardError, match=r"df_standin: ws \(ws, 28 bytes\): 4 damaged bytes starting 4 bytes before its start"):
        _run("before_workspace", 0x7F)


def test_a_read_past_an_input_makes_the_result_depend_on_the_fill():
    (_, _, clean_a), (_, _, clean_b) = _run("clean", 0xA5), _run("clean", 0x7F)
    assert guarded.same_bits(clean_a, clean_b)
    (_, _, a), (_, _, b) = _run("reads_past_input", 0xA5), _run("reads_past_input", 0x7F)
    assert not guarded.same_bits(a, b) and guarded.same_bits(a[:-1], b[:-1])
    assert float(b[-1]) > 1e38                                         # 0x7F7F7F7F read as a float


def test_harness_reports_a_short_wrapper_allocation_and_a_raw_pointer():
    with pytest.raises(guarded.GuardError, match=r"df_standin: y: the wrapper passed a tensor of 24 bytes, the header states 28"):
        _run("clean", 0xA5, y_elems=6)
    with pytest.raises(guarded.GuardError, match=r"df_standin: y: the pointer .* was not made by ptr\(\)"):
        _run("clean", 0xA5, record=False)
    g = guarded.Guard(0xA5, _standin("clean"), table=FAKE, query=lambda fn, n_: 4 * n_)
    with pytest.raises(guarded.GuardError, match=r"df_standin: x: NULL"):
        g.call("df_standin", None, 7, None, None, None)


def test_extent_is_the_views_own_span():
    t = torch.zeros(3, 10)
    assert guarded.extent(t) == 120 and guarded.extent(t[:, :8]) == (2 * 10 + 8) * 4 and guarded.extent(t[1:]) == 80
    assert guarded.extent(torch.zeros(0)) == 0
    v = t[1:]
    guarded.raw_bytes(v, 80).fill_(1)
    assert float(t.sum()) != 0 and float(t[0].sum()) == 0
