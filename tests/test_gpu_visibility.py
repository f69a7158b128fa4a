"""GPU: the depth cube of DESIGN.md section 6u (UNPINNED) -- df_depth_cube_build, df_depth_cube_test and ``visibility.DepthCube`` --
against the float32 restatement of tests/helpers/vis_ref.py, whose own conditions tests/test_visibility_cpu.py checks without a GPU.

Shapes: N and M in {600, 640} rows (three blocks of 256, the last one partial or exact), B = 3, R in {2, 8, 256}, halo in {0, 1, 2}.
Every output is EQUAL to the restatement: the bins' bit patterns, the flags and the window depths' bit patterns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import abi_sizes  # noqa: E402
import guarded  # noqa: E402
import vis_ref  # noqa: E402

pytestmark = pytest.mark.gpu

PARAMS = dict(margin=vis_ref.MARGIN, rel=vis_ref.REL, near=vis_ref.NEAR)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", torch.cuda.current_device())


def on(dev, case, B=3):
    return {k: torch.from_numpy(case[k][:B]).to(dev) for k in ("points", "count", "mask", "query", "count_q")}


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("R", [2, 8, 256])
@pytest.mark.parametrize("N,M", [(600, 640), (640, 600)])
def test_cube_and_flags_equal_the_restatement(dev, R, N, M):
    from deflow_amd.visibility import DepthCube
    case = vis_ref.kernel_case(R, N, M)
    d = on(dev, case)
    cube = DepthCube(3, R, dev)
    img = u32(cube.build(d["points"], d["count"], d["mask"]))
    want = [vis_ref.build(case["points"][b], case["count"][b], case["mask"][b], R) for b in range(3)]
    assert img.shape == (3, 6, R, R)
    for b in range(3):
        assert np.array_equal(img[b], vis_ref.image(want[b], R)), b
    assert (img[2] == vis_ref.EMPTY).all() and (img[1] != vis_ref.EMPTY).sum() == 1            # count 0; N - 5 rows in one bin
    flagged = 0
    for halo in (0, 1, 2):
        flag, depth = cube.seen_through(d["query"], d["count_q"], halo=halo, depth=True, **PARAMS)
        assert flag.dtype == torch.int32 and tuple(flag.shape) == (3, M) and depth.dtype == torch.float32
        flag, depth = flag.cpu().numpy(), u32(depth)
        for b in range(3):
            f, dm = vis_ref.test(case["query"][b], case["count_q"][b], want[b], R, halo, **PARAMS)
            assert np.array_equal(flag[b], f) and np.array_equal(depth[b], dm), (b, halo)
        flagged += int(flag.sum())
        only = cube.seen_through(d["query"], d["count_q"], halo=halo, **PARAMS)                 # without the depth output
        assert np.array_equal(only.cpu().numpy(), flag)
    assert flagged > 20
    # no mask at all, and a bool mask
    img = u32(cube.build(d["points"], d["count"]))
    for b in range(3):
        assert np.array_equal(img[b], vis_ref.image(vis_ref.build(case["points"][b], case["count"][b], None, R), R)), b
    img = u32(cube.build(d["points"], d["count"], d["mask"] > 0))
    for b in range(3):
        assert np.array_equal(img[b], vis_ref.image(want[b], R)), b


def test_repetition_and_batch_independence(dev):
    from deflow_amd.visibility import DepthCube
    R = 8
    d = on(dev, vis_ref.kernel_case(R, 640, 600))

    def run(B):
        cube = DepthCube(B, R, dev)
        cube.img.fill_(7)                                              # whatever the buffer held: the fill launch replaces it
        img = cube.build(d["points"][:B], d["count"][:B], d["mask"][:B]).clone()
        flag, depth = cube.seen_through(d["query"][:B], d["count_q"][:B], halo=1, depth=True, **PARAMS)
        return img, flag, depth

    a, b, one = run(3), run(3), run(1)
    assert all(guarded.same_bits(x, y) for x, y in zip(a, b))
    assert all(guarded.same_bits(x, y[:1]) for x, y in zip(one, a))


# ---- the guarded-call harness -----------------------------------------------------------------------------------------------------------
_i, _o = abi_sizes.i, abi_sizes.o
CUBE_TABLE = {           # the header's sizes of the new entries, local to this file (abi_sizes.TABLE stays as it is)
    "df_depth_cube_build": abi_sizes._e("points count mask B N R img", points=_i("12 * B * N"), count=_i("4 * B"),
                                        mask=_i("4 * B * N", True), img=_o("24 * B * R * R")),
    "df_depth_cube_test": abi_sizes._e("query count_q img B M R halo margin rel near flag depth_out", query=_i("12 * B * M"),
                                       count_q=_i("4 * B"), img=_i("24 * B * R * R"), flag=_o("4 * B * M"),
                                       depth_out=_o("4 * B * M", True)),
}


def check_table(table):
    from deflow_amd import _lib
    protos = abi_sizes.header_prototypes()
    for name, entry in table.items():
        assert [p.name for p in protos[name]][:-1] == list(entry.params) and protos[name][-1].name == "stream"
        for p in protos[name][:-1]:
            assert p.pointer == (p.name in entry.bufs) and (not p.pointer or p.nullable == entry.bufs[p.name].nullable)
            assert not p.pointer or p.const == (entry.bufs[p.name].role == abi_sizes.IN)
        assert len(_lib._SIGS[name]) == len(protos[name])


def test_guarded_cube_entries_write_nothing_outside_their_buffers(dev, monkeypatch):
    from deflow_amd import _lib, args, visibility
    check_table(CUBE_TABLE)
    d = on(dev, vis_ref.kernel_case(8, 600, 640))

    def scenario():
        cube = visibility.DepthCube(3, 8, dev)
        img = cube.build(d["points"], d["count"], d["mask"]).clone()
        flag, depth = cube.seen_through(d["query"], d["count_q"], halo=2, depth=True, **PARAMS)
        cube.build(d["points"], d["count"])
        return [img, flag, depth, cube.img, cube.seen_through(d["query"], d["count_q"], halo=0, **PARAMS)]

    outs = [scenario()]
    for fill in (0xA5, 0x7F):
        with monkeypatch.context() as mp:
            g = guarded.Guard(fill, _lib.call, table=CUBE_TABLE)
            for mod in (visibility, args):
                mp.setattr(mod, "call", g.call)
                mp.setattr(mod, "ptr", g.ptr)
            outs.append(scenario())
        assert g.seen == ["df_depth_cube_build", "df_depth_cube_test"] * 2
    for k, (a, b, c) in enumerate(zip(*outs)):
        assert guarded.same_bits(a, b) and guarded.same_bits(a, c), k


def test_cube_argument_errors(dev):
    from deflow_amd._lib import call, ptr
    from deflow_amd.visibility import DepthCube
    with pytest.raises(TypeError, match="DepthCube: device must be a CUDA device"):
        DepthCube(1, 8, "cpu")
    with pytest.raises(ValueError, match="DepthCube: res must be even"):
        DepthCube(1, 7, dev)
    with pytest.raises(ValueError, match="DepthCube: res must be an integer"):
        DepthCube(1, 4096, dev)
    with pytest.raises(ValueError, match="beyond the entries' limit"):
        DepthCube(43, 2048, dev)
    cube = DepthCube(2, 8, dev)
    x, c = torch.zeros(2, 5, 3, device=dev), torch.full((2,), 5, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError, match="DepthCube.build: points must be a CUDA tensor"):
        cube.build(x.cpu(), c)
    with pytest.raises(ValueError, match="DepthCube.build: points must hold 2 samples"):
        cube.build(x[:1], c[:1])
    with pytest.raises(ValueError, match="DepthCube.build: count must be torch.int32"):
        cube.build(x, c.long())
    with pytest.raises(ValueError, match="DepthCube.build: mask must be an integer or bool CUDA tensor"):
        cube.build(x, c, torch.zeros(2, 5, device=dev))
    cube.build(x, c)
    for bad in (dict(halo=5), dict(halo=-1), dict(margin=-0.5), dict(rel=float("nan")), dict(near=float("inf"))):
        with pytest.raises(ValueError, match="DepthCube.seen_through: " + next(iter(bad))):
            cube.seen_through(x, c, **{**dict(halo=1, margin=0.5, rel=0.02, near=3.0), **bad})
    flag = torch.empty(2, 5, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="df_depth_cube_test failed: DF_E_ARG"):
        call("df_depth_cube_test", ptr(x), ptr(c), ptr(cube.img), 2, 5, 8, 5, 0.5, 0.02, 3.0, ptr(flag), None, s)
    with pytest.raises(RuntimeError, match="df_depth_cube_build failed: DF_E_SHAPE"):
        call("df_depth_cube_build", ptr(x), ptr(c), None, 2, 5, 6 + 1, ptr(cube.img), s)
