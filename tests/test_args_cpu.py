"""deflow_amd.args without a GPU: the one tensor check and the cloud check refuse what is no CUDA tensor with the documented TypeError,
the workspace rounds the query's bytes up to int32 elements and raises the caller's sentence, and the parameter checks are the same
functions under ``args`` and ``pairflow``."""
import numpy as np
import pytest
import torch

from deflow_amd import args, pairflow

NOT_CUDA = [torch.zeros(2, 5, 3), np.zeros((2, 5, 3), dtype=np.float32), None]
SENTENCE = r"op: x must be a CUDA tensor \(deflow_amd has no CPU fallback\)"


@pytest.mark.parametrize("t", NOT_CUDA, ids=["cpu", "numpy", "none"])
def test_tensor_and_cloud_refuse_what_is_no_cuda_tensor(t):
    with pytest.raises(TypeError, match="^" + SENTENCE + "$"):
        args.tensor("op", "x", t, torch.float32, (2, 5, 3))
    with pytest.raises(TypeError, match="^" + SENTENCE + "$"):
        args.tensor("op", "x", t)
    for limit in (None, 1, 3):
        with pytest.raises(TypeError, match="^" + SENTENCE + "$"):
            args.cloud("op", "x", t, limit)


def test_workspace_rounds_up_and_raises_the_callers_sentence(monkeypatch):
    asked = []
    answers = {"q0": 0, "q1": 1, "q5": 5, "qneg": -1}
    monkeypatch.setattr(args, "call", lambda name, *dims: (asked.append((name, dims)), answers[name])[1])
    for q, elements in (("q0", 1), ("q1", 1), ("q5", 2)):
        ws = args.workspace(q, (3, 7), "cpu", "never raised")
        assert ws.dtype == torch.int32 and ws.numel() == elements and ws.numel() * 4 >= answers[q]
    with pytest.raises(ValueError, match="^the caller's own sentence, B = 3$"):
        args.workspace("qneg", (3, 7), "cpu", "the caller's own sentence, B = 3")
    assert args.ws_bytes("q5", (1,), "never raised") == 5
    assert asked == [("q0", (3, 7)), ("q1", (3, 7)), ("q5", (3, 7)), ("qneg", (3, 7)), ("q5", (1,))]


def test_cluster_and_chamfer_refuse_a_numpy_array_with_the_type_error():
    from deflow_amd.chamfer import chamfer_nn
    from deflow_amd.cluster import dbscan, dynamic_cluster_labels
    p, n = np.zeros((1, 8, 3), dtype=np.float32), np.full((1,), 8, dtype=np.int32)
    with pytest.raises(TypeError, match=r"dbscan: points must be a CUDA tensor \(deflow_amd has no CPU fallback\)"):
        dbscan(p, n)
    with pytest.raises(TypeError, match=r"dbscan: points must be a CUDA tensor \(deflow_amd has no CPU fallback\)"):
        dynamic_cluster_labels(p, n, np.ones((1, 8), dtype=bool))
    with pytest.raises(TypeError, match=r"chamfer_nn: query must be a CUDA tensor \(deflow_amd has no CPU fallback\)"):
        chamfer_nn(p, n, p, n)


def test_the_parameter_checks_are_one_set_of_functions():
    for name in ("merged", "integer", "positive", "nonneg", "flag"):
        assert getattr(args, name) is getattr(pairflow, name), name
    out = args.merged("op", {"k": 1, "x": 0.5, "on": False}, {"k": 3.0})
    args.integer("op", out, "k", 1, 4), args.positive("op", out, "x"), args.nonneg("op", out, "x"), args.flag("op", out, "on")
    assert out == {"k": 3, "x": 0.5, "on": False} and isinstance(out["k"], int)
    for check, bad in ((lambda o: args.integer("op", o, "k", 1, 4), 5), (lambda o: args.positive("op", o, "k"), 0.0),
                       (lambda o: args.nonneg("op", o, "k"), -1.0), (lambda o: args.flag("op", o, "k"), 1)):
        with pytest.raises(ValueError, match="^op: k must be .*, got " + repr(bad).replace(".", r"\.") + "$"):
            check({"k": bad})
    with pytest.raises(ValueError, match="op: unknown parameter 'j'; known: k"):
        args.merged("op", {"k": 1}, {"j": 2})
