"""Child process of tests/test_gpu_decoder_bf16_cases.py::test_wave_forms_bit_identical: the lean decoder's waves-per-workgroup forms
(DF_GRU_WAVES, DF_GRU_FWD_WAVES; csrc/decoder4.hip) are read once per process, so each form runs in a process of its own.

    python tests/helpers/decoder_wave_child.py OUT.npz

runs the module step of tests/test_gpu_decoder_cases.py on the `edges` case under the environment it was started in, once in fp32
(bf16x2) mode and once under ops.mfma_bf16(True), and saves every tensor as "<mode>/<name>" (flow concatenated over the samples)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    sys.path.insert(0, p)
import decoder_cases as DC  # noqa: E402


def tensors(res):
    out = {"flow": torch.cat(res["flow"]), "d(before)": res["gbefore"], "d(after)": res["gafter"]}
    out.update({"grad " + k: g for k, g in res["gw"].items()})
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def main(path):
    from deflow_amd import ops
    from test_gpu_decoder_cases import _module_step
    dev, c, out = torch.device("cuda"), DC.case("edges"), {}
    for k, v in tensors(_module_step(c, dev)).items():
        out["fp32/" + k] = v
    with ops.mfma_bf16(True):
        res = _module_step(c, dev)
    for k, v in tensors(res).items():
        out["bf16/" + k] = v
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
