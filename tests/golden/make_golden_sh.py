"""Generates tests/golden/sh_basis.npz by RUNNING the reference's own SH evaluation (LoG/model/sh_utils.py: SH2RGB +
eval_sh_wobase, the colour of activation.py:27-34 before its clamp) on CPU, for the inputs of
tests/test_sh.py::_inputs(scale=0.2) at degrees 1..3 (build container only: needs the reference tree).

    LOG_REFERENCE=<LoG checkout> python tests/golden/make_golden_sh.py
"""
import os
import sys

import numpy as np
import torch

REF = os.environ["LOG_REFERENCE"]          # a checkout of the reference (LoG)
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

from LoG.model.sh_utils import SH2RGB, eval_sh_wobase   # noqa: E402  reference code, imported not copied


def main():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_sh import _inputs
    means, campos, shs = _inputs(scale=0.2)
    d = torch.tensor(means - campos[None])
    d = d / d.norm(dim=-1, keepdim=True)
    out = {}
    for degree in (1, 2, 3):
        ref = SH2RGB(torch.tensor(shs[:, 0])) + eval_sh_wobase(d, torch.tensor(shs[:, 1:]), degree=degree)
        out["colour_deg%d" % degree] = ref.numpy().astype(np.float32)
    path = os.path.join(HERE, "sh_basis.npz")
    np.savez_compressed(path, **out)
    print(path, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
