"""The C oracle's SH forward and backward held to the float64 twin at the shapes of tests/test_gpu_sh_edges.py (which holds
the HIP kernels to the oracle bit for bit there), and the seeds of those cases checked: tests/sh_edge_cases.py."""
import numpy as np
import pytest
import torch

import sh_edge_cases as E
from util import rel_l2


@pytest.mark.parametrize("M", E.MS)
def test_oracle_matches_the_float64_twin_at_the_edge_shapes(oracle_mod, M):
    """Bounds of test_sh.py::test_oracle_sh_backward_vs_autograd: colours 1e-6, dL/dshs 1e-5 (relative L2), dL/dmeans
    1e-4 * max.  The clamp mask equals the twin's wherever the float64 colour is further than 1e-5 from the clamp; at
    most 0.5 % of a case's channels are closer."""
    from oracle import torch_oracle
    left_out = 0
    for n, _, degree in E.cases(M):
        means, campos, shs, g = E.inputs(n, M, degree)
        col, clamped = oracle_mod.sh_forward(means, campos, shs, degree)
        r = E.twin_unclamped(means, campos, shs, degree)
        sure = np.abs(r) > E.NEAR_CLAMP
        assert (~sure).sum() <= E.MAX_NEAR_CLAMP * r.size, (n, M, degree)
        left_out += int((~sure).sum())
        assert ((clamped != 0) == (r < 0))[sure].all(), (n, M, degree)
        if degree > 0:                                              # both sides of the clamp in every case that can have them
            assert clamped.any() and not clamped.all(), (n, M, degree)
        else:
            assert not clamped.any()
        g_shs, g_means = oracle_mod.sh_backward(means, campos, shs, degree, clamped, g)
        tm = torch.tensor(means, dtype=torch.float64, requires_grad=True)
        ts = torch.tensor(shs, dtype=torch.float64, requires_grad=True)
        out = torch_oracle.sh_colors(tm, torch.tensor(campos, dtype=torch.float64), ts, degree)
        assert rel_l2(col, out.detach().numpy()) < 1e-6, (n, M, degree)
        (out * torch.tensor(g, dtype=torch.float64)).sum().backward()
        if sure.all():                                              # a channel at the clamp: its gradient is the mask's call
            assert rel_l2(g_shs, ts.grad.numpy()) < 1e-5, (n, M, degree)
            tmg = tm.grad.numpy() if tm.grad is not None else np.zeros_like(means)
            assert np.abs(g_means - tmg).max() <= 1e-4 * max(np.abs(tmg).max(), 1e-3), (n, M, degree)
        nk = (degree + 1) ** 2
        assert (g_shs[:, nk:] == 0).all()
    print("M = %d: %d channels within 1e-5 of the clamp" % (M, left_out))


def test_case_list_covers_both_copy_paths_and_every_admitted_degree():
    assert {M: E.degrees(M) for M in E.MS} == {1: [0], 4: [0, 1], 5: [0, 1], 9: [0, 1, 2], 12: [0, 1, 2], 16: [0, 1, 2, 3]}
    assert {M for M in E.MS if 3 * M % 4 == 0} == {4, 12, 16}
    assert sum(len(E.cases(M)) for M in E.MS) == 15 * len(E.NS)
