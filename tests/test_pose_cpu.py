"""tests/pose_ref.py -- the float64 restatement the GPU tests hold log_amd.pose's kernels to -- checked on its own: it is the
parametrisation the package documents, xi = 0 is the identity to the bit, the series and the closed forms of Rodrigues'
coefficients agree where the code switches, and autograd's derivative matches central differences."""
import numpy as np
import pytest
import torch

import pose_ref
from util import rel_l2, small_case


def _camera(view=1):
    cam, _ = small_case(view=view)
    return torch.tensor(cam["world_view_transform"]), torch.tensor(cam["full_proj_transform"]), cam


XIS = {"series": [0.03, -0.02, 0.04, 0.02, -0.01, 0.03],        # |omega|^2 = 2.9e-3 < SERIES
       "closed": [0.09, -0.08, 0.03, -0.02, 0.04, 0.01],        # |omega|^2 = 1.5e-2 > SERIES
       "large": [0.7, -0.4, 0.9, 0.3, -0.2, 0.5]}


def test_zero_row_is_the_identity_to_the_bit():
    for view in range(3):
        V, P, cam = _camera(view)
        Vn, Pn, cp = pose_ref.camera(torch.zeros(6), V, P)
        assert torch.equal(Vn.to(torch.float32), V) and torch.equal(Pn.to(torch.float32), P)
        assert rel_l2(cp.numpy(), cam["camera_center"]) < 1e-6


@pytest.mark.parametrize("name", list(XIS))
def test_it_is_the_documented_perturbation(name):
    """p_cam' = R(omega) p_cam + upsilon for every point, R a rotation by |omega| about omega; P' projects as P does in
    the perturbed frame; campos' is the point that V' sends to the origin."""
    V, P, _ = _camera()
    xi = torch.tensor(XIS[name], dtype=torch.float64)
    Vn, Pn, cp = pose_ref.camera(xi, V, P)
    V, P = V.double(), P.double()
    R = pose_ref.rotation_minus_identity(xi[:3]) + torch.eye(3, dtype=torch.float64)
    assert rel_l2((R @ R.t()).numpy(), np.eye(3)) < 1e-14 and abs(float(torch.det(R)) - 1) < 1e-14
    assert rel_l2((R @ xi[:3]).numpy(), xi[:3].numpy()) < 1e-14                      # the axis stays
    assert abs(float(torch.trace(R)) - (1 + 2 * np.cos(float(xi[:3].norm())))) < 1e-14   # the angle is |omega|
    p = torch.tensor(np.random.default_rng(0).standard_normal((20, 3)))
    h = torch.cat([p, torch.ones(20, 1, dtype=torch.float64)], dim=1)
    cam0, cam1 = (h @ V)[:, :3], (h @ Vn)[:, :3]
    assert rel_l2(cam1.numpy(), (cam0 @ R.t() + xi[3:]).numpy()) < 1e-13
    proj = pose_ref.rigid_inverse(V) @ P                                              # the projection alone
    assert rel_l2((h @ Pn).numpy(), (h @ Vn @ proj).numpy()) < 1e-6                   # (V^-1 of an fp32 V: orthonormal to 1e-7)
    assert float((torch.cat([cp, torch.ones(1, dtype=torch.float64)]) @ Vn)[:3].abs().max()) < 1e-6


def test_series_and_closed_form_agree_across_the_switch():
    for s in (pose_ref.SERIES * (1 - 1e-9), pose_ref.SERIES, pose_ref.SERIES * (1 + 1e-9), 1e-3, 1e-4):
        s = torch.tensor(s, dtype=torch.float64, requires_grad=True)
        out = []
        for series in (True, False):
            A, B = pose_ref.coefficients(s, series)
            dA, = torch.autograd.grad(A, s, retain_graph=True)
            dB, = torch.autograd.grad(B, s)
            out.append([float(A), float(B), float(dA), float(dB)])
        # values: neither form cancels, 1e-13; derivatives: autograd's closed forms are differences of terms of size 1 / s
        # that cancel to O(1): 1e-16 / s <= 1e-12 on this range, and the series' first dropped term is below 1e-16
        for (a, b), tol in zip(zip(*out), (1e-13, 1e-13, 1e-10, 1e-10)):
            assert abs(a - b) < tol * abs(b), (float(s), out)
    # the whole function on either side of the switch, each side in both forms: no step where the code changes form
    V, P, _ = _camera()
    d = torch.tensor([0.6, -0.48, 0.64, 0, 0, 0], dtype=torch.float64)   # unit axis
    for scale in (1 - 1e-9, 1 + 1e-9):
        xi = d * (pose_ref.SERIES ** 0.5) * scale
        assert bool(xi[:3].square().sum() < pose_ref.SERIES) == (scale < 1)
        for a, b in zip(pose_ref.camera(xi, V, P, series=True), pose_ref.camera(xi, V, P, series=False)):
            assert rel_l2(a.numpy(), b.numpy()) < 1e-14


@pytest.mark.parametrize("name", list(XIS) + ["zero"])
def test_derivative_matches_central_differences(name):
    V, P, _ = _camera()
    rng = np.random.default_rng(3)
    wV, wP, wc = (torch.tensor(rng.standard_normal(s)) for s in ((4, 4), (4, 4), (3,)))
    loss = lambda xi: sum((a * w).sum() for a, w in zip(pose_ref.camera(xi, V, P), (wV, wP, wc)))
    xi = torch.tensor(XIS.get(name, [0.0] * 6), dtype=torch.float64, requires_grad=True)
    g, = torch.autograd.grad(loss(xi), xi)
    fd = np.zeros(6)
    h = 1e-6
    for k in range(6):
        d = torch.zeros(6, dtype=torch.float64)
        d[k] = h
        fd[k] = float(loss(xi.detach() + d) - loss(xi.detach() - d)) / (2 * h)
    assert rel_l2(g.numpy(), fd) < 1e-8, (g, fd)
    assert float(g.abs().min()) > 0


def test_pose_table_has_no_cpu_fallback():
    from log_amd import _lib
    from log_amd.pose import PoseTable
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        PoseTable(4, "cpu", 1e-3, 1e-4)
