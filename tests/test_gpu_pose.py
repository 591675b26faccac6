"""log_amd.pose on the device: the two one-wave kernels against their float64 restatement (tests/pose_ref.py, checked on its
own by tests/test_pose_cpu.py), dL/dxi through PoseTable.camera and the rasterizer's camera gradients against pose_ref in front
of the float64 twin, the row step against the view-correction restatement at width 6, and a short fit."""
import numpy as np
import pytest
import torch

import camera_grad_cases as C
import pose_ref
import view_correction_ref as vref
from util import cam_tan, rel_l2, small_case

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4     # relative L2 against the reference, stated by BASELINE.json
ROUND_TOL = 1e-6    # a float64 result rounded once to fp32 (2^-24 per element) against the float64 restatement
DEV = "cuda:0"
XIS = {"zero": [0.0] * 6, "series": [0.03, -0.02, 0.04, 0.02, -0.01, 0.03], "closed": [0.09, -0.08, 0.03, -0.02, 0.04, 0.01],
       "large": [0.7, -0.4, 0.9, 0.3, -0.2, 0.5]}


def _table(views=4, lr=1e-3, **kw):
    from log_amd.pose import PoseTable
    return PoseTable(views, DEV, lr, lr, **kw)


def _matrices(view=1):
    cam, _ = small_case(view=view)
    return torch.tensor(cam["world_view_transform"]), torch.tensor(cam["full_proj_transform"])


@pytest.mark.parametrize("name", list(XIS))
def test_apply_and_backward_against_the_restatement(name):
    V, P = _matrices()
    pose = _table()
    row = 2
    pose.table[row] = torch.tensor(XIS[name], device=DEV)
    Vn, Pn, cp = pose.camera(row, V, P)
    xi = pose.table[row].cpu().double().requires_grad_(True)             # the fp32 row the kernel read
    rV, rP, rc = pose_ref.camera(xi, V, P)
    if name == "zero":
        assert torch.equal(Vn.cpu(), V) and torch.equal(Pn.cpu(), P)
    for got, want in ((Vn, rV), (Pn, rP), (cp, rc)):
        assert got.dtype == torch.float32 and got.requires_grad
        assert rel_l2(got.detach().cpu().numpy(), want.detach().numpy()) < ROUND_TOL
    rng = np.random.default_rng(5)
    w = [torch.tensor(rng.standard_normal(s), dtype=torch.float32) for s in ((4, 4), (4, 4), (3,))]
    want, = torch.autograd.grad(sum((a * b.double()).sum() for a, b in zip((rV, rP, rc), w)), xi)
    sum((a * b.to(DEV)).sum() for a, b in zip((Vn, Pn, cp), w)).backward()
    torch.cuda.synchronize()
    assert rel_l2(pose.grad[row].cpu().numpy(), want.numpy()) < ROUND_TOL
    assert not pose.grad[[0, 1, 3]].any()
    # a second backward ADDS into the row; a gradient that reaches one output only is that output's alone
    Vn2, Pn2, cp2 = pose.camera(row, V, P)
    (Pn2 * w[1].to(DEV)).sum().backward()
    want_p, = torch.autograd.grad((pose_ref.camera(xi, V, P)[1] * w[1].double()).sum(), xi)
    assert rel_l2(pose.grad[row].cpu().numpy(), (want + want_p).numpy()) < ROUND_TOL


def _render(c, V, P, dev=DEV):
    """The scene through the public package with the given matrices (device tensors, possibly with a graph)."""
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    cam, sc = c["cam"], c["sc"]
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    tfx, tfy = cam_tan(cam)
    rs = R.GaussianRasterizationSettings(cam["image_height"], cam["image_width"], tfx, tfy, t(C.BG), 1.0, V, P, 0,
                                         t(cam["camera_center"]), False, False)
    n = len(sc["xyz"])
    return wo.GaussianRasterizer(raster_settings=rs)(
        means3D=t(sc["xyz"]), means2D=torch.zeros(n, 3, device=dev), shs=None, colors_precomp=t(sc["colors"]),
        opacities=t(sc["opacity"]), scales=t(sc["scaling"]), rotations=t(sc["rotation"]), cov3D_precomp=None)[0]


def test_row_gradient_through_the_rasterizer_against_restatement_and_twin():
    c = C.SCENES["small-wodilate-filter"]()
    pose = _table(views=3)
    pose.table[1] = torch.tensor([0.01, -0.015, 0.008, 0.02, -0.01, 0.015], device=DEV)
    Vn, Pn, _ = pose.camera(1, torch.tensor(c["V"]), torch.tensor(c["P"]))
    image = _render(c, Vn, Pn)
    (image * torch.tensor(C.dL_of(c), device=DEV)).sum().backward()
    torch.cuda.synchronize()
    xi = pose.table[1].cpu().double().requires_grad_(True)
    rV, rP, _ = pose_ref.camera(xi, torch.tensor(c["V"]), torch.tensor(c["P"]))
    C.twin(c, V=rV, P=rP)                                               # (its backward runs through pose_ref to xi)
    e = rel_l2(pose.grad[1].cpu().numpy(), xi.grad.numpy())
    print(f"dL/dxi {e:.2e}")
    assert float(xi.grad.abs().min()) > 0 and e < GRAD_TOL, e
    assert not pose.grad[[0, 2]].any()                                  # untouched rows keep zero gradient


@pytest.mark.parametrize("start", [0, 3])
def test_step_is_the_corrector_step_at_width_six(start):
    """start = 3: the first call comes before start_step and moves only the row's count (the call with s = 0 is skipped
    here as in the view-correction tests: the reference's bias correction 1 - beta^0 divides by zero there)."""
    from log_amd.pose import PoseTable
    pose = PoseTable(3, DEV, 0.1, 0.001, start_step=start)
    rng = np.random.default_rng(6)
    state = ("table", "grad", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")
    for k in state:
        x = rng.standard_normal((3, 6)).astype(np.float32)
        getattr(pose, k).copy_(torch.tensor(np.abs(x) if k.endswith("sq") else x))
    snap = lambda: {k: getattr(pose, s).cpu().clone() for k, s in zip(vref.STATE, state)}
    if start:
        pose.steps[1] = 0
    for nth in range(2):
        before = snap()
        count = int(pose.steps[1])
        if start and nth == 1:
            pose.steps[1] = count = start              # past s = 0
        pose.step(1)
        after = snap()
        steps, want, S = vref.corrector_step({k: before[k][1] for k in vref.STATE}, count, start, 0.1, 0.001)
        _, want32, _ = vref.corrector_step({k: before[k][1] for k in vref.STATE}, count, start, 0.1, 0.001, dtype=torch.float32)
        assert pose.steps.tolist() == [0, steps, 0] and (want is None) == (start > 0 and nth == 0)
        for k in vref.STATE:
            assert torch.equal(after[k][[0, 2]], before[k][[0, 2]]), k
            if want is None:
                assert torch.equal(after[k][1], before[k][1]), k
            else:
                ok, ratio = vref.within(after[k][1], want32[k], want[k], S[k], 8.0)
                assert ok, (nth, k, ratio)
        if want is not None:
            assert not pose.grad[1].any()
            pose.grad[1] = torch.tensor(rng.standard_normal(6).astype(np.float32), device=DEV)


def test_twenty_steps_move_one_view_towards_its_target():
    """One view, 64x48, 300 Gaussians: the target is rendered with a known small xi*, the row starts at 0.  After twenty steps
    the loss is below the first one and the row is nearer to xi* than it started (a condition, not a measurement: the same
    fit in float64 with torch's Adam goes from 1.4e-3 to 7.6e-5 and from 0.047 to 0.033)."""
    cam, sc = small_case(n=300, W=64, H=48, focal=80.0, seed=4, opacity=None)
    c = C.case(cam, sc)
    V, P = torch.tensor(c["V"]), torch.tensor(c["P"])
    star = torch.tensor([0.01, -0.012, 0.008, 0.03, -0.02, 0.025], device=DEV)
    pose = _table(views=2, lr=1e-3)
    pose.table[0] = star
    with torch.no_grad():
        target = _render(c, *pose.camera(0, V, P)[:2]).clone()
    pose.table[0] = 0.0
    losses = []
    for _ in range(20):
        Vn, Pn, _ = pose.camera(0, V, P)
        loss = ((_render(c, Vn, Pn) - target) ** 2).mean()
        loss.backward()
        pose.step(0)
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu()
    dist = float((pose.table[0] - star).norm())
    print(f"loss {float(losses[0]):.3e} -> {float(losses[-1]):.3e}; |xi - xi*| {float(star.norm()):.4f} -> {dist:.4f}")
    assert float(losses[-1]) < float(losses[0]) and dist < float(star.norm())
    assert not pose.table[1].any() and pose.steps.tolist() == [20, 0]
