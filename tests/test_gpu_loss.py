"""The fused L1 + SSIM loss on the device (log_amd.loss.l1_ssim_loss -> lograst_loss_forward / _backward) against

* the reference's own float64 results (tests/golden/loss_*.npz, written by tests/golden/make_golden_loss.py) and
* the float64 restatement tests/loss_ref.py (held to those results by tests/test_loss_cpu.py) at sizes no fixture has.

Tolerances.  A gradient is within rel-L2 1e-4 of float64 (the project's standing gradient tolerance) AND within 8 * gap32,
gap32 = the distance between the reference's own fp32 and float64 runs, stored in the fixtures by the generator: the HIP
kernels and the reference's fp32 run are two fp32 evaluations in different summation orders, so their errors add (x2), and
the largest gap over a handful of cases underestimates the tail (x4).  The three scalars are within 8 * max(gap32 over all
fixtures).  Inputs that are no fixture take the gap32 of the fixture made by the same recipe (named at each test)."""
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import loss_ref  # noqa: E402
from loss_ref import load_case, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "loss_*.npz")))
IDS = [os.path.basename(p)[5:-4] for p in GOLDEN]
DEV = "cuda:0"
GRAD_TOL = 1e-4
FACTOR = 8.0


def _gaps():
    zs = [np.load(p) for p in GOLDEN]
    return {k: max(float(z["gap32_" + k]) for z in zs) for k in ("l1", "ssim", "loss")}


def _gap_of(name):
    return float(np.load(os.path.join(HERE, "golden", "loss_%s.npz" % name))["gap32_grad_render"])


def _run(render, gt, render_l1=None, a=0.2, b=0.8, upstream=None):
    """-> (loss, l1, ssim as python floats via ONE transfer; grad_render; grad_render_l1 or None; the raw 0-dim tensors)"""
    from log_amd.loss import l1_ssim_loss
    r = render.detach().clone().requires_grad_(True) if render.is_contiguous() else render.detach().requires_grad_(True)
    rl = None if render_l1 is None else render_l1.detach().clone().requires_grad_(True)
    loss, l1, ssim = l1_ssim_loss(r, gt, rl, a, b)
    assert loss.requires_grad and not l1.requires_grad and not ssim.requires_grad
    assert loss.dim() == 0 and l1.dim() == 0 and ssim.dim() == 0 and loss.is_cuda
    (loss if upstream is None else upstream * loss).backward()
    return (float(loss), float(l1), float(ssim)), r.grad, None if rl is None else rl.grad, (loss.detach(), l1, ssim)


def _check_scalars(got, want, tag):
    gaps = _gaps()
    for k, g, w in zip(("loss", "l1", "ssim"), got, want):
        err, bound = abs(g - w), FACTOR * gaps[k]
        print(f"{tag} {k}: |{g:.9f} - {w:.9f}| = {err:.3e} <= {bound:.3e}")
        assert err <= bound, (tag, k, err, bound)


def _check_grad(got, want, gap32, tag):
    err, bound = rel_l2(got.cpu(), want.cpu()), min(GRAD_TOL, FACTOR * gap32)
    print(f"{tag} grad rel-L2 {err:.3e} <= {bound:.3e} (gap32 {gap32:.3e})")
    assert torch.isfinite(got).all()
    assert err <= bound, (tag, err, bound)


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_golden_cases(path):
    c = load_case(path)
    render, gt = c["render"].to(DEV), c["gt"].to(DEV)          # .to keeps the permuted (channels-last) strides of gt
    if "gt_nhwc" in c:
        assert gt.stride()[1] == 1 and not gt.is_contiguous()
    rl = None if c["render_l1"] is None else c["render_l1"].to(DEV)
    scalars, g, gl, _ = _run(render, gt, rl)
    _check_scalars(scalars, [float(c[k + "64"]) for k in ("loss", "l1", "ssim")], IDS[GOLDEN.index(path)])
    _check_grad(g, torch.from_numpy(c["grad_render64"]), float(c["gap32_grad_render"]), IDS[GOLDEN.index(path)])
    if rl is not None:
        _check_grad(gl, torch.from_numpy(c["grad_render_l164"]), float(c["gap32_grad_render_l1"]), "render_l1")
    if "half_equal" in path:          # render == gt on the left half: the L1 term is exactly 0 there (sign(0) = 0)
        only_l1 = _run(render, gt, None, 0.0, 1.0)[1]
        assert float(only_l1[..., :24].abs().max()) == 0.0 and float(only_l1[..., 24:].abs().max()) > 0.0


def _image_pair(B, H, W, seed):
    """The recipe of fixture nhwc_64x96 (a smooth field, render and gt = field + noise, clipped) at any size, on the device."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    coarse = torch.rand(B, 3, max(H // 8, 2), max(W // 8, 2), device=DEV, generator=g, dtype=torch.float64)
    field = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    render = (field + 0.05 * torch.randn(field.shape, device=DEV, generator=g, dtype=torch.float64)).clamp(0, 1).float()
    gt = (field + 0.08 * torch.randn(field.shape, device=DEV, generator=g, dtype=torch.float64)).clamp(0, 1).float()
    return render.contiguous(), gt.contiguous()


@pytest.fixture(scope="module")
def full_hd():
    """1920x1080, B = 2: inputs and the float64 restatement of the whole batch and of its first image (computed once)."""
    render, gt = _image_pair(2, 1080, 1920, 5)
    ref2 = loss_ref.loss_ref(render, gt)
    ref1 = loss_ref.loss_ref(render[:1], gt[:1])
    torch.cuda.synchronize()
    return render, gt, {1: ref1, 2: ref2}


@pytest.mark.parametrize("B", [1, 2])
def test_full_hd_against_restatement(full_hd, B):
    render, gt, refs = full_hd
    render, gt, ref = render[:B], gt[:B], refs[B]
    gt_cl = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # [B,H,W,3] permuted, as LoG's batch['image']
    assert gt_cl.stride()[1] == 1
    gap = _gap_of("nhwc_64x96")                                          # same recipe (see _image_pair)
    s_c, g_c, _, t_c = _run(render, gt)
    s_l, g_l, _, t_l = _run(render, gt_cl)
    for tag, s, g in (("contiguous", s_c, g_c), ("channels-last", s_l, g_l)):
        _check_scalars(s, [ref[k] for k in ("loss", "l1", "ssim")], f"1080p B={B} {tag}")
        _check_grad(g, ref["grad_render"], gap, f"1080p B={B} {tag}")
    assert torch.equal(g_c, g_l) and all(torch.equal(x, y) for x, y in zip(t_c, t_l))


def test_two_calls_are_bit_identical(full_hd):
    render, gt, _ = full_hd
    for r, g, rl in ((render, gt, None), (render[:1], gt[:1], (render[:1] * 1.05).contiguous())):
        a, b = _run(r, g, rl), _run(r, g, rl)
        assert all(torch.equal(x, y) for x, y in zip(a[3], b[3]))
        assert torch.equal(a[1], b[1]) and (rl is None or torch.equal(a[2], b[2]))


@pytest.mark.parametrize("H", [11, 12, 42, 43])
@pytest.mark.parametrize("W", [11, 12, 42, 43])
def test_sizes_at_the_tile_edges(H, W):
    """11 = one output pixel, T + 10 = exactly one tile, T + 11 = a second tile of one column / row (T = loss.TILE);
    uniform random inputs as fixture 1x11x11, whose gap32 applies."""
    from log_amd import loss
    assert loss.TILE + 10 == 42
    g = torch.Generator(device=DEV).manual_seed(H * 100 + W)
    render, gt = torch.rand(1, 3, H, W, device=DEV, generator=g), torch.rand(1, 3, H, W, device=DEV, generator=g)
    ref = loss_ref.loss_ref(render, gt)
    s, gr, _, _ = _run(render, gt)
    _check_scalars(s, [ref[k] for k in ("loss", "l1", "ssim")], f"{H}x{W}")
    _check_grad(gr, ref["grad_render"], _gap_of("1x11x11"), f"{H}x{W}")


def test_upstream_gradient_and_reuse():
    from log_amd.loss import l1_ssim_loss
    render, gt = _image_pair(1, 75, 131, 9)
    gap = _gap_of("nhwc_64x96")
    ref = loss_ref.loss_ref(render, gt, upstream=3.0)
    _check_grad(_run(render, gt, upstream=3.0)[1], ref["grad_render"], gap, "3 * loss")
    # the loss used twice in one graph: d(loss^2 + 2 loss)/d render = (2 loss + 2) * d loss / d render
    r = render.clone().requires_grad_(True)
    loss = l1_ssim_loss(r, gt)[0]
    (loss * loss + 2.0 * loss).backward()
    one = loss_ref.loss_ref(render, gt)
    _check_grad(r.grad, (2.0 * one["loss"] + 2.0) * one["grad_render"], gap, "loss used twice")
    # ssim alone = weights (1, 0)
    from log_amd.loss import ssim
    assert abs(float(ssim(render, gt)) - one["ssim"]) <= FACTOR * _gaps()["ssim"]
    # no gradient asked: forward only
    assert not l1_ssim_loss(render, gt)[0].requires_grad


def test_into_the_rasterizer():
    """The scene of __graft_entry__.smoke() rendered by the drop-in package; loss.backward() gives the Gaussians the
    gradients that image.backward(gradient = the float64 restatement's dL/dimage, cast to fp32) gives them."""
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    from log_amd import scenes
    from log_amd.loss import l1_ssim_loss
    dev = torch.device(DEV)
    cam = scenes.orbit_cameras(3, W=160, H=96, focal=180.0)[1]
    sc = scenes.random_scene(3000, seed=3, opacity=None, smax=0.06)
    T = lambda a, g=True: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=g)
    rs = GaussianRasterizationSettings(
        image_height=96, image_width=160, tanfovx=math.tan(cam["FoVx"] * 0.5), tanfovy=math.tan(cam["FoVy"] * 0.5),
        bg=T([0.2, 0.5, 0.8], False), scale_modifier=1.0, viewmatrix=T(cam["world_view_transform"], False),
        projmatrix=T(cam["full_proj_transform"], False), sh_degree=0, campos=T(cam["camera_center"], False),
        prefiltered=False, debug=False)
    rast = GaussianRasterizer(raster_settings=rs)
    gt = torch.rand(1, 96, 160, 3, device=dev, generator=torch.Generator(device=DEV).manual_seed(2)).permute(0, 3, 1, 2)
    names = ("xyz", "scaling", "rotation", "opacity", "colors")
    grads = []
    for fused in (True, False):
        m3, sca, rot, op, col = (T(sc[k]) for k in names)
        m2 = torch.zeros_like(m3, requires_grad=True)
        image = rast(means3D=m3, means2D=m2, shs=None, colors_precomp=col, opacities=op, scales=sca, rotations=rot,
                     cov3D_precomp=None)[0]
        if fused:
            l1_ssim_loss(image[None], gt)[0].backward()
        else:
            image.backward(gradient=loss_ref.loss_ref(image[None], gt)["grad_render"][0].float())
        grads.append([t.grad.clone() for t in (m3, sca, rot, op, col, m2)])
    for name, a, b in zip(names + ("means2D",), *grads):
        err = rel_l2(a.cpu(), b.cpu())
        print(f"{name}: rel-L2 {err:.3e}")
        assert float(b.abs().sum()) > 0 and err <= GRAD_TOL, (name, err)


def test_graph_capture_replays_the_eager_result():
    from log_amd.loss import l1_ssim_loss
    render, gt = _image_pair(1, 270, 480, 4)
    gt = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    _, g_eager, _, t_eager = _run(render, gt)
    r = render.clone().requires_grad_(True)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):                       # warm-up on the capture stream
        l1_ssim_loss(r, gt)[0].backward()
    torch.cuda.synchronize()
    r.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        loss, l1, ssim = l1_ssim_loss(r, gt)
        loss.backward()
    torch.cuda.synchronize()
    for _ in range(2):
        r.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip((loss.detach(), l1, ssim), t_eager))
        assert torch.equal(r.grad, g_eager)


def test_profile_slots_time_the_new_kernels():
    from log_amd import _lib
    render, gt = _image_pair(1, 64, 64, 1)
    _lib.profile_enable(True)
    _lib.profile_reset()
    try:
        _run(render, gt)
        prof = _lib.profile_read()
    finally:
        _lib.profile_enable(False)
    assert prof["loss_fwd"][1] == 1 and prof["loss_bwd"][1] == 1
