"""The fused L1 + SSIM loss on the device (log_amd.loss.l1_ssim_loss -> lograst_loss_forward / _backward) against

* the reference's own float64 results (tests/golden/loss_*.npz, written by tests/golden/make_golden_loss.py) and
* the float64 restatement tests/loss_ref.py (held to those results by tests/test_loss_cpu.py) at sizes no fixture has.

Tolerances.  A gradient is within rel-L2 1e-4 of float64 (the project's standing gradient tolerance) AND within 8 * gap32,
gap32 = the distance between the reference's own fp32 and float64 runs, stored in the fixtures by the generator: the HIP
kernels and the reference's fp32 run are two fp32 evaluations in different summation orders, so their errors add (x2), and
the largest gap over a handful of cases underestimates the tail (x4).  The three scalars are within 8 * max(gap32 over all
fixtures).  Inputs that are no fixture take the gap32 of the fixture made by the same recipe (named at each test).

The cases at the end of the file (other channel / batch counts, strides, weights, contents) take their yardstick from the
restatement itself, loss_ref(dtype=float32) on the same inputs: gradients by the same rule with that gap32; scalars within
8 * max(the fixtures' gap32, this input's own |fp32 - float64|) -- never tighter than the rule above, wider only where the
input's own fp32 evaluation is coarser than any fixture's (values outside [0, 1]); where the gradient is analytically zero
(render == gt) the 1e-4 cap, relative to a norm of 1e-17, is left out.  See _check_against_restatement."""
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
    rl = None if render_l1 is None else (render_l1.detach().clone() if render_l1.is_contiguous()
                                         else render_l1.detach()).requires_grad_(True)
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


# ---- shapes, strides and contents no fixture has: each against loss_ref in float64, the yardstick taken from
# ---- loss_ref(dtype=float32) on the same inputs ----------------------------------------------------------------------
def _pair(B, C, H, W, seed, lo=0.0, hi=1.0):
    """_image_pair's recipe for any channel count and value range."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    coarse = torch.rand(B, C, max(H // 8, 2), max(W // 8, 2), device=DEV, generator=g, dtype=torch.float64)
    field = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    noisy = lambda s: ((field + s * torch.randn(field.shape, device=DEV, generator=g, dtype=torch.float64)).clamp(0, 1)
                       * (hi - lo) + lo).float().contiguous()
    return noisy(0.05), noisy(0.08)


def _check_against_restatement(tag, render, gt, render_l1=None, a=0.2, b=0.8, zero_gradient=False):
    """Scalars: within 8 * the larger of the fixtures' gap32 and this input's own |fp32 - float64| (values beyond [0, 1]
    round coarser than any fixture's).  Gradients: the file's rule, rel-L2 <= min(1e-4, 8 * gap32), with gap32 = rel-L2 of
    loss_ref(dtype=float32) to loss_ref(float64) on these inputs -- written without the division, so that it also holds
    where the gradient is analytically zero (zero_gradient: render == gt, a maximum of SSIM and the kink of L1; the 1e-4 cap
    is relative to a norm that is rounding noise there and is left out)."""
    ref = loss_ref.loss_ref(render, gt, render_l1, a, b)
    ref32 = loss_ref.loss_ref(render, gt, render_l1, a, b, dtype=torch.float32)
    scalars, g, gl, _ = _run(render, gt, render_l1, a, b)
    gaps = _gaps()
    for k, got in zip(("loss", "l1", "ssim"), scalars):
        err, bound = abs(got - ref[k]), FACTOR * max(gaps[k], abs(ref32[k] - ref[k]))
        print(f"{tag} {k}: |{got:.9f} - {ref[k]:.9f}| = {err:.3e} <= {bound:.3e}")
        assert err <= bound, (tag, k, err, bound)
    norm = lambda t: float(torch.linalg.norm(t.double()))
    for name, got, want, want32 in (("grad_render", g, ref["grad_render"], ref32["grad_render"]),
                                    ("grad_render_l1", gl, ref["grad_render_l1"], ref32["grad_render_l1"])):
        if want is None:
            assert got is None
            continue
        assert torch.isfinite(got).all()
        err, gap, n64 = norm(got.double() - want), norm(want32.double() - want), norm(want)
        bound = FACTOR * gap if zero_gradient else min(GRAD_TOL * n64, FACTOR * gap)
        print(f"{tag} {name}: |hip - ref64| {err:.3e} <= {bound:.3e} (|ref32 - ref64| {gap:.3e}, |ref64| {n64:.3e})")
        assert err <= bound, (tag, name, err, bound)
    return scalars, g, gl


@pytest.mark.parametrize("B,C,H,W", [(3, 1, 64, 80), (5, 4, 50, 70), (5, 1, 43, 44), (3, 4, 33, 75)])
def test_other_channel_and_batch_counts(B, C, H, W):
    render, gt = _pair(B, C, H, W, 10 * B + C)
    _check_against_restatement(f"B={B} C={C}", render, gt)
    _check_against_restatement(f"B={B} C={C} render_l1", render, gt, (render * 1.03 + 0.01).contiguous())


def test_render_l1_as_a_channel_slice_of_a_four_channel_tensor():
    """calculate_loss passes output["render_correct"][:, :3]: rows of 3 channels out of 4, at 270x480."""
    render, gt = _pair(2, 3, 270, 480, 21)
    g = torch.Generator(device=DEV).manual_seed(22)
    four = torch.rand(2, 4, 270, 480, device=DEV, generator=g)
    four[:, :3] = (render * 0.97 + 0.02)
    rl = four[:, :3]
    assert not rl.is_contiguous() and rl.stride()[0] == 4 * 270 * 480
    s_v, g_v, gl_v = _check_against_restatement("render_l1 = [:, :3]", render, gt, rl)
    s_c, g_c, gl_c, _ = _run(render, gt, rl.contiguous())
    assert s_v == s_c and torch.equal(g_v, g_c) and torch.equal(gl_v, gl_c)          # strides change nothing


def test_gt_expanded_over_the_batch_and_cropped_views():
    render, gt = _pair(3, 3, 96, 130, 31)
    gt_e = gt[:1].expand(3, -1, -1, -1)
    assert gt_e.stride()[0] == 0
    s_v, g_v, _ = _check_against_restatement("gt stride 0", render, gt_e)
    s_c, g_c, _, _ = _run(render, gt_e.contiguous())
    assert s_v == s_c and torch.equal(g_v, g_c)
    # W- and H-cropped views of larger tensors (all three inputs)
    big_r, big_g = _pair(2, 3, 140, 200, 32)
    crop = (slice(None), slice(None), slice(9, 9 + 75), slice(13, 13 + 131))
    r_v, g_v_, rl_v = big_r[crop], big_g[crop], (big_r * 1.02)[crop]
    assert not r_v.is_contiguous() and r_v.stride()[2] == 200
    s_v, gr_v, gl_v = _check_against_restatement("cropped views", r_v, g_v_, rl_v)
    s_c, gr_c, gl_c, _ = _run(r_v.contiguous(), g_v_.contiguous(), rl_v.contiguous())
    assert s_v == s_c and torch.equal(gr_v, gr_c) and torch.equal(gl_v, gl_c)


@pytest.mark.parametrize("a,b", [(1.0, 0.0), (0.0, 1.0), (0.5, 0.5)])
def test_other_weights(a, b):
    render, gt = _pair(2, 3, 75, 131, 41)
    _check_against_restatement(f"weights ({a}, {b})", render, gt, None, a, b)
    _check_against_restatement(f"weights ({a}, {b}) render_l1", render, gt, (render * 1.03).contiguous(), a, b)


def test_inputs_outside_the_unit_interval():
    render, gt = _pair(2, 3, 64, 96, 51, lo=-1.5, hi=3.0)
    assert float(render.min()) < -0.5 and float(render.max()) > 2.0
    _check_against_restatement("[-1.5, 3]", render, gt)


def test_constant_images_and_equal_images():
    ones = torch.ones(2, 3, 48, 60, device=DEV)
    level = lambda vals: (ones * torch.tensor(vals, device=DEV).view(1, 3, 1, 1)).contiguous()
    _check_against_restatement("constant, different", level([0.3, 0.5, 0.9]), level([0.6, 0.5, 0.1]))
    _check_against_restatement("constant, black and white", level([0.0, 0.0, 1.0]), level([1.0, 0.0, 1.0]))
    render, _ = _pair(2, 3, 48, 60, 61)
    scalars, g, _ = _check_against_restatement("render == gt", render, render.clone(), zero_gradient=True)
    assert scalars[1] == 0.0                                    # |x - x| sums to exactly 0
