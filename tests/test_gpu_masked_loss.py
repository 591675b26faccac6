"""The masked training loss on the device (log_amd.masked_loss -> lograst_loss_*_masked, lograst_mask_bounds*).

* Bit identity.  The blend and the composite are the fp32 operations of the torch expressions around log_amd.loss, so an
  ignore mask gives the bits of ``l1_ssim_loss(gt * m + render * (1 - m), gt)`` taken through autograd, and a foreground
  mask the bits of the unmasked kernels on the torch composite: no tolerance.
* The reference's own results (tests/golden/fgmask_*.npz: MaskForeground.forward on the CPU in fp32 and float64) by the
  rules of tests/test_gpu_loss.py: scalars within 8 * the largest gap32 over the fixtures, gradients rel-L2 within
  min(1e-4, 8 * gap32) of float64.
* Gain with a mask, and the full-size crop: against tests/masked_loss_ref.py in float64, the yardstick its own float32
  evaluation of the same inputs (test_gpu_loss._check_against_restatement's rule): scalars within 8 * max(the fixtures'
  gap32, this input's |fp32 - float64|), gradients |hip - ref64| <= min(1e-4 |ref64|, 8 |ref32 - ref64|); the gain's gradient
  per element within 8 * (|ref32 - ref64| + 2^-24 * S), S its condition scale (tests/view_correction_ref.within).
* The bounds: exact integers against numpy.
* The drop-in MaskForeground.forward on stand-in renderer and model classes (the reference is not needed on the device).
* Which of the six C entry points each kind of input calls, forward and backward, counted."""
import glob
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import masked_loss_ref as mref  # noqa: E402
import view_correction_ref as vref  # noqa: E402
from loss_ref import rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "fgmask_*.npz")))
IDS = [os.path.basename(p)[len("fgmask_"):-4] for p in GOLDEN]
DEV = "cuda:0"
GRAD_TOL, FACTOR = 1e-4, 8.0


def _gaps():
    zs = [np.load(p) for p in GOLDEN]
    return {k: max(float(z["gap32_" + k]) for z in zs) for k in ("l1", "ssim", "loss")}


def _leaf(t):
    return None if t is None else t.detach().requires_grad_(True)


def _masked(render, gt, mask=None, render_l1=None, foreground=None, background=None, gain=None, a=0.2, b=0.8):
    """-> ((loss, l1, ssim) 0-dim tensors, grad_render, grad_render_l1 or None, grad_gain or None, gt_used)"""
    from log_amd.masked_loss import masked_l1_ssim_loss
    r, rl, k = _leaf(render), _leaf(render_l1), _leaf(gain)
    loss, l1, ssim, gt_used = masked_l1_ssim_loss(r, gt, mask, foreground, background, rl, k, a, b)
    assert loss.requires_grad and not l1.requires_grad and not ssim.requires_grad and not gt_used.requires_grad
    assert loss.dim() == 0 and l1.dim() == 0 and ssim.dim() == 0 and loss.is_cuda
    loss.backward()
    return (loss.detach(), l1, ssim), r.grad, None if rl is None else rl.grad, None if k is None else k.grad, gt_used


def _torch_blend(render, gt, mask, render_l1=None):
    """The path as it is without this module: the torch blend, then the unmasked kernels, autograd back to render."""
    from log_amd.loss import l1_ssim_loss
    r, rl = _leaf(render), _leaf(render_l1)
    x = r if mask is None else gt * mask[:, None] + r * (1 - mask[:, None])
    loss, l1, ssim = l1_ssim_loss(x, gt, rl)
    loss.backward()
    return (loss.detach(), l1, ssim), r.grad, None if rl is None else rl.grad


def _same(a, b, tag):
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y), (tag, float(x), float(y))
    assert torch.equal(a[1], b[1]), (tag, "grad_render", float((a[1] - b[1]).abs().max()))
    assert (a[2] is None) == (b[2] is None) and (a[2] is None or torch.equal(a[2], b[2])), (tag, "grad_render_l1")


def _inputs(B, C, H, W, seed, views=False):
    """render, gt, render_l1, four masks (random in [0, 1], binary, zeros, ones); views: every tensor a crop at an odd
    offset of a larger one, gt channels-last."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    pad = (3, 5) if views else (0, 0)
    full = (H + pad[0] + 2, W + pad[1] + 4) if views else (H, W)
    rand = lambda *s: torch.rand(*s, device=DEV, generator=g)
    cut = lambda t: t[..., pad[0]:pad[0] + H, pad[1]:pad[1] + W]
    render, render_l1 = cut(rand(B, C, *full)), cut(rand(B, C, *full))
    gt = cut(rand(B, *full, C).permute(0, 3, 1, 2)) if views else rand(B, C, H, W)
    soft = cut(rand(B, *full))
    masks = {"random": soft, "binary": cut((rand(B, *full) > 0.5).float()), "zeros": cut(torch.zeros(B, *full, device=DEV)),
             "ones": cut(torch.ones(B, *full, device=DEV))}
    if views:
        assert not render.is_contiguous() and gt.stride()[1] == 1 and not soft.is_contiguous()
    return render, gt, render_l1, masks


SHAPES = [(1, 3, H, W) for H in (11, 12, 42, 43) for W in (11, 12, 42, 43)] + [(2, 3, 37, 53), (1, 1, 37, 53)]


@pytest.mark.parametrize("B,C,H,W", SHAPES, ids=["%dx%dx%dx%d" % s for s in SHAPES])
def test_an_ignore_mask_gives_the_bits_of_the_torch_blend(B, C, H, W):
    from log_amd.loss import l1_ssim_loss
    for views in (False, True):
        render, gt, render_l1, masks = _inputs(B, C, H, W, 1000 * H + W + B, views)
        for name, m in masks.items():
            tag = f"{name} views={views}"
            got = _masked(render, gt, m)
            _same(got, _torch_blend(render, gt, m), tag)
            assert got[4] is gt
            _same(_masked(render, gt, m, render_l1), _torch_blend(render, gt, m, render_l1), tag + " render_l1")
            if name == "zeros":                          # ... and the plain unmasked call
                _same(got, _torch_blend(render, gt, None), tag + " unmasked")
            if name == "ones":
                assert float(got[1].abs().max()) == 0.0 and float(got[0][1]) == 0.0
        r = render.detach().requires_grad_(True)
        assert torch.equal(l1_ssim_loss(r, gt)[0], _masked(render, gt, masks["zeros"])[0][0])


@pytest.mark.parametrize("B,C,H,W", [(1, 3, 11, 11), (1, 3, 42, 43), (1, 3, 43, 42), (2, 3, 37, 53), (1, 1, 37, 53)])
def test_the_composite_gives_the_bits_of_the_unmasked_kernels_on_the_torch_composite(B, C, H, W):
    for views in (False, True):
        render, gt, render_l1, masks = _inputs(B, C, H, W, 77 * H + W, views)
        bg = torch.rand(C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(H))
        for name in ("random", "binary", "zeros", "ones"):
            f = masks[name]
            want_gt = gt * f[:, None] + (1 - f[:, None]) * bg[None, :, None, None]
            got = _masked(render, gt, foreground=f, background=bg)
            assert torch.equal(got[4], want_gt) and got[4].is_contiguous() and got[4].shape == gt.shape, name
            _same(got, _torch_blend(render, want_gt, None), f"composite {name} views={views}")
            _same(_masked(render, gt, None, render_l1, f, bg), _torch_blend(render, want_gt, None, render_l1), name + " render_l1")
            # composite and blend together
            m = masks["random"].flip(-1)
            both = _masked(render, gt, m, None, f, bg)
            assert torch.equal(both[4], want_gt)
            _same(both, _torch_blend(render, want_gt, m), f"composite {name} + blend views={views}")
            _same(_masked(render, gt, m, render_l1, f, bg), _torch_blend(render, want_gt, m, render_l1), name + " both render_l1")


def test_inputs_that_need_a_gradient_or_do_not_fit_raise():
    from log_amd import _lib
    from log_amd.masked_loss import masked_l1_ssim_loss
    render, gt, _, masks = _inputs(1, 3, 16, 17, 3)
    m, bg = masks["random"], torch.rand(3, device=DEV)
    for kw in (dict(gt=gt.clone().requires_grad_(True), mask=m), dict(gt=gt, mask=m.clone().requires_grad_(True)),
               dict(gt=gt, foreground=m.clone().requires_grad_(True), background=bg),
               dict(gt=gt, foreground=m, background=bg.clone().requires_grad_(True))):
        with pytest.raises(_lib.LograstError, match="gets no gradient"):
            masked_l1_ssim_loss(render, **kw)
    with pytest.raises(ValueError, match="mask: expected a float32 tensor"):
        masked_l1_ssim_loss(render, gt, mask=m[:, :-1])
    with pytest.raises(ValueError, match="background"):
        masked_l1_ssim_loss(render, gt, foreground=m, background=torch.rand(4, device=DEV))
    assert not masked_l1_ssim_loss(render, gt, mask=m)[0].requires_grad           # no gradient asked: forward only


# ---- the reference's recorded results --------------------------------------------------------------------------------

def _check_fixture(c, scalars, grad, tag):
    gaps = _gaps()
    for k, got in zip(("loss", "l1", "ssim"), scalars):
        err, bound = abs(float(got) - float(c[k + "64"])), FACTOR * gaps[k]
        print(f"{tag} {k}: |{float(got):.9f} - {float(c[k + '64']):.9f}| = {err:.3e} <= {bound:.3e}")
        assert err <= bound, (tag, k, err, bound)
    gap32 = float(c["gap32_grad_render"])
    err, bound = rel_l2(grad.cpu(), torch.from_numpy(c["grad_render64"])), min(GRAD_TOL, FACTOR * gap32)
    print(f"{tag} grad rel-L2 {err:.3e} <= {bound:.3e} (gap32 {gap32:.3e})")
    assert torch.isfinite(grad).all() and err <= bound, (tag, err, bound)


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_golden_cases(path):
    c = mref.load_case(path)
    for k in ("image", "mask", "render", "background", "mask_ignore"):
        c[k] = None if c[k] is None else c[k].to(DEV)
    render, gt, fg, mi = mref.cropped_inputs(c)
    assert list(render.shape) == c["crop_shape"].tolist() and render.storage_offset() == int(c["crop_offset"])
    assert gt.stride()[1] == 1
    scalars, grad, _, _, gt_used = _masked(render, gt, mi, None, fg, c["background"])
    assert torch.equal(gt_used.cpu(), torch.from_numpy(c["gt32"]))          # the same three fp32 operations per element
    _check_fixture(c, scalars, grad, IDS[GOLDEN.index(path)])


# ---- against the restatement ----------------------------------------------------------------------------------------

def _smooth_pair(B, H, W, seed):
    """test_gpu_loss._image_pair's recipe: a smooth field, render and gt = field + noise, clipped."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    coarse = torch.rand(B, 3, max(H // 8, 2), max(W // 8, 2), device=DEV, generator=g, dtype=torch.float64)
    field = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)
    render = (field + 0.05 * torch.randn(field.shape, device=DEV, generator=g, dtype=torch.float64)).clamp(0, 1).float()
    gt = (field + 0.08 * torch.randn(field.shape, device=DEV, generator=g, dtype=torch.float64)).clamp(0, 1).float()
    return render.contiguous(), gt.contiguous(), g


def _check_against_restatement(tag, got, ref, ref32, render=None):
    scalars, grad, _, grad_gain, _ = got
    gaps = _gaps()
    for k, s in zip(("loss", "l1", "ssim"), scalars):
        err, bound = abs(float(s) - ref[k]), FACTOR * max(gaps[k], abs(ref32[k] - ref[k]))
        print(f"{tag} {k}: |{float(s):.9f} - {ref[k]:.9f}| = {err:.3e} <= {bound:.3e}")
        assert err <= bound, (tag, k, err, bound)
    norm = lambda t: float(torch.linalg.norm(t.double()))
    want, want32 = ref["grad_render"], ref32["grad_render"]
    err, gap, n64 = norm(grad.double() - want), norm(want32.double() - want), norm(want)
    bound = min(GRAD_TOL * n64, FACTOR * gap)
    print(f"{tag} grad_render: |hip - ref64| {err:.3e} <= {bound:.3e} (|ref32 - ref64| {gap:.3e}, |ref64| {n64:.3e})")
    assert torch.isfinite(grad).all() and err <= bound, (tag, err, bound)
    if ref["grad_gain"] is not None:
        B, C, H, W = render.shape
        S = 0.8 / (B * C * H * W) * render.double().abs().sum(dim=(2, 3))
        ok, ratio = vref.within(grad_gain, ref32["grad_gain"], ref["grad_gain"], S)
        print(f"{tag} grad_gain: largest error / bound {ratio:.3f}")
        assert ok, (tag, ratio)


def test_gain_with_a_mask_against_the_restatement():
    """One call with gain and mask (what view_correction's calculate_loss makes with the switch on); the two-call path it
    replaces rounds the weighted sum differently, so the comparison is with float64."""
    render, gt, g = _smooth_pair(2, 37, 53, 11)
    mask = torch.rand(2, 37, 53, device=DEV, generator=g)
    mask[:, 5:20, 10:30] = 1.0
    gain = torch.tensor([[1.1, 0.93, 1.04], [0.9, 1.02, 1.2]], device=DEV)
    got = _masked(render, gt, mask, gain=gain)
    ref = mref.masked_loss(render, gt, mask, gain=gain)
    ref32 = mref.masked_loss(render, gt, mask, gain=gain, dtype=torch.float32)
    _check_against_restatement("gain + mask", got, ref, ref32, render)
    assert float(got[1][:, :, 5:20, 10:30].abs().max()) > 0          # ignored pixels keep the gain's L1 term, as the reference
    again = _masked(render, gt, mask, gain=gain)
    assert all(torch.equal(x, y) for x, y in zip(got[0], again[0])) and torch.equal(got[1], again[1]) and torch.equal(got[3], again[3])
    # ... and with a composite as well
    fg, bg = (torch.rand(2, 37, 53, device=DEV, generator=g) > 0.3).float(), torch.tensor([0.2, 0.5, 0.8], device=DEV)
    got = _masked(render, gt, mask, None, fg, bg, gain)
    _check_against_restatement("gain + mask + composite", got, mref.masked_loss(render, gt, mask, fg, bg, gain=gain),
                               mref.masked_loss(render, gt, mask, fg, bg, gain=gain, dtype=torch.float32), render)
    got = _masked(render, gt, None, None, fg, bg, gain)
    _check_against_restatement("gain + composite", got, mref.masked_loss(render, gt, None, fg, bg, gain=gain),
                               mref.masked_loss(render, gt, None, fg, bg, gain=gain, dtype=torch.float32), render)


def test_two_calls_are_bit_identical():
    render, gt, g = _smooth_pair(2, 75, 131, 13)
    m, f = torch.rand(2, 75, 131, device=DEV, generator=g), (torch.rand(2, 75, 131, device=DEV, generator=g) > 0.4).float()
    bg = torch.tensor([0.1, 0.6, 0.3], device=DEV)
    a, b = _masked(render, gt, m, None, f, bg), _masked(render, gt, m, None, f, bg)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[4], b[4])


def test_full_size_crop_against_the_restatement():
    """A 700 x 1100 crop at (123, 457) of 1080 x 1920 tensors: offsets and strides at full size."""
    render, gt, g = _smooth_pair(1, 1080, 1920, 17)
    image = gt.permute(0, 2, 3, 1).contiguous()                                  # [1, H, W, 3], as batch['image']
    fg_full = torch.zeros(1, 1080, 1920, device=DEV)
    fg_full[:, 140:800, 480:1530] = 1.0
    ignore_full = (torch.rand(1, 1080, 1920, device=DEV, generator=g) > 0.8).float()
    sl = (slice(123, 123 + 700), slice(457, 457 + 1100))
    r, gt_v = render[:, :, sl[0], sl[1]], image.permute(0, 3, 1, 2)[:, :, sl[0], sl[1]]
    f, m = fg_full[:, sl[0], sl[1]], ignore_full[:, sl[0], sl[1]]
    bg = torch.tensor([0.2, 0.5, 0.8], device=DEV)
    assert r.storage_offset() == 123 * 1920 + 457 and gt_v.stride() == (1080 * 1920 * 3, 1, 1920 * 3, 3)
    leaf = render.detach().requires_grad_(True)
    from log_amd.masked_loss import masked_l1_ssim_loss
    loss, l1, ssim, gt_used = masked_l1_ssim_loss(leaf[:, :, sl[0], sl[1]], gt_v, m, f, bg)
    loss.backward()
    ref = mref.masked_loss(r, gt_v, m, f, bg)
    ref32 = mref.masked_loss(r, gt_v, m, f, bg, dtype=torch.float32)
    assert torch.equal(gt_used, ref32["gt"])
    inside = leaf.grad[:, :, sl[0], sl[1]]
    _check_against_restatement("1080p crop", ((loss.detach(), l1, ssim), inside, None, None, gt_used), ref, ref32)
    outside = leaf.grad.clone()
    outside[:, :, sl[0], sl[1]] = 0
    assert float(outside.abs().max()) == 0.0


# ---- the bounds ------------------------------------------------------------------------------------------------------

def _bounds_match(mask_np, mask_dev=None):
    from log_amd.masked_loss import mask_bounds
    dev = torch.from_numpy(mask_np).to(DEV) if mask_dev is None else mask_dev
    got = mask_bounds(dev)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (mask_np.shape[0], 8)
    assert got.cpu().numpy().tolist() == mref.bounds_record(mask_np).tolist(), (mask_np.shape, got.cpu().tolist())
    return got


@pytest.mark.parametrize("H", [1, 5, 70])
@pytest.mark.parametrize("W", [1, 63, 64, 65, 300])
def test_bounds_are_exact(H, W):
    from log_amd.masked_loss import mask_bounds_host
    rng = np.random.default_rng(100 * H + W)
    blobs = (rng.random((2, H, W)) > 0.9).astype(np.float32) * rng.random((2, H, W)).astype(np.float32)
    _bounds_match(blobs)                                                          # B = 2, random foreground, values in (0, 1)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):                 # a single pixel at each corner
        one = np.zeros((2, H, W), np.float32)
        one[1, y, x] = 1.0
        rec = _bounds_match(one)
        assert rec[1, :5].tolist() == [x, y, x, y, 1] and rec[0, :5].tolist() == [W, H, -1, -1, 0]
    assert _bounds_match(np.ones((2, H, W), np.float32))[0, :5].tolist() == [0, 0, W - 1, H - 1, H * W]
    empty = np.zeros((1, H, W), np.float32)
    assert _bounds_match(empty)[0, 4].item() == 0
    with pytest.raises(IndexError):
        mask_bounds_host(torch.from_numpy(empty).to(DEV), 2)
    half = np.full((1, H, W), 0.5, np.float32)                                    # exactly the threshold, and NaN: not foreground
    half[0, H // 2, W // 2] = np.nan
    assert _bounds_match(half)[0, :5].tolist() == [W, H, -1, -1, 0]
    big = rng.random((2, 2 * H + 1, 3 * W + 2)).astype(np.float32)                # a strided view
    dev = torch.from_numpy(big).to(DEV)[:, 1::2, 2::3]
    assert dev.stride() == ((2 * H + 1) * (3 * W + 2), 2 * (3 * W + 2), 3) and tuple(dev.shape) == (2, H, W)
    _bounds_match(np.ascontiguousarray(big[:, 1::2, 2::3]), dev)
    box = np.zeros((1, H, W), np.float32)
    box[0, H // 3:H // 2 + 1, W // 4:W // 2 + 1] = 0.75
    assert mask_bounds_host(torch.from_numpy(box).to(DEV), 3) == mref.bounds(box, 3)
    a, b = _bounds_match(blobs), _bounds_match(blobs)
    assert torch.equal(a, b)


# ---- the drop-in forward on stand-ins --------------------------------------------------------------------------------

class _Renderer:
    """What MaskForeground.forward reads of its renderer."""

    def __init__(self, background, use_randback=False, split="train"):
        self.split, self.use_randback = split, use_randback
        self.background = background
        self.ssim_loss = types.SimpleNamespace(window_size=11, padding=0)
        self.l1_loss = torch.nn.L1Loss()
        self.seen = []

    def vis(self, batch, model, background=None):
        self.seen.append(background)
        return {"render": self.leaf}


def _reference_forward(self, batch, model):
    raise AssertionError("the stand-in reference's forward was called")


@pytest.fixture()
def standin():
    from log_amd import masked_loss as ml
    ml.reset_stats()
    with ml.dropins.substituted(forward=_reference_forward, bound_from_mask=_reference_forward):
        yield ml
    ml.reset_stats()


def _batch(c):
    batch = {"image": c["image"].to(DEV), "mask": c["mask"].to(DEV)}
    if c["mask_ignore"] is not None:
        batch["mask_ignore"] = c["mask_ignore"].to(DEV)
    return batch


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_dropin_forward(standin, path):
    ml = standin
    c = mref.load_case(path)
    renderer = _Renderer(c["background"].to(DEV))
    renderer.leaf = c["render"].to(DEV).requires_grad_(True)
    batch = _batch(c)
    output = ml.forward(renderer, batch, types.SimpleNamespace(training=True))
    output["loss"].backward()
    assert len(renderer.seen) == 1 and renderer.seen[0] is renderer.background
    crop = output["render"]
    assert list(crop.shape) == c["crop_shape"].tolist() and crop.storage_offset() == int(c["crop_offset"])
    assert torch.equal(output["gt"].cpu(), torch.from_numpy(c["gt32"])) and not output["gt"].requires_grad
    h, w = crop.shape[2:]
    t, l = int(c["ltrb"][1]), int(c["ltrb"][0])
    if c["mask_ignore"] is not None:
        assert torch.equal(output["mask_ignore"], batch["mask_ignore"][:, t:t + h, l:l + w])
    else:
        assert "mask_ignore" not in output
    assert set(output["loss_dict"]) == {"l1", "ssim"} and all(isinstance(v, float) for v in output["loss_dict"].values())
    scalars = (output["loss"].detach(), output["loss_dict"]["l1"], output["loss_dict"]["ssim"])
    grad = renderer.leaf.grad
    _check_fixture(c, scalars, grad[:, :, t:t + h, l:l + w], "forward " + IDS[GOLDEN.index(path)])
    outside = grad.clone()
    outside[:, :, t:t + h, l:l + w] = 0
    assert float(outside.abs().max()) == 0.0
    s = ml.stats()
    assert s["readbacks"] == {"forward": 2} and s["fallbacks"] == {} and s["calls"] == {"forward": 1}
    # bound_from_mask, as process_gt / process_pred call it
    assert ml.bound_from_mask(renderer, batch["mask"][..., None], 0) == mref.bounds(c["mask"].numpy(), 0)
    assert ml.stats()["readbacks"] == {"forward": 2, "bound_from_mask": 1}


def test_dropin_forward_random_background_and_other_splits(standin):
    ml = standin
    c = mref.load_case(GOLDEN[0])
    renderer = _Renderer(c["background"].to(DEV), use_randback=True)
    renderer.leaf = c["render"].to(DEV).requires_grad_(True)
    torch.manual_seed(123)
    output = ml.forward(renderer, _batch(c), types.SimpleNamespace(training=True))
    torch.manual_seed(123)
    want = torch.rand(3, device=torch.device(DEV))
    assert len(renderer.seen) == 1 and torch.equal(renderer.seen[0], want)
    render, gt, fg, _ = mref.cropped_inputs({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()})
    assert torch.equal(output["gt"], gt * fg[:, None] + (1 - fg[:, None]) * want[None, :, None, None])
    renderer.split = "val"
    assert ml.forward(renderer, _batch(c), types.SimpleNamespace(training=False)) == {"render": renderer.leaf}
    assert renderer.seen[1] is None and ml.stats()["readbacks"] == {"forward": 2}


def test_dropin_forward_falls_back_by_reason(standin):
    ml = standin
    c = mref.load_case(GOLDEN[0])
    calls = []

    def reference(self, batch, model):
        calls.append(batch)
        return "reference"

    def case(reason, batch=None, renderer=None, model=None):
        renderer = renderer or _Renderer(c["background"].to(DEV))
        renderer.leaf = c["render"].to(DEV).requires_grad_(True)
        before = len(calls)
        assert ml.forward(renderer, batch or _batch(c), model or types.SimpleNamespace(training=True)) == "reference"
        assert len(calls) == before + 1 and ml.stats()["fallbacks"].get(("forward", reason)) == 1, (reason, ml.stats())

    with ml.dropins.substituted(forward=reference):
        two = {k: torch.cat([v, v]) for k, v in _batch(c).items()}
        case("a batch of more than one image", batch=two)
        case(ml.OFF_GPU, batch={k: v.cpu() for k, v in _batch(c).items()})
        tiny = _batch(c)
        tiny["mask"] = torch.zeros_like(tiny["mask"])
        tiny["mask"][0, 30, 40:45] = 1.0                                # padding 1: a crop of 3 x 7
        case("a crop under 11 pixels", batch=tiny)
        case("render_correct in output", model=types.SimpleNamespace(training=True, view_correction=object()))
        other = _Renderer(c["background"].to(DEV))
        other.ssim_loss.window_size = 7
        case("loss modules the kernels do not cover", renderer=other)
        grad = _batch(c)
        grad["mask"] = grad["mask"].clone().requires_grad_(True)
        case(ml.NEEDS_GRAD, batch=grad)
        short = _batch(c)
        short["mask_ignore"] = torch.zeros_like(short["mask"])[:, :-1]
        case(ml.SHAPES, batch=short)
    assert len(ml.stats()["fallbacks"]) == 7 and ml.stats()["calls"]["forward"] == 7
    assert ml.stats()["readbacks"] == {"forward": 1}                 # the crop's bounds: every other reason needs no device work


def test_dropin_forward_raises_when_vis_contradicts_the_checks(standin):
    """A vis that returns render_correct, or a render of another shape, after every check has passed: the background is drawn
    and the view rendered, so the reference's method is NOT called (it would draw and render again)."""
    from log_amd import _lib
    ml = standin
    c = mref.load_case(GOLDEN[0])
    for extra, leaf, words in (({"render_correct": None}, c["render"], "render_correct"),
                               ({}, c["render"][:, :, :-1], "a render torch.float32"),
                               ({}, c["render"].double(), "a render torch.float64")):
        renderer = _Renderer(c["background"].to(DEV), use_randback=True)
        renderer.leaf = leaf.to(DEV).requires_grad_(True)
        vis = renderer.vis
        renderer.vis = lambda batch, model, background=None: dict(vis(batch, model, background), **extra)
        with pytest.raises(_lib.LograstError, match=words):
            ml.forward(renderer, _batch(c), types.SimpleNamespace(training=True))
        assert len(renderer.seen) == 1                               # one render, one draw
    assert ml.stats()["fallbacks"] == {} and ml.stats()["calls"] == {"forward": 3}


# ---- the switch: both calculate_loss through the masked kernels ------------------------------------------------------

@pytest.fixture()
def switch_on():
    from log_amd import masked_loss as ml, view_correction as vc
    was = ml.enabled()
    vc.reset_stats()
    vc.handed_out.take()
    ml.set_enabled(True)
    yield ml
    ml.set_enabled(was)
    vc.handed_out.take()
    vc.reset_stats()


def _no_original(*args):
    raise AssertionError("the wrapped calculate_loss was called")


@pytest.mark.parametrize("with_correct", [False, True])
def test_loss_calculate_loss_with_the_switch_on_is_the_torch_blend_bit_for_bit(switch_on, with_correct):
    """log_amd.loss's calculate_loss with a mask_ignore: switch on (one masked call) against switch off (the torch blend in
    front of the unmasked kernels) -- loss, loss_dict and both gradients with the same bits."""
    from log_amd import loss
    ml = switch_on
    render0, gt, g = _smooth_pair(2, 37, 53, 23)
    gt = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    mask = (torch.rand(2, 37, 53, device=DEV, generator=g) < 0.3).float()
    four0 = torch.rand(2, 4, 37, 53, device=DEV, generator=g)
    me = types.SimpleNamespace(ssim_loss=types.SimpleNamespace(window_size=11, padding=0), l1_loss=torch.nn.L1Loss())
    calculate_loss = loss._make_calculate_loss(_no_original)
    results = {}
    for on in (True, False):
        ml.set_enabled(on)
        render, four = render0.clone().requires_grad_(True), four0.clone().requires_grad_(True)
        output = {"render_correct": four} if with_correct else {}
        assert calculate_loss(me, gt, render, output, mask) is None
        output["loss"].backward()
        results[on] = (output["loss"].detach(), output["loss_dict"], render.grad, four.grad)
    on, off = results[True], results[False]
    assert torch.equal(on[0], off[0]) and on[1] == off[1] and torch.equal(on[2], off[2])
    assert set(on[1]) == {"l1", "ssim"} and all(isinstance(v, float) for v in on[1].values())
    if with_correct:
        assert torch.equal(on[3], off[3]) and float(on[3][:, :3].abs().min()) > 0 and not on[3][:, 3].any()
    else:
        assert on[3] is None and off[3] is None
    # ... and it is the masked kernels that ran: the same bits as the direct call
    direct = _masked(render0, gt, mask, four0[:, :3] if with_correct else None)
    assert torch.equal(direct[0][0], on[0]) and torch.equal(direct[1], on[2])


def test_view_correction_calculate_loss_with_the_switch_on_takes_gain_and_mask_in_one_call(switch_on):
    """log_amd.view_correction's calculate_loss with rows handed out and a mask_ignore: the bits of the direct call with gain
    and mask, the gain's gradient in the handed-out rows of the dense view_correction.grad, one read-back; against the
    float64 restatement by the file's rule (the two-call path of the switch-off branch rounds differently)."""
    from log_amd import view_correction as vc
    B, V, H, W = 2, 4, 37, 53
    render0, gt, g = _smooth_pair(B, H, W, 29)
    gt = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    mask = (torch.rand(B, H, W, device=DEV, generator=g) < 0.3).float()
    param = torch.nn.Parameter(torch.tensor([[1.1, 0.93, 1.04], [1.0, 1.0, 1.0], [0.88, 1.02, 1.21], [1.0, 1.0, 1.0]], device=DEV))
    indices = [2, 0]
    me = types.SimpleNamespace(ssim_loss=types.SimpleNamespace(window_size=11, padding=0), l1_loss=torch.nn.L1Loss())
    render = render0.clone().requires_grad_(True)
    rows = [param[i] for i in indices]
    for row in rows:
        vc.handed_out.note(row)
    output = {"render_correct": torch.stack([render[b] * row[:, None, None] for b, row in enumerate(rows)])}
    with vc.dropins.substituted(calculate_loss=_no_original):
        vc.calculate_loss(me, gt, render, output, mask)
    assert vc.stats()["fallbacks"] == {} and vc.stats()["readbacks"] == {"calculate_loss": 1} and vc.handed_out.count == 0
    output["loss"].backward()
    gain = param.detach()[indices]
    direct = _masked(render0, gt, mask, gain=gain)
    assert torch.equal(output["loss"].detach(), direct[0][0]) and torch.equal(render.grad, direct[1])
    assert output["loss_dict"] == {"l1": float(direct[0][1]), "ssim": float(direct[0][2])}
    assert tuple(param.grad.shape) == (V, 3) and torch.equal(param.grad[indices], direct[3]) and not param.grad[[1, 3]].any()
    got = ((output["loss"].detach(), output["loss_dict"]["l1"], output["loss_dict"]["ssim"]), render.grad, None,
           param.grad[indices], None)
    _check_against_restatement("view_correction switch on", got, mref.masked_loss(render0, gt, mask, gain=gain),
                               mref.masked_loss(render0, gt, mask, gain=gain, dtype=torch.float32), render0)


# ---- which entry point runs ------------------------------------------------------------------------------------------

LOSS_ENTRY_POINTS = ("forward", "backward", "forward_gain", "backward_gain", "forward_masked", "backward_masked")
# input kind -> (what it adds to (render, gt), the entry point of the forward, the entry point of the backward)
DISPATCH = {
    "plain": ((), "forward", "backward"),
    "render_l1 of its own": (("render_l1",), "forward", "backward"),
    "render_l1 is render": (("render_l1 is render",), "forward", "backward"),
    "gain": (("gain",), "forward_gain", "backward_gain"),
    "mask": (("mask",), "forward_masked", "backward_masked"),
    "mask + gain": (("mask", "gain"), "forward_masked", "backward_masked"),
    "mask + render_l1": (("mask", "render_l1"), "forward_masked", "backward_masked"),
    "foreground": (("foreground",), "forward_masked", "backward"),
    "foreground + gain": (("foreground", "gain"), "forward_masked", "backward_gain"),
    "foreground + mask": (("foreground", "mask"), "forward_masked", "backward_masked"),
}


@pytest.mark.parametrize("H,W", [(11, 11), (43, 42)])
def test_each_input_kind_calls_its_entry_points(monkeypatch, H, W):
    """The six C functions behind counters: a mask or a foreground takes the masked forward, else a gain the gain forward, else
    the plain one; an ignore mask takes the masked backward, else a gain the gain backward, else the plain backward (after a
    foreground alone: on the composited ground truth).  One call each, no other."""
    from log_amd import _lib
    from log_amd.loss import l1_ssim_loss
    from log_amd.masked_loss import masked_l1_ssim_loss
    L = _lib.lib()
    calls = []

    def counted(name, fn):
        def call(*args):
            calls.append(name)
            return fn(*args)
        return call
    for name in LOSS_ENTRY_POINTS:
        monkeypatch.setattr(L, "lograst_loss_" + name, counted(name, getattr(L, "lograst_loss_" + name)))
    render0, gt, render_l1, masks = _inputs(1, 3, H, W, 31 * H + W)
    bg = torch.tensor([0.2, 0.5, 0.8], device=DEV)
    gain = torch.tensor([[1.1, 0.93, 1.04]], device=DEV)
    for kind, (adds, forward, backward) in DISPATCH.items():
        r = _leaf(render0)
        rl = r if "render_l1 is render" in adds else _leaf(render_l1) if "render_l1" in adds else None
        k = _leaf(gain) if "gain" in adds else None
        m = masks["random"] if "mask" in adds else None
        f = masks["binary"] if "foreground" in adds else None
        del calls[:]
        if m is None and f is None:
            loss = l1_ssim_loss(r, gt, rl, l1_gain=k)[0]
        else:
            loss = masked_l1_ssim_loss(r, gt, m, f, bg if f is not None else None, rl, k)[0]
        assert calls == [forward], (kind, calls)
        loss.backward()
        assert calls == [forward, backward], (kind, calls)
        assert r.grad is not None and (k is None or k.grad is not None) and (rl is None or rl.grad is not None), kind
