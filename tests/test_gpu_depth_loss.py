"""The fused depth patch loss on the device (log_amd.depth_loss.depth_patch_loss -> lograst_depth_loss_forward /
_backward) against

* the reference's own float64 results (tests/golden/depth_loss_*.npz, written by tests/golden/make_golden_depth_loss.py)
* the float64 restatement tests/depth_loss_ref.py (held to those results by tests/test_depth_loss_cpu.py) at shapes no
  fixture has.

Tolerances (one rule for every comparison in this file):
    gradient  rel-L2 <= min(1e-4, 8 * gap32_grad)
    loss      |loss - loss64| <= min(1e-4 * |loss64|, 8 * (gap32_loss + 2^-24 * |loss64|))
1e-4 is the project's standing bar; gap32 is the distance between the reference's own fp32 and float64 runs (stored in
the fixtures; for other inputs depth_loss_ref(float32) against depth_loss_ref(float64) on the same inputs), the factor 8
and the 2^-24 term (the loss leaves the kernel as one fp32 number) are those of tests/test_gpu_loss.py and
tools/fuzz_step_ops.py.  On the nearly constant fixture the reference's fp32 run is lost (gap32_grad about 1), the bound
is the 1e-4 cap, and only double arithmetic inside the kernels meets it.

No test here reads the reference tree."""
import glob
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from depth_loss_ref import depth_loss_ref, load_case, rel_l2  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "depth_loss_*.npz")))
IDS = [os.path.basename(p)[11:-4] for p in GOLDEN]
DEV = "cuda:0"
CAP = 1e-4
FACTOR = 8.0
ULP = 2.0 ** -24


def _run(pred, gt, acc, rows, cols, upstream=None):
    """-> (loss as a python float, grad_pred, the 0-dim loss tensor detached)"""
    from log_amd.depth_loss import depth_patch_loss
    p = pred.detach().requires_grad_(True)
    loss = depth_patch_loss(p, gt, acc, rows, cols)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    (loss if upstream is None else upstream * loss).backward()
    assert p.grad.shape == pred.shape and p.grad.dtype == torch.float32
    return float(loss.detach()), p.grad, loss.detach().clone()


def _check(tag, loss, grad, loss64, grad64, gap_loss, gap_grad):
    """Prints every measured figure next to its bound, then asserts both."""
    e_loss, b_loss = abs(loss - loss64), min(CAP * abs(loss64), FACTOR * (gap_loss + ULP * abs(loss64)))
    e_grad, b_grad = rel_l2(grad.cpu(), grad64.cpu()), min(CAP, FACTOR * gap_grad)
    print(f"[depth loss] {tag}: loss |{loss:.9g} - {loss64:.9g}| = {e_loss:.3e} <= {b_loss:.3e} (ratio {e_loss / b_loss:.3f}); "
          f"grad rel-L2 {e_grad:.3e} <= {b_grad:.3e} (ratio {e_grad / b_grad:.3f}; gap32 loss {gap_loss:.3e} grad {gap_grad:.3e})")
    assert torch.isfinite(grad).all()
    assert e_loss <= b_loss, (tag, "loss", e_loss, b_loss)
    assert e_grad <= b_grad, (tag, "grad", e_grad, b_grad)


def _check_against_restatement(tag, pred, gt, acc, rows, cols):
    r64 = depth_loss_ref(pred, gt, acc, rows, cols)
    r32 = depth_loss_ref(pred, gt, acc, rows, cols, dtype=torch.float32)
    loss, grad, _ = _run(pred, gt, acc, rows, cols)
    _check(tag, loss, grad, r64["loss"], r64["grad"], abs(r32["loss"] - r64["loss"]), rel_l2(r32["grad"], r64["grad"]))
    return loss, grad


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_golden_cases(path):
    c = load_case(path)
    pred, gt, acc, rows, cols = (c[k].to(DEV) for k in ("pred", "gt", "acc", "rows", "cols"))
    if "grad64" not in c:                                       # empty: no valid pixel anywhere
        from log_amd.depth_loss import depth_patch_loss
        assert math.isnan(float(depth_patch_loss(pred, gt, acc, rows, cols))) and math.isnan(float(c["loss64"]))
        return
    loss, grad, _ = _run(pred, gt, acc, rows, cols)
    _check(IDS[GOLDEN.index(path)], loss, grad, float(c["loss64"]), torch.from_numpy(c["grad64"]), float(c["gap32_loss"]),
           float(c["gap32_grad"]))


def _maps(H, W, seed, margin=0):
    """The recipe of fixture `smooth` at any size, on the device: depth in [2, 4] with 0.05 noise, a smooth target, an
    accumulation map that crosses 0.5.  margin > 0: each image is the middle of a larger allocation (margin pixels on
    every side, filled the same way), so that a read beyond the image would still land in memory of this test."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    Hb, Wb = H + 2 * margin, W + 2 * margin

    def field(cells):
        coarse = torch.rand(1, 1, cells, cells, device=DEV, generator=g, dtype=torch.float64)
        return torch.nn.functional.interpolate(coarse, size=(Hb, Wb), mode="bilinear", align_corners=True)[0, 0]
    pred = (2.1 + 1.8 * field(6) + 0.05 * torch.randn(Hb, Wb, device=DEV, generator=g, dtype=torch.float64)).float()
    gt = (0.1 + 0.5 * field(5)).float()
    acc = (0.15 + 0.8 * field(4)).float()
    crop = (slice(margin, margin + H), slice(margin, margin + W))
    return pred[crop], gt[crop], acc[crop]


def _starts(H, W, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randint(0, H - 64 + 1, (n,), device=DEV, generator=g), torch.randint(0, W - 64 + 1, (n,), device=DEV, generator=g))


def _t(v):
    return torch.tensor(v, dtype=torch.int64, device=DEV)


def test_65x65_and_64x64():
    pred, gt, acc = _maps(65, 65, 1)
    _check_against_restatement("65x65 starts (0,0) (1,1) (0,1)", pred, gt, acc, _t([0, 1, 0]), _t([0, 1, 1]))
    pred, gt, acc = _maps(64, 64, 2)
    _check_against_restatement("64x64 n=1", pred, gt, acc, _t([0]), _t([0]))


@pytest.mark.parametrize("n", [1, 3, 64, 256])
def test_patch_counts(n):
    pred, gt, acc = _maps(150, 203, 10 + n)
    rows, cols = _starts(150, 203, n, 20 + n)
    _check_against_restatement(f"150x203 n={n}", pred, gt, acc, rows, cols)


def test_64_identical_patches():
    pred, gt, acc = _maps(97, 131, 3)
    _check_against_restatement("64 identical patches", pred, gt, acc, _t([17] * 64), _t([40] * 64))


def test_last_valid_start():
    pred, gt, acc = _maps(97, 131, 4)
    _check_against_restatement("start (H-64, W-64)", pred, gt, acc, _t([97 - 64, 0, 97 - 64]), _t([131 - 64, 131 - 64, 0]))


@pytest.fixture(scope="module")
def full_hd():
    pred, gt, acc = _maps(1080, 1920, 5)
    rows, cols = _starts(1080, 1920, 64, 6)
    return pred, gt, acc, rows, cols


def test_full_hd_and_exact_zeros_outside_the_patches(full_hd):
    pred, gt, acc, rows, cols = full_hd
    _, grad = _check_against_restatement("1080x1920 n=64", pred, gt, acc, rows, cols)
    covered = torch.zeros(1080, 1920, dtype=torch.bool, device=DEV)
    for r, c in zip(rows.tolist(), cols.tolist()):
        covered[r:r + 64, c:c + 64] = True
    outside = grad[~covered]
    assert outside.numel() > 1080 * 1920 // 2
    assert torch.equal(outside.view(torch.int32), torch.zeros_like(outside, dtype=torch.int32))      # +0.0, bit for bit
    assert float(grad[covered].abs().max()) > 0.0


def test_strides_change_nothing():
    H, W = 97, 131
    pred, gt, acc = _maps(H, W, 7)
    rows, cols = _starts(H, W, 64, 8)
    base = _run(pred, gt, acc, rows, cols)
    # pred is channel 0 and acc channel 2 of one [3, H, W] tensor (LoG's depth render); gt a crop out of a larger tensor
    three = torch.stack([pred, torch.rand_like(pred), acc])
    big = torch.rand(H + 40, W + 50, device=DEV)
    big[11:11 + H, 23:23 + W] = gt
    gt_v = big[11:11 + H, 23:23 + W]
    assert not gt_v.is_contiguous() and gt_v.stride() == (W + 50, 1) and three[2].storage_offset() == 2 * H * W
    a = _run(three[0], gt_v, three[2], rows, cols)
    # the same render stored pixel-major [H, W, 3]: element stride 3 along x
    hw3 = three.permute(1, 2, 0).contiguous()
    assert hw3[..., 0].stride() == (3 * W, 3)
    b = _run(hw3[..., 0], gt_v.t().contiguous().t(), hw3[..., 2], rows, cols)
    for other in (a, b):
        assert torch.equal(other[2], base[2]) and torch.equal(other[1], base[1])


@pytest.mark.parametrize("bad", [("row", 1), ("row", -1), ("col", 1), ("col", -1), ("row", 1 << 40), ("col", -(1 << 40))],
                         ids=["r=H-63", "r=-1", "c=W-63", "c=-1", "r=2^40", "c=-2^40"])
def test_out_of_range_patch(bad):
    """A patch that does not lie inside the image is not read: the loss is nan, the patch adds nothing to the gradient,
    and the next call is unaffected.  Every image is a crop with 64 pixels of margin inside its allocation."""
    from log_amd.depth_loss import depth_patch_loss
    H, W = 97, 131
    pred, gt, acc = _maps(H, W, 9, margin=64)
    assert pred.storage_offset() == 64 * (W + 128) + 64
    good_r, good_c = [0, 20, H - 64], [5, W - 64, 30]
    before = _run(pred, gt, acc, _t(good_r), _t(good_c))
    which, v = bad
    r = {1: H - 63, -1: -1}.get(v, v) if which == "row" else 10
    c = {1: W - 63, -1: -1}.get(v, v) if which == "col" else 10
    rows, cols = _t(good_r[:2] + [r] + good_r[2:]), _t(good_c[:2] + [c] + good_c[2:])
    loss, grad, _ = _run(pred, gt, acc, rows, cols)
    assert math.isnan(loss)
    assert torch.equal(grad, before[1])                 # M and every sum come from the valid patches, in the same order
    after = _run(pred, gt, acc, _t(good_r), _t(good_c))
    assert torch.equal(after[2], before[2]) and torch.equal(after[1], before[1])
    assert math.isnan(float(depth_patch_loss(pred, gt, acc, _t([r]), _t([c]))))


def test_reproducible_half_upstream_and_no_grad(full_hd):
    from log_amd.depth_loss import depth_patch_loss
    pred, gt, acc, rows, cols = full_hd
    a, b = _run(pred, gt, acc, rows, cols), _run(pred, gt, acc, rows, cols)
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1])
    h = _run(pred, gt, acc, rows, cols, upstream=0.5)
    assert torch.equal(h[1], 0.5 * a[1]) and float(a[1].abs().max()) > 0
    with torch.no_grad():
        l0 = depth_patch_loss(pred, gt, acc, rows, cols)
    l1 = depth_patch_loss(pred, gt, acc, rows, cols)        # nothing requires grad
    assert not l0.requires_grad and not l1.requires_grad and torch.equal(l0, a[2]) and torch.equal(l1, a[2])


def test_graph_capture_replays_the_eager_result_at_new_positions():
    from log_amd.depth_loss import depth_patch_loss
    H, W = 270, 480
    pred, gt, acc = _maps(H, W, 11)
    rows, cols = _starts(H, W, 64, 12)
    rows2, cols2 = _starts(H, W, 64, 13)
    eager1, eager2 = _run(pred, gt, acc, rows, cols), _run(pred, gt, acc, rows2, cols2)
    assert not torch.equal(eager1[1], eager2[1])
    p = pred.clone().requires_grad_(True)
    r, c = rows.clone(), cols.clone()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):                       # warm-up on the capture stream
        depth_patch_loss(p, gt, acc, r, c).backward()
    torch.cuda.synchronize()
    p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        loss = depth_patch_loss(p, gt, acc, r, c)
        loss.backward()
    torch.cuda.synchronize()
    for want, (rr, cc) in ((eager1, (rows, cols)), (eager2, (rows2, cols2)), (eager1, (rows, cols))):
        r.copy_(rr)
        c.copy_(cc)
        p.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), want[2]) and torch.equal(p.grad, want[1])


def test_append_depth_loss_without_the_reference():
    from log_amd.depth_loss import append_depth_loss, depth_patch_loss
    H, W = 150, 203
    pred, gt, acc = _maps(H, W, 14)
    seed = 1234
    torch.manual_seed(seed)
    rows = torch.randint(0, H - 64, (64,), device=DEV)
    cols = torch.randint(0, W - 64, (64,), device=DEV)
    third = torch.randint(0, 1000, (8,), device=DEV)
    want = _run(pred, gt, acc, rows, cols)
    p = pred.clone().requires_grad_(True)
    render_loss = (p * 0.0).sum() + 0.25
    output = {"accmap": acc[None], "loss": render_loss, "loss_dict": {"l1": 0.1}}
    torch.manual_seed(seed)
    assert append_depth_loss(gt[None], p[None], output) is output
    assert torch.equal(torch.randint(0, 1000, (8,), device=DEV), third)       # the generator advanced as under two randint calls
    assert set(output) == {"accmap", "loss", "loss_dict", "gt_depth", "pred_depth"} and set(output["loss_dict"]) == {"l1", "depth"}
    depth = output["loss_dict"]["depth"]
    assert torch.is_tensor(depth) and torch.equal(depth.detach(), want[2])    # the same positions: the same bits
    assert torch.equal(output["loss"].detach(), (render_loss + want[2]).detach())
    assert torch.equal(output["gt_depth"], gt[None])
    mask = acc > 0.5
    vis = 1. / (pred + 1e-5)
    vis = (vis - vis[mask].min()) / (vis[mask].max() - vis[mask].min())      # renderer.py:287-288
    assert not output["pred_depth"].requires_grad and torch.equal(output["pred_depth"], vis[None])
    output["loss"].backward()
    assert torch.equal(p.grad, want[1])
    # a generator of its own
    g = torch.Generator(device=DEV).manual_seed(5)
    out2 = {"accmap": acc[None], "loss": 0, "loss_dict": {}}
    append_depth_loss(gt[None], pred[None], out2, generator=g)
    g.manual_seed(5)
    rows = torch.randint(0, H - 64, (64,), device=DEV, generator=g)
    cols = torch.randint(0, W - 64, (64,), device=DEV, generator=g)
    assert torch.equal(out2["loss"], depth_patch_loss(pred, gt, acc, rows, cols))


@pytest.mark.parametrize("reuse", [False, True], ids=["rebin", "reuse_geometry"])
def test_into_the_rasterizer(reuse):
    """A trained-like scene of 50 000 Gaussians at 400 x 400 (the framing of the C1 plumbing test, so the patches hold
    geometry), an RGB call and a depth-colour call through one rasterizer object as LoG makes them.  Run A:
    l1_ssim_loss + depth_patch_loss, backward.  Run B: the depth term replaced by (depth image * G).sum(), G =
    depth_loss_ref(float64)'s gradient on A's depth image, rounded to fp32.  Every Gaussian gradient agrees within 1e-4
    rel-L2 (the bar of tests/test_gpu_loss.py::test_into_the_rasterizer)."""
    import gpu_util as G
    from log_amd import rasterizer as R, scenes
    from log_amd.depth_loss import depth_patch_loss
    from log_amd.loss import l1_ssim_loss
    import diff_gaussian_rasterization_wodilate as wo
    dev = torch.device(DEV)
    N, S = 50000, 400
    cam = scenes.orbit_cameras(2, W=S, H=S, focal=1200.0)[0]
    sc = scenes.trained_like_scene(N, seed=0)
    sc["opacity"] = np.clip(sc["opacity"], 0.05, 0.95)
    gen = torch.Generator(device=DEV).manual_seed(5)
    gt_image = torch.rand(1, S, S, 3, device=dev, generator=gen).permute(0, 3, 1, 2)
    gt_depth = 2.0 + 2.0 * torch.rand(S, S, device=dev, generator=gen)
    rows, cols = _starts(S, S, 64, 15)
    xyz1 = np.concatenate([sc["xyz"], np.ones((N, 1), np.float32)], axis=1).astype(np.float32)
    point_depth = torch.tensor(np.ascontiguousarray((xyz1 @ np.asarray(cam["world_view_transform"], np.float32))[:, 2]), device=dev)
    names = ("xyz", "scaling", "rotation", "opacity", "colors")
    prev = R.set_geometry_reuse(reuse)
    try:
        grads, weight = [], None
        for fused in (True, False):
            L = {k: torch.tensor(np.ascontiguousarray(sc[k], np.float32), device=dev, requires_grad=True) for k in names}
            m2 = torch.zeros(N, 3, device=dev, requires_grad=True)
            rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, (1.0, 1.0, 1.0), dev))
            kw = dict(means3D=L["xyz"], means2D=m2, shs=None, colors_precomp=L["colors"], opacities=L["opacity"],
                      scales=L["scaling"], rotations=L["rotation"], cov3D_precomp=None)
            image = rast(**kw)[0]
            colours = torch.stack([point_depth, L["xyz"][:, 2], torch.ones_like(point_depth)], dim=-1)     # renderer.py:187-189
            depth3 = rast(**dict(kw, colors_precomp=colours))[0]
            loss = l1_ssim_loss(image[None], gt_image)[0]
            if fused:
                assert float((depth3[2] > 0.5).float().mean()) > 0.25          # the patches hold geometry
                weight = depth_loss_ref(depth3[0], gt_depth, depth3[2], rows, cols)["grad"].float()
                loss = loss + depth_patch_loss(depth3[0], gt_depth, depth3[2], rows, cols)
            else:
                loss = loss + (depth3[0] * weight).sum()
            loss.backward()
            grads.append([t.grad.clone() for t in list(L.values()) + [m2]])
    finally:
        R.set_geometry_reuse(prev)
    for name, a, b in zip(names + ("means2D",), *grads):
        err = rel_l2(a.cpu(), b.cpu())
        print(f"[depth loss] into the rasterizer ({'reuse' if reuse else 'rebin'}) {name}: rel-L2 {err:.3e}")
        assert float(a.abs().sum()) > 0 and float(b.abs().sum()) > 0 and err <= CAP, (name, err)
