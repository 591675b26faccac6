"""CPU checks of the masked training loss (log_amd.masked_loss, lograst_loss_*_masked, lograst_mask_bounds*):

* tests/masked_loss_ref.py, the restatement the GPU tests lean on, against the reference's own recorded results
  (tests/golden/fgmask_*.npz, written by tests/golden/make_golden_fgmask.py from MaskForeground.forward): float64 scalars to
  1e-12 relative, float64 gradients to 1e-10 rel-L2, the composited ground truth and the bounds exactly; its float32
  evaluation by the rules the GPU tests apply to the kernels (scalars within 8 * the largest gap32 over the fixtures,
  gradients within min(1e-4, 8 * gap32));
* the exports, the scratch sizes and the argument checks of the entry points, which happen before any device work;
* the switch inside log_amd.loss's and log_amd.view_correction's calculate_loss, with the kernels stood in for;
* the drop-ins on the reference's own classes (LOG_REFERENCE; skipped without): install / uninstall, and a CPU call, which
  falls back and returns the recorded fp32 result to the bit."""
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
from loss_ref import rel_l2  # noqa: E402

REF = os.environ.get("LOG_REFERENCE", "/root/reference")
GOLDEN = sorted(glob.glob(os.path.join(HERE, "golden", "fgmask_*.npz")))
IDS = [os.path.basename(p)[len("fgmask_"):-4] for p in GOLDEN]
FACTOR, GRAD_TOL = 8.0, 1e-4


def _window():
    """The reference's SSIM buffer (its fp32 outer product, not the library's separable taps), as the loss fixtures hold it."""
    return torch.from_numpy(np.load(os.path.join(HERE, "golden", "loss_1x11x11.npz"))["window"]).double()


def _scalar_gaps():
    zs = [np.load(p) for p in GOLDEN]
    return {k: max(float(z["gap32_" + k]) for z in zs) for k in ("l1", "ssim", "loss")}


def test_the_fixtures_cover_what_they_should():
    assert IDS == ["box_60x90", "box_ignore_60x90", "cols42_40x80", "cols43_40x80", "corner_48x64", "pixel_26x400", "soft_60x90"]
    z = {i: np.load(p) for i, p in zip(IDS, GOLDEN)}
    assert z["box_60x90"]["crop_shape"].tolist() == [1, 3, 37, 52] and int(z["box_60x90"]["crop_offset"]) == 829
    assert "mask_ignore" not in z["box_60x90"] and "mask_ignore" in z["box_ignore_60x90"]
    assert z["cols42_40x80"]["crop_shape"][3] == 42 and z["cols43_40x80"]["crop_shape"][3] == 43
    c = z["corner_48x64"]                                # the clamp to 0 at the top, the slice's clamp at the right
    assert c["ltrb"].tolist() == [39, 0, 64, 21] and int(c["mask"][0].nonzero()[0].min()) == 0
    assert c["crop_shape"].tolist() == [1, 3, 22, 25] and c["image"].shape[2] == 64
    p = z["pixel_26x400"]
    assert int((p["mask"] > 0.5).sum()) == 1 and min(p["crop_shape"][2:]) >= 11
    s = z["soft_60x90"]["mask"]
    assert 0 < s.min() and s.max() < 1 and len(np.unique(s)) > 100
    for name, f in z.items():
        assert float(f["gap32_grad_render"]) < 1.25e-5, name
        assert os.path.getsize(GOLDEN[IDS.index(name)]) < 400 * 1024


@pytest.mark.parametrize("path", GOLDEN, ids=IDS)
def test_restatement_against_the_reference(path):
    c = mref.load_case(path)
    H, W = c["mask"].shape[1:]
    ltrb = mref.bounds(c["mask"].numpy(), int(max(1, H, W) / 50))
    assert list(ltrb) == c["ltrb"].tolist()
    t, l, h, w = mref.crop_of((H, W), ltrb)
    assert [1, 3, h, w] == c["crop_shape"].tolist() and t * W + l == int(c["crop_offset"])
    render, gt, fg, mi = mref.cropped_inputs(c, ltrb)
    r64 = mref.masked_loss(render, gt, mi, fg, c["background"], window=_window())
    for k in ("loss", "l1", "ssim"):
        assert abs(r64[k] - float(c[k + "64"])) <= 1e-12 * abs(float(c[k + "64"])), k
    assert rel_l2(r64["grad_render"], torch.from_numpy(c["grad_render64"])) <= 1e-10
    assert torch.equal(r64["gt"], torch.from_numpy(c["gt64"]))
    r32 = mref.masked_loss(render, gt, mi, fg, c["background"], dtype=torch.float32)
    assert torch.equal(r32["gt"], torch.from_numpy(c["gt32"]))          # the composite: the same three fp32 operations
    gaps = _scalar_gaps()
    for k in ("loss", "l1", "ssim"):
        assert abs(r32[k] - float(c[k + "64"])) <= FACTOR * gaps[k], k
    assert rel_l2(r32["grad_render"], torch.from_numpy(c["grad_render64"])) <= min(GRAD_TOL, FACTOR * float(c["gap32_grad_render"]))


def test_restatement_rules():
    """The L1 rule (render_l1 and the gain read the plain render; without either the blend), an all-one mask, the bounds."""
    g = torch.Generator().manual_seed(5)
    r, gt = torch.rand(2, 3, 14, 15, generator=g), torch.rand(2, 3, 14, 15, generator=g)
    m = torch.rand(2, 14, 15, generator=g)
    gain = torch.tensor([[1.1, 0.9, 1.0], [0.8, 1.2, 1.05]])
    plain = mref.masked_loss(r, gt, m)
    x = mref.blend(r.double(), gt.double(), m.double())
    assert abs(plain["l1"] - float((x - gt.double()).abs().mean())) < 1e-15
    rl = r * 1.5
    with_l1 = mref.masked_loss(r, gt, m, render_l1=rl)
    assert abs(with_l1["l1"] - float((rl.double() - gt.double()).abs().mean())) < 1e-15 and with_l1["ssim"] == plain["ssim"]
    with_gain = mref.masked_loss(r, gt, m, gain=gain)
    assert abs(with_gain["l1"] - float((gain.double()[:, :, None, None] * r.double() - gt.double()).abs().mean())) < 1e-15
    assert with_gain["grad_gain"].shape == (2, 3) and with_gain["ssim"] == plain["ssim"]
    ones = mref.masked_loss(r, gt, torch.ones(2, 14, 15))
    assert float(ones["grad_render"].abs().max()) == 0.0 and ones["l1"] == 0.0 and abs(ones["ssim"]) < 1e-15
    mask = np.zeros((2, 7, 9), np.float32)
    mask[0, 2, 3] = mask[0, 5, 8] = 1.0
    mask[1, 1, 1] = 0.5                                    # not above the threshold
    mask[1, 6, 0] = np.nan
    assert mref.bounds_record(mask).tolist() == [[3, 2, 8, 5, 2, 0, 0, 0], [9, 7, -1, -1, 0, 0, 0, 0]]
    assert mref.bounds(mask[:1], 4) == (0, 0, 12, 9) and mref.crop_of((7, 9), (0, 0, 12, 9)) == (0, 0, 7, 9)
    with pytest.raises(IndexError):
        mref.bounds(mask[1:], 0)


# ---- the entry points, as far as they go without a GPU ---------------------------------------------------------------

NAMES = ("lograst_loss_masked_scratch_bytes", "lograst_loss_forward_masked", "lograst_loss_backward_masked",
         "lograst_mask_bounds_bytes", "lograst_mask_bounds", "lograst_mask_bounds_read")


def test_exports_sizes_and_argument_checks():
    import ctypes
    from log_amd import _lib, masked_loss
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name)
    for shape in ((1, 3, 11, 11), (2, 3, 1080, 1920), (1, 1, 43, 44), (2, 3, 100, 70)):
        n = L.lograst_loss_masked_scratch_bytes(*shape)
        assert n % 256 == 0 and n >= L.lograst_loss_scratch_bytes(*shape) and n >= L.lograst_loss_gain_scratch_bytes(*shape)
    assert L.lograst_mask_bounds_bytes(1) == 32 and L.lograst_mask_bounds_bytes(3) == 96 and masked_loss.RECORD_INTS == 8

    s4, s3 = (ctypes.c_int64 * 4)(768, 256, 16, 1), (ctypes.c_int64 * 3)(256, 16, 1)
    P = 0x1000                                               # never dereferenced: every call below fails its checks first

    def fwd(H=16, W=16, B=1, render_l1=None, gain=None, mask=P, fg=None, bg=None, gt_out=None, scratch=P, nbytes=1 << 20, rs=s4):
        return L.lograst_loss_forward_masked(B, 3, H, W, P, rs, render_l1, s4 if render_l1 else None, P, s4, gain, mask,
                                             s3 if mask else None, fg, s3 if fg else None, bg, gt_out, 0.2, 0.8, P, None,
                                             scratch, nbytes, None)

    def bwd(H=16, W=16, render_l1=None, gain=None, mask=P, g_l1=None, g_gain=None, scratch=P, nbytes=1 << 20):
        return L.lograst_loss_backward_masked(1, 3, H, W, P, s4, render_l1, s4 if render_l1 else None, P, s4, gain, mask,
                                              s3 if mask else None, 0.8, P, P, P, g_l1, g_gain, scratch, nbytes, None)

    def fails(rc, words):
        assert rc < 0 and words in L.lograst_last_error(), (rc, L.lograst_last_error())

    fails(fwd(H=10), b"11-pixel window")
    fails(fwd(W=8), b"11-pixel window")
    fails(fwd(B=-1), b"negative")
    fails(fwd(H=40000, W=40000), b"2^31 - 1 image elements")
    fails(fwd(rs=(ctypes.c_int64 * 4)(0, 0, 2 ** 31, 1)), b"strides reach beyond")
    fails(fwd(render_l1=P, gain=P), b"mutually exclusive")
    fails(fwd(mask=None), b"both NULL")
    fails(fwd(fg=P, gt_out=P), b"foreground needs background and gt_out")
    fails(fwd(fg=P, bg=P), b"foreground needs background and gt_out")
    fails(fwd(nbytes=8), b"lograst_loss_masked_scratch_bytes")
    fails(fwd(scratch=P + 4), b"8-byte aligned")
    fails(fwd(scratch=None), b"scratch")
    fails(bwd(H=10), b"11-pixel window")
    fails(bwd(render_l1=P, gain=P), b"mutually exclusive")
    fails(bwd(mask=None), b"mask is NULL")
    fails(bwd(render_l1=0x2000), b"grad_render_l1 is NULL")
    fails(bwd(gain=P), b"NULL pointer")
    fails(bwd(gain=P, g_gain=P, nbytes=8), b"lograst_loss_masked_scratch_bytes")
    fails(L.lograst_mask_bounds(-1, 4, 4, P, s3, 0.5, P, 64, None), b"negative")
    fails(L.lograst_mask_bounds(2, 4, 4, P, s3, 0.5, P, 32, None), b"lograst_mask_bounds_bytes")
    fails(L.lograst_mask_bounds(1, 4, 4, P, s3, 0.5, P + 2, 32, None), b"4-byte aligned")
    fails(L.lograst_mask_bounds(1, 4, 4, None, s3, 0.5, P, 32, None), b"NULL pointer")
    fails(L.lograst_mask_bounds_read(None, 1, None, None), b"NULL pointer")
    assert L.lograst_mask_bounds(0, 4, 4, None, None, 0.5, None, 0, None) == 0          # nothing to do


def test_python_argument_checks():
    from log_amd import _lib, masked_loss as ml
    r, g = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    m = torch.rand(1, 16, 16)
    with pytest.raises(ValueError, match="needs a mask or a foreground"):
        ml.masked_l1_ssim_loss(r, g)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ml.masked_l1_ssim_loss(r, g, mask=m, render_l1=r * 1.1, l1_gain=torch.ones(1, 3))
    with pytest.raises(ValueError, match="background"):
        ml.masked_l1_ssim_loss(r, g, foreground=m)
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        ml.masked_l1_ssim_loss(r, g, mask=m)
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        ml.mask_bounds(m)
    assert ml.enabled() is False


def test_the_switch_inside_both_calculate_loss(monkeypatch):
    """The kernels stood in for by recorders: off, both calculate_loss blend in torch and call what they call today; on,
    each makes ONE call with the mask (and, in view_correction, the gain)."""
    from log_amd import loss, masked_loss as ml, view_correction as vc
    g = torch.Generator().manual_seed(1)
    r, gt = torch.rand(1, 3, 12, 13, generator=g).requires_grad_(True), torch.rand(1, 3, 12, 13, generator=g)
    m = torch.rand(1, 12, 13, generator=g)
    calls = []
    stats = torch.tensor([0.25, 0.5])
    monkeypatch.setattr(loss, "_fusable", lambda *t: all(torch.is_tensor(x) and x.dim() == 4 for x in t))
    monkeypatch.setattr(loss, "_fused", lambda *a: (calls.append(("fused",) + a), (a[0].sum(), stats))[1])
    monkeypatch.setattr(loss, "_fused_gain", lambda *a: (calls.append(("fused_gain",) + a), (a[0].sum(), stats))[1])
    monkeypatch.setattr(ml, "_fused_masked", lambda *a: (calls.append(("masked",) + a), (a[0].sum(), stats, a[1]))[1])
    me = types.SimpleNamespace(ssim_loss=types.SimpleNamespace(window_size=11, padding=0), l1_loss=torch.nn.L1Loss())
    calculate_loss = loss._make_calculate_loss(lambda *a: calls.append(("original",) + a))
    blend = gt * m[:, None] + r * (1 - m[:, None])
    try:
        assert not ml.enabled()
        out = {}
        calculate_loss(me, gt, r, out, m)
        (kind, x, g_, x_l1, a, b), = calls
        assert kind == "fused" and torch.equal(x, blend) and x_l1 is x and g_ is gt and (a, b) == (0.2, 0.8)
        assert out["loss_dict"] == {"l1": 0.25, "ssim": 0.5}
        calls.clear()
        ml.set_enabled(True)
        assert ml.enabled()
        out = {}
        calculate_loss(me, gt, r, out, m)
        assert calls == [("masked", r, gt, m, None, None, None, None, 0.2, 0.8)] and out["loss_dict"] == {"l1": 0.25, "ssim": 0.5}
        calls.clear()
        rc = torch.rand(1, 4, 12, 13, generator=g)
        calculate_loss(me, gt, r, {"render_correct": rc}, m)
        assert calls[0][0] == "masked" and torch.equal(calls[0][6], rc[:, :3]) and calls[0][7] is None
        calls.clear()
        calculate_loss(me, gt, r, {}, None)                          # no mask: today's call, switch or not
        assert calls[0][0] == "fused" and calls[0][1] is r
        calls.clear()
        calculate_loss(me, gt, r, {}, m.double())                    # a mask the kernels do not take: the torch blend
        assert calls[0][0] == "fused" and calls[0][1].dtype == torch.float64
        # view_correction: gain and mask in one call
        calls.clear()
        row = torch.ones(3)
        vc.handed_out.take()
        vc.handed_out.note(row)
        out = {"render_correct": rc}
        with vc.dropins.substituted(calculate_loss=lambda *a: calls.append(("wrapped",) + a)):
            vc.calculate_loss(me, gt, r, out, m)
            assert [c[0] for c in calls] == ["masked"] and calls[0][3] is m and torch.equal(calls[0][7], row[None])
            assert calls[0][6] is None and out["loss_dict"] == {"l1": 0.25, "ssim": 0.5}
            ml.set_enabled(False)
            calls.clear()
            vc.handed_out.note(row)
            vc.calculate_loss(me, gt, r, {"render_correct": rc}, m)
            assert [c[0] for c in calls] == ["fused", "fused_gain"] and torch.equal(calls[0][1], blend)
    finally:
        ml.set_enabled(False)
        vc.handed_out.take()
        vc.reset_stats()


# ---- the drop-ins on the reference's classes -------------------------------------------------------------------------

@pytest.fixture()
def log_path():
    """The reference importable (cv2 stubbed: only its visualisation helpers use it); what the test installs is put back."""
    added = REF not in sys.path
    if added:
        sys.path.insert(0, REF)
    stubs = {}
    if "cv2" not in sys.modules:
        stubs["cv2"] = types.ModuleType("cv2")
    sys.modules.update(stubs)
    old_radius = sys.modules.get("LoG.cuda.compute_radius")
    import log_amd
    log_amd.install_compute_radius()
    yield
    from log_amd import loss, masked_loss, view_correction
    masked_loss.uninstall()
    masked_loss.set_enabled(False)
    view_correction.uninstall()
    loss.uninstall()
    masked_loss.reset_stats()
    if old_radius is not None:
        sys.modules["LoG.cuda.compute_radius"] = old_radius
    else:
        sys.modules.pop("LoG.cuda.compute_radius", None)
    for k in stubs:
        sys.modules.pop(k, None)
    if added:
        sys.path.remove(REF)


needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")


@needs_reference
def test_install_and_uninstall(log_path):
    from log_amd import loss, masked_loss as ml
    from LoG.render.loss import SSIM
    from LoG.render.renderer import MaskForeground, NaiveRendererAndLoss
    bound, forward = MaskForeground.bound_from_mask, MaskForeground.forward
    calc, depth, ssim_forward = NaiveRendererAndLoss.calculate_loss, NaiveRendererAndLoss.append_depth_loss, SSIM.forward
    assert ml.install() is MaskForeground
    assert MaskForeground.bound_from_mask is ml.bound_from_mask and MaskForeground.forward is ml.forward and ml.enabled()
    assert "calculate_loss" not in vars(MaskForeground) and "append_depth_loss" not in vars(MaskForeground)
    assert MaskForeground.calculate_loss._lograst_original is calc           # log_amd.loss, installed first
    assert MaskForeground.append_depth_loss is depth and SSIM.forward._lograst_original is ssim_forward
    assert ml.dropins.original("forward") is forward and ml.dropins.original("bound_from_mask") is bound
    ml.install()                                                             # a second call wraps nothing twice
    assert ml.dropins.original("forward") is forward and MaskForeground.calculate_loss._lograst_original is calc
    ml.uninstall()
    assert (MaskForeground.bound_from_mask, MaskForeground.forward) == (bound, forward) and not ml.enabled()
    assert (NaiveRendererAndLoss.calculate_loss, NaiveRendererAndLoss.append_depth_loss, SSIM.forward) == (calc, depth, ssim_forward)
    # with log_amd.loss installed by the caller and the switch set by the caller, uninstall() leaves both
    loss.install()
    mine = NaiveRendererAndLoss.calculate_loss
    ml.set_enabled(True)
    ml.install()
    ml.uninstall()
    assert NaiveRendererAndLoss.calculate_loss is mine and ml.enabled() and MaskForeground.forward is forward


@needs_reference
def test_install_all_takes_the_flag(log_path):
    import log_amd
    from log_amd import masked_loss as ml
    from LoG.model.counter import Counter
    from LoG.model.level_of_gaussian import LoG
    from LoG.model.sparse_optimizer import SparseOptimizer
    from LoG.model.tensor_tree import TensorTree
    import LoG.render.renderer as ref_renderer
    saved = (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
             ref_renderer.torch)
    forward = ref_renderer.MaskForeground.forward
    try:
        log_amd.install_all()
        assert ref_renderer.MaskForeground.forward is forward and not ml.enabled()
        assert ref_renderer.MaskForeground in log_amd.install_all(masked_loss=True)
        assert ref_renderer.MaskForeground.forward is ml.forward and ml.enabled()
    finally:
        ml.uninstall()
        (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
         ref_renderer.torch) = saved
        if hasattr(SparseOptimizer, "_lograst_load_state_dict"):
            del SparseOptimizer._lograst_load_state_dict
    assert ref_renderer.MaskForeground.forward is forward and not ml.enabled()


@needs_reference
@pytest.mark.parametrize("path", GOLDEN[:2], ids=IDS[:2])
def test_a_cpu_call_falls_back_to_the_recorded_result(log_path, path):
    from log_amd import masked_loss as ml
    from LoG.render.renderer import MaskForeground
    c = mref.load_case(path)

    class FixedRender(MaskForeground):
        def vis(self, batch, model, background=None):
            return {"render": self.leaf}

    ml.install()
    ml.reset_stats()
    module = FixedRender(split="train", use_randback=False, background=c["background"].tolist())
    module.leaf = c["render"].clone().requires_grad_(True)
    batch = {"image": c["image"], "mask": c["mask"]}
    if c["mask_ignore"] is not None:
        batch["mask_ignore"] = c["mask_ignore"]
    output = module(batch, types.SimpleNamespace(training=True))
    output["loss"].backward()
    t, l, h, w = mref.crop_of(c["mask"].shape[1:], [int(v) for v in c["ltrb"]])
    assert np.float32(output["loss"].item()) == c["loss32"]
    assert np.float32(output["loss_dict"]["l1"]) == c["l132"] and np.float32(output["loss_dict"]["ssim"]) == c["ssim32"]
    assert np.array_equal(module.leaf.grad[:, :, t:t + h, l:l + w].numpy(), c["grad_render32"])
    assert np.array_equal(output["gt"].numpy(), c["gt32"]) and list(output["render"].shape) == c["crop_shape"].tolist()
    s = ml.stats()
    assert s["calls"]["forward"] == 1 and s["readbacks"] == {}
    assert s["fallbacks"][("forward", ml.OFF_GPU)] == 1
    assert s["fallbacks"][("bound_from_mask", ml.OFF_GPU)] == 1             # the reference's forward calls the installed method
    # the other splits go straight to vis
    module.split = "val"
    assert module(batch, types.SimpleNamespace(training=False)) == {"render": module.leaf}
