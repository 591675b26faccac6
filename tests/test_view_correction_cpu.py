"""CPU checks of the view correction on the device (log_amd.view_correction, lograst_loss_*_gain, lograst_corrector_step):

* tests/view_correction_ref.py, the float64 restatement the GPU tests lean on, against the reference's own recorded results
  (tests/golden/view_correction_*.npz, written by tests/golden/make_golden_view_correction.py): its float64 evaluation to
  1e-12 relative, its float32 evaluation by the rules the GPU tests apply to the kernels --
    scalars within 8 * gap32 (the largest over the fixtures), grad_render rel-L2 <= min(1e-4, 8 * gap32),
    grad_gain and the row step's state per element within 8 * (|ref32 - ref64| + 2^-24 * S), S the condition scale;
* the drop-ins on the reference's own classes (LOG_REFERENCE; skipped without): install / uninstall, and a CPU Corrector
  driven through the installed methods, which reproduces the recorded trajectory bit for bit through the fall-back;
* the new keyword and entry points: argument checks that need no GPU."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import view_correction_ref as vref  # noqa: E402
from loss_ref import rel_l2  # noqa: E402

REF = os.environ.get("LOG_REFERENCE", "/root/reference")
LOSS = sorted(glob.glob(os.path.join(HERE, "golden", "view_correction_loss_*.npz")))
LOSS_IDS = [os.path.basename(p)[len("view_correction_loss_"):-4] for p in LOSS]
STEPS = sorted(glob.glob(os.path.join(HERE, "golden", "view_correction_steps_*.npz")))
STEP_IDS = [os.path.basename(p)[len("view_correction_steps_"):-4] for p in STEPS]
FACTOR, GRAD_TOL = 8.0, 1e-4


def test_the_fixtures_cover_what_they_should():
    assert LOSS_IDS == ["1x11x11", "2x37x53", "half_equal_40x40", "nhwc_slice_45x70"] and STEP_IDS == ["start0", "start3"]
    z = np.load(STEPS[0])
    assert len(z["index"]) >= 240 and int(z["start_step"]) == 0 and int(z["steps_after"].max()) > 101
    assert {1, 99, 100, 101} <= set(int(s) for s in z["steps_after"])
    assert np.array_equal(z["param_before32"][0], np.ones(3, np.float32))
    z3 = np.load(STEPS[1])
    early = z3["steps_after"] < 3
    assert int(z3["start_step"]) == 3 and early.sum() >= 2 and (~early).sum() >= 2
    assert np.array_equal(z3["grad_after32"][early], z3["grad_before32"][early]) and np.abs(z3["grad_after32"][early]).min() > 0
    h = np.load(LOSS[2])
    n = int(h["equal_left"])
    assert np.array_equal(h["gt"][..., :n], (h["gain"][:, :, None, None] * h["render"])[..., :n])
    assert float(np.abs(h["grad_gain32"]).min()) > 0


def _scalar_gaps():
    zs = [np.load(p) for p in LOSS]
    return {k: max(float(z["gap32_" + k]) for z in zs) for k in ("l1", "ssim", "loss")}


@pytest.mark.parametrize("path", LOSS, ids=LOSS_IDS)
def test_restatement_of_the_loss_against_the_reference(path):
    c = vref.load_loss_case(path)
    # (the reference's SSIM buffer -- its fp32 outer product, not the library's separable taps -- as the loss fixtures hold it)
    window = torch.from_numpy(np.load(os.path.join(HERE, "golden", "loss_1x11x11.npz"))["window"]).double()
    r64 = vref.loss_gain(c["render"], vref.gt_for(c, torch.float64), c["gain"], window=window)
    for k in ("loss", "l1", "ssim"):
        assert abs(r64[k] - float(c[k + "64"])) <= 1e-12 * abs(float(c[k + "64"])), k
    for k in ("grad_render", "grad_gain"):
        want = torch.from_numpy(c[k + "64"])
        assert float((r64[k] - want).abs().max()) <= 1e-12 * float(want.abs().max()), k
    r32 = vref.loss_gain(c["render"], vref.gt_for(c, torch.float32), c["gain"], dtype=torch.float32)
    gaps = _scalar_gaps()
    for k in ("loss", "l1", "ssim"):
        assert abs(r32[k] - float(c[k + "64"])) <= FACTOR * gaps[k], k
    assert rel_l2(r32["grad_render"], torch.from_numpy(c["grad_render64"])) <= min(GRAD_TOL, FACTOR * float(c["gap32_grad_render"]))
    ok, ratio = vref.within(r32["grad_gain"], c["grad_gain32"], c["grad_gain64"], r64["S_gain"])
    assert ok, ratio
    if "equal_left" in c:             # the L1 term alone: exactly zero where gt == gain * render
        n = int(c["equal_left"])
        only = vref.l1_gain(c["render"], vref.gt_for(c, torch.float32), c["gain"], dtype=torch.float32)["grad_render"]
        assert float(only[..., :n].abs().max()) == 0.0 and float(only[..., n:].abs().min()) > 0.0


@pytest.mark.parametrize("path", STEPS, ids=STEP_IDS)
def test_restatement_of_the_row_step_against_the_reference(path):
    z = np.load(path)
    start, lr_init, lr_final = int(z["start_step"]), float(z["lr_init"]), float(z["lr_final"])
    worst = 0.0
    for t in range(len(z["index"])):
        for suffix, dtype in (("64", torch.float64), ("32", torch.float32)):
            before = vref.step_rows(z, t, "before", suffix)
            steps, after, S = vref.corrector_step(before, z["steps_before"][t], start, lr_init, lr_final, dtype=dtype)
            assert steps == int(z["steps_after"][t])
            if after is None:
                after, S = before, {k: torch.zeros(3) for k in before}        # an early return: nothing else changes
            for k in vref.STATE:
                want64, want32 = z[f"{k}_after64"][t], z[f"{k}_after32"][t]
                if suffix == "64":
                    got, want = after[k].numpy(), want64
                    assert np.array_equal(np.isnan(got), np.isnan(want)), (t, k)
                    m = ~np.isnan(want)
                    assert np.all(np.abs(got[m] - want[m]) <= 1e-12 * np.abs(want[m])), (t, k, got, want)
                else:
                    ok, ratio = vref.within(after[k], want32, want64, S[k])
                    worst = max(worst, ratio)
                    assert ok, (t, k, after[k], want32, want64)
    print(f"largest error / bound of the float32 restatement: {worst:.3f}")


# ---- the keyword and the entry points, as far as they go without a GPU -----------------------------------------------

def test_keyword_and_argument_checks():
    from log_amd import _lib, loss
    r, g = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    with pytest.raises(ValueError, match="mutually exclusive"):
        loss.l1_ssim_loss(r, g, render_l1=r * 1.1, l1_gain=torch.ones(1, 3))
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        loss.l1_ssim_loss(r, g, l1_gain=torch.ones(1, 3))
    L = _lib.lib()
    for name in ("lograst_loss_gain_scratch_bytes", "lograst_loss_forward_gain", "lograst_loss_backward_gain",
                 "lograst_corrector_step"):
        assert name in _lib.EXPORTS
    # one double per 32 x 32 image tile and plane, never less than the forward's float pair per output tile
    assert L.lograst_loss_gain_scratch_bytes(2, 3, 100, 70) == (8 * 4 * 3 * 6 + 255) // 256 * 256
    for shape in ((1, 3, 11, 11), (2, 3, 1080, 1920), (1, 1, 43, 44)):
        assert L.lograst_loss_gain_scratch_bytes(*shape) >= L.lograst_loss_scratch_bytes(*shape)
    # validation happens on the host, before any device work
    for args, words in (((2, 3, 2, 0), b"index outside"), ((2, 3, -1, 0), b"index outside"), ((2, 65, 0, 0), b"width"),
                        ((0, 3, 0, 0), b"views")):
        assert L.lograst_corrector_step(*args, 0.1, 0.001, *([None] * 7)) < 0 and words in L.lograst_last_error()
    assert L.lograst_corrector_step(2, 3, 0, 0, 0.0, 0.001, *([None] * 7)) < 0 and b"positive" in L.lograst_last_error()
    assert L.lograst_corrector_step(2, 3, 0, 0, 0.1, 0.001, *([None] * 7)) < 0 and b"NULL" in L.lograst_last_error()
    assert L.lograst_loss_forward_gain(1, 3, 8, 16, *([None] * 5), 0.2, 0.8, None, None, None, 0, None) < 0
    assert b"11-pixel window" in L.lograst_last_error()


def test_handed_out_rows_stay_bounded():
    from log_amd import view_correction as vc
    vc.handed_out.take()
    for i in range(10 * vc.MAX_NOTED):
        vc.handed_out.note(torch.zeros(3))
    assert len(vc.handed_out.rows) == vc.MAX_NOTED
    count, rows = vc.handed_out.take()
    assert count == 10 * vc.MAX_NOTED and len(rows) == vc.MAX_NOTED and vc.handed_out.take() == (0, [])


# ---- the drop-ins on the reference's classes -------------------------------------------------------------------------

@pytest.fixture()
def log_path():
    """The reference importable (cv2 stubbed: only its visualisation helpers use it); what the test installs is put back."""
    import types
    added = REF not in sys.path
    if added:
        sys.path.insert(0, REF)
    stubs = {}
    if "cv2" not in sys.modules:
        stubs["cv2"] = types.ModuleType("cv2")
    sys.modules.update(stubs)
    old_radius = sys.modules.get("LoG.cuda.compute_radius")
    import log_amd
    log_amd.install_compute_radius()                      # level_of_gaussian.py imports it at import time
    yield
    from log_amd import loss, view_correction
    view_correction.uninstall()
    loss.uninstall()
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
def test_install_and_uninstall_replace_and_restore_the_three_methods(log_path):
    from log_amd import view_correction as vc
    from LoG.model.corrector import Corrector
    from LoG.render.loss import SSIM
    from LoG.render.renderer import NaiveRendererAndLoss
    step, getitem, calc, ssim_forward = Corrector.step, Corrector.__getitem__, NaiveRendererAndLoss.calculate_loss, SSIM.forward
    assert vc.install() is Corrector
    assert Corrector.step is vc.step and Corrector.__getitem__ is vc.__getitem__
    assert NaiveRendererAndLoss.calculate_loss is vc.calculate_loss
    wrapped = vc.dropins.original("calculate_loss")           # log_amd.loss's method, itself around the reference's
    assert wrapped._lograst_original is calc and SSIM.forward._lograst_original is ssim_forward
    vc.install()                                              # a second call wraps nothing twice
    assert vc.dropins.original("calculate_loss") is wrapped and vc.dropins.original("step") is step
    # CPU tensors: the loss goes through both wrappers to the reference's own code
    g = torch.Generator().manual_seed(3)
    a, b = torch.rand(2, 3, 24, 31, generator=g), torch.rand(2, 3, 24, 31, generator=g)
    r = NaiveRendererAndLoss(split="train", use_origin_render=False, background=[1., 1., 1.])
    out_p, out_o = {}, {}
    vc.reset_stats()
    r.calculate_loss(b, a.clone().requires_grad_(True), out_p)
    calc(r, b, a.clone().requires_grad_(True), out_o)
    assert torch.equal(out_p["loss"], out_o["loss"]) and out_p["loss_dict"] == out_o["loss_dict"]
    assert vc.stats()["fallbacks"] == {("calculate_loss", "no render_correct in output"): 1}
    vc.uninstall()
    assert (Corrector.step, Corrector.__getitem__, NaiveRendererAndLoss.calculate_loss, SSIM.forward) == (step, getitem, calc, ssim_forward)
    # with log_amd.loss installed by the caller, uninstall() leaves it in place
    from log_amd import loss
    loss.install()
    mine = NaiveRendererAndLoss.calculate_loss
    vc.install()
    vc.uninstall()
    assert NaiveRendererAndLoss.calculate_loss is mine and mine._lograst_original is calc


@needs_reference
def test_install_all_takes_the_flag(log_path):
    import log_amd
    from log_amd import view_correction as vc
    from LoG.model.corrector import Corrector
    from LoG.model.counter import Counter
    from LoG.model.level_of_gaussian import LoG
    from LoG.model.sparse_optimizer import SparseOptimizer
    from LoG.model.tensor_tree import TensorTree
    import LoG.render.renderer as ref_renderer
    saved = (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
             ref_renderer.torch)
    step = Corrector.step
    try:
        log_amd.install_all()
        assert Corrector.step is step
        assert Corrector in log_amd.install_all(device_view_correction=True) and Corrector.step is vc.step
        assert ref_renderer.NaiveRendererAndLoss.calculate_loss is vc.calculate_loss
    finally:
        vc.uninstall()
        (TensorTree.traverse, Counter.update_by_output, SparseOptimizer.step, SparseOptimizer.load_state_dict, LoG.get_all,
         ref_renderer.torch) = saved
        if hasattr(SparseOptimizer, "_lograst_load_state_dict"):
            del SparseOptimizer._lograst_load_state_dict
    assert Corrector.step is step


@needs_reference
@pytest.mark.parametrize("path", STEPS, ids=STEP_IDS)
def test_cpu_corrector_through_the_dropins_reproduces_the_trajectory(log_path, path, capsys):
    """The generator's loop with the installed methods: every call falls back (the tensors are on the CPU), so the fp32
    trajectory is the recorded one to the bit."""
    from log_amd import view_correction as vc
    from LoG.model.corrector import Corrector
    vc.install()
    vc.reset_stats()
    z = np.load(path)
    render, gt = torch.from_numpy(z["render"]), torch.from_numpy(z["gt"])
    cor = Corrector(True, start_step=int(z["start_step"]))
    cor.init(render.shape[0])
    cor.training_setup()
    l1_loss = torch.nn.L1Loss()
    opt = cor.optimizer
    for t, i in enumerate(int(i) for i in z["index"]):
        row = cor[i]
        (0.8 * l1_loss((render[i] * row[:, None, None])[None][:, :3], gt[i][None])).backward()
        assert np.array_equal(cor.view_correction.grad[i].numpy(), z["grad_before32"][t], equal_nan=True), t
        cor.step()
        state = dict(param=cor.view_correction.data[i], grad=cor.view_correction.grad[i],
                     exp_avg=opt.exp_avg["view_correction"][i], exp_avg_sq=opt.exp_avg_sq["view_correction"][i],
                     max_exp_avg_sq=opt.max_exp_avg_sq["view_correction"][i])
        assert int(opt.steps["view_correction"][i]) == int(z["steps_after"][t])
        for k, v in state.items():
            assert np.array_equal(v.numpy(), z[k + "_after32"][t], equal_nan=True), (t, k)
    T = len(z["index"])
    s = vc.stats()
    assert s["calls"]["step"] == T and s["calls"]["__getitem__"] == T
    assert s["fallbacks"] == {("step", "tensors are not on the GPU"): T}
    assert vc.handed_out.count == T and len(vc.handed_out.rows) == min(T, vc.MAX_NOTED)
