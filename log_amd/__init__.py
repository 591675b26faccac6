"""lograst: the LoG rasterizer hot path (and the callers either side of it) on MI355X.  See README.md / DESIGN.md."""
import sys
import types


def install_compute_radius():
    """Register this repo's ``compute_radius_module`` as the module ``LoG.cuda.compute_radius`` so that
    ``from LoG.cuda.compute_radius import compute_radius_module`` (/root/reference/LoG/model/level_of_gaussian.py:11,
    executed at import time) resolves to the HIP kernel instead of JIT-compiling the reference's CUDA file -- no
    reference file needs editing.  Call before LoG.model is imported."""
    from .compute_radius import compute_radius_module
    shim = types.ModuleType("LoG.cuda.compute_radius")
    shim.compute_radius_module = compute_radius_module
    shim.__doc__ = "log_amd stand-in for LoG/cuda/compute_radius.py (HIP kernel behind lograst_compute_radius)"
    sys.modules["LoG.cuda.compute_radius"] = shim
    return shim


def uninstall_abs_grad():
    """What install_all(abs_grad=True) switched on, off again: the rasterizer's switch and the counter's."""
    from . import counter, rasterizer
    rasterizer.set_abs_grad(False)
    counter.set_abs_grad(False)


def install_all(fused_step=False, fused_loss=False, reuse_geometry=False, fused_depth_loss=False, device_densify=False,
                device_prepare=False, device_decide=False, device_view_correction=False, device_evaluate=False, device_init=False,
                views_per_step=None, masked_loss=False, fused_depth_pass=False, abs_grad=False):
    """Everything a LoG process needs, in one call: the LoG.cuda.compute_radius module, then every
    drop-in method assigned onto LoG's own classes (needs LoG importable): LoG.get_all, TensorTree.traverse,
    Counter.update_by_output, SparseOptimizer.step.
    fused_step (opt-in, round 6): the backward of LoG.get_all applies SparseOptimizer's update itself, in the kernel that
    computes the raw gradients (log_amd.get_all.set_fused_step: the update then happens at backward time -- the same result
    for LoG's trainer, one backward per step).
    fused_loss (opt-in): SSIM.forward and NaiveRendererAndLoss.calculate_loss go through the fused L1 + SSIM kernels
    (log_amd.loss.install); without it the loss stays the reference's torch code.
    reuse_geometry (opt-in): the second rasterizer call of a view (LoG's depth pass, render_depth: True) composites the first
    call's tile lists again with its own colours instead of binning again (log_amd.rasterizer.set_geometry_reuse: same
    results; a rasterizer object then keeps one forward's records and lists alive until its next call).
    fused_depth_loss (opt-in): NaiveRendererAndLoss.append_depth_loss (the depth term of render_depth: True) goes through the
    fused patch-loss kernels (log_amd.depth_loss.install: double arithmetic, no read-backs); without it the depth term stays
    the reference's torch code, whatever fused_loss says.
    device_densify (opt-in): TensorTree.split_and_remove, Splitter.split_and_remove and Splitter.split_and_remove_other resize
    the model, the Adam moments and the tree on the device (log_amd.densify.install: one host synchronisation per call, no
    copy of the model to the CPU); without it densification stays the reference's code.
    device_prepare (opt-in): LoG.prepare, Gaussian.prepare, LoG.clamp_scale and LoG.step run their frustum test, root filter,
    leaf / node split and scale clamp on the device (log_amd.prepare.install: two host synchronisations per view, none per
    step, no activation of all points to index out the roots); without it they stay the reference's torch code around the
    installed TensorTree.traverse.
    device_decide (opt-in): LoG.update_depth_stage and LoG.update_init_stage compute their split / remove flags, the top-k cut
    and every logged statistic on the device (log_amd.decide.install: one read-back of a fixed-size record per event), then
    call the installed split_and_remove methods; without it the decisions stay the reference's torch code.
    device_view_correction (opt-in): Corrector.step becomes one launch with the row's step count and learning-rate schedule
    on the device (no host synchronisation), Corrector.__getitem__ notes the rows it hands out, and
    NaiveRendererAndLoss.calculate_loss gives them to the loss kernels as a per-image channel gain instead of reading
    render_correct (log_amd.view_correction.install, which installs log_amd.loss as well: one image gradient, the gain's
    gradient from the same kernel); without it the Corrector stays the reference's torch code.
    device_evaluate (opt-in): Trainer.make_validation, LoG.utils.metric.psnr / ssim and BaseRender.tensor_to_bgr compute the
    view-correction fit, L1, PSNR, the metric's SSIM and the 8-bit image on the device (log_amd.evaluate.install: one
    read-back of a 128-byte record per image, plus the 8-bit copy when an image is written); without it evaluation stays
    the reference's torch and numpy code.
    device_init (opt-in): LoG.init, Gaussian.init_radius3d and LoG.at_init_final run the initialisation pass of Trainer.init
    on the device (log_amd.init_pass.install with views_per_launch left at 1: one launch per view over all points, no host
    synchronisation, the state after every call the reference's); without it the pass stays the reference's torch code
    around the installed compute_radius.
    views_per_step (opt-in, an integer K >= 1): LoG.step takes ONE Adam step per K calls, over every row that one of the K
    views saw, from gradients that the backward of LoG.get_all added by model row (log_amd.multi_view.install, installed
    after device_prepare so that its fall-back is that module's step); None installs nothing: every step is one view wide.
    masked_loss (opt-in): a mask_ignore in calculate_loss is blended inside the loss kernels, and MaskForeground.forward /
    bound_from_mask take the mask's bounding box from one kernel, crop by views and composite the ground truth inside the
    same loss call (log_amd.masked_loss.install, which installs log_amd.loss as well: two read-backs per foreground step,
    the bounds and loss_dict); without it masks stay torch code around the loss.
    fused_depth_pass (opt-in): NaiveRendererAndLoss.render hands the reference's own render a proxy around the rasterizer, so
    that a render_depth: True view composites [view z, world z, 1] in the walk of its colour call and its second rasterizer
    call launches nothing (log_amd.depth_pass.install: same depth / height / accmap bits, one reverse walk and one chain rule
    for both images; quadrant kernels only -- see INTEGRATION 3b for where that is slower); reuse_geometry then has nothing
    left to reuse on such a view.
    abs_grad (opt-in): every rasterizer backward also sums the ABSOLUTE per-pixel terms of dL/dmeans2D
    (log_amd.rasterizer.set_abs_grad: ``means2D.absgrad``), and Counter.update_by_output accumulates their norm into grad_sum
    where the signed gradient's went (log_amd.counter.set_abs_grad) -- the AbsGS statistic under LoG's split decision.
    split_grad_thres was tuned for the signed statistic and the absolute one is larger: nothing is retuned here (INTEGRATION
    3b).  A render_depth: True view then takes two real rasterizer calls (fused_depth_pass falls back, reason abs_grad).
    ``uninstall_abs_grad()`` switches both off again."""
    install_compute_radius()
    from . import rasterizer
    rasterizer.set_geometry_reuse(bool(reuse_geometry))
    from . import counter, get_all, lod, sparse_optimizer
    if abs_grad:
        rasterizer.set_abs_grad(True)
        counter.set_abs_grad(True)
    get_all.set_fused_step(bool(fused_step))
    installed = [m.install() for m in (get_all, lod, counter, sparse_optimizer)]
    if fused_loss:
        from . import loss
        installed.append(loss.install())
    if fused_depth_loss:
        from . import depth_loss
        installed.append(depth_loss.install())
    if device_densify:
        from . import densify
        installed.append(densify.install())
    if device_prepare:
        from . import prepare
        installed.append(prepare.install())
    if views_per_step is not None:
        from . import multi_view
        installed.append(multi_view.install(views_per_step=views_per_step))
    if device_decide:
        from . import decide
        installed.append(decide.install())
    if device_view_correction:
        from . import view_correction
        installed.append(view_correction.install())
    if masked_loss:
        from . import masked_loss as masked
        installed.append(masked.install())
    if device_evaluate:
        from . import evaluate
        installed.append(evaluate.install())
    if device_init:
        from . import init_pass
        installed.append(init_pass.install())
    if fused_depth_pass:
        from . import depth_pass
        installed.append(depth_pass.install())
    return installed
