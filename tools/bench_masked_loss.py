"""Stage benchmark of the masked training loss (log_amd.masked_loss) on the foreground step of MaskForeground.forward
(LoG/render/renderer.py:343-370) at 1920x1080 with a 1100x700 crop: bounds of the mask, crop, composite of the ground
truth over the background, mask_ignore blend, loss, backward to the full render, and the read-back for loss_dict.

    python tools/bench_masked_loss.py [--reps 30] [--warmup 5]   -> one JSON line

Per-step arms, alternated inside one process (every shape warmed up first), wall-clock between two device
synchronisations, medians and the spread (10th / 90th percentile) over --reps:
  reference  the torch operations an unmodified LoG process issues, restated here from what they compute: `> 0.5`, `any` per axis,
             `nonzero`, python's max(tensor, 0), four tensor-bounded cuts, the composite and the blend as element-wise torch, five
             grouped conv2d + the SSIM chain + l1_loss
  parent     the same torch bounds, composite and blend around the fused loss (log_amd.loss.l1_ssim_loss)
  masked     log_amd.masked_loss: mask_bounds_host, views, ONE masked_l1_ssim_loss call
Kernel-time arms, HIP events around the C entry points called back to back (no autograd, no allocation in between):
  masked     lograst_loss_forward_masked (mask + foreground) / lograst_loss_backward_masked on the crop, lograst_mask_bounds
  unmasked   lograst_loss_forward / lograst_loss_backward on the same crop
Counted, not timed, per step and arm: device launches (torch.profiler kernel events; null where the profiler is not
available) and host synchronisations (torch's sync debug mode, plus the library's own read-backs)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import warnings

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from log_amd import _lib  # noqa: E402
from log_amd.loss import l1_ssim_loss, window_taps  # noqa: E402
from log_amd.masked_loss import mask_bounds_host, masked_l1_ssim_loss  # noqa: E402

dev = torch.device("cuda:0")
H, W = 1080, 1920
BOX = (161, 784, 495, 1518)        # rows, columns of the foreground: padding int(1920 / 50) = 38 -> crop 700 x 1100 at (123, 457)


def make_batch(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    render = torch.rand(1, 3, H, W, device=dev, generator=g)
    image = (render.permute(0, 2, 3, 1) + 0.1 * torch.randn(1, H, W, 3, device=dev, generator=g)).clamp(0, 1).contiguous()
    mask = torch.zeros(1, H, W, device=dev)
    mask[:, BOX[0]:BOX[1] + 1, BOX[2]:BOX[3] + 1] = 1.0
    ignore = (torch.rand(1, H, W, device=dev, generator=g) > 0.8).float()
    return {"render": render, "image": image, "mask": mask, "mask_ignore": ignore,
            "background": torch.tensor([0.2, 0.5, 0.8], device=dev)}


def occupied_range(flags):
    """flags: bool [N] on the device -> (first, last) set index as 0-dim device tensors (one nonzero: a synchronisation)."""
    index = torch.nonzero(flags, as_tuple=True)[0]
    return index[0], index[-1]


def box_of(mask, pad):
    """Bounding box of mask[0] > 0.5, grown by pad and clamped at 0 on the low side only -> (x_lo, y_lo, x_hi, y_hi): the low
    bounds through python's max on a 0-dim device tensor (a synchronisation each), the high bounds 0-dim device tensors."""
    above = mask[0] > 0.5
    x_first, x_last = occupied_range(above.any(dim=0))
    y_first, y_last = occupied_range(above.any(dim=1))
    return max(x_first - pad, 0), max(y_first - pad, 0), x_last + pad, y_last + pad


def cut_to(t, box, ydim):
    """t cut to the box along (ydim, ydim + 1), both ends inclusive: four bounds handed to the slice as they are (0-dim device
    tensors synchronise when the slice reads them), the `+ 1` of the upper ends taken per cut."""
    x_lo, y_lo, x_hi, y_hi = box
    index = [slice(None)] * t.dim()
    index[ydim], index[ydim + 1] = slice(y_lo, y_hi + 1), slice(x_lo, x_hi + 1)
    return t[tuple(index)]


def torch_ssim(window):
    def ssim_loss(img1, img2):
        mu1 = F.conv2d(img1, window, groups=3)
        mu2 = F.conv2d(img2, window, groups=3)
        mu1_sq, mu2_sq, mu1_mu2 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s11 = F.conv2d(img1 * img1, window, groups=3) - mu1_sq
        s22 = F.conv2d(img2 * img2, window, groups=3) - mu2_sq
        s12 = F.conv2d(img1 * img2, window, groups=3) - mu1_mu2
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        ssim_map = ((2 * mu1_mu2 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s11 + s22 + C2))
        return 1.0 - ssim_map.mean()
    return ssim_loss


def torch_front(batch, leaf):
    """Bounds, crop, composite and blend as torch operations on the device -> (blend, gt), both [1, 3, h, w]."""
    mask = batch["mask"]
    box = box_of(mask, int(max(tuple(mask.shape)) / 50))
    fg = cut_to(mask, box, 1)[..., None]                                           # [1, h, w, 1] against the [1, h, w, 3] image
    gt = (cut_to(batch["image"], box, 1) * fg + (1 - fg) * batch["background"]).permute(0, 3, 1, 2)
    ignore = cut_to(batch["mask_ignore"], box, 1)[:, None]
    return gt * ignore + cut_to(leaf[:, :3], box, 2) * (1 - ignore), gt


def arms(taps):
    ssim_loss = torch_ssim(taps)

    def reference(batch, leaf):
        render, gt = torch_front(batch, leaf)
        ssim, l1 = ssim_loss(render, gt), F.l1_loss(render, gt)
        values = {"l1": l1.item(), "ssim": ssim.item()}
        (0.2 * ssim + 0.8 * l1).backward()
        return values

    def parent(batch, leaf):
        render, gt = torch_front(batch, leaf)
        loss, l1, ssim = l1_ssim_loss(render, gt)
        l1_value, ssim_value = torch.stack([l1, ssim]).tolist()
        loss.backward()
        return {"l1": l1_value, "ssim": ssim_value}

    def masked(batch, leaf):
        mask = batch["mask"]
        l, t, r, b = mask_bounds_host(mask, int(max(tuple(mask.shape) + (1,)) / 50))
        render = leaf[:, :3][:, :, t:b + 1, l:r + 1]
        gt = batch["image"].permute(0, 3, 1, 2)[:, :, t:b + 1, l:r + 1]
        loss, l1, ssim, _ = masked_l1_ssim_loss(render, gt, batch["mask_ignore"][:, t:b + 1, l:r + 1], mask[:, t:b + 1, l:r + 1],
                                                batch["background"])
        l1_value, ssim_value = torch.stack([l1, ssim]).tolist()
        loss.backward()
        return {"l1": l1_value, "ssim": ssim_value}
    return {"reference": reference, "parent": parent, "masked": masked}


def spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(f * len(xs)))]
    return {"median_us": statistics.median(xs), "p10_us": q(0.1), "p90_us": q(0.9), "min_us": xs[0], "max_us": xs[-1]}


def time_steps(fns, batches, warmup, reps):
    times = {k: [] for k in fns}
    values = {}
    for it in range(warmup + reps):
        batch = batches[it % len(batches)]
        for name, fn in fns.items():
            leaf = batch["render"].detach().requires_grad_(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            values[name] = fn(batch, leaf)
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e6)
    return {k: spread(v) for k, v in times.items()}, values


def count_step(fn, batch, own_syncs):
    """-> (launches or None, host synchronisations) of one step."""
    leaf = batch["render"].detach().requires_grad_(True)
    syncs = None
    try:
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                fn(batch, leaf)
            syncs = sum("synchroniz" in str(w.message) for w in caught) + own_syncs
        finally:
            torch.cuda.set_sync_debug_mode("default")
    except RuntimeError as why:        # a torch build without the sync debug mode: the count is reported as not taken
        print("synchronisation count not taken:", why, file=sys.stderr)
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        leaf = batch["render"].detach().requires_grad_(True)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn(batch, leaf)
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                       and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
    except Exception as why:           # the profiler is optional here: the count is then reported as not taken
        print("launch count not taken:", why, file=sys.stderr)
    return launches, syncs


def time_entry_points(batch, warmup, reps):
    L = _lib.lib()
    t, b, l, r = 123, 822, 457, 1556
    render = batch["render"][:, :, t:b + 1, l:r + 1]
    gt = batch["image"].permute(0, 3, 1, 2)[:, :, t:b + 1, l:r + 1]
    fg, mi = batch["mask"][:, t:b + 1, l:r + 1], batch["mask_ignore"][:, t:b + 1, l:r + 1]
    B, C, h, w = render.shape
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    s4 = lambda x: (ctypes.c_int64 * 4)(*x.stride())
    s3 = lambda x: (ctypes.c_int64 * 3)(*x.stride())
    out3, one = torch.empty(3, device=dev), torch.ones(1, device=dev)
    maps = torch.empty(3 * B * C * (h - 10) * (w - 10), device=dev)
    nbytes = L.lograst_loss_masked_scratch_bytes(B, C, h, w)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    grad, gt_out = torch.empty(B, C, h, w, device=dev), torch.empty(B, C, h, w, device=dev)
    record = torch.empty(8, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    bg = batch["background"]

    def masked_fwd():
        _lib.check(L.lograst_loss_forward_masked(B, C, h, w, ptr(render), s4(render), None, None, ptr(gt), s4(gt), None, ptr(mi),
                                                 s3(mi), ptr(fg), s3(fg), ptr(bg), ptr(gt_out), 0.2, 0.8, ptr(out3), ptr(maps),
                                                 ptr(scratch), nbytes, stream))

    def masked_bwd():
        _lib.check(L.lograst_loss_backward_masked(B, C, h, w, ptr(render), s4(render), None, None, ptr(gt_out), s4(gt_out), None,
                                                  ptr(mi), s3(mi), 0.8, ptr(one), ptr(maps), ptr(grad), None, None, None, 0, stream))

    def plain_fwd():
        _lib.check(L.lograst_loss_forward(B, C, h, w, ptr(render), s4(render), None, None, ptr(gt), s4(gt), 0.2, 0.8, ptr(out3),
                                          ptr(maps), ptr(scratch), nbytes, stream))

    def plain_bwd():
        _lib.check(L.lograst_loss_backward(B, C, h, w, ptr(render), s4(render), None, None, ptr(gt), s4(gt), 0.8, ptr(one),
                                           ptr(maps), ptr(grad), None, stream))

    def bounds():
        m = batch["mask"]
        _lib.check(L.lograst_mask_bounds(1, H, W, ptr(m), s3(m), 0.5, ptr(record), 32, stream))

    pairs = {"masked": (masked_fwd, masked_bwd), "unmasked": (plain_fwd, plain_bwd)}
    times = {k: ([], []) for k in pairs}
    times_bounds = []
    for it in range(warmup + reps):
        for name, (fwd, bwd) in pairs.items():
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            fwd()
            e[1].record()
            bwd()
            e[2].record()
            e[2].synchronize()
            if it >= warmup:
                times[name][0].append(e[0].elapsed_time(e[1]) * 1e3)
                times[name][1].append(e[1].elapsed_time(e[2]) * 1e3)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        bounds()
        e[1].record()
        e[1].synchronize()
        if it >= warmup:
            times_bounds.append(e[0].elapsed_time(e[1]) * 1e3)
    out = {k: {"fwd_kernel": spread(f), "bwd_kernel": spread(b)} for k, (f, b) in times.items()}
    out["mask_bounds_1080p"] = spread(times_bounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_masked_loss needs the MI355X"
    window = window_taps().to(dev)
    window = (window[:, None] * window[None, :]).expand(3, 1, 11, 11).contiguous()
    fns = arms(window)
    batches = [make_batch(s) for s in (1, 2, 3)]
    steps, values = time_steps(fns, batches, a.warmup, a.reps)
    counts = {}
    for name, fn in fns.items():
        launches, syncs = count_step(fn, batches[0], 1 if name == "masked" else 0)
        counts[name] = {"launches": launches, "host_synchronisations": syncs}
    kernels = time_entry_points(batches[0], a.warmup, a.reps)
    result = {"workload": "MaskForeground step, 1920x1080, crop 1100x700 at (123, 457), B=1 C=3 fp32: bounds + composite + blend "
                          "+ loss + backward + loss_dict", "reps": a.reps, "warmup": a.warmup, "step": steps, "counted": counts,
              "entry_points_crop_700x1100": kernels, "last_values": values}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
