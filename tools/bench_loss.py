"""Stage benchmark of the training loss (log_amd.loss.l1_ssim_loss: lograst_loss_forward / _backward) against the torch
ops an unmodified LoG process runs (LoG/render/loss.py:26-44 + nn.L1Loss + autograd), written here from the formula: five
grouped 11x11 conv2d + the element-wise SSIM chain + l1_loss, `gt` a channels-last view as LoG passes it.

    python tools/bench_loss.py [--reps 20] [--warmup 5] [--sizes 1920x1080,3840x2160] [--no-baseline]   -> one JSON line

Per size (B = 1, C = 3, fp32, one device), median over --reps after --warmup:
  *_call_us    HIP events around the Python call (what a training step pays: kernels + launch gaps)
  *_kernel_us  HIP events around the C entry points alone (lograst_loss_forward = forward kernel + reduction,
               lograst_loss_backward), called back to back without autograd in between
  warm = the same image pair every repetition (both tensors stay in the 256 MiB Infinity Cache)
  cold = cycling through enough distinct pairs to exceed twice that cache
Algorithmic bytes: forward reads 2 * 4C and writes 3 * 4C per pixel, backward reads 5 * 4C and writes 4C: 11 * 4C = 132 B
per pixel at C = 3; achieved bytes/s = that over the kernel time, next to the rate lograst_stream_copy reaches in the
same run."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from log_amd import _lib  # noqa: E402
from log_amd.loss import l1_ssim_loss, window_taps  # noqa: E402

dev = torch.device("cuda:0")


def make_pairs(count, H, W, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    pairs = []
    for _ in range(count):
        render = torch.rand(1, 3, H, W, device=dev, generator=g)
        gt = (render + 0.1 * torch.randn(1, H, W, 3, device=dev, generator=g).permute(0, 3, 1, 2)).clamp(0, 1)
        gt = gt.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)       # [B,H,W,3] permuted: LoG's batch['image']
        pairs.append((render, gt))
    return pairs


def torch_loss(window):
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

    def loss(render, gt):
        return 0.2 * ssim_loss(render, gt) + 0.8 * F.l1_loss(render, gt), None, None
    return loss


def time_calls(fn, pairs, warmup, reps):
    """-> medians in us of the Python calls: forward, backward, both."""
    fwd, bwd, both = [], [], []
    for it in range(warmup + reps):
        render, gt = pairs[it % len(pairs)]
        r = render.detach().requires_grad_(True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        loss = fn(r, gt)[0]
        e[1].record()
        loss.backward()
        e[2].record()
        e[2].synchronize()
        if it >= warmup:
            fwd.append(e[0].elapsed_time(e[1]) * 1e3)
            bwd.append(e[1].elapsed_time(e[2]) * 1e3)
            both.append(e[0].elapsed_time(e[2]) * 1e3)
    return {"fwd_call_us": statistics.median(fwd), "bwd_call_us": statistics.median(bwd), "both_call_us": statistics.median(both)}


def time_entry_points(pairs, warmup, reps):
    """-> medians in us of lograst_loss_forward / lograst_loss_backward called directly (no autograd, no allocation between
    them): what the kernels themselves take."""
    L = _lib.lib()
    B, C, H, W = pairs[0][0].shape
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    strides = lambda t: (ctypes.c_int64 * 4)(*t.stride())
    out3 = torch.empty(3, device=dev)
    maps = torch.empty(3 * B * C * (H - 10) * (W - 10), device=dev)
    nbytes = L.lograst_loss_scratch_bytes(B, C, H, W)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    grad = torch.empty(B, C, H, W, device=dev)
    one = torch.ones(1, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    fwd, bwd = [], []
    for it in range(warmup + reps):
        r, g = pairs[it % len(pairs)]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _lib.check(L.lograst_loss_forward(B, C, H, W, ptr(r), strides(r), None, None, ptr(g), strides(g), 0.2, 0.8, ptr(out3),
                                          ptr(maps), ptr(scratch), nbytes, stream))
        e[1].record()
        _lib.check(L.lograst_loss_backward(B, C, H, W, ptr(r), strides(r), None, None, ptr(g), strides(g), 0.8, ptr(one),
                                           ptr(maps), ptr(grad), None, stream))
        e[2].record()
        e[2].synchronize()
        if it >= warmup:
            fwd.append(e[0].elapsed_time(e[1]) * 1e3)
            bwd.append(e[1].elapsed_time(e[2]) * 1e3)
    f, b = statistics.median(fwd), statistics.median(bwd)
    return {"fwd_kernel_us": f, "bwd_kernel_us": b, "both_kernel_us": f + b}


def stream_copy_rate(mib=1024, reps=4):
    """Best GB/s (read + write) of lograst_stream_copy over its forms and a few grid sizes, as bench.py measures it."""
    L = _lib.lib()
    nbytes = mib << 20
    a = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    pa, pb = ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr())
    best = float("inf")
    for form in range(5):
        for blocks in ((0,) if form in (1, 4) else (2048, 4096, 8192)):
            arg = (form << 20) | blocks
            _lib.check(L.lograst_stream_copy(pb, pa, nbytes, arg, stream))
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(L.lograst_stream_copy(pb, pa, nbytes, arg, stream))
                e1.record()
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1))
    return 2 * nbytes / (best * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loss needs the MI355X"
    copy_gbs = stream_copy_rate()
    print(f"stream copy {copy_gbs:.0f} GB/s", file=sys.stderr, flush=True)
    window = window_taps().to(dev)
    window = (window[:, None] * window[None, :]).expand(3, 1, 11, 11).contiguous()
    baseline = torch_loss(window)
    result = {"workload": "L1 + SSIM training loss, B=1 C=3 fp32, forward + backward", "reps": a.reps, "warmup": a.warmup,
              "measured_stream_copy_GBs": copy_gbs, "sizes": {}}
    for size in a.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        pair_bytes = 2 * 3 * H * W * 4
        n_cold = max(2, -(-2 * (256 << 20) // pair_bytes) + 1)
        pairs = make_pairs(n_cold, H, W, seed=H)
        alg_bytes = 11 * 4 * 3 * H * W
        entry = {"algorithmic_bytes": alg_bytes, "cold_pairs": n_cold, "cold_pairs_MiB": n_cold * pair_bytes / 2 ** 20}
        for mode, ps in (("warm", pairs[:1]), ("cold", pairs)):
            reps = max(a.reps, len(ps)) if mode == "cold" else a.reps
            t = time_calls(l1_ssim_loss, ps, a.warmup, reps)
            t.update(time_entry_points(ps, a.warmup, reps))
            t["achieved_GBs"] = alg_bytes / (t["both_kernel_us"] * 1e-6) / 1e9
            t["frac_of_measured_stream_copy"] = t["achieved_GBs"] / copy_gbs
            entry["fused_" + mode] = t
            print(size, "fused", mode, json.dumps(t), file=sys.stderr, flush=True)
        if not a.no_baseline:
            for mode, ps in (("warm", pairs[:1]), ("cold", pairs)):
                t = time_calls(baseline, ps, a.warmup, max(a.reps, len(ps)) if mode == "cold" else a.reps)
                entry["torch_" + mode] = t
                entry["speedup_call_" + mode] = t["both_call_us"] / entry["fused_" + mode]["both_call_us"]
                print(size, "torch", mode, json.dumps(t), file=sys.stderr, flush=True)
        result["sizes"][size] = entry
        del pairs
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
