"""Stage benchmark of the depth term (log_amd.depth_loss.depth_patch_loss: lograst_depth_loss_forward / _backward)
against the sequence of torch calls an unmodified LoG process makes for it (LoG/render/renderer.py:268-292 with
LoG/render/loss.py:47-117), written here from the formulas (tests/depth_loss_ref.py: stack_loss): device randint, 64
slices of pred / gt / mask whose bounds are device scalars (each a read-back), three stacks, the loss in fp32, backward.

    python tools/bench_depth_loss.py [--reps 20] [--warmup 3] [--size 1920x1080] [--scene N]      -> one JSON line

The two sides ALTERNATE in one process (fused, torch, fused, torch, ...): --warmup rounds, then --reps rounds; per side
the median and (min - max) of the wall time of forward + backward, from before the positions are drawn until the device
has finished (perf_counter around the call + one synchronize: the torch side synchronises by itself all along, so HIP
events alone would not see what its step pays).  Both sides draw their positions with the same device generator calls.
Also: HIP events around the two C entry points alone (kernel time of forward = patch kernel + sum, and of backward).
Inputs: synthetic maps (a smooth depth in [2, 4] with noise, an accumulation map that crosses 0.5) or, with --scene N, the
depth and accumulation channels this repository's rasterizer renders of a trained-like scene of N Gaussians."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from depth_loss_ref import stack_loss  # noqa: E402
from log_amd import _lib  # noqa: E402
from log_amd.depth_loss import depth_patch_loss  # noqa: E402

dev = torch.device("cuda:0")
PATCH, NUM = 64, 64


def synthetic(H, W, seed):
    g = torch.Generator(device=dev).manual_seed(seed)

    def field(cells):
        coarse = torch.rand(1, 1, cells, cells, device=dev, generator=g)
        return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True)[0, 0]
    pred = 2.1 + 1.8 * field(12) + 0.05 * torch.randn(H, W, device=dev, generator=g)
    return pred.contiguous(), (0.1 + 0.5 * field(9)).contiguous(), (0.15 + 0.8 * field(7)).contiguous()


def rendered(H, W, n):
    """depth and accumulation as LoG's second rasterizer call renders them (colours [view z, world z, 1])."""
    import math
    from log_amd import scenes
    import diff_gaussian_rasterization_wodilate as wo
    cam = scenes.orbit_cameras(2, W=W, H=H, focal=1.2 * W)[0]
    sc = scenes.trained_like_scene(n, seed=0)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    rs = wo.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam["FoVx"] * 0.5), tanfovy=math.tan(cam["FoVy"] * 0.5),
        bg=t([0.0, 0.0, 0.0]), scale_modifier=1.0, viewmatrix=t(cam["world_view_transform"]),
        projmatrix=t(cam["full_proj_transform"]), sh_degree=0, campos=t(cam["camera_center"]), prefiltered=False, debug=False)
    xyz = t(sc["xyz"])
    z = (torch.cat([xyz, torch.ones_like(xyz[:, :1])], dim=1) @ t(cam["world_view_transform"]))[:, 2]
    colours = torch.stack([z, xyz[:, 2], torch.ones_like(z)], dim=-1)
    with torch.no_grad():
        out = wo.GaussianRasterizer(raster_settings=rs)(
            means3D=xyz, means2D=torch.zeros_like(xyz), shs=None, colors_precomp=colours, opacities=t(sc["opacity"]),
            scales=t(sc["scaling"]), rotations=t(sc["rotation"]), cov3D_precomp=None)[0]
    g = torch.Generator(device=dev).manual_seed(1)
    gt = 0.1 + 0.5 * torch.rand(H, W, device=dev, generator=g)
    return out[0].contiguous(), gt, out[2].contiguous()


def draw(H, W):
    rows = torch.randint(0, H - PATCH, (NUM,), device=dev)
    cols = torch.randint(0, W - PATCH, (NUM,), device=dev)
    return rows, cols


def fused_step(pred, gt, acc):
    p = pred.detach().requires_grad_(True)
    rows, cols = draw(*pred.shape)
    loss = depth_patch_loss(p, gt, acc, rows, cols)
    loss.backward()
    return loss, p.grad


def torch_step(pred, gt, acc):
    p = pred.detach().requires_grad_(True)
    mask = acc > 0.5
    rows, cols = draw(*pred.shape)
    preds, gts, masks = [], [], []
    for i in range(NUM):
        preds.append(p[rows[i]:rows[i] + PATCH, cols[i]:cols[i] + PATCH])
        gts.append(gt[rows[i]:rows[i] + PATCH, cols[i]:cols[i] + PATCH])
        masks.append(mask[rows[i]:rows[i] + PATCH, cols[i]:cols[i] + PATCH])
    loss, _ = stack_loss(1. / (torch.stack(preds) + 1e-5), torch.stack(gts), torch.stack(masks).to(torch.float32))
    loss.backward()
    return loss, p.grad


def wall_us(fn, *args):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*args)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def entry_points(pred, gt, acc, warmup, reps):
    L = _lib.lib()
    H, W = pred.shape
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    strides = lambda t: (ctypes.c_int64 * 2)(*t.stride())
    nbytes = L.lograst_depth_loss_record_bytes(NUM)
    records = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(2, dtype=torch.float64, device=dev)
    grad = torch.empty(H, W, device=dev)
    one = torch.ones(1, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    fwd, bwd = [], []
    for it in range(warmup + reps):
        rows, cols = draw(H, W)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _lib.check(L.lograst_depth_loss_forward(H, W, ptr(pred), strides(pred), ptr(gt), strides(gt), ptr(acc), strides(acc), NUM,
                                                ptr(rows), ptr(cols), 0.5, 1e-5, 0.5, ptr(out), ptr(records), nbytes, stream))
        e[1].record()
        _lib.check(L.lograst_depth_loss_backward(H, W, ptr(pred), strides(pred), ptr(gt), strides(gt), ptr(acc), strides(acc), NUM,
                                                 ptr(records), ptr(one), ptr(grad), stream))
        e[2].record()
        e[2].synchronize()
        if it >= warmup:
            fwd.append(e[0].elapsed_time(e[1]) * 1e3)
            bwd.append(e[1].elapsed_time(e[2]) * 1e3)
    return {"fwd_kernel_us": statistics.median(fwd), "bwd_kernel_us": statistics.median(bwd)}


def summary(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--scene", type=int, default=0, help="render the maps from a trained-like scene of this many Gaussians")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_depth_loss needs the MI355X"
    W, H = (int(v) for v in a.size.split("x"))
    pred, gt, acc = rendered(H, W, a.scene) if a.scene else synthetic(H, W, 3)
    torch.manual_seed(7)
    times = {"fused": [], "torch": []}
    for it in range(a.warmup + a.reps):
        for name, fn in (("fused", fused_step), ("torch", torch_step)):
            us = wall_us(fn, pred, gt, acc)
            if it >= a.warmup:
                times[name].append(us)
    # the same positions on both sides once: the two losses next to each other
    state = torch.cuda.get_rng_state(dev)
    lf = float(fused_step(pred, gt, acc)[0].detach())
    torch.cuda.set_rng_state(state, dev)
    lt = float(torch_step(pred, gt, acc)[0].detach())
    f, t = summary(times["fused"]), summary(times["torch"])
    result = {"workload": f"depth patch loss, {NUM} patches of {PATCH}x{PATCH} in {W}x{H}, forward + backward",
              "inputs": f"trained-like scene, {a.scene} Gaussians" if a.scene else "synthetic",
              "valid_fraction": float((acc > 0.5).float().mean()), "reps": a.reps, "warmup": a.warmup,
              "fused": f, "torch": t, "torch_spread_us": t["max_us"] - t["min_us"],
              "median_saved_us": t["median_us"] - f["median_us"],
              "fused_lower_by_more_than_torch_spread": (t["median_us"] - f["median_us"]) > (t["max_us"] - t["min_us"]),
              "loss_fused": lf, "loss_torch_fp32": lt}
    result.update(entry_points(pred, gt, acc, a.warmup, a.reps))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
