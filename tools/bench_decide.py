"""Stage benchmark of the densification decisions on the device (log_amd.decide: flags, top-k cut and logged statistics
of LoG.update_depth_stage / update_init_stage) at the sizes a user runs, two ways on the same inputs:

1. ``device``: log_amd.decide.decide_depth / decide_init -- the kernels of csrc/decide.hip and ONE read-back of the record;
2. ``torch_device``: the reference's own op sequence (LoG/model/level_of_gaussian.py:401-428, :456-499), written here with
   torch ops ON THE DEVICE, its read-backs included: every ``.sum()`` of a log line, the four ``.item()`` of every
   ``str_min_mean_max`` line, the ``topk``.  The lines are formatted, not printed.

    python tools/bench_decide.py [--sizes 10000000,30000000] [--reps 5]      -> one JSON line per size and case

Cases: the depth stage with a cap that does not bind (``depth_nocut``), with the cap of the example configuration binding
(``depth_cut``), the init stage (``init``).  The tree is five levels deep, a quarter of the rows inner nodes; the counters are
drawn as tests/decide_ref.py draws them.  ``wall_ms``: host clock around the call with a synchronize on both sides, the two
ways alternating after one warm-up round each.  ``kernel_ms``: HIP events around the launches of lograst_decide_depth /
_init alone.  ``GBps``: the bytes the passes must move (43 B read + 2 B written per row for the depth stage; with a cut 5
more flag bytes per row and 20 B per candidate; 32 + 2 B per row for the init stage) over kernel_ms, and ``share_of_copy``
that rate over lograst_stream_copy's in the same run.  Both ways must give the same flags (``flag_rows_that_differ``)."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from log_amd import _lib, decide  # noqa: E402
from bench_densify import stream_copy_rate, wall_ms  # noqa: E402

dev = torch.device("cuda:0")
CFG = types.SimpleNamespace(min_steps_split=100, split_grad_thres=0.0002, radius2d_thres=6, remove_weights_thres=0.005,
                            max_split_points=100000, scaling_decay=0.9, init_radius_min=4, init_radius_split=16,
                            init_weight_min=0.1, min_steps=50)
CURRENT_DEPTH = 20


def make_inputs(n, seed, wide):
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda: torch.rand(n, device=dev, generator=g)
    area = (torch.randint(0, 40, (n,), device=dev, generator=g) * (u() < 0.9)).int()
    gmean = u() * (0.003 if wide else 0.0006)
    c = types.SimpleNamespace(
        create_steps=torch.randint(0, 400, (n,), device=dev, generator=g).int(), area_sum=area,
        grad_sum=gmean * area.clamp(min=1), weights_max=torch.where(u() < 0.1, u() * 0.005, u() * 0.9 + 0.005),
        radii_max_max=(torch.randint(0, 1600, (n,), device=dev, generator=g) if wide else
                       (torch.empty(n, device=dev).exponential_(0.04, generator=g) + 1).clamp(max=400)).int(),
        visible_count=torch.randint(0, 6, (n,), device=dev, generator=g).short(), radius3d_min=u() * 0.01 + 1e-4)
    t = types.SimpleNamespace(depth=torch.randint(0, 5, (n,), device=dev, generator=g).to(torch.int8),
                              node_index=torch.where(u() < 0.25, torch.arange(n, device=dev), -1).int())
    opacity = torch.randn((n, 1), device=dev, generator=g)
    scaling = torch.randn((n, 3), device=dev, generator=g) * 0.5 - 4.0
    return opacity, scaling, t, c


def line(name, data):
    """Counter.str_min_mean_max (LoG/model/counter.py:24-25)."""
    return f'{name:10s} {data.shape[0]:8d} [{data.min().item():.5f}~{data.float().mean().item():.5f}+{data.float().std().item():.5f}~{data.max().item():.5f}]'


def torch_depth(opacity_raw, scaling_raw, t, c, cfg):
    """level_of_gaussian.py:456-499 up to the flags handed to tree.split_and_remove."""
    opacity = torch.sigmoid(opacity_raw[:, 0])
    radius = torch.exp(scaling_raw)
    radius_max = radius.max(dim=-1).values
    radius_min = radius.min(dim=-1).values
    ratio = radius_max / (radius.sum(dim=-1) - radius_max - radius_min)
    flag_is_parent = (t.node_index == -1) & (t.depth < CURRENT_DEPTH)
    flag_depth_parent = flag_is_parent & (c.create_steps > cfg.min_steps_split)
    depth_minus1_sum = (t.depth < CURRENT_DEPTH).sum()
    flag_depth_child = (t.node_index == -1) & (t.depth > 0)
    grad = c.grad_sum / torch.clamp(c.area_sum, min=1)
    radii = c.radii_max_max.float()
    text = [line("opacity", opacity[flag_is_parent]), line("ratio", ratio[flag_is_parent]), line("grad", grad[flag_is_parent]),
            line("radii", radii[flag_is_parent])]
    flag_split_grad = grad > cfg.split_grad_thres
    flag_split_radii = c.radii_max_max > cfg.radius2d_thres
    text.append(f'split by grad: {flag_split_grad.sum():8d} split by radii: {flag_split_radii.sum():8d}')
    flag_split = flag_split_grad & flag_split_radii & flag_depth_parent
    if flag_depth_child.sum() == 0:
        flag_remove = torch.zeros_like(flag_split)
    else:
        flag_remove = flag_depth_child & (c.weights_max < cfg.remove_weights_thres) & (c.visible_count > 1)
    flag_split = flag_split & (~flag_remove)
    num_max_split = min(int(depth_minus1_sum * 0.05), cfg.max_split_points)
    if flag_split.sum() > num_max_split:
        thres = torch.topk(radii[flag_split], num_max_split, largest=True).values[-1]
        text.append(f'select top {num_max_split} points to split. New radii thres = {thres:.1f}')
        flag_split = flag_split & (radii >= thres)
    return flag_split, flag_remove, text


def torch_init(opacity_raw, c, rand, cfg, scale=1):
    """level_of_gaussian.py:401-428 ('split_by_2d') up to the flags handed to splitter.split_and_remove."""
    flag_remove_weight = c.weights_max < cfg.init_weight_min
    flag_nonmax = c.weights_max < torch.sigmoid(opacity_raw[:, 0]) * 0.1
    flag_remove_small = c.radii_max_max < (cfg.init_radius_min * scale) ** 2
    text = [f'{flag_remove_weight.sum():10d}', f'{flag_nonmax.sum():10d}', f'{flag_remove_small.sum():10d}']
    flag_remove = (flag_remove_small & (rand > 0.5)) | flag_remove_weight | flag_nonmax
    radii_max = c.radii_max_max.float()
    flag_activation = (c.create_steps > cfg.min_steps) & (radii_max > 0)
    text.append(line("radii_max_act", radii_max[flag_activation]))
    grad = c.grad_sum / torch.clamp(c.area_sum, min=1)
    text.append(line("grad", grad))
    radii_mean, radii_std = radii_max[flag_activation].mean(), radii_max[flag_activation].std()
    flag_split_grad = (grad > 10 * cfg.split_grad_thres) & (radii_max > cfg.init_radius_min * scale * 8)
    flag_split_radii = radii_max > (cfg.init_radius_split * scale) ** 2
    text += [f'{flag_split_grad.sum():8d}', f'{flag_split_radii.sum():8d}']
    flag_split = flag_activation & (flag_split_radii | flag_split_grad) & (~flag_remove)
    text.append(line("radii_split", radii_max[flag_split]))
    del radii_mean, radii_std
    return flag_split, flag_remove, text


def device_depth(opacity, scaling, t, c, cfg):
    return decide.decide_depth(opacity, scaling, t.node_index, t.depth, c, CURRENT_DEPTH, 128, cfg.min_steps_split,
                               cfg.split_grad_thres, cfg.radius2d_thres, cfg.remove_weights_thres, cfg.max_split_points)


def device_init(opacity, c, rand, cfg):
    return decide.decide_init(opacity, c, 4, cfg.init_weight_min, cfg.init_radius_min, cfg.init_radius_split,
                              cfg.split_grad_thres, cfg.min_steps, 1, rand)


def kernel_ms(fn, reps):
    """HIP events around the launches alone: the read-back is swapped for a no-op while fn runs."""
    L = _lib.lib()
    real = L.lograst_decide_read
    out = []
    try:
        L.lograst_decide_read = lambda *a: 0
        for _ in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
    finally:
        L.lograst_decide_read = real
    return statistics.median(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000000,30000000")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_decide needs the MI355X"
    copy_rate = stream_copy_rate(mib=512, reps=3)
    for n in (int(v) for v in a.sizes.split(",")):
        for case in ("depth_nocut", "depth_cut", "init"):
            cfg = types.SimpleNamespace(**vars(CFG))
            opacity, scaling, t, c = make_inputs(n, 3, wide=case == "init")
            if case == "depth_nocut":
                cfg.split_grad_thres = 0.000597          # about 0.1 % of the rows are candidates: below 5 % and the cap
            if case == "init":
                rand = torch.rand(n, device=dev)
                ways = {"device": lambda: device_init(opacity, c, rand, cfg), "torch_device": lambda: torch_init(opacity, c, rand, cfg)}
            else:
                ways = {"device": lambda: device_depth(opacity, scaling, t, c, cfg),
                        "torch_device": lambda: torch_depth(opacity, scaling, t, c, cfg)}
            got = {k: fn() for k, fn in ways.items()}                        # warm-up, and the results to compare
            # the init stage compares weights_max with sigmoid(opacity) * 0.1: a row within an ulp of it may fall either way
            differ = [int((got["device"][k] != got["torch_device"][k]).sum()) for k in (0, 1)]
            assert differ == [0, 0] or (case == "init" and max(differ) <= n // 100000), (case, differ)
            rec = got["device"][2]
            times = {k: [] for k in ways}
            for _ in range(a.reps):
                for k, fn in ways.items():
                    times[k].append(wall_ms(fn))
            kms = kernel_ms(ways["device"], a.reps)
            num_split = int(got["device"][0].sum())
            if case == "init":
                nbytes, cut = 34 * n, False
            else:
                cut = rec.need_cut
                assert cut == (case == "depth_cut"), (case, rec.counts, rec.num_max_split)
                nbytes = 45 * n + (5 * n + 20 * rec.counts[decide.C["candidates"]] if cut else 0)
            s = lambda v: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
            out = {"workload": f"{case}, {n} points", "reps": a.reps, "cut": bool(cut), "rows_split": num_split,
                   "rows_removed": int(got["device"][1].sum()), "flag_rows_that_differ": differ, "device": s(times["device"]),
                   "torch_device": s(times["torch_device"]), "kernel_ms": kms, "bytes_GB": nbytes / 1e9,
                   "GBps": nbytes / (kms * 1e-3) / 1e9, "stream_copy_GBps": copy_rate}
            out["share_of_copy"] = out["GBps"] / copy_rate
            out["ratio_torch_over_device"] = out["torch_device"]["median_ms"] / out["device"]["median_ms"]
            print(json.dumps(out), flush=True)
            del opacity, scaling, t, c, got
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
