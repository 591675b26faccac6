"""Randomised sweep of the step kernels around the rasterizer -- get_all forward + backward (log_amd.get_all), the native SH
forward / backward, sparse Adam and the fused activation-backward + Adam -- against the float64 restatement tests/step_ref.py:

    python tools/fuzz_step_ops.py --cases 400 --seed 1 [--backend hip|oracle] [--only SEED] [--out build/fuzz_step_ops.jsonl]

Each case draws an operation, a row count (log-uniform 1..300,000, a forced share at the wave / workgroup / 64k seams), the
shapes (K = 0..15 with every admissible active degree, M = (deg+1)^2..16, node rows or none, training / fix_parent both ways),
the contents (index as a permutation slice / sorted / reversed, gradient magnitudes 1e-6..1, prior moments or none, the bias
correction of several step numbers, a random subset of keys not optimised, nothing / half / everything visible) and plants
degenerate rows in at most 2 % of the rows: |q| = 0 and 1e-13..1e-11, opacity +-30 and +-100, scaling -20 and +10, xyz 1e-3
and 1e3 from the camera and exactly on it, and -- where the kernels document it -- index rows outside the model.

Criteria, over ALL rows:
  * raw copies, rows that must not move: bit-identical;
  * every other output element:  |got - ref64| <= F * (|ref32 - ref64| + 2^-24 * S + 2^-126),  ref32 = the restatement in
    torch float32, S = its condition scale (every summed term by its absolute value), 2^-126 = the smallest normal fp32
    (below it a result is rounded absolutely, or flushed), F = 8 as tests/test_gpu_loss.py argues for two fp32 evaluations
    against float64;
  * where ref64 is not finite, neither is the result, in the same places;
  * the native SH clamp mask equals the sign of the float64 colour wherever that colour is further from 0 than its bound.
--backend oracle runs the same cases on the CPU with tests/oracle_backend.OracleBackend in place of the kernels (the fused
step composed from its two halves): a correct fp32 implementation has to stay inside the bound.  A failing case is printed
with its seed (`--only SEED` replays it) and the run exits 1.  Test infrastructure, not product code."""
import argparse
import json
import math
import os
import sys
import time
import traceback
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F = 8.0
EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126
OPS = ("get_all", "native_sh", "sparse_adam", "fused_step")
SEAMS = (1, 63, 64, 65, 255, 256, 257, 65535, 65536, 65537)
PLANTS = ("q_zero", "q_tiny", "opacity_30", "opacity_100", "scaling_-20", "scaling_10", "xyz_near", "xyz_far", "xyz_at_camera")
WIDTHS = {"xyz": 3, "scaling": 3, "opacity": 1, "rotation": 4, "colors": 3}
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
LR = {"xyz": 1.6e-4, "scaling": 5e-3, "opacity": 0.05, "rotation": 1e-3, "colors": 2.5e-3, "shs": 1.25e-4}


def draw_case(seed):
    """-> the description of case `seed` (plain values; build_case() makes the tensors from it)."""
    rng = np.random.default_rng(seed)
    op = OPS[seed % 4]
    n = int(rng.choice(SEAMS)) if rng.random() < 0.3 else int(np.exp(rng.uniform(0.0, np.log(300000))))
    K = 15 if rng.random() < 0.3 else int(rng.integers(0, 16))      # (15 = LoG's max_sh_degree 3: what training runs with)
    degree = int(rng.choice([d for d in range(4) if d == 0 or (d + 1) ** 2 - 1 <= K]))
    sh_degree = int(rng.integers(0, 4))
    d = dict(seed=seed, op=op, n=n, K=K, degree=degree,
             extra_rows=int(rng.integers(0, max(2, n // 2))), index_mode=str(rng.choice(["permutation", "sorted", "reversed"])),
             n_node=0 if rng.random() < 0.4 else int(rng.integers(1, max(2, n // 4 + 1))),
             training=bool(rng.random() < 0.8), fix_parent=bool(rng.random() < 0.5),
             grad_mag=float(10.0 ** rng.uniform(-6, 0)), moments=str(rng.choice(["zero", "random", "random"])),
             steps=int(rng.choice([1, 2, 5, 100, 30000])), amsgrad=bool(rng.random() < 0.5),
             keys_off=[k for k in list(WIDTHS) + ["shs"] if rng.random() < 0.25],
             visible=float(rng.choice([0.0, 0.5, 0.5, 1.0])),
             plants=[str(p) for p in rng.choice(PLANTS, int(rng.integers(0, 4)), replace=False)] if n >= 50 else [],
             bad_index=bool(n >= 50 and rng.random() < 0.4),
             sh_degree=sh_degree, M=int(rng.integers((sh_degree + 1) ** 2, 17)), accumulate=bool(rng.random() < 0.5),
             sh_scale=float(rng.choice([0.2, 1.0, 2.0])))
    return d


def _plant(d, rng, bufs, rows, campos):
    """Degenerate values into the model rows `rows` (the gathered ones), at most 2 % of them in all."""
    import torch
    planted = {}
    if not d["plants"]:
        return planted
    budget = max(1, len(rows) // 50) // len(d["plants"])
    for what in d["plants"]:
        if budget < 1:
            break
        r = torch.as_tensor(rng.choice(rows, budget, replace=False))
        planted[what] = int(r.numel())
        unit = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((budget, 3)).astype(np.float32)), dim=-1)
        if what == "q_zero":
            bufs["rotation"][r] = 0.0
        elif what == "q_tiny":
            q = torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((budget, 4)).astype(np.float32)), dim=-1)
            bufs["rotation"][r] = q * torch.from_numpy(10.0 ** rng.uniform(-13, -11, (budget, 1))).float()
        elif what in ("opacity_30", "opacity_100"):
            sign = torch.from_numpy(rng.choice([-1.0, 1.0], (budget, 1))).float()
            bufs["opacity"][r] = sign * float(what.split("_")[1])
        elif what.startswith("scaling_"):
            bufs["scaling"][r] = float(what.split("_")[1])
        elif what == "xyz_near":
            bufs["xyz"][r] = campos + 1e-3 * unit
        elif what == "xyz_far":
            bufs["xyz"][r] = campos + 1e3 * unit
        elif what == "xyz_at_camera":
            bufs["xyz"][r] = campos
    return planted


def build_case(d):
    """-> types.SimpleNamespace of CPU tensors for case d."""
    import torch
    rng = np.random.default_rng(d["seed"] + 7)
    g = torch.Generator().manual_seed(d["seed"])
    rnd = lambda *s: torch.randn(*s, generator=g)
    n, K = d["n"], d["K"]
    c = types.SimpleNamespace(d=d)
    c.campos = torch.tensor([0.3, -2.0, 1.0]) * float(rng.choice([1.0, 1.0, 50.0]))
    if d["op"] == "native_sh":
        M = d["M"]
        c.bufs = {"xyz": rnd(n, 3) * 2, "rotation": rnd(n, 4), "opacity": rnd(n, 1), "scaling": rnd(n, 3)}
        c.planted = _plant(dict(d, plants=[p for p in d["plants"] if p.startswith("xyz")]), rng, c.bufs, np.arange(n), c.campos)
        c.means, c.shs = c.bufs["xyz"], rnd(n, M, 3) * d["sh_scale"]
        c.g_colors = rnd(n, 3) * d["grad_mag"]
        c.base_shs, c.base_means = rnd(n, M, 3) * d["grad_mag"], rnd(n, 3) * d["grad_mag"]
        return c
    P = n + d["extra_rows"]
    c.P = P
    c.bufs = {"xyz": rnd(P, 3) * 2, "scaling": rnd(P, 3) * 0.5 - 3.0, "opacity": rnd(P, 1) * 2, "rotation": rnd(P, 4),
              "colors": rnd(P, 3)}
    if K:
        c.bufs["shs"] = rnd(P, K, 3) * 0.3
    index = torch.randperm(P, generator=g)[:n]
    if d["index_mode"] != "permutation":
        index = index.sort(descending=d["index_mode"] == "reversed").values
    c.planted = _plant(d, rng, c.bufs, index.numpy(), c.campos)
    c.bad = torch.zeros(n, dtype=torch.bool)
    if d["bad_index"]:
        c.bad[torch.as_tensor(rng.choice(n, max(1, n // 100), replace=False))] = True
        index = torch.where(c.bad, torch.from_numpy(rng.choice([-1, -P - 5, P, P + 7, 2 ** 40], n)), index)
    c.index = index
    c.n_param = n if d["op"] == "sparse_adam" else max(1, n - min(d["n_node"], n - 1))
    c.ups = {k: rnd(n, w) * d["grad_mag"] for k, w in WIDTHS.items()}
    shapes = dict({k: (w,) for k, w in WIDTHS.items()}, **({"shs": (K, 3)} if K else {}))
    c.keys = [k for k in shapes if k not in d["keys_off"]] or ["xyz"]
    m = c.n_param
    c.grads = {k: rnd(m, *s) * d["grad_mag"] for k, s in shapes.items()}
    zero = d["moments"] == "zero"
    c.m1 = {k: torch.zeros(P, *s) if zero else rnd(P, *s) * d["grad_mag"] for k, s in shapes.items()}
    c.m2 = {k: torch.zeros(P, *s) if zero else (rnd(P, *s) * d["grad_mag"]) ** 2 for k, s in shapes.items()}
    c.mx = {k: torch.zeros(P, *s) if zero else (rnd(P, *s) * d["grad_mag"]) ** 2 for k, s in shapes.items()} if d["amsgrad"] else None
    c.visible = torch.rand(m, generator=g) < d["visible"] if 0.0 < d["visible"] < 1.0 else torch.full((m,), d["visible"] == 1.0)
    c.bc1, c.bc2 = 1 - BETA1 ** d["steps"], 1 - BETA2 ** d["steps"]
    return c


# ---- judging --------------------------------------------------------------------------------------------------------
def _judge(res, name, got, r64, r32, S):
    import torch
    got, r64, r32, S = (t.detach().cpu().double() for t in (got, r64, r32, S))
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    if got.numel() == 0:
        return
    fin = torch.isfinite(r64)
    if bool(torch.isfinite(got[~fin]).any()):
        res["fail"].append("%s: finite where the float64 value is not" % name)
    bound = F * ((r32 - r64).abs() + EPS32 * S + TINY32)
    judged = fin & torch.isfinite(bound)
    if bool((fin & ~judged).any()):                 # (the float32 restatement overflowed where float64 did not: nothing to judge by)
        res["fail"].append("%s: %d elements with a finite float64 value and no finite bound" % (name, int((fin & ~judged).sum())))
    err = (got - r64).abs()
    bad = judged & ~(err <= bound)
    ratio = torch.where(judged, err / bound, torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    res["worst"][name] = max(res["worst"].get(name, 0.0), float(ratio.max()))
    res["elements"] = res.get("elements", 0) + int(judged.sum())
    if bool(bad.any()):
        i = int(torch.argmax(ratio.reshape(-1)))
        res["fail"].append("%s: %d of %d elements outside the bound, worst err/bound %.3g (got %.9g, ref64 %.9g, ref32 %.9g, S %.3g)"
                           % (name, int(bad.sum()), got.numel(), float(ratio.reshape(-1)[i]), float(got.reshape(-1)[i]),
                              float(r64.reshape(-1)[i]), float(r32.reshape(-1)[i]), float(S.reshape(-1)[i])))


def _same(res, name, got, want):
    import torch
    got, want = got.detach().cpu(), want.detach().cpu()
    same = got.shape == want.shape and bool(((got == want) | (torch.isnan(got) & torch.isnan(want))).all()) \
        if got.is_floating_point() else torch.equal(got, want)
    if not same:
        res["fail"].append("%s: not bit-identical" % name)


# ---- the four operations ---------------------------------------------------------------------------------------------
def _run_get_all(c, dev, hip, res):
    import torch
    import step_ref
    from log_amd import get_all as GA
    d = c.d
    index = c.index if hip else torch.where(c.bad, torch.zeros_like(c.index), c.index)   # (the C oracle reads what it is told to)
    n_leaf = c.n_param
    gaussian = types.SimpleNamespace(keys=list(c.bufs), active_sh_degree=d["degree"])
    for k, v in c.bufs.items():
        setattr(gaussian, k, v.to(dev))
    gaussian.items = lambda: ((k, getattr(gaussian, k)) for k in gaussian.keys)
    flags = {"index": index[:n_leaf].to(dev)}
    if n_leaf < d["n"]:
        flags["index_node"] = index[n_leaf:].to(dev)
    gaussian.visibility_flag = flags
    model = types.SimpleNamespace(gaussian=gaussian, fix_parent=d["fix_parent"], training=d["training"])
    ret = GA.get_all(model, {"camera_center": c.campos.to(dev)}, None)
    n_param = n_leaf if d["fix_parent"] else d["n"]
    params = flags["params"]
    ups = c.ups if d["training"] else None
    r64 = step_ref.get_all(c.bufs, c.index, n_param, d["degree"], c.campos, ups)
    r32 = step_ref.get_all(c.bufs, c.index, n_param, d["degree"], c.campos, ups, dtype=torch.float32)
    for k in c.bufs:
        _same(res, "raw_" + k, params[k], r64["raw"][k][:n_param])
    _same(res, "act_xyz", ret["xyz"], r64["raw"]["xyz"])
    for k in ("scaling", "opacity", "rotation", "colors"):
        _judge(res, "act_" + k, ret[k], r64["act"][k], r32["act"][k], r64["S_act"][k])
    if not d["training"]:
        return
    sum((ret[k] * c.ups[k].to(dev)).sum() for k in ret).backward()
    for k, p in params.items():
        if k == "shs" and d["degree"] == 0:
            if p.grad is not None:
                res["fail"].append("grad_shs: a gradient for unused coefficients")
            continue
        if k == "xyz":
            _same(res, "grad_xyz", p.grad, c.ups["xyz"][:n_param])
        else:
            _judge(res, "grad_" + k, p.grad, r64["grads"][k], r32["grads"][k], r64["S_grads"][k])


def _run_native_sh(c, dev, hip, res):
    import torch
    import step_ref
    from log_amd import rasterizer as R
    d = c.d
    deg = d["sh_degree"]
    means, shs, cp = c.means.to(dev), c.shs.to(dev).contiguous(), c.campos.to(dev)
    colors, clamped = R._backend.sh_forward(means, cp, shs, deg)
    f64 = step_ref.native_sh(c.means, c.campos, c.shs, deg)
    f32 = step_ref.native_sh(c.means, c.campos, c.shs, deg, dtype=torch.float32)
    _judge(res, "sh_colors", colors, f64["colors"], f32["colors"], f64["S_colors"])
    pre = f64["pre"]
    sure = torch.isfinite(pre) & (pre.abs() > F * ((f32["pre"].double() - pre).abs() + EPS32 * f64["S_colors"] + TINY32))
    cl = clamped.cpu().bool()
    if bool((cl != (pre < 0))[sure].any()):
        res["fail"].append("sh_clamped: differs from the sign of the float64 colour outside its bound")
    res["clamped"] = int(cl.sum())
    g_means = c.base_means.clone().to(dev)
    if d["accumulate"] and hip:
        into = c.base_shs.clone().to(dev)
        assert R._backend.sh_backward(means, cp, shs, deg, clamped, c.g_colors.to(dev), g_means, into=into) is None
        g_shs = into
    else:
        g_shs = R._backend.sh_backward(means, cp, shs, deg, clamped, c.g_colors.to(dev), g_means)
        if d["accumulate"]:
            g_shs = c.base_shs.to(dev) + g_shs          # (the test double has no running-sum form: composed here)
    b64 = step_ref.native_sh(c.means, c.campos, c.shs, deg, c.g_colors, clamped=cl)
    b32 = step_ref.native_sh(c.means, c.campos, c.shs, deg, c.g_colors, clamped=cl, dtype=torch.float32)
    add = c.base_shs.double() if d["accumulate"] else 0.0
    _judge(res, "sh_g_shs", g_shs, b64["g_shs"] + add, b32["g_shs"].double() + add,
           b64["S_g_shs"] + (c.base_shs.abs().double() if d["accumulate"] else 0.0))
    _judge(res, "sh_g_means3D", g_means, b64["g_means3D"] + c.base_means.double(), b32["g_means3D"].double() + c.base_means.double(),
           b64["S_g_means3D"] + c.base_means.abs().double())


def _adam_reference(c, res, model, m1, m2, mx, sel, grads64, grads32, S_grads, keys):
    """Judge the model / moments after one step on the rows `sel` (positions among the parameter rows) -> nothing."""
    import torch
    import step_ref
    rows = c.index[:c.n_param][sel]
    untouched = torch.ones(c.P, dtype=torch.bool)
    untouched[rows] = False
    for k in c.bufs:
        if k not in keys:
            _same(res, "model_%s (not optimised)" % k, model[k], c.bufs[k])
            _same(res, "exp_avg_%s (not optimised)" % k, m1[k], c.m1[k])
            continue
        _same(res, "model_%s untouched rows" % k, model[k].cpu()[untouched], c.bufs[k][untouched])
        _same(res, "exp_avg_%s untouched rows" % k, m1[k].cpu()[untouched], c.m1[k][untouched])
        _same(res, "exp_avg_sq_%s untouched rows" % k, m2[k].cpu()[untouched], c.m2[k][untouched])
        if mx is not None:
            _same(res, "max_exp_avg_sq_%s untouched rows" % k, mx[k].cpu()[untouched], c.mx[k][untouched])
        args = (c.bufs[k][rows], None, c.m1[k][rows], c.m2[k][rows], c.mx[k][rows] if mx is not None else None, LR[k] / c.bc1,
                BETA1, BETA2, math.sqrt(c.bc2), EPS)
        a64 = step_ref.adam(args[0], grads64[k][sel], *args[2:], S_grad=None if S_grads is None else S_grads[k][sel])
        a32 = step_ref.adam(args[0], grads32[k][sel], *args[2:], dtype=torch.float32)
        got = {"param": model[k], "exp_avg": m1[k], "exp_avg_sq": m2[k]}
        if mx is not None:
            got["max_exp_avg_sq"] = mx[k]
        for name, t in got.items():
            _judge(res, "adam_%s_%s" % (name, k), t.cpu()[rows], a64[name], a32[name], a64["S_" + name])


def _state(c, dev):
    cl = lambda dct: {k: v.clone().to(dev) for k, v in dct.items()}
    return cl(c.bufs), cl(c.m1), cl(c.m2), cl(c.mx) if c.mx is not None else None


def _run_sparse_adam(c, dev, hip, res):
    import torch
    from log_amd import rasterizer as R
    model, m1, m2, mx = _state(c, dev)
    m = c.n_param
    ok_row = ~c.bad[:m]
    flag = c.visible if hip else (c.visible & ok_row)               # (the C oracle has no guard for rows outside the model)
    index = c.index[:m] if hip else torch.where(ok_row, c.index[:m], torch.zeros_like(c.index[:m]))
    safe = torch.where(ok_row, c.index[:m], torch.zeros_like(c.index[:m]))
    entries = [(model[k], c.bufs[k][safe].to(dev), c.grads[k].to(dev), m1[k], m2[k], mx[k] if mx is not None else None,
                LR[k] / c.bc1) for k in c.keys]
    R._backend.sparse_adam(index.to(dev), flag.to(dev), entries, BETA1, BETA2, math.sqrt(c.bc2), EPS)
    sel = c.visible & ok_row
    _adam_reference(c, res, model, m1, m2, mx, sel, c.grads, c.grads, None, c.keys)
    res["visible_rows"] = int(sel.sum())


def _run_fused_step(c, dev, hip, res):
    import torch
    import step_ref
    from log_amd import rasterizer as R
    d = c.d
    model, m1, m2, mx = _state(c, dev)
    n = c.n_param
    ok_row = ~c.bad[:n]
    safe_all = torch.where(c.bad, torch.zeros_like(c.index), c.index)
    deg = d["degree"]
    cp = c.campos.to(dev) if deg > 0 else None
    raw, _ = R._backend.gather_activate((c.index if hip else safe_all).to(dev), {k: v.to(dev) for k, v in c.bufs.items()}, deg, cp)
    keys = [k for k in c.keys if k != "shs" or deg > 0]
    radii = (c.visible.to(torch.int32) * 7)
    ups = {k: v.to(dev) for k, v in c.ups.items()}
    if hip:
        entries = {k: (model[k], m1[k], m2[k], mx[k] if mx is not None else None, LR[k] / c.bc1) for k in keys}
        R._backend.activate_backward_adam(raw, n, deg, cp, ups["xyz"], ups["scaling"], ups["opacity"], ups["rotation"],
                                          ups["colors"], c.index[:n].to(dev), radii.to(dev), entries, BETA1, BETA2,
                                          math.sqrt(c.bc2), EPS)
    else:                                                           # the two halves, one after the other
        g = R._backend.activate_backward(raw, n, deg, cp, ups["scaling"], ups["opacity"], ups["rotation"], ups["colors"])
        g["xyz"] = ups["xyz"][:n]
        entries = [(model[k], raw[k][:n], g[k], m1[k], m2[k], mx[k] if mx is not None else None, LR[k] / c.bc1) for k in keys]
        R._backend.sparse_adam(safe_all[:n], (radii[:n] > 0) & ok_row, entries, BETA1, BETA2, math.sqrt(c.bc2), EPS)
    r64 = step_ref.get_all(c.bufs, c.index, n, deg, c.campos, c.ups)
    r32 = step_ref.get_all(c.bufs, c.index, n, deg, c.campos, c.ups, dtype=torch.float32)
    sel = c.visible & ok_row
    _adam_reference(c, res, model, m1, m2, mx, sel, r64["grads"], r32["grads"], r64["S_grads"], keys)
    res["visible_rows"] = int(sel.sum())


RUN = {"get_all": _run_get_all, "native_sh": _run_native_sh, "sparse_adam": _run_sparse_adam, "fused_step": _run_fused_step}


def run_case(backend, seed):
    """backend: "hip" (the kernels, on cuda:0) or "oracle" (tests/oracle_backend.OracleBackend, on the CPU).  -> the case's
    description with `worst` = the largest err / bound per output; raises AssertionError naming what failed."""
    import torch
    from log_amd import rasterizer as R
    import oracle_backend
    d = draw_case(seed)
    c = build_case(d)
    res = dict(d, backend=backend, planted=c.planted, worst={}, fail=[])
    hip = backend == "hip"
    old = None if hip else oracle_backend.install(oracle_backend.OracleBackend())
    try:
        RUN[d["op"]](c, "cuda:0" if hip else "cpu", hip, res)
        if hip:
            torch.cuda.synchronize()
    finally:
        if not hip:
            oracle_backend.install(None if isinstance(old, R.HipBackend) else old)
    assert not res["fail"], "case %d (%s, n = %d): %s" % (seed, d["op"], d["n"], "; ".join(res["fail"]))
    return res


def summarize(results):
    """-> {operation: worst err / bound over its outputs and cases}"""
    worst = {}
    for r in results:
        for name, v in r.get("worst", {}).items():
            key = "%s / %s" % (r["op"], name.split("_")[0] if r["op"] in ("sparse_adam", "fused_step") else name)
            worst[key] = max(worst.get(key, 0.0), v)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", type=int, default=None, help="replay one case seed")
    ap.add_argument("--backend", choices=["hip", "oracle"], default="hip")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "fuzz_step_ops.jsonl"))
    args = ap.parse_args()
    from oracle import oracle
    oracle.build()
    seeds = [args.only] if args.only is not None else [args.seed * 100000 + i for i in range(args.cases)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    t0, failed, results = time.time(), [], []
    with open(args.out, "w") as f:
        for s in seeds:
            try:
                r = run_case(args.backend, s)
                r["ok"] = True
            except Exception as e:                            # noqa: BLE001 -- a fuzz harness reports everything
                r = dict(draw_case(s), ok=False, error=repr(e)[:1500], trace=traceback.format_exc()[-1500:])
                failed.append(s)
                print("FAIL", json.dumps(r, default=str)[:2500], flush=True)
            results.append(r)
            f.write(json.dumps(r, default=str) + "\n")
            f.flush()
    for k, v in sorted(summarize(results).items()):
        print("worst err/bound  %-40s %.3f" % (k, v))
    print("fuzz_step_ops (%s): %d cases, %d failed %s in %.0f s" % (args.backend, len(results), len(failed), failed[:20], time.time() - t0))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
