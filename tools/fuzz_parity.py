"""Randomised parity sweep of the HIP path against the CPU oracle (run ON a GPU box, from the repo root):

    python tools/fuzz_parity.py --cases 200 --seed 1 [--out gpurun_out/fuzz.jsonl]

Each case draws a scene (size, scale / opacity statistics, degenerate rows, duplicates), a camera (resolution not a multiple
of 16, focal, distance -- including cameras inside the cloud), a flavour (the fork's `wodilate` 5-tuple / the upstream
2-tuple), a path (plain backend call / the training forward that prepares the accumulator rows and hit masks), the
compositing form of the forward and of the reverse walk (package's choice / rows / quadrant) and a few launch-shape knobs,
then checks what tests/test_gpu_parity.py checks on its fixed cases:
  * forward: records, tile lists, image, final_T, n_contrib and the fork's maps BIT FOR BIT the oracle's;
  * reverse walk (dL/dmean2D, dL/dconic, dL/dopacity, dL/dcolour): rel-L2 <= 1e-4 against the oracle;
  * end to end (dL/dmeans3D, dL/dscales, dL/drotations): the float64-anchored criterion of tests/gpu_util.py.
A failing case is printed with its seed (`--only SEED` replays it) and the run exits 1.  The oracle is the checker here,
as in tests/ -- this is test infrastructure, not product code.

`--mode props`: bands and bucket accumulation on the same draws (run_props).  `--mode calls`: the same draws through the other
kinds of rasterizer call -- aux_colors, the second pass over a view's tile lists, camera gradients, native shs=, cov3D_precomp
-- each in a drawn capacity mode against its comparator in exact mode (draw_call / run_call; the relations per kind are listed
above tests/test_gpu_fuzz.py::test_random_calls, the full runs in profiles/fuzz_calls.md)."""
import argparse
import json
import os
import sys
import time
import traceback
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRAD_TOL = 1e-4
MAX_INSTANCES = 6_000_000


def draw_case(seed):
    """-> (description dict, cam, scene dict of numpy arrays, options dict)."""
    from log_amd import scenes
    rng = np.random.default_rng(seed)
    n = int(np.exp(rng.uniform(np.log(1), np.log(400000))))
    shape = rng.choice(["odd", "odd", "odd", "aligned", "tiny", "wide", "hd"])
    if shape == "odd":
        W, H = int(rng.integers(17, 700)), int(rng.integers(17, 500))
    elif shape == "aligned":
        W, H = 16 * int(rng.integers(1, 40)), 16 * int(rng.integers(1, 30))
    elif shape == "tiny":
        W, H = int(rng.integers(1, 17)), int(rng.integers(1, 17))
    elif shape == "wide":
        W, H = int(rng.integers(600, 2000)), int(rng.integers(1, 40))
    else:
        W, H = 1920, 1080
        n = min(n, 60000)
    focal = float(W * np.exp(rng.uniform(np.log(0.4), np.log(3.0))))
    radius = float(rng.choice([0.2, 0.8, 1.5, 2.5, 4.0]))
    nv = int(rng.integers(1, 9))
    cam = scenes.orbit_cameras(nv, W=W, H=H, focal=focal, radius=radius)[int(rng.integers(0, nv))]
    kind = rng.choice(["random", "random", "trained", "fine", "coarse"])
    if kind == "coarse":
        n = min(n, 3000)                            # (every splat covers much of the image: the oracle's time is the limit)
    if kind == "trained":
        sc = scenes.trained_like_scene(n, seed=seed % 1000)
    else:
        smax = {"random": float(np.exp(rng.uniform(np.log(0.003), np.log(0.3)))), "fine": 0.002, "coarse": 0.6}[kind]
        sc = scenes.random_scene(n, seed=seed % 1000, smax=smax)
    sc = {k: np.array(v, np.float32, copy=True) for k, v in sc.items()}
    sc["opacity"] = sc["opacity"].reshape(-1)
    omode = rng.choice(["keep", "opaque", "half", "uniform", "fog", "mixed"])
    if omode == "opaque":
        sc["opacity"][:] = 0.999
    elif omode == "half":
        sc["opacity"][:] = 0.5
    elif omode == "uniform":
        sc["opacity"] = rng.random(n, dtype=np.float32)
    elif omode == "fog":
        sc["opacity"] = (0.004 + 0.05 * rng.random(n, dtype=np.float32)).astype(np.float32)
    elif omode == "mixed":
        sc["opacity"] = np.where(rng.random(n) < 0.5, 0.999, 0.02 * rng.random(n)).astype(np.float32)
    degenerate = []
    if n >= 8 and rng.random() < 0.5:
        k = max(1, n // 50)
        pick = lambda: rng.integers(0, n, k)
        for what in rng.choice(["dup", "zero_scale", "zero_opacity", "needle", "giant", "unnormalised"], 2, replace=False):
            ids = pick()
            if what == "dup":                       # equal depths: the (depth, id) order decides
                src = pick()
                for f in ("xyz", "scaling", "rotation"):
                    sc[f][ids] = sc[f][src]
            elif what == "zero_scale":
                sc["scaling"][ids] = 0.0
            elif what == "zero_opacity":
                sc["opacity"][ids] = 0.0
            elif what == "needle":
                sc["scaling"][ids, 1:] *= 1e-3
            elif what == "giant":
                sc["scaling"][ids[: max(1, k // 8)]] = 3.0
            elif what == "unnormalised":            # the reference does not normalise the quaternion in the kernel
                sc["rotation"][ids] *= rng.uniform(0.3, 3.0, (len(ids), 1)).astype(np.float32)
            degenerate.append(str(what))
    opt = dict(flavour=str(rng.choice(["wodilate", "upstream"])), training=bool(rng.random() < 0.6),
               fwd_form=rng.choice([None, "rows", "quadrant"]), bwd_form=rng.choice([None, "rows", "quadrant"]),
               hit_masks=bool(rng.random() < 0.8), use_filter=bool(rng.random() < 0.9),
               scale_modifier=float(rng.choice([1.0, 1.0, 0.5, 2.3])),
               bg=tuple(float(x) for x in rng.random(3).round(2)),
               knobs={})
    for knob, values in (("LOGRAST_LAZY_SORT", (0, 1)), ("LOGRAST_MID_RANK", (0, 1)), ("LOGRAST_MID_COOP", (0, 1, 16)),
                         ("LOGRAST_FILL_STAGED", (0, 1, 2, 3)), ("LOGRAST_BATCH_SLOTS", (64, 256, 1024)),
                         ("LOGRAST_DEFER_TILES", (4, 16, 100)), ("LOGRAST_PBWD_LIST", (0, 1, 2)),
                         ("LOGRAST_HUGE_CHUNK", (256, 2048)), ("LOGRAST_PROJECT_BLOCKS", (64, 4096))):
        if rng.random() < 0.25:
            opt["knobs"][knob] = int(rng.choice(values))
    if opt["fwd_form"] is not None:
        opt["fwd_form"] = str(opt["fwd_form"])
    if opt["bwd_form"] is not None:
        opt["bwd_form"] = str(opt["bwd_form"])
    desc = dict(seed=int(seed), n=n, W=W, H=H, focal=round(focal, 1), radius=radius, scene=str(kind), opacity=str(omode),
                degenerate=degenerate, **{k: v for k, v in opt.items()})
    return desc, cam, sc, opt


def run_case(oracle, seed):
    import gpu_util as G
    from log_amd import rasterizer as R, tune
    from util import rel_l2
    desc, cam, sc, opt = draw_case(seed)
    fl = {"wodilate": R.WODILATE, "upstream": R.UPSTREAM}[opt["flavour"]]
    prev = {k: tune.get_knob(k) for k in opt["knobs"]}
    for k, v in opt["knobs"].items():
        tune.set_knob(k, v)
    try:
        hf = G.hip_forward(cam, sc, opt["bg"], flavour=fl, use_filter=opt["use_filter"], scale_modifier=opt["scale_modifier"],
                           scratch_floats=16 if opt["training"] else 0, fwd_form=opt["fwd_form"],
                           hit_masks=opt["hit_masks"] if opt["training"] else None)
        if hf["I"] > MAX_INSTANCES:
            return dict(desc, I=int(hf["I"]), skipped="more tile instances than the CPU oracle walks in seconds")
        v, of = G.oracle_forward(oracle, cam, sc, opt["bg"], flavour=fl, use_filter=opt["use_filter"],
                                 scale_modifier=opt["scale_modifier"])
        st = G.compare_forward(hf, of)
        bad = {k: x for k, x in st.items() if k not in ("I_hip", "I_oracle", "culled_instances", "lazy_lists") and x != 0}
        assert not bad, ("forward", bad)
        res = dict(desc, I=int(hf["I"]), visible=int((of["radii"] > 0).sum()), fwd_form=hf["fwd_form"],
                   lazy_lists=st["lazy_lists"], culled_instances=st.get("culled_instances", 0))
        dL = np.random.default_rng(seed + 7).standard_normal(of["image"].shape).astype(np.float32)
        hg = G.hip_backward(hf, dL, bwd_form=opt["bwd_form"])
        og = oracle.backward(v, of, dL)
        res.update(bwd_form=hg["bwd_form"], bwd_masks=hg["bwd_masks"])
        finite = all(np.isfinite(og[k]).all() for k in og if k in hg)
        res["oracle_finite"] = bool(finite)
        assert (hg["means2D"][:, 2] == 0).all()
        if not finite:
            for k in ("means3D", "scales", "rotations"):     # non-finite rows must be non-finite in the same places
                assert (np.isfinite(hg[k]) == np.isfinite(og[k])).all(), ("non-finite pattern", k)
            return res
        a = G.gradient_anchor_stats(hg, og, oracle.backward_f64(v, of, dL)) if res["visible"] > 0 else None
        for k in ("means2D", "conic", "opacities", "colors"):
            e = rel_l2(hg[k], og[k])
            res["rel_" + k] = e
            # within the tolerance of the oracle -- or, where ONE Gaussian sums a million signed terms (a splat over the
            # whole image: the fp32 sums of the oracle's pixel order and of the device's tree differ by more than that),
            # no further from the float64 twin than the oracle is (the criterion of tests/gpu_util.py)
            assert e < GRAD_TOL or (a is not None and a[k]["rel_l2_hip"] <= max(GRAD_TOL, 1.25 * a[k]["rel_l2_oracle"])), \
                ("reverse walk", k, e, a[k] if a else None)
        if a is not None:
            for k in ("means3D", "scales", "rotations"):
                s_ = a[k]
                res["rel_all_" + k] = s_["rel_l2_all_hip_vs_oracle"]
                res["excluded_" + k] = s_["excluded_fraction"]       # reported, not bounded: the draws plant degenerate rows
                assert s_["rel_l2_well_hip"] <= max(GRAD_TOL, 1.25 * s_["rel_l2_well_oracle"]), (k, s_)
                assert s_["row_bound_violations"] == 0, (k, s_)
                assert s_["zero_rows_nonzero"] == 0, (k, s_)
                if s_["rows"] > 64:                                  # (in L2 over a handful of rows one row IS the norm)
                    assert s_["err_l2_excess_units"] <= G.L2_FLOOR, (k, s_)
        return res
    finally:
        for k, v in prev.items():
            tune.set_knob(k, v)


def run_props(seed):
    """Size-independent properties on a drawn case, through the packages' autograd drop-in (no oracle):
    (1) the image split into `world` bands of tile rows (log_amd.rasterizer.tile_rows) renders the whole image bit for bit,
        radii / point_weight are the maxima over the bands, and the bands' reverse-walk gradients sum to the whole view's;
    (2) two or three views accumulated by the backward kernels into a gradient bucket (row-major rows / planar attribute
        blocks: accumulate_grads_into) equal autograd's own view-by-view accumulation."""
    import torch
    import gpu_util as G
    from diff_gaussian_rasterization_wodilate import GaussianRasterizer as RastFork
    from diff_gaussian_rasterization import GaussianRasterizer as RastUp
    from log_amd import dist as D, rasterizer as R, scenes
    desc, cam, sc, opt = draw_case(seed)
    rng = np.random.default_rng(seed + 99)
    dev = torch.device("cuda:0")
    n, W, H = desc["n"], desc["W"], desc["H"]
    fork = opt["flavour"] == "wodilate"
    Rast = RastFork if fork else RastUp
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    names = dict(means3D="xyz", scales="scaling", rotations="rotation", opacities="opacity", colors="colors")
    w = torch.tensor(rng.standard_normal((3, H, W)).astype(np.float32), device=dev)
    res = dict(desc)

    def render(camera, rows=None, sink=None, leaves=None):
        leaves = leaves or {k: T(sc[v]).requires_grad_(True) for k, v in names.items()}
        m2 = torch.zeros(n, 3, device=dev, requires_grad=True)
        rast = Rast(raster_settings=G.settings(camera, opt["bg"], dev, opt["scale_modifier"]))
        kw = dict(means3D=leaves["means3D"], means2D=m2, shs=None, colors_precomp=leaves["colors"], opacities=leaves["opacities"],
                  scales=leaves["scales"], rotations=leaves["rotations"], cov3D_precomp=None)
        with (R.tile_rows(*rows) if rows else R.tile_rows(0, 0)):
            if sink is not None:
                with R.accumulate_grads_into(sink):
                    out = rast(**kw)
                    (out[0] * w).sum().backward()
            else:
                out = rast(**kw)
                img = out[0] if rows is None else out[0][:, rows[0] * 16:rows[1] * 16]
                ww = w if rows is None else w[:, rows[0] * 16:rows[1] * 16]
                (img * ww).sum().backward()
        return out, leaves, m2

    # ---- (1) bands ----
    full, lv, m2 = render(cam)
    torch.cuda.synchronize()
    if R.last_state_info()[0] > 40_000_000:
        return dict(res, skipped="more instances than worth rendering several times")
    finite = bool(torch.isfinite(lv["means3D"].grad).all() and torch.isfinite(lv["scales"].grad).all())
    world = int(rng.choice([2, 3, 5, 8]))
    image = torch.empty_like(full[0])
    radii = torch.zeros_like(full[1])
    gs = {k: torch.zeros_like(v.grad) for k, v in lv.items()}
    gm2 = torch.zeros_like(m2.grad)
    pw = torch.zeros_like(full[4]) if fork else None
    for r in range(world):
        rows = D.band_rows(r, world, H)
        b, e = D.band_pixels(r, world, H)
        if rows[1] <= rows[0]:
            continue
        out, l2, mm = render(cam, rows=rows)
        image[:, b:e] = out[0][:, b:e]
        radii = torch.maximum(radii, out[1])
        if fork:
            pw = torch.maximum(pw, out[4])
        for k in gs:
            gs[k] += l2[k].grad
        gm2 += mm.grad
    covered = D.band_pixels(world - 1, world, H)[1] == H and all(D.band_rows(r, world, H)[1] > D.band_rows(r, world, H)[0] for r in range(world))
    if covered:
        assert torch.equal(image, full[0]), "bands: image"
        assert torch.equal(radii, full[1]), "bands: radii"
        assert not fork or torch.equal(pw, full[4]), "bands: point_weight"
        rel = lambda a, b: float((a - b).norm() / b.norm().clamp_min(1e-30))
        res["band_rel"] = {k: rel(gs[k], lv[k].grad) for k in ("opacities", "colors")}
        res["band_rel"]["means2D"] = rel(gm2, m2.grad)
        # (a splat over the whole image sums ~1e6 signed terms per Gaussian: the bands' partial sums and the whole view's
        # differ by fp32 summation order -- measured 1.1e-4 on one such case; 3e-4 there, 1e-4 everywhere else)
        tol = 3e-4 if ("giant" in desc["degenerate"] or desc["scene"] == "coarse") else GRAD_TOL
        for k, v in res["band_rel"].items():
            assert v < tol or not finite, ("bands", k, v, world)
    res["bands"] = world if covered else 0
    # ---- (2) accumulation into a bucket ----
    nv = int(rng.integers(2, 4))
    cams = [cam] + [scenes.orbit_cameras(5, W=W, H=H, focal=desc["focal"], radius=desc["radius"])[int(rng.integers(0, 5))] for _ in range(nv - 1)]
    prev = R.set_inplace_leaf_grads(False)
    try:
        leaves = {k: T(sc[v]).requires_grad_(True) for k, v in names.items()}
        for c in cams:
            render(c, leaves=leaves)
        torch.cuda.synchronize()
        want = {k: v.grad.clone() for k, v in leaves.items()}
    finally:
        R.set_inplace_leaf_grads(prev)
    for row_major in (True, False):
        bucket = D.GradientBucket(n, dev, 1, row_major=row_major)
        leaves = {k: T(sc[v]).requires_grad_(True) for k, v in names.items()}
        for c in cams:
            render(c, sink=bucket.sink(), leaves=leaves)
        torch.cuda.synchronize()
        got = {k: bucket.alias[k] for k in names}
        for k in ("opacities", "colors"):
            e = float((got[k].reshape(want[k].shape) - want[k]).norm() / want[k].norm().clamp_min(1e-30))
            res["sink_%s_%s" % ("rows" if row_major else "planar", k)] = e
            assert e < GRAD_TOL or not finite, ("sink", row_major, k, e)
        for k in ("means3D", "scales", "rotations"):      # behind the chain rule: reported (conditioning: see run_case)
            e = float((got[k].reshape(want[k].shape) - want[k]).norm() / want[k].norm().clamp_min(1e-30))
            res["sink_%s_%s" % ("rows" if row_major else "planar", k)] = e
    return res


# ---- mode "calls": the other kinds of rasterizer call, crossed with what draw_case varies ---------------------------------
KINDS = ("aux", "second_pass", "camera", "shs", "cov3d")
CAPACITIES = ("exact", "speculative", "fixed", "speculative_too_small")
# geometry_reuse_stats(): the reasons a drawn second call may name (log_amd.rasterizer._ReuseSlot.match) when it runs the full
# forward.  The draws keep object, settings, stream, form, plan and capacity policy: only a view without instances remains.
REUSE_FALLBACKS = ("no_instances",)
CAMERA_DROP_CAP = 0.01
EPS32 = 6e-8


def draw_call(seed):
    """draw_case(seed) as it is, plus -- from a random stream of its own -- the kind of call, the capacity mode and the
    kind's own parameters -> (description, cam, scene, options, call).  call["mapped"] lists what the packages refuse and
    what the draw was mapped to instead (today: use_filter=False under the upstream package, which has no such switch)."""
    desc, cam, sc, opt = draw_case(seed)
    rng = np.random.default_rng([int(seed), 0xCA11])
    call = dict(kind=str(rng.choice(KINDS)), capacity=str(rng.choice(CAPACITIES)), sh_degree=int(rng.integers(0, 4)),
                sh_extra=int(rng.integers(0, 3)), use_filter=opt["use_filter"], mapped=[])
    if not opt["use_filter"] and opt["flavour"] == "upstream":
        call["use_filter"] = True
        call["mapped"].append("use_filter=False under the upstream package -> True")
    # (aux / camera with a band, a sink or cov3D_precomp, camera with aux: one kind per call and no band or sink drawn)
    shown = {k: v for k, v in call.items() if k != "use_filter"}
    return dict(desc, call_use_filter=call["use_filter"], **shown), cam, sc, opt, call


def _decide(cam, sc, filter_mode, ndc_cull, scale_modifier, dt, cov6=None):
    """The forward's per-Gaussian decisions from the inputs, on the host, every operation in dtype dt: live (depth, |ndc|
    cull, det, tile rect), the x / y clamp branches of the EWA Jacobian (|t.x / t.z| against 1.3 tanfov), the CLAMP low-pass
    (raw diagonals against 0.3) -- and the compared values themselves."""
    from util import cam_tan
    f = lambda a: np.asarray(a, dt)
    W, H = int(cam["image_width"]), int(cam["image_height"])
    tfx, tfy = (dt(x) for x in cam_tan(cam))
    V, P, p = f(cam["world_view_transform"]), f(cam["full_proj_transform"]), f(sc["xyz"])
    with np.errstate(all="ignore"):
        fx, fy = dt(W) / (dt(2) * tfx), dt(H) / (dt(2) * tfy)
        t = p @ V[:3, :3] + V[3, :3]
        hom = p @ P[:3, :] + P[3, :]
        pw = dt(1) / (hom[:, 3] + dt(1e-7))
        nx, ny = hom[:, 0] * pw, hom[:, 1] * pw
        tz = t[:, 2]
        live = tz > dt(0.2)
        if ndc_cull:
            live &= (nx >= dt(-1.3)) & (nx <= dt(1.3)) & (ny >= dt(-1.3)) & (ny <= dt(1.3))
        if cov6 is not None:
            c6 = f(cov6)
            Sg = np.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4], c6[:, 2], c6[:, 4], c6[:, 5]], -1).reshape(-1, 3, 3)
        else:
            s, q = f(sc["scaling"]) * dt(scale_modifier), f(sc["rotation"])
            r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            one, two = dt(1), dt(2)
            R = np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
                          two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
                          two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], -1).reshape(-1, 3, 3)
            M = R * s[:, None, :]
            Sg = M @ M.transpose(0, 2, 1)
        limx, limy = dt(1.3) * tfx, dt(1.3) * tfy
        tzs = np.where(live, tz, dt(1))
        rx, ry = t[:, 0] / tzs, t[:, 1] / tzs
        cx, cy = np.abs(rx) > limx, np.abs(ry) > limy
        ux, uy = np.clip(rx, -limx, limx), np.clip(ry, -limy, limy)
        J = np.zeros((len(p), 2, 3), dt)
        J[:, 0, 0], J[:, 0, 2], J[:, 1, 1], J[:, 1, 2] = fx / tzs, -(fx * ux * tzs) / (tzs * tzs), fy / tzs, -(fy * uy * tzs) / (tzs * tzs)
        Tm = J @ V[:3, :3].T
        cov = Tm @ Sg @ Tm.transpose(0, 2, 1)
        a_raw, b, c_raw = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
        lowa, lowc = ~(a_raw >= dt(0.3)), ~(c_raw >= dt(0.3))
        a, c = a_raw, c_raw
        if filter_mode == 1:
            a, c = a + dt(0.3), c + dt(0.3)
        elif filter_mode == 2:
            a, c = np.maximum(a, dt(0.3)), np.maximum(c, dt(0.3))
        else:
            lowa, lowc = np.zeros_like(lowa), np.zeros_like(lowc)
        det = a * c - b * b
        live &= det != 0
        mid = dt(0.5) * (a + c)
        radius = np.ceil(dt(3) * np.sqrt(mid + np.sqrt(np.maximum(mid * mid - det, dt(0.1)))))
        mx, my = ((nx + dt(1)) * dt(W) - dt(1)) * dt(0.5), ((ny + dt(1)) * dt(H) - dt(1)) * dt(0.5)
        gx, gy = (W + 15) // 16, (H + 15) // 16
        x0, x1 = np.clip(np.trunc((mx - radius) / dt(16)), 0, gx), np.clip(np.trunc((mx + radius + dt(15)) / dt(16)), 0, gx)
        y0, y1 = np.clip(np.trunc((my - radius) / dt(16)), 0, gy), np.clip(np.trunc((my + radius + dt(15)) / dt(16)), 0, gy)
        live &= (x1 - x0) * (y1 - y0) > 0
        rect = np.where(live[:, None], np.stack([x0, x1, y0, y1], -1), 0).astype(np.int64)
    return dict(live=live, cx=cx, cy=cy, lowa=lowa, lowc=lowc, rx=rx, ry=ry, a_raw=a_raw, c_raw=c_raw, limx=limx, limy=limy,
                rect=rect)


def rect_lists(cam, sc, flavour, use_filter, scale_modifier):
    """(instances, longest tile list) of the plain rect rule, from the fp32 host decisions (no GPU, no oracle): what a draw
    costs the oracle, and whether it holds a list above the 4096 keys from which lists are ordered lazily."""
    fm = {"wodilate": 2, "upstream": 1}[flavour] if use_filter else 0
    r = _decide(cam, sc, fm, flavour == "wodilate", scale_modifier, np.float32)["rect"]
    gx, gy = (int(cam["image_width"]) + 15) // 16, (int(cam["image_height"]) + 15) // 16
    grid = np.zeros((gy + 1, gx + 1), np.int64)
    for ys, xs, sign in ((2, 0, 1), (2, 1, -1), (3, 0, -1), (3, 1, 1)):      # a 2-D difference array, summed twice
        np.add.at(grid, (r[:, ys], r[:, xs]), sign)
    lens = grid.cumsum(0).cumsum(1)[:gy, :gx]
    return int(((r[:, 1] - r[:, 0]) * (r[:, 3] - r[:, 2])).sum()), int(lens.max()) if lens.size else 0


def camera_prepass(cam, sc, flavour, use_filter, scale_modifier, cov6=None):
    """Which rows a float64 reference of the chain rule can follow the fp32 forward on (no GPU needed).  The reference must
    take the forward's decisions; they are computed here in fp32 and in float64, and a row is DROPPED (zero upstream gradient
    on both sides of the comparison) where the two disagree -- or where the compared value lies within four times the
    distance between its fp32 and its float64 evaluation of the threshold (+ 4 ulp of the threshold itself): the device
    evaluates in fp32 with its own operation order and contractions, so closer than that its decision is not the host's to know.
    -> dict(drop bool[N], live, dropped, decisions = the fp32 ones, share)."""
    fm = {"wodilate": 2, "upstream": 1}[flavour] if use_filter else 0
    cull = flavour == "wodilate"
    d32, d64 = (_decide(cam, sc, fm, cull, scale_modifier, dt, cov6) for dt in (np.float32, np.float64))
    either, both = d32["live"] | d64["live"], d32["live"] & d64["live"]

    def near(key, thr):
        v32, v64 = np.abs(d32[key].astype(np.float64)), np.abs(d64[key])
        with np.errstate(all="ignore"):
            return ~(np.abs(v64 - thr) > 4.0 * np.abs(v32 - v64) + 4.0 * EPS32 * thr)
    drop = d32["live"] != d64["live"]
    why = dict(live=int(drop.sum()))
    branch = both & ((d32["cx"] != d64["cx"]) | (d32["cy"] != d64["cy"]))
    close = both & (near("rx", float(d64["limx"])) | near("ry", float(d64["limy"])))
    if fm == 2:
        branch |= both & ((d32["lowa"] != d64["lowa"]) | (d32["lowc"] != d64["lowc"]))
        close |= both & (near("a_raw", 0.3) | near("c_raw", 0.3))
    drop |= branch | close
    why.update(branch=int(branch.sum()), near=int((close & ~branch).sum()))   # (branch: the rows between the fp32 and the float64 limit)
    live, dropped = int(d32["live"].sum()), int((drop & either).sum())
    return dict(drop=drop, live=live, dropped=dropped, share=dropped / max(live, 1), decisions=d32, why=why)


def _chain_f64(cam, sc, flavour, use_filter, scale_modifier, live, dec, g2, gc, cov6=None, device="cpu"):
    """float64 autograd of the projection alone (oracle/torch_oracle.py::project under the fp32 forward's decisions `dec`):
    the gradients of sum(g2 . ndc + gc . conic) over the `live` rows -> dict(V, P, means3D[, cov3D]) float64."""
    import torch
    from oracle import torch_oracle
    from util import cam_tan
    tfx, tfy = cam_tan(cam)
    fm = {"wodilate": 2, "upstream": 1}[flavour] if use_filter else 0
    T = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, device=device, requires_grad=g)
    B = lambda a: torch.tensor(np.asarray(a, bool), device=device)
    V, P, m = T(cam["world_view_transform"], True), T(cam["full_proj_transform"], True), T(sc["xyz"], True)
    cv = T(cov6, True) if cov6 is not None else None
    n = len(sc["xyz"])
    d = dict(cx=B(dec["cx"]), cy=B(dec["cy"]), lowa=B(dec["lowa"]), lowc=B(dec["lowc"]), limx=float(dec["limx"]), limy=float(dec["limy"]))
    pr = torch_oracle.project(cam["image_width"], cam["image_height"], tfx, tfy, V, P, m, torch.zeros(n, 3, dtype=torch.float64, device=device),
                              None if cv is not None else T(sc["scaling"]), None if cv is not None else T(sc["rotation"]),
                              scale_modifier=scale_modifier, filter_mode=fm, ndc_cull=flavour == "wodilate", cov3D_precomp=cv,
                              decisions=d)
    w = B(live)
    g2t, gct = T(g2), T(gc)
    zero = torch.zeros(n, dtype=torch.float64, device=device)
    terms = g2t[:, 0] * pr["ndc"][:, 0] + g2t[:, 1] * pr["ndc"][:, 1] + sum(gct[:, j] * pr["conic"][j] for j in range(3))
    loss = torch.where(w, terms, zero).sum()
    out = dict(V=np.zeros((4, 4)), P=np.zeros((4, 4)), means3D=np.zeros((n, 3)))
    if bool(w.any()):
        loss.backward()
        z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.cpu().numpy()
        out = dict(V=z(V), P=z(P), means3D=z(m))
        if cv is not None:
            out["cov3D"] = z(cv)
    elif cv is not None:
        out["cov3D"] = np.zeros((n, 6))
    return out


def _cov6(sc, scale_modifier):
    """[N, 6] fp32 covariances (xx, xy, xz, yy, yz, zz) of the scene's scales (times the modifier) and rotations, in float64."""
    import torch
    from oracle import torch_oracle
    Rm = torch_oracle._rot(torch.tensor(sc["rotation"], dtype=torch.float64))
    M = Rm * (torch.tensor(sc["scaling"], dtype=torch.float64) * scale_modifier)[:, None, :]
    S = (M @ M.transpose(1, 2)).numpy()
    return np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1).astype(np.float32)


def _sum_f64(fs):
    """The float64 twin of a sum of backwards (the backward is linear in dL): the values add; the row's unit of the sum is the
    SUM of the addends' units (tests/gpu_util.py: unit_i = 6e-8 cond_i |g_i| + |chain32_i - g_i|) -- an addend's error budget
    does not shrink because the other addend cancels its value, nor because the two fp32 evaluation errors happen to point
    against each other.  gradient_anchor_stats builds its unit as 6e-8 max(cond, 1) |g| + |chain32 - g|, so both terms of
    every addend go into `cond` of the sum, cond = sum_i unit_i / (6e-8 |sum g_i|), and chain32 of the sum is the sum itself.
    (Adding the chain32 VALUES instead, signs and all, called the one row that owns seed 700579's figure well-conditioned:
    evaluation errors of 4.1e-5 and 2.8e-5 of the row, one per image, left 2.5e-5 in the signed sum, under the 3e-5 at which a
    row counts as one fp32 can know -- profiles/fuzz_calls.md.)"""
    out = {k: sum(f[k] for f in fs) for k in fs[0] if k not in ("cond", "chain32")}
    out["chain32"] = {k: out[k].copy() for k in fs[0]["chain32"]}
    cond = np.zeros_like(fs[0]["cond"])
    for j, k in enumerate(("means3D", "scales", "rotations")):
        units = sum(EPS32 * np.maximum(f["cond"][:, j], 1.0) * np.linalg.norm(f[k], axis=1) +
                    np.linalg.norm(f["chain32"][k].astype(np.float64) - f[k], axis=1) for f in fs)
        y = np.linalg.norm(out[k], axis=1)
        cond[:, j] = np.where(y > 0, units / np.maximum(EPS32 * y, 1e-300), 1.0)      # (a zero row has no unit)
    out["cond"] = cond
    return out


def _hold_anchored(res, hg, ogs, f64s, report=None):
    """dL/dmeans3D, dL/dscales, dL/drotations by the anchored criterion of run_case, against the oracle's backwards added.
    report: a prefix -- the figures of `hg` (the comparator's gradients) are only recorded under it, nothing is asserted."""
    import gpu_util as G
    og = {k: sum(np.asarray(o[k], np.float64) for o in ogs) for k in ogs[0]}
    g64 = _sum_f64(f64s) if len(f64s) > 1 else f64s[0]
    filler = {k: og[k] for k in ("means2D", "conic", "opacities", "colors")}      # (their statistics are not read here)
    a = G.gradient_anchor_stats(dict(filler, **hg), og, g64)
    if report:
        for k in ("means3D", "scales", "rotations"):
            res[report + "well_" + k] = (a[k]["rel_l2_well_hip"], a[k]["rel_l2_well_oracle"])
            res[report + "units_" + k] = (a[k]["worst_row_excess_units"], a[k]["err_l2_excess_units"])
        return
    _assert_anchored(res, a)


def _assert_anchored(res, a, names=None):
    """What run_case asserts of gradient_anchor_stats' chain-rule slots; names: slot -> the name it is reported under."""
    import gpu_util as G
    for slot, k in (names or dict(means3D="means3D", scales="scales", rotations="rotations")).items():
        s_ = a[slot]
        res["rel_all_" + k] = s_["rel_l2_all_hip_vs_oracle"]
        res["well_" + k] = (s_["rel_l2_well_hip"], s_["rel_l2_well_oracle"])
        res["excluded_" + k] = s_["excluded_fraction"]
        res["units_" + k] = (s_["worst_row_excess_units"], s_["err_l2_excess_units"])
        assert s_["rel_l2_well_hip"] <= max(GRAD_TOL, 1.25 * s_["rel_l2_well_oracle"]), (k, s_)
        assert s_["row_bound_violations"] == 0, (k, s_)
        assert s_["zero_rows_nonzero"] == 0, (k, s_)
        if s_["rows"] > 64:
            assert s_["err_l2_excess_units"] <= G.L2_FLOOR, (k, s_)


def run_call(oracle, seed):
    """One drawn call of a drawn kind through the public packages, in the drawn capacity mode, against its comparator in
    exact mode (module docstring of tests/test_gpu_fuzz.py lists the relations per kind)."""
    import contextlib
    import torch
    import gpu_util as G
    import diff_gaussian_rasterization as up
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R, tune
    from util import rel_l2
    desc, cam, sc, opt, call = draw_call(seed)
    res = dict(desc)
    dev = torch.device("cuda:0")
    fork = opt["flavour"] == "wodilate"
    mod, fl = (wo, R.WODILATE) if fork else (up, R.UPSTREAM)
    n, W, H, kind = desc["n"], desc["W"], desc["H"], call["kind"]
    uf, smod, bg = call["use_filter"], opt["scale_modifier"], opt["bg"]
    tol = 3e-4 if ("giant" in desc["degenerate"] or desc["scene"] == "coarse") else GRAD_TOL     # (run_props measured it)
    rng = np.random.default_rng([int(seed), 0xD1])
    w1 = rng.standard_normal((3, H, W)).astype(np.float32)
    w2 = rng.standard_normal((3, H, W)).astype(np.float32)
    T = lambda a, g=True: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=g)
    W1, W2 = T(w1, False), T(w2, False)
    rs0 = G.settings(cam, bg, dev, smod)
    fkw = {"use_filter": False} if (fork and not uf) else {}
    names = dict(means3D="xyz", scales="scaling", rotations="rotation", opacities="opacity", colors="colors")
    key = (dev.index or 0, W, H, (0, 0))

    def leaves(**more):
        L = {k: T(sc[v]) for k, v in names.items()}
        L["means2D"] = torch.zeros(n, 3, device=dev, requires_grad=True)
        L.update({k: T(v) for k, v in more.items()})
        return L

    def fwd(L, rast=None, rs=rs0, **over):
        kw = dict(means3D=L["means3D"], means2D=L["means2D"], shs=None, colors_precomp=L["colors"], opacities=L["opacities"],
                  scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None)
        kw.update(over)
        return (rast or mod.GaussianRasterizer(raster_settings=rs))(**kw, **fkw)

    def grads(L):
        torch.cuda.synchronize()
        return {k: (None if t.grad is None else t.grad.detach().cpu().numpy()) for k, t in L.items()}

    def bits(t):
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        return a.view(np.uint32) if a.dtype == np.float32 else a

    def same_outputs(x, y, what):
        out_names = ("image", "radii", "point_id_pixel", "point_weight_pixel", "point_weight") if fork else ("image", "radii")
        assert len(x) == len(y) == len(out_names), (what, len(x), len(y))
        for name, p, q in zip(out_names, x, y):
            assert np.array_equal(bits(p), bits(q)), (what, name)

    def close(got, want, what, bound=tol):
        """rel L2 of a reverse-walk output against the comparator's; all zeros against all zeros is exact."""
        if not np.any(want):
            assert got is None or not np.any(got), (what, "expected zeros")
            return
        e = rel_l2(got, want)
        res["rel_" + what] = e
        assert e < bound, (what, e, bound)

    def oracle_pair(colour_sets, dLs):
        """The oracle's forward, backward and float64 backward per colour set -> (forwards, og list, f64 list or None,
        finite)."""
        ofs, ogs, fs = [], [], []
        for col, dL in zip(colour_sets, dLs):
            v, of = G.oracle_forward(oracle, cam, dict(sc, colors=col), bg, flavour=fl, use_filter=uf, scale_modifier=smod)
            ofs.append(of)
            ogs.append(oracle.backward(v, of, dL))
        finite = all(np.isfinite(og[k]).all() for og in ogs for k in og)
        res["oracle_finite"] = bool(finite)
        res["visible"] = int((ofs[0]["radii"] > 0).sum())
        if finite and res["visible"] > 0:
            fs = [oracle.backward_f64(of["_view"], of, dL) for of, dL in zip(ofs, dLs)]
        return ofs, ogs, fs, finite

    def hold_chain(hg, ogs, fs, finite, comparator=None):
        """comparator: the same three gradients of the comparator's calls -- its figures under the same criterion are
        recorded next to the main call's (`pair_*`), so that a failing case says whether the established path shares it."""
        if finite and fs and comparator is not None:
            _hold_anchored(res, comparator, ogs, fs, report="pair_")
        if not finite:
            og = {k: sum(np.asarray(o[k], np.float64) for o in ogs) for k in ("means3D", "scales", "rotations")}
            for k in og:
                assert (np.isfinite(hg[k]) == np.isfinite(og[k])).all(), ("non-finite pattern", k)
        elif fs:
            _hold_anchored(res, hg, ogs, fs)
        else:                                    # a view that sees nothing: exact zeros
            assert res["visible"] == 0
            for k in ("means3D", "scales", "rotations"):
                assert not np.any(hg[k]), ("nothing visible, yet a gradient", k)

    state = {}

    @contextlib.contextmanager
    def capacity(mode):
        """The calls inside run in this capacity mode; afterwards: no overflow recorded, and under a guess that was too
        small the repeated stage 2 shows in capacity_stats()."""
        prev = R.set_speculative(mode != "exact")
        R.capacity_stats(reset=True)
        R.overflow_since_reset(dev)
        try:
            if mode == "fixed":
                R.set_instance_capacity(state["I"] + 64, max_tile_len=state["max_len"] + 64)
            if mode == "speculative_too_small":
                R._cap_model.hist[key] = dict(state["poison"])
            yield
            torch.cuda.synchronize()
            chk, st = R.overflow_since_reset(dev), R.capacity_stats()
            if mode != "exact":
                res["capacity_ran"], res["retries"] = mode, st["retries"]
            assert not chk["overflowed"], ("overflow", mode, chk)
            if mode == "speculative_too_small":
                assert st["retries"] >= 1, ("the guess was not too small", st)
        finally:
            R.set_instance_capacity(None)
            R.set_speculative(prev)
            R.capacity_stats(reset=True)

    prev_knobs = {k: tune.get_knob(k) for k in list(opt["knobs"]) + ["LOGRAST_FWD_ROWS", "LOGRAST_BWD_ROWS"]}
    for k, v in opt["knobs"].items():
        tune.set_knob(k, v)
    for k, form in (("LOGRAST_FWD_ROWS", opt["fwd_form"]), ("LOGRAST_BWD_ROWS", opt["bwd_form"])):
        if form is not None:
            tune.set_knob(k, {"rows": 1, "quadrant": 0}[form])
    prev_masks, prev_reuse = R.set_hit_masks(opt["hit_masks"]), R.set_geometry_reuse(False)
    try:
        # ---- the view's size first (exact mode, no gradients): the skip, the fixed capacity, the guess that is too small ----
        with capacity("exact"), torch.no_grad():
            fwd(leaves())
            info = R._status_block(dev).cpu().tolist()
        state["I"], state["max_len"], rect = int(info[1]), int(info[3]), int(info[4])
        res["I"] = state["I"]
        if max(rect, state["I"]) > MAX_INSTANCES:
            return dict(res, skipped="more tile instances than the CPU oracle walks in seconds")
        mode = call["capacity"]
        if mode == "speculative_too_small":      # a guess below the real numbers: of the instance count, else of the longest list
            tiles = ((W + 15) // 16) * ((H + 15) // 16)
            for poison in (dict(I=1.0, ratio=1e-6, L=float(1 << 20)), dict(I=float(4 * state["I"] + 4), ratio=0.0, L=1.0)):
                R._cap_model.hist[key] = dict(poison)
                cap, mlen = R._cap_model.guess(key, n, tiles)
                if cap < state["I"] or (mlen and mlen < state["max_len"]):
                    state["poison"] = poison
                    break
            R.capacity_stats(reset=True)
            if "poison" not in state:            # (every guess has a floor of 4096 instances and 256 entries: nothing is below)
                mode = "speculative"
                res["mapped"] = call["mapped"] + ["speculative_too_small on a view below the guess's floor -> speculative"]
        ctx = types.SimpleNamespace(          # what a kind gets: the draw, the tensors' makers, the shared checks
            oracle=oracle, res=res, call=call, cam=cam, sc=sc, opt=opt, n=n, dev=dev, mod=mod, fl=fl, fork=fork, uf=uf, tol=tol,
            rng=rng, w1=w1, w2=w2, W1=W1, W2=W2, T=T, rs0=rs0, mode=mode, leaves=leaves, fwd=fwd, grads=grads, bits=bits,
            same_outputs=same_outputs, close=close, oracle_pair=oracle_pair, hold_chain=hold_chain, capacity=capacity)
        CALL_KINDS[kind](ctx)
        return res
    except Exception as e:        # (the figures recorded up to the failing assertion travel with it: main() writes them out)
        e.partial = res
        raise
    finally:
        R.set_hit_masks(prev_masks)
        R.set_geometry_reuse(prev_reuse)
        for k, v in prev_knobs.items():
            tune.set_knob(k, v)


def _call_aux(c):
    from log_amd import rasterizer as R
    res, rng, n, sc = c.res, c.rng, c.n, c.sc
    aux = (rng.standard_normal((n, 3)) * 1.0e3 * rng.random((n, 1))).astype(np.float32)       # both signs, magnitudes up to ~1e3
    w2 = c.w2 * np.float32(1e-3)
    W2 = c.T(w2, False)
    with c.capacity("exact"):                       # the two-call pair, geometry reuse off
        Lp = c.leaves(aux=aux)
        p1 = c.fwd(Lp)
        sv = p1[0].grad_fn.saved
        fT, nc = sv["final_T"].clone(), sv["n_contrib"].clone()
        p2 = c.fwd(Lp, colors_precomp=Lp["aux"])
        ((p1[0] * c.W1).sum() + (p2[0] * W2).sum()).backward()
        gp = c.grads(Lp)
    with c.capacity(c.mode):
        La = c.leaves(aux=aux)
        a = c.fwd(La, aux_colors=La["aux"])
        sa = a[0].grad_fn.saved
        res["forms"] = dict(fwd=R._backend.last_forms["fwd"])
        ((a[0] * c.W1).sum() + (a[-1] * W2).sum()).backward()
        res["forms"]["bwd"] = R._backend.last_forms["bwd"]
        ga = c.grads(La)
    assert res["forms"] == dict(fwd="quadrant", bwd="quadrant"), res["forms"]
    c.same_outputs(a[:-1], p1, "aux call")
    assert np.array_equal(c.bits(a[-1]), c.bits(p2[0])), "aux_image"
    assert np.array_equal(c.bits(sa["final_T"]), c.bits(fT)) and np.array_equal(c.bits(sa["n_contrib"]), c.bits(nc))
    ofs, ogs, fs, finite = c.oracle_pair([sc["colors"], aux], [c.w1, w2])
    assert np.array_equal(c.bits(a[0]), ofs[0]["image"].view(np.uint32)), "image against the oracle"
    assert np.array_equal(c.bits(a[-1]), ofs[1]["image"].view(np.uint32)), "aux image against the oracle"
    for k in ("opacities", "colors", "aux"):
        c.close(ga[k], gp[k], k)
    c.close(ga["means2D"][:, :2], gp["means2D"][:, :2], "means2D")
    assert (ga["means2D"][:, 2] == 0).all()
    chain = ("means3D", "scales", "rotations")
    c.hold_chain({k: ga[k] for k in chain}, ogs, fs, finite, comparator={k: gp[k] for k in chain})


def _call_second_pass(c):
    from log_amd import rasterizer as R
    res, sc, cam, n = c.res, c.sc, c.cam, c.n
    xyz1 = np.concatenate([sc["xyz"], np.ones((n, 1), np.float32)], axis=1).astype(np.float32)
    pd = np.ascontiguousarray((xyz1 @ np.asarray(cam["world_view_transform"], np.float32))[:, 2], np.float32)
    col2 = np.ascontiguousarray(np.stack([pd, sc["xyz"][:, 2], np.ones(n, np.float32)], axis=-1), np.float32)   # [view z, world z, 1]

    def two_calls():
        L = c.leaves(colors2=col2)
        rast = c.mod.GaussianRasterizer(raster_settings=c.rs0)
        R.geometry_reuse_stats(reset=True)
        o1 = c.fwd(L, rast=rast)
        o2 = c.fwd(L, rast=rast, colors_precomp=L["colors2"])
        stats = R.geometry_reuse_stats()
        ((o1[0] * c.W1).sum() + (o2[0] * c.W2).sum()).backward()
        return o1, o2, c.grads(L), stats
    with c.capacity("exact"):
        a1, a2, ga, sa = two_calls()
    assert sa == dict(reused=0, fallback={}), sa
    R.set_geometry_reuse(True)
    try:
        with c.capacity(c.mode):
            b1, b2, gb, sb = two_calls()
    finally:
        R.set_geometry_reuse(False)
    why = [k for k in sb["fallback"] if k != "first"]
    assert sb["fallback"].get("first") == 1 and sb["reused"] + len(why) == 1, sb
    res["reuse"] = "reused" if sb["reused"] else why[0]
    assert res["reuse"] == "reused" or res["reuse"] in REUSE_FALLBACKS, sb
    c.same_outputs(b1, a1, "first call")
    c.same_outputs(b2, a2, "second call")
    ofs, ogs, fs, finite = c.oracle_pair([sc["colors"], col2], [c.w1, c.w2])
    assert np.array_equal(c.bits(b1[0]), ofs[0]["image"].view(np.uint32)), "first image against the oracle"
    assert np.array_equal(c.bits(b2[0]), ofs[1]["image"].view(np.uint32)), "second image against the oracle"
    for k in ("opacities", "colors", "colors2"):
        c.close(gb[k], ga[k], k)
    c.close(gb["means2D"][:, :2], ga["means2D"][:, :2], "means2D")
    chain = ("means3D", "scales", "rotations")
    c.hold_chain({k: gb[k] for k in chain}, ogs, fs, finite, comparator={k: ga[k] for k in chain})


def _call_camera(c):
    import torch
    import gpu_util as G
    from log_amd import rasterizer as R
    from util import rel_l2
    res, sc, cam, n, opt, T, dev = c.res, c.sc, c.cam, c.n, c.opt, c.T, c.dev
    # ---- through the package ----
    with c.capacity("exact"):
        Lp = c.leaves()
        p = c.fwd(Lp)
        (p[0] * c.W1).sum().backward()
        gp = c.grads(Lp)
    with c.capacity(c.mode):
        V, P = T(cam["world_view_transform"]), T(cam["full_proj_transform"])
        La = c.leaves()
        a = c.fwd(La, rs=c.rs0._replace(viewmatrix=V, projmatrix=P))
        (a[0] * c.W1).sum().backward()
        ga = c.grads(La)
    c.same_outputs(a, p, "camera call")
    dV, dP = V.grad.cpu().numpy(), P.grad.cpu().numpy()
    assert dV.shape == (4, 4) and dP.shape == (4, 4) and dV.dtype == np.float32
    assert (dV[:, 3] == 0.0).all() and (dP[:, 2] == 0.0).all(), (dV, dP)
    visible = int((p[1] > 0).sum())
    res["visible"] = visible
    if visible == 0:
        assert (dV == 0.0).all() and (dP == 0.0).all()
    for k in ("opacities", "colors"):
        c.close(ga[k], gp[k], k)
    c.close(ga["means2D"][:, :2], gp["means2D"][:, :2], "means2D")
    for k in ("means3D", "scales", "rotations"):             # (the fp32 chain's own rows: reported)
        res["camera_rel_" + k] = rel_l2(ga[k], gp[k]) if np.isfinite(gp[k]).all() and np.any(gp[k]) else None
    # ---- isolated: the chain rule on fixed upstream gradients, values against float64 autograd of the projection ----
    uf = opt["use_filter"]              # (the backend takes the upstream flavour without its filter; the package does not)
    pre = camera_prepass(cam, sc, opt["flavour"], uf, opt["scale_modifier"])
    res.update(camera_live=pre["live"], camera_dropped=pre["dropped"], camera_drop_why=pre["why"])
    assert pre["dropped"] <= CAMERA_DROP_CAP * pre["live"], ("camera pre-pass", pre["dropped"], pre["live"])
    hf = G.hip_forward(cam, sc, opt["bg"], c.fl, uf, dev, opt["scale_modifier"])
    rs, flavour, use_filter, m, s, r, saved = hf["_torch"]
    rng = np.random.default_rng([int(res["seed"]), 0xD2])
    g2 = np.concatenate([rng.standard_normal((n, 2)), np.zeros((n, 1))], axis=1).astype(np.float32)
    gc = np.concatenate([1e-3 * rng.standard_normal((n, 3)), np.zeros((n, 1))], axis=1).astype(np.float32)
    g2[pre["drop"]] = 0
    gc[pre["drop"]] = 0
    g2t, gct = T(g2, False), T(gc, False)
    run = lambda camera: R._backend.project_backward(rs, flavour, use_filter, m, s, r, saved["radii"], g2t, gct, camera=camera)
    plain, x, y = run(False), run(True), run(True)
    torch.cuda.synchronize()
    assert len(plain) == 3 and len(x) == 5
    for u, v in zip(plain, x[:3]):
        assert np.array_equal(c.bits(u), c.bits(v)), "per-Gaussian outputs with and without the camera sums"
    for u, v in zip(x, y):
        assert np.array_equal(c.bits(u), c.bits(v)), "two calls"
    iV, iP = x[3].cpu().numpy(), x[4].cpu().numpy()
    assert (iV[:, 3] == 0).all() and (iP[:, 2] == 0).all()
    live = (hf["radii"] > 0) & ~pre["drop"]
    ref = _chain_f64(cam, sc, opt["flavour"], uf, opt["scale_modifier"], live, pre["decisions"], g2[:, :2], gc[:, :3],
                     device=dev if n > 20000 else "cpu")
    res["camera_rows"] = int(live.sum())
    if not (np.isfinite(ref["V"]).all() and np.isfinite(ref["P"]).all()):
        res["camera_ref_finite"] = False         # (a live row whose float64 conic overflows: nothing to hold a value against)
        return
    for name, got, want in (("dV", iV, ref["V"]), ("dP", iP, ref["P"])):
        c.close(got, want, "isolated_" + name, GRAD_TOL)


def _call_shs(c):
    import torch
    from log_amd import rasterizer as R
    res, sc, n, rng, T, call = c.res, c.sc, c.n, c.rng, c.T, c.call
    deg = call["sh_degree"]
    K = min((deg + 1) ** 2 + call["sh_extra"], 16)       # (the library takes (degree + 1)^2 .. 16 coefficients)
    shs = (0.4 * rng.standard_normal((n, K, 3))).astype(np.float32)
    rs = c.rs0._replace(sh_degree=deg)
    m, sh = T(sc["xyz"], False), T(shs, False)
    cols, clamped = R._backend.sh_forward(m, rs.campos, sh, deg)
    cols_np = cols.cpu().numpy()
    # (the comparator's colours are the library's own: held here against the C oracle's, bit for bit with the clamp mask, the
    # relation of tests/test_gpu_sh_edges.py -- or a wrong sh_forward would be wrong on both sides of the comparison)
    campos = np.asarray(rs.campos.detach().cpu().numpy(), np.float32)
    ocol, ocl = c.oracle.sh_forward(sc["xyz"], campos, shs, deg)
    assert np.array_equal(clamped.cpu().numpy(), ocl), "sh_forward: clamp mask against the oracle"
    assert np.array_equal(c.bits(cols_np), c.bits(ocol)), "sh_forward: colours against the oracle"
    with c.capacity("exact"):                       # colors_precomp = the backend's own sh_forward
        Lp = c.leaves()
        Lp["colors"] = cols.clone().requires_grad_(True)
        p = c.fwd(Lp, rs=rs)
        (p[0] * c.W1).sum().backward()
        gp = c.grads(Lp)
        term = torch.zeros(n, 3, device=c.dev)
        want_shs = R._backend.sh_backward(m, rs.campos, sh, deg, clamped, Lp["colors"].grad.contiguous(), term)
        torch.cuda.synchronize()
        want_shs, term = want_shs.cpu().numpy(), term.cpu().numpy()
    res["sh_backward_held"] = bool(np.isfinite(gp["colors"]).all())      # (False is counted: profiles/fuzz_calls.md; never in the slice)
    if res["sh_backward_held"]:                        # (and the library's sh_backward against the oracle's, on the same dL/dcolors)
        ogs, ogm = c.oracle.sh_backward(sc["xyz"], campos, shs, deg, ocl, gp["colors"])
        c.close(want_shs, ogs, "sh_backward_shs", GRAD_TOL)
        c.close(term, ogm, "sh_backward_means3D", GRAD_TOL)
    with c.capacity(c.mode):
        La = c.leaves(shs=shs)
        a = c.fwd(La, rs=rs, shs=La["shs"], colors_precomp=None)
        (a[0] * c.W1).sum().backward()
        ga = c.grads(La)
    c.same_outputs(a, p, "shs call")
    assert ga["colors"] is None
    c.close(ga["shs"], want_shs, "shs")
    c.close(ga["opacities"], gp["opacities"], "opacities")
    c.close(ga["means2D"][:, :2], gp["means2D"][:, :2], "means2D")
    ofs, ogs, fs, finite = c.oracle_pair([cols_np], [c.w1])
    assert np.array_equal(c.bits(a[0]), ofs[0]["image"].view(np.uint32)), "image against the oracle"
    c.close(gp["colors"], ogs[0]["colors"], "colors")
    # dL/dmeans3D = the chain rule's + the view-direction term: the term is sh_backward's on the comparator's dL/dcolors, what
    # remains is anchored on the oracle
    rest = (ga["means3D"].astype(np.float64) - term.astype(np.float64)) if np.isfinite(ga["means3D"]).all() else ga["means3D"]
    c.hold_chain(dict(means3D=rest, scales=ga["scales"], rotations=ga["rotations"]), ogs, fs, finite)


def _call_cov3d(c):
    import torch
    import gpu_util as G
    from util import cam_tan, rel_l2
    oracle, res, sc, cam, n, opt, fl, T = c.oracle, c.res, c.sc, c.cam, c.n, c.opt, c.fl, c.T
    uf, smod, fork = c.uf, opt["scale_modifier"], c.fork
    cov = _cov6(sc, smod)
    with c.capacity(c.mode):
        L = {k: T(sc[v]) for k, v in dict(means3D="xyz", opacities="opacity", colors="colors").items()}
        L.update(means2D=torch.zeros(n, 3, device=c.dev, requires_grad=True), cov3D=T(cov), scales=None, rotations=None)
        a = c.fwd(L, scales=None, rotations=None, cov3D_precomp=L["cov3D"])
        (a[0] * c.W1).sum().backward()
        ga = c.grads({k: v for k, v in L.items() if v is not None})
    tfx, tfy = cam_tan(cam)
    fm = fl.filter_mode if uf else 0
    v = oracle.make_view(cam["image_width"], cam["image_height"], tfx, tfy, cam["world_view_transform"], cam["full_proj_transform"],
                         opt["bg"], scale_modifier=smod, filter_mode=fm, ndc_cull=fl.ndc_cull)
    of = oracle.forward(v, sc["xyz"], None, None, sc["opacity"], sc["colors"], cov3d=cov, extras=bool(fl.extras))
    assert np.array_equal(c.bits(a[0]), of["image"].view(np.uint32)), "image against the oracle's cov3D path"
    assert np.array_equal(a[1].cpu().numpy(), of["radii"]), "radii"
    if fork:
        assert np.array_equal(a[2].cpu().numpy(), of["point_id_pixel"]), "point_id_pixel"
        assert np.array_equal(c.bits(a[3]), of["point_weight_pixel"].view(np.uint32)), "point_weight_pixel"
        assert np.array_equal(c.bits(a[4]), of["point_weight"].view(np.uint32)), "point_weight"
    og = oracle.backward(v, of, c.w1)
    res["visible"] = int((of["radii"] > 0).sum())
    finite = all(np.isfinite(og[k]).all() for k in og)
    res["oracle_finite"] = bool(finite)
    if not finite:
        for k in ("means3D", "cov3D"):
            assert (np.isfinite(ga[k]) == np.isfinite(og[k])).all(), ("non-finite pattern", k)
        return
    assert (ga["means2D"][:, 2] == 0).all()
    hg = dict(means2D=ga["means2D"], opacities=ga["opacities"].reshape(-1, 1), colors=ga["colors"], means3D=ga["means3D"],
              cov3D=ga["cov3D"])
    errs = {k: rel_l2(hg[k], og[k]) if np.any(og[k]) else float(np.any(hg[k])) for k in hg}
    res.update({"rel_" + k: e for k, e in errs.items()})
    if all(e < c.tol for e in errs.values()) or res["visible"] == 0:
        assert all(e < c.tol for e in errs.values()), errs
        return
    # Beyond the tolerance against the fp32 oracle: the anchored criterion of run_case, with a float64 twin built here (the C
    # twin has no cov3D chain rule).  Reverse walk: the C twin's float64 sums.  Chain rule: float64 autograd of the projection
    # under the fp32 forward's decisions; chain32 = the oracle's fp32 chain rule on the float64 sums; cond = the C twin's
    # definition (lograst_oracle.c: ora64_project_bwd), the six stored covariance entries standing where scales and
    # quaternion stand there: worst relative change of the row over 3 draws, inputs scaled by (1 + pert u), the five sums
    # moved by pert u g_abs.  gradient_anchor_stats reads its three chain-rule slots as (means3D, cov3D, cov3D).
    import ctypes
    z = lambda *shape: np.zeros(shape, np.float64)
    nn, f64 = max(n, 1), np.float64
    g2, gcn, go, gcol, g_abs = z(nn, 3), z(nn, 4), z(nn), z(nn, 3), z(nn, 5)
    rec = np.ascontiguousarray(of["rec"])
    plist = of["point_list"] if of["I"] else np.zeros(1, np.uint32)
    P_ = oracle._p
    oracle.lib().ora64_blend_bwd(ctypes.byref(v), ctypes.c_int32(n), P_(rec), P_(of["tile_offsets"]), P_(plist), P_(of["n_contrib"]),
                                 P_(oracle._f32(c.w1)), P_(g2), P_(gcn), P_(go), P_(gcol), P_(g_abs))
    pre = camera_prepass(cam, sc, opt["flavour"], uf, smod, cov6=cov)
    res.update(cov3d_live=pre["live"], cov3d_dropped=pre["dropped"])
    assert pre["dropped"] <= CAMERA_DROP_CAP * pre["live"], ("cov3D pre-pass", pre["dropped"], pre["live"])
    keep = (of["radii"] > 0) & ~pre["drop"]
    where = c.dev if n > 20000 else "cpu"
    chain = lambda cv, a, b: _chain_f64(cam, sc, opt["flavour"], uf, smod, keep, pre["decisions"], a, b, cov6=cv, device=where)
    ref = chain(cov.astype(f64), g2[:n, :2], gcn[:n, :3])
    rng, pert = np.random.default_rng([int(res["seed"]), 0xD3]), 1e-7
    worst = {k: np.zeros(n) for k in ("means3D", "cov3D")}
    for _ in range(3):
        u = lambda *shape: rng.uniform(-1.0, 1.0, shape)
        alt = chain(cov.astype(f64) * (1.0 + pert * u(n, 6)), g2[:n, :2] + pert * u(n, 2) * g_abs[:n, :2],
                    gcn[:n, :3] + pert * u(n, 3) * g_abs[:n, 2:5])
        for k in worst:
            y = np.maximum(np.linalg.norm(ref[k], axis=1), 1e-300)
            worst[k] = np.maximum(worst[k], np.linalg.norm(alt[k] - ref[k], axis=1) / y)
    c32 = oracle.project_backward(v, of, g2[:n].astype(np.float32), gcn[:n].astype(np.float32))
    slots = lambda d: dict(means3D=np.where(keep[:, None], d["means3D"], 0), scales=np.where(keep[:, None], d["cov3D"], 0),
                           rotations=np.where(keep[:, None], d["cov3D"], 0))
    g64 = dict(slots(ref), cond=np.stack([worst["means3D"], worst["cov3D"], worst["cov3D"]], axis=1) / pert, chain32=slots(c32),
               means2D=g2[:n], conic=gcn[:n], opacities=go[:n].reshape(-1, 1), colors=gcol[:n])
    walk = {k: hg[k] for k in ("means2D", "opacities", "colors")}
    a_ = G.gradient_anchor_stats(dict(walk, conic=og["conic"], **slots(hg)), dict(og, **slots(og)), g64)
    for k in walk:           # (run_case: within the tolerance of the oracle, or no further from float64 than the oracle is)
        assert errs[k] < c.tol or a_[k]["rel_l2_hip"] <= max(c.tol, 1.25 * a_[k]["rel_l2_oracle"]), ("reverse walk", k, errs[k], a_[k])
    _assert_anchored(res, a_, dict(means3D="means3D", scales="cov3D"))


CALL_KINDS = dict(aux=_call_aux, second_pass=_call_second_pass, camera=_call_camera, shs=_call_shs, cov3d=_call_cov3d)
assert tuple(CALL_KINDS) == KINDS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only", type=int, default=None, help="replay one case seed")
    ap.add_argument("--mode", choices=["oracle", "props", "calls"], default="oracle",
                    help="oracle: HIP against the CPU oracle; props: bands / bucket accumulation against the whole view (no oracle); "
                         "calls: aux / second-pass / camera / shs / cov3D calls through the packages, per capacity mode")
    ap.add_argument("--out", default=os.path.join(ROOT, "gpurun_out", "fuzz_parity.jsonl"))
    ap.add_argument("--seconds", type=float, default=1e9, help="stop drawing new cases after this long")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    from oracle import oracle
    oracle.build()
    seeds = [args.only] if args.only is not None else [args.seed * 100000 + i for i in range(args.cases)]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    t0, failed, done = time.time(), [], 0
    with open(args.out, "w") as f:
        for s in seeds:
            if time.time() - t0 > args.seconds:
                break
            t_case = time.time()
            try:
                r = {"oracle": lambda: run_case(oracle, s), "props": lambda: run_props(s), "calls": lambda: run_call(oracle, s)}[args.mode]()
                r["ok"] = True
            except Exception as e:                            # noqa: BLE001 -- a fuzz harness reports everything
                desc = (draw_call if args.mode == "calls" else draw_case)(s)[0]
                r = dict(getattr(e, "partial", None) or desc, ok=False, error=repr(e)[:600], trace=traceback.format_exc()[-1500:])
                failed.append(s)
                print("FAIL", json.dumps(r, default=str)[:1500], flush=True)
            r["seconds"] = round(time.time() - t_case, 2)
            f.write(json.dumps(r, default=str) + "\n")
            f.flush()
            done += 1
    print("fuzz_parity: %d cases, %d failed %s in %.0f s" % (done, len(failed), failed[:20], time.time() - t0))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
