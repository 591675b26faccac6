"""Restatement of a step over several views, on top of tests/step_ref.py: per view the gradients of get_all's backward on the
rows with radii > 0, summed by model row in view order, then Adam on the rows some view saw.  In float64 it is the reference
value, in float32 the same formulas at the kernels' precision; next to every output comes its condition scale S (step_ref's
rule: every summed term replaced by its magnitude), so that the step kernels' bound applies as it stands:

    |got - ref64| <= 8 * (|ref32 - ref64| + 2^-24 * S)        per element (``within``)
"""
import math
import os

import numpy as np
import torch

import step_ref

KEYS = ("xyz", "scaling", "opacity", "rotation", "colors", "shs")
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "multi_view_log.npz")
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15
FACTOR = 8.0


def load(path=GOLDEN):
    """-> (bufs, exp_avg, exp_avg_sq, views, g): the fixture's model and moments before the step (fp32 tensors), its views as
    dicts (index, index_node, radii, campos, ups), and the file."""
    g = np.load(path)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    keys = [k for k in KEYS if "model_" + k in g]
    bufs = {k: T(g["model_" + k]) for k in keys}
    m1 = {k: T(g["exp_avg_" + k]) for k in keys}
    m2 = {k: T(g["exp_avg_sq_" + k]) for k in keys}
    views = []
    for v in range(int(g["views"])):
        views.append({"index": T(g[f"v{v}_index"]), "index_node": T(g[f"v{v}_index_node"]), "radii": T(g[f"v{v}_radii"]),
                      "campos": T(g[f"v{v}_camera_center"]),
                      "ups": {k: T(g[f"v{v}_up_{k}"].astype(np.float32)) for k in ("xyz", "scaling", "opacity", "rotation", "colors")}})
    return bufs, m1, m2, views, g


def accumulate(bufs, views, degree, dtype=torch.float64):
    """-> (sums, S_sums, seen): per key [P, ...] in `dtype`, the running sums taken in view order."""
    P = bufs["xyz"].shape[0]
    keys = [k for k in bufs if k != "shs" or degree > 0]
    sums = {k: torch.zeros(bufs[k].shape, dtype=dtype) for k in keys}
    S = {k: torch.zeros(bufs[k].shape, dtype=dtype) for k in keys}
    seen = torch.zeros(P, dtype=torch.int32)
    for v in views:
        n = int(v["index"].shape[0])
        index = torch.cat([v["index"], v["index_node"]])
        r = step_ref.get_all(bufs, index, n, degree, v["campos"], v["ups"], dtype=dtype)
        live = (v["radii"][:n] > 0) & (v["index"] >= 0) & (v["index"] < P)
        rows = v["index"][live]
        for k in keys:
            sums[k].index_add_(0, rows, r["grads"][k].detach()[live].to(dtype))
            S[k].index_add_(0, rows, r["S_grads"][k].detach()[live].to(dtype).abs())
        seen.index_add_(0, rows, torch.ones_like(rows, dtype=torch.int32))
    return sums, S, seen


def step(bufs, m1, m2, sums, S_sums, seen, lrs, steps, mmax=None, dtype=torch.float64):
    """Adam at optimizer step `steps` on the rows with seen > 0 -> {key: step_ref.adam's dict for those rows}, rows."""
    rows = torch.nonzero(seen > 0).squeeze(1)
    bc1, bc2 = 1 - BETA1 ** steps, 1 - BETA2 ** steps
    out = {}
    for k in sums:
        out[k] = step_ref.adam(bufs[k][rows], sums[k][rows], m1[k][rows], m2[k][rows], None if mmax is None else mmax[k][rows],
                               lrs[k] / bc1, BETA1, BETA2, math.sqrt(bc2), EPS, S_grad=S_sums[k][rows], dtype=dtype)
    return out, rows


def within(got, ref32, ref64, S, factor=FACTOR):
    """|got - ref64| <= factor * (|ref32 - ref64| + 2^-24 * S) per element -> (ok, the largest ratio error / bound)."""
    got, ref32, ref64, S = (torch.as_tensor(x).double().cpu() for x in (got, ref32, ref64, S))
    err = (got - ref64).abs()
    bound = factor * ((ref32 - ref64).abs() + 2.0 ** -24 * torch.where(torch.isfinite(S), S, torch.zeros_like(S)))
    ok = bool((err <= bound).all()) and not bool(torch.isnan(got).any())
    return ok, float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


def check_against_fixture(sums_rows, stepped, g, refs=None):
    """sums_rows: {key: the sums of the fixture's rows}; stepped: {key: (param, exp_avg, exp_avg_sq) of those rows} -- both
    held to the float64 restatement within the bound, the fixture being ref32's stand-in as well as `got`'s yardstick.
    -> the largest ratio seen."""
    bufs, m1, m2, views, _ = load()
    if refs is None:
        refs = reference(bufs, m1, m2, views, g)
    (s64, S64, seen64, a64, rows), (s32, _, _, a32, _) = refs
    worst = 0.0
    for k in s64:
        ok, ratio = within(sums_rows[k], s32[k][rows], s64[k][rows], S64[k][rows])
        assert ok, ("sum", k, ratio)
        worst = max(worst, ratio)
        for got, name in zip(stepped[k], ("param", "exp_avg", "exp_avg_sq")):
            ok, ratio = within(got, a32[k][name], a64[k][name], a64[k]["S_" + name])
            assert ok, (name, k, ratio)
            worst = max(worst, ratio)
    return worst


def reference(bufs, m1, m2, views, g):
    """The restatement on the fixture's inputs in float64 and float32 -> ((sums, S, seen, adam, rows) per dtype)."""
    out = []
    lrs = {k: float(g["lr_" + k]) for k in bufs}
    for dtype in (torch.float64, torch.float32):
        sums, S, seen = accumulate(bufs, views, int(g["degree"]), dtype)
        a, rows = step(bufs, m1, m2, sums, S, seen, lrs, int(g["step"]), dtype=dtype)
        out.append((sums, S, seen, a, rows))
    return tuple(out)
