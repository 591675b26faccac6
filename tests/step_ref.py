"""Plain-torch restatement of the step operations around the rasterizer, written from the formulas in the header comments
of log_amd/csrc/sh.hip and counter.hip (and the public real-SH polynomials), not from the kernels' code:

    get_all      rows = index ++ index_node;  scaling = exp(s), opacity = 1 / (1 + exp(-o)), rotation = q / max(|q|, 1e-12),
                 colour = 0.5 + C0 dc + sum_{k=1}^{(deg+1)^2-1} Y_k(d) shs_{k-1},  d = (xyz - campos) / |xyz - campos| with
                 xyz DETACHED; gradients (autograd) go to the first n_param rows only
    native SH    oracle/torch_oracle.sh_colors: max(0, 0.5 + sum_k Y_k(d) sh_k), the clamp cutting the gradient
    Adam         m = g (1-b1) + m b1;  v = (1-b2) g g + v b2;  denom = sqrt(amsgrad ? max(vmax, v) : v) / sqrt(bc2) + eps;
                 p = p - step_size * m / denom, on the rows index[flag_vis]
    fused step   get_all's backward followed by Adam on the rows with radii > 0

Every function takes a dtype: float64 is the reference value, float32 the same formulas at the kernels' precision (the
yardstick for what a second fp32 evaluation may differ by).  Next to every output it returns a CONDITION SCALE S of the
same shape: the same expression with every summed term replaced by its absolute value (|value| where nothing is summed),
so that 2^-24 * S is what one fp32 rounding per term costs, cancellations included."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import torch_oracle  # noqa: E402

C0, C1 = 0.28209479177387814, 0.4886025119029199
_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435]
# Y_k as sums of monomials (coefficient, power of x, of y, of z); Y_0 = C0
SH_TERMS = [
    [(C0, 0, 0, 0)],
    [(-C1, 0, 1, 0)], [(C1, 0, 0, 1)], [(-C1, 1, 0, 0)],
    [(_C2[0], 1, 1, 0)], [(_C2[1], 0, 1, 1)], [(2 * _C2[2], 0, 0, 2), (-_C2[2], 2, 0, 0), (-_C2[2], 0, 2, 0)],
    [(_C2[3], 1, 0, 1)], [(_C2[4], 2, 0, 0), (-_C2[4], 0, 2, 0)],
    [(3 * _C3[0], 2, 1, 0), (-_C3[0], 0, 3, 0)], [(_C3[1], 1, 1, 1)],
    [(4 * _C3[2], 0, 1, 2), (-_C3[2], 2, 1, 0), (-_C3[2], 0, 3, 0)],
    [(2 * _C3[3], 0, 0, 3), (-3 * _C3[3], 2, 0, 1), (-3 * _C3[3], 0, 2, 1)],
    [(4 * _C3[4], 1, 0, 2), (-_C3[4], 3, 0, 0), (-_C3[4], 1, 2, 0)],
    [(_C3[5], 2, 0, 1), (-_C3[5], 0, 2, 1)], [(_C3[6], 3, 0, 0), (-3 * _C3[6], 1, 2, 0)],
]


def _poly(terms, d, absolute, wrt=None):
    """sum of c x^a y^b z^c over `terms` at d[..., 3]; wrt = 0 / 1 / 2: its partial derivative with respect to that
    component.  absolute: the condition scale, the sum of (a + b + c) |c| |x|^a |y|^b |z|^c -- a component of d = v / |v| is
    itself computed (S_d = |d|: nothing in it cancels), and a product of p computed factors carries p times its value
    (S(a b) = S_a |b| + |a| S_b, the rule stated at step_ref.adam)."""
    out = torch.zeros(d.shape[:-1], dtype=d.dtype, device=d.device)
    v = d.abs() if absolute else d
    for c, *pw in terms:
        if wrt is not None:
            if pw[wrt] == 0:
                continue
            c, pw = c * pw[wrt], [p - (1 if a == wrt else 0) for a, p in enumerate(pw)]
        w = abs(c) * max(1, sum(pw)) if absolute else c
        out = out + w * v[..., 0] ** pw[0] * v[..., 1] ** pw[1] * v[..., 2] ** pw[2]
    return out


def sh_basis(d, nk, absolute=False, wrt=None):
    """[..., nk]: Y_0 .. Y_{nk-1} at the unit directions d (absolute / wrt: see _poly)."""
    return torch.stack([_poly(SH_TERMS[k], d, absolute, wrt) for k in range(nk)], dim=-1)


def direction(xyz, campos):
    v = xyz - campos[None]
    n = v.norm(dim=-1, keepdim=True)
    return v / n, n


# ---- get_all --------------------------------------------------------------------------------------------------------
def get_all(*args, **kwargs):
    with torch.enable_grad():             # (also when called from inside a backward or a no_grad block)
        return _get_all(*args, **kwargs)


def _get_all(bufs, index, n_param, degree, campos, ups=None, dtype=torch.float64):
    """bufs: xyz[P,3] scaling[P,3] opacity[P,1] rotation[P,4] colors[P,3] (shs[P,K,3]); index int64[n] = index ++ index_node
    (a row outside [0, P) reads row 0); ups: dL/d(activated) per key, or None for the forward alone.
    -> dict(raw, act, S_act[, grads, S_grads]): grads / S_grads are those of the first n_param raw rows (shs only when
    degree > 0, as the reference leaves unused coefficients without gradient)."""
    P = bufs["xyz"].shape[0]
    idx = torch.where((index >= 0) & (index < P), index, torch.zeros_like(index))
    raw = {k: v[idx] for k, v in bufs.items()}
    leaf = {k: v[:n_param].to(dtype).clone().requires_grad_(True) for k, v in raw.items()}
    full = {k: torch.cat([leaf[k], raw[k][n_param:].to(dtype)]) for k in raw}
    K = full["shs"].shape[1] if "shs" in full else 0
    nk = min((degree + 1) ** 2, K + 1)
    act, S = {"xyz": full["xyz"]}, {"xyz": full["xyz"].detach().abs()}
    act["scaling"] = torch.exp(full["scaling"])
    act["opacity"] = torch.sigmoid(full["opacity"])     # (1 / (1 + exp(-o)) written out has a 0 * inf backward in fp32 at o = -100)
    qn = full["rotation"].norm(dim=-1, keepdim=True).clamp_min(1e-12)
    act["rotation"] = full["rotation"] / qn
    col = 0.5 + C0 * full["colors"]
    S_col = 0.5 + C0 * full["colors"].detach().abs()
    d = None
    if degree > 0 and nk > 1:
        d, _ = direction(full["xyz"].detach(), campos.to(dtype))
        Y, Ya = sh_basis(d, nk), sh_basis(d, nk, absolute=True)
        col = col + (Y[:, 1:, None] * full["shs"][:, :nk - 1]).sum(dim=1)
        S_col = S_col + (Ya[:, 1:, None] * full["shs"][:, :nk - 1].detach().abs()).sum(dim=1)
    act["colors"] = col
    for k in ("scaling", "opacity", "rotation"):
        S[k] = act[k].detach().abs()
    S["colors"] = S_col
    out = dict(raw=raw, act={k: v.detach() for k, v in act.items()}, S_act=S)
    if ups is None:
        return out
    u = {k: ups[k].to(dtype) for k in act}
    sum((act[k] * u[k]).sum() for k in act).backward()
    n = n_param
    grads = {k: leaf[k].grad for k in leaf if k != "shs" or degree > 0}
    if "shs" in grads and grads["shs"] is None:
        grads["shs"] = torch.zeros_like(leaf["shs"])
    sg = out["act"]["opacity"][:n]
    q, y, gq = leaf["rotation"].detach(), out["act"]["rotation"][:n], u["rotation"][:n]
    qn = q.norm(dim=-1, keepdim=True)
    S_rot = torch.where(qn > 1e-12, (gq.abs() + y.abs() * (y * gq).abs().sum(dim=-1, keepdim=True)) / qn, gq.abs() * 1e12)
    Sg = {"xyz": u["xyz"][:n].abs(), "scaling": (u["scaling"][:n] * out["act"]["scaling"][:n]).abs(),
          "opacity": u["opacity"][:n].abs() * sg * (1.0 + sg), "rotation": S_rot, "colors": u["colors"][:n].abs() * C0}
    if "shs" in grads:
        Sg["shs"] = torch.zeros_like(leaf["shs"])
        if d is not None:
            Sg["shs"][:, :nk - 1] = sh_basis(d[:n], nk, absolute=True)[:, 1:, None] * u["colors"][:n, None, :].abs()
    out.update(grads=grads, S_grads=Sg)
    return out


# ---- native SH (the packages' shs= input) ---------------------------------------------------------------------------
def native_sh(*args, **kwargs):
    with torch.enable_grad():
        return _native_sh(*args, **kwargs)


def _native_sh(means3D, campos, shs, degree, g_colors=None, clamped=None, dtype=torch.float64):
    """-> dict(colors, pre (the colour before the clamp), clamped, S_colors[, g_shs, g_means3D, S_g_shs, S_g_means3D]).
    clamped (bool[N,3]): the mask the backward is given (the kernels' backward takes the forward's mask as an input); default:
    this evaluation's own."""
    m = means3D.to(dtype).clone().requires_grad_(True)
    s = shs.to(dtype).clone().requires_grad_(True)
    cp = campos.to(dtype)
    nk = (degree + 1) ** 2
    colors = torch_oracle.sh_colors(m, cp, s, degree)
    d, n = direction(m, cp)
    pre = 0.5 + (sh_basis(d, nk)[:, :, None] * s[:, :nk]).sum(dim=1)          # sh_colors before its clamp_min
    Ya = sh_basis(d.detach(), nk, absolute=True)
    out = dict(colors=colors.detach(), pre=pre.detach(), clamped=pre.detach() < 0,
               S_colors=0.5 + (Ya[:, :, None] * s.detach()[:, :nk].abs()).sum(dim=1))
    if g_colors is None:
        return out
    mask = out["clamped"] if clamped is None else clamped.bool()
    ge = torch.where(mask, torch.zeros_like(pre), g_colors.to(dtype))
    (pre * ge).sum().backward()
    d, n = d.detach(), n.detach()
    S_shs = torch.zeros_like(s.detach())
    S_shs[:, :nk] = Ya[:, :, None] * ge[:, None, :].abs()
    # dL/dd_a = sum_k dY_k/da (sh_k . g);  dL/dv = (dL/dd - d (d . dL/dd)) / |v|
    t = (s.detach()[:, :nk].abs() * ge[:, None, :].abs()).sum(dim=-1)
    S_gd = torch.stack([(sh_basis(d, nk, absolute=True, wrt=a) * t).sum(dim=-1) for a in range(3)], dim=-1)
    S_gm = (S_gd + d.abs() * (d.abs() * S_gd).sum(dim=-1, keepdim=True)) / n
    out.update(g_shs=s.grad, g_means3D=m.grad if m.grad is not None else torch.zeros_like(m.detach()),
               S_g_shs=S_shs, S_g_means3D=S_gm)
    return out


# ---- Adam -----------------------------------------------------------------------------------------------------------
def adam(param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, step_size, beta1, beta2, bc2_sqrt, eps, S_grad=None,
         dtype=torch.float64):
    """_single_tensor_adam on already selected rows (all tensors the same shape; max_exp_avg_sq None: no amsgrad).
    -> dict(param, exp_avg, exp_avg_sq[, max_exp_avg_sq]) and the same keys with an S_ prefix.
    S_grad: the condition scale of a gradient that was itself computed (the fused step); an input gradient is exact.  A
    computed factor carries its scale through a product, a root and a quotient to first order -- S(a b) = S_a |b| + |a| S_b,
    S(sqrt a) = S_a / (2 sqrt a), S(a / b) = S_a / |b| + |a| S_b / b^2 -- which for an exact g leaves S(g g) = g g."""
    p, g, m0, v0 = (t.to(dtype) for t in (param, grad, exp_avg, exp_avg_sq))
    m = g * (1 - beta1) + m0 * beta1
    v = (1 - beta2) * g * g + v0 * beta2
    if S_grad is None:
        S_m = g.abs() * (1 - beta1) + m0.abs() * beta1
        S_v = (1 - beta2) * g * g + v0.abs() * beta2
    else:
        Sg = S_grad.to(dtype)
        S_m = Sg * (1 - beta1) + m0.abs() * beta1
        S_v = (1 - beta2) * 2 * Sg * g.abs() + v0.abs() * beta2
    out = dict(exp_avg=m, exp_avg_sq=v, S_exp_avg=S_m, S_exp_avg_sq=S_v)
    vd, S_vd = v, S_v
    if max_exp_avg_sq is not None:
        vm = max_exp_avg_sq.to(dtype)
        vd = torch.maximum(vm, v)                   # (torch.maximum hands a NaN on, as the reference's does)
        S_vd = torch.maximum(vm.abs(), S_v)
        out.update(max_exp_avg_sq=vd, S_max_exp_avg_sq=S_vd)
    root = torch.sqrt(vd)
    S_root = torch.where(S_vd > 0, S_vd / (2 * root), torch.zeros_like(root))
    denom = root / bc2_sqrt + eps
    S_denom = S_root / bc2_sqrt + eps
    out["param"] = p - step_size * (m / denom)
    out["S_param"] = p.abs() + step_size * (S_m / denom + m.abs() * S_denom / (denom * denom))
    return out


# ---- the restatement behind the drop-ins' backend interface ----------------------------------------------------------
class StepRefBackend:
    """gather_activate / activate_backward / sparse_adam of log_amd.rasterizer's backend, computed by the functions above in
    `dtype` and handed back as fp32: lets the drop-ins' own tests (the reference's recorded results, their assertions and
    tolerances) run on the restatement.  Everything else is inherited from the oracle test double at install time."""

    def __init__(self, base=None, dtype=torch.float64):
        self.base, self.dtype = base, dtype

    def __getattr__(self, name):
        return getattr(self.base, name)

    def gather_activate(self, index, bufs, degree, campos):
        r = get_all(bufs, index, 0, degree, campos, dtype=self.dtype)
        raw = {k: v.clone() for k, v in r["raw"].items()}
        act = {k: v.to(torch.float32) for k, v in r["act"].items()}
        act["xyz"] = raw["xyz"]
        return raw, act

    def activate_backward(self, raw, n, degree, campos, g_scaling, g_opacity, g_rotation, g_colors):
        rows = raw["xyz"].shape[0]
        ups = {"xyz": torch.zeros(rows, 3), "scaling": g_scaling, "opacity": g_opacity.reshape(rows, 1),
               "rotation": g_rotation, "colors": g_colors}
        r = get_all(raw, torch.arange(rows), n, degree, campos, ups, dtype=self.dtype)
        return {k: v.to(torch.float32) for k, v in r["grads"].items() if k != "xyz"}

    def sparse_adam(self, index, flag_vis, entries, beta1, beta2, bias_correction2_sqrt, eps):
        vis = flag_vis.bool()
        rows = index[vis]
        for model_p, param, grad, m1, m2, mmax, step_size in entries:
            r = adam(param[vis], grad[vis], m1[rows], m2[rows], None if mmax is None else mmax[rows], step_size, beta1,
                     beta2, bias_correction2_sqrt, eps, dtype=self.dtype)
            model_p[rows], m1[rows], m2[rows] = (r[k].to(torch.float32) for k in ("param", "exp_avg", "exp_avg_sq"))
            if mmax is not None:
                mmax[rows] = r["max_exp_avg_sq"].to(torch.float32)
