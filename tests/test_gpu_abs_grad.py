"""Absolute screen-space gradients (``set_abs_grad`` / ``GaussianRasterizer(abs_grad=True)`` / ``lograst_backward_abs``):

    absgrad[g, 0] = sum over pixels |dL/dG dG/ddx 0.5 W|,   absgrad[g, 1] = sum over pixels |dL/dG dG/ddy 0.5 H|,   absgrad[g, 2] = 0

summed by the reverse walk next to the signed sums that are dL/dmeans2D, and left on the call's ``means2D`` as ``.absgrad``.

* Against float64: ``tests/absgrad_ref.py`` (a dense restatement of the compositing, pinned on the CPU against
  ``oracle/torch_oracle.render``: tests/test_abs_grad_cpu.py).  Relative L2 of ``absgrad[:, :2]`` <= GRAD_TOL = 1e-4
  (BASELINE.json's gradient tolerance).  A scene is admissible only if the SIGNED dL/dmeans2D of the same backward meets the
  same bound against the same restatement -- asserted in the same test, so that a miss caused by fp32-versus-float64
  contribution decisions shows as the scene's fault.  Row by row, all eleven sums of the abs backward -- slots 9 and 10 are
  the absolute ones -- are held against the oracle's float64 twin by the rule of gpu_util.assert_walk_rows.
* Exact relations, every case: column 2 is zero; rows with radii == 0 or point_weight == 0 are zero; finite and >= 0; and
  |grad[g, c]| <= absgrad[g, c] (1 + 2 H W 2^-24): the triangle inequality plus the worst-case error of an fp32 sum of at
  most H W addends in any order (gamma_n <= n u / (1 - n u) on each side, u = 2^-24; the addends are the same fp32 numbers on
  both sides).
* Same sums in another order (ORDER_TOL = 1e-5 relative L2, as tests/test_gpu_aux_channels.py): the seven ordinary gradients
  of the abs backward against the plain backward of an identical forward in the same walk form; absgrad of the row-split
  form against the quadrant form; absgrad under -dL/dimage against dL/dimage.
* The regimes the reverse walk has, accumulation on one means2D, the refusals, the counter and the depth-pass proxy.

Every case fails on a tree without the feature (no ``abs_grad`` keyword, no ``absgrad`` attribute, no entry point)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import absgrad_ref
import list_cases
from test_gpu_aux_channels import _StandInRenderer
from test_gpu_recomposite import _culled_scene, _lazy_scene, _ragged
from util import rel_l2, small_case

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4     # relative L2 against float64, stated by BASELINE.json
ORDER_TOL = 1e-5    # two device evaluations of the same sums, order of the additions only
DEV = "cuda:0"
BG = (0.25, 0.5, 0.75)
LEAVES = ("xyz", "scaling", "rotation", "opacity", "colors")


def _package(name):
    import diff_gaussian_rasterization as up
    import diff_gaussian_rasterization_wodilate as wo
    return wo if name == "wodilate" else up


def _weights(cam, sign=1.0, constant=False):
    H, W = cam["image_height"], cam["image_width"]
    if constant:
        return np.full((3, H, W), sign, np.float32)
    return (sign * np.random.default_rng(7).standard_normal((3, H, W))).astype(np.float32)


class Run:
    """One forward + backward through the package.  abs_on: the rasterizer object's ``abs_grad`` keyword."""

    def __init__(self, cam, sc, abs_on=True, package="wodilate", form=None, sign=1.0, bg=BG, constant=False, shs=None,
                 pre_grad=False):
        import gpu_util as G
        from log_amd import rasterizer as R
        mod = _package(package)
        dev = torch.device(DEV)
        n = len(sc["xyz"])
        T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
        self.leaves = {k: T(sc[k]) for k in LEAVES}
        L = self.leaves
        self.shs = T(shs) if shs is not None else None
        if pre_grad:     # leaves whose .grad exists already: what the in-place leaf route asks for
            for t in self.leaves.values():
                t.grad = torch.zeros_like(t)
        self.m2 = torch.zeros(n, 3, device=dev, requires_grad=True)
        self.cam, self.w = cam, _weights(cam, sign, constant)
        rs = G.settings(cam, bg, dev)
        if shs is not None:
            rs = rs._replace(sh_degree=1)
        rast = mod.GaussianRasterizer(raster_settings=rs, **({"abs_grad": True} if abs_on else {}))
        kw = dict(means3D=L["xyz"], means2D=self.m2, shs=self.shs, colors_precomp=None if shs is not None else L["colors"],
                  opacities=L["opacity"], scales=L["scaling"], rotations=L["rotation"], cov3D_precomp=None)
        with (R.walk_form(form) if form else contextlib.nullcontext()):
            self.out = rast(**kw)
            self.saved = self.out[0].grad_fn.saved
            (self.out[0] * torch.from_numpy(self.w).to(dev)).sum().backward()
        self.bwd_form = R._backend.last_forms.get("bwd")
        self.conic = R._backend.last_conic_grad.clone().cpu().numpy() if n else np.zeros((0, 4), np.float32)
        torch.cuda.synchronize()
        self.radii = self.out[1].cpu().numpy()
        self.pw = self.out[4].cpu().numpy() if len(self.out) == 5 else None
        self.absgrad = self.m2.absgrad.cpu().numpy() if hasattr(self.m2, "absgrad") else None

    def grads(self):
        g = {k: t.grad.detach().cpu().numpy() for k, t in self.leaves.items() if t.grad is not None}
        g["means2D"] = self.m2.grad.detach().cpu().numpy()
        conic = self.conic.copy()
        if self.pw is not None and len(conic):
            conic[self.pw == 0] = 0          # rows the forward did not clear and the chain rule does not read (touched-only)
        g["conic"] = conic
        if self.shs is not None:
            g["shs"] = self.shs.grad.detach().cpu().numpy()
        return g


def _relations(r):
    """The exact relations of one abs backward."""
    a, g = r.absgrad, r.m2.grad.detach().cpu().numpy()
    H, W = r.cam["image_height"], r.cam["image_width"]
    assert a is not None and a.shape == g.shape and a.dtype == np.float32
    assert not np.any(a[:, 2])
    assert np.isfinite(a).all() and (a >= 0).all()
    dead = r.radii == 0
    if r.pw is not None:
        dead = dead | (r.pw == 0)
    assert not np.any(a[dead])
    slack = 1.0 + 2.0 * H * W * 2.0 ** -24
    assert (np.abs(g[:, :2]).astype(np.float64) <= a[:, :2].astype(np.float64) * slack).all()


def _same(ga, gb, what, tol=ORDER_TOL):
    figures = {}
    for k in ga:
        if np.any(ga[k]) or np.any(gb[k]):
            figures[k] = rel_l2(ga[k], gb[k])
            print("%s %-9s rel L2 %.3g" % (what, k, figures[k]))
    assert all(f < tol for f in figures.values()), {k: f for k, f in figures.items() if not f < tol}
    return figures


def _check(cam, sc, package="wodilate", forms=("rows", "quadrant"), **kw):
    """The abs backward in both walk forms: the exact relations, its seven ordinary gradients against the plain backward of
    an identical forward in the same form, and absgrad form against form.  -> the runs by form."""
    runs = {}
    for form in forms:
        a, p = Run(cam, sc, True, package, form=form, **kw), Run(cam, sc, False, package, form=form, **kw)
        assert a.bwd_form == form and p.bwd_form == form, (a.bwd_form, p.bwd_form)
        assert p.absgrad is None
        for x, y in zip(a.out, p.out):
            assert torch.equal(x, y)
        _relations(a)
        ga, gp = a.grads(), p.grads()
        assert set(ga) == set(gp) and len(ga) >= 7
        _same(ga, gp, "abs vs plain (%s)" % form)
        runs[form] = a
    if len(forms) == 2:
        x, y = runs["rows"].absgrad, runs["quadrant"].absgrad
        if np.any(x) or np.any(y):
            f = rel_l2(x, y)
            print("absgrad rows vs quadrant: rel L2 %.3g" % f)
            assert f < ORDER_TOL, f
    return runs


# ---- against float64 ------------------------------------------------------------------------------------------------------

def _walk_rows(oracle_mod, a, cam, sc, flavour, name):
    """Every row, all eleven slots: |hip - f64| <= 2 |oracle - f64| + WALK_ROW_FLOOR * 6e-8 * unit (gpu_util.walk_row_stats)."""
    import gpu_util as G
    v, of = G.oracle_forward(oracle_mod, cam, sc, BG, flavour=flavour)
    og = oracle_mod.backward(v, of, a.w, abs_sums=True)
    g64 = oracle_mod.backward_f64(v, of, a.w, cond=False, abs_sums=True)
    g = a.grads()
    hg = dict(means2D=g["means2D"], conic=g["conic"], opacities=g["opacity"].reshape(-1, 1), colors=g["colors"], absgrad=a.absgrad[:, :2])
    st = G.walk_row_stats(hg, og, g64)
    assert st["slots"] == 11 and st["live"] > 0
    G.assert_walk_rows(st, name=name)


def _against_float64(cam, sc, package, form, oracle_mod=None, name=None):
    from log_amd import rasterizer as R
    a = Run(cam, sc, True, package, form=form)
    assert a.bwd_form == form
    _relations(a)
    ref = absgrad_ref.of_case(cam, sc, BG, a.w, flavour=R.WODILATE if package == "wodilate" else R.UPSTREAM)
    signed = rel_l2(a.m2.grad.cpu().numpy()[:, :2], ref["signed"])
    absolute = rel_l2(a.absgrad[:, :2], ref["abs"])
    rows = np.linalg.norm(ref["abs"], axis=1) > 0
    worst = float((np.linalg.norm(a.absgrad[rows, :2] - ref["abs"][rows], axis=1) / np.linalg.norm(ref["abs"][rows], axis=1)).max())
    print("%s %s: signed dL/dmeans2D vs float64 %.3g, absgrad vs float64 %.3g, worst row %.3g" % (package, form, signed, absolute, worst))
    assert signed <= GRAD_TOL, ("the scene is not admissible: its signed gradient misses the bound", signed)
    assert absolute <= GRAD_TOL, absolute
    _walk_rows(oracle_mod, a, cam, sc, R.WODILATE if package == "wodilate" else R.UPSTREAM, name)


@pytest.mark.parametrize("form", ["rows", "quadrant"])
@pytest.mark.parametrize("package", ["wodilate", "upstream"])
@pytest.mark.parametrize("shape", [(16, 16), (37, 21), (64, 48)])
def test_against_float64_shapes_both_packages(oracle_mod, shape, package, form):
    W, H = shape
    cam, sc = small_case(n=400, W=W, H=H, focal=1.1 * W, seed=2, smax=0.1)
    _against_float64(cam, sc, package, form, oracle_mod, "abs_%dx%d_%s_%s" % (W, H, package, form))


@pytest.mark.parametrize("form", ["rows", "quadrant"])
def test_against_float64_ragged_scene(oracle_mod, form):
    cam, sc = _ragged()
    _against_float64(cam, sc, "wodilate", form, oracle_mod, "abs_ragged_" + form)


# ---- same sums, another order ---------------------------------------------------------------------------------------------

def test_ordinary_gradients_and_forms_on_the_ragged_scene():
    cam, sc = _ragged()
    _check(cam, sc)


@pytest.mark.parametrize("form", ["rows", "quadrant"])
def test_sign_of_the_image_gradient_does_not_matter(form):
    cam, sc = _ragged()
    a, b = Run(cam, sc, form=form), Run(cam, sc, form=form, sign=-1.0)
    assert np.any(a.absgrad)
    assert rel_l2(b.m2.grad.cpu().numpy(), -a.m2.grad.cpu().numpy()) < ORDER_TOL
    f = rel_l2(b.absgrad, a.absgrad)
    print("absgrad under -dL/dimage vs dL/dimage (%s): rel L2 %.3g" % (form, f))
    assert f < ORDER_TOL


# ---- a cancelling splat ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["rows", "quadrant"])
def test_a_centred_splat_cancels_in_the_signed_sum_only(form):
    """One isotropic Gaussian on the pixel centre (16, 16) of a 32x32 image, dL/dimage constant, black background: the
    per-pixel terms are odd around the centre, the signed sum keeps their rounding only, the absolute sum all of them."""
    cam, sc = absgrad_ref.centred_splat()
    a = Run(cam, sc, form=form, bg=(0.0, 0.0, 0.0), constant=True)
    _relations(a)
    g, ab = a.m2.grad.cpu().numpy()[0], a.absgrad[0]
    print("centred splat (%s): signed %s, absolute %s" % (form, g[:2], ab[:2]))
    assert ab[0] > 0 and ab[1] > 0
    assert abs(g[0]) <= 1e-3 * ab[0] and abs(g[1]) <= 1e-3 * ab[1]
    ref = absgrad_ref.of_case(cam, sc, (0.0, 0.0, 0.0), a.w)
    assert rel_l2(ab[:2], ref["abs"][0]) <= GRAD_TOL


# ---- the regimes of the reverse walk --------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [1, 63, 64, 65, 128, 129])
def test_tile_lists_on_the_chunk_edges(L):
    cam, sc, lens = list_cases.one_tile(L, "spread")
    runs = _check(cam, sc)
    assert lens[list_cases.MAIN_TILE] == L
    assert int(runs["rows"].saved["n_contrib"][16:32, 16:32].max()) == L
    assert np.any(runs["rows"].absgrad)


def test_opaque_stack_saturates_pixels_mid_chunk():
    cam, sc, _ = list_cases.one_tile(200, "spread", front="closed")
    runs = _check(cam, sc)
    deepest = int(runs["quadrant"].saved["n_contrib"][16:32, 16:32].max())
    assert 0 < deepest <= list_cases.N_FRONT, deepest


@pytest.mark.parametrize("lazy", [1, 0])
@pytest.mark.parametrize("kind", ["open", "mixed"])
def test_long_lists_park_and_resume(kind, lazy):
    from log_amd import tune
    cam, sc = _lazy_scene(kind)
    tune.set_knob("LOGRAST_LAZY_SORT", lazy)
    try:
        runs = _check(cam, sc)
    finally:
        tune.reset_knobs()
    assert int(runs["rows"].saved["n_contrib"].max()) > 7680


@pytest.mark.parametrize("masks", [True, False])
def test_hit_masks_on_and_off(masks):
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    prev = R.set_hit_masks(masks)
    try:
        runs = _check(cam, sc)
    finally:
        R.set_hit_masks(prev)
    for form, code in (("rows", 1), ("quadrant", 2)):
        assert (runs[form].saved["hit_masks"] is not None) == masks
        assert runs[form].saved["hit_mask_form"] == (code if masks else 0)


def test_touched_only_regime_at_small_size():
    """LOGRAST_HELPER_MIN_N below n: the compositing kernel clears the accumulator rows it meets (all sixteen slots: 9 and
    10 too) and nobody clears the others; the chain rule skips them and writes zeros."""
    from log_amd import tune
    cam, sc = _ragged()
    tune.set_knob("LOGRAST_HELPER_MIN_N", 1000)
    try:
        _check(cam, sc)
    finally:
        tune.reset_knobs()


def test_empty_input_and_nothing_hit():
    cam, sc = _ragged()
    empty = {k: v[:0] for k, v in sc.items()}
    a = Run(cam, empty)
    assert a.absgrad is not None and a.absgrad.shape == (0, 3)
    for form in ("rows", "quadrant"):
        a = Run(cam, _culled_scene(cam, sc), form=form)
        _relations(a)
        assert a.absgrad.shape == (len(sc["xyz"]), 3) and not np.any(a.absgrad)


@pytest.mark.parametrize("mode", ["speculative", "exact", "fixed"])
def test_capacity_modes(mode):
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    ref = Run(cam, sc)
    n_inst, _, max_len, _ = R.last_state_info(torch.device(DEV))
    prev = R.set_speculative(mode == "speculative")
    if mode == "fixed":
        R.set_instance_capacity(n_inst + 64, max_tile_len=max_len + 64)
    try:
        a = Run(cam, sc)
    finally:
        R.set_instance_capacity(None)
        R.set_speculative(prev)
    _relations(a)
    assert a.bwd_form == ref.bwd_form
    _same(dict(a.grads(), absgrad=a.absgrad), dict(ref.grads(), absgrad=ref.absgrad), "capacity mode %s" % mode)


def test_captured_forward_and_backward_replay_identically():
    """Sync-free mode with a fixed capacity: forward + abs backward captured into a graph and replayed twice.  Every forward
    output has the eager call's bits; the atomically summed outputs lie within the order bound."""
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    dev = torch.device(DEV)
    eager = Run(cam, sc)
    ge = eager.grads()
    n_inst, _, max_len, _ = R.last_state_info(dev)
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
    leaves = {k: T(sc[k]) for k in LEAVES}
    m2 = torch.zeros(len(sc["xyz"]), 3, device=dev, requires_grad=True)
    rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, BG, dev), abs_grad=True)
    w = torch.from_numpy(eager.w).to(dev)
    order = [leaves[k] for k in LEAVES] + [m2]

    def step():
        if hasattr(m2, "absgrad"):
            del m2.absgrad                             # set, not added to: one replay = one backward
        out = rast(means3D=leaves["xyz"], means2D=m2, shs=None, colors_precomp=leaves["colors"], opacities=leaves["opacity"],
                   scales=leaves["scaling"], rotations=leaves["rotation"], cov3D_precomp=None)
        return out, torch.autograd.grad((out[0] * w).sum(), order), m2.absgrad

    R.set_instance_capacity(n_inst + 64, max_tile_len=max_len + 64)
    try:
        stream = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(stream):
            step()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            out, grads, ab = step()
        for _ in range(2):
            for t in tuple(out) + tuple(grads) + (ab,):
                t.detach().zero_()
            g.replay()
            torch.cuda.synchronize()
            for x, y in zip(out, eager.out):
                assert torch.equal(x, y)
            for k, t in zip(LEAVES + ("means2D",), grads):
                assert rel_l2(t.detach().cpu().numpy(), ge[k]) < ORDER_TOL, k
            assert rel_l2(ab.cpu().numpy(), eager.absgrad) < ORDER_TOL
            assert not np.any(ab.cpu().numpy()[:, 2])
        assert not R.overflow_since_reset(dev)["overflowed"]
    finally:
        R.set_instance_capacity(None)


def test_native_sh_colours_at_degree_one():
    cam, sc = small_case(n=300, W=37, H=21, focal=40.0, seed=4, smax=0.1)
    shs = np.random.default_rng(5).standard_normal((300, 4, 3)).astype(np.float32)
    runs = _check(cam, sc, shs=shs)
    assert np.any(runs["rows"].grads()["shs"])


# ---- accumulation on one means2D ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reuse", [False, True])
def test_two_calls_add_on_the_shared_means2d(reuse):
    """Two calls through ONE rasterizer object and ONE means2D (LoG's depth pass): absgrad is set by the first backward and
    added to by the second, as .grad accumulates; geometry reuse (the second call composites the first one's lists) or not."""
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    dev = torch.device(DEV)
    n = len(sc["xyz"])
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
    colors2 = np.random.default_rng(12).random((n, 3)).astype(np.float32)
    w = torch.from_numpy(_weights(cam)).to(dev)

    def calls(which):
        leaves = {k: T(sc[k]) for k in LEAVES}
        c2 = T(colors2)
        m2 = torch.zeros(n, 3, device=dev, requires_grad=True)
        rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, BG, dev), abs_grad=True)
        kw = dict(means3D=leaves["xyz"], means2D=m2, shs=None, opacities=leaves["opacity"], scales=leaves["scaling"],
                  rotations=leaves["rotation"], cov3D_precomp=None)
        R.geometry_reuse_stats(reset=True)
        loss = 0
        if "first" in which:
            loss = loss + (rast(colors_precomp=leaves["colors"], **kw)[0] * w).sum()
        if "second" in which:
            loss = loss + 0.5 * (rast(colors_precomp=c2, **kw)[0] * w).sum()
        stats = R.geometry_reuse_stats()
        loss.backward()
        torch.cuda.synchronize()
        return m2.absgrad.cpu().numpy(), m2.grad.cpu().numpy(), stats

    prev = R.set_geometry_reuse(reuse)
    try:
        both, g_both, stats = calls(("first", "second"))
    finally:
        R.set_geometry_reuse(prev)
    assert stats["reused"] == (1 if reuse else 0), stats
    one, g_one, _ = calls(("first",))
    two, g_two, _ = calls(("second",))
    f = rel_l2(both, one + two)
    print("absgrad of two calls on one means2D vs the two calls' own sums (reuse %s): rel L2 %.3g" % (reuse, f))
    assert f < ORDER_TOL
    assert rel_l2(g_both, g_one + g_two) < ORDER_TOL
    assert not np.any(both[:, 2]) and np.any(two)


# ---- refusals -------------------------------------------------------------------------------------------------------------

def _launches():
    from log_amd import _lib
    return {k: v[1] for k, v in _lib.profile_read().items()}


def test_refused_combinations_raise_before_any_launch():
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import _lib, rasterizer as R
    from log_amd.dist import GradientBucket
    cam, sc = small_case(n=64, W=32, H=32, focal=40.0, seed=1)
    dev = torch.device(DEV)
    T = lambda a, g=False: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=g)
    m3, sca, rot, op, col = T(sc["xyz"], True), T(sc["scaling"]), T(sc["rotation"]), T(sc["opacity"]), T(sc["colors"])
    rs = G.settings(cam, BG, dev)
    kw = dict(means3D=m3, means2D=torch.zeros(64, 3, device=dev, requires_grad=True), shs=None, colors_precomp=col, opacities=op)
    rast = wo.GaussianRasterizer(raster_settings=rs, abs_grad=True)
    bucket = GradientBucket(64, dev, 1, row_major=True)
    rs_cam = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True))
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    _lib.profile_reset()
    try:
        with pytest.raises(ValueError, match="abs_grad cannot be combined with aux_colors"):
            rast(scales=sca, rotations=rot, aux_colors=torch.zeros(64, 3, device=dev), **kw)
        with pytest.raises(ValueError, match="abs_grad cannot be combined with camera gradients"):
            wo.GaussianRasterizer(raster_settings=rs_cam, abs_grad=True)(scales=sca, rotations=rot, **kw)
        with pytest.raises(ValueError, match="abs_grad cannot be combined with cov3D_precomp"):
            rast(cov3D_precomp=torch.eye(3, device=dev).reshape(-1)[[0, 1, 2, 4, 5, 8]].repeat(64, 1), **kw)
        with R.tile_rows(0, 1), pytest.raises(ValueError, match="abs_grad cannot be combined with a tile_rows band"):
            rast(scales=sca, rotations=rot, **kw)
        with R.accumulate_grads_into(bucket.sink()), pytest.raises(ValueError, match="abs_grad cannot be combined with accumulate_grads_into"):
            rast(scales=sca, rotations=rot, **kw)
        assert _launches() == {}
        # a sink that appears between forward and backward is refused by the backward, before its launches
        out = rast(scales=sca, rotations=rot, **kw)
        torch.cuda.synchronize()
        _lib.profile_reset()
        with R.accumulate_grads_into(bucket.sink()), pytest.raises(ValueError, match="accumulate_grads_into"):
            out[0].sum().backward()
        assert _launches() == {}
    finally:
        _lib.profile_enable(False)


def test_inplace_leaf_route_is_not_taken():
    """set_inplace_leaf_grads(True) with leaves that qualify (their .grad exists): a plain call adds into .grad in place, an
    abs call returns fresh gradients that autograd adds -- the same values in .grad either way, and absgrad is there."""
    from log_amd import rasterizer as R
    cam, sc = _ragged()
    prev = R.set_inplace_leaf_grads(True)
    try:
        a, p = Run(cam, sc, True, form="quadrant", pre_grad=True), Run(cam, sc, False, form="quadrant", pre_grad=True)
    finally:
        R.set_inplace_leaf_grads(prev)
    _relations(a)
    assert np.any(a.absgrad) and p.absgrad is None
    _same(a.grads(), p.grads(), "abs vs plain under set_inplace_leaf_grads")


PTR = 0x10000


def test_entry_point_argument_errors_launch_nothing():
    from log_amd import _lib
    L = _lib.lib()

    def view(**over):
        v = _lib.LograstView()
        v.width, v.height, v.tanfovx, v.tanfovy, v.scale_modifier = 64, 64, 0.5, 0.5, 1.0
        v.filter_mode, v.ndc_cull, v.extras = 2, 1, 1
        v.viewmatrix = v.projmatrix = v.bg = PTR
        for k, val in over.items():
            setattr(v, k, val)
        return v

    def call(v, flags=1, out=PTR, n=2000):
        rc = L.lograst_backward_abs(ctypes.byref(v), n, None, *([PTR] * 17), flags, out, None)
        return rc, L.lograst_last_error()

    rows = [(view(tile_row_begin=1, tile_row_end=3), dict(), b"whole images only"),
            (view(cov3d_precomp=PTR, dl_dcov3d=PTR), dict(), b"no cov3d_precomp form"),
            (view(), dict(flags=1 | 2), b"fresh gradients"),
            (view(), dict(flags=1 | 8), b"fresh gradients"),
            (view(), dict(out=None), b"dl_dmeans2d_abs is NULL"),
            (view(), dict(out=None, n=0), b"dl_dmeans2d_abs is NULL"),
            (view(), dict(), b"NULL pointer")]          # passes the abs checks, reaches the common ones (means3d NULL)
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    _lib.profile_reset()
    try:
        for v, kw, fragment in rows:
            rc, msg = call(v, **kw)
            assert rc == -1 and fragment in msg, (rc, msg)
        assert _launches() == {}
    finally:
        _lib.profile_enable(False)


# ---- the counter ----------------------------------------------------------------------------------------------------------

class _StandInRender(_StandInRenderer):
    """The stand-in render's rasterizer call(s), and the keys of LoG/render/renderer.py:154-184 that the counter reads."""

    def render_view(self, rasterizer, camera, leaves, m2, n):
        from log_amd import counter
        seen = []

        def spy(**kw):
            ret = rasterizer(**kw)
            seen.append(ret)
            return ret
        spy.raster_settings = rasterizer.raster_settings
        out = self.render(spy, camera, leaves["xyz"], m2, leaves["colors"], leaves["opacity"], leaves["scaling"], leaves["rotation"])
        ids, counts = counter.unique_ids(seen[0][2], n)
        out.update(viewspace_points=m2, point_id=ids, point_count=counts)
        return out


def _output_dict(abs_on, render_depth=False):
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    cam, sc = _ragged()
    dev = torch.device(DEV)
    n = len(sc["xyz"])
    T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
    leaves = {k: T(sc[k]) for k in LEAVES}
    m2 = torch.zeros(n, 3, device=dev, requires_grad=True)
    camera = {"world_view_transform": torch.tensor(np.asarray(cam["world_view_transform"], np.float32), device=dev)}
    renderer = _StandInRender()
    renderer.render_depth = render_depth
    rast = wo.GaussianRasterizer(raster_settings=G.settings(cam, BG, dev), **({"abs_grad": True} if abs_on else {}))
    view = renderer.render_view(rast, camera, leaves, m2, n)
    (view["render"] * torch.from_numpy(_weights(cam)).to(dev)).sum().backward()
    P = 3 * n
    vis = torch.randperm(P, device=dev, generator=torch.Generator(device=dev).manual_seed(3))[:n]
    return {"render": [view["render"]], "visibility_flag": [{"index": vis}], "viewspace_points": [m2], "radii": [view["radii"]],
            "point_weight": [view["point_weight"]], "point_id": [view["point_id"]], "point_count": [view["point_count"]]}, P


def test_counter_reads_absgrad_where_grad_went():
    import types
    import train_util as U
    from log_amd import counter
    out, P = _output_dict(True)
    m2 = out["viewspace_points"][0]
    assert hasattr(m2, "absgrad") and not torch.equal(m2.absgrad, m2.grad)
    prev = counter.set_abs_grad(True)
    counter.abs_grad_stats(reset=True)
    try:
        c_on = U.fresh_counter(P, DEV)
        counter.update_by_output(c_on, out)
        flag_on = out["visibility_flag"][0]["flag_vis"].clone()
        assert counter.abs_grad_stats() == dict(enabled=True, missing=0)
        # the same function with the switch off, .grad replaced by the absgrad tensor
        counter.set_abs_grad(False)
        c_off = U.fresh_counter(P, DEV)
        swapped = dict(out, viewspace_points=[types.SimpleNamespace(grad=m2.absgrad.clone())],
                       visibility_flag=[{"index": out["visibility_flag"][0]["index"]}])
        counter.update_by_output(c_off, swapped)
        for k in U.COUNTER_DTYPES:
            assert torch.equal(getattr(c_on, k), getattr(c_off, k)), k
        assert torch.equal(flag_on, swapped["visibility_flag"][0]["flag_vis"])
        assert float(c_on.grad_sum.sum()) > 0
        # ... and it is not what the signed gradient gives
        c_signed = U.fresh_counter(P, DEV)
        counter.update_by_output(c_signed, dict(out, visibility_flag=[{"index": out["visibility_flag"][0]["index"]}],
                                                viewspace_points=[types.SimpleNamespace(grad=m2.grad)]))
        assert float(c_on.grad_sum.sum()) > float(c_signed.grad_sum.sum())
        # a tensor without absgrad: .grad, counted
        counter.set_abs_grad(True)
        c_miss = U.fresh_counter(P, DEV)
        counter.update_by_output(c_miss, dict(out, visibility_flag=[{"index": out["visibility_flag"][0]["index"]}],
                                              viewspace_points=[types.SimpleNamespace(grad=m2.grad)]))
        assert counter.abs_grad_stats(reset=True) == dict(enabled=True, missing=1)
        for k in U.COUNTER_DTYPES:
            assert torch.equal(getattr(c_miss, k), getattr(c_signed, k)), k
    finally:
        counter.set_abs_grad(prev)
        counter.abs_grad_stats(reset=True)


# ---- the depth-pass proxy -------------------------------------------------------------------------------------------------

def test_depth_pass_proxy_falls_back_to_two_calls():
    """With abs-grad on the proxy takes no aux path: both rasterizer calls launch, the reason is counted, the outputs are the
    two-call path's bits and the two calls' absolute sums add on the shared means2D."""
    import gpu_util as G
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import depth_pass, rasterizer as R
    cam, sc = _ragged()
    dev = torch.device(DEV)
    camera = {"world_view_transform": torch.tensor(np.asarray(cam["world_view_transform"], np.float32), device=dev)}
    rs = G.settings(cam, BG, dev)
    H, W = cam["image_height"], cam["image_width"]
    rng = np.random.default_rng(9)
    wr, wd = (torch.from_numpy(rng.standard_normal((3, H, W)).astype(np.float32)).to(dev) for _ in range(2))
    results = {}
    for name in ("plain", "wrapped", "switch"):
        T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=True)
        leaves = {k: T(sc[k]) for k in LEAVES}
        m2 = torch.zeros(len(sc["xyz"]), 3, device=dev, requires_grad=True)
        renderer = _StandInRenderer()
        render = _StandInRenderer.render if name == "plain" else depth_pass.wrap_render(_StandInRenderer.render)
        depth_pass.reset_stats()
        R.capacity_stats(reset=True)
        # "switch": the process-wide switch instead of the object's keyword
        rast = wo.GaussianRasterizer(raster_settings=rs, **({} if name == "switch" else {"abs_grad": True}))
        with (R.abs_grad(True) if name == "switch" else contextlib.nullcontext()):
            out = render(renderer, rast, camera, leaves["xyz"], m2, leaves["colors"], leaves["opacity"], leaves["scaling"],
                         leaves["rotation"])
        forwards = R.capacity_stats()["forwards"]
        loss = (out["render"] * wr).sum() + 1e-2 * (torch.cat([out["depth"], out["height"], out["accmap"]]) * wd).sum()
        loss.backward()
        torch.cuda.synchronize()
        results[name] = (out, forwards, m2.absgrad.cpu().numpy(), m2.grad.cpu().numpy(), depth_pass.stats())
    po, pf, pa, pg, _ = results["plain"]
    for name in ("wrapped", "switch"):
        wo_, wf, wa, wg, st = results[name]
        assert pf == 2 and wf == 2, (pf, wf)
        assert st["fused"] == 0 and st["fallback"].get("abs_grad") == 1, st     # (+ the second call's own fall-back reason)
        for k in ("render", "depth", "height", "accmap", "radii", "point_weight"):
            assert torch.equal(wo_[k], po[k]), k
        assert rel_l2(wa, pa) < ORDER_TOL and rel_l2(wg, pg) < ORDER_TOL
    assert np.any(pa) and not np.any(pa[:, 2])
