"""Absolute screen-space gradients without a GPU.

1. The float64 restatement of the GPU tests (tests/absgrad_ref.py) pins itself: its SIGNED sums equal the means2D gradient
   of ``oracle/torch_oracle.render`` on the same inputs within 1e-12 relative, on every scene of the GPU tests' float64
   comparison; its absolute sums dominate them; the centred splat of the cancelling test leaves less than 1e-4 of the
   absolute sum in the signed one.
2. ``lograst_backward_abs`` refuses what has no abs form before any device work.
3. The Python layer against a stub backend (the CPU oracle backend plus a ``backward_abs`` that returns marked values): the
   switch, the context manager and the constructor keyword; set-then-add on ``means2D.absgrad``; every refused combination;
   with the switch off the autograd function and the backend get exactly today's arguments.
4. ``log_amd.counter``'s switch, ``log_amd.depth_pass``'s reason, ``install_all(abs_grad=True)`` / ``uninstall_abs_grad()``."""
import contextlib
import ctypes
import types

import numpy as np
import pytest
import torch

import absgrad_ref
from util import cam_tan, rel_l2, small_case

PIN_TOL = 1e-12
BG = (0.25, 0.5, 0.75)


def _scenes():
    out = {"%dx%d" % (W, H): (lambda W=W, H=H: small_case(n=400, W=W, H=H, focal=1.1 * W, seed=2, smax=0.1))
           for W, H in ((16, 16), (37, 21), (64, 48))}
    out["ragged"] = lambda: small_case(n=2000, W=150, H=97, focal=170.0, seed=3, smax=0.08)   # test_gpu_recomposite._ragged
    return out


@pytest.mark.parametrize("flavour", ["wodilate", "upstream"])
@pytest.mark.parametrize("name", list(_scenes()))
def test_restatement_reproduces_the_oracle_means2d_gradient(name, flavour):
    from log_amd import rasterizer as R
    cam, sc = _scenes()[name]()
    fl = R.WODILATE if flavour == "wodilate" else R.UPSTREAM
    H, W = cam["image_height"], cam["image_width"]
    w = np.random.default_rng(7).standard_normal((3, H, W)).astype(np.float32)
    ref = absgrad_ref.of_case(cam, sc, BG, w, flavour=fl)
    tfx, tfy = cam_tan(cam)
    g, image = absgrad_ref.render_means2d_grad(W, H, tfx, tfy, cam["world_view_transform"], cam["full_proj_transform"], BG,
                                               sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], sc["colors"], w,
                                               filter_mode=fl.filter_mode, ndc_cull=bool(fl.ndc_cull))
    f = rel_l2(ref["signed"], g)
    print("%s %s: signed sums vs torch_oracle.render's dL/dmeans2D: rel L2 %.3g" % (name, flavour, f))
    assert f <= PIN_TOL
    assert np.array_equal(ref["image"], image)
    assert np.linalg.norm(g) > 0
    assert (np.abs(ref["signed"]) <= ref["abs"] * (1 + 1e-12)).all()
    assert not np.any(ref["abs"][ref["radii"] == 0])


def test_centred_splat_cancels_in_float64():
    cam, sc = absgrad_ref.centred_splat()
    ref = absgrad_ref.of_case(cam, sc, (0.0, 0.0, 0.0), np.ones((3, 32, 32), np.float32))
    assert (ref["abs"][0] > 0).all()
    assert (np.abs(ref["signed"][0]) < 1e-4 * ref["abs"][0]).all(), (ref["signed"], ref["abs"])


# ---- the C entry point -------------------------------------------------------------------------------------------------

PTR = 0x10000                                                # never dereferenced; 64-byte aligned


def _view(**over):
    from log_amd import _lib
    v = _lib.LograstView()
    v.width, v.height, v.tanfovx, v.tanfovy, v.scale_modifier = 64, 64, 0.5, 0.5, 1.0
    v.filter_mode, v.ndc_cull, v.extras = 2, 1, 1
    v.viewmatrix = v.projmatrix = v.bg = PTR
    for k, val in over.items():
        setattr(v, k, val)
    return v


REFUSED = [
    ("band view", dict(tile_row_begin=1, tile_row_end=3), dict(), b"whole images only"),
    ("cov3d_precomp", dict(cov3d_precomp=PTR, dl_dcov3d=PTR), dict(), b"no cov3d_precomp form"),
    ("running sums", dict(), dict(flags=1 | 2), b"fresh gradients"),
    ("row-major running sums", dict(), dict(flags=1 | 8), b"fresh gradients"),
    ("output NULL", dict(), dict(out=None), b"dl_dmeans2d_abs is NULL"),
    ("output NULL, n = 0", dict(), dict(out=None, n=0), b"dl_dmeans2d_abs is NULL"),
    ("passes the abs checks", dict(), dict(), b"NULL pointer"),          # means3d NULL: the common checks are reached
]


@pytest.mark.parametrize("row", REFUSED, ids=[r[0] for r in REFUSED])
def test_backward_abs_refuses_before_any_launch(row):
    from log_amd import _lib
    L = _lib.lib()
    _, view_over, arg, fragment = row
    rc = L.lograst_backward_abs(ctypes.byref(_view(**view_over)), arg.get("n", 2000), None, *([PTR] * 17), arg.get("flags", 1),
                                arg.get("out", PTR), None)
    assert rc == -1 and fragment in L.lograst_last_error(), (rc, L.lograst_last_error())


def test_additions_within_version_4():
    from log_amd import _lib
    L = _lib.lib()
    assert L.lograst_version() == 4 and L.lograst_knob_count() == 22 and _lib.NUM_KERNEL_SLOTS == 23
    assert "lograst_backward_abs" in _lib.EXPORTS


# ---- the Python layer against a stub backend ---------------------------------------------------------------------------

def _stub_backend():
    import oracle_backend

    class Stub(oracle_backend.OracleBackend):
        """The oracle backend + backward_abs: the plain backward's six gradients, then |dL/dmeans2D| + 1 in columns 0, 1."""

        def __init__(self):
            self.calls = []

        def forward(self, *a, **k):
            self.calls.append("forward")
            return super().forward(*a, **k)

        def backward(self, *a, **k):
            self.calls.append("backward")
            return super().backward(*a, **k)

        def backward_abs(self, rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image):
            self.calls.append("backward_abs")
            g = oracle_backend.OracleBackend.backward(self, rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image)
            ab = g[1].abs() + 1.0
            ab[:, 2] = 0
            return g + (ab,)

        def forward_aux(self, *a, **k):
            pytest.fail("forward_aux was called")

        def backward_aux(self, *a, **k):
            pytest.fail("backward_aux was called")

        def backward_camera(self, *a, **k):
            pytest.fail("backward_camera was called")
    return Stub()


@pytest.fixture
def stub(oracle_mod):
    import oracle_backend
    from log_amd import rasterizer as R
    s = _stub_backend()
    old = oracle_backend.install(s)
    yield s
    oracle_backend.install(old)
    R.set_abs_grad(False)


def _call(package="wodilate", grad_v=False, ctor=None, **extra):
    import diff_gaussian_rasterization as up
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    cam, sc = small_case(n=60, W=32, H=32, focal=40.0, seed=1)
    tfx, tfy = cam_tan(cam)
    t = torch.tensor
    V = t(cam["world_view_transform"], requires_grad=grad_v)
    rs = R.GaussianRasterizationSettings(cam["image_height"], cam["image_width"], tfx, tfy, t(BG), 1.0, V,
                                         t(cam["full_proj_transform"]), 0, t(cam["camera_center"]), False, False)
    n = len(sc["xyz"])
    kw = dict(means3D=t(sc["xyz"], requires_grad=True), means2D=torch.zeros(n, 3, requires_grad=True), shs=None,
              colors_precomp=t(sc["colors"], requires_grad=True), opacities=t(sc["opacity"]), scales=t(sc["scaling"]),
              rotations=t(sc["rotation"]), cov3D_precomp=None)
    kw.update(extra)
    mod = wo if package == "wodilate" else up
    return mod.GaussianRasterizer(raster_settings=rs, **(ctor or {})), kw


@pytest.mark.parametrize("package", ["wodilate", "upstream"])
@pytest.mark.parametrize("how", ["constructor", "switch", "context"])
def test_the_three_ways_to_switch_it_on(stub, how, package):
    from log_amd import rasterizer as R
    rast, kw = _call(package, ctor=dict(abs_grad=True) if how == "constructor" else None)
    assert R.set_abs_grad(False) is False                     # the default is off
    if how == "switch":
        assert R.set_abs_grad(True) is False
    with (R.abs_grad(True) if how == "context" else contextlib.nullcontext()):
        out = rast(**kw)
    assert R.set_abs_grad(False) is (how == "switch")
    out[0].sum().backward()
    assert stub.calls == ["forward", "backward_abs"]
    m2 = kw["means2D"]
    assert m2.absgrad.dtype == torch.float32 and m2.absgrad.shape == (60, 3) and m2.absgrad.device == m2.device
    assert torch.equal(m2.absgrad[:, :2], m2.grad[:, :2].abs() + 1.0) and not m2.absgrad[:, 2].any()
    assert kw["means3D"].grad is not None and kw["colors_precomp"].grad is not None


def test_off_is_todays_call(stub, monkeypatch):
    from log_amd import rasterizer as R
    seen = []
    apply = R._RasterizeGaussians.apply
    monkeypatch.setattr(R._RasterizeGaussians, "apply", staticmethod(lambda *a: seen.append(len(a)) or apply(*a)))
    for ctor, ctx in ((None, contextlib.nullcontext()), (dict(abs_grad=False), R.abs_grad(True)), (None, R.abs_grad(False))):
        rast, kw = _call(ctor=ctor)
        with ctx:
            out = rast(**kw)
        out[0].sum().backward()
        assert not hasattr(kw["means2D"], "absgrad")
        assert not hasattr(out[0].grad_fn, "abs_target")
    assert seen == [13, 13, 13]                               # nothing behind aux_colors
    assert stub.calls == ["forward", "backward"] * 3
    # on: one more argument, and under no_grad none
    rast, kw = _call(ctor=dict(abs_grad=True))
    rast(**kw)
    with torch.no_grad():
        rast(**kw)
    assert seen[3:] == [14, 13]


def test_the_object_keyword_overrides_the_switch_both_ways(stub):
    from log_amd import rasterizer as R
    R.set_abs_grad(True)
    try:
        rast, kw = _call(ctor=dict(abs_grad=False))
        rast(**kw)[0].sum().backward()
        assert not hasattr(kw["means2D"], "absgrad")
        with R.abs_grad(False):                               # the thread's block overrides the process-wide switch
            rast, kw = _call()
            rast(**kw)[0].sum().backward()
        assert not hasattr(kw["means2D"], "absgrad")
        rast, kw = _call()
        rast(**kw)[0].sum().backward()
        assert hasattr(kw["means2D"], "absgrad")
    finally:
        R.set_abs_grad(False)


def test_absgrad_is_set_then_added_to(stub):
    rast, kw = _call(ctor=dict(abs_grad=True))
    rast(**kw)[0].sum().backward()
    m2 = kw["means2D"]
    first, g1 = m2.absgrad, m2.grad.clone()
    want = first.clone()
    kw2 = dict(kw, colors_precomp=kw["colors_precomp"].detach() * 0.5)
    rast(**kw2)[0].sum().backward()                           # the same means2D object: added in place, as .grad is
    assert m2.absgrad is first
    g2 = m2.grad - g1
    second = g2.abs() + 1.0
    second[:, 2] = 0
    assert torch.allclose(m2.absgrad, want + second, rtol=0, atol=1e-6)
    assert not m2.absgrad.requires_grad


def test_no_image_gradient_leaves_no_absgrad(stub):
    rast, kw = _call(ctor=dict(abs_grad=True))
    out = rast(**kw)
    (out[0].detach().sum() + kw["means3D"].sum()).backward()
    assert not hasattr(kw["means2D"], "absgrad") and stub.calls == ["forward"]


def test_refused_combinations_raise_before_any_backend_call(stub):
    from log_amd import rasterizer as R
    n = 60
    sink = {k: torch.zeros(n, w) for k, w in (("means3D", 3), ("scales", 3), ("rotations", 4), ("opacities", 1), ("colors", 3))}
    rows = [
        (contextlib.nullcontext(), dict(), dict(aux_colors=torch.zeros(n, 3)), "aux_colors"),
        (contextlib.nullcontext(), dict(grad_v=True), dict(), "camera gradients"),
        (contextlib.nullcontext(), dict(), dict(scales=None, rotations=None, cov3D_precomp=torch.ones(n, 6)), "cov3D_precomp"),
        (R.tile_rows(0, 1), dict(), dict(), "a tile_rows band"),
        (R.accumulate_grads_into(sink), dict(), dict(), "accumulate_grads_into"),
    ]
    for ctx, call_kw, extra, fragment in rows:
        rast, kw = _call(ctor=dict(abs_grad=True), **call_kw, **extra)
        with ctx, pytest.raises(ValueError, match="abs_grad cannot be combined with " + fragment):
            rast(**kw)
    assert stub.calls == []
    # a sink that appears between forward and backward
    rast, kw = _call(ctor=dict(abs_grad=True))
    out = rast(**kw)
    with R.accumulate_grads_into(sink), pytest.raises(ValueError, match="abs_grad cannot be combined with accumulate_grads_into"):
        out[0].sum().backward()
    assert stub.calls == ["forward"]


def test_the_backends_own_list_of_refusals():
    """HipBackend.backward(_abs=True) holds the same list (a caller of the backend, not of autograd)."""
    from log_amd import rasterizer as R
    for kw, fragment in ((dict(sink=True), "accumulate_grads_into"), (dict(cov3D=True), "cov3D_precomp"), (dict(band=True), "tile_rows"),
                         (dict(aux=True), "aux_colors"), (dict(camera=True), "camera gradients")):
        with pytest.raises(ValueError, match=fragment):
            R._refuse_abs_grad_with(**kw)
    R._refuse_abs_grad_with()


def test_a_backend_without_the_method_raises(oracle_mod):
    import oracle_backend
    from log_amd import _lib
    old = oracle_backend.install(oracle_backend.OracleBackend())
    try:
        rast, kw = _call(ctor=dict(abs_grad=True))
        with pytest.raises(_lib.LograstError, match="this backend has no backward_abs"):
            rast(**kw)
    finally:
        oracle_backend.install(old)


def test_native_shs_is_allowed(stub):
    rast, kw = _call(ctor=dict(abs_grad=True))
    shs = torch.randn(60, 1, 3, generator=torch.Generator().manual_seed(0)).requires_grad_(True)
    rast(**dict(kw, colors_precomp=None, shs=shs))[0].sum().backward()
    assert hasattr(kw["means2D"], "absgrad") and shs.grad is not None


# ---- the LoG side ------------------------------------------------------------------------------------------------------

def test_counter_switch_hands_absgrad_to_the_backend(monkeypatch, caplog):
    from log_amd import counter, rasterizer as R
    seen = []

    class Backend:
        def counter_update(self, buffers, visible_index, grad, *rest):
            seen.append(grad)
            return torch.zeros(len(visible_index), dtype=torch.bool)
    monkeypatch.setattr(R, "_backend", Backend())
    c = types.SimpleNamespace(**{k: torch.zeros(4) for k in counter.COUNTER_BUFFERS})
    g, a = torch.ones(3, 3), torch.full((3, 3), 2.0)
    view = lambda **kw: {"render": [None], "visibility_flag": [{"index": torch.arange(3)}],
                         "viewspace_points": [types.SimpleNamespace(**kw)], "radii": [None], "point_weight": [torch.zeros(3)],
                         "point_id": [None], "point_count": [None]}
    assert counter.set_abs_grad(False) is False and counter.abs_grad_stats(reset=True)["enabled"] is False
    counter.update_by_output(c, view(grad=g, absgrad=a))
    assert seen[-1] is g                                      # off: .grad, whatever else the tensor carries
    assert counter.set_abs_grad(True) is False
    try:
        counter.update_by_output(c, view(grad=g, absgrad=a))
        assert seen[-1] is a and counter.abs_grad_stats() == dict(enabled=True, missing=0)
        with caplog.at_level("WARNING", logger="log_amd"):
            counter.update_by_output(c, view(grad=g))
            counter.update_by_output(c, view(grad=g))
        assert seen[-1] is g and counter.abs_grad_stats(reset=True) == dict(enabled=True, missing=2)
        assert sum("no .absgrad" in r.message for r in caplog.records) == 1      # logged once
        assert counter.abs_grad_stats()["missing"] == 0
    finally:
        assert counter.set_abs_grad(False) is True


class _TwoCallRender:
    render_depth = True
    use_origin_render = False

    def render(self, rasterizer, camera, kw):
        first = rasterizer(**kw)
        second = rasterizer(**dict(kw, colors_precomp=torch.ones_like(kw["colors_precomp"])))
        return first, second


@pytest.mark.parametrize("how", ["constructor", "switch"])
def test_depth_pass_proxy_counts_the_reason(stub, how):
    from log_amd import depth_pass, rasterizer as R
    rast, kw = _call(ctor=dict(abs_grad=True) if how == "constructor" else None)
    camera = {"world_view_transform": rast.raster_settings.viewmatrix}
    depth_pass.reset_stats()
    with (R.abs_grad(True) if how == "switch" else contextlib.nullcontext()):
        first, second = depth_pass.wrap_render(_TwoCallRender.render)(_TwoCallRender(), rast, camera, kw)
    st = depth_pass.stats()
    assert st["calls"] == 1 and st["fused"] == 0 and st["fallback"].get("abs_grad") == 1, st
    assert stub.calls == ["forward", "forward"]               # both calls are real (forward_aux would have failed the test)
    (first[0].sum() + second[0].sum()).backward()
    assert stub.calls[2:] == ["backward_abs", "backward_abs"]
    depth_pass.reset_stats()
    # off: the proxy's own aux path is asked for (the stub's forward_aux fails the test if the call gets there)
    rast, kw = _call()
    proxy = depth_pass._RasterizerProxy(rast, camera)
    assert proxy._covered((), kw) is None


def test_install_all_switches_both_on_and_uninstall_off(monkeypatch):
    import log_amd
    from log_amd import counter, get_all, lod, rasterizer as R, sparse_optimizer
    monkeypatch.setattr(log_amd, "install_compute_radius", lambda: None)
    for m in (get_all, lod, counter, sparse_optimizer):
        monkeypatch.setattr(m, "install", lambda: None)
    try:
        log_amd.install_all()
        assert R._abs_grad_on() is False and counter.abs_grad_stats()["enabled"] is False
        log_amd.install_all(abs_grad=True)
        assert R._abs_grad_on() is True and counter.abs_grad_stats()["enabled"] is True
        log_amd.install_all()                                 # does not switch it off behind the caller's back
        assert R._abs_grad_on() is True
        log_amd.uninstall_abs_grad()
        assert R._abs_grad_on() is False and counter.abs_grad_stats()["enabled"] is False
    finally:
        R.set_abs_grad(False)
        counter.set_abs_grad(False)
