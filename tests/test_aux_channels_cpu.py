"""Aux channels without a GPU.

1. The argument surface of the four aux entry points (lograst_forward_aux, lograst_forward_render_aux,
   lograst_forward_speculative_aux, lograst_backward_aux; log_amd/csrc/api.hip): every row fails a check before any device
   work, so the pointers are never dereferenced.
2. log_amd.depth_pass around the reference's UNMODIFIED NaiveRendererAndLoss with render_depth=True, through a test-side
   subclass of the oracle backend whose forward_aux / backward_aux are two oracle calls: patched against unpatched.  Skipped
   where the reference tree does not exist."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

OK, ERR_ARG = 0, -1
P = 0x10000                                                  # never dereferenced; 64-byte aligned
N, W, H = 8, 64, 64


def _view(**over):
    from log_amd import _lib
    v = _lib.LograstView()
    v.width, v.height, v.tanfovx, v.tanfovy, v.scale_modifier = W, H, 0.5, 0.5, 1.0
    v.filter_mode, v.ndc_cull, v.extras = 2, 1, 1
    v.viewmatrix = v.projmatrix = v.bg = P
    for k, val in over.items():
        setattr(v, k, val)
    return v


def _forward_args(entry, n=N, aux_colors=P, aux_image=P):
    """The arguments of a call that passes every check but the one a row breaks."""
    stage1 = [P] * 8                                         # means3d scales rotations opacities colors radii geom tile_state
    stage2 = [P, P, 1024, 0, P, P, P, P, P, P, P, 16, P]     # keys ... bwd_scratch, floats, status
    hosts = [ctypes.pointer(ctypes.c_uint32(0)), ctypes.pointer(ctypes.c_uint32(0))]
    if entry == "lograst_forward_aux":
        return [n] + stage1 + stage2 + [aux_colors, aux_image, None]
    if entry == "lograst_forward_render_aux":
        return [n, P, P] + stage2 + [aux_colors, aux_image, None]
    return [n] + stage1 + stage2 + [aux_colors, aux_image] + hosts + [None]


def _backward_args(aux_colors=P, dl_dimage=P, dl_daux=P, row_floats=16, dl_daux_colors=P, flags=1):
    #      means3d scales rot radii geom state plist final_t n_contrib
    return [N, P, P, P, P, P, P, P, P, P, aux_colors, dl_dimage, dl_daux, P, P, row_floats, P, P, dl_daux_colors, P, P, P, None,
            flags, None]


FORWARDS = ("lograst_forward_aux", "lograst_forward_render_aux", "lograst_forward_speculative_aux")
BAND = dict(tile_row_begin=1, tile_row_end=3)
FORWARD_TABLE = [
    ("aux_colors NULL", dict(), dict(aux_colors=None), b"aux_colors / aux_image are NULL"),
    ("aux_image NULL", dict(), dict(aux_image=None), b"aux_colors / aux_image are NULL"),
    ("band view", BAND, dict(), b"whole images only"),
    ("cov3d_precomp", dict(cov3d_precomp=P), dict(), b"no cov3d_precomp form"),
]
BACKWARD_TABLE = [
    ("band view", BAND, dict(), b"whole images only"),
    ("cov3d_precomp", dict(cov3d_precomp=P, dl_dcov3d=P), dict(), b"no cov3d_precomp form"),
    ("aux_colors NULL", dict(), dict(aux_colors=None), b"aux_colors / dl_daux_colors are NULL"),
    ("dl_daux_colors NULL", dict(), dict(dl_daux_colors=None), b"aux_colors / dl_daux_colors are NULL"),
    ("both image gradients NULL", dict(), dict(dl_dimage=None, dl_daux=None), b"both NULL"),
    ("rows of 9 floats", dict(), dict(row_floats=9), b"LOGRAST_BWD_ROW_FLOATS (16) floats per Gaussian"),
    ("rows of 12 floats", dict(), dict(row_floats=12), b"LOGRAST_BWD_ROW_FLOATS (16) floats per Gaussian"),
    ("running sums", dict(), dict(flags=1 | 2), b"fresh gradients"),
    ("row-major running sums", dict(), dict(flags=1 | 8), b"fresh gradients"),
]


@pytest.mark.parametrize("entry", FORWARDS)
@pytest.mark.parametrize("row", FORWARD_TABLE, ids=[r[0] for r in FORWARD_TABLE])
def test_forward_argument_errors(entry, row):
    from log_amd import _lib
    _, view_over, arg_over, fragment = row
    L = _lib.lib()
    v = _view(**view_over)
    rc = getattr(L, entry)(ctypes.byref(v), *_forward_args(entry, **arg_over))
    assert rc == ERR_ARG and fragment in L.lograst_last_error(), (rc, L.lograst_last_error())


@pytest.mark.parametrize("row", BACKWARD_TABLE, ids=[r[0] for r in BACKWARD_TABLE])
def test_backward_argument_errors(row):
    from log_amd import _lib
    _, view_over, arg_over, fragment = row
    L = _lib.lib()
    v = _view(**view_over)
    rc = L.lograst_backward_aux(ctypes.byref(v), *_backward_args(**arg_over))
    assert rc == ERR_ARG and fragment in L.lograst_last_error(), (rc, L.lograst_last_error())


@pytest.mark.parametrize("absent", ["dl_dimage", "dl_daux"])
def test_one_image_gradient_alone_is_no_argument_error(absent):
    """One NULL image gradient passes the aux checks: with it, a call whose means3d is NULL as well fails at the later,
    different check of the pointers every backward needs."""
    from log_amd import _lib
    L = _lib.lib()
    args = _backward_args(**{absent: None})
    args[1] = None                                           # means3d
    rc = L.lograst_backward_aux(ctypes.byref(_view()), *args)
    assert rc == ERR_ARG and L.lograst_last_error() == b"NULL pointer", (rc, L.lograst_last_error())


def test_empty_and_negative_counts():
    """n = 0 returns before any pointer is looked at (no launch: nothing to differentiate)."""
    from log_amd import _lib
    L = _lib.lib()
    v = _view()
    args = _backward_args()
    args[0] = 0
    assert L.lograst_backward_aux(ctypes.byref(v), *args) == OK
    args[0] = -1
    assert L.lograst_backward_aux(ctypes.byref(v), *args) == ERR_ARG and b"negative" in L.lograst_last_error()


def test_python_layer_refuses_without_a_backend_for_it():
    """A backend without forward_aux / backward_aux makes an aux call raise (and tensors off the GPU have no fall-back)."""
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    from log_amd import _lib, rasterizer as R
    rs = GaussianRasterizationSettings(32, 32, 0.5, 0.5, torch.zeros(3), 1., torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                       False, False)
    r = GaussianRasterizer(raster_settings=rs)
    z = torch.zeros
    kw = dict(means3D=z(2, 3), means2D=z(2, 3), shs=None, colors_precomp=z(2, 3), opacities=z(2, 1), scales=z(2, 3) + 1,
              rotations=z(2, 4) + 1, cov3D_precomp=None, aux_colors=z(2, 3))
    with pytest.raises(_lib.LograstError, match="no CPU fallback"):
        r(**kw)

    class Bare:
        pass
    old, R._backend = R._backend, Bare()
    try:
        with pytest.raises(_lib.LograstError, match="forward_aux"):
            r(**kw)
    finally:
        R._backend = old


# ---- the drop-in around the reference's renderer ----------------------------------------------------------------------------

REF = os.environ.get("LOG_REFERENCE", "/root/reference")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")


def _aux_backend():
    from oracle_backend import OracleBackend

    class AuxOracleBackend(OracleBackend):
        """forward_aux / backward_aux as two oracle calls each."""

        def forward_aux(self, rs, flavour, use_filter, means3D, scales, rotations, opacities, colors, aux_colors, scratch_floats=0):
            image, radii, pid, pwp, pw, s1 = self.forward(rs, flavour, use_filter, means3D, scales, rotations, opacities, colors)
            aux_image, _, _, _, _, s2 = self.forward(rs, flavour, use_filter, means3D, scales, rotations, opacities, aux_colors)
            return image, radii, pid, pwp, pw, aux_image, (s1, s2)

        def backward_aux(self, rs, flavour, use_filter, means3D, scales, rotations, saved, grad_image, grad_aux):
            zeros = torch.zeros(3, int(rs.image_height), int(rs.image_width))
            g1 = self.backward(rs, flavour, use_filter, means3D, scales, rotations, saved[0], zeros if grad_image is None else grad_image)
            g2 = self.backward(rs, flavour, use_filter, means3D, scales, rotations, saved[1], zeros if grad_aux is None else grad_aux)
            return (g1[0] + g2[0], g1[1] + g2[1], g1[2], g1[3] + g2[3], g1[4] + g2[4], g1[5] + g2[5], g2[2])
    return AuxOracleBackend()


@pytest.fixture()
def log_env(oracle_mod):
    """sys.path + the stubs of tests/test_log_plumbing_cpu.py (cv2, LoG.cuda.compute_radius); the backend is installed by
    the test."""
    from log_amd import rasterizer as R
    from log_amd.compute_radius import compute_radius_module
    import oracle_backend
    added = []
    if REF not in sys.path:
        sys.path.insert(0, REF)
        added.append(REF)
    stubs = {}
    if "cv2" not in sys.modules:
        stubs["cv2"] = types.ModuleType("cv2")
    drop = types.ModuleType("LoG.cuda.compute_radius")
    drop.compute_radius_module = compute_radius_module
    stubs["LoG.cuda.compute_radius"] = drop
    sys.modules.update(stubs)
    old = R._backend
    yield oracle_backend
    oracle_backend.install(None if isinstance(old, R.HipBackend) else old)
    for k in stubs:
        sys.modules.pop(k, None)
    for p in added:
        sys.path.remove(p)


def _batch(cams):
    keys = ["camera_center", "world_view_transform", "full_proj_transform", "K", "R", "T"]
    cam = {k: torch.tensor(np.stack([c[k] for c in cams])) for k in keys}
    for k in ("image_width", "image_height", "FoVx", "FoVy"):
        cam[k] = [c[k] for c in cams]
    return {"camera": cam}


def _render_once(train=True):
    """One view through the reference's vis() -> render() with render_depth=True, and a fixed linear loss over the four
    images -> (outputs, parameter gradients, dL/dviewspace_points)."""
    from LoG.render.renderer import NaiveRendererAndLoss          # reference code, unmodified
    from LoG.model.base_gaussian import BaseGaussian              # reference code, unmodified
    from log_amd import scenes
    n, Wd, focal = 600, 80, 90.0
    cams = scenes.orbit_cameras(1, W=Wd, H=Wd, focal=focal)
    sc = scenes.random_scene(n, seed=0, opacity=None, smax=0.06)
    sc["opacity"] = np.clip(sc["opacity"], 0.05, 0.95)
    model = BaseGaussian.create_from_record({k: v for k, v in sc.items()})
    renderer = NaiveRendererAndLoss(split="train", use_origin_render=False, background=[0.2, 0.5, 0.9], render_depth=True)
    model.train(train)
    out = renderer.vis(_batch(cams), model)
    rng = np.random.default_rng(3)
    w = [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in ((3, Wd, Wd), (Wd, Wd), (Wd, Wd), (Wd, Wd))]
    grads, vs = {}, None
    if train:
        loss = ((out["render"][0] * w[0]).sum() + (out["depth"][0] * w[1]).sum() + (out["height"][0] * w[2]).sum()
                + (out["accmap"][0] * w[3]).sum())
        loss.backward()
        grads = {k: getattr(model, k).grad.clone() for k in ("xyz", "colors", "scaling", "opacity", "rotation")}
        vs = out["viewspace_points"][0].grad.clone()
    return out, grads, vs


def _same_outputs(a, b):
    assert set(a) == set(b)
    for k in a:
        x, y = a[k], b[k]
        x, y = (x[0], y[0]) if isinstance(x, list) else (x, y)
        if torch.is_tensor(x):
            assert x.shape == y.shape and x.dtype == y.dtype, k
            if k in ("depth", "height", "accmap", "render"):
                assert np.array_equal(x.detach().numpy().view(np.uint32), y.detach().numpy().view(np.uint32)), k
            elif not x.requires_grad or x.grad_fn is not None:
                assert torch.equal(x.detach(), y.detach()), k
        else:
            assert x == y, k


@needs_reference
def test_reference_renderer_with_the_depth_pass_wrapped(log_env):
    from log_amd import depth_pass
    log_env.install(_aux_backend())
    plain_out, plain_g, plain_vs = _render_once()
    depth_pass.install()
    depth_pass.reset_stats()
    prev = depth_pass.set_verify(True)
    try:
        out, g, vs = _render_once()
        st = depth_pass.stats()
        assert st == dict(calls=1, fused=1, fallback={}), st
        _same_outputs(out, plain_out)
        for k in plain_g:                          # the same fp32 sums added in another order (the world-z path into xyz too)
            err = float((g[k] - plain_g[k]).norm() / plain_g[k].norm())
            assert float(plain_g[k].norm()) > 0 and err < 1e-6, (k, err)
        assert float((vs - plain_vs).norm() / plain_vs.norm()) < 1e-6     # one summed dL/dmeans2D, as Counter sees it
        # fall-backs, each counted by its reason: evaluation mode passes use_filter=False on the first call only ...
        depth_pass.reset_stats()
        ev, _, _ = _render_once(train=False)
        st = depth_pass.stats()
        assert st["fused"] == 0 and st["fallback"].get("use_filter differs between the two calls") == 1, st
        # ... and a backend without forward_aux
        log_env.install(log_env.OracleBackend())
        depth_pass.reset_stats()
        out2, g2, _ = _render_once()
        st = depth_pass.stats()
        assert st["fused"] == 0 and st["fallback"].get("the backend has no forward_aux") == 1, st
        _same_outputs(out2, plain_out)
        for k in plain_g:
            assert float((g2[k] - plain_g[k]).norm() / plain_g[k].norm()) < 1e-6, k
    finally:
        depth_pass.set_verify(prev)
        depth_pass.uninstall()
    from LoG.render.renderer import NaiveRendererAndLoss
    assert not hasattr(NaiveRendererAndLoss.render, "_lograst_original")
    ev_plain, _, _ = _render_once(train=False)
    _same_outputs(ev, ev_plain)


@needs_reference
def test_verify_raises_on_other_depth_colours(log_env):
    """The proxy's second call with a colors_precomp that is not what the first call composited: LograstError under
    set_verify(True); other geometry tensors go to the real rasterizer."""
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    from log_amd import _lib, depth_pass, scenes
    log_env.install(_aux_backend())
    cam = scenes.orbit_cameras(1, W=48, H=48, focal=50.0)[0]
    sc = scenes.random_scene(100, seed=1, opacity=None, smax=0.1)
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    rs = GaussianRasterizationSettings(48, 48, math.tan(cam["FoVx"] * 0.5), math.tan(cam["FoVy"] * 0.5), torch.zeros(3), 1.,
                                       t(cam["world_view_transform"]), t(cam["full_proj_transform"]), 0, t(cam["camera_center"]),
                                       False, False)
    camera = {"world_view_transform": t(cam["world_view_transform"])}
    kw = dict(means3D=t(sc["xyz"]), means2D=torch.zeros(100, 3), shs=None, opacities=t(sc["opacity"]), scales=t(sc["scaling"]),
              rotations=t(sc["rotation"]), cov3D_precomp=None)

    def two_calls(second_colors, second_kw=None):
        proxy = depth_pass._RasterizerProxy(GaussianRasterizer(raster_settings=rs), camera)
        assert proxy.raster_settings is rs                                   # everything but the call is the real object's
        first = proxy(colors_precomp=t(sc["colors"]), **kw)
        return first, proxy(colors_precomp=second_colors, **dict(kw, **(second_kw or {})))
    prev = depth_pass.set_verify(True)
    depth_pass.reset_stats()
    try:
        with pytest.raises(_lib.LograstError, match="view z, world z, 1"):
            two_calls(torch.rand(100, 3))
        first, second = two_calls(torch.rand(100, 3), dict(means3D=kw["means3D"].clone()))
        assert len(first) == 5 and len(second) == 5
        st = depth_pass.stats()
        assert st["fallback"] == {"the second call has other tensors": 1}, st
    finally:
        depth_pass.set_verify(prev)
