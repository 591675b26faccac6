"""Camera gradients (dL/dviewmatrix, dL/dprojmatrix) without a GPU.

1. The reference of the GPU tests checks itself: the float64 twin's autograd gradients in V and P against central finite
   differences of its own loss, within the 1e-6 relative L2 of tests/test_oracle_autograd.py's checks of this kind, on every
   scene of tests/camera_grad_cases.py (the largest at a reduced size: 64 twin evaluations each).  Column 3 of dL/dV and column
   2 of dL/dP are exactly zero.
2. Conditioning: on every scene at its full size, float64 inputs and their rounding through fp32 give camera gradients within
   1e-5 relative L2 of each other -- a tenth of GRAD_TOL, so the 1e-4 the kernels are held to on the GPU is a fair bound
   for fp32 arithmetic.  A scene that fails is replaced, not exempted.  The clamp scene holds its own condition: at least 8
   composited Gaussians in each clamp branch of the EWA Jacobian and with a clamped low-pass diagonal.
3. The C entry points refuse what has no camera form before any device work.
4. The Python layer: with the CPU oracle backend (no backward_camera) a matrix that requires grad raises "this backend has
   no ..."; the four refused combinations raise their own errors before any backend call; without requires_grad the autograd
   function and the backend get exactly today's arguments."""
import ctypes

import pytest
import torch

import camera_grad_cases as C
from util import rel_l2

FD_TOL = 1e-6      # tests/test_oracle_autograd.py: autograd against central differences in float64
COND_TOL = 1e-5    # fp32 rounding of the inputs against float64 inputs: a tenth of the GPU tests' GRAD_TOL


@pytest.mark.parametrize("name", list(C.SCENES))
def test_twin_autograd_against_central_differences(name):
    c = C.REDUCED.get(name, C.SCENES[name])()
    g = C.twin(c)
    # Two steps: a central difference is an estimate of the derivative only where no decision of the forward (tile rect, alpha
    # floor, cull) flips within the step -- which favours the small one -- and where the rounding of the loss, eps |loss| / h
    # with a loss dominated by the background term, stays below the bound -- which favours the large one (a scene of one
    # Gaussian: 4e-6 at 1e-7).  Either estimate within the bound confirms the autograd gradient; a wrong one matches neither.
    eV = eP = float("inf")
    for h in (1e-7, 1e-6):
        fV, fP = C.finite_differences(c, h)
        eV, eP = min(eV, rel_l2(g["V"], fV)), min(eP, rel_l2(g["P"], fP))
        if eV < FD_TOL and eP < FD_TOL:
            break
    print(f"{name}: dL/dV {eV:.2e}  dL/dP {eP:.2e}")
    assert eV < FD_TOL and eP < FD_TOL, (eV, eP)
    assert (g["V"][:, 3] == 0).all() and (g["P"][:, 2] == 0).all()
    assert abs(g["V"][:, :3]).min() > 0 and abs(g["P"][:, [0, 1, 3]]).min() > 0   # every other entry carries gradient


@pytest.mark.parametrize("name", list(C.SCENES))
def test_camera_gradients_are_well_conditioned_in_fp32(name):
    c = C.SCENES[name]()
    g32, g64 = C.twin(c), C.twin(c, unrounded=True)
    eV, eP = rel_l2(g32["V"], g64["V"]), rel_l2(g32["P"], g64["P"])
    print(f"{name}: dL/dV {eV:.2e}  dL/dP {eP:.2e}")
    assert (g32["point_weight"] > 0).sum() >= 1
    assert eV < COND_TOL and eP < COND_TOL, (eV, eP)


def test_clamp_scene_reaches_every_branch():
    c = C.clamp_case()
    nx, ny, nlow = C.clamp_branch_counts(c, C.twin(c, grads=False))
    assert nx >= 8 and ny >= 8 and nlow >= 8, (nx, ny, nlow)


def test_dead_middle_scene_has_a_workgroup_without_a_live_row():
    c = C.dead_middle_case()
    radii = C.twin(c, grads=False)["radii"]
    assert (radii[1024:2048] == 0).all() and (radii[:1024] > 0).sum() > 100 and radii[2048] > 0


def test_culled_scene_sees_nothing():
    assert (C.twin(C.culled_case(), grads=False)["radii"] == 0).all()


# ---- the C entry points ------------------------------------------------------------------------------------------------

OK, ERR_ARG = 0, -1
PTR = 0x10000                                                # never dereferenced; 64-byte aligned
N = 2000


def _view(**over):
    from log_amd import _lib
    v = _lib.LograstView()
    v.width, v.height, v.tanfovx, v.tanfovy, v.scale_modifier = 64, 64, 0.5, 0.5, 1.0
    v.filter_mode, v.ndc_cull, v.extras = 2, 1, 1
    v.viewmatrix = v.projmatrix = v.bg = PTR
    for k, val in over.items():
        setattr(v, k, val)
    return v


def _backward(view, n=N, flags=1, dv=PTR, dp=PTR, scratch=PTR, scratch_bytes=None, means3d=None):
    """lograst_backward_camera with means3d NULL: a call that passes the camera checks ends at 'NULL pointer'."""
    from log_amd import _lib
    L = _lib.lib()
    if scratch_bytes is None:
        scratch_bytes = L.lograst_camera_scratch_bytes(n)
    rc = L.lograst_backward_camera(ctypes.byref(view), n, means3d, *([PTR] * 17), flags, dv, dp, scratch, scratch_bytes, None)
    return rc, L.lograst_last_error()


def _project_backward(view, n=N, dv=PTR, dp=PTR, scratch=PTR, scratch_bytes=None):
    from log_amd import _lib
    L = _lib.lib()
    if scratch_bytes is None:
        scratch_bytes = L.lograst_camera_scratch_bytes(n)
    rc = L.lograst_project_backward_camera(ctypes.byref(view), n, None, *([PTR] * 8), dv, dp, scratch, scratch_bytes, None)
    return rc, L.lograst_last_error()


def test_scratch_size_is_one_row_of_24_floats_per_1024_gaussians():
    """... plus the 64 x 24 doubles the finishing kernels of a large view pass between them."""
    from log_amd import _lib
    L = _lib.lib()
    stage = 64 * 24 * 8
    assert [L.lograst_camera_scratch_bytes(n) - stage for n in (0, 1, 1024, 1025, 30_000_000)] == \
        [96, 96, 96, 192, 96 * ((30_000_000 + 1023) // 1024)]


REFUSED = [
    ("running sums", dict(), dict(flags=1 | 2), b"fresh gradients only"),
    ("row-major running sums", dict(), dict(flags=1 | 8), b"fresh gradients only"),
    ("cov3d_precomp", dict(cov3d_precomp=PTR, dl_dcov3d=PTR), dict(), b"no cov3d_precomp form"),
    ("band view", dict(tile_row_begin=1, tile_row_end=3), dict(), b"whole images only"),
    ("dl_dviewmatrix NULL", dict(), dict(dv=None), b"dl_dviewmatrix / dl_dprojmatrix are NULL"),
    ("dl_dprojmatrix NULL", dict(), dict(dp=None), b"dl_dviewmatrix / dl_dprojmatrix are NULL"),
    ("scratch NULL", dict(), dict(scratch=None), b"lograst_camera_scratch_bytes"),
    ("scratch one row short", dict(), dict(scratch_bytes=96 + 64 * 24 * 8), b"lograst_camera_scratch_bytes"),
    ("scratch misaligned", dict(), dict(scratch=PTR + 4), b"8-byte aligned"),
    ("negative count", dict(), dict(n=-1, scratch_bytes=96), b"negative"),
]


@pytest.mark.parametrize("row", REFUSED, ids=[r[0] for r in REFUSED])
def test_backward_camera_refuses_before_any_launch(row):
    _, view_over, arg_over, fragment = row
    rc, msg = _backward(_view(**view_over), **arg_over)
    assert rc == ERR_ARG and fragment in msg, (rc, msg)


@pytest.mark.parametrize("row", [r for r in REFUSED if "running" not in r[0]], ids=[r[0] for r in REFUSED if "running" not in r[0]])
def test_project_backward_camera_refuses_before_any_launch(row):
    _, view_over, arg_over, fragment = row
    rc, msg = _project_backward(_view(**view_over), **arg_over)
    assert rc == ERR_ARG and fragment in msg, (rc, msg)


def test_a_call_that_passes_the_camera_checks_reaches_the_common_ones():
    for call in (_backward, _project_backward):
        rc, msg = call(_view())
        assert rc == ERR_ARG and msg == b"NULL pointer", (rc, msg)


# ---- the Python layer ----------------------------------------------------------------------------------------------------

def _rasterizer_call(c, grad_v=False, grad_p=False, **extra):
    import diff_gaussian_rasterization_wodilate as wo
    from log_amd import rasterizer as R
    from util import cam_tan
    cam, sc = c["cam"], c["sc"]
    tfx, tfy = cam_tan(cam)
    t = torch.tensor
    V, P = t(c["V"], requires_grad=grad_v), t(c["P"], requires_grad=grad_p)
    rs = R.GaussianRasterizationSettings(cam["image_height"], cam["image_width"], tfx, tfy, t(C.BG), 1.0, V, P, 0,
                                         t(cam["camera_center"]), False, False)
    n = len(sc["xyz"])
    kw = dict(means3D=t(sc["xyz"], requires_grad=True), means2D=torch.zeros(n, 3), shs=None, colors_precomp=t(sc["colors"]),
              opacities=t(sc["opacity"]), scales=t(sc["scaling"]), rotations=t(sc["rotation"]), cov3D_precomp=None)
    kw.update(extra)
    return wo.GaussianRasterizer(raster_settings=rs), kw, V, P


class _Spy:
    """Wraps the oracle backend: counts every call that reaches it."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def __getattr__(self, name):
        attr = getattr(self.inner, name)     # (AttributeError for what the oracle backend does not have: backward_camera)
        if not callable(attr):
            return attr

        def call(*a, **k):
            self.calls.append((name, len(a), sorted(k)))
            return attr(*a, **k)
        return call


@pytest.fixture
def spy(oracle_mod):
    import oracle_backend
    s = _Spy(oracle_backend.OracleBackend())
    old = oracle_backend.install(s)
    yield s
    oracle_backend.install(old)


@pytest.mark.parametrize("which", ["viewmatrix", "projmatrix", "both"])
def test_a_backend_without_the_method_raises(spy, which):
    from log_amd import _lib
    rast, kw, _, _ = _rasterizer_call(C.rows_case(63), grad_v=which != "projmatrix", grad_p=which != "viewmatrix")
    with pytest.raises(_lib.LograstError, match="this backend has no backward_camera"):
        rast(**kw)
    assert spy.calls == []


def test_refused_combinations_raise_before_any_backend_call(spy):
    import contextlib
    from log_amd import rasterizer as R
    c = C.rows_case(63)
    n = len(c["sc"]["xyz"])
    spy.inner.backward_camera = lambda *a, **k: pytest.fail("the backend was called")   # a backend WITH the method
    sink = {k: torch.zeros(n, w) for k, w in (("means3D", 3), ("scales", 3), ("rotations", 4), ("opacities", 1), ("colors", 3))}
    rows = [
        (R.accumulate_grads_into(sink), dict(), "accumulate_grads_into"),
        (contextlib.nullcontext(), dict(scales=None, rotations=None, cov3D_precomp=torch.ones(n, 6)), "cov3D_precomp"),
        (R.tile_rows(0, 1), dict(), "a tile_rows band"),
        (contextlib.nullcontext(), dict(aux_colors=torch.zeros(n, 3)), "aux_colors"),
    ]
    for ctx, extra, fragment in rows:
        rast, kw, _, _ = _rasterizer_call(c, grad_v=True, **extra)
        with ctx, pytest.raises(ValueError, match="camera gradients cannot be combined with " + fragment):
            rast(**kw)
    assert spy.calls == []


def test_without_requires_grad_the_call_is_todays(spy, monkeypatch):
    from log_amd import rasterizer as R
    seen = []
    apply = R._RasterizeGaussians.apply
    monkeypatch.setattr(R._RasterizeGaussians, "apply", staticmethod(lambda *a: seen.append(len(a)) or apply(*a)))
    rast, kw, V, P = _rasterizer_call(C.rows_case(63))
    out = rast(**kw)
    out[0].sum().backward()
    assert seen == [13]                                       # no viewmatrix / projmatrix behind aux_colors
    assert [name for name, _, _ in spy.calls] == ["forward", "backward"]
    assert spy.calls[1][2] == ["cov3D", "sink"]               # the backend's backward got no further keyword
    assert V.grad is None and P.grad is None and kw["means3D"].grad is not None
    # ... and under no_grad a matrix that requires grad changes nothing either
    rast, kw, V, P = _rasterizer_call(C.rows_case(63), grad_v=True, grad_p=True)
    with torch.no_grad():
        rast(**kw)
    assert seen == [13, 13]
