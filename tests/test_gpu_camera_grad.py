"""Camera gradients on the device: viewmatrix.grad / projmatrix.grad of a rasterizer call whose settings hold matrices that
require grad, against the float64 autograd twin (tests/camera_grad_cases.py; oracle/torch_oracle.py is differentiable in both
matrices) at GRAD_TOL = 1e-4 relative L2 per matrix -- BASELINE's bound for every gradient of the project; the CPU file
tests/test_camera_grad_cpu.py holds that each scene's camera gradients move by less than a tenth of that when the inputs are
rounded through fp32.  Column 3 of dL/dviewmatrix and column 2 of dL/dprojmatrix are exactly 0.0.

The sums are made inside the chain-rule launch, one row of 24 partials per 1024-row workgroup, and added in workgroup order by
a finishing kernel: the row counts below sit on the edges of the wave (63, 65) and of the workgroup (1023, 1024, 1025), one
scene has a workgroup without a live row, one view sees nothing."""
import numpy as np
import pytest
import torch

import camera_grad_cases as C
from util import cam_tan, rel_l2

pytestmark = pytest.mark.gpu

GRAD_TOL = 1e-4     # relative L2 against the reference, stated by BASELINE.json
ORDER_TOL = 1e-5    # two device evaluations of the same sums, atomic order only
DEV = "cuda:0"
KEYS = {"means3D": "xyz", "scales": "scaling", "rotations": "rotation", "opacities": "opacity", "colors": "colors"}


def _package(name):
    import diff_gaussian_rasterization as up
    import diff_gaussian_rasterization_wodilate as wo
    return wo if name == "wodilate" else up


class Run:
    """One forward through the public package with V / P in the settings; backward() runs sum(image * dL).backward()."""

    def __init__(self, c, grad_v=True, grad_p=True, **extra):
        from log_amd import rasterizer as R
        cam, sc = c["cam"], c["sc"]
        dev = torch.device(DEV)
        t = lambda a, g=False: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev, requires_grad=g)
        self.V, self.P = t(c["V"], grad_v), t(c["P"], grad_p)
        tfx, tfy = cam_tan(cam)
        rs = R.GaussianRasterizationSettings(cam["image_height"], cam["image_width"], tfx, tfy, t(C.BG), c["scale_modifier"],
                                             self.V, self.P, 0, t(cam["camera_center"]), False, False)
        self.leaves = {k: t(sc[src], True) for k, src in KEYS.items()}
        self.leaves["means2D"] = torch.zeros(len(sc["xyz"]), 3, device=dev, requires_grad=True)
        L = self.leaves
        kw = dict(means3D=L["means3D"], means2D=L["means2D"], shs=None, colors_precomp=L["colors"], opacities=L["opacities"],
                  scales=L["scales"], rotations=L["rotations"], cov3D_precomp=None)
        kw.update(extra)
        if c["package"] == "wodilate" and not c["use_filter"]:
            kw["use_filter"] = False
        assert c["use_filter"] or c["package"] == "wodilate"
        self.out = _package(c["package"]).GaussianRasterizer(raster_settings=rs)(**kw)
        self.dL = t(C.dL_of(c))

    def backward(self, retain_graph=False):
        for x in list(self.leaves.values()) + [self.V, self.P]:
            x.grad = None
        (self.out[0] * self.dL).sum().backward(retain_graph=retain_graph)
        torch.cuda.synchronize()
        g = {k: v.grad.cpu().numpy() for k, v in self.leaves.items()}
        g["V"] = None if self.V.grad is None else self.V.grad.cpu().numpy()
        g["P"] = None if self.P.grad is None else self.P.grad.cpu().numpy()
        return g


_twins = {}


def _twin(name):
    """The reference of a scene, computed once (the largest scene on the device, in float64)."""
    if name not in _twins:
        _twins[name] = C.twin(C.SCENES[name](), device=DEV if name == "ragged" else "cpu")
    return _twins[name]


def _hold_camera(g, tw, name):
    eV, eP = rel_l2(g["V"], tw["V"]), rel_l2(g["P"], tw["P"])
    print(f"{name}: dL/dV {eV:.2e}  dL/dP {eP:.2e}")
    assert g["V"].dtype == np.float32 and g["V"].shape == (4, 4) and g["P"].shape == (4, 4)
    assert (g["V"][:, 3] == 0.0).all() and (g["P"][:, 2] == 0.0).all()
    assert eV < GRAD_TOL and eP < GRAD_TOL, (name, eV, eP)


@pytest.mark.parametrize("name", [n for n in C.SCENES if not (n.endswith("nofilter") and "upstream" in n)])
def test_camera_gradients_against_the_twin(name):
    """Both flavours, the fork's use_filter on / off (the upstream package has no such switch: its filter-off scene is the
    isolated chain rule's below), scale_modifier 1.7, a skewed V, the clamp branches, the row-count edges."""
    g = Run(C.SCENES[name]()).backward()
    tw = _twin(name)
    assert float(np.abs(tw["V"]).sum()) > 0
    _hold_camera(g, tw, name)


def test_upstream_flavour_without_its_filter():
    """FILTER_NONE under the upstream flavour (no |ndc| cull): the package has no switch for it, the backend has."""
    import gpu_util as G
    from log_amd import rasterizer as R
    name = "small-upstream-nofilter"
    c = C.SCENES[name]()
    hf = G.hip_forward(c["cam"], c["sc"], C.BG, R.UPSTREAM, False, DEV, scratch_floats=16)
    rs, flavour, use_filter, m, s, r, saved = hf["_torch"]
    out = R._backend.backward_camera(rs, flavour, use_filter, m, s, r, saved, torch.tensor(C.dL_of(c), device=m.device))
    torch.cuda.synchronize()
    _hold_camera(dict(V=out[6].cpu().numpy(), P=out[7].cpu().numpy()), _twin(name), name)


def test_clamp_scene_holds_its_condition():
    c = C.clamp_case()
    nx, ny, nlow = C.clamp_branch_counts(c, _twin("clamp-branches"))
    assert min(nx, ny, nlow) >= 8, (nx, ny, nlow)


@pytest.mark.parametrize("which", ["V", "P"])
def test_one_matrix_alone(which):
    name = "small-wodilate-filter"
    g = Run(C.SCENES[name](), grad_v=which == "V", grad_p=which == "P").backward()
    other = "P" if which == "V" else "V"
    assert g[other] is None
    e = rel_l2(g[which], _twin(name)[which])
    assert e < GRAD_TOL, e


def test_no_gaussians_and_nothing_visible_give_zeros():
    for c in (C.rows_case(0), C.culled_case()):
        g = Run(c).backward()
        for k in ("V", "P"):
            assert g[k] is not None and g[k].shape == (4, 4) and g[k].dtype == np.float32 and (g[k] == 0.0).all()


def test_second_backward_of_the_same_forward():
    """retain_graph: the second backward has no block the forward cleared (a fresh accumulator; live flags from radii)."""
    name = "small-wodilate-filter"
    run = Run(C.SCENES[name]())
    g1 = run.backward(retain_graph=True)
    g2 = run.backward()
    _hold_camera(g2, _twin(name), name + " (second backward)")
    for k in g1:
        assert rel_l2(g2[k], g1[k]) < ORDER_TOL, (k, rel_l2(g2[k], g1[k]))


@pytest.mark.parametrize("name", ["small-wodilate-filter", "small-upstream-filter", "ragged"])
def test_per_gaussian_gradients_are_unchanged(oracle_mod, name):
    """With the camera sums the per-Gaussian gradients stay within ORDER_TOL of the same backward without them and within
    GRAD_TOL of the oracle, as before."""
    import gpu_util as G
    from log_amd import rasterizer as R
    c = C.SCENES[name]()
    with_cam, without = Run(c).backward(), Run(c, grad_v=False, grad_p=False).backward()
    assert without["V"] is None and without["P"] is None
    flavour = R.WODILATE if c["package"] == "wodilate" else R.UPSTREAM
    v, f = G.oracle_forward(oracle_mod, c["cam"], c["sc"], C.BG, flavour, c["use_filter"], c["scale_modifier"])
    og = oracle_mod.backward(v, f, C.dL_of(c))
    for k in C.PER_GAUSSIAN:
        a, b, o = with_cam[k], without[k], np.asarray(og[k]).reshape(with_cam[k].shape)
        if k == "means2D":
            a, b, o = a[:, :2], b[:, :2], o[:, :2]
        assert rel_l2(a, b) < ORDER_TOL, (k, rel_l2(a, b))
        assert rel_l2(a, o) < GRAD_TOL, (k, rel_l2(a, o))


@pytest.mark.parametrize("name", ["small-upstream-nofilter", "rows-1025", "dead-middle-2049"])
def test_isolated_chain_rule_on_fixed_inputs(name):
    """lograst_project_backward_camera on fixed dL/dmeans2D / dL/dconic: two calls give the same bits (the partials are added
    in a fixed order, no atomics); the per-Gaussian outputs are the bits of the call without the camera sums; and the
    structural zeros are zeros.  (upstream-nofilter: FILTER_NONE under the upstream flavour, which the package cannot ask for.)"""
    import gpu_util as G
    from log_amd import rasterizer as R
    c = C.SCENES[name]()
    flavour = R.WODILATE if c["package"] == "wodilate" else R.UPSTREAM
    cam = dict(c["cam"], world_view_transform=c["V"], full_proj_transform=c["P"])
    hf = G.hip_forward(cam, c["sc"], C.BG, flavour, c["use_filter"], DEV, c["scale_modifier"])
    rs, flavour, use_filter, m, s, r, saved = hf["_torch"]
    n = m.shape[0]
    rng = np.random.default_rng(9)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=m.device)
    g2 = t(np.concatenate([rng.standard_normal((n, 2)), np.zeros((n, 1))], axis=1))
    gc = t(np.concatenate([1e-3 * rng.standard_normal((n, 3)), np.zeros((n, 1))], axis=1))
    call = lambda camera: R._backend.project_backward(rs, flavour, use_filter, m, s, r, saved["radii"], g2, gc, camera=camera)
    plain, a, b = call(False), call(True), call(True)
    torch.cuda.synchronize()
    assert len(plain) == 3 and len(a) == 5
    for x, y in zip(plain, a[:3]):
        assert torch.equal(x, y)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    dV, dP = a[3].cpu().numpy(), a[4].cpu().numpy()
    assert (dV[:, 3] == 0).all() and (dP[:, 2] == 0).all() and np.abs(dV[:, :3]).min() > 0 and np.abs(dP[:, [0, 1, 3]]).min() > 0
    assert np.isfinite(dV).all() and np.isfinite(dP).all()


def test_backend_refuses_what_has_no_camera_form():
    """HipBackend.backward(camera=True) next to a sink, cov3D_precomp, a band or aux: its own error, before any launch; the
    C entry point says the same of the accumulate flags (tests/test_camera_grad_cpu.py)."""
    import gpu_util as G
    from log_amd import rasterizer as R
    c = C.rows_case(63)
    hf = G.hip_forward(c["cam"], c["sc"], C.BG, scratch_floats=16)
    rs, flavour, use_filter, m, s, r, saved = hf["_torch"]
    g = torch.ones(3, c["cam"]["image_height"], c["cam"]["image_width"], device=m.device)
    n = m.shape[0]
    sink = dict(rows=torch.zeros(n, 16, device=m.device))
    with pytest.raises(ValueError, match="accumulate_grads_into"):
        R._backend.backward(rs, flavour, use_filter, m, s, r, saved, g, sink=sink, camera=True)
    with pytest.raises(ValueError, match="cov3D_precomp"):
        R._backend.backward(rs, flavour, use_filter, m, None, None, saved, g, cov3D=torch.ones(n, 6, device=m.device), camera=True)
    out = R._backend.backward_camera(rs, flavour, use_filter, m, s, r, saved, g)
    assert len(out) == 8 and out[6].shape == (4, 4) and out[7].shape == (4, 4)
