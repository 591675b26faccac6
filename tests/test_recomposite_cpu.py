"""CPU checks of geometry reuse (log_amd.rasterizer.set_geometry_reuse / lograst_recomposite): the ABI names, the argument
validation of the new entry point (no device work), and the decision logic -- which second call composites the first
call's lists again and which runs the full forward -- under a test double defined here."""
import contextlib
import ctypes
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from util import rel_l2, small_case

ORDER_TOL = 1e-5   # the oracle's backward sums in thread order: two evaluations of the same sums (the suite's bound for those)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("LOG_REFERENCE", "/root/reference")


def test_abi_names_are_declared_bound_and_exported():
    from log_amd import _lib
    src = open(os.path.join(ROOT, "include", "lograst.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("lograst_recomposite", "lograst_record_bytes"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    L = _lib.lib()
    assert L.lograst_version() == 4                                  # an addition within version 4
    assert L.lograst_record_bytes(10) == 640 and L.lograst_record_bytes(0) == 0 and L.lograst_record_bytes(-3) == 0
    assert L.lograst_record_bytes(10) < L.lograst_geom_bytes(10)
    names = [L.lograst_kernel_name(i) for i in range(_lib.NUM_KERNEL_SLOTS)]
    assert names[-1] == b"recolor" and names[:_lib.NUM_KERNELS][-2:] == [b"loss_fwd", b"loss_bwd"]   # appended
    assert L.lograst_kernel_name(_lib.NUM_KERNEL_SLOTS) == b""


def test_recomposite_validates_its_arguments_before_device_work():
    """n < 0, NULL outputs, a mis-aligned bwd_scratch, a band view and records == geom are refused with a message -- on a
    machine without a GPU (the pointers below are never dereferenced)."""
    from log_amd import _lib
    L = _lib.lib()
    P = lambda a: ctypes.c_void_p(a)
    v = _lib.LograstView()
    v.width, v.height, v.tanfovx, v.tanfovy, v.scale_modifier = 64, 48, 0.5, 0.5, 1.0
    v.filter_mode, v.ndc_cull, v.extras = _lib.FILTER_CLAMP, 1, 1
    v.viewmatrix, v.projmatrix, v.bg = 0x1000, 0x2000, 0x3000

    def call(n=8, radii=0x10000, geom=0x20000, state=0x30000, plist=0x40000, cap=100, colors=0x50000, records=0x60000,
             radii_out=0x70000, image=0x80000, final_t=0x90000, n_contrib=0xa0000, pid=0xb0000, pwp=0xc0000, pw=0xd0000,
             scratch=0xe0000, scratch_floats=16, view=v):
        rc = L.lograst_recomposite(ctypes.byref(view) if view is not None else None, n, P(radii), P(geom), P(state),
                                   P(plist), cap, 0, P(colors), P(records), P(radii_out), P(image), P(final_t), P(n_contrib),
                                   P(pid), P(pwp), P(pw), P(scratch), scratch_floats, None, None)
        return rc, L.lograst_last_error()

    rc, msg = call(n=-1)
    assert rc == -1 and b"negative" in msg
    for kw in (dict(image=0), dict(final_t=0), dict(n_contrib=0), dict(records=0), dict(radii_out=0), dict(state=0),
               dict(colors=0), dict(radii=0), dict(geom=0), dict(plist=0)):
        rc, msg = call(**kw)
        assert rc == -1 and b"NULL" in msg, (kw, msg)
    rc, msg = call(pid=0)
    assert rc == -1 and b"extras" in msg
    rc, msg = call(scratch=0xe0010)
    assert rc == -1 and b"64-byte aligned" in msg
    rc, msg = call(scratch_floats=12)
    assert rc == -1 and b"bwd_scratch" in msg
    rc, msg = call(records=0x20000)
    assert rc == -1 and b"records" in msg
    rc, msg = call(records=0x60004)
    assert rc == -1 and b"16-byte aligned" in msg
    rc, msg = call(view=None)
    assert rc == -1 and b"view" in msg
    band = _lib.LograstView.from_buffer_copy(v)
    band.tile_row_begin, band.tile_row_end = 1, 2
    rc, msg = call(view=band)
    assert rc == -1 and b"whole images" in msg


# ---- the decision logic, under a test double -------------------------------------------------------------------------------
def _double():
    """TEST DOUBLE: the oracle backend of tests/oracle_backend.py with a `recomposite` -- the oracle's forward on the
    geometry the remembered forward ran on, with the new colours -- that counts its calls."""
    from oracle_backend import OracleBackend

    class Recompositing(OracleBackend):
        def __init__(self):
            self.inputs, self.recomposites, self.forwards, self.plan = {}, 0, 0, 0

        def forward(self, rs, flavour, use_filter, means3D, scales, rotations, opacities, colors, scratch_floats=0,
                    cov3D=None):
            self.forwards += 1
            out = super().forward(rs, flavour, use_filter, means3D, scales, rotations, opacities, colors,
                                  scratch_floats=scratch_floats, cov3D=cov3D)
            self.inputs[id(out[-1][1])] = (means3D.clone(), None if scales is None else scales.clone(),
                                           None if rotations is None else rotations.clone(), opacities.clone(), out[-1])
            return out

        def plan_key(self, saved):
            return self.plan

        def recomposite(self, rs, flavour, use_filter, saved, colors, scratch_floats=0):
            self.recomposites += 1
            m, s, r, o, _keep = self.inputs[id(saved[1])]
            return OracleBackend.forward(self, rs, flavour, use_filter, m, s, r, o, colors, scratch_floats=scratch_floats)

    return Recompositing()


@contextlib.contextmanager
def _installed(backend, reuse=True):
    import oracle_backend
    from log_amd import rasterizer as R
    old = oracle_backend.install(backend)
    prev = R.set_geometry_reuse(reuse)
    R.geometry_reuse_stats(reset=True)
    try:
        yield R
    finally:
        R.set_geometry_reuse(prev)
        R.set_instance_capacity(None)
        oracle_backend.install(None if isinstance(old, R.HipBackend) else old)


def _settings(cam):
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    return GaussianRasterizationSettings(
        image_height=cam["image_height"], image_width=cam["image_width"], tanfovx=math.tan(cam["FoVx"] * 0.5),
        tanfovy=math.tan(cam["FoVy"] * 0.5), bg=t([0.3, 0.6, 0.9]), scale_modifier=1.0, viewmatrix=t(cam["world_view_transform"]),
        projmatrix=t(cam["full_proj_transform"]), sh_degree=0, campos=t(cam["camera_center"]), prefiltered=False, debug=False)


class _Scene:
    def __init__(self, n=120):
        import diff_gaussian_rasterization_wodilate as wo
        self.cam, sc = small_case(n=n, W=48, H=40, seed=0)
        T = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), requires_grad=True)
        self.m3, self.sca, self.rot, self.op, self.col = (T(sc[k]) for k in ("xyz", "scaling", "rotation", "opacity", "colors"))
        self.m2 = torch.zeros_like(self.m3, requires_grad=True)
        self.rs = _settings(self.cam)
        self.rast = wo.GaussianRasterizer(raster_settings=self.rs)
        self.wo = wo
        self.col2 = torch.stack([self.m3.detach()[:, 0] + 3.0, self.m3[:, 2], torch.ones(len(self.m3))], dim=-1)

    def kw(self, colors, **over):
        kw = dict(means3D=self.m3, means2D=self.m2, shs=None, colors_precomp=colors, opacities=self.op, scales=self.sca,
                  rotations=self.rot, cov3D_precomp=None)
        kw.update(over)
        return kw


def _touch(t):
    with torch.no_grad():
        t.mul_(1.0)


def _band():
    from log_amd import rasterizer as R
    return R.tile_rows(1, 2)


def _rows():
    from log_amd import rasterizer as R
    return R.walk_form("rows")


# name -> (what happens between the two calls / around the second one, the reason geometry_reuse_stats must give)
BREAKS = {
    "means3D": (lambda s, R, be: _touch(s.m3), "geometry"),
    "scales": (lambda s, R, be: _touch(s.sca), "geometry"),
    "rotations": (lambda s, R, be: _touch(s.rot), "geometry"),
    "opacities": (lambda s, R, be: _touch(s.op), "geometry"),
    "viewmatrix": (lambda s, R, be: s.rs.viewmatrix.mul_(1.0), "view_modified"),
    "projmatrix": (lambda s, R, be: s.rs.projmatrix.mul_(1.0), "view_modified"),
    "bg": (lambda s, R, be: s.rs.bg.mul_(1.0), "view_modified"),
    "settings_object": (lambda s, R, be: setattr(s.rast, "raster_settings", s.rs._replace()), "settings"),
    "flavour": (lambda s, R, be: setattr(s.rast, "FLAVOUR", R.WODILATE._replace(ndc_cull=0)), "flavour"),
    "plan": (lambda s, R, be: setattr(be, "plan", 1), "plan"),
    "capacity_hint": (lambda s, R, be: R.set_instance_capacity(100000), "capacity_hint"),
    "radii_modified": (lambda s, R, be: s.out1[1].add_(0), "radii_modified"),
}
SECOND = {
    "use_filter": (dict(use_filter=False), None, "use_filter"),
    "band": ({}, _band, "band"),
    "walk_form": ({}, _rows, "walk_form"),
}


def test_reuse_happens_when_every_condition_holds():
    be = _double()
    with _installed(be) as R:
        s = _Scene()
        out1 = s.rast(**s.kw(s.col))
        out2 = s.rast(**s.kw(s.col2))
        assert R.geometry_reuse_stats() == dict(reused=1, fallback={"first": 1})
        (out1[0].sum() + out2[0].sum()).backward()            # the unchanged backward on either `saved`
        g_on = [t.grad.clone() for t in (s.m3, s.sca, s.rot, s.op, s.col, s.m2)]
        with torch.no_grad():
            out3 = s.rast(**s.kw(s.col))                      # a third call over the same geometry reuses again
        assert R.geometry_reuse_stats() == dict(reused=2, fallback={"first": 1})
        assert (be.forwards, be.recomposites) == (1, 2)
        assert torch.equal(out3[0], out1[0]) and not torch.equal(out2[0], out1[0])
    with _installed(_double(), reuse=False) as R:
        f = _Scene()
        ref1, ref2 = f.rast(**f.kw(f.col)), f.rast(**f.kw(f.col2))
        assert R.geometry_reuse_stats() == dict(reused=0, fallback={})
        (ref1[0].sum() + ref2[0].sum()).backward()
        g_off = [t.grad.clone() for t in (f.m3, f.sca, f.rot, f.op, f.col, f.m2)]
        assert "_reuse_slot" not in f.rast.__dict__ and "_reuse_slot" in s.rast.__dict__
        with torch.no_grad():
            s.rast(**s.kw(s.col))                             # reuse is off again: the object lets go of what it held
        assert "_reuse_slot" not in s.rast.__dict__
    for a, b in zip(out1 + out2, ref1 + ref2):
        assert torch.equal(a, b)
    for a, b in zip(g_on, g_off):
        assert rel_l2(a.numpy(), b.numpy()) < ORDER_TOL


@pytest.mark.parametrize("name", list(BREAKS) + list(SECOND))
def test_every_condition_falls_back_on_its_own(name):
    be = _double()
    with _installed(be) as R:
        s = _Scene()
        s.out1 = s.rast(**s.kw(s.col))
        over, ctx, reason = {}, None, None
        if name in BREAKS:
            change, reason = BREAKS[name]
            change(s, R, be)
        else:
            over, ctx, reason = SECOND[name]
        with (ctx() if ctx is not None else contextlib.nullcontext()):
            out2 = s.rast(**s.kw(s.col2, **over))
        assert R.geometry_reuse_stats() == dict(reused=0, fallback={"first": 1, reason: 1}), R.geometry_reuse_stats()
        assert (be.forwards, be.recomposites) == (2, 0)
        use_filter = over.get("use_filter", True)
        flavour = s.rast.FLAVOUR
        ref = be.forward(s.rast.raster_settings, flavour, use_filter, s.m3.detach(), s.sca.detach(), s.rot.detach(),
                         s.op.detach().reshape(-1), s.col2.detach())
        for a, b in zip(out2, ref[:5]):
            assert torch.equal(a, b)


def test_other_object_cov3d_empty_and_plain_backend_fall_back():
    be = _double()
    with _installed(be) as R:
        s = _Scene()
        s.rast(**s.kw(s.col))
        s.wo.GaussianRasterizer(raster_settings=s.rs)(**s.kw(s.col2))            # another object, equal settings
        assert R.geometry_reuse_stats(reset=True) == dict(reused=0, fallback={"first": 2})
        cov = torch.eye(3)[None].repeat(len(s.m3), 1, 1) * 0.01
        cov6 = torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], dim=1)
        for c in (s.col, s.col2):
            s.rast(**s.kw(c, scales=None, rotations=None, cov3D_precomp=cov6))
        assert R.geometry_reuse_stats(reset=True) == dict(reused=0, fallback={"cov3D": 2})
        e = _Scene()
        z = lambda t: t.detach()[:0]
        for _ in range(2):
            e.rast(means3D=z(e.m3), means2D=z(e.m2), shs=None, colors_precomp=z(e.col), opacities=z(e.op), scales=z(e.sca),
                   rotations=z(e.rot), cov3D_precomp=None)
        assert R.geometry_reuse_stats(reset=True) == dict(reused=0, fallback={"empty": 2})
        assert be.recomposites == 0
    from oracle_backend import OracleBackend
    with _installed(OracleBackend()) as R:                                        # a backend without `recomposite`
        s = _Scene()
        a, b = s.rast(**s.kw(s.col)), s.rast(**s.kw(s.col))
        assert R.geometry_reuse_stats() == dict(reused=0, fallback={"no_recomposite": 2})
        assert torch.equal(a[0], b[0])


def test_no_grad_on_either_call_still_reuses():
    be = _double()
    with _installed(be) as R:
        s = _Scene()
        with torch.no_grad():
            s.rast(**s.kw(s.col))
        out2 = s.rast(**s.kw(s.col2))
        out2[0].sum().backward()
        assert s.op.grad is not None and s.col.grad is None
        with torch.no_grad():
            s.rast(**s.kw(s.col))
        assert R.geometry_reuse_stats() == dict(reused=2, fallback={"first": 1})


# ---- the reference's renderer with its depth pass ---------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "LoG")), reason="reference tree not present")
def test_reference_depth_pass_with_install_all_reuse(oracle_mod):
    """The reference's unmodified NaiveRendererAndLoss with render_depth=True (the configuration its documentation trains
    with) under log_amd.install_all(reuse_geometry=True): the second rasterizer call of each view reuses, and depth /
    height / accmap, the loss and every gradient are those of the run with reuse off."""
    import log_amd
    from log_amd import rasterizer as R, scenes
    from log_amd.compute_radius import compute_radius_module
    added = []
    if REF not in sys.path:
        sys.path.insert(0, REF)
        added.append(REF)
    stubs = {}
    if "cv2" not in sys.modules:
        stubs["cv2"] = types.ModuleType("cv2")
    sys.modules.update(stubs)
    patched = {}
    import oracle_backend
    old_backend = oracle_backend.install(_double())
    try:
        log_amd.install_compute_radius()
        from LoG.render.renderer import NaiveRendererAndLoss          # reference code, unmodified
        from LoG.model.base_gaussian import BaseGaussian              # reference code, unmodified
        from LoG.model.tensor_tree import TensorTree
        from LoG.model.counter import Counter
        from LoG.model.sparse_optimizer import SparseOptimizer
        from LoG.model.level_of_gaussian import LoG
        import LoG.render.renderer as ref_renderer
        patched = dict(traverse=TensorTree.traverse, update=Counter.update_by_output, step=SparseOptimizer.step,
                       load=SparseOptimizer.load_state_dict, get_all=LoG.get_all, torch=ref_renderer.torch)
        W = H = 96
        n = 1500
        cams = scenes.orbit_cameras(2, W=W, H=H, focal=110.0)
        sc = scenes.random_scene(n, seed=0, opacity=None, smax=0.06)
        sc["opacity"] = np.clip(sc["opacity"], 0.05, 0.95)
        keys = ["camera_center", "world_view_transform", "full_proj_transform", "K", "R", "T"]
        cam = {k: torch.tensor(np.stack([c[k] for c in cams[:1]])) for k in keys}
        for k in ("image_width", "image_height", "FoVx", "FoVy"):
            cam[k] = [c[k] for c in cams[:1]]
        torch.manual_seed(3)
        batch = {"camera": cam, "image": torch.rand(1, H, W, 3), "depth": torch.rand(1, H, W) + 0.5}

        def run(reuse):
            log_amd.install_all(reuse_geometry=reuse)
            R.geometry_reuse_stats(reset=True)
            model = BaseGaussian.create_from_record({k: v for k, v in sc.items()})
            renderer = NaiveRendererAndLoss(split="train", use_origin_render=False, background=[1., 1., 1.],
                                            render_depth=True)
            model.train()
            torch.manual_seed(5)                                       # append_depth_loss draws its patches
            out = renderer(batch, model)
            out["loss"].backward()
            grads = {k: getattr(model, k).grad.clone() for k in ("xyz", "colors", "scaling", "opacity", "rotation")}
            grads["viewspace"] = out["viewspace_points"][0].grad.clone()
            return out, grads, R.geometry_reuse_stats()

        off, g_off, st_off = run(False)
        on, g_on, st_on = run(True)
        assert st_off == dict(reused=0, fallback={})
        assert st_on == dict(reused=1, fallback={"first": 1}), st_on    # one view: its second call reused
        for k in ("depth", "height", "accmap"):
            assert torch.equal(on[k][0], off[k][0]), k
        assert float(off["accmap"][0].detach().max()) > 0.5
        assert torch.equal(on["render"], off["render"]) and torch.equal(on["loss"], off["loss"])
        for k in g_off:
            assert rel_l2(g_on[k].numpy(), g_off[k].numpy()) < ORDER_TOL and float(g_off[k].abs().sum()) > 0, k
    finally:
        R.set_geometry_reuse(False)
        oracle_backend.install(None if isinstance(old_backend, R.HipBackend) else old_backend)
        if patched:
            ref_renderer.torch = patched["torch"]
            TensorTree.traverse, Counter.update_by_output = patched["traverse"], patched["update"]
            SparseOptimizer.step, SparseOptimizer.load_state_dict = patched["step"], patched["load"]
            LoG.get_all = patched["get_all"]
            if hasattr(SparseOptimizer, "_lograst_load_state_dict"):
                del SparseOptimizer._lograst_load_state_dict
        for k in list(stubs) + ["LoG.cuda.compute_radius"]:
            sys.modules.pop(k, None)
        for p in added:
            sys.path.remove(p)


def test_forward_and_recomposite_leave_the_same_record():
    """HipBackend.forward and HipBackend.recomposite build `saved` with one function: the same keys whichever of the two made
    it and whatever was optional (no training buffers, no kept key buffer, the upstream flavour's missing point_weight), and
    among them every key that bench.py, the GPU tests and tools/ index."""
    from log_amd import _lib
    from log_amd.rasterizer import HipBackend
    n, H, W = 5, 4, 6
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8)
    view = _lib.LograstView()
    view.walk_form = _lib.FORM_ROWS

    def record(training, extras, keys):
        o = {"image": torch.zeros(3, H, W), "radii": torch.zeros(n, dtype=torch.int32)}
        if extras:
            o.update(pid=torch.zeros(H, W, dtype=torch.int32), pwp=torch.zeros(H, W), pw=torch.zeros(n))
        k = {"geom": u8(64 * n), "state": u8(256), "final_T": torch.zeros(H, W), "n_contrib": torch.zeros(H, W, dtype=torch.int32)}
        if training:
            k["bwd_scratch"] = torch.zeros(16 * n)
        masks = torch.zeros(32, dtype=torch.int64) if training else None
        out = HipBackend._finish(view, o, k, k["state"].view(torch.int32), torch.zeros(9, dtype=torch.int32), (0, 0), 7, 0, 9, 3,
                                 masks, 1 if training else 0, u8(144) if keys else None)
        assert out[0] is o["image"] and out[1] is o["radii"] and out[4] is o.get("pw")
        return out[-1]

    fwd = record(True, True, True)                       # a training forward of the fork under keep_keys(True)
    plain = record(False, False, False)                  # an upstream forward under no_grad
    assert set(fwd) == set(plain)
    assert set(fwd) >= {"n_contrib", "final_T", "geom", "radii", "plist", "state", "hit_masks", "hit_mask_form", "point_weight",
                        "keys", "bwd_scratch", "tile_rows", "instances", "walk_form_pin", "capacity", "max_len", "fwd_walk_form"}
    assert all(plain[k] is None for k in ("keys", "bwd_scratch", "hit_masks", "point_weight")) and plain["hit_mask_form"] == 0
    assert all(fwd[k] is not None for k in ("keys", "bwd_scratch", "hit_masks", "point_weight")) and fwd["hit_mask_form"] == 1
    assert fwd["geom"].dtype == torch.float32 and fwd["state"].dtype == torch.int32 and fwd["fwd_walk_form"] == _lib.FORM_ROWS
    # the autograd node keeps nothing of the record's layout: a backend may hand it any object (tests/oracle_backend.py: a tuple)
    import inspect
    from log_amd import rasterizer as R
    assert "ctx.saved[" not in inspect.getsource(R._RasterizeGaussians) and ".saved.get" not in inspect.getsource(R)
