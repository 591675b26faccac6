"""The device initialisation pass (log_amd/init_pass.py -> log_amd/csrc/init.hip) against the numpy restatement
tests/init_ref.py in mode "fixed" (the kernel's own op sequences: oracle.lod_radius on the raw rows, lr_exp_any through
libm's fmaf, 3.f / r as one division) and the fixture recorded from the reference's own LoG.init
(tests/golden/init_log.npz; tests/test_init_pass_cpu.py holds the restatement to it).  No test here reads the reference
tree: the drop-ins run on stand-in objects that carry the attributes the reference's LoG / GaussianPoint / Counter carry.

Everything is compared bit for bit: values as uint32 words (so a NaN start value has to survive with its payload), flags
exactly."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import init_ref as IR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ACT = types.SimpleNamespace(scaling_activation=torch.exp, scaling_inverse_activation=torch.log,
                             rotation_activation=torch.nn.functional.normalize)
_CACHE = {}
START_RANGE = (3e-5, 1e-2)     # where radius3d falls for these scenes and cameras: start values bind for some rows only


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)       # a copy: the cached cases are read-only


def cpu(t):
    return t.detach().cpu().numpy()


def rasterizer(proj, view, W, H, tfx, tfy, scale_modifier=1.0):
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    campos = np.linalg.inv(np.asarray(view, np.float64))[3, :3].astype(np.float32)
    rs = GaussianRasterizationSettings(
        image_height=int(H), image_width=int(W), tanfovx=tfx, tanfovy=tfy, bg=torch.ones(3, device=DEV),
        scale_modifier=scale_modifier, viewmatrix=dev(view), projmatrix=dev(proj), sh_degree=0, campos=dev(campos),
        prefiltered=False, debug=False)
    return GaussianRasterizer(raster_settings=rs)


def ref_args(rast):
    """The camera of a rasterizer as tests/init_ref.py takes it."""
    rs = rast.raster_settings
    return (cpu(rs.projmatrix), cpu(rs.viewmatrix), rs.image_width / (2.0 * rs.tanfovx),
            rs.image_height / (2.0 * rs.tanfovy), rs.tanfovx, rs.tanfovy)


def orbit_rasterizers(n):
    from log_amd import scenes
    cams = scenes.orbit_cameras(n, radius=1.1, W=160, H=120, focal=176.0)
    return cams, [rasterizer(c["full_proj_transform"], c["world_view_transform"], 160, 120, math.tan(c["FoVx"] * 0.5),
                             math.tan(c["FoVy"] * 0.5)) for c in cams]


def renderer():
    """What the drop-ins ask of a renderer: prepare_camera(batch, 0, background) -> (camera, rasterizer, background); the
    batch of these tests carries its rasterizer."""
    return types.SimpleNamespace(background=None, prepare_camera=lambda batch, bn, bg: ({}, batch["rasterizer"], bg))


def stand_in(xyz, scaling, rotation, radius3d_min):
    g = types.SimpleNamespace(xyz=dev(xyz), scaling=dev(scaling), rotation=dev(rotation), activation=_ACT, xyz_scale=1.0)
    return types.SimpleNamespace(gaussian=g, counter=types.SimpleNamespace(radius3d_min=dev(radius3d_min)), num_views=0)


def case(P, V):
    """-> (xyz, scaling, rotation, start, rasterizers, [(valid, radius3d_min) after each view] in mode "fixed"), computed
    once.  Unit cube, raw scales log-uniform over two decades, randn quaternions, start values log-uniform across the range
    the results have.  From 255 rows on, rows 0..7 are planted.  In front of every camera: 0 a NaN raw scale, 1 raw scale
    +200, 2 raw scale -200, 3 a zero quaternion, 6 a NaN start value (minimum(NaN, x) stays NaN).  4: a point at the centre
    of camera 0.  5: a point straight behind camera 0 (the radius rule has no depth cull: it is valid).  7: a NaN start
    value with a payload on a row far above every camera, which no view may touch."""
    if (P, V) not in _CACHE:
        rng = np.random.default_rng([P, V, 0x1217])
        cams, rasts = orbit_rasterizers(8)
        cams, rasts = cams[:V], rasts[:V]
        xyz = (rng.random((P, 3)) - 0.5).astype(np.float32)
        scaling = rng.uniform(np.log(0.002), np.log(0.2), (P, 3)).astype(np.float32)
        rotation = rng.standard_normal((P, 4)).astype(np.float32)
        start = np.exp(rng.uniform(np.log(START_RANGE[0]), np.log(START_RANGE[1]), P)).astype(np.float32)
        if P >= 255:
            c0 = cams[0]["camera_center"].astype(np.float32)
            for k in (0, 1, 2, 3, 6):
                xyz[k] = (0.05 * k - 0.1, 0.02, -0.03)
            scaling[0, :] = np.nan
            scaling[1, :] = 200.0
            scaling[2, :] = -200.0
            rotation[3, :] = 0.0
            xyz[4] = c0
            xyz[5] = (1.5 * c0).astype(np.float32)
            xyz[7] = (0.0, 0.0, 50.0)
            start[6] = np.nan
            start[7] = np.array([0x7FC01234], np.uint32).view(np.float32)[0]
        want = IR.log_init("fixed", xyz, scaling, rotation, [ref_args(r) for r in rasts], start)
        for a in (xyz, scaling, rotation, start):
            a.setflags(write=False)
        _CACHE[(P, V)] = (xyz, scaling, rotation, start, rasts, want)
    return _CACHE[(P, V)]


@pytest.mark.parametrize("V", [1, 3, 8])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 5000])
def test_radius3d_min_sizes_and_planted_rows(P, V):
    """Partial and whole workgroups, more than one, no rows at all; one camera and several.  radius3d_min after all V views
    in one launch; with V = 1 also Gaussian.init_radius3d's flag and radius3d."""
    from log_amd import init_pass
    xyz, scaling, rotation, start, rasts, want = case(P, V)
    rmin = dev(start)
    out = init_pass.update_radius3d_min(dev(xyz), dev(scaling), dev(rotation), rasts, rmin)
    assert out is rmin
    final = want[-1][1] if V else start
    assert IR.same_bits(cpu(rmin), final), (P, V)
    if P >= 255:
        first = want[0][0]
        assert first[[0, 1, 2, 3, 5, 6]].all() and not np.any([v[7] for v, _ in want])
        got = cpu(rmin)
        assert np.isnan(got[6]) and got[7:8].view(np.uint32)[0] == 0x7FC01234
        assert 0.05 < np.mean(final.view(np.uint32) == start.view(np.uint32)) and np.mean(final < start) > 0.05
    if V == 1:
        model = stand_in(xyz, scaling, rotation, start)
        valid, radius3d = init_pass.init_radius3d(model.gaussian, {"rasterizer": rasts[0]}, renderer())
        assert valid.dtype == torch.bool and valid.shape == (P,) and radius3d.dtype == torch.float32
        w_valid, w_r3d = IR.init_radius3d("fixed", xyz, scaling, rotation, ref_args(rasts[0]))
        assert np.array_equal(cpu(valid), w_valid) and IR.same_bits(cpu(radius3d), w_r3d), P
        if P >= 255:
            assert not w_valid.all() and IR.same_bits(w_r3d[~w_valid], IR.exp_any(scaling[~w_valid, 0]))


def test_grid_stride_rows_beyond_the_grid():
    """More rows than the grid has threads (2048 workgroups of 256): the second trip of the grid-stride loop.  Rows repeat
    the 5000-row case, so its reference serves (a row's result depends on that row alone)."""
    from log_amd import init_pass
    xyz, scaling, rotation, start, rasts, want = case(5000, 3)
    P = 2048 * 256 + 257
    idx = np.arange(P) % 5000
    rmin = dev(start[idx])
    init_pass.update_radius3d_min(dev(xyz[idx]), dev(scaling[idx]), dev(rotation[idx]), rasts, rmin)
    assert IR.same_bits(cpu(rmin), want[-1][1][idx])


def _count_launches(monkeypatch):
    from log_amd import init_pass
    views = []
    launch = init_pass._launch

    def counted(device, P, xyz, scaling, rotation, table, *rest):
        views.append(int(table.shape[0]))
        return launch(device, P, xyz, scaling, rotation, table, *rest)
    monkeypatch.setattr(init_pass, "_launch", counted)
    return views


def test_batching_does_not_change_a_bit(monkeypatch):
    """Eight cameras in one launch, eight launches of one, and flushes of 3, 3 and 2: the same bits; num_views is 8."""
    from log_amd import init_pass
    xyz, scaling, rotation, start, rasts, want = case(5000, 8)
    views = _count_launches(monkeypatch)
    rmin = dev(start)
    init_pass.update_radius3d_min(dev(xyz), dev(scaling), dev(rotation), rasts, rmin)
    assert views == [8] and IR.same_bits(cpu(rmin), want[-1][1])
    try:
        for k, launches in ((1, [1] * 8), (3, [3, 3, 2]), (8, [8])):
            del views[:]
            init_pass.set_views_per_launch(k)
            model = stand_in(xyz, scaling, rotation, start)
            for i, r in enumerate(rasts):
                init_pass.log_init(model, renderer(), {"rasterizer": r}, i)
                if k == 1:           # the state after every call is the reference's
                    assert IR.same_bits(cpu(model.counter.radius3d_min), want[i][1]), i
            if k == 3:
                assert views == [3, 3] and not IR.same_bits(cpu(model.counter.radius3d_min), want[-1][1])
            init_pass.flush(model)
            init_pass.flush(model)          # nothing pending: nothing happens
            assert views == launches and model.num_views == 8, k
            assert IR.same_bits(cpu(model.counter.radius3d_min), cpu(rmin)), k
    finally:
        init_pass.set_views_per_launch(1)


def _fixture_rasterizers(fx):
    out = []
    for v in IR.views(fx):
        W, H = fx[f"{v}_wh"]
        tfx, tfy = (float(x) for x in fx[f"{v}_tanfov"])
        out.append(rasterizer(fx[f"{v}_proj"], fx[f"{v}_view"], W, H, tfx, tfy))
    return out


def _reference_at_init_final(self):
    """What the reference's LoG.at_init_final does to the model (its prints aside), for a stand-in model."""
    floor = torch.log(self.counter.radius3d_min)[:, None].repeat(1, 3)
    self.gaussian.scaling = torch.maximum(self.gaussian.scaling, floor)


def test_fixture_on_a_stand_in_model():
    """The reference's own run: after every view the flags are the fixture's and the values are mode "fixed"'s;
    at_init_final launches what is pending and leaves scaling = max(scaling, log(radius3d_min))."""
    from log_amd import init_pass
    fx = {k: v for k, v in IR.load("log").items()}
    P = fx["xyz"].shape[0]
    rasts = _fixture_rasterizers(fx)
    want = IR.log_init("fixed", fx["xyz"], fx["scaling"], fx["rotation"], [ref_args(r) for r in rasts], fx["radius3d_min_start"])
    model = stand_in(fx["xyz"], fx["scaling"], fx["rotation"], fx["radius3d_min_start"])
    rnd = renderer()
    for i, (v, r) in enumerate(zip(IR.views(fx), rasts)):
        valid, _ = init_pass.init_radius3d(model.gaussian, {"rasterizer": r}, rnd)
        assert np.array_equal(cpu(valid), IR.bits(fx, f"{v}_valid", P)), v
        init_pass.log_init(model, rnd, {"rasterizer": r}, i)
        assert IR.same_bits(cpu(model.counter.radius3d_min), want[i][1]), v
    assert model.num_views == int(fx["num_views"])
    # the same views, five to a launch: four are left to at_init_final, the 1080p one among them
    batched = stand_in(fx["xyz"], fx["scaling"], fx["rotation"], fx["radius3d_min_start"])
    try:
        init_pass.set_views_per_launch(5)
        for i, r in enumerate(rasts):
            init_pass.log_init(batched, rnd, {"rasterizer": r}, i)
        assert getattr(batched, init_pass._PENDING).table.count == 4
        assert IR.same_bits(cpu(batched.counter.radius3d_min), want[4][1]) and not IR.same_bits(want[4][1], want[-1][1])
        with init_pass.dropins.substituted(at_init_final=_reference_at_init_final):
            init_pass.at_init_final(batched)
    finally:
        init_pass.set_views_per_launch(1)
    assert getattr(batched, init_pass._PENDING) is None and batched.num_views == 9
    assert IR.same_bits(cpu(batched.counter.radius3d_min), want[-1][1])
    floor = torch.log(batched.counter.radius3d_min)[:, None].repeat(1, 3)
    assert torch.equal(batched.gaussian.scaling, torch.maximum(dev(fx["scaling"]), floor))         # on the flushed result
    got = cpu(batched.gaussian.scaling)
    assert (got > fx["scaling"]).any() and (got == fx["scaling"]).any()
    assert np.abs(got - np.maximum(fx["scaling"], np.log(want[-1][1].astype(np.float64))[:, None])).max() < 1e-5


@pytest.mark.parametrize("k", [1, 4])
def test_no_host_synchronisation(k):
    """LoG.init over all fixture cameras under torch's synchronisation check: no blocking call, no read-back."""
    from log_amd import init_pass
    fx = {k_: v for k_, v in IR.load("log").items()}
    rasts = _fixture_rasterizers(fx)
    model = stand_in(fx["xyz"], fx["scaling"], fx["rotation"], fx["radius3d_min_start"])
    rnd = renderer()
    init_pass.log_init(model, rnd, {"rasterizer": rasts[0]}, 0)         # warm-up: the first launch loads the code object
    torch.cuda.synchronize()
    model = stand_in(fx["xyz"], fx["scaling"], fx["rotation"], fx["radius3d_min_start"])
    init_pass.reset_stats()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        init_pass.set_views_per_launch(k)
        torch.cuda.set_sync_debug_mode("error")
        for i, r in enumerate(rasts):
            init_pass.log_init(model, rnd, {"rasterizer": r}, i)
        init_pass.flush(model)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
        init_pass.set_views_per_launch(1)
    st = init_pass.stats()
    assert st["readbacks"] == {} and st["fallbacks"] == {} and st["calls"] == {"log_init": len(rasts)}
    want = IR.log_init("fixed", fx["xyz"], fx["scaling"], fx["rotation"], [ref_args(r) for r in rasts], fx["radius3d_min_start"])
    assert IR.same_bits(cpu(model.counter.radius3d_min), want[-1][1])


def test_scale_modifier_falls_back():
    from log_amd import init_pass
    xyz, scaling, rotation, start, rasts, want = case(257, 1)
    rs = rasts[0].raster_settings
    scaled = rasterizer(cpu(rs.projmatrix), cpu(rs.viewmatrix), rs.image_width, rs.image_height, rs.tanfovx, rs.tanfovy,
                        scale_modifier=1.7)
    model = stand_in(xyz, scaling, rotation, start)
    calls = []
    init_pass.reset_stats()
    with init_pass.dropins.substituted(log_init=lambda *a: calls.append(a)):
        init_pass.log_init(model, renderer(), {"rasterizer": scaled}, 0)
    assert len(calls) == 1 and calls[0][0] is model and model.num_views == 0
    assert init_pass.stats()["fallbacks"] == {("log_init", "scale_modifier != 1"): 1}
    assert IR.same_bits(cpu(model.counter.radius3d_min), start) and getattr(model, init_pass._PENDING, None) is None
    with pytest.raises(ValueError, match="scale_modifier"):
        init_pass.update_radius3d_min(model.gaussian.xyz, model.gaussian.scaling, model.gaussian.rotation, [scaled],
                                      model.counter.radius3d_min)


def test_a_model_changed_while_views_are_pending_raises():
    from log_amd import _lib, init_pass
    xyz, scaling, rotation, start, rasts, want = case(257, 3)
    rnd = renderer()
    try:
        init_pass.set_views_per_launch(4)
        model = stand_in(xyz, scaling, rotation, start)
        init_pass.log_init(model, rnd, {"rasterizer": rasts[0]}, 0)
        model.gaussian.scaling.add_(0.1)                                 # in place: the version counter moves
        with pytest.raises(_lib.LograstError, match="changed while 1 view"):
            init_pass.flush(model)
        with pytest.raises(_lib.LograstError, match="changed while 1 view"):
            init_pass.log_init(model, rnd, {"rasterizer": rasts[1]}, 1)
        model = stand_in(xyz, scaling, rotation, start)
        init_pass.log_init(model, rnd, {"rasterizer": rasts[0]}, 0)
        model.gaussian.scaling = model.gaussian.scaling.clone()          # another buffer: the pointer moves
        with pytest.raises(_lib.LograstError, match="changed while 1 view"):
            init_pass.flush(model)
        assert IR.same_bits(cpu(model.counter.radius3d_min), start)      # nothing was launched
    finally:
        init_pass.set_views_per_launch(1)
