"""Steps over several views on the GPU: lograst_activate_backward_accumulate and lograst_accumulated_adam held, bit for bit, to
what the PARENT's kernels give -- lograst_activate_backward + index_add_ per view in order for the sums, lograst_sparse_adam
over arange(P) with seen > 0 as the flag for the step -- then to the reference's fixture within the step kernels' bound, and
driven through log_amd.multi_view on stand-ins of the reference's classes (eager, under torch's synchronisation check, and
captured in a graph)."""
import math
import sys
import types

import numpy as np
import pytest
import torch

import multi_view_ref as mref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("xyz", "scaling", "opacity", "rotation", "colors", "shs")
WIDTH = {"xyz": 3, "scaling": 3, "opacity": 1, "rotation": 4, "colors": 3}
SHAPES = [(n, P) for n in (0, 1, 255, 256, 257, 3000) for P in (1, 257, 5000)]
SH = [(0, 0), (3, 1), (15, 2), (15, 3)]
SH_SCHEDULE = [(15, 0), (15, 1), (8, 1)]     # active degree below the stored one, as a training run starts (the sums only)
B1, B2, EPS = 0.9, 0.999, 1e-15


def _bits(t):
    return t.contiguous().view(torch.int32)


def _view(gen, n, P, K, live=True):
    """One view of n parameter rows + 3 node rows: raw rows, upstream gradients, index (unique inside [0, P); what does not fit
    the model lies outside it, on both sides), radii with zeros and negatives; planted: a zero quaternion, raw scales +-80."""
    rows = n + 3
    r = lambda *s: torch.randn(*s, generator=gen, device=DEV)
    raw = {"xyz": r(rows, 3), "scaling": r(rows, 3) - 3.0, "opacity": r(rows, 1) * 2, "rotation": r(rows, 4), "colors": r(rows, 3)}
    if K:
        raw["shs"] = r(rows, K, 3) * 0.3
    raw["rotation"][0] = 0.0
    raw["scaling"][1 % rows] = 80.0
    raw["scaling"][2 % rows] = -80.0
    # 16-byte aligned quaternion rows, as gather_activate carves them
    assert raw["rotation"].data_ptr() % 16 == 0
    ups = tuple(r(rows, w) for w in (3, 3, 1, 4, 3))
    perm = torch.randperm(max(P, 1), generator=gen, device=DEV)[:rows]
    extra = rows - int(perm.numel())
    if extra > 0:
        off = torch.arange(extra, device=DEV)
        perm = torch.cat([perm, torch.where(off % 2 == 0, P + off, -1 - off)])
        perm = perm[torch.randperm(rows, generator=gen, device=DEV)]
    radii = torch.randint(-2, 6, (rows,), generator=gen, device=DEV, dtype=torch.int32)
    if not live:
        radii = -radii.abs()
    campos = torch.tensor([0.3, -2.5, 0.8], device=DEV)
    return raw, ups, perm.to(torch.int64), radii, campos


def _targets(P, K, degree, row_major, gen, sentinel=True):
    """-> (flat bucket of log_amd.dist, {key: its block}) pre-filled with random bits the kernels must keep where no view goes."""
    from log_amd.dist import _Flat
    from log_amd.multi_view import KEY_TO_FLAT
    flat = _Flat(P, DEV, sh_coeffs=K, row_major=row_major)
    if sentinel:
        flat.flat.copy_(torch.randn(flat.flat.shape, generator=gen, device=DEV))
    keys = [k for k in KEYS if k != "shs" or (K and degree > 0)]
    return flat, {k: flat.alias[KEY_TO_FLAT[k]] for k in keys}


def _parent_add(R, view, n, degree, want, seen):
    """The parent's lograst_activate_backward, then index_add_ of the live rows (unique: one fp32 add per element)."""
    raw, ups, index, radii, campos = view
    P = int(seen.numel())
    g = R._backend.activate_backward(raw, n, degree, campos, ups[1], ups[2], ups[3], ups[4]) if n else {}
    g["xyz"] = ups[0][:n]
    idx = index[:n]
    live = (radii[:n] > 0) & (idx >= 0) & (idx < P)
    rows = idx[live]
    for k, t in want.items():
        gk = g[k][live] if n else torch.zeros((0,) + tuple(t.shape[1:]), device=DEV)
        t.index_add_(0, rows, gk.reshape((-1,) + tuple(t.shape[1:])))
    seen.index_add_(0, rows, torch.ones_like(rows, dtype=torch.int32))
    return int(rows.numel())


# Keys without a target: the kernel must neither load their inputs nor touch their blocks.  The smallest shapes of SHAPES
# that have a row, up to the first that fills a workgroup's four waves but for a lane.  Radii are positive with probability
# 5 / 8 and two of the three views are live: 2 x 255 x 5 / 8 = 319 live rows expected at (255, 257), +- 11.
_SUMS_LEFT_OUT = ("opacity", "rotation")
_SUMS_SMALLEST = [(1, 1), (1, 257), (255, 257)]


@pytest.mark.parametrize("K,degree,row_major,left_out", [
    pytest.param(K, degree, row_major, (), id="%d-%d-%s" % (K, degree, name))
    for name, row_major in (("attribute_major", False), ("row_major", True)) for K, degree in SH + SH_SCHEDULE
] + [pytest.param(15, 2, False, _SUMS_LEFT_OUT, id="15-2-attribute_major-no_opacity_no_rotation")])
def test_sums_equal_the_parents_backward_added_by_index(K, degree, row_major, left_out):
    from log_amd import multi_view as mv, rasterizer as R
    gen = torch.Generator(device=DEV).manual_seed(17 * K + degree + int(row_major))
    total_live = 0
    for n, P in (_SUMS_SMALLEST if left_out else SHAPES):
        got_flat, got = _targets(P, K, degree, row_major, gen)
        want_flat, want = _targets(P, K, degree, row_major, gen, sentinel=False)
        for k in left_out:                                                          # their blocks keep the sentinel's bits
            del got[k], want[k]
        want_flat.flat.copy_(got_flat.flat)
        seen, seen_want = (torch.zeros(P, dtype=torch.int32, device=DEV) for _ in range(2))
        for v in range(3):
            view = _view(gen, n, P, K, live=(v != 1 or n == 3000))          # the second view of most shapes has no live row
            raw, ups, index, radii, campos = view
            mv.accumulate(raw, n, degree, campos, ups, index, radii, got, seen)
            total_live += _parent_add(R, view, n, degree, want, seen_want)
            assert torch.equal(_bits(got_flat.flat), _bits(want_flat.flat)), (n, P, v)       # sums AND every untouched float
            assert torch.equal(seen, seen_want), (n, P, v)
    assert total_live > (200 if left_out else 5000)


def _optimizer_state(P, K, gen, amsgrad):
    r = lambda *s: torch.randn(*s, generator=gen, device=DEV)
    shapes = {k: (P, w) for k, w in WIDTH.items()}
    if K:
        shapes["shs"] = (P, K, 3)
    model = {k: r(*s) for k, s in shapes.items()}
    m1 = {k: r(*s) * 0.01 for k, s in shapes.items()}
    m2 = {k: r(*s).abs() * 1e-4 for k, s in shapes.items()}
    mx = {k: r(*s).abs() * 1e-4 for k, s in shapes.items()} if amsgrad else None
    return model, m1, m2, mx


LRS = {"xyz": 1.6e-4, "scaling": 5e-3, "opacity": 0.05, "rotation": 1e-3, "colors": 2.5e-3, "shs": 1.25e-4}


@pytest.mark.parametrize("amsgrad,skip", [(False, None), (True, None), (False, "opacity")], ids=["adam", "amsgrad", "null_key"])
@pytest.mark.parametrize("row_major", [False, True], ids=["attribute_major", "row_major"])
@pytest.mark.parametrize("K,degree", SH)
def test_step_equals_the_parents_sparse_adam_over_all_rows(K, degree, row_major, amsgrad, skip):
    from log_amd import multi_view as mv, rasterizer as R
    gen = torch.Generator(device=DEV).manual_seed(5 + K + int(row_major) + 2 * int(amsgrad))
    steps = 7
    bc1, bc2 = 1 - B1 ** steps, 1 - B2 ** steps
    stepped = 0
    for n, P in SHAPES:
        flat, acc = _targets(P, K, degree, row_major, gen, sentinel=False)
        seen = torch.zeros(P, dtype=torch.int32, device=DEV)
        for v in range(2):
            raw, ups, index, radii, campos = _view(gen, n, P, K)
            mv.accumulate(raw, n, degree, campos, ups, index, radii, acc, seen)
        model, m1, m2, mx = _optimizer_state(P, K, gen, amsgrad)
        keys = [k for k in acc if k != skip]
        clone = lambda d: None if d is None else {k: v.clone() for k, v in d.items()}
        w_model, w_m1, w_m2, w_mx = clone(model), clone(m1), clone(m2), clone(mx)
        flag = seen > 0
        # the parent: lograst_sparse_adam over every row, the flag selecting
        R._backend.sparse_adam(torch.arange(P, device=DEV), flag,
                               [(w_model[k], w_model[k].clone(), acc[k].contiguous().clone(), w_m1[k], w_m2[k],
                                 w_mx[k] if amsgrad else None, LRS[k] / bc1) for k in keys], B1, B2, math.sqrt(bc2), EPS)
        kept = {k: acc[k].clone() for k in acc}
        moved = torch.full((P,), 7, dtype=torch.uint8, device=DEV)
        entries = {k: (model[k], acc[k], m1[k], m2[k], mx[k] if amsgrad else None, LRS[k] / bc1) for k in keys}
        mv.step(seen, entries, B1, B2, math.sqrt(bc2), EPS, moved)
        for k in model:
            for name, a, b in (("model", model, w_model), ("exp_avg", m1, w_m1), ("exp_avg_sq", m2, w_m2)) + \
                    ((("max_exp_avg_sq", mx, w_mx),) if amsgrad else ()):
                assert torch.equal(_bits(a[k]), _bits(b[k])), (n, P, k, name)
        assert torch.equal(moved, flag.to(torch.uint8)) and int(seen.abs().sum()) == 0, (n, P)
        for k in acc:
            if k == skip:
                assert torch.equal(_bits(acc[k]), _bits(kept[k])), (n, P, k)          # a NULL key: its sums are not touched
            else:
                assert float(acc[k].abs().sum()) == 0.0, (n, P, k)
                if int(flag.sum()):
                    assert float(kept[k][flag].abs().sum()) > 0
        stepped += int(flag.sum())
        # a second step with nothing seen changes no bit
        everything = [flat.flat] + [d[k] for d in (model, m1, m2) + ((mx,) if amsgrad else ()) for k in d]
        before = [t.clone() for t in everything]
        mv.step(seen, entries, B1, B2, math.sqrt(bc2), EPS, moved)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(everything, before)), (n, P)
        assert int(moved.sum()) == 0 and int(seen.abs().sum()) == 0
    assert stepped > 3000


def test_sums_and_step_against_the_reference_fixture():
    """The three views of tests/golden/multi_view_log.npz through the two kernels: the sums of the rows some view saw and the
    stepped model and moments within 8 * (|ref32 - ref64| + 2^-24 S) of the float64 restatement; every other row keeps its
    bits."""
    from log_amd import multi_view as mv, rasterizer as R
    bufs, m1, m2, views, g = mref.load()
    degree, steps = int(g["degree"]), int(g["step"])
    dev = lambda d: {k: v.to(DEV) for k, v in d.items()}
    model, e1, e2 = dev(bufs), dev(m1), dev(m2)
    P, K = model["xyz"].shape[0], model["shs"].shape[1]
    flat, acc = _targets(P, K, degree, False, None, sentinel=False)
    seen = torch.zeros(P, dtype=torch.int32, device=DEV)
    for v in views:
        index = torch.cat([v["index"], v["index_node"]]).to(DEV)
        raw, _act = R._backend.gather_activate(index, model, degree, v["campos"].to(DEV))
        ups = tuple(v["ups"][k].to(DEV) for k in ("xyz", "scaling", "opacity", "rotation", "colors"))
        mv.accumulate(raw, int(v["index"].shape[0]), degree, v["campos"].to(DEV), ups, index, v["radii"].to(DEV), acc, seen)
    assert torch.equal(seen.cpu(), torch.from_numpy(g["seen"]))
    rows = torch.from_numpy(g["rows"]).to(DEV)
    sums = {k: acc[k][rows].cpu() for k in acc}
    bc1, bc2 = 1 - B1 ** steps, 1 - B2 ** steps
    entries = {k: (model[k], acc[k], e1[k], e2[k], None, float(g["lr_" + k]) / bc1) for k in acc}
    mv.step(seen, entries, B1, B2, math.sqrt(bc2), EPS)
    stepped = {k: (model[k][rows].cpu(), e1[k][rows].cpu(), e2[k][rows].cpu()) for k in acc}
    worst = mref.check_against_fixture(sums, stepped, g)
    print(f"kernels vs float64 restatement on the fixture: largest error / bound {worst:.3f}")
    rest = torch.ones(P, dtype=torch.bool)
    rest[g["rows"]] = False
    for k in bufs:
        for got, want in ((model, bufs), (e1, m1), (e2, m2)):
            assert torch.equal(got[k].cpu()[rest], want[k][rest]), k


# ---- through log_amd.multi_view, the reference's classes stood in ---------------------------------------------------------

class _Render(torch.autograd.Function):
    """Stands where the rasterizer does: its backward publishes the render's radii for the rows it was given, as the
    rasterizer's backward node does, and hands fixed gradients to the five activated inputs."""

    @staticmethod
    def forward(ctx, radii, ups, xyz, scaling, opacity, rotation, colors):
        ctx.radii, ctx.ups, ctx.xyz = radii, ups, xyz
        return sum((t * u).sum() for t, u in zip((xyz, scaling, opacity, rotation, colors), ups))

    @staticmethod
    def backward(ctx, g):
        from log_amd import rasterizer as R
        R._publish_backward_view(ctx.radii, ctx.xyz)
        return (None, None) + tuple(u * g for u in ctx.ups)


class _World:
    """A model of P rows in the shape LoG.step and LoG.get_all read, as an instance of a stand-in LoG class that
    log_amd.multi_view.install patches, + two views with fixed selections, radii and upstream gradients."""

    def __init__(self, LoG, P=5000, n=1200, K=3, degree=1):
        gen = torch.Generator(device=DEV).manual_seed(3)
        model, m1, m2, _ = _optimizer_state(P, K, gen, False)
        model["scaling"] -= 3.0
        self.P, self.n, self.degree = P, n, degree
        keys = ["scaling", "colors", "xyz", "opacity", "rotation", "shs"]
        self.bufs = {k: model[k] for k in keys}
        g = types.SimpleNamespace(keys=keys, active_sh_degree=degree, visibility_flag=None,
                                  items=lambda: ((k, self.bufs[k]) for k in keys),
                                  activation=types.SimpleNamespace(scaling_inverse_activation=torch.log), **self.bufs)
        opt = types.SimpleNamespace(global_steps=torch.tensor(4.0, device=DEV), _lograst_steps=4, lr_dict=dict(LRS),
                                    exp_avg=m1, exp_avg_sq=m2, use_amsgrad=False, xyz_lr=None, optimize_keys=list(keys),
                                    xyz_scheduler_args=lambda st: 1.6e-4 * 0.99 ** st, scaling_scheduler_args=lambda st: 5e-3)
        counter = types.SimpleNamespace(radius3d_min=torch.full((P,), math.exp(-3.2), device=DEV),
                                        radius3d_max=torch.full((P,), math.exp(-2.9), device=DEV))
        self.log = LoG()
        self.log.__dict__.update(gaussian=g, optimizer=opt, counter=counter, fix_parent=True, training=True, base_iter=1,
                                 use_view_correction=False, lr=None)
        self.views = []
        for v in range(2):
            raw, ups, index, radii, campos = _view(gen, n, P, K)
            self.views.append((index[:n].clone(), index[n:].clone(), radii, ups, {"camera_center": campos}))

    def tensors(self):
        o = self.log.optimizer
        return [self.bufs[k] for k in self.bufs] + [o.exp_avg[k] for k in self.bufs] + [o.exp_avg_sq[k] for k in self.bufs] + \
               [o.global_steps]

    def one_view(self, v):
        from log_amd import get_all
        index, index_node, radii, ups, camera = self.views[v]
        g = self.log.gaussian
        g.visibility_flag = {"index": index, "index_node": index_node, "flag_vis": radii > 0}
        act = get_all.get_all(self.log, camera, None)
        loss = _Render.apply(radii, ups, act["xyz"], act["scaling"], act["opacity"], act["rotation"], act["colors"])
        loss.backward()
        params = g.visibility_flag["params"]
        assert all(p.grad is None for p in params.values())
        self.log.step()


@pytest.fixture()
def stand_in_log():
    """A module LoG.model.level_of_gaussian with a class LoG whose step nobody should reach."""
    from log_amd import get_all, multi_view as mv

    class LoG:
        visibility_flag = property(lambda self: self.gaussian.visibility_flag)

        def step(self):
            raise AssertionError("the reference's step ran")

        def clamp_scale(self, index):
            raise AssertionError("the reference's clamp_scale ran")

    names = ("LoG", "LoG.model", "LoG.model.level_of_gaussian")
    old = {k: sys.modules.get(k) for k in names}
    for k in names:
        sys.modules[k] = types.ModuleType(k)
    sys.modules["LoG.model.level_of_gaussian"].LoG = LoG
    mv.dropins._saved.clear()
    mv.reset_stats()
    try:
        yield LoG
    finally:
        mv.uninstall()
        mv.dropins._saved.clear()
        get_all._multi_view = None
        for k, m in old.items():
            if m is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = m


def test_two_views_through_the_model_are_the_kernel_level_sequence(stand_in_log):
    """install(views_per_step=2): two views, two calls of step -> the bits of accumulate, accumulate, step, clamp on a copy;
    no host synchronisation in backward or step; the same sequence captured in a graph replays to the same bits."""
    from log_amd import _lib, multi_view as mv, rasterizer as R
    assert mv.install(views_per_step=2) is stand_in_log
    w = _World(stand_in_log)
    start = [t.clone() for t in w.tensors()]
    # ---- the kernel-level sequence on copies
    model = {k: v.clone() for k, v in w.bufs.items()}
    e1 = {k: v.clone() for k, v in w.log.optimizer.exp_avg.items()}
    e2 = {k: v.clone() for k, v in w.log.optimizer.exp_avg_sq.items()}
    flat, acc = _targets(w.P, 3, w.degree, False, None, sentinel=False)
    seen = torch.zeros(w.P, dtype=torch.int32, device=DEV)
    for index, index_node, radii, ups, camera in w.views:
        raw, _ = R._backend.gather_activate(torch.cat([index, index_node]), model, w.degree, camera["camera_center"])
        mv.accumulate(raw, w.n, w.degree, camera["camera_center"], ups, index, radii, acc, seen)
    steps = 5
    bc1, bc2 = 1 - B1 ** steps, 1 - B2 ** steps
    lr = dict(LRS, xyz=1.6e-4 * 0.99 ** steps)
    moved = torch.zeros(w.P, dtype=torch.uint8, device=DEV)
    mv.step(seen, {k: (model[k], acc[k], e1[k], e2[k], None, lr[k] / bc1) for k in acc}, B1, B2, math.sqrt(bc2), EPS, moved)
    rows = torch.arange(w.P, device=DEV)
    _lib.check(_lib.lib().lograst_clamp_scale(w.P, R._ptr(rows), R._ptr(moved), w.P, R._ptr(model["scaling"]),
                                              R._ptr(w.log.counter.radius3d_min), R._ptr(w.log.counter.radius3d_max),
                                              R._stream_ptr(torch.device(DEV))))
    want = [model[k] for k in w.bufs] + [e1[k] for k in w.bufs] + [e2[k] for k in w.bufs] + [torch.tensor(5.0, device=DEV)]
    assert 0 < int(moved.sum()) < w.P
    clamped = (model["scaling"][moved.bool()] <= -2.9 + 1e-5).all() and (model["scaling"][moved.bool()] >= -3.2 - 1e-5).all()
    assert bool(clamped) and float(model["scaling"][~moved.bool()].max()) > -2.8           # the clamp ran, on moved rows only

    def run():
        w.one_view(0)
        assert mv.pending(w.log) == 1
        w.one_view(1)
        assert mv.pending(w.log) == 0

    def restore():
        for t, s in zip(w.tensors(), start):
            t.copy_(s)
        w.log.optimizer._lograst_steps = 4

    # ---- eager (the first run allocates the state), then again under the synchronisation check
    run()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(w.tensors(), want))
    assert w.log.lr == lr["xyz"] and w.log.optimizer.xyz_lr == lr["xyz"]
    restore()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(w.tensors(), want))
    st = mv.stats()
    assert st["counts"] == {"views": 4, "accumulated": 4, "ordinary": 0, "steps": 2} and not st["fallbacks"]
    # ---- captured
    restore()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        run()
    restore()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(w.tensors(), start))        # capturing ran nothing
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(w.tensors(), want))


def test_cpu_tensors_and_bad_sizes_raise():
    from log_amd import multi_view as mv
    gen = torch.Generator(device=DEV).manual_seed(1)
    raw, ups, index, radii, campos = _view(gen, 10, 50, 3)
    flat, acc = _targets(50, 3, 1, False, gen, sentinel=False)
    seen = torch.zeros(50, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="GPU"):
        mv.accumulate(raw, 10, 1, campos, ups, index.cpu(), radii, acc, seen)
    with pytest.raises(ValueError):
        mv.accumulate(raw, 10, 1, campos, ups, index, radii[:-1], acc, seen)
    with pytest.raises(ValueError):
        mv.accumulate(raw, 10, 1, campos, ups, index, radii, acc, seen[:-1])
    with pytest.raises(ValueError):
        mv.accumulate(raw, 10, 1, campos, ups, index, radii, {"xyz": acc["xyz"][:-1]}, seen)
    assert int(seen.sum()) == 0 and float(flat.flat.abs().sum()) == 0.0
