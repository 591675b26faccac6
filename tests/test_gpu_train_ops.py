"""N4 on the GPU: lograst_id_histogram / lograst_counter_update / lograst_sparse_adam through the drop-ins
(log_amd/counter.py, log_amd/sparse_optimizer.py) against results of the reference's own Counter / SparseOptimizer /
torch.unique (tests/golden/*.npz) and against the oracle (same fp32 op sequence: compared bit for bit)."""
import os

import numpy as np
import pytest
import torch

import train_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_id_histogram_matches_reference_lists():
    from log_amd import counter
    g = U.load("counter_a.npz")
    for v in range(int(g["n_views"])):
        ids, counts = counter.unique_ids(torch.from_numpy(g[f"v{v}_pid_map"]).to(DEV), int(g[f"v{v}_radii"].shape[0]))
        assert ids.dtype == torch.int32 and counts.dtype == torch.int64
        np.testing.assert_array_equal(ids.cpu().numpy(), g[f"v{v}_point_id"])
        np.testing.assert_array_equal(counts.cpu().numpy(), g[f"v{v}_point_count"])


@pytest.mark.parametrize("n,shape", [(1000000, (1080, 1920)), (5, (7, 13)), (70000, (100, 100))])
def test_id_histogram_matches_torch_unique(n, shape):
    from log_amd import counter
    gen = torch.Generator(device=DEV).manual_seed(n)
    # runs of equal ids along rows (what a splat produces), -1 holes, ids spread over [0, n)
    base = torch.randint(0, n, (shape[0], (shape[1] + 4) // 5), generator=gen, device=DEV, dtype=torch.int32)
    pid = base.repeat_interleave(5, dim=1)[:, :shape[1]].contiguous()
    pid[torch.rand(shape, generator=gen, device=DEV) < 0.2] = -1
    ids, counts = counter.unique_ids(pid, n)
    want_ids, want_counts = torch.unique(pid, sorted=True, return_counts=True)
    if want_ids[0] == -1:
        want_ids, want_counts = want_ids[1:], want_counts[1:]
    assert torch.equal(ids, want_ids) and torch.equal(counts, want_counts)
    # nothing hit at all
    ids, counts = counter.unique_ids(torch.full(shape, -1, dtype=torch.int32, device=DEV), n)
    assert ids.numel() == 0 and counts.numel() == 0


def test_counter_matches_reference_counter_and_oracle(oracle_mod):
    from log_amd import counter
    g = U.load("counter_a.npz")
    P = int(g["P"])
    c = U.fresh_counter(P, DEV)
    out = U.counter_output(g, DEV)
    counter.update_by_output(c, out, fix_parent=True)
    U.check_counter(c, g)                                            # the reference's own class, run on CPU
    state = {k: np.zeros(P, dt) for k, dt in oracle_mod.COUNTER_FIELDS}
    for v in range(int(g["n_views"])):
        flag = oracle_mod.counter_update(state, g[f"v{v}_visible_index"], g[f"v{v}_grad"], g[f"v{v}_radii"],
                                         g[f"v{v}_point_weight"], g[f"v{v}_point_id"], g[f"v{v}_point_count"])
        np.testing.assert_array_equal(out["visibility_flag"][v]["flag_vis"].cpu().numpy(), flag)
        np.testing.assert_array_equal(out["visibility_flag"][v]["index_vis"].cpu().numpy(), np.nonzero(flag)[0])
    for k, _ in oracle_mod.COUNTER_FIELDS:
        np.testing.assert_array_equal(getattr(c, k).cpu().numpy(), state[k], err_msg=k)     # bit for bit


def test_counter_on_rasterizer_outputs():
    """End to end on the device: render a view with the drop-in rasterizer, histogram its id map, update a counter;
    check the invariants LoG's densification relies on."""
    import math
    from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
    from log_amd import counter, scenes
    N, W, H = 20000, 320, 240
    sc = scenes.random_scene(N, seed=4, opacity=None, smax=0.03)
    cam = scenes.orbit_cameras(1, W=W, H=H, focal=300.0)[0]
    t = lambda a: torch.tensor(a, device=DEV)
    rs = GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(cam["FoVx"] * 0.5), tanfovy=math.tan(cam["FoVy"] * 0.5),
        bg=torch.ones(3, device=DEV), scale_modifier=1.0, viewmatrix=t(cam["world_view_transform"]),
        projmatrix=t(cam["full_proj_transform"]), sh_degree=0, campos=t(cam["camera_center"]), prefiltered=False,
        debug=False)
    means2D = torch.zeros(N, 3, device=DEV, requires_grad=True)
    xyz = t(sc["xyz"]).requires_grad_(True)
    image, radii, pid, pwp, pw = GaussianRasterizer(raster_settings=rs)(
        means3D=xyz, means2D=means2D, shs=None, colors_precomp=t(sc["colors"]), opacities=t(sc["opacity"]),
        scales=t(sc["scaling"]), rotations=t(sc["rotation"]), cov3D_precomp=None)
    image.sum().backward()
    ids, counts = counter.unique_ids(pid, N)
    wi, wc = torch.unique(pid, sorted=True, return_counts=True)
    assert torch.equal(ids, wi[1:] if wi[0] == -1 else wi) and torch.equal(counts, wc[1:] if wi[0] == -1 else wc)
    P = 3 * N
    c = U.fresh_counter(P, DEV)
    vis_index = torch.randperm(P, device=DEV)[:N]
    out = {"render": [image], "visibility_flag": [{"index": vis_index}],
           "viewspace_points": [means2D], "radii": [radii], "point_weight": [pw], "point_id": [ids],
           "point_count": [counts]}
    counter.update_by_output(c, out)
    assert int(c.area_sum.sum()) == int((pid >= 0).sum())
    assert int(c.visible_count.sum()) == int((radii > 0).sum()) == int(c.create_steps.sum())
    assert torch.equal(c.weights_max[vis_index], torch.where(radii > 0, pw, torch.zeros_like(pw)))
    assert torch.equal(c.radii_max[vis_index].int(), radii.clamp(min=0))
    gn = torch.norm(means2D.grad[:, :2], dim=-1)
    want = torch.zeros(P, device=DEV)
    want[vis_index[ids.long()]] = gn[ids.long()] * counts
    torch.testing.assert_close(c.grad_sum, want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", ["adam_a.npz", "adam_ams.npz"])
def test_sparse_adam_matches_reference_optimizer_and_oracle(name, oracle_mod):
    from log_amd import sparse_optimizer, rasterizer as R
    import oracle_backend
    from oracle_backend import OracleBackend
    g = U.load(name)
    model, opt = U.run_adam(g, DEV, sparse_optimizer.step)
    U.check_adam(model, opt, g)                                      # the reference's own class, run on CPU
    old = oracle_backend.install(OracleBackend())
    try:
        m_o, o_o = U.run_adam(g, "cpu", sparse_optimizer.step)       # same host logic, oracle arithmetic
    finally:
        oracle_backend.install(None if isinstance(old, R.HipBackend) else old)
    for k in U.ADAM_KEYS:
        np.testing.assert_array_equal(getattr(model, k).cpu().numpy(), getattr(m_o, k).numpy(), err_msg=k)
        np.testing.assert_array_equal(opt.exp_avg[k].cpu().numpy(), o_o.exp_avg[k].numpy(), err_msg=k)
        np.testing.assert_array_equal(opt.exp_avg_sq[k].cpu().numpy(), o_o.exp_avg_sq[k].numpy(), err_msg=k)


def test_sparse_adam_many_rows_and_untouched_rows():
    """1 M rows: rows outside index[flag_vis] keep parameters and moments bit for bit."""
    from log_amd import sparse_optimizer
    import types
    P, m = 1000000, 400000
    gen = torch.Generator(device=DEV).manual_seed(0)
    model = types.SimpleNamespace(xyz=torch.randn(P, 3, device=DEV, generator=gen),
                                  shs=torch.randn(P, 15, 3, device=DEV, generator=gen))
    before = {k: getattr(model, k).clone() for k in ("xyz", "shs")}
    zeros = lambda: {k: torch.zeros_like(getattr(model, k)) for k in ("xyz", "shs")}
    opt = types.SimpleNamespace(global_steps=torch.tensor(0., device=DEV), lr_dict={"shs": 1e-3}, exp_avg=zeros(),
                                exp_avg_sq=zeros(), use_amsgrad=False, xyz_lr=None,
                                xyz_scheduler_args=lambda step: 1e-2, scaling_scheduler_args=lambda step: 5e-3)
    index = torch.randperm(P, device=DEV, generator=gen)[:m]
    flag_vis = torch.rand(m, device=DEV, generator=gen) < 0.7
    params = {}
    for k in ("xyz", "shs"):
        p = torch.nn.Parameter(getattr(model, k)[index].clone())
        p.grad = torch.randn(p.shape, device=DEV, generator=gen)
        params[k] = p
    sparse_optimizer.step(opt, model, index, params, flag_vis)
    touched = torch.zeros(P, dtype=torch.bool, device=DEV)
    touched[index[flag_vis]] = True
    for k in ("xyz", "shs"):
        now = getattr(model, k)
        assert torch.equal(now[~touched], before[k][~touched])
        assert bool((opt.exp_avg[k][~touched] == 0).all())
        # first Adam step moves every touched element by lr * sign(g) (m / sqrt(v) = +-1 after bias correction)
        lr = 1e-2 if k == "xyz" else 1e-3
        sel = index[flag_vis]
        torch.testing.assert_close(now[sel] - before[k][sel], -lr * torch.sign(params[k].grad[flag_vis]), rtol=1e-3, atol=1e-6)
    assert float(opt.global_steps) == 1.0


def test_host_resident_adam_moments_are_moved_to_the_device():
    """LoG parks the moments on the host above 50 M points (LoG/model/splitter.py:198-204); the drop-in moves them
    next to the parameters at the first step (288 GB of HBM) instead of refusing, and the step equals the all-device one."""
    from log_amd import sparse_optimizer
    import types
    P, m = 5000, 2000
    gen = torch.Generator(device=DEV).manual_seed(3)

    def fresh(state_dev):
        g2 = torch.Generator(device=DEV).manual_seed(4)
        model = types.SimpleNamespace(xyz=torch.randn(P, 3, device=DEV, generator=g2), opacity=torch.randn(P, 1, device=DEV, generator=g2))
        z = lambda: {k: torch.zeros(getattr(model, k).shape, device=state_dev) for k in ("xyz", "opacity")}
        opt = types.SimpleNamespace(global_steps=torch.tensor(0., device=DEV), lr_dict={"opacity": 0.05}, exp_avg=z(),
                                    exp_avg_sq=z(), use_amsgrad=False, xyz_lr=None,
                                    xyz_scheduler_args=lambda step: 1e-3, scaling_scheduler_args=lambda step: 5e-3)
        return model, opt

    index = torch.randperm(P, device=DEV, generator=gen)[:m]
    flag_vis = torch.rand(m, device=DEV, generator=gen) < 0.7
    grads = {"xyz": torch.randn(m, 3, device=DEV, generator=gen), "opacity": torch.randn(m, 1, device=DEV, generator=gen)}
    results = []
    for state_dev in ("cpu", DEV):
        model, opt = fresh(state_dev)
        for _ in range(2):
            params = {}
            for k in ("xyz", "opacity"):
                p = torch.nn.Parameter(getattr(model, k)[index].clone())
                p.grad = grads[k].clone()
                params[k] = p
            sparse_optimizer.step(opt, model, index, params, flag_vis)
        assert all(t.device.type == "cuda" for d in (opt.exp_avg, opt.exp_avg_sq) for t in d.values())
        results.append((model, opt))
    (m0, o0), (m1, o1) = results
    for k in ("xyz", "opacity"):
        assert torch.equal(getattr(m0, k), getattr(m1, k)) and torch.equal(o0.exp_avg[k], o1.exp_avg[k])


def test_owner_computes_step_on_device_matches_reference_golden():
    """log_amd.dist.OwnerAdam at world = 1 through the HIP Adam kernel: the golden produced by the reference's own
    SparseOptimizer (tests/golden/make_golden_owner.py)."""
    from log_amd.dist import FlatParams, GradientBucket, OwnerAdam
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "owner_adam.npz"))
    names = ("means3D", "scales", "rotations", "opacities", "colors", "shs")
    P = int(g["P"])
    params = FlatParams({n: torch.from_numpy(g["init_" + n].copy()).to(DEV) for n in names}, DEV, 1)
    bucket = GradientBucket(P, DEV, 1, sh_coeffs=15)
    opt = OwnerAdam(params, 0)
    for it in range(int(g["n_steps"])):
        bucket.zero()
        for n in names:
            bucket.views[n].copy_(torch.from_numpy(g[f"s{it}_grad_{n}"]).to(DEV).reshape(bucket.views[n].shape))
        bucket.mark_seen(torch.from_numpy(g[f"s{it}_seen"]).to(DEV).to(torch.int32) * 3)
        lr = {"means3D": float(g[f"s{it}_lr_means3D"]), "scales": float(g[f"s{it}_lr_scales"]), "rotations": 0.001,
              "opacities": 0.05, "colors": 0.0025, "shs": 0.000125}
        moved = opt.step(bucket, params, lr)
        assert int(moved) == int(g[f"s{it}_seen"].sum())
    for n in names:
        np.testing.assert_allclose(params.views[n].cpu().numpy().reshape(g["final_" + n].shape), g["final_" + n], rtol=2e-6, atol=1e-9)
        np.testing.assert_allclose(opt.exp_avg[n].cpu().numpy()[:P].reshape(g["final_exp_avg_" + n].shape),
                                   g["final_exp_avg_" + n], rtol=2e-6, atol=1e-12)


# (degree, K) a degree-3 model trains through before the active degree reaches the stored one, and gathered / parameter
# row counts on the edges of the kernels' 64-row waves and 256-row workgroups
_FUSED_SCHEDULE = [(0, 15), (1, 15), (2, 15)]
_FUSED_SIZES = [(1, 1), (65, 63), (257, 256), (321, 300)]


@pytest.mark.parametrize("degree,amsgrad,K,sizes,left_out",
                         [pytest.param(3, False, None, None, (), id="3-False"), pytest.param(1, True, None, None, (), id="1-True"),
                          pytest.param(0, False, None, None, (), id="0-False")] +
                         [pytest.param(d, d == 1, k, None, (), id="deg%d-K%d" % (d, k)) for d, k in _FUSED_SCHEDULE] +
                         [pytest.param(d, d == 2, k, sz, (), id="deg%d-K%d-%dof%d" % (d, k, sz[1], sz[0]))
                          for d, k in _FUSED_SCHEDULE + [(3, 15)] for sz in _FUSED_SIZES] +
                         # keys that are not optimised: their inputs are not loaded, their rows and moments stay
                         [pytest.param(2, True, 15, (65, 63), ("rotation", "scaling"), id="deg2-K15-63of65-no_rotation_no_scaling")])
def test_fused_step_kernel_equals_activation_backward_plus_sparse_adam(degree, amsgrad, K, sizes, left_out):
    """Round 6 (round-5 verdict, next #6): lograst_activate_backward_adam -- the activation backward applying the reference's
    sparse Adam itself, the compact raw gradients never written -- against the two kernels it replaces, on IDENTICAL inputs
    (the same gathered rows, the same dL/d(activated), the same visibility): same op sequences, so the model, both moments
    and the amsgrad maximum come out BIT FOR BIT the same.  The unfused pair is pinned to goldens produced by the reference's
    own SparseOptimizer / Activation (adam_*.npz, getall_*.npz), so the pin carries over."""
    import math
    import torch
    from log_amd import rasterizer as R
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(7 + degree)
    P, n_all, n = 50_000, 20_011, 17_003                      # model rows, gathered rows, rows that are parameters
    if sizes is not None:
        n_all, n = sizes
        P = 2 * n_all + 5
    if K is None:
        K = max((degree + 1) ** 2 - 1, 3)
    rnd = lambda *sh: torch.randn(*sh, device=dev, generator=gen)
    bufs = {"xyz": rnd(P, 3), "scaling": rnd(P, 3) * 0.3 - 3.0, "opacity": rnd(P, 1), "rotation": rnd(P, 4),
            "colors": rnd(P, 3), "shs": rnd(P, K, 3) * 0.2}
    index = torch.randperm(P, device=dev, generator=gen)[:n_all]
    campos = torch.tensor([0.3, -2.0, 1.0], device=dev)
    raw, act = R._backend.gather_activate(index, bufs, degree, campos if degree > 0 else None)
    ups = {"xyz": rnd(n_all, 3), "scaling": rnd(n_all, 3), "opacity": rnd(n_all, 1), "rotation": rnd(n_all, 4),
           "colors": rnd(n_all, 3)}
    radii = (torch.rand(n_all, device=dev, generator=gen) < 0.6).to(torch.int32) * 7
    if sizes is not None:
        radii[0] = 7                                          # a handful of rows: at least one of them is visible
    keys = [k for k in bufs if (k != "shs" or degree > 0) and k not in left_out]
    lr = {"xyz": 1.6e-4, "scaling": 5e-3, "opacity": 0.05, "rotation": 1e-3, "colors": 2.5e-3, "shs": 1.25e-4}
    m1_0 = {k: rnd(*v.shape) * 1e-3 for k, v in bufs.items()}
    m2_0 = {k: (rnd(*v.shape) * 1e-3) ** 2 for k, v in bufs.items()}
    mx_0 = {k: (rnd(*v.shape) * 1e-3) ** 2 for k, v in bufs.items()}
    results = []
    for fused in (False, True):
        model = {k: v.clone() for k, v in bufs.items()}
        m1, m2 = {k: v.clone() for k, v in m1_0.items()}, {k: v.clone() for k, v in m2_0.items()}
        mx = {k: v.clone() for k, v in mx_0.items()} if amsgrad else None
        steps = 5
        bc1, bc2 = 1 - 0.9 ** steps, 1 - 0.999 ** steps
        if fused:
            entries = {k: (model[k], m1[k], m2[k], mx[k] if amsgrad else None, lr[k] / bc1) for k in keys}
            R._backend.activate_backward_adam(raw, n, degree, campos if degree > 0 else None, ups["xyz"], ups["scaling"],
                                              ups["opacity"], ups["rotation"], ups["colors"], index[:n], radii, entries,
                                              0.9, 0.999, math.sqrt(bc2), 1e-15)
        else:
            g = R._backend.activate_backward(raw, n, degree, campos if degree > 0 else None, ups["scaling"], ups["opacity"],
                                             ups["rotation"], ups["colors"])
            g["xyz"] = ups["xyz"][:n]
            entries = [(model[k], raw[k][:n], g[k], m1[k], m2[k], mx[k] if amsgrad else None, lr[k] / bc1) for k in keys]
            R._backend.sparse_adam(index[:n], radii[:n] > 0, entries, 0.9, 0.999, math.sqrt(bc2), 1e-15)
        torch.cuda.synchronize()
        results.append((model, m1, m2, mx))
    (ma, a1, a2, ax), (mb, b1, b2, bx) = results
    touched = 0
    for k in bufs:
        assert torch.equal(ma[k], mb[k]) and torch.equal(a1[k], b1[k]) and torch.equal(a2[k], b2[k]), k
        if amsgrad:
            assert torch.equal(ax[k], bx[k]), k
        touched += int((mb[k] != bufs[k]).sum())
    for k in left_out:                                        # the fused kernel left the key's model rows and moments alone
        assert torch.equal(mb[k], bufs[k]) and torch.equal(b1[k], m1_0[k]) and torch.equal(b2[k], m2_0[k]), k
        assert not amsgrad or torch.equal(bx[k], mx_0[k]), k
    # a visible row moves in all of its 14 + 3 K values and both moments move with it; counted on the model alone, and with
    # the 100 000 of the full size (17 003 rows, about 10 200 visible: 9.8 per visible row) scaled to the rows of this case
    n_vis = int((radii[:n] > 0).sum())
    assert n_vis > 0 and touched > 9.8 * n_vis
    if sizes is None:
        assert touched > 100_000
    if degree == 0:
        assert torch.equal(mb["shs"], bufs["shs"])            # unused coefficients: no gradient, no update
    vis_rows = index[:n][radii[:n] > 0]
    hidden = torch.ones(P, dtype=torch.bool, device=dev)
    hidden[vis_rows] = False
    assert torch.equal(mb["xyz"][hidden], bufs["xyz"][hidden])  # rows that are not visible parameters never move


def test_fused_step_through_the_drop_ins():
    """``log_amd.get_all.set_fused_step(True)`` in the flow of a LoG training view (select -> gather / activate -> rasterize
    fwd + bwd -> counter -> step): the update is applied by the backward, nothing is left on ``params[key].grad``, ``step``
    is reduced to its bookkeeping (step counter, the learning rate the trainer reads back), and the model agrees with the
    unfused drop-ins' to the run-to-run noise of the rasterizer's own gradients (its reverse walk sums with atomics)."""
    import os
    import sys
    import torch
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_log_step as B
    from log_amd import get_all
    wl = B.Workload(roots=3000, levels=4, sh_degree=3, views=3, root_scale=0.05)
    packs = [wl.rasterizer_for(c) for c in wl.cams]
    states = []
    for fused in (False, True):
        st = B.State(wl)
        prev = get_all.set_fused_step(fused)
        try:
            for p in packs + packs[:1]:
                B.view(wl, st, p, True, lambda name: None)
                params = st.gaussian.visibility_flag["params"]
                if fused:
                    assert all(p_.grad is None for p_ in params.values())          # nothing was written for the optimizer to read
                else:
                    assert params["xyz"].grad is not None
                assert not getattr(st.opt, "_lograst_fused_pending", False)        # step() consumed it
            if fused:
                # two training get_all's before ONE step (a batch of several views): neither backward may apply an update
                # of its own -- both go the ordinary way and leave their gradients on the parameters
                from log_amd import lod
                rast, camera = packs[1]
                index, index_node = B.split_leaf_node(wl, lod.traverse(wl.tree, st.gaussian, wl.roots, rast))
                before = {k: st.bufs[k].clone() for k in wl.keys}
                images, packs_params = [], []
                for _ in range(2):                                                 # renderer.py: every view's forward ...
                    st.gaussian.visibility_flag = {"index": index, "index_node": index_node}
                    act = get_all.get_all(st.model, camera, rast)
                    packs_params.append(st.gaussian.visibility_flag["params"])
                    means2D = torch.zeros_like(act["xyz"], requires_grad=True)
                    images.append(rast(means3D=act["xyz"], means2D=means2D, shs=None, colors_precomp=act["colors"],
                                       opacities=act["opacity"], scales=act["scaling"], rotations=act["rotation"],
                                       cov3D_precomp=None)[0])
                (images[0] + images[1]).backward(gradient=wl.wloss)                # ... then ONE backward over the batch
                for params in packs_params:
                    assert params["xyz"].grad is not None
                assert not getattr(st.opt, "_lograst_fused_pending", False)
                assert all(torch.equal(before[k], st.bufs[k]) for k in wl.keys)    # nothing applied at backward time
                st.opt._lograst_open_packs = 0                                     # (what step() does)
        finally:
            get_all.set_fused_step(prev)
        states.append(st)
    a, b = states
    assert float(a.opt.global_steps) == float(b.opt.global_steps) == 4.0 and a.opt.xyz_lr == b.opt.xyz_lr
    for k in wl.keys:
        da = (a.bufs[k] - wl.bufs[k]).double()
        assert float((b.bufs[k] - a.bufs[k]).double().norm()) <= 1e-4 * float(da.norm()), k
        assert float(da.norm()) > 0


def test_fused_step_takes_its_row_mask_from_its_own_render_only():
    """The fused step next to flows it must not fuse (tests/fused_step_util.py; 3000 Gaussians, two 160 x 96 views that see
    different rows; the ordinary step, case (a), is the test above): (b) a step whose loss touches the get_all outputs only,
    (c) a render whose image receives no gradient -- each must leave ordinary gradients and, after step() with the caller's
    flag_vis, equal the unfused drop-ins on a copy of the model in parameters and both moments (rtol 2e-6: the two start
    from identical state and no rasterizer gradient enters the second step, so nothing but rounding may differ) --, and
    (d) a second backward through one pack before step(): refused with an error that names the cause, the applied update
    left exactly as it was."""
    import fused_step_util as F
    F.run_cases("cuda:0", P=3000, W=160, H=96, focal=300.0)


@pytest.mark.parametrize("seed", range(6))
def test_random_views_and_steps_against_reference_classes_on_device(seed):
    """The reference's recorded random cases (radii beyond int16, keys without gradient, amsgrad, K from 1 to 15) through the
    HIP counter and sparse Adam: the body, assertions and tolerances of the CPU test of the same name."""
    U.check_random_case(seed, DEV)
