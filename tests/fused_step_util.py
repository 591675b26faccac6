"""The fused step's row mask (log_amd.get_all.set_fused_step) in flows other than render -> loss -> backward -> step, shared
by the CPU test (tests/test_getall_cpu.py: the oracle backend, the fused kernel stood in for by the pair it replaces) and the
GPU test (tests/test_gpu_train_ops.py: the kernels).  Every case starts from a model that has taken one ordinary fused step
on view A, and compares a second step through the fused path with the same step through the unfused drop-ins on a COPY of
that model -- so the two start bit-identical and differ only by what the second step does."""
import math
import types

import numpy as np
import torch

LR = {"colors": 0.0025, "shs": 0.000125, "opacity": 0.05, "rotation": 0.001}
DEGREE, K = 1, 3


class State:
    """Model buffers + optimizer in the shape the drop-ins read (LoG.gaussian / SparseOptimizer attributes)."""

    def __init__(self, bufs, steps=0.0, moments=None):
        dev = bufs["xyz"].device
        self.bufs = {k: v.clone() for k, v in bufs.items()}
        keys = list(self.bufs)
        self.gaussian = types.SimpleNamespace(keys=keys, active_sh_degree=DEGREE, visibility_flag=None,
                                              items=lambda: ((k, self.bufs[k]) for k in keys), **self.bufs)
        z = lambda i: {k: (torch.zeros_like(v) if moments is None else moments[i][k].clone()) for k, v in self.bufs.items()}
        self.opt = types.SimpleNamespace(global_steps=torch.tensor(float(steps), device=dev), lr_dict=dict(LR), exp_avg=z(0),
                                         exp_avg_sq=z(1), use_amsgrad=False, xyz_lr=None,
                                         xyz_scheduler_args=lambda st: 1.6e-4, scaling_scheduler_args=lambda st: 5e-3)
        self.model = types.SimpleNamespace(gaussian=self.gaussian, fix_parent=True, training=True, optimizer=self.opt)
        self.model_ns = types.SimpleNamespace(**self.bufs)

    def copy(self):
        return State(self.bufs, float(self.opt.global_steps), (self.opt.exp_avg, self.opt.exp_avg_sq))

    def tensors(self):
        out = {"model_" + k: v for k, v in self.bufs.items()}
        out.update({"exp_avg_" + k: v for k, v in self.opt.exp_avg.items()})
        out.update({"exp_avg_sq_" + k: v for k, v in self.opt.exp_avg_sq.items()})
        return out


class Setup:
    """P Gaussians in a cube, two narrow cameras a quarter turn apart (each sees its own part of the cube), a selection of
    n_leaf parameter rows + n_node further rows (fix_parent: gathered and rendered, not optimised)."""

    def __init__(self, device, P, W, H, focal):
        from diff_gaussian_rasterization_wodilate import GaussianRasterizationSettings, GaussianRasterizer
        from log_amd import scenes
        self.dev, self.P, self.W, self.H = torch.device(device), P, W, H
        sc = scenes.random_scene(P, seed=4, opacity=None, smax=0.08, extent=2.0)
        gen = torch.Generator().manual_seed(9)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)
        self.bufs = {"scaling": t(np.log(sc["scaling"] + 0.01)), "colors": torch.randn(P, 3, generator=gen).to(self.dev),
                     "xyz": t(sc["xyz"]), "opacity": (torch.randn(P, 1, generator=gen) + 1.0).to(self.dev),
                     "rotation": t(sc["rotation"]), "shs": (torch.randn(P, K, 3, generator=gen) * 0.2).to(self.dev)}
        perm = torch.randperm(P, generator=gen)
        n_leaf = int(0.8 * P)
        self.index, self.index_node = perm[:n_leaf].to(self.dev), perm[n_leaf:n_leaf + P // 10].to(self.dev)
        self.n_leaf, self.n_all = n_leaf, n_leaf + P // 10
        self.views = []
        for cam in scenes.orbit_cameras(4, radius=2.5, W=W, H=H, focal=focal, end_deg=270.0)[:2]:
            rs = GaussianRasterizationSettings(
                image_height=H, image_width=W, tanfovx=math.tan(cam["FoVx"] * 0.5), tanfovy=math.tan(cam["FoVy"] * 0.5),
                bg=t([1.0, 1.0, 1.0]), scale_modifier=1.0, viewmatrix=t(cam["world_view_transform"]),
                projmatrix=t(cam["full_proj_transform"]), sh_degree=0, campos=t(cam["camera_center"]), prefiltered=False,
                debug=False)
            self.views.append((GaussianRasterizer(raster_settings=rs), {"camera_center": t(cam["camera_center"])}))
        self.wloss = torch.rand(3, H, W, generator=gen).to(self.dev)
        self.ups = {k: torch.randn(self.n_all, c, generator=gen).to(self.dev)
                    for k, c in (("xyz", 3), ("scaling", 3), ("opacity", 1), ("rotation", 4), ("colors", 3))}
        self.flag_b = (torch.rand(n_leaf, generator=gen) < 0.5).to(self.dev)          # case (b): the caller's own flag_vis

    def gather(self, st, view):
        from log_amd import get_all
        rast, camera = self.views[view]
        st.gaussian.visibility_flag = {"index": self.index, "index_node": self.index_node}
        act = get_all.get_all(st.model, camera, rast)
        return act, st.gaussian.visibility_flag["params"]

    def render(self, st, view):
        act, params = self.gather(st, view)
        rast = self.views[view][0]
        means2D = torch.zeros_like(act["xyz"], requires_grad=True)
        image, radii = rast(means3D=act["xyz"], means2D=means2D, shs=None, colors_precomp=act["colors"],
                            opacities=act["opacity"], scales=act["scaling"], rotations=act["rotation"], cov3D_precomp=None)[:2]
        return act, params, image, radii

    def regulariser(self, act):
        return sum((act[k] * self.ups[k]).sum() for k in self.ups)

    def step(self, st, params, flag_vis):
        from log_amd import sparse_optimizer
        sparse_optimizer.step(st.opt, st.model_ns, self.index, params, flag_vis)


class NoImageGradient(torch.autograd.Function):
    """value = `other`; the image is an input whose gradient is None (what a loss node may return for an input it did not
    use): the rasterizer's backward node then runs with grad_image None."""

    @staticmethod
    def forward(ctx, image, other):
        return other.clone()

    @staticmethod
    def backward(ctx, g):
        return None, g


def same(a, b, rtol=2e-6):
    """Parameters and both moments, as train_util.check_adam compares them (rtol 0: bit for bit)."""
    ta, tb = a.tensors(), b.tensors()
    for name in ta:
        if rtol == 0:
            assert torch.equal(ta[name], tb[name]), name
            continue
        atol = 1e-9 if name.startswith("model_") else (1e-20 if name.startswith("exp_avg_sq_") else 1e-12)
        np.testing.assert_allclose(ta[name].cpu().numpy(), tb[name].cpu().numpy(), rtol=rtol, atol=atol, err_msg=name)


def run_cases(device, P, W, H, focal):
    """-> dict of what each case observed; asserts the comparisons themselves (same code for both backends)."""
    from log_amd import get_all
    su = Setup(device, P, W, H, focal)
    prev = get_all.set_fused_step(True)
    try:
        # ---- step 1, view A, the ordinary fused step (case (a) is tests/test_gpu_train_ops.py's existing test)
        base = State(su.bufs)
        act, params, image, radii_a = su.render(base, 0)
        (image * su.wloss).sum().backward()
        assert all(p.grad is None for p in params.values()) and base.opt._lograst_fused_pending
        vis_a = (radii_a > 0)[:su.n_leaf]
        su.step(base, params, vis_a)
        assert not base.opt._lograst_fused_pending and float(base.opt.global_steps) == 1.0
        moved = (base.bufs["xyz"][su.index] != su.bufs["xyz"][su.index]).any(1)
        # only rows view A saw moved (a seen row whose gradient is exactly zero stays), and it saw a part of them
        assert not bool((moved & ~vis_a).any()) and int(moved.sum()) > 0.5 * int(vis_a.sum())
        assert 0.2 * su.n_leaf < int(vis_a.sum()) < 0.8 * su.n_leaf
        seen = {}

        def second_step(case, fused):
            st = base.copy()
            get_all.set_fused_step(fused)
            if case == "b":       # a regulariser on the activated rows alone: no rasterizer in the graph
                act, params = su.gather(st, 1)
                su.regulariser(act).backward()
                flag = su.flag_b
            else:                 # view B rendered, but the image's gradient is None: only the regulariser's flows
                act, params, image, radii = su.render(st, 1)
                NoImageGradient.apply(image, su.regulariser(act)).backward()
                flag = (radii > 0)[:su.n_leaf]
                seen["vis_b"] = flag
            # the fused path found no render of its own: ordinary gradients, nothing applied at backward time
            assert all(params[k].grad is not None for k in params), case
            assert not getattr(st.opt, "_lograst_fused_pending", False), case
            same(st, base, rtol=0)
            su.step(st, params, flag)
            assert float(st.opt.global_steps) == 2.0
            return st

        for case in ("b", "c"):
            ref = second_step(case, False)
            got = second_step(case, True)
            same(got, ref)
            assert float((ref.bufs["xyz"] - base.bufs["xyz"]).abs().sum()) > 0, case
        # the two views and the caller's flag really select different rows (else a stale mask could not show)
        for other in (seen["vis_b"], su.flag_b):
            assert int((other != vis_a).sum()) > 0.1 * su.n_leaf
        # ---- (d) two backwards through one pack before one step(): the first applies the update, the second is refused
        get_all.set_fused_step(True)
        st = base.copy()
        act, params, image, radii = su.render(st, 1)
        loss = (image * su.wloss).sum()
        loss.backward(retain_graph=True)
        assert st.opt._lograst_fused_pending and all(p.grad is None for p in params.values())
        after_first = st.copy()
        assert float((after_first.bufs["xyz"] - base.bufs["xyz"]).abs().sum()) > 0
        try:
            loss.backward()
        except RuntimeError as e:
            seen["error_d"] = str(e)
        else:
            raise AssertionError("a second backward before step() went through silently")
        assert "second backward" in seen["error_d"] and "step()" in seen["error_d"], seen["error_d"]
        same(st, after_first, rtol=0)                                       # no second update, no half of one
        assert all(p.grad is None for p in params.values())
        su.step(st, params, (radii > 0)[:su.n_leaf])                        # the bookkeeping of the ONE update
        same(st, after_first, rtol=0)
        assert float(st.opt.global_steps) == 2.0 and not st.opt._lograst_fused_pending
        # gradients that reach the parameters some other way while the update is applied: step() refuses them too
        st = base.copy()
        act, params, image, radii = su.render(st, 1)
        (image * su.wloss).sum().backward()
        params["xyz"].grad = torch.ones_like(params["xyz"])
        after_first = st.copy()
        try:
            su.step(st, params, (radii > 0)[:su.n_leaf])
        except RuntimeError as e:
            assert "gradients were left" in str(e), str(e)
        else:
            raise AssertionError("step() applied a second update of the same step")
        same(st, after_first, rtol=0)
        assert float(st.opt.global_steps) == 1.0
        return seen
    finally:
        get_all.set_fused_step(prev)
