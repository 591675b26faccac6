"""Helpers shared by the CPU and GPU tests of the N4 drop-ins (counter / id histogram / sparse Adam): rebuild the
objects the drop-in methods expect (the attributes they read from LoG's Counter / SparseOptimizer) from the golden
files written by tests/golden/make_golden_train.py."""
import os
import types

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
COUNTER_DTYPES = {"weights_max": torch.float32, "weights_sum": torch.float32, "grad_sum": torch.float32,
                  "radii_max": torch.int16, "visible_count": torch.int16, "radii_max_max": torch.int32,
                  "area_sum": torch.int32, "create_steps": torch.int32}
ADAM_KEYS = ["xyz", "colors", "scaling", "opacity", "rotation", "shs"]
LR = {"colors": 0.0025, "shs": 0.000125, "opacity": 0.05, "rotation": 0.001}


def load(name):
    return np.load(os.path.join(GOLDEN_DIR, name))


def fresh_counter(P, device):
    """Counter.__init__ (LoG/model/counter.py:5-19): zeros of the registered dtypes."""
    return types.SimpleNamespace(**{k: torch.zeros(P, dtype=dt, device=device) for k, dt in COUNTER_DTYPES.items()})


def counter_output(g, device, with_lists=True):
    """The `output` dict Counter.update_by_output receives (LoG/render/renderer.py:168-184, lists over views)."""
    nv = int(g["n_views"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    out = {k: [] for k in ("render", "visibility_flag", "viewspace_points", "radii", "point_weight", "point_id",
                           "point_count")}
    for v in range(nv):
        vis = g[f"v{v}_visible_index"]
        n_leaf = int(0.5 * int(g["P"]))
        out["render"].append(None)
        out["visibility_flag"].append({"index": t(vis[:n_leaf]), "index_node": t(vis[n_leaf:])})
        out["viewspace_points"].append(types.SimpleNamespace(grad=t(g[f"v{v}_grad"])))
        out["radii"].append(t(g[f"v{v}_radii"]))
        out["point_weight"].append(t(g[f"v{v}_point_weight"]))
        if with_lists:
            out["point_id"].append(t(g[f"v{v}_point_id"]))
            out["point_count"].append(t(g[f"v{v}_point_count"]))
    return out


def check_counter(counter, g, rtol=2e-6):
    for k, dt in COUNTER_DTYPES.items():
        got, want = getattr(counter, k).cpu().numpy(), g["final_" + k]
        if dt.is_floating_point:
            np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-12, err_msg=k)
        else:
            np.testing.assert_array_equal(got, want, err_msg=k)


def fresh_optimizer(g, device):
    """What SparseOptimizer.__init__ sets up (sparse_optimizer.py:118-160) that step() reads."""
    amsgrad = bool(int(g["amsgrad"]))
    model = types.SimpleNamespace(**{k: torch.from_numpy(g["init_" + k].copy()).to(device) for k in ADAM_KEYS})
    zeros = lambda: {k: torch.zeros_like(getattr(model, k)) for k in ADAM_KEYS}
    opt = types.SimpleNamespace(
        global_steps=torch.tensor(float(g["start_global_steps"]), dtype=torch.float32, device=device),
        lr_dict=dict(LR), exp_avg=zeros(), exp_avg_sq=zeros(), use_amsgrad=amsgrad, xyz_lr=None,
        scaling_scheduler_args=lambda step: 0.005)
    if amsgrad:
        opt.max_exp_avg_sq = zeros()
    return model, opt


def adam_step_inputs(g, it, device):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    params = {}
    for k in ADAM_KEYS:
        p = torch.nn.Parameter(t(g[f"s{it}_param_{k}"]))
        if f"s{it}_grad_{k}" in g:
            p.grad = t(g[f"s{it}_grad_{k}"])
        params[k] = p
    return t(g[f"s{it}_index"]), params, t(g[f"s{it}_flag_vis"])


def run_adam(g, device, step_fn):
    model, opt = fresh_optimizer(g, device)
    for it in range(int(g["n_steps"])):
        index, params, flag_vis = adam_step_inputs(g, it, device)
        lr_xyz = float(g[f"s{it}_lr_xyz"])
        opt.xyz_scheduler_args = lambda step, lr=lr_xyz: lr       # the schedule itself is host code of the reference
        step_fn(opt, model, index, params, flag_vis)
        assert opt.xyz_lr == lr_xyz
    return model, opt


def check_adam(model, opt, g, rtol=2e-6):
    for k in ADAM_KEYS:
        np.testing.assert_allclose(getattr(model, k).cpu().numpy(), g["final_" + k], rtol=rtol, atol=1e-9, err_msg=k)
        np.testing.assert_allclose(opt.exp_avg[k].cpu().numpy(), g["final_exp_avg_" + k], rtol=rtol, atol=1e-12, err_msg=k)
        np.testing.assert_allclose(opt.exp_avg_sq[k].cpu().numpy(), g["final_exp_avg_sq_" + k], rtol=rtol, atol=1e-20, err_msg=k)
        if opt.use_amsgrad:
            np.testing.assert_allclose(opt.max_exp_avg_sq[k].cpu().numpy(), g["final_max_exp_avg_sq_" + k], rtol=rtol,
                                       atol=1e-20, err_msg=k)
    assert float(opt.global_steps) == float(g["final_global_steps"])


# ---- random cases: tests/test_train_ops_cpu.py::test_random_views_and_steps_against_reference_classes ----------------
# The reference's Counter / SparseOptimizer ran on exactly these inputs in tests/golden/make_golden_train_random.py; what
# they computed is stored in tests/golden/train_random_<seed>.npz.
RANDOM_LR = {"xyz": 0.00016, "xyz_final": 0.0000016, "colors": 0.0025, "shs": 0.000125, "scaling": 0.005, "opacity": 0.05,
             "rotation": 0.001, "max_steps": 30000}


def random_case(seed):
    """Random sizes, views with random visible sets / radii / id lists, random subsets of keys without gradient, amsgrad
    on odd seeds, one to three Adam steps.  -> dict(P, views, shapes, amsgrad, start_steps, steps, init_model)."""
    rng = np.random.default_rng(100 + seed)
    g = torch.Generator().manual_seed(seed)
    P = int(rng.integers(50, 3000))
    views = []
    for _ in range(int(rng.integers(1, 4))):
        nv = int(rng.integers(1, P + 1))
        vis = rng.permutation(P)[:nv]
        n_leaf = int(rng.integers(0, nv + 1))
        radii = rng.integers(0, 40000, nv).astype(np.int32) * (rng.random(nv) < 0.8)       # > int16 range too (.short() wraps)
        k = int(rng.integers(0, nv + 1))
        pid = np.sort(rng.permutation(nv)[:k]).astype(np.int32)
        views.append(dict(index=vis[:n_leaf], index_node=vis[n_leaf:], grad=rng.standard_normal((nv, 3)).astype(np.float32),
                          radii=radii.astype(np.int32), pw=rng.random(nv).astype(np.float32), pid=pid,
                          pc=rng.integers(1, 5000, k).astype(np.int64)))
    amsgrad = bool(seed % 2)
    shapes = {"xyz": (3,), "colors": (3,), "scaling": (3,), "opacity": (1,), "rotation": (4,), "shs": (int(rng.integers(1, 16)), 3)}

    def init_model():
        gg = torch.Generator().manual_seed(seed)
        return types.SimpleNamespace(**{k: torch.randn(P, *s, generator=gg) for k, s in shapes.items()})

    steps = []
    for _ in range(int(rng.integers(1, 4))):
        m = int(rng.integers(1, P + 1))
        index = torch.randperm(P, generator=g)[:m]
        flag_vis = torch.rand(m, generator=g) < 0.7
        no_grad = {k for k in shapes if rng.random() < 0.25}
        grads = {k: torch.randn(m, *s, generator=g) * 10.0 ** float(rng.integers(-6, 1)) for k, s in shapes.items()}
        steps.append(dict(index=index, flag_vis=flag_vis, no_grad=no_grad, grads=grads))
    return dict(P=P, views=views, shapes=shapes, amsgrad=amsgrad, start_steps=int(seed * 7), steps=steps,
                init_model=init_model)


def random_counter_output(views, device="cpu"):
    """The `output` dict Counter.update_by_output receives, for random_case()'s views."""
    t = lambda a: torch.from_numpy(a).to(device)
    return {"render": [None] * len(views),
            "visibility_flag": [{"index": t(v["index"]), "index_node": t(v["index_node"])} for v in views],
            "viewspace_points": [types.SimpleNamespace(grad=t(v["grad"])) for v in views],
            "radii": [t(v["radii"]) for v in views], "point_weight": [t(v["pw"]) for v in views],
            "point_id": [t(v["pid"]) for v in views], "point_count": [t(v["pc"]) for v in views]}


def random_step_params(model, step, shapes):
    """The `params` of one SparseOptimizer.step call: the selected rows as fresh leaves, gradients on all but `no_grad`."""
    out = {}
    for k in shapes:
        p = torch.nn.Parameter(getattr(model, k)[step["index"]].clone())
        if k not in step["no_grad"]:
            p.grad = step["grads"][k].clone()
        out[k] = p
    return out


def check_random_case(seed, device):
    """random_case(seed) through the drop-ins on `device` (the backend installed there does the arithmetic) against what
    the reference's unpatched Counter / SparseOptimizer computed on the same inputs (train_random_<seed>.npz).  One body
    for the CPU test (oracle backend) and the GPU test (HIP kernels): same assertions, same tolerances."""
    from log_amd import counter, sparse_optimizer
    c = random_case(seed)
    ref = load("train_random_%d.npz" % seed)
    P = c["P"]
    assert int(ref["P"]) == P and int(ref["n_views"]) == len(c["views"]) and int(ref["n_steps"]) == len(c["steps"])
    # ---- counter
    c_new = fresh_counter(P, device)
    o_new = random_counter_output(c["views"], device)
    counter.update_by_output(c_new, o_new, fix_parent=True)
    for k in COUNTER_DTYPES:
        a, b = getattr(c_new, k).cpu().numpy(), ref["counter_" + k]
        assert a.dtype == b.dtype, k
        if a.dtype.kind == "f":
            np.testing.assert_allclose(a, b, rtol=3e-6, atol=1e-12, err_msg=k)
        else:
            np.testing.assert_array_equal(a, b, err_msg=k)
    for v in range(len(c["views"])):
        assert torch.equal(o_new["visibility_flag"][v]["flag_vis"].cpu(), torch.from_numpy(ref[f"v{v}_flag_vis"]))
        assert torch.equal(o_new["visibility_flag"][v]["index_vis"].cpu(), torch.from_numpy(ref[f"v{v}_index_vis"]))
    # ---- sparse Adam: what SparseOptimizer.__init__ sets up that step() reads, with the reference's learning rates
    amsgrad, shapes = c["amsgrad"], c["shapes"]
    m_new = c["init_model"]()
    for k in shapes:
        setattr(m_new, k, getattr(m_new, k).to(device))
    zeros = lambda: {k: torch.zeros_like(getattr(m_new, k)) for k in shapes}
    lrs = {int(ref[f"s{i}_step"]): (float(ref[f"s{i}_lr_xyz"]), float(ref[f"s{i}_lr_scaling"])) for i in range(len(c["steps"]))}
    op_new = types.SimpleNamespace(
        global_steps=torch.tensor(float(ref["start_global_steps"]), dtype=torch.float32, device=device),
        lr_dict={k: float(ref["lr_" + k]) for k in ("colors", "shs", "opacity", "rotation")}, exp_avg=zeros(),
        exp_avg_sq=zeros(), use_amsgrad=amsgrad, xyz_lr=None, xyz_scheduler_args=lambda step: lrs[step][0],
        scaling_scheduler_args=lambda step: lrs[step][1])
    if amsgrad:
        op_new.max_exp_avg_sq = zeros()
    for st in c["steps"]:
        st = dict(st, index=st["index"].to(device), flag_vis=st["flag_vis"].to(device),
                  grads={k: v.to(device) for k, v in st["grads"].items()})
        sparse_optimizer.step(op_new, m_new, st["index"], random_step_params(m_new, st, shapes), st["flag_vis"])
    assert float(op_new.global_steps) == float(ref["final_global_steps"])
    if not np.isnan(float(ref["final_xyz_lr"])):
        assert op_new.xyz_lr == float(ref["final_xyz_lr"])
    for k in shapes:
        np.testing.assert_allclose(getattr(m_new, k).cpu().numpy(), ref["final_" + k], rtol=3e-6, atol=2e-8, err_msg=k)
        np.testing.assert_allclose(op_new.exp_avg[k].cpu().numpy(), ref["final_exp_avg_" + k], rtol=3e-6, atol=1e-12, err_msg=k)
        np.testing.assert_allclose(op_new.exp_avg_sq[k].cpu().numpy(), ref["final_exp_avg_sq_" + k], rtol=3e-6, atol=1e-20, err_msg=k)
        if amsgrad:
            np.testing.assert_allclose(op_new.max_exp_avg_sq[k].cpu().numpy(), ref["final_max_exp_avg_sq_" + k], rtol=3e-6,
                                       atol=1e-20, err_msg=k)
