"""Shared by the CPU and GPU tests of the fused get_all drop-in: rebuild a LoG-shaped object from a golden file
(tests/golden/make_golden_getall.py) and compare the drop-in's outputs and gradients with the reference's."""
import glob
import os
import types

import numpy as np
import torch

GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "getall_*.npz")))
KEYS = ["scaling", "colors", "xyz", "opacity", "rotation", "shs"]     # GaussianPoint.keys order (level_of_gaussian.py:155-160)


def log_like(g, device, training=True, fix_parent=True):
    keys = [k for k in KEYS if "model_" + k in g]
    gaussian = types.SimpleNamespace(keys=keys, active_sh_degree=int(g["degree"]))
    for k in keys:
        setattr(gaussian, k, torch.from_numpy(g["model_" + k]).to(device))
    gaussian.items = lambda: ((k, getattr(gaussian, k)) for k in keys)
    flags = {"index": torch.from_numpy(g["index"]).to(device)}
    if g["index_node"].shape[0]:
        flags["index_node"] = torch.from_numpy(g["index_node"]).to(device)
    gaussian.visibility_flag = flags
    model = types.SimpleNamespace(gaussian=gaussian, fix_parent=fix_parent, training=training)
    camera = {"camera_center": torch.from_numpy(g["camera_center"]).to(device)}
    return model, camera


def check(g, model, camera, get_all, rtol=3e-6, grad_rtol=2e-5):
    ret = get_all(model, camera, None)
    assert list(ret) == ["xyz", "scaling", "opacity", "rotation", "colors"]
    for k in ret:
        np.testing.assert_allclose(ret[k].detach().cpu().numpy(), g["act_" + k], rtol=rtol, atol=1e-6, err_msg=k)
    params = model.gaussian.visibility_flag["params"]
    assert list(params) == model.gaussian.keys
    n_leaf = g["index"].shape[0]
    for k, p in params.items():
        assert isinstance(p, torch.nn.Parameter) and p.shape[0] == n_leaf
        np.testing.assert_array_equal(p.detach().cpu().numpy(), g["model_" + k][g["index"]])
    loss = sum((ret[k] * torch.from_numpy(g["up_" + k]).to(ret[k].device)).sum() for k in ret)
    loss.backward()
    for k, p in params.items():
        if not int(g["has_grad_" + k]):
            assert p.grad is None, k
            continue
        want = g["grad_" + k]
        got = p.grad.cpu().numpy()
        assert got.shape == want.shape, k
        err = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
        assert err < grad_rtol, (k, err)
        np.testing.assert_allclose(got, want, rtol=1e-3, atol=1e-5 * np.abs(want).max(), err_msg=k)


def stand_in(bufs, index, index_node, degree):
    """A LoG-shaped object around plain buffers: what log_amd.get_all reads of the model."""
    keys = list(bufs)
    flags = {"index": index}
    if index_node is not None and int(index_node.shape[0]):
        flags["index_node"] = index_node
    gaussian = types.SimpleNamespace(keys=keys, active_sh_degree=degree, items=lambda: ((k, bufs[k]) for k in keys),
                                     visibility_flag=flags)
    return types.SimpleNamespace(gaussian=gaussian, fix_parent=True, training=True)


def torch_get_all64(bufs, index, index_node, campos, degree):
    """level_of_gaussian.py:262-296 + activation.py:27-44 restated in float64 torch for degrees 0..3: gather, exp, sigmoid,
    normalize, SH2RGB + the real SH polynomial over the higher coefficients (shs[:, k - 1] is coefficient k), the direction
    taken from detached xyz, no clamp.  For (degree, K) pairs no reference configuration produces.
    -> (params, activated)."""
    C0, C1 = 0.28209479177387814, 0.4886025119029199
    C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
    C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
          1.445305721320277, -0.5900435899266435]
    b64 = {k: v.double() for k, v in bufs.items()}
    params = {k: torch.nn.Parameter(v[index]) for k, v in b64.items()}
    full = {k: torch.cat([params[k], v[index_node]]) for k, v in b64.items()}
    colors = full["colors"] * C0 + 0.5
    if degree > 0:
        d = full["xyz"].detach() - campos.double()[None]
        d = d / torch.norm(d, dim=-1, keepdim=True)
        x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
        sh = full["shs"]
        colors = colors - C1 * y * sh[:, 0] + C1 * z * sh[:, 1] - C1 * x * sh[:, 2]
        if degree > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            colors = colors + C2[0] * xy * sh[:, 3] + C2[1] * yz * sh[:, 4] + C2[2] * (2 * zz - xx - yy) * sh[:, 5] + \
                C2[3] * xz * sh[:, 6] + C2[4] * (xx - yy) * sh[:, 7]
        if degree > 2:
            colors = colors + C3[0] * y * (3 * xx - yy) * sh[:, 8] + C3[1] * xy * z * sh[:, 9] + \
                C3[2] * y * (4 * zz - xx - yy) * sh[:, 10] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 11] + \
                C3[4] * x * (4 * zz - xx - yy) * sh[:, 12] + C3[5] * z * (xx - yy) * sh[:, 13] + \
                C3[6] * x * (xx - 3 * yy) * sh[:, 14]
    act = {"xyz": full["xyz"], "scaling": torch.exp(full["scaling"]), "opacity": torch.sigmoid(full["opacity"]),
           "rotation": torch.nn.functional.normalize(full["rotation"]), "colors": colors}
    return params, act
