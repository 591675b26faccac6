"""TEST INFRASTRUCTURE shared by tests/test_camera_grad_cpu.py and tests/test_gpu_camera_grad.py: the scenes of the camera-
gradient tests and their reference, the float64 autograd twin (oracle/torch_oracle.py::render is differentiable in
viewmatrix / projmatrix as it stands).

Every scene is a dict(cam=, sc=, package=, use_filter=, scale_modifier=, V=, P=): V / P default to the camera's matrices.
The loss is sum(image * dL) with dL = default_rng(1).random(image.shape): the weights every parity test of the suite uses.
The CPU file holds, for every scene listed in SCENES, that the twin's camera gradients are well conditioned (all inputs
rounded through fp32 move them by less than 1e-5 relative L2), which is what makes GRAD_TOL = 1e-4 a fair bound for fp32
kernels; the GPU file compares the kernels with the twin on the same scenes."""
import numpy as np
import torch

from log_amd import scenes
from util import cam_tan, small_case

BG = (0.3, 0.6, 0.9)
FLAVOURS = {"wodilate": dict(filter_mode=2, ndc_cull=True), "upstream": dict(filter_mode=1, ndc_cull=False)}
PER_GAUSSIAN = ("means3D", "means2D", "scales", "rotations", "opacities", "colors")


def case(cam, sc, package="wodilate", use_filter=True, scale_modifier=1.0, V=None, P=None):
    return dict(cam=cam, sc=sc, package=package, use_filter=use_filter, scale_modifier=scale_modifier,
                V=np.asarray(cam["world_view_transform"] if V is None else V, np.float32),
                P=np.asarray(cam["full_proj_transform"] if P is None else P, np.float32))


def rows_case(n):
    """n Gaussians in the small view (row-count edges of the chain rule's 1024-row workgroup)."""
    cam, sc = small_case(n=max(n, 1), seed=5, opacity=None, smax=0.12 if n > 500 else 0.25)
    if n == 0:
        sc = {k: v[:0] for k, v in sc.items()}
    return case(cam, sc)


def dead_middle_case():
    """2049 rows in three workgroups of the chain rule, rows [0, 1024), [1024, 2048), [2048, 2049): the whole middle one is
    behind the camera (a workgroup without a live row)."""
    cam, sc = small_case(n=2049, seed=6, opacity=None, smax=0.12)
    sc = {k: v.copy() for k, v in sc.items()}
    behind = np.asarray(cam["camera_center"], np.float32) - 2.0 * np.asarray(cam["R"], np.float32)[2]   # 2 units behind
    sc["xyz"][1024:2048] = behind + 0.1 * sc["xyz"][1024:2048]
    return case(cam, sc)


def culled_case():
    """A view that sees nothing: every Gaussian at the camera centre (tests/test_gpu_recomposite.py::_culled_scene)."""
    cam, sc = small_case(n=150, seed=0)
    sc = dict(sc)
    sc["xyz"] = np.tile(np.asarray(cam["camera_center"], np.float32), (len(sc["xyz"]), 1))
    return case(cam, sc)


def ragged_case(reduced=False):
    """tests/test_gpu_recomposite.py::_ragged (2000 Gaussians, 150x97); reduced: the same generator at a size whose finite
    differences the dense twin takes in seconds (300 Gaussians, 75x49, the same field of view).  Finite differences need a
    neighbourhood of the scene without a flip of one of the forward's decisions (tile rect, alpha floor, cull): 300
    Gaussians have one, 400 of the same generator have a flip within 1e-7 of the scene."""
    if reduced:
        return case(*small_case(n=300, W=75, H=49, focal=85.0, seed=3, smax=0.08))
    return case(*small_case(n=2000, W=150, H=97, focal=170.0, seed=3, smax=0.08))


def skewed_case():
    """A slightly non-orthonormal V (and the P that goes with it): all 12 entries of V[:, :3] are free variables."""
    cam, sc = small_case(n=150, seed=2, opacity=None)
    rng = np.random.default_rng(11)
    V = np.asarray(cam["world_view_transform"], np.float64).copy()
    proj = np.linalg.inv(V) @ np.asarray(cam["full_proj_transform"], np.float64)
    V[:, :3] += 0.01 * rng.standard_normal((4, 3))
    return case(cam, sc, V=V, P=V @ proj)


def clamp_case():
    """Off-centre principal point (cx = 0.2 W, cy = 0.25 H): ndc.x = (t.x / t.z) / tanfovx - 0.6, so Gaussians with t.x / t.z in
    (1.3, 1.6) tanfovx are on screen, survive the |ndc| <= 1.3 cull and take the EWA Jacobian's clamp branch (likewise y in
    (1.3, 1.5) tanfovy).  A third of the Gaussians are small enough for the CLAMP low-pass to clamp their diagonals."""
    W, H, focal = 48, 40, 60.0
    base = scenes.orbit_cameras(3, W=W, H=H, focal=focal, radius=2.5)[1]
    K = np.array([[focal, 0, 0.2 * W], [0, focal, 0.25 * H], [0, 0, 1.0]])
    cam = scenes.make_camera(base["R"], base["T"], K, W, H)
    sc = scenes.random_scene(600, seed=8, opacity=None, smax=0.2, extent=2.2)
    sc["scaling"][::3] *= 0.04
    return case(cam, sc)


def clamp_branch_counts(c, tw):
    """Composited Gaussians (twin point_weight > 0) in the x clamp branch, the y clamp branch, and with a clamped low-pass
    diagonal -- from the inputs, in float64."""
    cam, sc = c["cam"], c["sc"]
    tfx, tfy = cam_tan(cam)
    V = c["V"].astype(np.float64)
    p = sc["xyz"].astype(np.float64)
    t = p @ V[:3, :3] + V[3, :3]
    live = tw["point_weight"] > 0
    cx = np.abs(t[:, 0] / t[:, 2]) > 1.3 * tfx
    cy = np.abs(t[:, 1] / t[:, 2]) > 1.3 * tfy
    # raw EWA diagonals
    fx, fy = cam["image_width"] / (2 * tfx), cam["image_height"] / (2 * tfy)
    s = sc["scaling"].astype(np.float64) * c["scale_modifier"]
    from oracle import torch_oracle
    R = torch_oracle._rot(torch.tensor(sc["rotation"], dtype=torch.float64)).numpy()
    M = R * s[:, None, :]
    Sigma = M @ M.transpose(0, 2, 1)
    tz = t[:, 2]
    ux = np.clip(t[:, 0] / tz, -1.3 * tfx, 1.3 * tfx)
    uy = np.clip(t[:, 1] / tz, -1.3 * tfy, 1.3 * tfy)
    J = np.zeros((len(p), 2, 3))
    J[:, 0, 0], J[:, 0, 2], J[:, 1, 1], J[:, 1, 2] = fx / tz, -fx * ux / tz, fy / tz, -fy * uy / tz
    T = J @ V[:3, :3].T
    cov = T @ Sigma @ T.transpose(0, 2, 1)
    low = (cov[:, 0, 0] < 0.3) | (cov[:, 1, 1] < 0.3)
    return int((live & cx).sum()), int((live & cy).sum()), int((live & low).sum())


SCENES = {
    "small-wodilate-filter": lambda: case(*small_case(seed=0, opacity=None), package="wodilate", use_filter=True),
    "small-wodilate-nofilter": lambda: case(*small_case(seed=0, opacity=None), package="wodilate", use_filter=False),
    "small-upstream-filter": lambda: case(*small_case(seed=0, opacity=None), package="upstream", use_filter=True),
    "small-upstream-nofilter": lambda: case(*small_case(seed=0, opacity=None), package="upstream", use_filter=False),
    "scale-modifier": lambda: case(*small_case(seed=1, opacity=None), scale_modifier=1.7),
    "skewed-V": skewed_case,
    "clamp-branches": clamp_case,
    "ragged": ragged_case,
    "dead-middle-2049": dead_middle_case,
    **{f"rows-{n}": (lambda n=n: rows_case(n)) for n in (1, 63, 65, 1023, 1024, 1025)},
}
# the scenes whose finite differences the CPU file takes at a size the dense twin differentiates 48 times in seconds
REDUCED = {"ragged": lambda: ragged_case(reduced=True), "dead-middle-2049": lambda: rows_case(65),
           "rows-1023": lambda: rows_case(63), "rows-1024": lambda: rows_case(65), "rows-1025": lambda: rows_case(65)}


def dL_of(c):
    cam = c["cam"]
    return np.random.default_rng(1).random((3, cam["image_height"], cam["image_width"]), dtype=np.float32)


def twin(c, device="cpu", unrounded=False, V=None, P=None, grads=True):
    """The float64 twin's loss and gradients for scene c: dict(loss=, V=, P=, <per-Gaussian gradients>, radii=,
    point_weight=), numpy float64.  The scene's arrays are fp32 values: what the kernels read.  unrounded: every input x
    (Gaussians, V, P) is replaced by the float64 x (1 + u 2^-25), u uniform in (-1, 1) from a fixed seed -- float64 inputs
    whose rounding through fp32 is the scene (the conditioning check compares the two).  V / P: override the scene's
    matrices (finite differences); float64 torch tensors are taken as they are, with their graph (a pose in front of the
    camera: the caller reads the gradient off its own leaf, out["V"] / out["P"] are then zeros)."""
    from oracle import torch_oracle
    cam, sc = c["cam"], c["sc"]
    dev = torch.device(device)
    tfx, tfy = cam_tan(cam)
    rng = np.random.default_rng(2)

    def T(a):
        a = np.asarray(a, np.float64)
        if unrounded:
            a = a * (1.0 + (2.0 * rng.random(a.shape) - 1.0) * 2.0 ** -25)
        return torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=grads)
    n = len(sc["xyz"])
    leaves = dict(means3D=T(sc["xyz"]), scales=T(sc["scaling"]), rotations=T(sc["rotation"]),
                  opacities=T(sc["opacity"]), colors=T(sc["colors"]), means2D=T(np.zeros((n, 3))))
    Vt, Pt = (x if torch.is_tensor(x) else T(d if x is None else x) for x, d in ((V, c["V"]), (P, c["P"])))
    fl = FLAVOURS[c["package"]]
    with torch.device(dev):
        img, radii, aux = torch_oracle.render(
            cam["image_width"], cam["image_height"], tfx, tfy, Vt, Pt, torch.tensor(BG, dtype=torch.float64, device=dev),
            leaves["means3D"], leaves["means2D"], leaves["scales"], leaves["rotations"], leaves["opacities"], leaves["colors"],
            scale_modifier=c["scale_modifier"], filter_mode=fl["filter_mode"] if c["use_filter"] else 0, ndc_cull=fl["ndc_cull"])
        loss = (img * torch.tensor(dL_of(c), dtype=torch.float64, device=dev)).sum()
    out = dict(loss=float(loss.detach()), radii=radii.cpu().numpy(), point_weight=aux["point_weight"].cpu().numpy())
    if grads:
        if loss.requires_grad:
            loss.backward()
        z = lambda t: (t.grad if t.is_leaf and t.grad is not None else torch.zeros_like(t)).detach().cpu().numpy()
        out.update(V=z(Vt), P=z(Pt), **{k: z(v) for k, v in leaves.items()})
    return out


def finite_differences(c, h=1e-7):
    """Central differences of the twin's loss in the 16 + 16 entries of V and P, float64."""
    V0, P0 = c["V"].astype(np.float64), c["P"].astype(np.float64)
    gV, gP = np.zeros((4, 4)), np.zeros((4, 4))
    for which, g in (("V", gV), ("P", gP)):
        for r in range(4):
            for k in range(4):
                d = np.zeros((4, 4))
                d[r, k] = h
                kw = lambda sgn: {which: (V0 if which == "V" else P0) + sgn * d}
                g[r, k] = (twin(c, grads=False, **kw(+1))["loss"] - twin(c, grads=False, **kw(-1))["loss"]) / (2 * h)
    return gV, gP
