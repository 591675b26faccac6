"""Absolute screen-space gradients in float64: a dense restatement of the COMPOSITING only.  TEST INFRASTRUCTURE ONLY.

The projected quantities (ndc centre, conic, visibility, radius, depth) come from ``oracle/torch_oracle.project``; the
compositing is ``torch_oracle.render``'s, line for line, except that the pixel-to-centre offsets ``dx`` / ``dy`` are leaf
tensors [pixels, Gaussians] with ``retain_grad()``: after backpropagating ``sum(image * w)`` their gradients are the
per-pixel, per-Gaussian terms whose signed sum over pixels (times 0.5 W / 0.5 H) is dL/dmeans2D -- and whose sum of absolute
values is the quantity ``lograst_backward_abs`` produces:

    abs[g, 0] = 0.5 W * sum_p |dL/ddx[p, g]|,   abs[g, 1] = 0.5 H * sum_p |dL/ddy[p, g]|

``signed`` (the same sums without the absolute value) pins the restatement: it must equal the ``means2D`` gradient of
``torch_oracle.render`` on the same inputs (tests/test_abs_grad_cpu.py: within 1e-12 relative).  Small scenes only."""
import numpy as np
import torch

from oracle import torch_oracle as TO

PIXEL_CHUNK = 2048


def absgrad(width, height, tanfovx, tanfovy, viewmatrix, projmatrix, bg, means3D, scales, rotations, opacities, colors,
            weights, scale_modifier=1.0, filter_mode=TO.FILTER_CLAMP, ndc_cull=True):
    """-> dict(abs [N, 2], signed [N, 2], image [3, H, W], radii [N]) as float64 / int numpy arrays; weights = dL/dimage."""
    dt = torch.float64
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dt)
    viewmatrix, projmatrix, bg = T(viewmatrix), T(projmatrix), T(bg)
    means3D, scales, rotations, colors = T(means3D), T(scales), T(rotations), T(colors)
    opacities, weights = T(opacities).reshape(-1), T(weights)
    N = means3D.shape[0]
    W, H = int(width), int(height)
    with torch.no_grad():
        pr = TO.project(width, height, tanfovx, tanfovy, viewmatrix, projmatrix, means3D, torch.zeros(N, 3, dtype=dt), scales,
                        rotations, scale_modifier=scale_modifier, filter_mode=filter_mode, ndc_cull=ndc_cull)
    ndc, (cA, cB, cC), vis, radius, tz = pr["ndc"], pr["conic"], pr["vis"], pr["radius"], pr["tz"]
    mx = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5
    my = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5
    gx, gy = (W + 15) // 16, (H + 15) // 16
    x0 = torch.clamp(torch.trunc((mx - radius) / 16), 0, gx)
    y0 = torch.clamp(torch.trunc((my - radius) / 16), 0, gy)
    x1 = torch.clamp(torch.trunc((mx + radius + 15) / 16), 0, gx)
    y1 = torch.clamp(torch.trunc((my + radius + 15) / 16), 0, gy)
    vis = vis & (((x1 - x0) * (y1 - y0)) > 0)
    radii = torch.where(vis, radius, torch.zeros_like(radius)).to(torch.int32)
    depth32 = tz.to(torch.float32)
    order = torch.argsort(depth32.to(dt) * 1.0, stable=True)
    o = order[vis[order]]
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    px, py = xs.reshape(-1), ys.reshape(-1)
    tix, tiy = torch.div(px, 16, rounding_mode="floor"), torch.div(py, 16, rounding_mode="floor")
    out_abs, out_signed = np.zeros((N, 2)), np.zeros((N, 2))
    image = torch.zeros(H * W, 3, dtype=dt)
    wpix = weights.reshape(3, H * W).t()                                         # [pixels, 3]
    idx = o.numpy()
    # pixels in chunks (every pixel composites on its own: the chunking changes no number, only the memory)
    for p0 in range(0, H * W, PIXEL_CHUNK):
        sl = slice(p0, min(H * W, p0 + PIXEL_CHUNK))
        member = (tix[sl, None] >= x0[o][None]) & (tix[sl, None] < x1[o][None]) & \
                 (tiy[sl, None] >= y0[o][None]) & (tiy[sl, None] < y1[o][None])
        dx = (mx[o][None, :] - px[sl, None]).clone().requires_grad_(True)        # the leaves: [pixels, K]
        dy = (my[o][None, :] - py[sl, None]).clone().requires_grad_(True)
        power = -0.5 * (cA[o][None] * dx * dx + cC[o][None] * dy * dy) - cB[o][None] * dx * dy
        G = torch.exp(torch.clamp(power, max=0.0))
        raw = opacities[o][None] * G
        alpha = raw + (torch.clamp(raw, max=0.99) - raw).detach()               # straight-through cap
        ok = member & (power.detach() <= 0) & (alpha.detach() >= 1.0 / 255.0)
        alpha_eff = torch.where(ok, alpha, torch.zeros_like(alpha))
        one_m = 1.0 - alpha_eff
        Tincl = torch.cumprod(one_m, dim=1)
        Texcl = torch.cat([torch.ones_like(Tincl[:, :1]), Tincl[:, :-1]], dim=1)
        stop = ok & (Tincl.detach() < 1e-4)
        stopped = torch.cumsum(stop.to(torch.int64), dim=1) > 0
        use = ok & ~stopped
        w = torch.where(use, alpha_eff * Texcl, torch.zeros_like(alpha_eff))
        C = w @ colors[o]
        T_final = torch.prod(torch.where(use, one_m, torch.ones_like(one_m)), dim=1)
        img = C + T_final[:, None] * bg[None, :]
        image[sl] = img.detach()
        if o.shape[0] > 0:
            (img * wpix[sl]).sum().backward()
            out_abs[idx, 0] += (0.5 * W * dx.grad.abs().sum(dim=0)).numpy()
            out_abs[idx, 1] += (0.5 * H * dy.grad.abs().sum(dim=0)).numpy()
            out_signed[idx, 0] += (0.5 * W * dx.grad.sum(dim=0)).numpy()
            out_signed[idx, 1] += (0.5 * H * dy.grad.sum(dim=0)).numpy()
    image = image.t().reshape(3, H, W)
    return dict(abs=out_abs, signed=out_signed, image=image.numpy(), radii=radii.numpy())


def render_means2d_grad(width, height, tanfovx, tanfovy, viewmatrix, projmatrix, bg, means3D, scales, rotations, opacities,
                        colors, weights, scale_modifier=1.0, filter_mode=TO.FILTER_CLAMP, ndc_cull=True):
    """dL/dmeans2D [N, 2] of ``torch_oracle.render`` itself under the same loss: what ``signed`` above must reproduce."""
    dt = torch.float64
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64), dtype=dt)
    m2 = torch.zeros(len(means3D), 3, dtype=dt, requires_grad=True)
    image, _, _ = TO.render(width, height, tanfovx, tanfovy, T(viewmatrix), T(projmatrix), T(bg), T(means3D), m2, T(scales),
                            T(rotations), T(opacities).reshape(-1), T(colors), scale_modifier=scale_modifier,
                            filter_mode=filter_mode, ndc_cull=ndc_cull)
    (image * T(weights)).sum().backward()
    return m2.grad[:, :2].numpy(), image.detach().numpy()


def of_case(cam, sc, bg, weights, flavour=None):
    """absgrad() on a scene of the tests' builders (cam / sc dicts); flavour: a log_amd.rasterizer.Flavour (default: the fork)."""
    from util import cam_tan
    tfx, tfy = cam_tan(cam)
    fm, cull = (TO.FILTER_CLAMP, True) if flavour is None else (flavour.filter_mode, bool(flavour.ndc_cull))
    return absgrad(cam["image_width"], cam["image_height"], tfx, tfy, cam["world_view_transform"], cam["full_proj_transform"],
                   bg, sc["xyz"], sc["scaling"], sc["rotation"], sc["opacity"], sc["colors"], weights, filter_mode=fm,
                   ndc_cull=cull)


def centred_splat(W=32, H=32, sigma_px=3.0, opacity=0.8, z=4.0, focal=None):
    """One isotropic Gaussian whose projected centre is the pixel centre (W / 2, H / 2) -- in this pixel convention
    (pixel centres at integers: mx = ((ndc + 1) W - 1) / 2) that is ndc = 1 / W, exactly representable, and with
    tan(fov / 2) = 0.5 and z = 4 the world position 2 / W is exact too -- seen by an identity camera down +z.
    -> (cam, sc) in the tests' dict layout."""
    tan = 0.5
    fx = W / (2.0 * tan)
    V = np.eye(4, dtype=np.float32)
    P = np.zeros((4, 4), np.float32)       # row-vector convention: hom = [p 1] P
    P[0, 0], P[1, 1] = 1.0 / tan, 1.0 / tan
    P[2, 2], P[2, 3], P[3, 2] = 1.0, 1.0, -0.01
    cam = dict(image_width=W, image_height=H, FoVx=2.0 * np.arctan(tan), FoVy=2.0 * np.arctan(tan),
               world_view_transform=V, full_proj_transform=P, camera_center=np.zeros(3, np.float32))
    s = sigma_px * z / fx                  # world-space sigma that projects to sigma_px pixels
    sc = dict(xyz=np.array([[tan * z / W * 1.0, tan * z / H * 1.0, z]], np.float32),
              scaling=np.full((1, 3), s, np.float32), rotation=np.array([[1.0, 0.0, 0.0, 0.0]], np.float32),
              opacity=np.array([[opacity]], np.float32), colors=np.array([[0.7, 0.4, 0.9]], np.float32))
    return cam, sc
