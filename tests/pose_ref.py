"""TEST INFRASTRUCTURE: a float64 torch restatement of the pose parametrisation of log_amd/pose.py (csrc/pose.hip), with
autograd for its derivative.

A row xi = (omega[3], upsilon[3]) perturbs the camera frame: p_cam' = R(omega) p_cam + upsilon, R = I + A K + B K^2 (Rodrigues;
K = [omega]x, s = |omega|^2, A = sin(sqrt s) / sqrt s, B = (1 - cos(sqrt s)) / s).  In the rasterizer's row-vector convention
(p_cam = [p 1] V), with E = [[R^T - I, 0], [upsilon, 0]] and W = V E:

    V' = V + W,   P' = P + W (V^-1 P),   campos' = row 3 of V'^-1,

both inverses by the rigid closed form ([[A3, 0], [b, 1]]^-1 = [[A3^T, 0], [-b A3^T, 1]]).  Written as differences from V and
P, so that xi = 0 gives V and P exactly whatever the rounding of V^-1.  Below SERIES (s < 1e-2) A and B come from their
series through s^4: the first dropped term, s^5 / 39916800, is under 1e-17 there; above it the closed forms (B by the half
angle, 2 sin^2(th / 2) / s, which does not cancel) and their derivatives lose less than 1e-16 / s."""
import torch

SERIES = 1e-2


def coefficients(s, series=None):
    """(A, B) at s = |omega|^2; series: True / False forces one form, None = the switch at SERIES."""
    use_series = bool(s.detach() < SERIES) if series is None else series
    if use_series:
        A = 1.0 + s * (-1.0 / 6.0 + s * (1.0 / 120.0 + s * (-1.0 / 5040.0 + s * (1.0 / 362880.0))))
        B = 0.5 + s * (-1.0 / 24.0 + s * (1.0 / 720.0 + s * (-1.0 / 40320.0 + s * (1.0 / 3628800.0))))
    else:
        th = torch.sqrt(s)
        A = torch.sin(th) / th
        hs = torch.sin(0.5 * th) / (0.5 * th)
        B = 0.5 * hs * hs
    return A, B


def rotation_minus_identity(omega, series=None):
    x, y, z = omega[0], omega[1], omega[2]
    s = x * x + y * y + z * z
    A, B = coefficients(s, series)
    zero = torch.zeros_like(x)
    K = torch.stack([torch.stack([zero, -z, y]), torch.stack([z, zero, -x]), torch.stack([-y, x, zero])])
    return A * K + B * (omega[:, None] * omega[None, :] - s * torch.eye(3, dtype=omega.dtype))


def rigid_inverse(V):
    A3, b = V[:3, :3], V[3, :3]
    top = torch.cat([A3.t(), torch.zeros(3, 1, dtype=V.dtype)], dim=1)
    bottom = torch.cat([-(b @ A3.t()), torch.ones(1, dtype=V.dtype)])[None]
    return torch.cat([top, bottom], dim=0)


def camera(xi, V, P, series=None):
    """-> (V', P', campos'), float64; xi [6], V / P [4, 4] (any dtype: cast to float64 first)."""
    xi, V, P = xi.to(torch.float64), V.to(torch.float64), P.to(torch.float64)
    Rm = rotation_minus_identity(xi[:3], series)
    E = torch.cat([torch.cat([Rm.t(), torch.zeros(3, 1, dtype=torch.float64)], dim=1),
                   torch.cat([xi[3:], torch.zeros(1, dtype=torch.float64)])[None]], dim=0)
    W = V @ E
    Vn = V + W
    Pn = P + W @ (rigid_inverse(V) @ P)
    campos = rigid_inverse(Vn)[3, :3]
    return Vn, Pn, campos
