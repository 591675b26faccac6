"""Shapes and inputs shared by tests/test_sh_edges_cpu.py and tests/test_gpu_sh_edges.py: the native `shs=` kernels
(log_amd/csrc/sh.hip) at the edges of their wave-staged layout.

N: one row, a wave less / exactly / plus one row (63, 64, 65), a workgroup less / exactly / plus one row (255, 256, 257) and a
second workgroup whose second wave is a one-row tail (321).  M: every copy path (3 M % 4 == 0 for M = 4, 12, 16: float4;
M = 1, 5, 9: scalar), M above the active degree, and M that is no perfect square, each with every degree the entry points
admit for it ((degree + 1)^2 <= M).

Inputs as tests/test_sh.py draws them, coefficient scale 2.0 so that the clamp at 0 is reached.  The seed of a case is the
first one for which the float64 twin (oracle/torch_oracle.py: sh_colors) alone says that the case is usable: with a view
dependent term (degree > 0) it has clamped and unclamped channels, and at most 0.5 % of its channels lie within 1e-5 of
the clamp (those are left out of the clamp-mask comparison with the twin).  Degree 0 cannot reach the clamp at this scale:
0.5 + 0.2821 * [-1, 1] stays positive."""
import functools

import numpy as np
import torch

NS = (1, 63, 64, 65, 255, 256, 257, 321)
MS = (1, 4, 5, 9, 12, 16)
CAMPOS = np.array([3.0, 0.5, -0.2], np.float32)
NEAR_CLAMP = 1e-5          # |unclamped float64 colour| below this: the fp32 sign is not the twin's to decide
MAX_NEAR_CLAMP = 0.005     # at most this fraction of a case's channels


def degrees(M):
    return [d for d in range(4) if (d + 1) ** 2 <= M]


def cases(M):
    return [(n, M, d) for d in degrees(M) for n in NS]


def draw(n, M, seed, scale=2.0):
    rng = np.random.default_rng(seed)
    means = (rng.random((n, 3), dtype=np.float32) - 0.5) * 2
    shs = ((rng.random((n, M, 3), dtype=np.float32) - 0.5) * scale).astype(np.float32)
    return means, CAMPOS.copy(), shs


def twin_unclamped(means, campos, shs, degree):
    """The float64 twin's colour before the clamp: coefficients negated turn clamp_min(r, 0) into -clamp_max(r, 0), so the
    two calls together give r itself."""
    from oracle import torch_oracle
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    pos = torch_oracle.sh_colors(t(means), t(campos), t(shs), degree)                      # max(0.5 + s, 0)
    neg = torch_oracle.sh_colors(t(means), t(campos), -t(shs), degree)                     # max(0.5 - s, 0)
    s = torch.where(pos > 0, pos - 0.5, 0.5 - neg)
    return (0.5 + s).numpy()


def usable(n, M, degree, seed):
    means, campos, shs = draw(n, M, seed)
    r = twin_unclamped(means, campos, shs, degree)
    near = np.abs(r) <= NEAR_CLAMP
    if near.sum() > MAX_NEAR_CLAMP * r.size:
        return False
    sure = ~near
    return degree == 0 or bool((r[sure] < 0).any() and (r[sure] > 0).any())


@functools.lru_cache(maxsize=None)
def seed_of(n, M, degree):
    for seed in range(1000 * degree + 10 * M, 1000 * degree + 10 * M + 400):
        if usable(n, M, degree, seed):
            return seed
    raise AssertionError(("no usable seed", n, M, degree))


def inputs(n, M, degree):
    """-> means[n,3], campos[3], shs[n,M,3], dl_dcolors[n,3] (fp32)."""
    seed = seed_of(n, M, degree)
    means, campos, shs = draw(n, M, seed)
    g = np.random.default_rng(seed + 7).random((n, 3), dtype=np.float32)
    return means, campos, shs, g
