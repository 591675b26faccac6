"""tests/step_ref.py (the float64 restatement of get_all, native SH and sparse Adam that the randomised sweep of the step
kernels measures against) held to the reference's recorded results: installed behind the drop-ins in place of the kernels,
it has to pass the checks the kernels pass on tests/golden/getall_*.npz, adam_*.npz, train_random_*.npz and sh_basis.npz --
the same helper functions, so the same assertions and tolerances."""
import os

import numpy as np
import pytest
import torch

import getall_util as GU
import step_ref
import train_util as TU


def _installed(dtype):
    from log_amd import rasterizer as R
    import oracle_backend
    old = oracle_backend.install(step_ref.StepRefBackend(oracle_backend.OracleBackend(), dtype))
    yield dtype
    oracle_backend.install(None if isinstance(old, R.HipBackend) else old)


@pytest.fixture(params=[torch.float64, torch.float32], ids=["float64", "float32"])
def restatement(request, oracle_mod):
    yield from _installed(request.param)


# (seed, dtype) of the reference's random cases: every seed in float32, and in float64 all but seed 1 (see the test)
RANDOM_CASES = [(s, torch.float32) for s in range(6)] + [(s, torch.float64) for s in (0, 2, 3, 4, 5)]


@pytest.fixture()
def restatement_of_case(request, oracle_mod):
    yield from _installed(request.getfixturevalue("case")[1])


@pytest.mark.parametrize("path", GU.GOLDEN, ids=[os.path.basename(p) for p in GU.GOLDEN])
def test_get_all_restatement_matches_reference_activation_and_autograd(path, restatement):
    from log_amd import get_all
    g = np.load(path)
    model, camera = GU.log_like(g, "cpu")
    GU.check(g, model, camera, get_all.get_all)


@pytest.mark.parametrize("name", ["adam_a.npz", "adam_ams.npz"])
def test_adam_restatement_matches_reference_optimizer(name, restatement):
    from log_amd import sparse_optimizer
    g = TU.load(name)
    model, opt = TU.run_adam(g, "cpu", sparse_optimizer.step)
    TU.check_adam(model, opt, g)


@pytest.mark.parametrize("case", RANDOM_CASES, ids=["%d-%s" % (s, str(t)[6:]) for s, t in RANDOM_CASES])
def test_adam_restatement_on_the_reference_random_cases(case, restatement_of_case):
    """Every recorded random case holds the float32 evaluation of the restatement, and every case but seed 1 the float64 one.
    The recorded results are fp32 results: where m = g (1-b1) + m b1 cancels, a float64 value differs from ANY fp32
    evaluation by up to 2^-24 * S_m.  In seed 1 one element of 14475 of exp_avg (shs) sits 4.1e-6 (8.4e-12 absolute) from the
    recorded value, above the 3e-6 of the check, with every formula right -- the one (seed, dtype) pair not in RANDOM_CASES;
    test_float64_and_float32_evaluations_agree_within_the_condition_scale ties the two evaluations together."""
    TU.check_random_case(case[0], "cpu")


def test_float64_and_float32_evaluations_agree_within_the_condition_scale():
    """|ref32 - ref64| <= 4 * 2^-24 * S on every Adam output (m, v: two roundings per term; the parameter: m, the root, two
    divisions and the sum), prior moments of both signs so that m cancels."""
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g)
    for amsgrad in (False, True):
        p, gr, m0 = rnd(4000, 7), rnd(4000, 7) * 1e-3, rnd(4000, 7) * 1e-4
        v0, vm = (rnd(4000, 7) * 1e-3) ** 2, (rnd(4000, 7) * 1e-3) ** 2
        args = (p, gr, m0, v0, vm if amsgrad else None, 1e-3 / (1 - 0.9 ** 3), 0.9, 0.999, (1 - 0.999 ** 3) ** 0.5, 1e-15)
        r64, r32 = step_ref.adam(*args), step_ref.adam(*args, dtype=torch.float32)
        for k in ("param", "exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ()):
            err = (r32[k].double() - r64[k]).abs()
            assert bool((err <= 4 * 2.0 ** -24 * r64["S_" + k]).all()), (k, float((err / r64["S_" + k]).max()) * 2 ** 24)


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_native_sh_restatement_matches_reference_sh_utils(degree):
    """As tests/test_sh.py::test_oracle_basis_matches_reference_sh_utils, same inputs and tolerance; the monomial table that
    yields the condition scales reproduces the basis the colours were computed with."""
    from test_sh import _inputs
    means, campos, shs = _inputs(scale=0.2)
    r = step_ref.native_sh(torch.from_numpy(means), torch.from_numpy(campos), torch.from_numpy(shs), degree)
    assert not r["clamped"].any()
    ref = np.load(os.path.join(TU.GOLDEN_DIR, "sh_basis.npz"))["colour_deg%d" % degree]
    np.testing.assert_allclose(r["colors"].numpy(), ref, rtol=2e-5, atol=2e-6)
    d, _ = step_ref.direction(torch.from_numpy(means).double(), torch.from_numpy(campos).double())
    nk = (degree + 1) ** 2
    own = 0.5 + (step_ref.sh_basis(d, nk)[:, :, None] * torch.from_numpy(shs).double()[:, :nk]).sum(dim=1)
    np.testing.assert_allclose(own.numpy(), r["colors"].numpy(), rtol=1e-12, atol=1e-13)
    assert bool((r["S_colors"] >= r["colors"].abs() - 1e-12).all())


def test_condition_scales_bound_their_values():
    """S >= |value| for every output, by construction (the triangle inequality), on a random case with planted rows."""
    g = torch.Generator().manual_seed(3)
    P, n, K, deg = 500, 300, 8, 2
    rnd = lambda *s: torch.randn(*s, generator=g)
    bufs = {"xyz": rnd(P, 3), "scaling": rnd(P, 3), "opacity": rnd(P, 1) * 5, "rotation": rnd(P, 4), "colors": rnd(P, 3),
            "shs": rnd(P, K, 3)}
    bufs["rotation"][:5] = 0.0
    index = torch.randperm(P, generator=g)[:n]
    ups = {k: rnd(n, w) for k, w in (("xyz", 3), ("scaling", 3), ("opacity", 1), ("rotation", 4), ("colors", 3))}
    r = step_ref.get_all(bufs, index, 200, deg, torch.tensor([0.1, 2.0, -1.0]), ups)
    for k, v in r["act"].items():
        assert bool((r["S_act"][k] >= v.abs() * (1 - 1e-12)).all()), k
    for k, v in r["grads"].items():
        assert v.shape[0] == 200 and bool((r["S_grads"][k] >= v.abs() * (1 - 1e-12)).all()), k
    assert bool((r["grads"]["shs"][:, 8:] == 0).all()) if K > 8 else True
    s = step_ref.native_sh(bufs["xyz"], torch.tensor([0.1, 2.0, -1.0]), rnd(P, 16, 3), 3, rnd(P, 3))
    assert s["clamped"].any()
    for k in ("colors", "g_shs", "g_means3D"):
        assert bool((s["S_" + k] >= s[k].abs() * (1 - 1e-9) - 1e-300).all()), k
