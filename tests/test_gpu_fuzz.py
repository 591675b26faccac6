"""A fixed slice of the randomised parity sweep (tools/fuzz_parity.py; the full 1200-case run of the round:
profiles/r06_fuzz_parity.md): scenes, cameras, flavours, paths, compositing forms and launch-shape knobs drawn per seed --
forward bit for bit the oracle's, gradients to the criteria of tests/gpu_util.py."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

SEEDS = [100000 + i for i in range(0, 24)] + [200000 + i for i in range(0, 12)] + [300000 + i for i in (239, 253, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250)]


@pytest.mark.parametrize("block", range(6))
def test_random_cases_vs_oracle(oracle_mod, block):
    import fuzz_parity as F
    ran = 0
    for seed in SEEDS[block * 8:(block + 1) * 8]:
        r = F.run_case(oracle_mod, seed)
        ran += "skipped" not in r
    assert ran >= 6


# ---- the other kinds of call (tools/fuzz_parity.py --mode calls; the full run: profiles/fuzz_calls.md) -------------------
# One block per kind, eight seeds each, chosen on the CPU from draw_call and the rect rule's instance count (the number behind
# each seed: what the oracle walks, twice for aux / second_pass).  Relations per kind, every call through the public packages
# under the drawn flavour, forms, hit masks, knobs, scale_modifier, background and use_filter, the main call in the drawn
# capacity mode (exact / speculative / fixed / a speculative guess that is too small), its comparator in exact mode:
#   aux          one call with aux_colors == the two-call pair, reuse off: every output bit for bit (and both images the
#                oracle's), the quadrant kernels ran, reverse-walk gradients within GRAD_TOL of the pair's sums, dL/dmeans3D /
#                dL/dscales / dL/drotations anchored on the oracle's two backwards (fp32 and float64) added
#   second_pass  two calls reuse off / two calls reuse on through a fresh object / the oracle with the second call's colours:
#                both calls' outputs bit for bit in all three, gradients as for aux, geometry_reuse_stats() says recomposited
#   camera       image bit for bit the call without camera gradients, column 3 of dL/dV and column 2 of dL/dP exactly 0.0,
#                reverse-walk gradients within GRAD_TOL of the backward without the camera sums, a view that sees nothing gives
#                zeros; isolated chain rule on fixed upstream gradients: per-Gaussian outputs the bits of camera=False, two calls
#                the same bits, dL/dV and dL/dP within GRAD_TOL per matrix of float64 autograd of the projection alone under
#                the fp32 forward's decisions (rows where fp32 and float64 decide differently: dropped on both sides, <= 1 %)
#   shs          shs= == colors_precomp set to the backend's own sh_forward: forward bit for bit, dL/dshs against sh_backward of
#                the comparator's dL/dcolors, dL/dmeans3D minus that call's view-direction term anchored on the oracle
#   cov3d        cov3D_precomp from the scene's scales and rotations: forward bit for bit the oracle's cov3D path, gradients
#                within GRAD_TOL of the oracle, or held by the anchored criterion on a float64 twin of the cov3D chain rule
# Every mode: no overflow recorded; under the guess that is too small, capacity_stats() shows the repeated stage 2.
CALL_SEEDS = {
    "aux": [500153,          # 39698
            500728,          # 1269
            500142,          # 100299 (fog, one list of 100299 entries on a 2 x 11 image: parks and resumes)
            500289,          # 82527
            500716,          # 14925
            500091,          # 19786
            500137,          # 18986
            500734],         # 19966
    "second_pass": [500639,  # 19535
                    500015,  # 664
                    500020,  # 73121
                    500517,  # 2452
                    500552,  # 17692
                    500239,  # 19986
                    500474,  # 19034
                    500081],  # 16320
    "camera": [500405,       # 102
               500439,       # 29923
               500682,       # 6
               500768,       # 73245
               500415,       # 7021
               500108,       # 21098
               500708,       # 23859
               500205],      # 0 (a view that sees nothing)
    "shs": [500435,          # 45649
            500796,          # 54444
            500143,          # 339
            500367,          # 30
            500234,          # 19941
            500260,          # 22133
            500133,          # 22829
            500102],         # 16955
    "cov3d": [500574,        # 25951
              500311,        # 6385
              500300,        # 522
              500333,        # 26092
              500372,        # 19440
              500519,        # 31653
              500049,        # 19594
              500053],       # 20515
}
# The seeds that failed in the two full runs (profiles/fuzz_calls.md), each after its fix; no kernel changed.
# cov3d, run 1: failed the sweep's first criterion for the outputs behind the chain rule (relative L2 over ALL rows against a
# float64 reference, no conditioning: needles and pancakes own that norm) -- replaced by the anchored criterion of run_case with
# a float64 twin of the cov3D chain rule.  (The sixth seed of that cause, 600643, walks 1.56 M instances through the oracle: 6 s,
# too long for a test; `--mode calls --only 600643` replays it.)
# aux, run 2: 700579 -- the float64 twin of a SUM of two backwards added the addends' chain32 values, signs and all, and called
# the one row that owns the figure well-conditioned; `_sum_f64` now adds the addends' units (tests/test_fuzz_calls_cpu.py).
CALL_REGRESSIONS = [600084,   # cov3d, 2042 instances (dL/dmeans2D 1.2e-4 from the fp32 oracle: held through the float64 sums)
                    600090,   # cov3d, 7343
                    600229,   # cov3d, 6272
                    600544,   # cov3d, 129041
                    600870,   # cov3d, 12347
                    700579]   # aux, 38102


def _held_in_full(r):
    """No value check of a slice case may be passed over: not skipped, and none of the recorded exits taken."""
    assert "skipped" not in r, r                           # no case of the slice may be skipped
    assert "camera_ref_finite" not in r, r                 # (camera: the float64 reference was finite, the values were held)
    assert r.get("sh_backward_held", True), r              # (shs: sh_backward was held against the oracle)


@pytest.mark.parametrize("kind", list(CALL_SEEDS))
def test_random_calls(oracle_mod, kind):
    import fuzz_parity as F
    too_small = 0
    for seed in CALL_SEEDS[kind]:
        r = F.run_call(oracle_mod, seed)
        assert r["kind"] == kind
        _held_in_full(r)
        if kind == "second_pass":                          # (a slice that only ever falls back tests nothing)
            assert r["reuse"] == "reused", r
        too_small += r.get("capacity_ran") == "speculative_too_small" and r["retries"] >= 1
    assert too_small >= 1                                  # a guess that really was too small, on the device, in every block


@pytest.mark.parametrize("seed", CALL_REGRESSIONS)
def test_random_calls_regressions(oracle_mod, seed):
    import fuzz_parity as F
    _held_in_full(F.run_call(oracle_mod, seed))


def test_random_cases_bands_and_bucket_accumulation():
    """The same draws through the packages' autograd drop-in: the image split into 2 / 3 / 5 / 8 bands of tile rows renders the
    whole image bit for bit (radii / point_weight: maxima over the bands; reverse-walk gradients: sums), and views
    accumulated by the backward kernels into a row-major / planar gradient bucket equal autograd's own accumulation."""
    import fuzz_parity as F
    banded = 0
    for seed in [400000 + i for i in range(0, 40)]:
        r = F.run_props(seed)
        banded += bool(r.get("bands"))
    assert banded >= 20
