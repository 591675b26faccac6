"""A fixed slice of the randomised sweep of the step kernels (tools/fuzz_step_ops.py; the full runs: profiles/step_ops_tests.md):
get_all forward + backward, native SH, sparse Adam and the fused step on drawn shapes, contents and planted degenerate rows,
every output element against the float64 restatement tests/step_ref.py within F * (|ref32 - ref64| + 2^-24 S).  No case is
skipped.  tests/test_fuzz_step_cpu.py runs the same seeds through the oracle backend."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# Named regression cases (docs/HISTORY.md):
#   100175          fused step with amsgrad, rows exactly at the camera (NaN direction, NaN SH gradient): fmaxf in the amsgrad
#                   maximum dropped the NaN that the reference's torch.maximum hands on -- the kernels and the oracle both
#   100005, 100057, 100117   native SH, means exactly at the camera: the NaN colour came out as 0 through fmaxf(c, 0)
#   100008 (in the first 48), 100204, 100396   get_all with K = 1: the row division by multiplication in ga_fwd_kernel needs
#                   2^32 / K + 1 in 32 bits, 0 for K = 1 -- every row of a wave gathered its coefficients from the first row's
#                   address on (wrong raw copies, reads up to 63 rows past that row)
REGRESSIONS = [100175, 100005, 100057, 100117, 100204, 100396]
LARGE = [100055, 100060, 100073, 100106, 100283]          # 220-280 k rows: fused / get_all at K = 15 degree 3, SH, Adam
LOG_STATES = [100064, 100148, 100272, 100304]             # get_all in training at (K, degree) = (15, 0), (15, 1), (8, 1), (15, 2)
SEEDS = [100000 + i for i in range(48)] + [s for s in REGRESSIONS + LARGE + LOG_STATES if s >= 100048]
BLOCK = 8
BLOCKS = (len(SEEDS) + BLOCK - 1) // BLOCK


def run_block(backend, block):
    import fuzz_step_ops as F
    results = [F.run_case(backend, seed) for seed in SEEDS[block * BLOCK:(block + 1) * BLOCK]]
    for key, worst in sorted(F.summarize(results).items()):
        print("%s block %d worst err/bound  %-40s %.3f" % (backend, block, key, worst))
    assert len(results) == len(SEEDS[block * BLOCK:(block + 1) * BLOCK])


@pytest.mark.gpu
@pytest.mark.parametrize("block", range(BLOCKS))
def test_random_step_cases_vs_restatement(oracle_mod, block):
    run_block("hip", block)


def test_the_fixed_seeds_cover_every_operation_and_edge():
    import fuzz_step_ops as F
    ds = [F.draw_case(s) for s in SEEDS]
    assert {d["op"] for d in ds} == set(F.OPS)
    assert {p for d in ds for p in d["plants"]} == set(F.PLANTS)
    assert {d["visible"] for d in ds if d["op"] in ("sparse_adam", "fused_step")} == {0.0, 0.5, 1.0}
    assert any(d["bad_index"] for d in ds) and any(d["n"] in F.SEAMS for d in ds) and any(d["n"] > 100000 for d in ds)
    assert {d["degree"] for d in ds} == {0, 1, 2, 3} and {d["sh_degree"] for d in ds if d["op"] == "native_sh"} == {0, 1, 2, 3}
    assert 1 in {d["K"] for d in ds if d["op"] == "get_all"}
    assert {d["K"] % 4 == 0 for d in ds if d["K"]} == {True, False}          # float4 and scalar paths of the row copy
    # the states LoG trains in: the active degree raised step by step under a fixed K
    trained = {(d["K"], d["degree"]) for d in ds if d["op"] == "get_all" and d["training"]}
    assert {(15, 0), (15, 1), (15, 2), (15, 3), (8, 1)} <= trained
