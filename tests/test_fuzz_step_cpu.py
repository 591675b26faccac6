"""The seeds of tests/test_gpu_fuzz_step.py through tests/oracle_backend.OracleBackend in place of the kernels (the fused step
composed from its two halves): a correct fp32 implementation stays inside the sweep's bound, so a kernel that leaves it is
wrong and not unlucky.  Has to pass before the same seeds mean anything on the device."""
import pytest

from test_gpu_fuzz_step import BLOCKS, run_block


@pytest.mark.parametrize("block", range(BLOCKS))
def test_random_step_cases_through_the_oracle_backend(oracle_mod, block):
    run_block("oracle", block)
