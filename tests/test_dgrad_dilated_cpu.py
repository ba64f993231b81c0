"""The cases of tests/test_dgrad_dilated_gpu.py reach the launch they are written for: the host-only query answers the
uniform-tap data-gradient instantiation without buffer loads and the split count of the table, in both arithmetics.  No GPU."""
import pytest

from tests import gemm_cases as G
from tests.test_dgrad_dilated_gpu import CASES, DEEP32, MODES, NAME, UNDILATED
from tests.test_dispatch_cpu import lib, query  # noqa: F401  (lib: the fixture that builds and resets the tuning)

MMA = {"bf16x3": 3, "f32": 0}


@pytest.mark.parametrize("mode", list(MODES))
def test_cases_pick_the_dilated_instantiation(lib, mode):  # noqa: F811
    try:
        for case, setup in [(c, None) for c in CASES] + [(UNDILATED, -200)] + ([(DEEP32, -32)] if mode in DEEP32[2] else []):
            assert lib.phnet_tune_reset() == 0 and lib.phnet_tune_mma(MMA[mode]) == 0
            assert setup is None or lib.phnet_tune_force_k_tile(setup) == 0
            shape, reason, picks = case
            k_tile, splits = picks[mode]
            assert query(lib, "dgrad", G.query_args(lib, "dgrad", shape)) == (NAME % (k_tile, MODES[mode]), splits), reason
    finally:
        assert lib.phnet_tune_reset() == 0


def test_split_counts_cover_one_two_and_four():
    assert {picks["bf16x3"][1] for _, _, picks in CASES} == {1, 2, 4}
    assert {picks["bf16x3"][0] for _, _, picks in CASES + [DEEP32]} == {16, 32, 64}
