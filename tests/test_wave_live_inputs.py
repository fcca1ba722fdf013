"""lbm_set_obstacles and lbm_write_state where lbm_wave runs: every entry of KERNELS on both SHAPES of
tests/test_wave_fields.py with wave_rows 24 (chunk edges at rows 24 and 48), through the yardstick of
tests/test_live_inputs.py -- a live context against a fresh one, every output and lattice bit for bit.

What these cases add to that file's: lbm_wave's force, probe and force-and-probe maps are obstacle bytes with marks on
them, so they must be rebuilt from the new map; a stale map shows as different bits in the runs that ride in the launches
(forces_in_wave, probes_in_wave, window_in_wave, driven_observed_in_wave and wave_launches are asserted per call)."""
import pytest

from test_live_inputs import WAVE_CASES, check_case

CASES = list(WAVE_CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("path,inp", CASES)
def test_a_live_context_is_the_fresh_context_in_lbm_wave(gpu, path, inp):
    check_case(gpu, path, inp)
