"""CPU only: the planting of tests/test_gpu_record_step_pairs.py that tests/test_gpu_record_step_packed.py does not have - population
k = 1, c = (0, -1, -1), the cx = 0 direction of the (cy, cz) its cx = -1 and cx = +1 plantings share. What the oracle alone leaves out
of that comparison (tests/_edge_states.py nonfinite_pull_cells) is no cell for NaN and the first step's one puller for +Inf, at every
placement, and the value does spread: the same check test_nonfinite_cases_leave_out_one_cell_at_most makes for k = 0, 26 and 10."""
import numpy as np
import pytest

import _record_pairs_cases as rp


@pytest.mark.parametrize("place", list(rp.NF_PLACE))
@pytest.mark.parametrize("kind", list(rp.NF_KIND))
def test_the_cx0_planting_leaves_out_one_cell_at_most(kind, place):
    want, allowed = rp.oracle_with_allowed(kind, "cx0", place, check_nan=True)
    assert int(allowed.sum()) == (0 if kind == "nan" else 1)
    assert np.isnan(want["rho"]).sum() >= 27, "after two steps the 27 cells around the puller have met the value"
    assert np.isfinite(want["rho"]).sum() >= want["rho"].size - 125
