"""The device build issues what the emulation issued: for the single-rank configurations of tests/golden/factor_trace.json (factor_trace_cases.CASES;
recorded through the CPU emulation, test_factor_trace_cpu.py) the host code of the GPU library takes the same decisions, so the launch counters of
sluamd_get_stats after the factorisation equal the recorded ones -- and the solution meets the residual bound of test_stream_order.py.
No single-rank configuration is left out: none of them depends on the device's memory (the tile records of these sizes always fit)."""
import json
import pytest
import factor_trace_cases as ftc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(ftc.GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", ftc.SINGLE_RANK)
def test_launch_counters_equal_the_recorded_ones(recorded, name):
    (rank,), res = ftc.run(name)
    want = {k: recorded[name][0][k] for k in ftc.COUNTERS}
    print(name, rank["stats"], want, res)
    assert rank["stats"] == want
    assert res <= 1e-12
