"""superlu_dist_amd.autograd on the device: the integer systems of tests/adjoint_cases.py end to end and bitwise (factorisation, forward solve, adjoint solve,
values kernel), torch.autograd.gradcheck on the general matrices that tests/test_adjoint_cases_cpu.py vets, and the bookkeeping of the resident factors.
The bodies are in tests/autograd_gpu_cases.py and run in ONE child process that imports torch first (torch.cuda reports no device once the library has
initialised the HIP runtime in a process: tests/test_gpu_update_values.py); every case is asserted on its own here."""
import json, os, subprocess, sys
import pytest
import adjoint_cases as ac

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def results():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "autograd_gpu_cases.py"), ROOT], capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and lines, r.stdout[-1500:] + r.stderr[-1500:]
    return json.loads(lines[-1][7:])


@pytest.mark.parametrize("case", ac.autograd_case_ids())
def test_autograd_case(results, case):
    assert results.get(case) == "ok", results.get(case, "the child process did not run this case")
