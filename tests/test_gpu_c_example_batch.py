"""examples/pddrive3d_amd N --batch K: the batch interface used from plain C -- K Poisson operators with shifted diagonals as one batch, info and the maximum
residual per matrix."""
import os, re, subprocess
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "examples", "pddrive3d_amd")


def test_c_driver_batch():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "examples")], stdout=subprocess.DEVNULL)
    r = subprocess.run([EXE, "8", "--batch", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    rows = re.findall(r"BATCH matrix (\d+): info (\d+)  max residual ([0-9.e+-]+)", r.stdout)
    assert [int(k) for k, _, _ in rows] == list(range(5))
    assert all(int(i) == 0 and float(res) < 1e-12 for _, i, res in rows), rows
    assert re.search(r"BATCH 5 matrices of order 512:", r.stdout)
