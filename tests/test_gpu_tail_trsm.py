"""The 64-high blocked substitution of the tail levels -- the strip in registers (k_panel_tsub, the default) and in LDS (k_panel_trsm<64> under
SLUAMD_TRSM_LDS_STRIP=1) -- against EXACT factors and solutions: tests/tail_trsm_cases.py builds one chain of single-supernode tail levels per supernode
width (256, 255, 200, 129, 96, 64, 33: the three register builds, odd widths, ragged last blocks), with panels of fewer than 16 rows and of 64 + 16 + 5,
skyline columns with the leads 0, 1, 31, 32 and width - 1; every case runs split (urgent and remaining lists) and whole (prefix form), under the look-ahead
and the serial schedule, with either kernel.  Every comparison of values is numpy.array_equal; the `[sluamd panel]` lines of SLUAMD_FACTOR_DEBUG prove that
the tail levels ran the substitution form, the `[sluamd trsm64]` lines which kernel ran it.  The raw factors of the two kernels on random (non-integer)
values are compared with array_equal too: the register kernel keeps the summation order of the LDS one."""
import functools, json, os, subprocess, sys
import numpy as np
import pytest
import panel_cases as pn
import pivot_cases as pc
import schur_cases as sc
import sweep_cases as sw
import tail_trsm_cases as tt
from superlu_dist_amd import driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = "emul" in os.path.basename(os.environ.get("SLUAMD_LIB", ""))
NRHS = (1, 3)
SWITCHES = ("SLUAMD_PANEL_SPLIT", "SLUAMD_NO_LOOKAHEAD", "SLUAMD_TRSM_LDS_STRIP")


@functools.lru_cache(maxsize=None)
def _prepared(w):
    """(case, flat store holding B, expected Lnzval, expected Unzval, sources, DAG levels): built once per width, shared and never written"""
    c = tt.CASES[w]()
    n, rp, ci = c.pattern_csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    assert np.array_equal(symb.perm_c, np.arange(n))
    assert symb.xsup().tolist() == c.xsup.tolist(), symb.xsup().tolist()
    fs = symb.flat_store(values=False)
    symb.free()
    expL, expU = c.fill(fs)
    srcs = sc.sources(fs)
    return c, fs, expL, expU, srcs, sw.levels_of(srcs)


def _copy(fs):
    return driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind.copy(), fs.Lnzval_off, fs.Lnzval.copy(), fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off,
                            fs.Unzval.copy())


def _run_exact(w, tag, mark=None):
    """one handle under the environment as it stands: the factors at every stored position, the integer x for 1 and 3 right-hand sides"""
    c, fs0, expL, expU = _prepared(w)[:4]
    fs = _copy(fs0)
    h = driver.LUHandle.from_store(fs)
    if mark:
        mark("factor")
    assert h.pdgstrf3d(0.0) == 0, (w, tag)
    h.copy_to_host(fs)
    if mark:
        mark("solve")
    for which, got, exp in (("L", fs.Lnzval, expL), ("U", fs.Unzval, expU)):
        assert np.array_equal(got, exp), (w, tag, which, int(np.count_nonzero(got != exp)), int(np.flatnonzero(got != exp)[0]))
    for nrhs in NRHS:
        x, b = c.rhs(nrhs)
        got = h.pdgstrs3d(b.copy(order="F"))
        assert np.array_equal(got, x), (w, tag, nrhs, int(np.count_nonzero(got != x)))
    h.destroy()


def _set_env(env):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)


@pytest.mark.parametrize("w", tt.WIDTHS)
def test_every_form_is_exact(w, monkeypatch):
    """split / whole / serial x registers / LDS: L0 and U0 at every stored position and the integer x, all six"""
    for form, (env, _) in tt.FORMS.items():
        for impl, ienv in tt.IMPLS.items():
            for k in SWITCHES:
                monkeypatch.delenv(k, raising=False)
            for k, v in dict(env, **ienv).items():
                monkeypatch.setenv(k, v)
            _run_exact(w, form + "/" + impl)


# ---------------------------------------------------------------------------------------------------------------------------------------
# The launch lines: SLUAMD_FACTOR_DEBUG is read when the library is loaded -- one child process runs every width, form and kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_gpu_tail_trsm as t
print("RESULT " + json.dumps(t.child_body()))
"""


def child_body():
    out = {}
    for w in tt.WIDTHS:
        for form, (env, _) in tt.FORMS.items():
            for impl, ienv in tt.IMPLS.items():
                _set_env(dict(env, **ienv))
                key = "%d:%s:%s" % (w, form, impl)

                def mark(phase):
                    sys.stderr.write("[case] %s %s\n" % (key, phase)); sys.stderr.flush()
                try:
                    _run_exact(w, key, mark=mark)
                    out[key] = True
                except AssertionError as e:
                    out[key] = repr(e)[:300]
    _set_env({})
    return out


@functools.lru_cache(maxsize=None)
def _child():
    """run once, never retried"""
    env = dict(os.environ, SLUAMD_FACTOR_DEBUG="1")
    for k in SWITCHES:
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    return r.returncode, r.stdout, r.stderr


def test_exact_under_the_launch_lines():
    rc, out, err = _child()
    assert rc == 0, out[-1500:] + err[-1500:]
    res = json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == len(tt.WIDTHS) * len(tt.FORMS) * len(tt.IMPLS) and all(v is True for v in res.values()), {k: v for k, v in res.items() if v is not True}


def test_the_tail_levels_ran_and_the_kernel_is_the_chosen_one():
    """per width, form and kernel: the `[sluamd panel]` lines ARE those of the restated rules -- every panel solve of the three tail levels the 64-high
    substitution (trsm64), a's level as two lists under the look-ahead schedule, whole elsewhere -- the same lines whichever kernel runs; each of them is
    followed by one `[sluamd trsm64]` line naming the kernel the switch selects, with the same level and unit counts; the solves launch nothing of the chain"""
    if EMUL:
        pytest.skip("the emulation engine has no forms")
    rc, out, err = _child()
    assert rc == 0, out[-1500:] + err[-1500:]
    key, per, impl_lines = None, {}, {}
    for ln in err.splitlines():
        if ln.startswith("[case] "):
            _, k, phase = ln.split()
            key = (k, phase)
            per[key], impl_lines[key] = [], []
        elif key and ln.startswith("[sluamd panel] "):
            per[key] += pn.parse_lines(ln)
        elif key and ln.startswith("[sluamd trsm64] "):
            f = dict(tok.split("=") for tok in ln.split()[2:])
            impl_lines[key].append((f["impl"], int(f["level"]), int(f["mx"]), int(f["nl"]), int(f["nu"])))
    for w in tt.WIDTHS:
        srcs, lev = _prepared(w)[4:]
        for form, (_, st) in tt.FORMS.items():
            want = pn.predicted_lines(srcs, lev, False, dict(pn.DEFAULTS, **st))
            panels = [x for x in want if x[0] == "panel"]
            assert len(panels) == (4 if form == "split" else 3) and all(x[1] == "trsm64" for x in panels)
            for impl in tt.IMPLS:
                k = "%d:%s:%s" % (w, form, impl)
                assert sorted(per[(k, "factor")]) == want, (k, per[(k, "factor")])
                assert sorted(impl_lines[(k, "factor")]) == sorted((impl, x[2], x[4], x[5], x[6]) for x in panels), (k, impl_lines[(k, "factor")])
                assert per[(k, "solve")] == [] and impl_lines[(k, "solve")] == [], k


# ---------------------------------------------------------------------------------------------------------------------------------------
# Random values: the raw factors of the two kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
def _random_store(w):
    """the structure of the case filled with non-integer random values in (-1, 1), the diagonal raised to n: no small pivot"""
    fs0 = _prepared(w)[1]
    (lr, lc), _ = pc.store_positions(fs0)
    rng = np.random.default_rng(20 + w)
    fs = _copy(fs0)
    fs.Lnzval[:] = rng.uniform(-1.0, 1.0, fs.Lnzval.shape)
    fs.Unzval[:] = rng.uniform(-1.0, 1.0, fs.Unzval.shape)
    fs.Lnzval[(lr >= 0) & (lr == lc)] += fs.n
    return fs


@pytest.mark.parametrize("sched", ["lookahead", "serial"])
@pytest.mark.parametrize("w", [256, 200])
def test_raw_factors_of_the_two_kernels_are_equal(w, sched, monkeypatch):
    """non-integer values: every stored value of L and U after the factorisation with the register kernel equals the one with the LDS kernel, bit for bit
    (the same products in the same order: t ascending, k ascending, the subtraction, the product with the 32 x 32 inverse)"""
    if EMUL:
        pytest.skip("the emulation engine has one substitution")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if sched == "serial":
        monkeypatch.setenv("SLUAMD_NO_LOOKAHEAD", "1")
    got = {}
    for impl, ienv in tt.IMPLS.items():
        for k, v in ienv.items():
            monkeypatch.setenv(k, v)
        fs = _random_store(w)
        h = driver.LUHandle.from_store(fs)
        assert h.pdgstrf3d(0.0) == 0
        h.copy_to_host(fs)
        h.destroy()
        got[impl] = (fs.Lnzval.copy(), fs.Unzval.copy())
        assert np.all(np.isfinite(got[impl][0])) and np.all(np.isfinite(got[impl][1]))
    for which, a, b in (("L", got["regs"][0], got["lds"][0]), ("U", got["regs"][1], got["lds"][1])):
        d = np.abs(a - b) / np.maximum(np.abs(b), np.finfo(float).tiny)
        print("width %d %s %s: %d of %d values differ, largest relative difference %.3e" % (w, sched, which, int(np.count_nonzero(a != b)), a.size, float(d.max())))
        assert np.array_equal(a, b), (w, sched, which, int(np.count_nonzero(a != b)), float(d.max()))
