"""The launch sequence of the link sweeps of a one-rank double handle, pinned by a recorded fixture.  tests/golden/link_launches.json holds, for every solve
below, the `[sluamd sweep] family=... build=... units=... mx=... nrhs=... rk=...` lines that SLUAMD_SOLVE_DEBUG makes the launch wrappers print, in the
order of the launches, and stats()["solve_launches"]; tests/golden/make_link_launches.py recorded them on the device at the commit BEFORE the forward and
the backward link drivers were each written once.  The test replays the same solves and requires the same lines and counts, line for line: the drivers of
sluamd_factor.cpp may be rearranged, what they queue may not change.

Cases: `levels` of sweep_cases.py (levels of 66, 1, 33, 4, 2 and 1 supernodes: joined and two-launch links meet in both orders) and `one_level` (three
independent supernodes, built by the same SweepCase: the last level is also the first).  Each with 1, 3, 4 and 16 right-hand sides (joined units; blocks
of four, which keep every level on two launches; the MFMA form) under the defaults, SLUAMD_SOLVE_JOIN=0 (no joined tables), SLUAMD_JOIN_MAX_NODES=1 (of
the values test_gpu_sweep_shapes.py runs on `levels`, the one whose joined levels differ from the defaults': only the two single-supernode levels join),
SLUAMD_SOLVE_GROUPS=1 and a handle created with options.deterministic (the serial links).  One child process per setting: the switches are read when the
library is loaded.  The values are checked too (the integer x, numpy.array_equal), at no cost; test_gpu_sweep_shapes.py owns that property."""
import functools, json, os, subprocess, sys
import numpy as np
import pytest
import sweep_cases as sw
from superlu_dist_amd import driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "link_launches.json")
NRHS = (1, 3, 4, 16)
CONFIGS = {"default": {}, "join0": {"SLUAMD_SOLVE_JOIN": "0"}, "join_max_1": {"SLUAMD_JOIN_MAX_NODES": "1"}, "groups": {"SLUAMD_SOLVE_GROUPS": "1"},
           "deterministic": {}}


def one_level():
    """three supernodes of 40, 100 and 65 columns with no block between them: a forest of three roots, ONE level (narrow and wide diagonal units in it)"""
    return sw.SweepCase("one_level", "a single level: the last level is the first", [40, 100, 65], {}, {})


CASES = {"levels": sw.CASES["levels"], "one_level": one_level}


def _factored(name, deterministic):
    """a handle holding the exact factors of the case (asserted), and the case with its exact images filled in"""
    c = CASES[name]()
    n, rp, ci = c.pattern_csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    assert np.array_equal(symb.perm_c, np.arange(n)) and symb.xsup().tolist() == c.xsup.tolist(), symb.xsup().tolist()
    fs = symb.flat_store(values=False)
    symb.free()
    expL, expU = c.fill(fs)
    h = driver.LUHandle.from_store(fs, deterministic=deterministic)
    assert h.pdgstrf3d(0.0) == 0
    h.copy_to_host()
    assert np.array_equal(fs.Lnzval, expL) and np.array_equal(fs.Unzval, expU), name
    return h, c


def child_main(deterministic):
    """runs in the child process: every case and nrhs on one handle per case; a `[case]` line on stderr ahead of each solve's launch lines"""
    out = {}
    for name in CASES:
        h, c = _factored(name, deterministic)
        for nrhs in NRHS:
            x, b = c.rhs(nrhs)
            sys.stderr.write("[case] %s:%d\n" % (name, nrhs)); sys.stderr.flush()
            got = h.pdgstrs3d(b.copy(order="F"))
            out["%s:%d" % (name, nrhs)] = {"exact": bool(np.array_equal(got, x)), "solve_launches": int(h.stats()["solve_launches"])}
        h.destroy()
    print("RESULT " + json.dumps(out))


CHILD = ("import os, sys\nsys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests'))\n"
         "import test_gpu_link_launches as t\nt.child_main(sys.argv[2] == '1')\n")


@functools.lru_cache(maxsize=None)
def record(cfg):
    """{"case:nrhs": {"lines": [...], "solve_launches": n}} of one setting; run once, never retried"""
    env = dict(os.environ, SLUAMD_SOLVE_DEBUG="1", **CONFIGS[cfg])
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, "1" if cfg == "deterministic" else "0"], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert len(res) == len(CASES) * len(NRHS) and all(v["exact"] for v in res.values()), sorted(k for k, v in res.items() if not v["exact"])
    key, out = None, {k: {"lines": [], "solve_launches": v["solve_launches"]} for k, v in res.items()}
    for ln in r.stderr.splitlines():
        if ln.startswith("[case] "):
            key = ln.split()[1]
        elif ln.startswith("[sluamd sweep] ") and key is not None:      # (before the first solve: the sweeps of the inverses' set-up, if any, are not links)
            out[key]["lines"].append(ln.strip())
    return out


@functools.lru_cache(maxsize=None)
def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_every_solve_and_both_forms():
    """the recorded runs themselves (a launch of no unit prints no line): every setting, case and nrhs is there; at the defaults `levels` queues joined
    launches beside two-launch links (sweep_join, sweep_step and bwd_update lines) below four right-hand sides and no joined launch from four on; with
    SLUAMD_SOLVE_JOIN=0 none at all; SLUAMD_JOIN_MAX_NODES=1 changes the sequence below four right-hand sides; the serial links queue one update unit per
    launch, so every counted launch has its line; `one_level` has nothing to update: its diagonal units, once per sweep"""
    fx = _fixture()
    assert sorted(fx) == sorted(CONFIGS)
    for cfg in CONFIGS:
        assert sorted(fx[cfg]) == sorted("%s:%d" % (name, nrhs) for name in CASES for nrhs in NRHS), cfg
    fields = lambda cfg, key: [dict(tok.split("=") for tok in ln.split()[2:]) for ln in fx[cfg][key]["lines"]]
    for nrhs in NRHS:
        key = "levels:%d" % nrhs
        fam = [f["family"] for f in fields("default", key)]
        assert ("sweep_join" in fam) == (nrhs < 4) and "sweep_step" in fam and "bwd_update" in fam, (nrhs, fam)
        assert all(f["family"] != "sweep_join" for f in fields("join0", key))
        assert (fx["join_max_1"][key]["lines"] != fx["default"][key]["lines"]) == (nrhs < 4)
        det = fields("deterministic", key)
        assert len(det) == fx["deterministic"][key]["solve_launches"] and all(f["units"] == "1" for f in det if f["family"] != "sweep_step")
        for cfg in CONFIGS:
            assert all(int(f["nrhs"]) == nrhs for f in fields(cfg, key))
            one = [f["family"] for f in fields(cfg, "one_level:%d" % nrhs)]
            assert len(one) == 2 and set(one) <= {"sweep_step", "sweep_join"}, (cfg, nrhs, one)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_link_launches_are_the_recorded_ones(cfg):
    """the launch lines of every solve of the setting, in order, and its solve_launches equal the recorded ones"""
    got, want = record(cfg), _fixture()[cfg]
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key]["solve_launches"] == want[key]["solve_launches"], (cfg, key, got[key]["solve_launches"], want[key]["solve_launches"])
        g, w = got[key]["lines"], want[key]["lines"]
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        assert g == w, (cfg, key, "launches", len(g), len(w), "first difference at", first, g[first:first + 2], w[first:first + 2])
