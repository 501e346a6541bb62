"""The program of the factorisation driver, pinned (CPU): the emulated runtime and the CPU engine keep, per thread, one line per call in the
order the HOST issued it -- event records and waits, asynchronous memsets, grouped exchanges with peers and lengths, every eng:: launch with the
scalars that decide it and eng::panel_site as the driver left it (oracle/emul/emul_rt.cpp, engine_cpu.cpp, comm_norccl.cpp).  Streams and events
carry the names of their first appearance, so the traces of two builds compare as text.  tests/golden/factor_trace.json holds, per configuration
of factor_trace_cases.CASES and rank, the line count, a sha256 of the trace, the launch counters of sluamd_get_stats and the first 40 lines.

The golden file was recorded ONCE, with the driver as it stood before run_factor_sched was split into FactorRun / factor_serial /
factor_lookahead, and is not regenerated: a trace that differs is a change of the driver's program, to be fixed in the driver.
(`python tests/test_factor_trace_cpu.py --record` writes the file; that is for a deliberate change of the program only.)"""
import hashlib
import json
import os
import re
import sys
import pytest

HEAD = 40
_runs = {}


def _ranks(name):
    """the traced ranks of a case, run once per session (the emulation library must be bound: `emul` fixture)"""
    import factor_trace_cases as ftc
    if name not in _runs:
        ranks, res = ftc.run(name, trace=True)
        assert res <= 1e-12, (name, res)
        _runs[name] = ranks
    return _runs[name]


def _record_of(rank):
    lines = rank["trace"].splitlines()
    return dict(lines=len(lines), sha256=hashlib.sha256(rank["trace"].encode()).hexdigest(), **rank["stats"], head=lines[:HEAD])


if __name__ == "__main__":      # run as a script (--record): no conftest has set the path
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [_here, os.path.dirname(_here)]


def _case_names():
    import factor_trace_cases as ftc
    return list(ftc.CASES)


@pytest.fixture(scope="module")
def golden_traces():
    import factor_trace_cases as ftc
    with open(ftc.GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", _case_names())
def test_issue_order_is_the_recorded_one(emul, golden_traces, tmp_path, name):
    ranks = _ranks(name)
    want = golden_traces[name]
    assert len(ranks) == len(want)
    for r, (rank, w) in enumerate(zip(ranks, want)):
        got = _record_of(rank)
        if got != w:
            path = tmp_path / f"{name}.rank{r}.trace"
            path.write_text(rank["trace"])
            first = next((i for i, (a, b) in enumerate(zip(got["head"], w["head"])) if a != b), None)
            where = f"first differing line {first}: got {got['head'][first]!r}, recorded {w['head'][first]!r}" if first is not None else f"the first {HEAD} lines agree"
            counters = {k: (got[k], w[k]) for k in got if k not in ("head", "sha256") and got[k] != w[k]}
            pytest.fail(f"{name} rank {r}: the driver issues a different program than the recorded one ({where}; (got, recorded) {counters}); whole trace in {path}")


# ---- the paths the configurations were chosen for: each must occur in some trace, or a configuration no longer reaches its path ----
def _split_level(t):        # a split level: panel solves of part 0 and of part 1
    return re.search(r"^panel_\w+ .*site=\d+,\d+,0,0 ", t, re.M) and re.search(r"^panel_\w+ .*site=\d+,\d+,1,0 ", t, re.M)


def _deferred_inv(t):       # tail level: the full inverses beside the chain
    return re.search(r"^full_inv .*site=\d+,\d+,-1,1 ", t, re.M)


def _ksplit(t):
    return re.search(r"^schur .* ksplit=([2-9]|\d\d) ", t, re.M)


def _balanced_bulk(t):      # a launch over the XCD ranges of LevelSched::x_off
    return re.search(r"^schur .* xoff=1 ", t, re.M)


def _group_inverse(t):
    return re.search(r"^grp_gather ", t, re.M)


def _fused_serial_level(t):
    """serial program (one stream), a K-fused level: its part-0 and part-1 tiles are launched apart, so one tile configuration is launched
    at least three times between two diagonal factorisations (a balanced level launches it twice, any other once)"""
    if len(set(re.findall(r"^(?:schur|diag_lu|panel_\w+) .*@(s\d+)$", t, re.M))) != 1:
        return False
    for level in re.split(r"^diag_lu .*$", t, flags=re.M):
        # update launches from the lists: not the build of the tile records (mmode=1, in front of the first level), not the deterministic mode's launches per supernode
        cfgs = re.findall(r"^schur cfg=(\d+) .* mmode=[02] .* nodes=0 ", level, re.M)
        if any(cfgs.count(c) >= 3 for c in set(cfgs)):
            return True
    return False


def _reduction_chunk_wait(t):
    """pipelined Z reduction: a stream waits for the event recorded right behind one chunk's additions"""
    lines = t.splitlines()
    chunk_events = {lines[i + 1].split()[1] for i in range(len(lines) - 1) if lines[i].startswith("add_atomic ") and lines[i + 1].startswith("hipEventRecord ")}
    return any(ln.startswith("hipStreamWaitEvent ") and ln.split()[1] in chunk_events for ln in lines)


PATHS = {"split level": _split_level, "deferred full_inv": _deferred_inv, "ksplit > 1": _ksplit, "balanced bulk launch": _balanced_bulk,
         "K-fused serial level": _fused_serial_level, "group inverse": _group_inverse, "wait on a reduction chunk event": _reduction_chunk_wait}


def test_traces_reach_the_paths_they_were_chosen_for(emul):
    traces = {f"{name}[{r}]": rank["trace"] for name in _case_names() for r, rank in enumerate(_ranks(name))}
    reached = {what: [k for k, t in traces.items() if found(t)] for what, found in PATHS.items()}
    print(json.dumps(reached, indent=1))
    missing = [what for what, where in reached.items() if not where]
    assert not missing, f"no configuration reaches: {missing}"
    # complex16, an XY exchange and the tile-record build are on record too
    assert any(re.search(r"^zschur ", t, re.M) for t in traces.values()) and any(re.search(r"^exchange .*(send|recv)", t, re.M) for t in traces.values())
    assert any(re.search(r"^schur .* mmode=1 ", t, re.M) for t in traces.values()) and any(re.search(r"^schur .* mmode=2 ", t, re.M) for t in traces.values())


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], __doc__
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from superlu_dist_amd import _lib
    _lib._lib = _lib.bind(ctypes.CDLL(os.path.join(root, "oracle", "libsluamd_emul.so")))
    out = {name: [_record_of(rank) for rank in _ranks(name)] for name in _case_names()}
    for what, found in PATHS.items():
        print(what, [name for name in out for rank in _ranks(name) if found(rank["trace"])])
    import factor_trace_cases as ftc
    with open(ftc.GOLDEN_FILE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
