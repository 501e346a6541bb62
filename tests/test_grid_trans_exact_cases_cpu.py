"""CPU checks behind tests/test_gpu_grid_trans_exact.py: the exactness bounds of trans_cases.rhs_t hold for every (case, nrhs, conj) the GPU file runs, the
exceptions are listed, and the chosen (case, grid) pairs reach every decision of the transposed grid sweeps that the file was written for -- recomputed from
the planner's exchange lists on the CPU test build of the library's host sources (the `emul` fixture: the planner is the product's, no sweep runs here)."""
import numpy as np
import pytest
import grid_trans_exact_cases as gx
import trans_cases as tc


def test_the_narrowed_cases_are_the_listed_ones():
    """no case of the set needs x in {-1, 0, 1}; the set keeps the three sweep cases and a double case with a supernode wider than 128 columns"""
    assert gx.NARROW == set()
    assert set(gx.SWEEP_CASES) == {"widths", "narrow", "z_narrow"} and set(gx.PANEL_CASES) == {"mixed_level", "z_chain"}
    wide = [name for name in gx.CASES if not gx.is_z(name) and max(gx.prepared(name)[0].widths) > 128]
    assert "widths" in wide, wide


@pytest.mark.parametrize("name", gx.CASES)
def test_bounds_of_the_transposed_sweeps_hold(name):
    """every (nrhs, conj) the GPU tests run on this case: both sweep bounds below 2^53 with the margin of 64 (rhs_t asserts; the margins are printed), x
    integer with pairwise different columns, T and C different systems on complex16"""
    c = gx.prepared(name)[0]
    todo = [(nrhs, conj) for n_, nrhs, conj in gx.runs() if n_ == name]
    assert {nrhs for nrhs, _ in todo} >= set(gx.NRHS)
    for nrhs, conj in todo:
        x, b = gx.rhs_t(name, nrhs, conj)
        assert x.shape == b.shape == (c.n, nrhs) and np.array_equal(x, np.rint(x.real) + (1j * np.rint(x.imag) if c.z else 0))
        assert np.unique(x, axis=1).shape[1] == nrhs
        fwd, bwd = tc.bounds_t(c, nrhs, conj, narrow=name in gx.NARROW)
        assert 0 < fwd < tc.LIMIT and 0 < bwd < tc.LIMIT
        print(f"{name} nrhs {nrhs} {'C' if conj else 'T'}: forward bound 2^{np.log2(fwd):.1f}, backward bound 2^{np.log2(bwd):.1f} of 2^53 (margin 64 inside)")
    if c.z:
        assert not np.array_equal(gx.rhs_t(name, 5, False)[1], gx.rhs_t(name, 5, True)[1])


def test_the_chunk_runs_exceed_one_chunk():
    for name, grid, nrhs in gx.CHUNK_RUNS:
        c = gx.prepared(name)[0]
        assert nrhs == tc.max_rhs_chunk(max(c.widths), z=c.z) + 1, (name, nrhs)
    assert gx.CHUNK_RUNS[0][2] == 49


@pytest.fixture(scope="module")
def planned():
    return {}


def _plans(planned, name, grid):
    if (name, grid) not in planned:
        planned[(name, grid)] = gx.plans(name, grid)
    return planned[(name, grid)]


@pytest.mark.parametrize("grid", gx.GRIDS, ids=lambda g: "%dx%dx%d" % g)
@pytest.mark.parametrize("name", gx.CASES)
def test_the_plan_of_a_pair_is_the_same_on_two_calls(emul, planned, name, grid):
    first, tree = _plans(planned, name, grid)
    again, tree2 = gx.plans(name, grid)
    assert len(first) == len(again) == grid[0] * grid[1] * grid[2] and np.array_equal(tree, tree2)
    for rank, (a, b) in enumerate(zip(first, again)):
        for w in gx.XT_LISTS:
            assert np.array_equal(a[w], b[w]), (name, grid, rank, w)


def test_the_pairs_cover_every_decision(emul, planned):
    """the coverage table (printed), every tag from the pair that was chosen to supply it, and the union over all pairs"""
    seen = set()
    for name in gx.CASES:
        for grid in gx.GRIDS:
            cov = gx.coverage(name, grid, _plans(planned, name, grid))
            assert cov <= set(gx.TAGS)
            print("%-12s %dx%dx%d  " % ((name,) + grid) + " ".join("x" if t in cov else "." for t in gx.TAGS))
            seen |= cov
    print("columns: " + " | ".join(gx.TAGS))
    for tag, (name, grid) in gx.SUPPLIERS.items():
        assert tag in gx.coverage(name, grid, _plans(planned, name, grid)), f"{tag!r} was to come from {name} on {grid}"
    assert seen == set(gx.TAGS), set(gx.TAGS) - seen
    assert set(gx.SUPPLIERS) == set(gx.TAGS)
