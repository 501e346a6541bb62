"""The Schur update (k_schur) against EXACT factors, over the decisions its loader takes at run time: tile configuration, K of the source,
U leads inside a tile, ragged and merged tiles, K-fused predecessors with absent rows, split-K chain tiles, per-tile records, the last slot
of the arena, the complex16 embedding.  tests/schur_cases.py builds B = L0 U0 from small integers on designed block patterns, so that every
intermediate of any summation order is an exact double: pdgstrf3d must return L0 and U0 at every stored position, and the solve the integer
x it was built from.  No tolerance appears in this file: every comparison is numpy.array_equal (the rule for the sign of a stored zero is in
schur_cases.py).  test_the_cases_cover_every_loader_decision recomputes from the exported structure what each case is for."""
import functools
import numpy as np
import pytest
import oracle as orc
import pivot_cases as pc
import schur_cases as sc
import grid_cases
from superlu_dist_amd import driver, grid3d

pytestmark = pytest.mark.gpu

@functools.lru_cache(maxsize=None)
def _prepared(name):
    """(case, flat store holding B, expected Lnzval, expected Unzval, sources): built once per case"""
    c = sc.CASES[name]()
    n, rp, ci = c.pattern_csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    assert np.array_equal(symb.perm_c, np.arange(n))                 # the construction order is the factored order
    assert symb.xsup().tolist() == c.xsup.tolist(), symb.xsup().tolist()      # ... and the designed supernodes are the library's
    fs = symb.flat_store(values=False)
    symb.free()
    expL, expU = c.fill(fs)
    return c, fs, expL, expU, sc.sources(fs)


def _copy(fs):
    return driver.FlatStore(fs.n, fs.xsup, fs.Lrowind_off, fs.Lrowind.copy(), fs.Lnzval_off, fs.Lnzval.copy(), fs.Ufstnz_off, fs.Ufstnz, fs.Unzval_off,
                            fs.Unzval.copy())


def _where(fs, which, idx):
    (lr, lc), (ur, uc) = pc.store_positions(fs)
    r, c = (lr, lc) if which == "L" else (ur, uc)
    sn = np.searchsorted(fs.xsup, [r[idx], c[idx]], side="right") - 1
    return dict(part=which, row=int(r[idx]), col=int(c[idx]), supernode_of_row=int(sn[0]), supernode_of_col=int(sn[1]))


def _assert_exact(fs, expL, expU, what):
    for which, got, exp in (("L", fs.Lnzval, expL), ("U", fs.Unzval, expU)):
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(~(got == exp))
            raise AssertionError((what, len(bad), _where(fs, which, bad[0]), got[bad[0]], exp[bad[0]]))


def _factor(name, shuffle=None, **opts):
    """B of case `name` through the view path: info == 0 and every stored value of L and U equal to L0 / U0.  Returns (handle, store)."""
    c, fs0, expL, expU, _ = _prepared(name)
    fs = _copy(fs0)
    if shuffle is not None:                                         # rows inside every L block permuted, index entries and values alike
        ref = _copy(fs0); ref.Lnzval[:] = expL
        grid_cases.shuffle_block_rows(fs, shuffle); grid_cases.shuffle_block_rows(ref, shuffle)
        expL = ref.Lnzval
        fs._build_view()
    h = driver.LUHandle.from_store(fs, **opts)
    assert (h.pzgstrf3d if c.z else h.pdgstrf3d)(0.0) == 0
    h.copy_to_host()
    _assert_exact(fs, expL, expU, name)
    return h, fs


def _solve_exact(name, h):
    c = _prepared(name)[0]
    for nrhs in (1, 3):
        x, b = c.rhs(nrhs)
        got = h.pdgstrs3d(b.copy(order="F"))
        assert np.array_equal(got, x), (name, nrhs, int(np.count_nonzero(got != x)))


@pytest.mark.parametrize("name", list(sc.CASES))
def test_factors_and_solution_are_exact(name):
    """every case at the defaults: L and U equal L0 and U0 at every stored position, the CPU oracle's factorisation of the same store gives the same
    values, and the solves with 1 and 3 right-hand sides return the integer x bitwise (the sweeps only add integer products and scale by powers
    of two; Case.rhs asserts the 2^53 bound for b and for the intermediate y = U0 x)"""
    c, fs0, expL, expU, _ = _prepared(name)
    o = orc.LUStore(fs0.n, fs0.xsup, fs0.Lrowind_off, fs0.Lrowind, fs0.Lnzval_off, fs0.Lnzval.copy(), fs0.Ufstnz_off, fs0.Ufstnz, fs0.Unzval_off,
                    fs0.Unzval.copy())
    info_o = orc.dfactor(o)[0]
    assert info_o == 0
    assert np.array_equal(o.Lnzval, expL) and np.array_equal(o.Unzval, expU)      # the oracle is exact on these inputs
    h, fs = _factor(name)
    assert np.array_equal(fs.Lnzval, o.Lnzval) and np.array_equal(fs.Unzval, o.Unzval)
    _solve_exact(name, h)
    h.destroy()


VARIANTS = [
    ("k_big", {"SLUAMD_NO_BIG_TILES": "1"}, {}), ("k_big", {"SLUAMD_SCHUR_4WAVES": "1"}, {}), ("k_big", {"SLUAMD_NO_TILE_MAPS": "1"}, {}),
    ("leads_big", {"SLUAMD_NO_BIG_TILES": "1"}, {}), ("leads_big", {"SLUAMD_SCHUR_4WAVES": "1"}, {}), ("leads_big", {"SLUAMD_NO_TILE_MAPS": "1"}, {}),
    ("leads_big", {}, {"deterministic": True}), ("leads_small", {"SLUAMD_NO_TILE_MAPS": "1"}, {}),
    ("rows_and_merges", {"SLUAMD_NO_MERGE_TILES": "1"}, {}), ("rows_and_merges", {}, {"deterministic": True}),
    ("fuse_clean", {"SLUAMD_NO_FUSE": "1"}, {}), ("fuse_absent", {"SLUAMD_NO_FUSE": "1"}, {}), ("fuse_absent", {}, {"deterministic": True}),
    ("fuse_absent", {"SLUAMD_NO_TILE_MAPS": "1"}, {}), ("fuse_three", {"SLUAMD_FUSE_MAX_PREV": "3", "SLUAMD_FUSE_GROUP_MIN_NODES": "1"}, {}),
    ("fuse_three", {"SLUAMD_NO_FUSE": "1"}, {}), ("chain_top", {"SLUAMD_KSPLIT": "4"}, {}), ("chain_top", {"SLUAMD_KSPLIT": "1"}, {}),
    ("last_slot", {"SLUAMD_NO_TILE_MAPS": "1"}, {}),
]


@pytest.mark.parametrize("name,env,opts", VARIANTS, ids=[f"{n}-{'-'.join(list(e) + list(o)) }" for n, e, o in VARIANTS])
def test_variants_are_exact(name, env, opts, monkeypatch):
    """the same cases with the planner switched: 64 x 64 tiles for the big sources, the 4-wave 128 x 128 configuration, no per-tile records, the
    deterministic schedule (no fusion, no merged tiles, no atomics races), no merged tiles, no K-fusion, groups of three, split K on and off.
    Everything is exact, so every variant gives the values of the default run: L0 and U0."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, _ = _factor(name, **opts)
    st = h.stats()
    if "SLUAMD_NO_BIG_TILES" in env:
        assert st["flops_schur_exact_big"] == 0
    if "SLUAMD_NO_FUSE" in env or opts.get("deterministic"):
        assert st["reserved_i"] == 0
    if "SLUAMD_FUSE_GROUP_MIN_NODES" in env:
        assert st["reserved_i"] >= 2                                # a0 and a both deferred into b: the group of three
    _solve_exact(name, h)
    h.destroy()


@pytest.mark.parametrize("name", ["leads_big", "fuse_absent", "rows_and_merges"])
def test_second_factorisation_after_set_values_is_exact(name):
    """set_values() + a second factorisation on the same handle: the same exact factors.  (The per-tile records are written by a record-only launch
    at the start of the FIRST factorisation, which already reads them: the second run repeats its kernel mode on records that have lived through
    a factorisation, with the arena's values replaced.  A handle made from a store has no device copy of A: sluamd_dSetValues is its
    reset_values().)"""
    c, fs0, expL, expU, _ = _prepared(name)
    h, fs = _factor(name)
    fs.Lnzval[:] = fs0.Lnzval; fs.Unzval[:] = fs0.Unzval
    h.set_values(fs)
    assert h.pdgstrf3d(0.0) == 0
    fs.Lnzval[:] = 0; fs.Unzval[:] = 0
    h.copy_to_host()
    _assert_exact(fs, expL, expU, name + " (second factorisation)")
    h.destroy()


@pytest.mark.parametrize("sort", [True, False])
def test_shuffled_block_rows_are_exact(sort, monkeypatch):
    """rows inside the L blocks in another order than ascending (the reference's discovery order).  sort=True (the default): the library sorts a
    view's block rows on load and permutes them back in copy_to_host, so the kernel sees sorted panels -- this pins the host-side sort and its
    value permutation.  sort=False (SLUAMD_SORT_BLOCK_ROWS=0): the panels stay as given; a supernode's own row pairs are 16-byte runs of its
    panel whatever the row indices are, but the scatter maps and the pair maps of a K-fused predecessor (or the planner's refusal to fuse, when
    rows present in both panels are no neighbours) see the caller's order."""
    if not sort:
        monkeypatch.setenv("SLUAMD_SORT_BLOCK_ROWS", "0")
    for name in ("rows_and_merges", "fuse_absent"):
        h, _ = _factor(name, shuffle=5)
        _solve_exact(name, h)
        h.destroy()


def _two_tops_permuted():
    """the store of fuse_two_tops with the predecessor's off-diagonal L blocks (b, top 1, top 2) stored as (top 2, b, top 1), and its expected factors"""
    c, fs0, expL, expU, _ = _prepared("fuse_two_tops")
    fs, expL = _copy(fs0), expL.copy()
    sc.permute_l_blocks(fs, 1, [2, 0, 1], values=(expL,))
    fs._build_view()
    return fs, expL, expU


@pytest.mark.parametrize("env", [{}, {"SLUAMD_NO_BIG_TILES": "1"}, {"SLUAMD_NO_TILE_MAPS": "1"}, {"SLUAMD_NO_MERGE_TILES": "1"}, {"SLUAMD_NO_FUSE": "1"}],
                         ids=["default", "small-tiles", "no-records", "no-merge", "no-fuse"])
def test_fused_predecessor_with_blocks_in_another_order(env, monkeypatch):
    """the K-fused predecessor lists its L blocks in another order than its successor (l3_source / build_pair_maps): the fusion happens, and the
    factors are L0 and U0 in the caller's layout -- in both tile configurations, with and without the tile records and the merged row tiles
    (without them no tile pairs rows of two blocks), and with the fusion off"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fs, expL, expU = _two_tops_permuted()
    h = driver.LUHandle.from_store(fs)
    assert h.stats()["reserved_i"] == (0 if "SLUAMD_NO_FUSE" in env else 1)
    assert h.pdgstrf3d(0.0) == 0
    h.copy_to_host()
    _assert_exact(fs, expL, expU, "fuse_two_tops, blocks permuted")
    _solve_exact("fuse_two_tops", h)
    h.destroy()


def test_the_cases_cover_every_loader_decision(monkeypatch):
    """Coverage recomputed from the exported structure (xsup, L row lists, Ufstnz), plan_table() and stats(), never from the kernel: every row of the
    table of loader decisions has a case that exercises it, and the restatement of the planner's tile-configuration rule agrees with the
    library's own count.  Tiles are the UNMERGED tiles of a (source, row block, column block): schur_cases.tiles.
    Three tags are structural PRECONDITIONS, not observed launches (no statistic tells them): 'chain:split-K' (two 256-column pieces at the top and
    a big source below; by default every urgent big-tile launch of at most 64 tiles runs split K, so SLUAMD_KSPLIT=1 on chain_top is where the
    unsplit form of those tiles runs), 'rows:pair-split-across-blocks' and 'fuse:pair-across-blocks-only-second-row-present' (an odd-height
    block followed by another one: a pair straddles them where the planner merges the two into one row tile, which 'merged-tiles' shows it does
    for rows_and_merges by the tile count)."""
    seen = set()
    for name in sc.CASES:
        c, fs0, expL, expU, srcs = _prepared(name)
        h = driver.LUHandle.from_store(_copy(fs0))
        st = h.stats()
        nlev = len(h.plan_table())
        h.destroy()
        big = {s["k"]: sc.source_is_big(s, c.z) for s in srcs}
        # a K-fused (deferred) source runs in its successor's configuration: the restatement is checked with the fusion off, and the sources that
        # the planner may defer (their next supernode is one of their destinations) carry no label below -- the fuse_* cases look at them
        monkeypatch.setenv("SLUAMD_NO_FUSE", "1")
        h = driver.LUHandle.from_store(_copy(fs0))
        st1 = h.stats()
        h.destroy()
        monkeypatch.delenv("SLUAMD_NO_FUSE")
        assert st1["flops_schur_exact_big"] == (4.0 if c.z else 1.0) * sum(sc.exact_flops(s) for s in srcs if big[s["k"]]), name
        assert st1["flops_schur_exact"] == (4.0 if c.z else 1.0) * sum(sc.exact_flops(s) for s in srcs), name
        assert (st["flops_schur_exact_big"] > 0) == any(big.values()), name
        pre = "z:" if c.z else ""
        dests = {}
        for s in srcs:
            if not s["lblocks"] or not s["ublocks"] or s["lblocks"][0][0] == s["k"] + 1:
                continue
            K, cfg, kb = s["w"], "big" if big[s["k"]] else "small", sc.kbeg_of(s)
            seen.add(pre + "tile:" + cfg)
            for tag, ok in (("<16", K < 16), ("16", K == 16), ("16m", K % 16 == 0 and K > 16), ("16m+1", K % 16 == 1 and K > 16), ("16m+15", K % 16 == 15),
                            ("odd", K % 2 == 1), ("255", K == 255), ("256", K == 256)):
                if ok:
                    seen.add(f"{pre}K:{tag}:{cfg}")
            if len(s["lblocks"]) > 1 and any(len(r) % 2 for _, r in s["lblocks"][:-1]):
                seen.add(pre + "rows:pair-split-across-blocks")
            for rows, lds, cols, gi, gj in sc.tiles(s, big[s["k"]], c.z):
                nr, nc = len(rows), len(cols)
                clean = all(ld <= kb for ld in lds)
                dests.setdefault((gi, gj), set()).add(clean)
                seen.add(f"{pre}source:{'clean' if clean else 'unclean'}:{cfg}")
                for v in (1, 2, 127, 128, 129 - 128):
                    if nr == v:
                        seen.add(f"{pre}nr:{v}:{cfg}")
                if nr % 2:
                    seen.add(f"{pre}nr:odd:{cfg}")
                if nr % 2 == 0:
                    seen.add(f"{pre}nr:even:{cfg}")
                for v in (1, 63, 64, 65, 127, 128):
                    if nc == v:
                        seen.add(f"{pre}nc:{v}:{cfg}")
                if any(b - a > 1 for a, b in zip(cols[:-1], cols[1:])):
                    seen.add(pre + "nc:empty-segment-between")
                rel = [ld - kb for ld in lds]
                if sorted(rel).count(1) == 1 and sorted(rel)[-2] <= 0:
                    seen.add(f"{pre}lead:one-column-1:{cfg}")
                if any(ld % 2 for ld in lds) and any(ld and ld % 2 == 0 for ld in lds):
                    seen.add(f"{pre}lead:odd-and-even:{cfg}")
                if any(r >= 16 for r in rel):
                    seen.add(f"{pre}lead:>=16:{cfg}")
                if any(ld == K - 1 for ld in lds):
                    seen.add(f"{pre}lead:K-1:{cfg}")
                if kb >= 16:
                    seen.add(f"{pre}lead:source-starts-late:{cfg}")
                byc = dict(zip(cols, lds))
                if any((cc ^ 1) in byc and byc[cc ^ 1] != ld for cc, ld in byc.items()):
                    seen.add(f"{pre}lead:swizzle-pair-differs:{cfg}")
                if len({lds[i] for i in range(0, len(lds), 8)}) > 2:
                    seen.add(f"{pre}lead:differs-across-groups-of-8:{cfg}")      # (the loader's eight-column groups are groups of TILE columns)
        if any(v == {True, False} for v in dests.values()):
            seen.add(pre + "dest:clean-and-unclean-source")
        if name in ("fuse_clean", "fuse_absent", "fuse_three"):
            assert st["reserved_i"] >= 1, name                      # the fusion happened
            a, b = srcs[-3], srcs[-2]                                # predecessor and successor of the (last) pair
            rb = [r for _, rows in b["lblocks"] for r in rows]
            ra = set(r for g, rows in a["lblocks"] if g > b["k"] for r in rows)
            has = [r in ra for r in rb]
            pairs = list(zip(has[0::2], has[1::2]))
            seen.add("fuse:pair")
            if all(has):
                seen.add("fuse:all-rows-present")
            if (False, True) in pairs:
                seen.add("fuse:first-row-of-pair-absent")
            if (True, False) in pairs:
                seen.add("fuse:second-row-of-pair-absent")
            if (False, False) in pairs:
                seen.add("fuse:both-rows-absent")
            la, lb = dict(a["ublocks"])[srcs[-1]["k"]], dict(b["ublocks"])[srcs[-1]["k"]]
            if any(la[cc] != lb[cc] for cc in lb if cc in la):
                seen.add("fuse:leads-differ")
        if name == "fuse_two_tops":
            fsp = _two_tops_permuted()[0]
            h = driver.LUHandle.from_store(fsp)
            assert h.stats()["reserved_i"] == 1                     # the planner fuses the store with the permuted blocks
            h.destroy()
            a, b = sc.sources(fsp)[1:3]
            ga, gb = [g for g, _ in a["lblocks"] if g > b["k"]], [g for g, _ in b["lblocks"]]
            if sorted(ga) == gb and ga != gb:
                seen.add("fuse:predecessor-blocks-in-another-order")
            rb = [(g, r) for g, rows in b["lblocks"] for r in rows]
            ra = set(r for g, rows in a["lblocks"] if g > b["k"] for r in rows)
            posa = {g: i for i, g in enumerate(ga)}
            for (g0, r0), (g1, r1) in zip(rb[0::2], rb[1::2]):       # pairs of b's panel rows (of its merged row tiles: 251 rows, tiles start at even rows)
                if g0 != g1 and r0 not in ra and r1 in ra and posa[g1] < posa[g0]:
                    seen.add("fuse:pair-across-blocks-only-second-row-present")
        if name == "fuse_three":
            monkeypatch.setenv("SLUAMD_FUSE_GROUP_MIN_NODES", "1")
            h = driver.LUHandle.from_store(_copy(fs0))
            assert h.stats()["reserved_i"] >= 2
            h.destroy()
            monkeypatch.delenv("SLUAMD_FUSE_GROUP_MIN_NODES")
            seen.add("fuse:three")
        if name == "rows_and_merges":
            monkeypatch.setenv("SLUAMD_NO_MERGE_TILES", "1")
            h = driver.LUHandle.from_store(_copy(fs0))
            assert h.stats()["schur_tiles"] > st["schur_tiles"]    # rows / columns of several blocks share tiles at the defaults
            h.destroy()
            monkeypatch.delenv("SLUAMD_NO_MERGE_TILES")
            seen.add("merged-tiles")
        if name == "chain_top":
            assert np.diff(fs0.xsup)[-2:].tolist() == [256, 256] and nlev >= 3 and big[len(srcs) - 2]
            seen.add("chain:split-K")
        if name == "last_slot":
            last = [s for s in srcs if s["lblocks"] and s["ublocks"]][-1]
            nsupr = last["w"] + sum(len(r) for _, r in last["lblocks"])
            seg = last["w"] - list(last["ublocks"][-1][1].values())[-1]
            assert nsupr % 2 == 1 and seg % 2 == 1 and last["k"] == len(srcs) - 2
            seen.add("last-slot:odd-panel-and-odd-last-segment")
    need = {"tile:big", "tile:small", "z:tile:big", "z:tile:small",
            "K:<16:small", "K:16:small", "K:16m:big", "K:16m+1:big", "K:16m+1:small", "K:16m+15:big", "K:16m+15:small", "K:odd:big", "K:odd:small", "K:255:big", "K:256:big",
            "z:K:odd:big", "z:K:odd:small", "z:K:<16:small",
            "source:clean:big", "source:unclean:big", "source:clean:small", "source:unclean:small", "z:source:unclean:small", "z:source:unclean:big",
            "dest:clean-and-unclean-source", "z:dest:clean-and-unclean-source",
            "nr:1:big", "nr:127:big", "nr:128:big", "nr:1:small", "nr:2:small", "nr:odd:small", "nr:odd:big", "z:nr:odd:small", "z:nr:even:small", "z:nr:odd:big",
            "rows:pair-split-across-blocks",
            "nc:1:big", "nc:127:big", "nc:128:big", "nc:1:small", "nc:63:small", "nc:64:small", "nc:65:big", "nc:empty-segment-between",
            "fuse:pair", "fuse:three", "fuse:all-rows-present", "fuse:first-row-of-pair-absent", "fuse:second-row-of-pair-absent", "fuse:both-rows-absent",
            "fuse:leads-differ", "fuse:predecessor-blocks-in-another-order", "fuse:pair-across-blocks-only-second-row-present", "merged-tiles", "chain:split-K", "last-slot:odd-panel-and-odd-last-segment"}
    for cfg in ("big", "small"):
        need |= {f"lead:{t}:{cfg}" for t in ("one-column-1", "odd-and-even", ">=16", "K-1", "source-starts-late", "swizzle-pair-differs", "differs-across-groups-of-8")}
    need |= {"z:lead:odd-and-even:small", "z:lead:K-1:small", "z:lead:>=16:small"}
    assert need <= seen, sorted(need - seen)


def _tree_stores(name, Pz):
    """the 1 x 1 x Pz ranks' stores (full structure, ancestors zeroed on layers z > 0), forests and the supernodes each rank factors"""
    c, fs0, expL, expU, _ = _prepared(name)
    n, rp, ci = c.pattern_csr()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    tree = symb.partition(Pz)
    symb.free()
    out = []
    for z in range(Pz):
        fs = _copy(fs0)
        if c.z:
            fs.z = True
        fs.grid, fs.coords = (1, 1, Pz), (0, 0, z)
        fs._build_view()
        fr = grid_cases.forests_from_partition(tree, Pz, z)
        mine = np.zeros(len(tree), dtype=bool)
        for l, t in enumerate(fr["myTreeIdxs"]):
            if not fr["myZeroTrIdxs"][l]:
                mine |= tree == t
        if z:
            for k in np.flatnonzero(tree < Pz - 1):                  # ancestors start at zero on layers z > 0
                fs.Lnzval[fs.Lnzval_off[k]:fs.Lnzval_off[k + 1]] = 0
                fs.Unzval[fs.Unzval_off[k]:fs.Unzval_off[k + 1]] = 0
        out.append((fs, fr, mine))
    return out, expL, expU


@pytest.mark.parametrize("name", ["leads_big", "z_leads"])
def test_two_z_layers_hold_exact_factors(name):
    """1 x 1 x 2 through the view path (grid3d.local_comms): every supernode a rank factors holds L0 / U0, every stored value, per rank"""
    stores, expL, expU = _tree_stores(name, 2)
    comms = grid3d.local_comms(1, 1, 2)

    def body(z):
        fs, fr, mine = stores[z]
        h = grid3d.GridHandle.from_store(fs, fr, comms[z])
        info = h.pdgstrf3d(0.0)
        h.copy_to_host(fs)
        h.destroy()
        bad = []
        for k in np.flatnonzero(mine):
            a, e = fs.Lnzval_off[k], fs.Lnzval_off[k + 1]
            if not np.array_equal(fs.Lnzval[a:e], expL[a:e]):
                bad.append(("L", z, int(k)))
            a, e = fs.Unzval_off[k], fs.Unzval_off[k + 1]
            if not np.array_equal(fs.Unzval[a:e], expU[a:e]):
                bad.append(("U", z, int(k)))
        return info, bad, int(mine.sum())

    out = grid3d.run_ranks(2, body)
    assert all(info == 0 for info, _, _ in out) and not any(bad for _, bad, _ in out), out
    assert all(cnt > 0 for _, _, cnt in out)


@pytest.mark.parametrize("grid", [(2, 1, 1), (1, 1, 2), (2, 2, 2)])
@pytest.mark.parametrize("name", ["leads_small", "z_leads"])
def test_process_grids_return_the_exact_solution(name, grid):
    """B through the library's own distribution on Pr x Pc x Pz thread grids: info == 0 on every rank and the integer x back from every rank's solve,
    bitwise -- which needs every factor entry the sweeps read to be exact.  (The ranks' stores of an XY layer have no host-side export; their
    values are pinned through the solution.)"""
    c = _prepared(name)[0]
    n, rp, ci = c.pattern_csr()
    rows = np.repeat(np.arange(n), np.diff(rp))
    v = c.B[rows, ci].copy()
    symb = driver.Symbolic(n, rp, ci, np.arange(n, dtype=np.int32), relax=1, maxsup=c.maxsup, unsym=True)
    Pr, Pc, Pz = grid
    tree = symb.partition(Pz) if Pz > 1 else None
    comms = grid3d.local_comms(Pr, Pc, Pz)
    x, b = c.rhs(3)

    def body(rank):
        h = grid3d.GridHandle.from_symbolic(symb, v, comms[rank], tree)
        info = h.pdgstrf3d(0.0)
        y = h.pdgstrs3d(b.copy(order="F"))
        h.destroy()
        return info, y

    out = grid3d.run_ranks(Pr * Pc * Pz, body)
    symb.free()
    for rank, (info, y) in enumerate(out):
        assert info == 0
        assert np.array_equal(y, x), (rank, int(np.count_nonzero(y != x)))
