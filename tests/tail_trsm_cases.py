"""Chains of single-supernode tail levels for the 64-high blocked substitution of the panel chain (k_panel_tsub, and k_panel_trsm<64> under
SLUAMD_TRSM_LDS_STRIP): one case per supernode width, built with the machinery of panel_cases.py / sweep_cases.py -- exact factors, dense exactly known
inverses of the diagonal blocks, both panel forms bounded entry by entry (test helper for test_gpu_tail_trsm.py and test_tail_trsm_cases_cpu.py; not a
conftest).

A case of width W is  guard (1 column) -> a (W) -> b (W) -> top (90):  four single-supernode levels, all tail levels at the default SLUAMD_TRSM_TAIL.
  a: 5 rows below the diagonal block (fewer than a wave's 16: one partly filled wave, three idle ones), all in b; 85 = 64 + 16 + 5 skyline columns, 20 in b
     and 65 in top, with the leads 0, 1, 31, 32 and W - 1 in turn (a follows a one-column guard: its designed leads survive the symbolic factorisation).
     Its level is split by build_panel_split: the strip and the first column chunk feed b's diagonal block (urgent list), the second chunk does not.
  b: 85 rows and 85 columns of top (a full unit, a full wave and a partly filled one), stored at full height; every unit feeds the top's diagonal block, so the
     split is refused and the level takes the prefix form.
The widths: 256 (eight full blocks), 255 (odd: no 16-byte loads anywhere), 200 (ragged last block, 6 x 32 + 8), 129 (one column into the fifth block: the
narrowest width of the 64-register build), 96 (the 32-register build), 64 and 33 (the 16-register build, full and one column into the second block)."""
import panel_cases as pn

WIDTHS = [256, 255, 200, 129, 96, 64, 33]
TOP = 90
G, A, B, T = range(4)


def lead_set(w):
    return [0, 1, 31, 32, w - 1]


def tail_chain(w):
    leads = lead_set(w)
    L = {G: {A: [0]}, A: {B: list(range(1, 6))}, B: {T: list(range(1, 86))}}
    U = {G: {A: {0: 0}},
         A: {B: {c: leads[c % 5] for c in range(1, 21)}, T: {c: leads[(c + 2) % 5] for c in range(1, 66)}},
         B: {T: {c: 0 for c in range(1, 86)}}}
    return pn.PanelCase("tail%d" % w, "tail levels of %d-column supernodes" % w, [1, w, w, TOP], L, U, guards=[G])


CASES = {w: (lambda w=w: tail_chain(w)) for w in WIDTHS}

# the forms of the tests: name -> (environment, settings of panel_cases.predicted_lines); each runs with the strip in registers and, under
# SLUAMD_TRSM_LDS_STRIP=1, in LDS -- the switch changes no launch line
FORMS = {
    "split": ({}, {}),                                                      # look-ahead schedule: a's level as urgent and remaining lists, b's whole
    "whole": ({"SLUAMD_PANEL_SPLIT": "0"}, {"panel_split": 0}),             # look-ahead schedule, prefix form on every level
    "serial": ({"SLUAMD_NO_LOOKAHEAD": "1"}, {"no_lookahead": True}),       # serial schedule (prefix form)
}
IMPLS = {"regs": {}, "lds": {"SLUAMD_TRSM_LDS_STRIP": "1"}}
