"""Refinement entry points on the CPU test build of the library's host sources (oracle/libsluamd_emul.so, the `emul` fixture).
That build restates the double kernels only: it has no complex16 refinement, and the ctypes layer must still bind it and say
which entry point is missing.  The double refinement on process grids (GridHandle, replicated form, collective stopping
decision) runs here on the reference's grid fixtures, as on the GPU in test_gpu_zrefine.py."""
import numpy as np
import pytest
import refine_cases as rc


def test_binding_the_cpu_build_names_the_missing_complex_entry_point(emul):
    from superlu_dist_amd import _lib, driver, matgen
    assert _lib.load() is emul                       # _lib.bind succeeded on a library without the complex refinement symbols
    assert not hasattr(emul, "sluamd_zAttachMatrix")
    n, rp, ci, v = matgen.poisson3d(4)
    v = matgen.complex_shift(v, rp, ci, seed=1)
    b = np.ones((n, 1), dtype=np.complex128)
    x, info, st, h, symb = driver.pzgssvx3d(n, rp, ci, v, b, relax=8, maxsup=16, keep=True)
    try:
        assert info == 0 and h.z
        with pytest.raises(RuntimeError, match="sluamd_zAttachMatrix"):
            h.attach_matrix(n, rp, ci, v, symb.perm_c)
        with pytest.raises(RuntimeError, match="sluamd_pzgsrfs3d"):
            h.pzgsrfs3d(b, x)
    finally:
        h.destroy(); symb.free()


@pytest.mark.parametrize("case", ["g20_1x1x2", "g20_2x1x1", "g20_2x2x2"])
def test_double_refinement_on_grid_fixtures_on_the_cpu_build(emul, golden, case):
    rc.check_refined_fixture_on_grid(golden(case), check_steps=False)
