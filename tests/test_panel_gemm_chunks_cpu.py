"""The chunk and stage index arithmetic of k_panel_gemm on the host: scripts/panel_gemm_chunks_check.cpp restates it for one workgroup and runs every
supernode width 1 .. 256 in both modes, with 16-byte aligned and odd bases, as a stand-alone program under AddressSanitizer and UBSan (host code only:
nothing here touches a device or loads into Python).  It asserts that the trimmed, flattened chunk sequence feeds each output block exactly the k range
[0, 32 (jb + 1)) once and in ascending order, from the buffer the pipeline filled for it, and that no global or stage index leaves its array."""
import os, subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_sequence_and_stage_indices_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pgc")
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           os.path.join(ROOT, "scripts", "panel_gemm_chunks_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-1000:] + r.stderr[-2000:]
