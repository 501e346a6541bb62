// Host check of the chunk and stage index arithmetic of panel_gemm_wg (sluamd_kernels.hip), restated for one workgroup of 256 threads and run for
// every supernode width 1 .. 256 in both modes.  Build with -fsanitize=address,undefined and run: every global and LDS access goes through a real
// heap array of exactly the size the kernel has, so an index that leaves its buffer is a sanitizer report; the assertions check that the flat,
// trimmed chunk sequence feeds the MFMAs of output block jb exactly the k range [0, 32 (jb + 1)) once, in ascending order, from the right buffer.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined scripts/panel_gemm_chunks_check.cpp -o pgc && ./pgc
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

constexpr int DB = 32, PGK = 32, PG_LD0 = PGK + 2, PG_LD1 = 48, PG_BUF = PGK * PG_LD1, PG_LDS = 2 * PG_BUF, NT = 256;

static double tinv(int k, int n) { return k <= n ? 1000.0 * k + n + 1 : 0.0; }      // upper triangular, every stored non-zero distinct

template <int MODE>
static long check(int ns, int NQ, bool aligned_base)
{
    const int nblk = (ns + DB - 1) / DB;
    constexpr int LD = MODE == 0 ? PG_LD0 : PG_LD1;
    // the inverse as the kernel sees it: MODE 0 Tinv(k, n) at [k + n ns], MODE 1 at [n + k ns]; one spare double in front models an odd base offset
    std::vector<double> mem((size_t) ns * ns + (aligned_base ? 0 : 1));
    double *Ti = mem.data() + (aligned_base ? 0 : 1);
    for (int k = 0; k < ns; ++k)
        for (int n = 0; n < ns; ++n) Ti[MODE == 0 ? k + (size_t) n * ns : n + (size_t) k * ns] = tinv(k, n);
    std::vector<double> lds(PG_LDS, -1.0);
    double *Ts = lds.data();
    std::vector<int> cover((size_t) 256 * 256, 0), lastk(256, -1);
    const bool wide = (ns & 1) == 0 && aligned_base;      // (the kernel tests the address itself: base offsets are even or odd doubles)
    long wide_loads = 0;
    std::vector<double> regs((size_t) NT * 4);
    auto fetch = [&](int jb, int kb) {
        for (int tid = 0; tid < NT; ++tid) {
            double *r = &regs[(size_t) tid * 4];
            const int f2 = (tid & 15) * 2, s0 = tid >> 4;
            const int F0 = (MODE == 0 ? kb : jb) * DB + f2, S0 = (MODE == 0 ? jb : kb) * DB + s0;
            if (wide && jb * DB + DB <= ns) {
                for (int e = 0; e < 2; ++e) {
                    const double *p = Ti + F0 + (size_t) (S0 + 16 * e) * ns;
                    assert(((p - mem.data()) & 1) == 0);                               // a 16-byte load at a 16-byte aligned address
                    r[2 * e] = p[0]; r[2 * e + 1] = p[1];
                    ++wide_loads;
                }
            } else {
                for (int e = 0; e < 2; ++e) {
                    const int S = S0 + 16 * e;
                    r[2 * e] = (F0 < ns && S < ns) ? Ti[F0 + (size_t) S * ns] : 0.0;
                    r[2 * e + 1] = (F0 + 1 < ns && S < ns) ? Ti[F0 + 1 + (size_t) S * ns] : 0.0;
                }
            }
        }
    };
    auto stash = [&](int buf) {
        for (int tid = 0; tid < NT; ++tid) {
            const int f2 = (tid & 15) * 2, s0 = tid >> 4;
            for (int e = 0; e < 2; ++e) {
                const int at = buf * PG_BUF + (s0 + 16 * e) * LD + f2;
                assert((at & 1) == 0 && at / PG_BUF == buf);                           // 16-byte store inside its own buffer
                Ts[at] = regs[(size_t) tid * 4 + 2 * e]; Ts[at + 1] = regs[(size_t) tid * 4 + 2 * e + 1];
            }
        }
    };
    long mfma = 0;
    fetch(0, 0); stash(0);
    int buf = 0;
    for (int jb = 0; jb < nblk; ++jb)
        for (int kb = 0; kb < NQ / 8; ++kb)
            if (kb <= jb) {
                const int njb = kb == jb ? jb + 1 : jb, nkb = kb == jb ? 0 : kb + 1;
                const bool more = njb < nblk;
                if (more) fetch(njb, nkb);
                const double *Tc = Ts + buf * PG_BUF;
                for (int qq = 0; qq < 8; ++qq) {
                    assert(8 * kb + qq < NQ);                                          // the strip fragment register a[8 kb + qq]
                    for (int lane = 0; lane < 64; ++lane) {
                        const int li = lane & 15, lk = lane >> 4, kl = 4 * qq + lk;
                        for (int h = 0; h < 2; ++h) {
                            const int at = MODE == 0 ? (16 * h + li) * LD + kl : kl * LD + 16 * h + li;
                            assert(at >= 0 && at < PG_BUF);
                            const int kg = kb * DB + kl, n = jb * DB + 16 * h + li;
                            const double want = (kg < ns && n < ns) ? tinv(kg, n) : 0.0;
                            assert(Tc[at] == want);                                    // the right element of the right chunk from the right buffer
                            if (n < ns && kg < ns) {
                                ++cover[(size_t) kg * 256 + n];
                                if (lk == 0 && h == 0 && li == 0) { assert(kg > lastk[jb] || lastk[jb] < 0); }
                            }
                        }
                    }
                    lastk[jb] = kb * DB + 4 * qq;                                      // k groups of a block come in ascending order
                    mfma += 2;
                }
                if (more) stash(buf ^ 1);
                buf ^= 1;
            }
    for (int k = 0; k < ns; ++k)
        for (int n = 0; n < ns; ++n) {
            const int want = k < DB * (n / DB + 1) ? 1 : 0;                            // exactly the block upper triangle: every non-zero once, no zero block
            assert(cover[(size_t) k * 256 + n] == want);
            if (k <= n) assert(want == 1);
        }
    assert(mfma == 8L * nblk * (nblk + 1));                                           // 16 per chunk, nblk (nblk + 1) / 2 chunks
    if (!wide) assert(wide_loads == 0);
    if (wide && ns >= DB) assert(wide_loads > 0);
    return mfma;
}

int main()
{
    long total = 0, old_total = 0;
    for (int ns = 1; ns <= 256; ++ns) {
        const int NQ = ns <= 64 ? 16 : ns <= 128 ? 32 : 64;
        for (int al = 0; al < 2; ++al) {
            total += check<0>(ns, NQ, al);
            total += check<1>(ns, NQ, al);
            if (NQ < 64) { check<0>(ns, 64, al); check<1>(ns, 64, al); }               // a narrow supernode on a level of wide ones
        }
        const int nblk = (ns + DB - 1) / DB;
        for (int jb = 0; jb < nblk; ++jb) old_total += 4L * 32 * (jb / 2 + 1);       // the untrimmed 64-deep chunks: 32 MFMAs each, twice two runs
    }
    std::printf("panel_gemm chunk check: ns 1..256, both modes, aligned and odd bases: ok; MFMAs %ld (64-deep untrimmed chunks: %ld)\n", total, old_total);
    return 0;
}
