// devmem_check.cpp -- stand-alone check of the device-memory owners (superlu_dist_amd/csrc/sluamd_devmem.h) on the CPU, over the emulated runtime, for
// sanitizer builds:
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -Ioracle/emul -Isuperlu_dist_amd/csrc -Iinclude scripts/devmem_check.cpp oracle/emul/emul_rt.cpp -o devmem_check && ./devmem_check
// DevBuf: alloc / reserve / reset / move, a failed allocation and a failed-then-retried one; DevBag: allocation, move, failure; PoolBuf.  After every
// block nothing is left allocated (sluamd_emul_live_allocs), and the sanitizers see every byte the buffers hand out written and every free.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include "sluamd_devmem.h"

extern "C" long long sluamd_emul_live_allocs();
extern "C" long long sluamd_emul_alloc_count();
extern "C" void sluamd_emul_alloc_fail(long long first, long long count);

static std::string g_err;
namespace sluamd { void set_error(const std::string &m) { g_err = m; } }
using namespace sluamd;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

int main()
{
    const long long live0 = sluamd_emul_live_allocs();
    {   // alloc, reserve (grow-only), reset
        DevBuf<double> b;
        CHECK(!b && b.get() == nullptr && b.cap == 0);
        CHECK(b.reserve(10, 0, "ten doubles") == 0 && b && b.cap == 10);
        std::memset(b.p, 0, sizeof(double) * 10);
        double *p10 = b.p;
        CHECK(b.reserve(4, 0, "four doubles") == 0 && b.p == p10 && b.cap == 10);          // never shrinks, never reallocates
        const long long c = sluamd_emul_alloc_count();
        CHECK(b.reserve(10, 0, "ten doubles") == 0 && sluamd_emul_alloc_count() == c);      // a compare and a return
        CHECK(b.reserve(100, 0, "a hundred doubles") == 0 && b.cap == 100);
        std::memset(b.p, 1, sizeof(double) * 100);
        CHECK(b.alloc(0, 0, "nothing") == 0 && b && b.cap == 0);                            // max(bytes, 1): a valid pointer
        b.reset();
        CHECK(!b && b.cap == 0);
        b.reset();                                                                          // twice is fine
        CHECK(sluamd_emul_live_allocs() == live0);
    }
    {   // move construction and assignment: one owner at any time
        DevBuf<int> a;
        CHECK(a.alloc(7, 0, "seven ints") == 0);
        int *pa = a.p;
        DevBuf<int> b(std::move(a));
        CHECK(!a && a.cap == 0 && b.p == pa && b.cap == 7);
        DevBuf<int> c;
        CHECK(c.alloc(3, 0, "three ints") == 0);
        c = std::move(b);                                                                   // frees its three ints first
        CHECK(!b && c.p == pa && c.cap == 7);
        c = std::move(c);                                                                   // self-assignment keeps the buffer
        CHECK(c.p == pa && c.cap == 7);
        c.p[6] = 42;
        CHECK(sluamd_emul_live_allocs() == live0 + 1);
    }
    CHECK(sluamd_emul_live_allocs() == live0);
    {   // failure: SLUAMD_ENOMEM, a message that names the buffer, the sticky error cleared, the buffer empty; a single failure is retried
        DevBuf<double> b;
        CHECK(b.alloc(5, 0, "five doubles") == 0);
        sluamd_emul_alloc_fail(0, -1);
        g_err.clear();
        CHECK(b.reserve(50, 0, "the fifty doubles") == SLUAMD_ENOMEM);
        CHECK(!b && b.cap == 0);
        CHECK(g_err.find("the fifty doubles") != std::string::npos && g_err.find("400 bytes") != std::string::npos);
        CHECK(hipGetLastError() == hipSuccess);
        sluamd_emul_alloc_fail(0, 1);
        g_err.clear();
        const long long c = sluamd_emul_alloc_count();
        CHECK(b.reserve(50, 0, "the fifty doubles") == 0 && b.cap == 50 && g_err.empty());
        CHECK(sluamd_emul_alloc_count() == c + 2);                                          // the failed attempt and the retry
        CHECK(hipGetLastError() == hipSuccess);
        sluamd_emul_alloc_fail(-1, 0);
        std::memset(b.p, 0, sizeof(double) * 50);
    }
    CHECK(sluamd_emul_live_allocs() == live0);
    {   // the bag: raw pointers out, everything freed with it; a failed allocation adds nothing; move
        DevBag bag;
        int *i3 = nullptr; double *d0 = nullptr;
        CHECK(bag.alloc(&i3, 3, "three ints") == 0 && i3);
        CHECK(bag.alloc(&d0, 0, "no doubles") == 0 && d0);
        i3[2] = 1;
        sluamd_emul_alloc_fail(0, -1);
        char *c9 = (char *) 1;
        CHECK(bag.alloc(&c9, 9, "nine chars") == SLUAMD_ENOMEM && c9 == nullptr);
        sluamd_emul_alloc_fail(-1, 0);
        CHECK(sluamd_emul_live_allocs() == live0 + 2);
        DevBag other(std::move(bag));
        CHECK(sluamd_emul_live_allocs() == live0 + 2);
        DevBag third;
        int *i1 = nullptr;
        CHECK(third.alloc(&i1, 1, "one int") == 0);
        third = std::move(other);                                                           // frees its one int first
        CHECK(sluamd_emul_live_allocs() == live0 + 2);
        i3[0] = 2;                                                                          // still alive, owned by `third`
        third.clear();
        CHECK(sluamd_emul_live_allocs() == live0);
    }
    {   // the arena wrapper: the emulated pool declines, the plain path serves; failure as above
        PoolBuf v;
        CHECK(v.alloc(64, 0, true, "the value arena") == 0 && v);
        std::memset(v.p, 0, 64);
        CHECK(v.alloc(128, 0, false, "the value arena") == 0);                              // frees the first
        CHECK(sluamd_emul_live_allocs() == live0 + 1);
        sluamd_emul_alloc_fail(0, -1);
        CHECK(v.alloc(256, 0, true, "the value arena") == SLUAMD_ENOMEM && !v);
        sluamd_emul_alloc_fail(-1, 0);
    }
    CHECK(sluamd_emul_live_allocs() == live0);
    printf(fails ? "devmem_check: %d checks FAILED\n" : "devmem_check: all checks passed\n", fails);
    return fails ? 1 : 0;
}
