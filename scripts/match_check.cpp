// match_check.cpp -- stand-alone check of the host part of LargeDiag_MC64 (superlu_dist_amd/csrc/sluamd_match.cpp) on the CPU, for sanitizer builds:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Isuperlu_dist_amd/csrc scripts/match_check.cpp superlu_dist_amd/csrc/sluamd_match.cpp -o match_check && ./match_check
// Random sparse integer-cost problems (dense enough to be matchable, plus singular ones), from empty and from greedy partial matchings: after the call the
// matching is consistent, the duals are feasible, matched entries are tight, and the cost equals that of a run from the empty matching.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "sluamd_match.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

int main()
{
    std::mt19937 rng(12345);
    for (int trial = 0; trial < 200; ++trial) {
        const int n = 1 + rng() % 60;
        const double dens = 0.05 + (rng() % 100) / 250.0;
        std::vector<int32_t> rp(n + 1, 0), ci;
        std::vector<double> cost;
        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < n; ++j)
                if ((rng() % 1000) < dens * 1000 || (trial % 3 && j == (i * 7 + 3) % n && n % 7)) { ci.push_back(j); cost.push_back(rng() % 5 == 0 ? HUGE_VAL : (double) (rng() % 9)); }
            rp[i + 1] = (int32_t) ci.size();
        }
        // initial feasible duals: u = row minimum, v = column minimum of cost - u
        std::vector<double> u(n, HUGE_VAL), v(n, HUGE_VAL);
        for (int i = 0; i < n; ++i) for (int e = rp[i]; e < rp[i + 1]; ++e) u[i] = std::fmin(u[i], cost[e]);
        for (int i = 0; i < n; ++i) for (int e = rp[i]; e < rp[i + 1]; ++e) if (cost[e] < HUGE_VAL) v[ci[e]] = std::fmin(v[ci[e]], cost[e] - u[i]);
        double total[2] = {0, 0};
        int64_t left[2] = {0, 0};
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<double> uu = u, vv = v;
            std::vector<int32_t> rm(n, -1), cm(n, -1);
            if (pass)   // greedy on the tight entries
                for (int i = 0; i < n; ++i) for (int e = rp[i]; e < rp[i + 1]; ++e)
                    if (cost[e] < HUGE_VAL && cm[ci[e]] < 0 && cost[e] - u[i] == v[ci[e]]) { rm[i] = ci[e]; cm[ci[e]] = i; break; }
            int64_t aug = -1;
            left[pass] = sluamd::match_augment(n, rp.data(), ci.data(), cost.data(), uu.data(), vv.data(), rm.data(), cm.data(), &aug);
            int64_t matched = 0;
            for (int i = 0; i < n; ++i) {
                if (rm[i] >= 0) { ++matched; CHECK(cm[rm[i]] == i); }
                for (int e = rp[i]; e < rp[i + 1]; ++e) {
                    if (!(cost[e] < HUGE_VAL)) { CHECK(rm[i] != ci[e]); continue; }
                    if (!std::isfinite(uu[i]) || !std::isfinite(vv[ci[e]])) continue;
                    CHECK(cost[e] - uu[i] - vv[ci[e]] >= 0);
                    if (rm[i] == ci[e]) { CHECK(cost[e] - uu[i] - vv[ci[e]] == 0); total[pass] += cost[e]; }
                }
            }
            CHECK(matched + left[pass] == n);
            CHECK(aug >= 0 && aug <= n);
        }
        CHECK(left[0] == left[1]);
        if (left[0] == 0) CHECK(total[0] == total[1]);
    }
    printf(fails ? "match_check: %d FAILED\n" : "match_check: ok\n", fails);
    return fails != 0;
}
