// sluamd_match.cpp -- see sluamd_match.h.  Host only, no HIP.
#include "sluamd_match.h"
#include <cmath>
#include <queue>
#include <utility>
#include <vector>

namespace sluamd {

int64_t match_augment(int64_t n, const int32_t *rowptr, const int32_t *colind, const double *cost, double *u, double *v, int32_t *rowmatch,
                      int32_t *colmatch, int64_t *augmentations)
{
    typedef std::pair<double, int32_t> Item;                       // (distance, column): the smallest distance first, then the lowest column
    std::vector<double> dist((size_t) n, HUGE_VAL);
    std::vector<int32_t> pred((size_t) n, -1);
    std::vector<uint8_t> done((size_t) n, 0);
    std::vector<int32_t> touched, settled;
    int64_t unmatched = 0, paths = 0;
    for (int64_t r0 = 0; r0 < n; ++r0) {
        if (rowmatch[r0] >= 0) continue;
        std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
        touched.clear(); settled.clear();
        int32_t row = (int32_t) r0, sink = -1;
        double drow = 0.0, dsink = 0.0;
        for (;;) {
            const double ui = u[row];
            for (int32_t e = rowptr[row]; e < rowptr[row + 1]; ++e) {
                const double c = cost[e];
                if (!(c < HUGE_VAL)) continue;
                const int32_t j = colind[e];
                if (done[j]) continue;
                const double red = std::fmax((c - ui) - v[j], 0.0), nd = drow + red;
                if (nd < dist[j]) {
                    if (dist[j] == HUGE_VAL) touched.push_back(j);
                    dist[j] = nd; pred[j] = row;
                    heap.push(Item(nd, j));
                }
            }
            int32_t j = -1;
            while (!heap.empty()) {                                 // stale entries: a column settled already, or pushed again with a smaller distance
                const Item t = heap.top(); heap.pop();
                if (!done[t.second] && t.first == dist[t.second]) { j = t.second; break; }
            }
            if (j < 0) break;
            done[j] = 1; settled.push_back(j);
            if (colmatch[j] < 0) { sink = j; dsink = dist[j]; break; }
            row = colmatch[j]; drow = dist[j];                      // the matched entry is tight: the row is as far as its column
        }
        if (sink < 0) {
            ++unmatched;
        } else {
            // duals: a settled column moves down by what it lacks to the sink's distance, its matched row up by the same amount, the root up by the whole
            for (int32_t j : settled) {
                const double d = dsink - dist[j];
                if (j != sink) u[colmatch[j]] += d;
                v[j] -= d;
            }
            u[r0] += dsink;
            for (int32_t j = sink; j >= 0;) {                       // flip the path back to the root
                const int32_t i = pred[j], jn = rowmatch[i];
                rowmatch[i] = j; colmatch[j] = i;
                j = jn;
            }
            ++paths;
        }
        for (int32_t j : touched) { dist[j] = HUGE_VAL; pred[j] = -1; done[j] = 0; }
    }
    if (augmentations) *augmentations = paths;
    return unmatched;
}

}  // namespace sluamd
