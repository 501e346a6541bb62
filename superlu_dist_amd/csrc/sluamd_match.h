// sluamd_match.h -- host part of RowPerm = LargeDiag_MC64: shortest augmenting paths that complete a partial minimum-cost matching (Duff & Koster 2001,
// section 4: Dijkstra on the reduced costs, dual update, augmentation).  Plain C++, no HIP: sluamd_rowperm.cpp hands it the costs, duals and partial matching
// the device computed; a stand-alone program can link this file alone.
#pragma once
#include <cstdint>

namespace sluamd {

// CSR pattern (rowptr[n + 1], colind) with cost[e] >= 0 per entry, +inf: not an edge.  u[n], v[n]: duals with (cost - u_i) - v_j >= 0 on every edge and == 0
// on the matched ones; rowmatch[i] = column of row i or -1, colmatch[j] = row of column j or -1 (consistent with each other).
// For every unmatched row in ascending order: the shortest path, in reduced costs, to a free column (binary heap; ties go to the lower column index);
// the duals of the scanned rows and settled columns move so that the path becomes tight and feasibility holds, then the matching is flipped along the path.
// A row that reaches no free column stays unmatched and leaves the duals alone.  Returns the number of such rows; *augmentations = paths found.
int64_t match_augment(int64_t n, const int32_t *rowptr, const int32_t *colind, const double *cost, double *u, double *v, int32_t *rowmatch,
                      int32_t *colmatch, int64_t *augmentations);

}  // namespace sluamd
