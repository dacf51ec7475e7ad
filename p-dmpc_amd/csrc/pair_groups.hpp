// pair_groups.hpp — where a coupler kernel writes vehicle i's row of results and which columns the row has: the whole n x n matrix of
// the ungrouped calls, or the n_g x n_g block of i's group (PairGroup, pdmpc_device.h) in the grouped ones.  DESIGN.md §3.20.
#pragma once
#include <hip/hip_runtime.h>

#include "pdmpc_device.h"

struct RowOut {
    int first, end;  // the columns (vehicles) of the row
    size_t base;     // element offset of the block
    int stride;      // = end - first
    __device__ size_t at(int i, int j) const { return base + (size_t)(i - first) * stride + (j - first); }
};
template <bool GROUPED>
__device__ inline RowOut row_out(const int32_t* group, int n, int i) {
    RowOut r;
    if (GROUPED) {
        const PairGroup g = ((const PairGroup*)group)[i];
        r.first = g.first;
        r.end = g.end;
        r.base = (size_t)g.block;
    } else {
        r.first = 0;
        r.end = n;
        r.base = 0;
    }
    r.stride = r.end - r.first;
    return r;
}
