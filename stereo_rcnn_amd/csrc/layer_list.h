// A LIST of tensors or layers in one library call: what csrc/optim.hip, prep_weights.hip, train_weights.hip and train_fold.hip
// share.  The list travels by value in kernel-argument blocks (nothing is uploaded by the host runtime), all the way (optim,
// prep_weights) or as far as a table in the workspace (row_table_kernel: train_weights, train_fold); a workgroup finds the entry of
// its unit of work by first_run_above.  The search and the part lookup compile as plain C++ (tests/test_layer_list_cpu.py).
#pragma once

#if defined(__HIPCC__)
#include "common.h"
#define SRCNN_LIST_HD __host__ __device__ __forceinline__
#else
#define SRCNN_LIST_HD inline
#endif

namespace srcnn {

// The first index i of n whose running count end(i) exceeds u, for u below the last count: entry i owns the units
// [end(i - 1), end(i)), an entry without units owns none and is skipped.  Uniform over a workgroup when u is (scalar loads).
template <typename End>
SRCNN_LIST_HD int first_run_above(int n, int u, End end)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (u < end(mid)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// ... over a plain array of counts
SRCNN_LIST_HD int first_run_above(const int *end, int n, int u)
{
    return first_run_above(n, u, [end](int i) { return end[i]; });
}

// ... over the member `end` of a table's rows
template <typename Row>
SRCNN_LIST_HD int first_run_above(const Row *table, int Row::*end, int n, int u)
{
    return first_run_above(n, u, [table, end](int i) { return table[i].*end; });
}

// part p and row r inside it of row `row` of up to three parts concatenated along their rows
SRCNN_LIST_HD void part_of_row(int nparts, const int *rows, int row, int &p, int &r)
{
    p = 0, r = row;
    if (nparts > 1 && r >= rows[0]) {
        r -= rows[0], p = 1;
        if (nparts > 2 && r >= rows[1]) r -= rows[1], p = 2;
    }
}

#if defined(__HIPCC__)

// N rows of a table on their way to the device; a user asserts sizeof(RowBlock) <= 4096 - sizeof(void *), HIP's argument block
template <typename Row, int N>
struct RowBlock {
    Row r[N];
    int n, base;                                   // rows of this block, number of its first row in the table
};

// CLEAR_WORD: the row's `word` (a device word that atomics of a LATER launch accumulate into) is zeroed with the row
template <typename Row, int N, bool CLEAR_WORD>
__global__ __launch_bounds__(64) void row_table_kernel(const RowBlock<Row, N> b, Row *table)
{
    static_assert(N <= 64, "one thread per row");
    const int i = threadIdx.x;
    if (i < b.n) {
        table[b.base + i] = b.r[i];
        if constexpr (CLEAR_WORD) *b.r[i].word = 0u;
    }
}

// Host: the caller has filled b.r[b.n]; a full block, and the list's last one, goes to table[b.base ..] in one launch
// (table == nullptr: a counting pass, nothing is launched).  Start with b.n = b.base = 0.
template <bool CLEAR_WORD, typename Row, int N>
inline void push_row(RowBlock<Row, N> &b, bool last, Row *table, hipStream_t st)
{
    if (++b.n == N || last) {
        if (table) launch_kernel(row_table_kernel<Row, N, CLEAR_WORD>, dim3(1), dim3(64), 0, st, b, table);
        b.base += b.n, b.n = 0;
    }
}

#endif

}  // namespace srcnn
