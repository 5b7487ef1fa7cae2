// pair.hpp -- the phases every pair kernel ends with, defined once: pair_k and pair_pred_k (local_w.hip) and pair_gen_pred_k
// (local_x.hip) call them.  Each is inlined into its kernel; the LDS arrays belong to the kernels and come in as pointers.
#pragma once
#include <type_traits>

#include "local_args.hpp"

namespace esplocal {

// place scan: where the lane's column starts among the pair's records, and how many records the pair emits (total comes from
// LDS: the same answer in every lane).  One barrier: behind it every lane holds its run in registers
struct PairPlace {
    u32 at0, total;
};
__device__ __forceinline__ PairPlace pair_place(u32 ec, u32 *lw, int lane, int w) {
    const u32 einc = esp_wave_scan_add(ec);
    if (lane == 63) lw[w] = einc;
    __syncthreads();
    PairPlace pl{einc - ec, 0u};
#pragma unroll
    for (int i = 0; i < WAVES; i++) {
        pl.at0 += i < w ? lw[i] : 0u;
        pl.total += lw[i];
    }
    return pl;
}

// table hit (the PREDICTED forms): the pair's place is the table's when it emits what the table says -- pred[0] = 0 and every
// pair's count right: the table is the exclusive prefix sum the look-back would resolve -- and ends inside the output arrays.
// This is what keeps a spoiled table from storing outside them: on a miss the kernel stores nothing
__device__ __forceinline__ bool pair_table_hit(u64 dst, u64 dst_next, u32 total, u64 out_cap, int s) {
    return dst_next >= dst && dst_next - dst == (u64)total && dst <= out_cap && (u64)total <= out_cap - dst && (s > 0 || dst == 0);
}

// store: coalesced rowval / nzval stores of the dense records; the lane of a column writes its colptr (the columns' range is
// clamped: [c_lo, c_hi)), the last pair the closing one.  row_add makes the records' rows 1-based.  KEEP: the values alone
template <bool KEEP>
__device__ __forceinline__ void pair_store(const Args &a, const u32 *rows, const double *vals, i64 row_add, u64 dst, PairPlace pl, u64 hi,
                                           int ncl, int s, int t) {
    for (int p = t; p < (int)pl.total; p += THREADS) {
        if constexpr (!KEEP) a.out_row[dst + p] = (i64)rows[p] + row_add;
        a.out_val[dst + p] = vals[p];
    }
    if constexpr (!KEEP) {
        const i64 c_lo = (i64)(hi >> a.rb);
        const i64 c_hi = min(c_lo + (i64)ncl, a.col_end);
        if (c_lo + t < c_hi) a.colptr_out[c_lo + t] = (i64)(dst + pl.at0) + 1;
        if (s == a.S - 1 && t == 0) a.colptr_out[a.col_end] = (i64)(dst + pl.total) + 1;
    }
}

// grand total (the PREDICTED forms, stored by lane 0 of the last pair where the host reads it): lb_complete's last granule
__device__ __forceinline__ u64 pair_grand_total(u64 dst, u32 total) { return ST_PRE | ((dst + (u64)total) & ST_VAL); }

// the launchers' dispatch: f(std::integral_constant<int, KEYS>) for the 4-byte keys of one kind (keys 1 / 2); false: no such form
template <class F>
bool pair_for_keys(int keys, F f) {
    if (keys == 1) return f(std::integral_constant<int, 1>{}), true;
    if (keys == 2) return f(std::integral_constant<int, 2>{}), true;
    return false;
}

}  // namespace esplocal
