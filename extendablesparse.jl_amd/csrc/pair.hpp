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
    const int wu = __builtin_amdgcn_readfirstlane(w);  // (the wave's number: the same in its lanes, so `i < wu` is a scalar compare)
#pragma unroll
    for (int i = 0; i < WAVES; i++) {
        pl.at0 += i < wu ? lw[i] : 0u;
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
// clamped: [c_lo, c_hi)), the last pair the closing one.  row_add makes the records' rows 1-based.  KEEP: the values alone.
// A lane stores two consecutive records per round, 16 bytes to each array: where out_val + dst is no multiple of 16 bytes one
// record goes first by itself, and one follows where a record is left over -- the parity is the address's own, so every 16-byte
// store is aligned and the stores cover [dst, dst + total) exactly, as one record per lane did.  (rowval and nzval are both arrays
// of 8-byte elements: where their bases differ in parity -- no allocation of the handle's does -- a lane stores one record.)
template <bool KEEP>
__device__ __forceinline__ void pair_store(const Args &a, const u32 *rows, const double *vals, i64 row_add, u64 dst, PairPlace pl, u64 hi,
                                           int ncl, int s, int t) {
    typedef double dbl2 __attribute__((ext_vector_type(2)));
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    const int total = (int)pl.total;
    double *const ov = a.out_val + dst;
    i64 *orow = nullptr;  // (the values-only form never forms an address in rowval)
    bool wide = true;
    if constexpr (!KEEP) {
        orow = a.out_row + dst;
        wide = (((uintptr_t)ov ^ (uintptr_t)orow) & 8) == 0;
    }
    if (wide) {
        const int head = (int)(((uintptr_t)ov >> 3) & 1);  // (the first record does not start a 16-byte unit)
        if (t == 0 && head && total > 0) {
            if constexpr (!KEEP) orow[0] = (i64)rows[0] + row_add;
            ov[0] = vals[0];
        }
        const int npair = (total - head) >> 1;  // (total = 0, head = 1: -1, no round)
        for (int q = t; q < npair; q += THREADS) {
            const int p = head + 2 * q;  // p + 1 < total
            if constexpr (!KEEP) *reinterpret_cast<ll2 *>(orow + p) = ll2{(i64)rows[p] + row_add, (i64)rows[p + 1] + row_add};
            *reinterpret_cast<dbl2 *>(ov + p) = dbl2{vals[p], vals[p + 1]};
        }
        if (t == ESP_WAVE && total > head && ((total - head) & 1)) {  // (another wave than the head's)
            if constexpr (!KEEP) orow[total - 1] = (i64)rows[total - 1] + row_add;
            ov[total - 1] = vals[total - 1];
        }
    } else {
        for (int p = t; p < total; p += THREADS) {
            if constexpr (!KEEP) orow[p] = (i64)rows[p] + row_add;
            ov[p] = vals[p];
        }
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
