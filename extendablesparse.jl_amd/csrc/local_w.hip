// local_w.hip -- the PAIR form of the fresh-matrix bucket kernel: one workgroup takes TWO neighbouring producer buckets (at most
// 512 columns and 6144 entries) as one segment.
//
// local_k's small variant takes one bucket of 256 columns x 12 updates per workgroup (three workgroups per CU).  Its time follows
// the number of segments -- ticket, window fetch, seven barriers, look-back, launch and retirement cost a segment about 4-5 ns of
// chip time whatever it holds -- and half its waves idle in the register tier, where one lane takes one of the 256 columns.
// Here the producer's cut stays as it is and a segment is a pair of its buckets (Args::pair_buckets: the buckets of the table; the
// last pair of an odd count has one); an entry's bucket comes from its position (the producer writes the pair bucket by bucket).
//   load  : 12 entries per lane (4-byte keys of one kind + values, all 24 loads in flight); values to LDS; the pair's smallest and
//           largest row
//   count : counting sort by local column (bucket << cl_bits | column inside the bucket) with LDS atomics; one lane per column
//           scans the counts
//   sort  : 32-bit sort keys (row - smallest row) << 13 | slot go to LDS in column order -- 24 KiB where local_k keeps 8-byte
//           packed keys: 74 KiB of LDS in all, two workgroups per CU -- and one lane per column sorts its run (<= 12) with the
//           42-comparator network on u32 (v_min_u32 / v_max_u32): every lane of the workgroup has a column
//   fold  : the counts of emitted entries are scanned, the pair's total is published for the look-back, every lane folds its run
//           straight to its dense place in LDS (row, value) and writes its column's colptr itself
//   store : coalesced rowval / nzval stores
// A pair whose rows span 2^19 or more, or that has a column run of more than 12 entries, emits nothing and raises PAIR_REFUSED in
// Args::err: the host runs the flush again with local_k, which rewrites everything a fresh-matrix flush writes.
//
// Two kernels share the body below: pair_k (ticket, window of bounds, look-back) and pair_pred_k, the PREDICTED form of a flush
// that repeats the plan of the handle's last one -- see there.
#include "local.hpp"

namespace esplocal {

namespace {
constexpr int P_CAP = THREADS * PAIR_ITEMS;  // 6144 entries per pair
constexpr int P_SLOT_BITS = 13;               // slot index of an entry inside the pair
constexpr u32 P_SLOT_MASK = (1u << P_SLOT_BITS) - 1u;
constexpr int P_ROW_BITS = 32 - P_SLOT_BITS;  // rows of a pair must span less than 2^19
static_assert(P_CAP <= (1 << P_SLOT_BITS), "the slot index covers the pair");
static_assert(NetOf<PAIR_RUN>::net.n == 42, "the 12-input network");
}  // namespace

template <int KEYS>
__global__ __launch_bounds__(THREADS, 4) void pair_k(Args a) {
    static_assert(KEYS == 1 || KEYS == 2, "4-byte keys of one kind");
    constexpr bool UPD = KEYS == 2;
    constexpr int NI = PAIR_ITEMS, R = PAIR_RUN;
    __shared__ u32 skey[P_CAP];     // sort keys in column order; then the records' rows
    __shared__ double sval[P_CAP];  // values by slot; then the records' values
    __shared__ u32 ccnt[THREADS];   // entries per local column, then where its run starts
    __shared__ u32 lw[2 * WAVES];
    __shared__ u64 s_dst;
    __shared__ int s_seg;
    __shared__ u32 s_rmin, s_rmax;
    constexpr int WIN = 32;  // pairs around the expected ticket whose bounds are fetched while the ticket is in flight
    __shared__ i64 s_win[2 * WIN + 3];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const i64 nb = a.pair_buckets;
    const i64 w0 = max((i64)0, a.first + (i64)blockIdx.x - WIN / 2);
    if (t <= 2 * WIN + 2) s_win[t] = a.seg_start[min(2 * w0 + t, nb)];
    if (t == 0) {
        s_seg = (int)atomicAdd(a.ticket, 1u);
        s_rmin = ~0u;
        s_rmax = 0u;
    }
    ccnt[t] = 0;
    __syncthreads();
    const int s = esp_uniform_i32(s_seg);
    if (s >= a.S) return;
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 0] = wall_clock64();
#endif
    const bool inwin = s >= w0 && (i64)s - w0 <= WIN;
    const int o = 2 * (int)((i64)s - w0);
    const i64 b0 = 2 * (i64)s;
    const i64 beg = esp_uniform_i64(inwin ? s_win[o] : a.seg_start[b0]);
    const i64 mid = esp_uniform_i64(inwin ? s_win[o + 1] : a.seg_start[min(b0 + 1, nb)]);
    const i64 seg_end = esp_uniform_i64(inwin ? s_win[o + 2] : a.seg_start[min(b0 + 2, nb)]);
    const int n = (int)min(seg_end - beg, (i64)P_CAP);
    const u32 split = (u32)(mid - beg);  // positions from here on belong to the pair's second bucket
    if (a.total >= 0 && s == a.S - 1 && seg_end != a.total && t == 0) atomicOr(a.err, 2u);  // (an entry behind the last column)
    const int cb = a.cl_bits;  // column bits of ONE bucket
    const int ncl = 2 << cb;
    const u64 hi = ((u64)s << (a.rem_bits + 1)) + a.base;  // the pair's prefix: that of its first bucket
    const u32 rowmask32 = (1u << a.rb) - 1u;                // (rb < 32: the host's condition)
    const int wbase = w * (NI * ESP_WAVE) + lane;
    // all 24 loads of a lane in flight, indices clamped (slots past the end re-read the last entry and are discarded)
    const i64 lbeg = n > 0 ? beg : max(beg - 1, (i64)0);
    const int nlast = n > 0 ? n - 1 : 0;
    u32 k[NI];
    double v[NI];
    {
        const u32 *k32 = reinterpret_cast<const u32 *>(a.keys_in);
#pragma unroll
        for (int i = 0; i < NI; i++) k[i] = k32[lbeg + min(wbase + i * ESP_WAVE, nlast)];
#pragma unroll
        for (int i = 0; i < NI; i++) v[i] = a.vals_in[lbeg + min(wbase + i * ESP_WAVE, nlast)];
    }
    auto local_col = [&](u32 key, int p) -> u32 {
        return min((((u32)p >= split ? 1u : 0u) << cb) | (key >> a.rb), (u32)(ncl - 1));
    };
    {
        u32 rmin = ~0u, rmax = 0u;
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int p = wbase + i * ESP_WAVE;
            sval[p] = v[i];
            if (p < n) {
                const u32 row = k[i] & rowmask32;
                rmin = min(rmin, row);
                rmax = max(rmax, row);
            }
        }
        rmin = ~esp_wave_max(~rmin);
        rmax = esp_wave_max(rmax);
        if (lane == 0 && n > 0) {
            atomicMin(&s_rmin, rmin);
            atomicMax(&s_rmax, rmax);
        }
    }
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 1] = wall_clock64();
#endif
    // ---- counting sort by local column
    unsigned short slot[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int p = wbase + i * ESP_WAVE;
        slot[i] = 0;
        if (p < n) slot[i] = (unsigned short)atomicAdd(&ccnt[local_col(k[i], p)], 1u);
    }
    __syncthreads();
    // one lane per local column: exclusive scan of the counts + the longest run
    const u32 cnt = ccnt[t];
    u32 rs = 0, maxrun = 0;
    {
        const u32 inc = esp_wave_scan_add(cnt);
        const u32 mx = esp_wave_max(cnt);
        if (lane == 63) lw[w] = inc;
        if (lane == 0) lw[WAVES + w] = mx;
        __syncthreads();
        rs = inc - cnt;
#pragma unroll
        for (int i = 0; i < WAVES; i++) {
            rs += i < w ? lw[i] : 0u;
            maxrun = max(maxrun, lw[WAVES + i]);
        }
        ccnt[t] = rs;
    }
    const u32 rmin = s_rmin;
    const bool fits = n == 0 || (maxrun <= (u32)R && s_rmax - rmin < (1u << P_ROW_BITS) && seg_end - beg <= (i64)P_CAP);
    if (!fits && t == 0) atomicOr(a.err, PAIR_REFUSED);
    __syncthreads();  // (ccnt: the run starts)
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 2] = wall_clock64();
#endif
    if (fits) {
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int p = wbase + i * ESP_WAVE;
            if (p < n) skey[ccnt[local_col(k[i], p)] + slot[i]] = (((k[i] & rowmask32) - rmin) << P_SLOT_BITS) | (u32)p;
        }
    }
    __syncthreads();
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 3] = wall_clock64();
#endif
    // ---- one lane per column: the run in registers, sorted by (row, slot) -- the slot is the append order
    const int len = fits ? (int)cnt : 0;
    u32 x[R];
    double xv[R];
#pragma unroll
    for (int j = 0; j < R; j++) x[j] = ~0u;
    if (len > 0) {
#pragma unroll
        for (int j = 0; j < R; j++) x[j] = j < len ? skey[rs + j] : ~0u;
#pragma unroll
        for (int q = 0; q < NetOf<R>::net.n; q++) {
            const u32 lo = x[NetOf<R>::net.a[q]], hh = x[NetOf<R>::net.b[q]];
            x[NetOf<R>::net.a[q]] = min(lo, hh);
            x[NetOf<R>::net.b[q]] = max(lo, hh);
        }
    }
#pragma unroll
    for (int j = 0; j < R; j++) xv[j] = sval[j < len ? (x[j] & P_SLOT_MASK) : 0u];
    // entries the run emits: one per row that one of its updates creates (fold_step: a RAWUPDATE / COO entry or a non-zero value)
    u32 ec = 0;
    {
        bool any = false;
        u32 prow = 0;
#pragma unroll
        for (int j = 0; j <= R; j++) {
            const bool valid = j < R && j < len;
            const u32 row = (j < R ? x[j] : ~0u) >> P_SLOT_BITS;
            const bool fresh = j == 0 || !valid || row != prow;
            if (fresh && j > 0 && j <= len) ec += any ? 1u : 0u;
            if (valid) {
                if (fresh) {
                    prow = row;
                    any = false;
                }
                if constexpr (UPD)
                    any |= xv[j < R ? j : 0] != 0.0;
                else
                    any |= a.kind32 >= (u32)ESP_RAWUPDATE || xv[j < R ? j : 0] != 0.0;
            }
        }
    }
    const u32 einc = esp_wave_scan_add(ec);
    if (lane == 63) lw[w] = einc;
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 8] = wall_clock64();
#endif
    __syncthreads();  // (every lane holds its run in registers: skey / sval are free for the records)
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 9] = wall_clock64();
#endif
    u32 at0 = einc - ec, total = 0;
#pragma unroll
    for (int i = 0; i < WAVES; i++) {
        at0 += i < w ? lw[i] : 0u;
        total += lw[i];
    }
    LbState lbs;
    lb_init(lbs, 0);
    // (the publication is one store: the last wave folds its columns like the others and resolves the chain behind its fold)
    if (w == WAVES - 1) lb_publish(a, lbs, s, total, lane);
    // ---- ordered fold of the run straight to the dense records (row, value)
    if (len > 0) {
        u32 at = at0;
        bool present = false;
        double acc = 0.0;
        u32 prow = 0;
#pragma unroll
        for (int j = 0; j <= R; j++) {
            const bool valid = j < R && j < len;
            const u32 row = (j < R ? x[j] : ~0u) >> P_SLOT_BITS;
            const bool fresh = j == 0 || !valid || row != prow;
            if (fresh && j > 0 && j <= len && present) {
                skey[at] = prow + rmin;
                sval[at] = acc;
                at++;
            }
            if (fresh) {
                prow = row;
                present = false;
                acc = 0.0;
            }
            if (valid) {
                if constexpr (UPD)
                    espfold::fold_step_update(present, acc, xv[j < R ? j : 0]);
                else
                    espfold::fold_step_sel(present, acc, a.kind32, xv[j < R ? j : 0]);
            }
        }
    }
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 10] = wall_clock64();
#endif
    if (w == WAVES - 1) {
        const u64 excl = lb_complete(a, lbs, s, total, lane);
        if (lane == 0) s_dst = excl;
#ifdef ESP_LOCAL_STAMPS
        if (a.stamps && lane == 0) a.stamps[(size_t)s * 16 + 11] = wall_clock64();
#endif
    }
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 4] = wall_clock64();
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 5] = wall_clock64();
#endif
    __syncthreads();
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 6] = wall_clock64();
#endif
    if (!fits) return;  // (the flush runs again with local_k)
    const u64 dst = esp_uniform_u64(s_dst);
    // ---- coalesced stores; the lane of a column writes its colptr (the columns' range is clamped: [c_lo, c_hi))
    for (int p = t; p < (int)total; p += THREADS) {
        a.out_row[dst + p] = (i64)skey[p] + 1;
        a.out_val[dst + p] = sval[p];
    }
    const i64 c_lo = (i64)(hi >> a.rb);
    const i64 c_hi = min(c_lo + (i64)ncl, a.col_end);
    if (c_lo + t < c_hi) a.colptr_out[c_lo + t] = (i64)(dst + at0) + 1;
    if (s == a.S - 1 && t == 0) a.colptr_out[a.col_end] = (i64)(dst + total) + 1;
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 7] = wall_clock64();
#endif
}

// The PREDICTED form: a flush that repeats the producer plan of the handle's last flush (esp_handle::PredTable).  pair_k's
// phases, but the segment is the workgroup's number and its place is pred[s]: no ticket, no window of bounds, no look-back --
// nothing here waits for another workgroup, so the order in which workgroups start does not matter.  A pair that emits another
// count than pred[s + 1] - pred[s] raises PRED_MISS and stores nothing; when no pair did, every place was the exclusive prefix sum
// of the true counts and the output is pair_k's byte for byte.  Stamps as in pair_k (none at 11: there is no look-back).
template <int KEYS>
__global__ __launch_bounds__(THREADS, 4) void pair_pred_k(Args a, const u64 *pred, u64 out_cap) {
    static_assert(KEYS == 1 || KEYS == 2, "4-byte keys of one kind");
    constexpr bool UPD = KEYS == 2;
    constexpr int NI = PAIR_ITEMS, R = PAIR_RUN;
    __shared__ u32 skey[P_CAP];     // sort keys in column order; then the records' rows
    __shared__ double sval[P_CAP];  // values by slot; then the records' values
    __shared__ u32 ccnt[THREADS];   // entries per local column, then where its run starts
    __shared__ u32 lw[2 * WAVES];
    __shared__ u32 s_rmin, s_rmax;

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const i64 nb = a.pair_buckets;
    // the segment is the workgroup's number; its bounds and its place come back in one round trip (uniform loads)
    const int s = (int)(a.first + (i64)blockIdx.x);
    if (s >= a.S) return;
    const i64 b0 = 2 * (i64)s;
    const i64 beg = esp_uniform_i64(a.seg_start[b0]);
    const i64 mid = esp_uniform_i64(a.seg_start[min(b0 + 1, nb)]);
    const i64 seg_end = esp_uniform_i64(a.seg_start[min(b0 + 2, nb)]);
    const u64 dst = esp_uniform_u64(pred[s]);
    const u64 dst_next = esp_uniform_u64(pred[s + 1]);
    if (t == 0) {
        s_rmin = ~0u;
        s_rmax = 0u;
    }
    ccnt[t] = 0;
    __syncthreads();
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 0] = wall_clock64();
#endif
    const int n = (int)min(seg_end - beg, (i64)P_CAP);
    const u32 split = (u32)(mid - beg);  // positions from here on belong to the pair's second bucket
    if (a.total >= 0 && s == a.S - 1 && seg_end != a.total && t == 0) atomicOr(a.err, 2u);  // (an entry behind the last column)
    const int cb = a.cl_bits;  // column bits of ONE bucket
    const int ncl = 2 << cb;
    const u64 hi = ((u64)s << (a.rem_bits + 1)) + a.base;  // the pair's prefix: that of its first bucket
    const u32 rowmask32 = (1u << a.rb) - 1u;                // (rb < 32: the host's condition)
    const int wbase = w * (NI * ESP_WAVE) + lane;
    // all 24 loads of a lane in flight, indices clamped (slots past the end re-read the last entry and are discarded)
    const i64 lbeg = n > 0 ? beg : max(beg - 1, (i64)0);
    const int nlast = n > 0 ? n - 1 : 0;
    u32 k[NI];
    double v[NI];
    {
        const u32 *k32 = reinterpret_cast<const u32 *>(a.keys_in);
#pragma unroll
        for (int i = 0; i < NI; i++) k[i] = k32[lbeg + min(wbase + i * ESP_WAVE, nlast)];
#pragma unroll
        for (int i = 0; i < NI; i++) v[i] = a.vals_in[lbeg + min(wbase + i * ESP_WAVE, nlast)];
    }
    auto local_col = [&](u32 key, int p) -> u32 {
        return min((((u32)p >= split ? 1u : 0u) << cb) | (key >> a.rb), (u32)(ncl - 1));
    };
    {
        u32 rmin = ~0u, rmax = 0u;
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int p = wbase + i * ESP_WAVE;
            sval[p] = v[i];
            if (p < n) {
                const u32 row = k[i] & rowmask32;
                rmin = min(rmin, row);
                rmax = max(rmax, row);
            }
        }
        rmin = ~esp_wave_max(~rmin);
        rmax = esp_wave_max(rmax);
        if (lane == 0 && n > 0) {
            atomicMin(&s_rmin, rmin);
            atomicMax(&s_rmax, rmax);
        }
    }
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 1] = wall_clock64();
#endif
    // ---- counting sort by local column
    unsigned short slot[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int p = wbase + i * ESP_WAVE;
        slot[i] = 0;
        if (p < n) slot[i] = (unsigned short)atomicAdd(&ccnt[local_col(k[i], p)], 1u);
    }
    __syncthreads();
    // one lane per local column: exclusive scan of the counts + the longest run
    const u32 cnt = ccnt[t];
    u32 rs = 0, maxrun = 0;
    {
        const u32 inc = esp_wave_scan_add(cnt);
        const u32 mx = esp_wave_max(cnt);
        if (lane == 63) lw[w] = inc;
        if (lane == 0) lw[WAVES + w] = mx;
        __syncthreads();
        rs = inc - cnt;
#pragma unroll
        for (int i = 0; i < WAVES; i++) {
            rs += i < w ? lw[i] : 0u;
            maxrun = max(maxrun, lw[WAVES + i]);
        }
        ccnt[t] = rs;
    }
    const u32 rmin = s_rmin;
    const bool fits = n == 0 || (maxrun <= (u32)R && s_rmax - rmin < (1u << P_ROW_BITS) && seg_end - beg <= (i64)P_CAP);
    if (!fits && t == 0) atomicOr(a.err, PAIR_REFUSED);
    __syncthreads();  // (ccnt: the run starts)
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 2] = wall_clock64();
#endif
    if (fits) {
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int p = wbase + i * ESP_WAVE;
            if (p < n) skey[ccnt[local_col(k[i], p)] + slot[i]] = (((k[i] & rowmask32) - rmin) << P_SLOT_BITS) | (u32)p;
        }
    }
    __syncthreads();
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 3] = wall_clock64();
#endif
    // ---- one lane per column: the run in registers, sorted by (row, slot) -- the slot is the append order
    const int len = fits ? (int)cnt : 0;
    u32 x[R];
    double xv[R];
#pragma unroll
    for (int j = 0; j < R; j++) x[j] = ~0u;
    if (len > 0) {
#pragma unroll
        for (int j = 0; j < R; j++) x[j] = j < len ? skey[rs + j] : ~0u;
#pragma unroll
        for (int q = 0; q < NetOf<R>::net.n; q++) {
            const u32 lo = x[NetOf<R>::net.a[q]], hh = x[NetOf<R>::net.b[q]];
            x[NetOf<R>::net.a[q]] = min(lo, hh);
            x[NetOf<R>::net.b[q]] = max(lo, hh);
        }
    }
#pragma unroll
    for (int j = 0; j < R; j++) xv[j] = sval[j < len ? (x[j] & P_SLOT_MASK) : 0u];
    // entries the run emits: one per row that one of its updates creates (fold_step: a RAWUPDATE / COO entry or a non-zero value)
    u32 ec = 0;
    {
        bool any = false;
        u32 prow = 0;
#pragma unroll
        for (int j = 0; j <= R; j++) {
            const bool valid = j < R && j < len;
            const u32 row = (j < R ? x[j] : ~0u) >> P_SLOT_BITS;
            const bool fresh = j == 0 || !valid || row != prow;
            if (fresh && j > 0 && j <= len) ec += any ? 1u : 0u;
            if (valid) {
                if (fresh) {
                    prow = row;
                    any = false;
                }
                if constexpr (UPD)
                    any |= xv[j < R ? j : 0] != 0.0;
                else
                    any |= a.kind32 >= (u32)ESP_RAWUPDATE || xv[j < R ? j : 0] != 0.0;
            }
        }
    }
    const u32 einc = esp_wave_scan_add(ec);
    if (lane == 63) lw[w] = einc;
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 8] = wall_clock64();
#endif
    __syncthreads();  // (every lane holds its run in registers: skey / sval are free for the records)
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 9] = wall_clock64();
#endif
    u32 at0 = einc - ec, total = 0;
#pragma unroll
    for (int i = 0; i < WAVES; i++) {
        at0 += i < w ? lw[i] : 0u;
        total += lw[i];
    }
    // the pair's place is the table's when it emits what the table says -- pred[0] = 0 and every pair's count right: the table
    // is the exclusive prefix sum the look-back would resolve -- and ends inside the output arrays; else nothing is stored (the
    // same answer in every lane: total comes from LDS)
    const bool hit = dst_next >= dst && dst_next - dst == (u64)total && dst <= out_cap && (u64)total <= out_cap - dst && (s > 0 || dst == 0);
    if (!hit) {
        if (t == 0) atomicOr(a.err, PRED_MISS);
        return;
    }
    // ---- ordered fold of the run straight to the dense records (row, value)
    if (len > 0) {
        u32 at = at0;
        bool present = false;
        double acc = 0.0;
        u32 prow = 0;
#pragma unroll
        for (int j = 0; j <= R; j++) {
            const bool valid = j < R && j < len;
            const u32 row = (j < R ? x[j] : ~0u) >> P_SLOT_BITS;
            const bool fresh = j == 0 || !valid || row != prow;
            if (fresh && j > 0 && j <= len && present) {
                skey[at] = prow + rmin;
                sval[at] = acc;
                at++;
            }
            if (fresh) {
                prow = row;
                present = false;
                acc = 0.0;
            }
            if (valid) {
                if constexpr (UPD)
                    espfold::fold_step_update(present, acc, xv[j < R ? j : 0]);
                else
                    espfold::fold_step_sel(present, acc, a.kind32, xv[j < R ? j : 0]);
            }
        }
    }
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 10] = wall_clock64();
#endif
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 4] = wall_clock64();
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 5] = wall_clock64();
#endif
    __syncthreads();
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 6] = wall_clock64();
#endif
    if (!fits) return;  // (the flush runs again with pair_k, then local_k)
    // ---- coalesced stores; the lane of a column writes its colptr (the columns' range is clamped: [c_lo, c_hi))
    for (int p = t; p < (int)total; p += THREADS) {
        a.out_row[dst + p] = (i64)skey[p] + 1;
        a.out_val[dst + p] = sval[p];
    }
    const i64 c_lo = (i64)(hi >> a.rb);
    const i64 c_hi = min(c_lo + (i64)ncl, a.col_end);
    if (c_lo + t < c_hi) a.colptr_out[c_lo + t] = (i64)(dst + at0) + 1;
    if (s == a.S - 1 && t == 0) {
        a.colptr_out[a.col_end] = (i64)(dst + total) + 1;
        a.status[s] = ST_PRE | ((dst + (u64)total) & ST_VAL);  // (the grand total where the host reads it: lb_complete's last granule)
    }
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && t == 0) a.stamps[(size_t)s * 16 + 7] = wall_clock64();
#endif
}

__global__ __launch_bounds__(256) void pair_record_k(const i64 *__restrict__ colptr, i64 col_end, int ncl_bits, int Sp, u64 *__restrict__ pred) {
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s > Sp) return;
    pred[s] = (u64)(colptr[s < Sp ? min((i64)s << ncl_bits, col_end) : col_end] - 1);
}

void launch_pair_record(hipStream_t stream, const i64 *colptr, i64 col_end, int ncl_bits, int Sp, u64 *pred) {
    hipLaunchKernelGGL(pair_record_k, dim3((unsigned)(Sp / 256 + 1)), dim3(256), 0, stream, colptr, col_end, ncl_bits, Sp, pred);
}

bool launch_pair_predicted(const Variant &v, unsigned grid, hipStream_t stream, const Args &a, const u64 *pred, u64 out_cap) {
    if (!v.fresh || v.pieces) return false;
    if (v.keys == 1) {
        hipLaunchKernelGGL((pair_pred_k<1>), dim3(grid), dim3(THREADS), 0, stream, a, pred, out_cap);
        return true;
    }
    if (v.keys == 2) {
        hipLaunchKernelGGL((pair_pred_k<2>), dim3(grid), dim3(THREADS), 0, stream, a, pred, out_cap);
        return true;
    }
    return false;
}

bool launch_pair(const Variant &v, unsigned grid, hipStream_t stream, const Args &a) {
    if (!v.fresh || v.pieces) return false;
    if (v.keys == 1) {
        hipLaunchKernelGGL((pair_k<1>), dim3(grid), dim3(THREADS), 0, stream, a);
        return true;
    }
    if (v.keys == 2) {
        hipLaunchKernelGGL((pair_k<2>), dim3(grid), dim3(THREADS), 0, stream, a);
        return true;
    }
    return false;
}

}  // namespace esplocal
