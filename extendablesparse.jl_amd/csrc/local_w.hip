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
// Every phase is one function: those below (pair_open .. pair_fold) and, shared with pair_gen_pred_k (local_x.hip), those of
// pair.hpp (pair_place, pair_table_hit, pair_store, pair_grand_total).  Two kernels call them in the same order: pair_k (ticket,
// window of bounds, look-back) and pair_pred_k, the PREDICTED form of a flush that repeats the plan of the handle's last one.
// What a kernel spells out itself is what the two do differently: how the pair is claimed, how it learns its place in the
// output, and its LDS.
#include "local.hpp"
#include "pair.hpp"

namespace esplocal {

namespace {
constexpr int NI = PAIR_ITEMS, R = PAIR_RUN;
constexpr int P_CAP = THREADS * NI;  // 6144 entries per pair
constexpr int P_SLOT_BITS = 13;      // slot index of an entry inside the pair
constexpr u32 P_SLOT_MASK = (1u << P_SLOT_BITS) - 1u;
constexpr int P_ROW_BITS = 32 - P_SLOT_BITS;  // rows of a pair must span less than 2^19
static_assert(P_CAP <= (1 << P_SLOT_BITS), "the slot index covers the pair");
static_assert(NetOf<R>::net.n == 42, "the 12-input network");

// diagnostics (builds with -DESP_LOCAL_STAMPS only): wall-clock stamp i of segment s
__device__ __forceinline__ void pair_stamp(const Args &a, int s, int i, bool on) {
#ifdef ESP_LOCAL_STAMPS
    if (a.stamps && on) a.stamps[(size_t)s * 16 + i] = wall_clock64();
#endif
}

// a claimed pair: its entries [beg, seg_end) and what the flush's layout makes of them -- the same in every lane but wbase
struct Pair {
    i64 beg, seg_end;
    int n;          // entries taken (a pair of more than P_CAP is refused)
    u32 split;      // positions from here on belong to the pair's second bucket
    int rb, cb;     // row bits; column bits of ONE bucket
    int ncl;        // local columns of the pair
    u64 hi;         // the pair's prefix: that of its first bucket
    u32 rowmask32;  // (rb < 32: the host's condition)
    int wbase;      // the lane's first position; its i-th is wbase + i * ESP_WAVE
    __device__ __forceinline__ u32 local_col(u32 key, int p) const {
        return min((((u32)p >= split ? 1u : 0u) << cb) | (key >> rb), (u32)(ncl - 1));
    }
};
__device__ __forceinline__ Pair pair_open(const Args &a, int s, i64 beg, i64 mid, i64 seg_end, int t) {
    if (a.total >= 0 && s == a.S - 1 && seg_end != a.total && t == 0) atomicOr(a.err, 2u);  // (an entry behind the last column)
    return Pair{beg, seg_end, (int)min(seg_end - beg, (i64)P_CAP), (u32)(mid - beg), a.rb, a.cl_bits, 2 << a.cl_bits,
                ((u64)s << (a.rem_bits + 1)) + a.base, (1u << a.rb) - 1u, (t >> 6) * (NI * ESP_WAVE) + (t & 63)};
}

// load: all 24 loads of a lane in flight, indices clamped (slots past the end re-read the last entry and are discarded); values
// to LDS by slot; the pair's smallest and largest row to s_rmin / s_rmax (initialised by the kernel before its first barrier)
__device__ __forceinline__ void pair_load(const Args &a, const Pair &pr, int lane, u32 (&k)[NI], double *sval, u32 *s_rmin, u32 *s_rmax) {
    const int n = pr.n;
    const i64 lbeg = n > 0 ? pr.beg : max(pr.beg - 1, (i64)0);
    const int nlast = n > 0 ? n - 1 : 0;
    double v[NI];
    const u32 *k32 = reinterpret_cast<const u32 *>(a.keys_in);
#pragma unroll
    for (int i = 0; i < NI; i++) k[i] = k32[lbeg + min(pr.wbase + i * ESP_WAVE, nlast)];
#pragma unroll
    for (int i = 0; i < NI; i++) v[i] = a.vals_in[lbeg + min(pr.wbase + i * ESP_WAVE, nlast)];
    u32 rmin = ~0u, rmax = 0u;
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int p = pr.wbase + i * ESP_WAVE;
        sval[p] = v[i];
        if (p < n) {
            const u32 row = k[i] & pr.rowmask32;
            rmin = min(rmin, row);
            rmax = max(rmax, row);
        }
    }
    rmin = ~esp_wave_max(~rmin);
    rmax = esp_wave_max(rmax);
    if (lane == 0 && n > 0) {
        atomicMin(s_rmin, rmin);
        atomicMax(s_rmax, rmax);
    }
}

// count: counting sort by local column with LDS atomics (slot: the entry's arrival number in its column); then one lane per local
// column: exclusive scan of the counts into ccnt (the caller's next barrier publishes them) and the longest run.  A pair that does
// not fit raises PAIR_REFUSED and has runs of length 0.  Two barriers
struct PairRun {
    u32 rs;    // where the lane's column starts in skey
    int len;   // its entries (0 in a refused pair)
    u32 rmin;  // the pair's smallest row
    bool fits;
};
__device__ __forceinline__ PairRun pair_count(const Args &a, const Pair &pr, int t, const u32 (&k)[NI], unsigned short (&slot)[NI], u32 *ccnt,
                                              u32 *lw, const u32 *s_rmin, const u32 *s_rmax) {
    const int lane = t & 63, w = t >> 6;
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int p = pr.wbase + i * ESP_WAVE;
        slot[i] = 0;
        if (p < pr.n) slot[i] = (unsigned short)atomicAdd(&ccnt[pr.local_col(k[i], p)], 1u);
    }
    __syncthreads();
    const u32 cnt = ccnt[t];
    const u32 inc = esp_wave_scan_add(cnt);
    const u32 mx = esp_wave_max(cnt);
    if (lane == 63) lw[w] = inc;
    if (lane == 0) lw[WAVES + w] = mx;
    __syncthreads();
    u32 rs = inc - cnt, maxrun = 0;
#pragma unroll
    for (int i = 0; i < WAVES; i++) {
        rs += i < w ? lw[i] : 0u;
        maxrun = max(maxrun, lw[WAVES + i]);
    }
    ccnt[t] = rs;
    const u32 rmin = *s_rmin;
    const bool fits = pr.n == 0 || (maxrun <= (u32)R && *s_rmax - rmin < (1u << P_ROW_BITS) && pr.seg_end - pr.beg <= (i64)P_CAP);
    if (!fits && t == 0) atomicOr(a.err, PAIR_REFUSED);
    return PairRun{rs, fits ? (int)cnt : 0, rmin, fits};
}

// scatter: the 32-bit sort keys (row - smallest row) << 13 | slot go to LDS in column order
__device__ __forceinline__ void pair_scatter(const Pair &pr, const PairRun &run, const u32 (&k)[NI], const unsigned short (&slot)[NI],
                                             const u32 *ccnt, u32 *skey) {
    if (!run.fits) return;
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int p = pr.wbase + i * ESP_WAVE;
        if (p < pr.n) skey[ccnt[pr.local_col(k[i], p)] + slot[i]] = (((k[i] & pr.rowmask32) - run.rmin) << P_SLOT_BITS) | (u32)p;
    }
}

// sort: one lane per column: the run in registers, sorted by (row, slot) -- the slot is the append order -- and its values
__device__ __forceinline__ void pair_sort_run(const PairRun &run, const u32 *skey, const double *sval, u32 (&x)[R], double (&xv)[R]) {
    const int len = run.len;
#pragma unroll
    for (int j = 0; j < R; j++) x[j] = ~0u;
    if (len > 0) {
#pragma unroll
        for (int j = 0; j < R; j++) x[j] = j < len ? skey[run.rs + j] : ~0u;
#pragma unroll
        for (int q = 0; q < NetOf<R>::net.n; q++) {
            const u32 lo = x[NetOf<R>::net.a[q]], hh = x[NetOf<R>::net.b[q]];
            x[NetOf<R>::net.a[q]] = min(lo, hh);
            x[NetOf<R>::net.b[q]] = max(lo, hh);
        }
    }
#pragma unroll
    for (int j = 0; j < R; j++) xv[j] = sval[j < len ? (x[j] & P_SLOT_MASK) : 0u];
}

// emitted: entries the run emits: one per row that one of its updates creates (fold_step: a RAWUPDATE / COO entry or a non-zero
// value)
template <int KEYS>
__device__ __forceinline__ u32 pair_emitted(const Args &a, int len, const u32 (&x)[R], const double (&xv)[R]) {
    u32 ec = 0;
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
            if constexpr (KEYS == 2)
                any |= xv[j < R ? j : 0] != 0.0;
            else
                any |= a.kind32 >= (u32)ESP_RAWUPDATE || xv[j < R ? j : 0] != 0.0;
        }
    }
    return ec;
}

// fold: ordered fold of the run straight to the dense records (row, value) from place `at` on: skey / sval are free for them
// behind pair_place's barrier
template <int KEYS>
__device__ __forceinline__ void pair_fold(const Args &a, const PairRun &run, const u32 (&x)[R], const double (&xv)[R], u32 at, u32 *skey,
                                          double *sval) {
    const int len = run.len;
    if (len <= 0) return;
    bool present = false;
    double acc = 0.0;
    u32 prow = 0;
#pragma unroll
    for (int j = 0; j <= R; j++) {
        const bool valid = j < R && j < len;
        const u32 row = (j < R ? x[j] : ~0u) >> P_SLOT_BITS;
        const bool fresh = j == 0 || !valid || row != prow;
        if (fresh && j > 0 && j <= len && present) {
            skey[at] = prow + run.rmin;
            sval[at] = acc;
            at++;
        }
        if (fresh) {
            prow = row;
            present = false;
            acc = 0.0;
        }
        if (valid) {
            if constexpr (KEYS == 2)
                espfold::fold_step_update(present, acc, xv[j < R ? j : 0]);
            else
                espfold::fold_step_sel(present, acc, a.kind32, xv[j < R ? j : 0]);
        }
    }
}
}  // namespace

template <int KEYS>
__global__ __launch_bounds__(THREADS, 4) void pair_k(Args a) {
    static_assert(KEYS == 1 || KEYS == 2, "4-byte keys of one kind");
    __shared__ u32 skey[P_CAP];     // sort keys in column order; then the records' rows
    __shared__ double sval[P_CAP];  // values by slot; then the records' values
    __shared__ u32 ccnt[THREADS];   // entries per local column, then where its run starts
    __shared__ u32 lw[2 * WAVES];
    __shared__ u64 s_dst;
    __shared__ int s_seg;
    __shared__ u32 s_rmin, s_rmax;
    constexpr int WIN = 32;  // pairs around the expected ticket whose bounds are fetched while the ticket is in flight
    __shared__ i64 s_win[2 * WIN + 3];

    // ---- claim: a ticket; the bounds come from the window fetched while it was in flight
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
    pair_stamp(a, s, 0, t == 0);
    const bool inwin = s >= w0 && (i64)s - w0 <= WIN;
    const int o = 2 * (int)((i64)s - w0);
    const i64 b0 = 2 * (i64)s;
    const i64 beg = esp_uniform_i64(inwin ? s_win[o] : a.seg_start[b0]);
    const i64 mid = esp_uniform_i64(inwin ? s_win[o + 1] : a.seg_start[min(b0 + 1, nb)]);
    const i64 seg_end = esp_uniform_i64(inwin ? s_win[o + 2] : a.seg_start[min(b0 + 2, nb)]);
    const Pair pr = pair_open(a, s, beg, mid, seg_end, t);
    // ---- the run of the lane's column, sorted, and what it emits
    u32 k[NI];
    unsigned short slot[NI];
    pair_load(a, pr, lane, k, sval, &s_rmin, &s_rmax);
    pair_stamp(a, s, 1, t == 0);
    const PairRun run = pair_count(a, pr, t, k, slot, ccnt, lw, &s_rmin, &s_rmax);
    __syncthreads();  // (ccnt: the run starts)
    pair_stamp(a, s, 2, t == 0);
    pair_scatter(pr, run, k, slot, ccnt, skey);
    __syncthreads();
    pair_stamp(a, s, 3, t == 0);
    u32 x[R];
    double xv[R];
    pair_sort_run(run, skey, sval, x, xv);
    const u32 ec = pair_emitted<KEYS>(a, run.len, x, xv);
    pair_stamp(a, s, 8, t == 0);
    const PairPlace pl = pair_place(ec, lw, lane, w);
    pair_stamp(a, s, 9, t == 0);
    // ---- place: the look-back.  The publication is one store: the last wave folds its columns like the others and resolves the
    // chain behind its fold
    LbState lbs;
    lb_init(lbs, 0);
    if (w == WAVES - 1) lb_publish(a, lbs, s, pl.total, lane);
    pair_fold<KEYS>(a, run, x, xv, pl.at0, skey, sval);
    pair_stamp(a, s, 10, t == 0);
    if (w == WAVES - 1) {
        const u64 excl = lb_complete(a, lbs, s, pl.total, lane);
        if (lane == 0) s_dst = excl;
        pair_stamp(a, s, 11, lane == 0);
    }
    pair_stamp(a, s, 4, t == 0);
    pair_stamp(a, s, 5, t == 0);
    __syncthreads();
    pair_stamp(a, s, 6, t == 0);
    if (!run.fits) return;  // (the flush runs again with local_k)
    const u64 dst = esp_uniform_u64(s_dst);
    pair_store<false>(a, skey, sval, 1, dst, pl, pr.hi, pr.ncl, s, t);
    pair_stamp(a, s, 7, t == 0);
}

// The PREDICTED form: a flush that repeats the producer plan of the handle's last flush (esp_handle::PredTable).  pair_k's
// phases, but the segment is the workgroup's number and its place is pred[s]: no ticket, no window of bounds, no look-back --
// nothing here waits for another workgroup, so the order in which workgroups start does not matter.  A pair that emits another
// count than pred[s + 1] - pred[s] raises PRED_MISS and stores nothing; when no pair did, every place was the exclusive prefix sum
// of the true counts and the output is pair_k's byte for byte.  Stamps as in pair_k (none at 11: there is no look-back).
template <int KEYS>
__global__ __launch_bounds__(THREADS, 4) void pair_pred_k(Args a, const u64 *pred, u64 out_cap) {
    static_assert(KEYS == 1 || KEYS == 2, "4-byte keys of one kind");
    __shared__ u32 skey[P_CAP];     // sort keys in column order; then the records' rows
    __shared__ double sval[P_CAP];  // values by slot; then the records' values
    __shared__ u32 ccnt[THREADS];   // entries per local column, then where its run starts
    __shared__ u32 lw[2 * WAVES];
    __shared__ u32 s_rmin, s_rmax;

    // ---- claim: the segment is the workgroup's number; its bounds and its place come back in one round trip (uniform loads)
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const i64 nb = a.pair_buckets;
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
    pair_stamp(a, s, 0, t == 0);
    const Pair pr = pair_open(a, s, beg, mid, seg_end, t);
    // ---- the run of the lane's column, sorted, and what it emits
    u32 k[NI];
    unsigned short slot[NI];
    pair_load(a, pr, lane, k, sval, &s_rmin, &s_rmax);
    pair_stamp(a, s, 1, t == 0);
    const PairRun run = pair_count(a, pr, t, k, slot, ccnt, lw, &s_rmin, &s_rmax);
    __syncthreads();  // (ccnt: the run starts)
    pair_stamp(a, s, 2, t == 0);
    pair_scatter(pr, run, k, slot, ccnt, skey);
    __syncthreads();
    pair_stamp(a, s, 3, t == 0);
    u32 x[R];
    double xv[R];
    pair_sort_run(run, skey, sval, x, xv);
    const u32 ec = pair_emitted<KEYS>(a, run.len, x, xv);
    pair_stamp(a, s, 8, t == 0);
    const PairPlace pl = pair_place(ec, lw, lane, w);
    pair_stamp(a, s, 9, t == 0);
    // ---- place: the table's, or nothing is stored
    if (!pair_table_hit(dst, dst_next, pl.total, out_cap, s)) {
        if (t == 0) atomicOr(a.err, PRED_MISS);
        return;
    }
    pair_fold<KEYS>(a, run, x, xv, pl.at0, skey, sval);
    pair_stamp(a, s, 10, t == 0);
    pair_stamp(a, s, 4, t == 0);
    pair_stamp(a, s, 5, t == 0);
    __syncthreads();
    pair_stamp(a, s, 6, t == 0);
    if (!run.fits) return;  // (the flush runs again with pair_k, then local_k)
    pair_store<false>(a, skey, sval, 1, dst, pl, pr.hi, pr.ncl, s, t);
    if (s == a.S - 1 && t == 0) a.status[s] = pair_grand_total(dst, pl.total);  // (where the host reads it)
    pair_stamp(a, s, 7, t == 0);
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
    return pair_for_keys(v.keys, [&](auto K) {
        hipLaunchKernelGGL((pair_pred_k<decltype(K)::value>), dim3(grid), dim3(THREADS), 0, stream, a, pred, out_cap);
    });
}

bool launch_pair(const Variant &v, unsigned grid, hipStream_t stream, const Args &a) {
    if (!v.fresh || v.pieces) return false;
    return pair_for_keys(v.keys, [&](auto K) { hipLaunchKernelGGL((pair_k<decltype(K)::value>), dim3(grid), dim3(THREADS), 0, stream, a); });
}

}  // namespace esplocal
