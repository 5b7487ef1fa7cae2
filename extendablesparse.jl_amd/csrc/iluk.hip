// iluk.hip -- libesparse_hip: ILUKPreconditioner, the level-of-fill ILU(k), on the device CSC (see internal.hpp for the map of the
// translation units)
//
// lev(i,j) = 0 where A stores (i,j), else infinite; for i = 0..n-1, for k < i increasing with lev(i,k) <= K, for j > k with
// lev(k,j) <= K: lev(i,j) = min(lev(i,j), lev(i,k) + lev(k,j) + 1).  B holds every position of level <= K -- A's bits where the level
// is 0, +0.0 elsewhere -- and the preconditioner is ILUAM of B: the factorization, the solves, the values-only update and the
// solvers' dispatch are iluam.hip's, on B's handle (tests/iluk_model.c restates the sequential rule).
//
// The pattern comes from one bounded search per column (lev(i,j) + 1 is the length of the shortest path i -> j whose interior
// vertices are all below min(i,j)):
//   lower part  column j of B below the diagonal: a level-synchronous breadth-first search from j in the graph "the neighbours of u
//               are the stored rows of column u".  A first-visited row w > j is the entry (w, j) with the level dist(u) of the vertex
//               it was found from, and is never expanded; a first-visited w < j is enqueued with dist(u) + 1 while that is <= K.
//   upper part  the same search over transpose(A) (esp_transpose into an internal handle): an emitted (w, j) is the entry (j, w).
//   diagonal    the stored (j, j) of column j, met at depth 0 of the lower search.
// iluk_search_k runs one source column per workgroup: the visited set is an open-addressing table in LDS (insertion by compare-and-swap,
// so that a row two frontier vertices of one depth reach is emitted once), the frontier a queue in LDS whose depth slices follow each
// other.  The wave form (64 lanes, ESP_ILUK_WAVE_VISITS vertices) serves every column first; a column whose visited set -- the source,
// every enqueued vertex and every row emitted beyond level 0 (the level-0 rows are the column itself: they never enter the table, so
// k = 0 takes any matrix) -- outgrows it is listed and redone by the workgroup form (512 lanes,
// ESP_ILUK_VISIT_MAX vertices, 96 KiB of LDS); beyond that the create is refused in the count pass.
//   count       the searches add the entries of every column of B into the column counts (an overflowing search adds nothing), a scan
//               makes the column starts;
//   fill        the same searches emit (row, payload) behind a cursor per column; payload = level << 32 | position in A's nzval of a
//               level-0 entry (ILUK_FILL otherwise; the upper search finds the position by bisection in A's column);
//   sort        every column by row: the lane / workgroup column sorts of linalg.hip, or -- a column above their limit -- the entries
//               as ESP_COO records through a flush of a scratch handle (block.hip's routes);
//   unpack      src[q], lev[q] and B.nzval[q] from the sorted payloads, the largest level beside them.
// update! with the pattern kept: B.nzval[q] = src[q] == ILUK_FILL ? +0.0 : A.nzval[src[q]] (one gather) and the inner values-only
// update -- bitwise what a fresh create gives.
#include "internal.hpp"

namespace {

constexpr int WAVE_T = 64, WIDE_T = 512;  // lanes of the two forms of the search
constexpr int SHORT_COL = 16;           // a frontier vertex with more stored rows is expanded by the whole workgroup
constexpr u32 ILUK_EMPTY = 0xFFFFFFFFu;  // (n < 2^32 - 16: no vertex)
static_assert((ESP_ILUK_WAVE_VISITS & (ESP_ILUK_WAVE_VISITS - 1)) == 0 && (ESP_ILUK_VISIT_MAX & (ESP_ILUK_VISIT_MAX - 1)) == 0,
              "the visited tables hold twice the capacity, a power of two");
static_assert(ESP_ILUK_WAVE_VISITS >= 2 * WAVE_T && ESP_ILUK_VISIT_MAX >= 2 * WIDE_T, "insertions in flight when the table is closed");
static_assert((size_t)ESP_ILUK_VISIT_MAX * 12 + 64 <= 160 * 1024, "table and queue of the workgroup form: the LDS of one CU");

struct SearchOut {
    unsigned long long *cnt;   // count: the entries of every column of B (n, added atomically)
    const i64 *cp;             // fill: the 0-based start of every column of B (n + 1)
    unsigned long long *cur;   // fill: entries written to every column so far (n)
    i64 *rowB;                 // fill: 1-based rows ...
    u64 *pay;                  // ... and payloads
    u64 *keys;                 // ... or, keys != nullptr: ESP_COO records (key, pay) for the flush of a scratch handle
    KeyLayout L;
    uint8_t *wide;             // per source column: the wave form overflowed (count sets it, fill skips the column)
    u32 *list;                 // count, wave form: the overflowed columns
    unsigned long long *nlist; // ... how many
    unsigned long long *bad;   // count, workgroup form: the smallest column that overflowed it
    unsigned long long *err;   // fill: an entry fell outside its column (count and fill disagree)
};

constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x >> 1); }

template <bool FILL>
__device__ __forceinline__ void iluk_emit(const SearchOut &o, i64 row, i64 col, u32 level, u32 pos) {
    if (!FILL) return;
    const i64 q = o.cp[col] + (i64)atomicAdd(&o.cur[col], 1ull);
    if (q >= o.cp[col + 1]) {
        atomicMax(o.err, 1ull);
        return;
    }
    const u64 pay = ((u64)level << 32) | (u64)pos;
    if (o.keys) o.keys[q] = esp_pack(o.L, row + 1, col + 1, ESP_COO);
    else o.rowB[q] = row + 1;
    o.pay[q] = pay;
}

// one source column per workgroup (sources != nullptr: the listed ones).  gcp / grv: the graph searched (A: lower, transpose(A):
// upper); A: the matrix itself (the upper search looks its level-0 positions up there)
template <int T, int CAP, bool FILL>
__global__ __launch_bounds__(T) void iluk_search_k(const i64 *__restrict__ gcp, const i64 *__restrict__ grv, espfold::Csc A, i64 n, int K,
                                                   bool upper, const u32 *__restrict__ sources, SearchOut o) {
    constexpr int TS = 2 * CAP;
    constexpr int SHIFT = 32 - ilog2(TS);
    __shared__ u32 tab[TS];
    __shared__ u32 queue[CAP];
    __shared__ int s_tail, s_nvis, s_ovf;
    __shared__ unsigned s_emit;
    const int tid = threadIdx.x;
    const i64 j = sources ? (i64)sources[blockIdx.x] : (i64)blockIdx.x;
    if (j >= n) return;
    if (FILL && !sources && o.wide[j]) return;  // (the workgroup form writes this column)
    for (int t = tid; t < TS; t += T) tab[t] = ILUK_EMPTY;
    if (tid == 0) {
        s_tail = 1;
        s_nvis = 1;
        s_ovf = 0;
        s_emit = 0;
        queue[0] = (u32)j;
    }
    __syncthreads();
    if (tid == 0) tab[((u32)j * 0x9E3779B1u) >> SHIFT] = (u32)j;
    __syncthreads();
    // the stored row at position k of the column of a vertex at distance d.  The rows of column j itself (d = 0) are distinct and
    // known: those above j are emitted without entering the table, and a later depth that reaches one finds it in the column
    auto visit = [&](i64 k, int d) {
        if (*(volatile int *)&s_ovf) return;
        const u32 w = (u32)(grv[k] - 1);
        if (w == (u32)j) {
            if (FILL && d == 0 && !upper) iluk_emit<FILL>(o, j, j, 0u, (u32)k);  // the diagonal of column j
            return;
        }
        const bool above = w > (u32)j;
        if (above && d == 0) {
            if (!FILL) return;  // (counted from the column below)
            if (!upper) iluk_emit<FILL>(o, (i64)w, j, 0u, (u32)k);
            else iluk_emit<FILL>(o, j, (i64)w, 0u, (u32)espfold::csc_find(A, (i64)w, j));  // A stores (j, w): transpose(A) stores (w, j)
            return;
        }
        if (!above && (i64)d + 1 > (i64)K) return;
        u32 s = (w * 0x9E3779B1u) >> SHIFT;
        if (above) {  // visited before?  Then: a row of column j?
            u32 t = s;
            for (int probe = 0; probe < TS; probe++) {
                const u32 old = *(volatile u32 *)&tab[t];
                if (old == w) return;
                if (old == ILUK_EMPTY) break;
                t = (t + 1) & (u32)(TS - 1);
            }
            i64 lo = gcp[j] - 1, hi = gcp[j + 1] - 1;
            while (lo < hi) {
                const i64 mid = lo + ((hi - lo) >> 1);
                if (grv[mid] < (i64)w + 1) lo = mid + 1;
                else hi = mid;
            }
            if (lo < gcp[j + 1] - 1 && grv[lo] == (i64)w + 1) return;
        }
        bool fresh = false;
        for (int probe = 0; probe < TS; probe++) {
            const u32 old = atomicCAS(&tab[s], ILUK_EMPTY, w);
            if (old == w) return;  // visited before (or by another lane of this depth)
            if (old == ILUK_EMPTY) {
                fresh = true;
                break;
            }
            s = (s + 1) & (u32)(TS - 1);
        }
        if (!fresh || atomicAdd(&s_nvis, 1) + 1 > CAP) {
            s_ovf = 1;
            return;
        }
        if (!above) {
            queue[atomicAdd(&s_tail, 1)] = w;  // (at most CAP - 1 vertices get here: the source holds slot 0)
            return;
        }
        if (!FILL) return;  // (counted from the table below)
        if (!upper) iluk_emit<FILL>(o, (i64)w, j, (u32)d, ILUK_FILL);
        else iluk_emit<FILL>(o, j, (i64)w, (u32)d, ILUK_FILL);
    };
    int head = 0, tail = 1;
    for (int d = 0; head < tail; d++) {
        for (int f = head + tid; f < tail; f += T) {  // short columns: a lane each
            const i64 u = (i64)queue[f];
            const i64 s = gcp[u] - 1, e = gcp[u + 1] - 1;
            if (e - s <= SHORT_COL)
                for (i64 k = s; k < e; k++) visit(k, d);
        }
        for (int f = head; f < tail; f++) {  // long columns: all lanes
            const i64 u = (i64)queue[f];
            const i64 s = gcp[u] - 1, e = gcp[u + 1] - 1;
            if (e - s > SHORT_COL)
                for (i64 k = s + tid; k < e; k += T) visit(k, d);
        }
        __syncthreads();
        head = tail;
        tail = s_tail;
        const int ovf = s_ovf;
        __syncthreads();
        if (ovf) break;
    }
    if (s_ovf) {
        if (tid == 0 && !FILL) {
            if (!sources) {
                o.wide[j] = 1;
                o.list[atomicAdd(o.nlist, 1ull)] = (u32)j;
            } else {
                atomicMin(o.bad, (unsigned long long)j);
            }
        } else if (tid == 0) {
            atomicMax(o.err, 1ull);
        }
        return;
    }
    if (FILL) return;
    // count: every row of column j from the diagonal on (lower; above it: upper) and every visited w > j is an entry -- of column j
    // (lower) or of column w (upper)
    unsigned mine = 0;
    for (i64 k = gcp[j] - 1 + tid; k < gcp[j + 1] - 1; k += T) {
        const u32 w = (u32)(grv[k] - 1);
        if (w < (u32)j || (upper && w == (u32)j)) continue;
        if (upper) atomicAdd(&o.cnt[w], 1ull);
        else mine++;
    }
    for (int t = tid; t < TS; t += T) {
        const u32 w = tab[t];
        if (w == ILUK_EMPTY || w <= (u32)j) continue;
        if (upper) atomicAdd(&o.cnt[w], 1ull);
        else mine++;
    }
    if (!upper) {
        if (mine) atomicAdd(&s_emit, mine);
        __syncthreads();
        if (tid == 0 && s_emit) atomicAdd(&o.cnt[j], (unsigned long long)s_emit);
    }
}

// derived_update's builder: B from A's current CSC, installed in p->der.bh, src in p->der.src, the levels in p->iluk_lev; nothing of p
// changes when it fails
int32_t build_b(esp_precon *p) {
    esp_handle *h = p->h, *bh = p->der.bh, *th = p->iluk_th;
    hipStream_t s = h->stream;
    const i64 n = p->n;
    const int K = p->iluk_k;
    Temps tmp;
    DevBuf &cp = tmp.b[0], &rv = tmp.b[1], &nz = tmp.b[2], &src = tmp.b[3], &pay = tmp.b[4], &stat = tmp.b[6], &ws = tmp.b[7],
           &lev = tmp.b[8], &cur = tmp.b[9], &wide = tmp.b[10], &wlist = tmp.b[11];
    ColumnSort cs(h, "esp_precon_iluk");
    int l = 0;
    if (n > 0) {
        const int32_t ts = esp_transpose(h, th, nullptr);
        if (ts != ESP_OK) FAIL(h, ts, "esp_precon_iluk: transpose(A): %s", th->err.c_str());
    }
    CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, stat, sizeof(u64) * 8));
    CK(ensure(h, wide, (size_t)std::max<i64>(2 * n, 1)));
    CK(ensure(h, wlist, sizeof(u32) * (size_t)std::max<i64>(2 * n, 1)));
    HIPCK(h, hipMemsetAsync(cp.p, 0, sizeof(i64) * (size_t)(n + 1), s));
    HIPCK(h, hipMemsetAsync(wide.p, 0, (size_t)std::max<i64>(2 * n, 1), s));
    HIPCK(h, hipMemsetAsync(stat.p, 0, sizeof(u64) * 8, s));
    unsigned long long *st = (unsigned long long *)stat.p;  // 0 / 1: listed columns (L, U), 2: smallest refused column, 3: fill error,
                                                            // 4: largest level, 5 / 6: the sort's listed columns and longest column
    hipLaunchKernelGGL(fill_i64_k, dim3(1), dim3(1), 0, s, (i64 *)st + 2, (i64)1, (i64)-1);
    const espfold::Csc A{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (double *)h->nzval.p, h->nnz};
    const i64 *gcp[2] = {(const i64 *)h->colptr.p, (const i64 *)th->colptr.p};
    const i64 *grv[2] = {(const i64 *)h->rowval.p, (const i64 *)th->rowval.p};
    SearchOut base{};
    base.cnt = (unsigned long long *)cp.p;
    base.L = h->L;
    base.bad = st + 2;
    base.err = st + 3;
    auto side = [&](int u) {  // the lower (0) / upper (1) search's own arrays
        SearchOut o = base;
        o.wide = (uint8_t *)wide.p + (size_t)u * (size_t)n;
        o.list = (u32 *)wlist.p + (size_t)u * (size_t)n;
        o.nlist = st + u;
        return o;
    };
    i64 nwide[2] = {0, 0};
    if (n > 0 && h->nnz > 0) {
        for (int u = 0; u < 2; u++)
            hipLaunchKernelGGL((iluk_search_k<WAVE_T, ESP_ILUK_WAVE_VISITS, false>), dim3((unsigned)n), dim3(WAVE_T), 0, s, gcp[u], grv[u], A, n, K,
                               u == 1, (const u32 *)nullptr, side(u));
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, st, sizeof(u64) * 2, hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        nwide[0] = (i64)h->pin_scalar[0];
        nwide[1] = (i64)h->pin_scalar[1];
        for (int u = 0; u < 2; u++)
            if (nwide[u] > 0)
                hipLaunchKernelGGL((iluk_search_k<WIDE_T, ESP_ILUK_VISIT_MAX, false>), dim3((unsigned)nwide[u]), dim3(WIDE_T), 0, s, gcp[u], grv[u],
                                   A, n, K, u == 1, (const u32 *)side(u).list, side(u));
        if (nwide[0] + nwide[1] > 0) {
            HIPCK(h, hipGetLastError());
            HIPCK(h, hipMemcpyAsync(h->pin_scalar, st + 2, sizeof(u64), hipMemcpyDeviceToHost, s));
            HIPCK(h, hipStreamSynchronize(s));
            if (h->pin_scalar[0] != ~0ull)
                FAIL(h, ESP_ERR_UNSUPPORTED,
                     "esp_precon_iluk: the search of column %llu with k = %d visits more than ESP_ILUK_VISIT_MAX = %d vertices (the smallest such "
                     "column)",
                     h->pin_scalar[0], K, (int)ESP_ILUK_VISIT_MAX);
        }
    }
    if (n > 0) CK(scan_inplace<i64, false>(h, (i64 *)cp.p, n + 1, ws, &l));
    HIPCK(h, hipGetLastError());
    i64 nnzB = 0;
    CK(read_i64(h, (const i64 *)cp.p + n, &nnzB));
    if (nnzB < h->nnz) FAIL(h, ESP_ERR_HIP, "esp_precon_iluk: %lld entries of B for %lld of A", (long long)nnzB, (long long)h->nnz);
    if (nnzB >= 0xFFFFFFF0ll)
        FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_iluk: k = %d fills the matrix to %lld entries (the preconditioners' index holds 32-bit positions)", K,
             (long long)nnzB);
    CK(ensure(h, src, sizeof(u32) * (size_t)std::max<i64>(nnzB, 1)));
    CK(ensure(h, lev, sizeof(int32_t) * (size_t)std::max<i64>(nnzB, 1)));
    CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nnzB, 1)));
    bool one_based = false;
    if (nnzB > 0) {
        CK(ensure(h, cur, sizeof(u64) * (size_t)n));
        HIPCK(h, hipMemsetAsync(cur.p, 0, sizeof(u64) * (size_t)n, s));
        CK(cs.plan(cp, n, nnzB, st + 5, rv, pay));
        base.cnt = nullptr;
        base.cp = (const i64 *)cp.p;
        base.cur = (unsigned long long *)cur.p;
        base.rowB = cs.rowB;
        base.pay = cs.pay;
        base.keys = cs.keys;
        base.L = cs.L;
        for (int u = 0; u < 2; u++) {
            hipLaunchKernelGGL((iluk_search_k<WAVE_T, ESP_ILUK_WAVE_VISITS, true>), dim3((unsigned)n), dim3(WAVE_T), 0, s, gcp[u], grv[u], A, n, K,
                               u == 1, (const u32 *)nullptr, side(u));
            if (nwide[u] > 0)
                hipLaunchKernelGGL((iluk_search_k<WIDE_T, ESP_ILUK_VISIT_MAX, true>), dim3((unsigned)nwide[u]), dim3(WIDE_T), 0, s, gcp[u],
                                   grv[u], A, n, K, u == 1, (const u32 *)side(u).list, side(u));
        }
        CK(cs.finish(&one_based));
    }
    if (nnzB == 0) CK(ensure(h, rv, sizeof(i64)));
    if (!one_based) add_one_launch(s, (i64 *)cp.p, n + 1);
    if (nnzB > 0)
        derived_gather_launch(s, (const u64 *)pay.p, (u32 *)src.p, (int32_t *)lev.p, (const u64 *)h->nzval.p, (u64 *)nz.p, nnzB, st + 4);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, st + 3, sizeof(u64) * 2, hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    if (h->pin_scalar[0] != 0) FAIL(h, ESP_ERR_HIP, "esp_precon_iluk: the fill pass of the search disagrees with its count pass");
    const i64 maxlev = (i64)h->pin_scalar[1];
    install(bh, cp, rv, nz, nnzB);
    std::swap(p->der.src, src);
    std::swap(p->iluk_lev, lev);
    p->iluk_stats[0] = nnzB;
    p->iluk_stats[1] = maxlev;
    p->iluk_stats[2] = nwide[0];
    p->iluk_stats[3] = nwide[1];
    return ESP_OK;
}

}  // namespace

int32_t iluk_update(esp_precon *p) { return derived_update(p, "esp_precon_iluk", build_b, ""); }

void iluk_release(esp_precon *p) {
    if (p->iluk_th) (void)esp_destroy(p->iluk_th);
    p->iluk_th = nullptr;
    release(p->iluk_lev);
}

extern "C" int32_t esp_precon_iluk_create(esp_handle *h, int32_t k, esp_precon **out) {
    if (!h || !out) return ESP_ERR_INVALID;
    *out = nullptr;
    if (k < 0) FAIL(h, ESP_ERR_INVALID, "esp_precon_iluk_create: k = %d < 0", k);
    CK(precon_check_handle(h, "esp_precon_iluk_create"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_iluk_create: a column window / column shard");
    esp_precon *p = precon_new(h, ESP_PRECON_ILUK);
    p->der.inner_kind = ESP_PRECON_ILUAM;
    p->iluk_k = k;
    const int32_t st = [&]() -> int32_t {
        for (esp_handle **q : {&p->der.bh, &p->iluk_th}) {
            const int32_t cs = esp_create(h->n, h->n, h->device, 0, q);
            if (cs != ESP_OK) FAIL(h, cs, "esp_precon_iluk_create: an internal handle: %s", esp_last_error(nullptr));
        }
        return iluk_update(p);
    }();
    return precon_finish(p, st, out);
}

extern "C" int32_t esp_precon_iluk_matrix(esp_precon *p, esp_handle **b) {
    if (!p || p->kind != ESP_PRECON_ILUK) return ESP_ERR_INVALID;
    if (b) *b = p->der.bh;
    return ESP_OK;
}

extern "C" int32_t esp_precon_iluk_levels(esp_precon *p, int32_t *lev, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_ILUK || !lev) return ESP_ERR_INVALID;
    return copy_out(p->h, lev, p->iluk_lev.p, sizeof(int32_t) * (size_t)p->iluk_stats[0], on_device);
}

extern "C" int32_t esp_precon_iluk_stats(esp_precon *p, int64_t out[4]) {
    if (!p || p->kind != ESP_PRECON_ILUK || !out) return ESP_ERR_INVALID;
    for (int k = 0; k < 4; k++) out[k] = p->iluk_stats[k];
    return ESP_OK;
}
