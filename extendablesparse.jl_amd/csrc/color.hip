// color.hip -- libesparse_hip: the multicolour ordering (esp_graph_coloring) and ColoredPreconditioner (esp_precon_colored_create)
// (see internal.hpp for the map of the translation units)
//
// The reference (src/factorizations/parallel_ilu0.jl) colours the graph of A + transpose(A) by repeated independent sets over
// rand(); the rule here draws nothing.  It is stated in full in include/esparse_hip.h and DESIGN.md 5m; tests/coloring_model.c restates
// it as plain loops and is normative.  In short: i and j != i are neighbours when A[i,j] or A[j,i] is stored (the pattern alone),
// key(i) = (u64)amg_mix(i) << 32 | i, and in round r = 1, 2, ... an uncoloured i receives colour r iff its key exceeds the key of every
// neighbour that was uncoloured at the start of the round.  ncolors = the rounds, c = the vertices sorted by (colour, index).
//
//   color_round_k   one round, one lane per vertex of the round's list (round 1: every vertex).  The neighbours are column i of the
//                   CSC and row i of esp_mul's row-wise index; a vertex whose column or row holds more than AMG_LONG entries is folded
//                   by its whole wave, 64 entries at a time, as rs_pmis_k does.  ONE colour array serves: in round r a neighbour whose
//                   colour reads 0 or r was uncoloured at the round's start.  One that receives r during the round has a larger key
//                   than every uncoloured neighbour of its own, the reader among them: the reader is beaten whichever of the two
//                   values it sees.  A beaten vertex joins the next round's list (wave-aggregated atomicAdd: the list's order varies
//                   from run to run, no decision depends on it) and the list's length is the one counter the host reads per round.
//                   Rounds are separated by kernel boundaries on the handle's stream and by nothing else.
//   the permutation a stable LSD sort of the vertices in index order on the colour bits (the radix passes of ILUAM's level sort), then
//                   new(c[k]) = k and part = 0: the maps of block.hip's permuted path over the single partition c.
//   the kind        everything else is block.hip's: build_b forms A[c,c] (renumbering, column sort, src), block_update gathers the
//                   values and drives the inner preconditioner, block_ldiv_launch is gather / inner ldiv! / scatter.
#include "amg.hpp"

using namespace espamg;

namespace {

constexpr int CT = 256;  // threads of every kernel here

__device__ __forceinline__ u64 color_key(i64 i) { return ((u64)amg_mix(i) << 32) | (u64)(u32)i; }

// is the neighbour j a member of U in round r with a key above k?  (j == i never is: its key equals k)
__device__ __forceinline__ bool color_beats(const u32 *color, u32 r, i64 j, u64 k) {
    const u32 cj = color[j];
    return (cj == 0u || cj == r) && color_key(j) > k;
}

// rp = csr_rowptr + 1: the entries of row i are [rp[i], rp[i+1]) of col.  list == nullptr: the vertices 0..count-1.
// color is read and written by the same launch (see above): no __restrict__
__global__ __launch_bounds__(CT) void color_round_k(const i64 *__restrict__ colptr, const i64 *__restrict__ rowval, const u64 *__restrict__ rp,
                                                    const u32 *__restrict__ col, u32 *color, u32 r, const u32 *__restrict__ list,
                                                    u32 count, u32 *__restrict__ next, u32 *__restrict__ cnt) {
    const i64 t = (i64)blockIdx.x * CT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = t < (i64)count;
    i64 i = 0, s = 0, e = 0;
    u64 rs = 0, re = 0, ki = 0;
    if (live) {
        i = list ? (i64)list[t] : t;
        s = colptr[i] - 1;
        e = colptr[i + 1] - 1;
        rs = rp[i];
        re = rp[i + 1];
        ki = color_key(i);
    }
    bool beaten = false;
    const bool longv = e - s > AMG_LONG || re - rs > (u64)AMG_LONG;
    if (!longv) {
        for (i64 k = s; k < e; k++) beaten = beaten || color_beats(color, r, rowval[k] - 1, ki);
        for (u64 k = rs; k < re; k++) beaten = beaten || color_beats(color, r, (i64)col[k], ki);
    }
    // the wave's long vertices one after the other, 64 entries at a time (every lane of the wave gets here: nobody left early)
    u64 mask = __ballot(longv);
    while (mask) {
        const int sl = __builtin_ctzll(mask);
        mask &= mask - 1;
        const i64 ls = __shfl(s, sl), le = __shfl(e, sl);
        const u64 lrs = __shfl(rs, sl), lre = __shfl(re, sl), lk = __shfl(ki, sl);
        bool v = false;
        for (i64 b = ls; b < le; b += 64) {
            const i64 k = b + lane;
            if (k < le) v = v || color_beats(color, r, rowval[k] - 1, lk);
        }
        for (u64 b = lrs; b < lre; b += 64) {
            const u64 k = b + (u64)lane;
            if (k < lre) v = v || color_beats(color, r, (i64)col[k], lk);
        }
        const bool any = __ballot(v) != 0ull;
        if (lane == sl) beaten = any;
    }
    const bool lose = live && beaten;
    const u64 m = __ballot(lose);
    if (m) {
        const int lead = __builtin_ctzll(m);
        u32 base = 0;
        if (lane == lead) base = atomicAdd(cnt, (u32)__popcll(m));
        base = __shfl(base, lead);
        if (lose) next[base + (u32)__popcll(m & ((1ull << lane) - 1ull))] = (u32)i;
    }
    if (live && !beaten) color[i] = r;
}

__global__ void color_keys_k(const u32 *__restrict__ color, i64 n, u64 *__restrict__ key, double *__restrict__ payload) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = (u64)(color[i] - 1u) << ESP_TAG_BITS;
    payload[i] = __longlong_as_double((long long)i);
}
// c[k] = the k-th vertex of the sorted order, new(c[k]) = k, part = 0
__global__ void color_maps_k(const double *__restrict__ spayload, i64 n, u32 *__restrict__ perm, u32 *__restrict__ newpos, u32 *__restrict__ part) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const u32 i = (u32)__double_as_longlong(spayload[k]);
    perm[k] = i;
    newpos[i] = (u32)k;
    part[k] = 0u;
}

// the colouring of h's stored pattern (checked, square, flushed): color (u32 n, 1-based colours), ptr = the colours' offsets in c
int32_t color_graph(esp_handle *h, DevBuf &color, std::vector<i64> &ptr) {
    hipStream_t s = h->stream;
    const i64 n = h->n;
    ptr.assign(1, 0);
    CK(ensure(h, color, sizeof(u32) * (size_t)std::max<i64>(n, 1)));
    if (n == 0) return ESP_OK;
    CK(csr_current(h));
    Temps tmp;
    DevBuf &l0 = tmp.b[0], &l1 = tmp.b[1], &cnt = tmp.b[2];
    CK(ensure(h, l0, sizeof(u32) * (size_t)n));
    CK(ensure(h, l1, sizeof(u32) * (size_t)n));
    CK(ensure(h, cnt, sizeof(u32) * 2));
    HIPCK(h, hipMemsetAsync(color.p, 0, sizeof(u32) * (size_t)n, s));
    const u32 *list = nullptr;
    u32 *next = (u32 *)l0.p, *other = (u32 *)l1.p;
    i64 count = n;
    for (i64 r = 1; count > 0; r++) {  // the largest key of U is coloured in every round: at most n rounds
        if (r > n) FAIL(h, ESP_ERR_HIP, "esp_graph_coloring: the colouring did not end after %lld rounds", (long long)n);
        HIPCK(h, hipMemsetAsync(cnt.p, 0, sizeof(u32) * 2, s));
        hipLaunchKernelGGL(color_round_k, dim3(grid_for(count, CT)), dim3(CT), 0, s, (const i64 *)h->colptr.p, (const i64 *)h->rowval.p,
                           (const u64 *)h->csr_rowptr.p + 1, (const u32 *)h->csr_col.p, (u32 *)color.p, (u32)r, list, (u32)count, next,
                           (u32 *)cnt.p);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, cnt.p, sizeof(u32), hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        const i64 left = (i64) * (const u32 *)h->pin_scalar;
        if (left >= count) FAIL(h, ESP_ERR_HIP, "esp_graph_coloring: round %lld coloured nothing (%lld left)", (long long)r, (long long)left);
        ptr.push_back(ptr.back() + (count - left));
        list = next;
        std::swap(next, other);
        count = left;
    }
    return ESP_OK;
}

// perm = the vertices sorted by (colour, index); newpos = its inverse; part = 0 (u32 n each)
int32_t color_maps(esp_handle *h, const DevBuf &color, i64 ncolors, DevBuf &perm, DevBuf &newpos, DevBuf &part) {
    hipStream_t s = h->stream;
    const i64 n = h->n;
    for (DevBuf *b : {&perm, &newpos, &part}) CK(ensure(h, *b, sizeof(u32) * (size_t)std::max<i64>(n, 1)));
    if (n == 0) return ESP_OK;
    Temps tmp;
    CK(ensure(h, tmp.b[0], (size_t)n * 4 * 8));
    const PingPong d = carve_pingpong(tmp.b[0].p, n);
    const unsigned g = grid_for(n, CT);
    hipLaunchKernelGGL(color_keys_k, dim3(g), dim3(CT), 0, s, (const u32 *)color.p, n, d.k[0], d.v[0]);
    int B = 1;
    while (((i64)1 << B) < ncolors) B++;
    SortPair r;
    CK(sort_segment_lsd(h, d.half(0), d, n, 0, B, 62, &r));
    hipLaunchKernelGGL(color_maps_k, dim3(g), dim3(CT), 0, s, r.v, n, (u32 *)perm.p, (u32 *)newpos.p, (u32 *)part.p);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(s));
    return ESP_OK;
}

int32_t colored_current(esp_precon *p, const char *what) {
    esp_handle *h = p->h;
    if (h->pattern_version != p->pattern_version || h->nnz != p->nnz)
        FAIL(h, ESP_ERR_STATE, "%s: the matrix pattern changed since the preconditioner's last update!", what);
    return ESP_OK;
}

}  // namespace

int32_t color_update(esp_precon *p) {
    esp_handle *h = p->h;
    CK(precon_check_handle(h, "esp_precon_update"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_colored: a column window / column shard");
    CK(derived_follow_stream(p));
    if (!derived_stale(p)) return block_update(p);  // the values only
    // A's pattern is new: the colouring and the maps anew, in buffers of their own until block_update has replaced B -- a rebuild that
    // fails before that leaves p as its last good update made it
    DevBuf color, perm, newpos, part;
    std::vector<i64> ptr;
    const bool was_rebuild = p->der.rebuild;
    int32_t st = color_graph(h, color, ptr);
    if (st == ESP_OK) st = color_maps(h, color, (i64)ptr.size() - 1, perm, newpos, part);
    if (st == ESP_OK) {
        std::swap(p->blk_new, newpos);
        std::swap(p->blk_part, part);
        p->der.rebuild = true;
        st = block_update(p);
        if (st != ESP_OK && p->der.rebuild) {  // B was not replaced: the earlier maps again
            std::swap(p->blk_new, newpos);
            std::swap(p->blk_part, part);
            p->der.rebuild = was_rebuild;
        } else {
            std::swap(p->col_color, color);
            std::swap(p->col_perm, perm);
            p->col_ptr.swap(ptr);
        }
    }
    (void)hipStreamSynchronize(h->stream);
    for (DevBuf *b : {&color, &perm, &newpos, &part}) release(*b);
    return st;
}

void color_release(esp_precon *p) {
    release(p->col_color);
    release(p->col_perm);
}

extern "C" int32_t esp_graph_coloring(esp_handle *h, int64_t *ncolors, int64_t *color, int32_t on_device) {
    if (!h || !ncolors) return ESP_ERR_INVALID;
    CK(precon_check_handle(h, "esp_graph_coloring"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_graph_coloring: a column window / column shard");
    DevBuf col;
    std::vector<i64> ptr;
    int32_t st = color_graph(h, col, ptr);
    if (st == ESP_OK && color) st = export_u32_as_i64(h, col.p, h->n, 1u, color, on_device);
    (void)hipStreamSynchronize(h->stream);
    release(col);
    if (st == ESP_OK) *ncolors = (i64)ptr.size() - 1;
    return st;
}

extern "C" int32_t esp_precon_colored_create(esp_handle *h, int32_t inner_kind, esp_precon **out) {
    if (!h || !out) return ESP_ERR_INVALID;
    *out = nullptr;
    if (inner_kind != ESP_PRECON_ILU0 && inner_kind != ESP_PRECON_ILUAM)
        FAIL(h, ESP_ERR_INVALID, "esp_precon_colored_create: inner_kind %d is neither ILU0 nor ILUAM", inner_kind);
    CK(precon_check_handle(h, "esp_precon_colored_create"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_colored_create: a column window / column shard");
    const i64 n = h->n;
    esp_precon *p = precon_new(h, ESP_PRECON_COLORED);
    p->der.inner_kind = inner_kind;
    p->blk_increasing = n == 0;  // the permuted path always (an empty matrix: the identity path, nothing to permute)
    p->der.rebuild = true;
    const int32_t st = [&]() -> int32_t {
        const int32_t cs = esp_create(n, n, h->device, 0, &p->der.bh);
        if (cs != ESP_OK) FAIL(h, cs, "esp_precon_colored_create: the handle of B: %s", esp_last_error(nullptr));
        return color_update(p);
    }();
    return precon_finish(p, st, out);
}

extern "C" int32_t esp_precon_colored_info(esp_precon *p, int64_t out[2]) {
    if (!p || p->kind != ESP_PRECON_COLORED || !out) return ESP_ERR_INVALID;
    out[0] = (i64)p->col_ptr.size() - 1;
    out[1] = p->der.bh ? p->der.bh->nnz : 0;
    return ESP_OK;
}

extern "C" int32_t esp_precon_colored_colors(esp_precon *p, int64_t *color, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_COLORED || !color) return ESP_ERR_INVALID;
    CK(colored_current(p, "esp_precon_colored_colors"));
    return export_u32_as_i64(p->h, p->col_color.p, p->h->n, 1u, color, on_device);
}

extern "C" int32_t esp_precon_colored_perm(esp_precon *p, int64_t *c, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_COLORED || !c) return ESP_ERR_INVALID;
    CK(colored_current(p, "esp_precon_colored_perm"));
    return export_u32_as_i64(p->h, p->col_perm.p, p->h->n, 0u, c, on_device);
}

extern "C" int32_t esp_precon_colored_matrix(esp_precon *p, esp_handle **b) {
    if (!p || p->kind != ESP_PRECON_COLORED) return ESP_ERR_INVALID;
    if (b) *b = p->der.bh;
    return ESP_OK;
}
