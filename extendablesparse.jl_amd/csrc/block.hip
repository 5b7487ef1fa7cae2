// block.hip -- libesparse_hip: BlockPreconditioner on the device CSC (see internal.hpp for the map of the translation units)
//
// The reference (src/factorizations/blockpreconditioner.jl) extracts A[part, part] for every partition, factorizes each with
// the chosen point preconditioner and solves the partitions one by one.  Here the whole preconditioner is ONE matrix B and ONE
// inner esp_precon: B holds exactly the stored A[i,j] with part(i) == part(j).  Jacobi, ILU0 and ILUAM touch row i and column j
// of their matrix only through stored entries, and every ordered loop of theirs runs over a column or row in index order; in a
// matrix whose entries never join two partitions, the entries a row or column of one block meets are that block's alone, in
// the block's own order as long as the numbering is monotone inside every block.  So the factorization and both solves of B
// perform, for every block, the operations of that block's own factorization in the same order: bit-identical.
//
//   maps       new(i) = the position of i in the concatenation of the partitions, part(i) = its partition (u32, n each), made
//              once at create together with the validation (an index out of range, repeated, missing) and the flag "every
//              partition is strictly increasing".
//   path 0     identity (the flag holds): new is monotone inside every block, B keeps A's numbering.  One lane per column
//              counts / copies the kept entries in stored order; a column longer than BK_LONG is compacted by its whole wave,
//              64 entries at a time, the kept ones placed by a 64-bit ballot and a prefix popcount: order is kept, no sort.
//   path 1     permuted: output column new(j) takes column j's kept entries with rows new(i) (the same compaction), then every
//              column is sorted by row (the lane / workgroup column sorts of linalg.hip; keys distinct) with the entry's
//              position in A's nzval as the payload.  A column above that sort's limit: the entries go as ESP_COO records, the
//              position as the value's bits, through a flush of a scratch handle (as esp_transpose's generic path).
//   src[q]     the position in A's nzval entry q of B came from: the values-only refresh is one gather, B.nzval[q] = A.nzval[src[q]]
//              (the bits, moved as they are).
//   vectors    path 1 only: t[new(i)] = v[i] in front of the inner ldiv!, u[i] = s[new(i)] behind it.
#include "internal.hpp"

namespace {

constexpr int BT = 256;       // threads of every kernel here
constexpr int BK_LONG = 32;   // a column with more stored entries is compacted by its whole wave

// ---- validation and maps ---------------------------------------------------------------------------------------------------
// st[0] = first position k of part_idx with an index outside 0..n-1, st[3] = 1 when some partition is not strictly increasing
__global__ void blk_scatter_k(const i64 *__restrict__ idx, const i64 *__restrict__ pptr, i64 nparts, i64 n, u32 *__restrict__ newpos,
                              u32 *__restrict__ part, u32 *__restrict__ cnt, unsigned long long *__restrict__ st) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const i64 v = idx[k];
    if (v < 0 || v >= n) {
        atomicMin(&st[0], (unsigned long long)k);
        return;
    }
    i64 lo = 0, hi = nparts - 1;  // the last partition that starts at or before k (empty ones share a start: the last holds k)
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (pptr[mid] <= k) lo = mid;
        else hi = mid - 1;
    }
    atomicAdd(&cnt[v], 1u);
    newpos[v] = (u32)k;  // (an index named twice is refused before anybody reads this)
    part[v] = (u32)lo;
    if (k > pptr[lo] && !(idx[k - 1] < v)) atomicMax(&st[3], 1ull);
}
// st[1] = smallest index named twice, st[2] = smallest index never named
__global__ void blk_check_k(const u32 *__restrict__ cnt, i64 n, unsigned long long *__restrict__ st) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 c = cnt[i];
    if (c > 1u) atomicMin(&st[1], (unsigned long long)i);
    if (c == 0u) atomicMin(&st[2], (unsigned long long)i);
}

// ---- the masked extraction: count (FILL = false) and fill --------------------------------------------------------------------
struct BlkOut {
    i64 *cp;      // count: the kept entries of output column c (n entries written); fill: the 0-based start of every column
    i64 *rowB;    // fill: 1-based rows of B ...
    u32 *src;     // ... and the entry's position in A's nzval (path 0)
    u64 *pay;     // ... or that position as the sort's payload (path 1; src == nullptr)
    u64 *keys;    // ... or, keys != nullptr: ESP_COO records (key, pay) for the flush of a scratch handle
    KeyLayout L;
};
template <bool FILL>
__device__ __forceinline__ void blk_emit(const BlkOut &o, const u32 *__restrict__ newpos, i64 q, i64 r, i64 k, i64 oc) {
    if (!FILL) return;
    const i64 ro = newpos ? (i64)newpos[r] : r;
    if (o.keys) {
        o.keys[q] = esp_pack(o.L, ro + 1, oc + 1, ESP_COO);
        o.pay[q] = (u64)k;
        return;
    }
    o.rowB[q] = ro + 1;
    if (o.src) o.src[q] = (u32)k;
    else o.pay[q] = (u64)k;
}
template <bool FILL>
__global__ __launch_bounds__(BT) void blk_compact_k(const i64 *__restrict__ colptr, const i64 *__restrict__ rowval, i64 n,
                                                    const u32 *__restrict__ part, const u32 *__restrict__ newpos, BlkOut o) {
    const i64 j = (i64)blockIdx.x * BT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    i64 s = 0, e = 0, oc = 0;
    u32 pj = 0;
    if (j < n) {
        s = colptr[j] - 1;
        e = colptr[j + 1] - 1;
        pj = part[j];
        oc = newpos ? (i64)newpos[j] : j;
    }
    const bool longc = e - s > BK_LONG;
    if (j < n && !longc) {  // one lane, stored order
        i64 q = FILL ? o.cp[oc] : 0;
        for (i64 k = s; k < e; k++) {
            const i64 r = rowval[k] - 1;
            if (part[r] == pj) {
                blk_emit<FILL>(o, newpos, q, r, k, oc);
                q++;
            }
        }
        if (!FILL) o.cp[oc] = q;
    }
    // the wave's long columns one after the other: 64 entries at a time, a kept entry lands behind the kept entries of the
    // lanes below it (every lane of the wave gets here: nobody left early)
    u64 mask = __ballot(longc);
    while (mask) {
        const int sl = __builtin_ctzll(mask);
        mask &= mask - 1;
        const i64 ls = __shfl(s, sl), le = __shfl(e, sl), loc = __shfl(oc, sl);
        const u32 lp = __shfl(pj, sl);
        i64 q = FILL ? o.cp[loc] : 0;
        for (i64 b = ls; b < le; b += 64) {
            const i64 k = b + lane;
            i64 r = 0;
            bool keep = false;
            if (k < le) {
                r = rowval[k] - 1;
                keep = part[r] == lp;
            }
            const u64 m = __ballot(keep);
            if (keep) blk_emit<FILL>(o, newpos, q + __popcll(m & ((1ull << lane) - 1ull)), r, k, loc);
            q += __popcll(m);
        }
        if (!FILL && lane == sl) o.cp[loc] = q;
    }
}
// the build's last step: B.nzval[q] = A.nzval[src[q]] (the bits); pay != nullptr: src[q] is taken from the sort's payload first
__global__ void blk_gather_k(const u64 *__restrict__ pay, u32 *__restrict__ src, const u64 *__restrict__ nzA, u64 *__restrict__ nzB, i64 nnzB) {
    const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nnzB) return;
    u32 s;
    if (pay) {
        s = (u32)pay[q];
        src[q] = s;
    } else {
        s = src[q];
    }
    nzB[q] = nzA[s];
}
// t[new(i)] = v[i]
__global__ void blk_vec_gather_k(const u32 *__restrict__ newpos, const double *__restrict__ v, double *__restrict__ t, i64 n) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) t[newpos[i]] = v[i];
}
// u[i] = s[new(i)]; sub (simple!'s `u .-= upd`): u[i] = u[i] - s[new(i)]
__global__ void blk_vec_scatter_k(const u32 *__restrict__ newpos, const double *__restrict__ s, double *__restrict__ u, i64 n, bool sub) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = s[newpos[i]];
    u[i] = sub ? u[i] - x : x;
}

// the two for the live columns of a chunk: t[new(i) + d*ldt] = v[i + d*ldv]; u[i + d*ldu] = s[new(i) + d*lds] (new(i) read once)
__global__ void blk_vec_gather_many_k(const u32 *__restrict__ newpos, const double *__restrict__ v, i64 ldv, double *__restrict__ t, i64 ldt,
                                      i64 n, u32 live) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const i64 q = newpos[i];
#pragma unroll
    for (int d = 0; d < ESP_MANY_CHUNK; d++)
        if (is_live(live, d)) t[(i64)d * ldt + q] = v[(i64)d * ldv + i];
}
__global__ void blk_vec_scatter_many_k(const u32 *__restrict__ newpos, const double *__restrict__ s, i64 lds, double *__restrict__ u, i64 ldu,
                                       i64 n, u32 live) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const i64 q = newpos[i];
#pragma unroll
    for (int d = 0; d < ESP_MANY_CHUNK; d++)
        if (is_live(live, d)) u[(i64)d * ldu + i] = s[(i64)d * lds + q];
}

// derived_update's builder: B from A's current CSC, installed in p->der.bh, src in p->der.src.  Everything that can fail comes in
// front of the two, the vectors of the permuted path included: nothing of p changes when it fails
int32_t build_b(esp_precon *p) {
    esp_handle *h = p->h;
    hipStream_t s = h->stream;
    const i64 n = p->n;
    const int path = p->blk_force == 1 || !p->blk_increasing ? 1 : 0;
    if (path) {
        CK(ensure(h, p->blk_t, sizeof(double) * (size_t)std::max<i64>(n, 1)));
        CK(ensure(h, p->blk_s, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    }
    Temps tmp;
    DevBuf &cp = tmp.b[0], &rv = tmp.b[1], &nz = tmp.b[2], &src = tmp.b[3], &pay = tmp.b[4], &stat = tmp.b[6], &ws = tmp.b[7];
    ColumnSort cs(h, "esp_precon_block");
    const u32 *newpos = path ? (const u32 *)p->blk_new.p : (const u32 *)nullptr;
    const u32 *part = (const u32 *)p->blk_part.p;
    const i64 *colptr = (const i64 *)h->colptr.p, *rowval = (const i64 *)h->rowval.p;
    int l = 0;
    CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
    HIPCK(h, hipMemsetAsync(cp.p, 0, sizeof(i64) * (size_t)(n + 1), s));
    BlkOut o{(i64 *)cp.p, nullptr, nullptr, nullptr, nullptr, h->L};
    if (n > 0 && h->nnz > 0)
        hipLaunchKernelGGL(blk_compact_k<false>, dim3(grid_for(n, BT)), dim3(BT), 0, s, colptr, rowval, n, part, newpos, o);
    if (n > 0) CK(scan_inplace<i64, false>(h, (i64 *)cp.p, n + 1, ws, &l));
    HIPCK(h, hipGetLastError());
    i64 nnzB = 0;
    CK(read_i64(h, (const i64 *)cp.p + n, &nnzB));
    if (nnzB < 0 || nnzB > h->nnz) FAIL(h, ESP_ERR_HIP, "esp_precon_block: %lld kept entries of %lld", (long long)nnzB, (long long)h->nnz);
    CK(ensure(h, src, sizeof(u32) * (size_t)std::max<i64>(nnzB, 1)));
    CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nnzB, 1)));
    bool one_based = false;
    if (nnzB > 0 && path == 0) {
        CK(ensure(h, rv, sizeof(i64) * (size_t)nnzB));
        o.rowB = (i64 *)rv.p;
        o.src = (u32 *)src.p;
        hipLaunchKernelGGL(blk_compact_k<true>, dim3(grid_for(n, BT)), dim3(BT), 0, s, colptr, rowval, n, part, newpos, o);
    } else if (nnzB > 0) {
        CK(ensure(h, stat, sizeof(u64) * 2));
        HIPCK(h, hipMemsetAsync(stat.p, 0, sizeof(u64) * 2, s));
        CK(cs.plan(cp, n, nnzB, (unsigned long long *)stat.p, rv, pay));
        o.rowB = cs.rowB;
        o.pay = cs.pay;
        o.keys = cs.keys;
        o.L = cs.L;
        hipLaunchKernelGGL(blk_compact_k<true>, dim3(grid_for(n, BT)), dim3(BT), 0, s, colptr, rowval, n, part, newpos, o);
        CK(cs.finish(&one_based));
    }
    if (nnzB == 0) CK(ensure(h, rv, sizeof(i64)));
    if (!one_based) add_one_launch(s, (i64 *)cp.p, n + 1);
    if (nnzB > 0)
        hipLaunchKernelGGL(blk_gather_k, dim3(grid_for(nnzB, BT)), dim3(BT), 0, s, path ? (const u64 *)pay.p : (const u64 *)nullptr, (u32 *)src.p,
                           (const u64 *)h->nzval.p, (u64 *)nz.p, nnzB);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(s));
    install(p->der.bh, cp, rv, nz, nnzB);
    std::swap(p->der.src, src);
    p->blk_path = path;
    return ESP_OK;
}

}  // namespace

int32_t block_update(esp_precon *p) {
    return derived_update(p, "esp_precon_block", build_b, " (a column of B: the position in the concatenated partitions)");
}

// ldiv! on device vectors (u may be v); sub: u[i] = u[i] - x[i] (simple!'s step on the permuted path)
int32_t block_ldiv_launch(esp_precon *p, const double *v, double *u, bool sub) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    if (n == 0) return ESP_OK;
    CK(derived_follow_stream(p));
    if (p->lup) return lup_solve(p, v, u, sub);  // LUFactorization's panel form: its own gather, depth launches and scatter
    if (p->blk_path == 0) {  // (simple! fuses its `u .-= upd` into the inner kind's own kernels there)
        if (sub) FAIL(h, ESP_ERR_STATE, "esp_precon_block: the identity path has no subtracting ldiv!");
        return precon_ldiv_launch(p->der.inner, v, u);
    }
    const u32 *newpos = (const u32 *)p->blk_new.p;
    double *t = (double *)p->blk_t.p, *sv = (double *)p->blk_s.p;
    const unsigned g = grid_for(n, BT);
    hipLaunchKernelGGL(blk_vec_gather_k, dim3(g), dim3(BT), 0, h->stream, newpos, v, t, n);
    CK(precon_ldiv_launch(p->der.inner, t, sv));
    hipLaunchKernelGGL(blk_vec_scatter_k, dim3(g), dim3(BT), 0, h->stream, newpos, (const double *)sv, u, n, sub);
    return ESP_OK;
}

// ldiv! of the live columns of one chunk (nr <= ESP_MANY_CHUNK; u may be v where ldu == ldv).  The inner solve is iluam_solve_many
// or, for an inner Jacobi / ILU0, the many-column kernels of krylov_many.hip.  The identity path adds no launch; the permuted path
// has one gather and one scatter for the whole chunk
int32_t block_ldiv_many_launch(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, int nr, u32 live) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    live &= all_live(nr);
    if (n == 0 || nr <= 0) return ESP_OK;
    CK(derived_follow_stream(p));
    if (p->lup) FAIL(h, ESP_ERR_STATE, "esp_precon_block: LUFactorization's panel form has its own many-column solve");
    esp_precon *inner = p->der.inner;
    auto inner_solve = [&](const double *src, i64 lds, double *dst, i64 ldd) -> int32_t {
        if (inner->kind == ESP_PRECON_ILUAM) return iluam_solve_many(inner, src, lds, dst, ldd, nr, live);
        return precon_ldiv_chunk_launch(inner, src, lds, dst, ldd, nr, live);
    };
    if (p->blk_path == 0) return inner_solve(v, ldv, u, ldu);
    CK(ensure(h, p->blk_t, sizeof(double) * (size_t)n * ESP_MANY_CHUNK));
    CK(ensure(h, p->blk_s, sizeof(double) * (size_t)n * ESP_MANY_CHUNK));
    const u32 *newpos = (const u32 *)p->blk_new.p;
    double *t = (double *)p->blk_t.p, *sv = (double *)p->blk_s.p;
    const unsigned g = grid_for(n, BT);
    hipLaunchKernelGGL(blk_vec_gather_many_k, dim3(g), dim3(BT), 0, h->stream, newpos, v, ldv, t, n, n, live);
    CK(inner_solve(t, n, sv, n));
    hipLaunchKernelGGL(blk_vec_scatter_many_k, dim3(g), dim3(BT), 0, h->stream, newpos, (const double *)sv, n, u, ldu, n, live);
    HIPCK(h, hipGetLastError());
    return ESP_OK;
}

void block_release(esp_precon *p) {
    if (p->der.inner) (void)esp_precon_destroy(p->der.inner);
    p->der.inner = nullptr;
    if (p->der.bh) (void)esp_destroy(p->der.bh);
    p->der.bh = nullptr;
    for (DevBuf *b : {&p->blk_new, &p->blk_part, &p->der.src, &p->blk_t, &p->blk_s}) release(*b);
}

extern "C" int32_t esp_precon_block_create(esp_handle *h, int32_t inner_kind, int64_t nparts, const int64_t *part_ptr,
                                           const int64_t *part_idx, int32_t on_device, esp_precon **out) {
    if (!h || !out) return ESP_ERR_INVALID;
    *out = nullptr;
    if (inner_kind != ESP_PRECON_JACOBI && inner_kind != ESP_PRECON_ILU0 && inner_kind != ESP_PRECON_ILUAM)
        FAIL(h, ESP_ERR_INVALID, "esp_precon_block_create: inner_kind %d is none of Jacobi, ILU0, ILUAM", inner_kind);
    if (nparts < 0) FAIL(h, ESP_ERR_INVALID, "esp_precon_block_create: nparts < 0");
    CK(precon_check_handle(h, "esp_precon_block_create"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_block_create: a column window / column shard");
    const i64 n = h->n;
    hipStream_t s = h->stream;
    if (!part_ptr || (n > 0 && !part_idx)) FAIL(h, ESP_ERR_INVALID, "esp_precon_block_create: a partition array is NULL");
    // part_ptr on the host: checked here
    std::vector<i64> pp;
    try {
        pp.resize((size_t)nparts + 1);
    } catch (const std::exception &) {  // (empty partitions make any nparts legal: an absurd one must not throw across the C boundary)
        FAIL(h, ESP_ERR_NOMEM, "esp_precon_block_create: no memory for %lld partition pointers", (long long)nparts);
    }
    if (on_device) {
        HIPCK(h, hipMemcpyAsync(pp.data(), part_ptr, sizeof(i64) * pp.size(), hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
    } else {
        memcpy(pp.data(), part_ptr, sizeof(i64) * pp.size());
    }
    if (pp[0] != 0) FAIL(h, ESP_ERR_INVALID, "esp_precon_block_create: part_ptr[0] = %lld, not 0", (long long)pp[0]);
    for (i64 k = 0; k < nparts; k++)
        if (pp[(size_t)k + 1] < pp[(size_t)k])
            FAIL(h, ESP_ERR_INVALID, "esp_precon_block_create: part_ptr decreases at %lld", (long long)(k + 1));
    if (pp[(size_t)nparts] != n)
        FAIL(h, ESP_ERR_INVALID, "esp_precon_block_create: the partitions hold %lld indices, the matrix has %lld (the reference only warns)",
             (long long)pp[(size_t)nparts], (long long)n);
    esp_precon *p = precon_new(h, ESP_PRECON_BLOCK);
    p->der.inner_kind = inner_kind;
    const int32_t st = [&]() -> int32_t {
        Temps tmp;
        DevBuf &dptr = tmp.b[0], &didx = tmp.b[1], &cnt = tmp.b[2], &stat = tmp.b[3];
        CK(ensure(h, p->blk_new, sizeof(u32) * (size_t)std::max<i64>(n, 1)));
        CK(ensure(h, p->blk_part, sizeof(u32) * (size_t)std::max<i64>(n, 1)));
        p->blk_increasing = true;
        if (n > 0) {
            CK(ensure(h, dptr, sizeof(i64) * pp.size()));
            CK(ensure(h, cnt, sizeof(u32) * (size_t)n));
            CK(ensure(h, stat, sizeof(u64) * 4));
            const i64 *idx = part_idx;
            if (!on_device) {
                CK(ensure(h, didx, sizeof(i64) * (size_t)n));
                CK(h2d_pipelined(h, didx.p, part_idx, sizeof(i64) * (size_t)n));
                idx = (const i64 *)didx.p;
            }
            HIPCK(h, hipMemcpyAsync(dptr.p, pp.data(), sizeof(i64) * pp.size(), hipMemcpyHostToDevice, s));
            HIPCK(h, hipMemsetAsync(cnt.p, 0, sizeof(u32) * (size_t)n, s));
            hipLaunchKernelGGL(set_i64_k, dim3(1), dim3(1), 0, s, (i64 *)stat.p, (i64)-1, (i64)-1, (i64)-1, (i64)0);
            hipLaunchKernelGGL(blk_scatter_k, dim3(grid_for(n, BT)), dim3(BT), 0, s, idx, (const i64 *)dptr.p, (i64)nparts, n, (u32 *)p->blk_new.p,
                               (u32 *)p->blk_part.p, (u32 *)cnt.p, (unsigned long long *)stat.p);
            hipLaunchKernelGGL(blk_check_k, dim3(grid_for(n, BT)), dim3(BT), 0, s, (const u32 *)cnt.p, n, (unsigned long long *)stat.p);
            HIPCK(h, hipGetLastError());
            HIPCK(h, hipMemcpyAsync(h->pin_scalar, stat.p, sizeof(u64) * 4, hipMemcpyDeviceToHost, s));
            HIPCK(h, hipStreamSynchronize(s));  // (pp and the caller's arrays are free from here)
            const unsigned long long oor = h->pin_scalar[0], dup = h->pin_scalar[1], miss = h->pin_scalar[2], noninc = h->pin_scalar[3];
            if (oor != ~0ull) {
                i64 bad = 0;
                if (on_device) CK(read_i64(h, part_idx + oor, &bad));
                else bad = part_idx[oor];
                FAIL(h, ESP_ERR_INVALID, "esp_precon_block_create: part_idx[%llu] = %lld is outside 0..%lld", oor, (long long)bad,
                     (long long)(n - 1));
            }
            if (dup != ~0ull)  // (n indices, one of them twice: another one is missing)
                FAIL(h, ESP_ERR_INVALID, "esp_precon_block_create: index %llu appears more than once (and index %llu is in no partition)", dup,
                     miss);
            if (miss != ~0ull) FAIL(h, ESP_ERR_INVALID, "esp_precon_block_create: index %llu is in no partition", miss);
            p->blk_increasing = noninc == 0;
        }
        const int32_t cs = esp_create(n, n, h->device, 0, &p->der.bh);
        if (cs != ESP_OK) FAIL(h, cs, "esp_precon_block_create: the handle of B: %s", esp_last_error(nullptr));
        return block_update(p);
    }();
    return precon_finish(p, st, out);
}

extern "C" int32_t esp_precon_block_matrix(esp_precon *p, esp_handle **b, int32_t *path) {
    if (!p || p->kind != ESP_PRECON_BLOCK) return ESP_ERR_INVALID;
    if (b) *b = p->der.bh;
    if (path) *path = p->blk_path;
    return ESP_OK;
}

extern "C" int32_t esp_debug_block_path(esp_precon *p, int32_t path) {
    if (!p || p->kind != ESP_PRECON_BLOCK || path < 0 || path > 1) return ESP_ERR_INVALID;
    if (p->blk_force != path) p->der.rebuild = true;
    p->blk_force = path;
    return ESP_OK;
}
