// matops.hip -- libesparse_hip: the algebra of an assembled matrix on the device CSC (abstractextendablesparsematrixcsc.jl:224-280):
// A*B (esp_matmul), A+B / A-B (esp_add) and Diagonal scaling (esp_diag_scale).  (See internal.hpp for the map of the units.)
//
// The reference calls Julia's SparseArrays stdlib for all three; its documented behaviour, restated as the assumptions this
// file reproduces bit for bit (tests/matops_model.c restates the same loops literally):
//   A*B (spmatmul, Gustavson): for every column i of B, for every stored B[j,i] in stored order, for every stored A[k,j] in
//     stored order, p = A[k,j]*B[j,i]; the first product that reaches row k is ASSIGNED, later ones are added in the order
//     they arrive.  Every reached row is stored, zeros included; rows sorted.  No FMA (the build passes -ffp-contract=off),
//     no tree reduction, no atomics on values.  That is the rule of an ESP_COO flush into an empty matrix, which is what the
//     generic tier runs.
//   A+B, A-B (map(f, A, B), zero-preserving): per column the two sorted row runs merge; both stored: f(a,b), A only: f(a,0.0),
//     B only: f(0.0,b); a result that compares == 0 is not stored (-0.0 goes too, NaN stays).
//   Diagonal(d)*A, A*Diagonal(d): the pattern of A exactly (computed zeros stay), nzval[p] = d[row]*nzval[p] / d[col]*nzval[p].
//
// A*B in two tiers, chosen per output column by its product count cnt (the sum of nnz(A[:,j]) over the stored B[j,i]):
//   fused   (cnt <= MM_CAP): columns are packed into BINS of contiguous columns (weight cnt+1 each, a bin closes every MM_BIN of
//           weight: <= MM_BIN columns and < MM_BIN + MM_CAP products).  A workgroup forms its bin's products in loop order in
//           LDS, each keyed (local column, row, sequence number), bitonic-sorts the keys, and the head of every (column, row) run
//           folds the run sequentially in sequence order.  Two passes: the count pass (no values) gives every column its
//           number of distinct rows, the write pass recomputes and stores at colptr.  (One pass into scratch would need
//           16 bytes per PRODUCT -- 13 GB at 256^3 -- written and compacted again: more traffic than the recomputation.)
//   generic (the longer columns): their products go, in loop order, as ESP_COO records into the buffer of a scratch handle;
//           its flush folds them, and the columns are copied into place.
// colptr of C comes from the per-column counts of both tiers and one scan; rowval / nzval are allocated at exactly nnz(C).
//
// A+B is a merge path over the two globally (col,row)-sorted entry sequences (A first on equal keys): split points per tile
// of MM_TILE merged elements by binary search, then inside a tile every element finds its merged position and its partner
// by binary search in LDS; equal keys combine (the B element of a pair is dropped), zero results are dropped.  A count pass
// per tile, a scan, a write pass; colptr from the columns of the written entries (a max scan).  No loop runs over a column.
#include "internal.hpp"

namespace {

constexpr int MT = 256;               // threads of every kernel here
constexpr i64 MM_CAP = 2048;          // fused tier: products of one column
constexpr i64 MM_BIN = 1920;          // fused tier: a bin closes every MM_BIN of weight (cnt + 1 per column)
constexpr int MM_SMAX = 4096;         // keys a bin sorts: > MM_BIN - 1 + MM_CAP products (12 bits of sequence number)
constexpr int MM_SEQ_BITS = 12, MM_ROW_BITS = 32;
constexpr int MM_TILE = 1024;         // A+B: merged elements per tile
constexpr int DS_TILE = 2048;         // diagonal scaling: entries per workgroup

struct Csc64 {
    const i64 *colptr, *rowval;
    const double *nzval;
    i64 n, nnz;
};

// the 0-based column of entry p (largest c in [lo, hi] with colptr[c] - 1 <= p)
__device__ __forceinline__ i64 col_of(const i64 *__restrict__ colptr, i64 p, i64 lo, i64 hi) {
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (colptr[mid] - 1 <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// largest q in [lo, hi) with a[q] <= g (a non-decreasing, a[lo] <= g)
__device__ __forceinline__ i64 last_le(const i64 *__restrict__ a, i64 lo, i64 hi, i64 g) {
    hi -= 1;
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (a[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// ---- A*B: product counts, tiers, bins --------------------------------------------------------------------------------
// poff[q] = nnz(A[:, rowB[q]]) (scanned afterwards into the products' sequence offsets)
__global__ void mm_plen_k(const i64 *__restrict__ colptrA, const i64 *__restrict__ rowB, i64 nB, i64 *__restrict__ poff) {
    const i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > nB) return;
    if (q == nB) {
        poff[q] = 0;
        return;
    }
    const i64 j = rowB[q];  // 1-based column of A
    poff[q] = colptrA[j] - colptrA[j - 1];
}
__device__ __forceinline__ bool mm_fused(i64 cnt, int tier) { return tier != 2 && cnt <= MM_CAP; }
// per column i of B: W[i] = fused weight (cnt + 1, or 1), G[i] = generic products (0 for a fused column)
__global__ void mm_cols_k(const i64 *__restrict__ colptrB, const i64 *__restrict__ poff, i64 n, int tier, i64 *__restrict__ W,
                          i64 *__restrict__ G) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        W[i] = 0;
        G[i] = 0;
        return;
    }
    const i64 cnt = poff[colptrB[i + 1] - 1] - poff[colptrB[i] - 1];
    const bool f = mm_fused(cnt, tier);
    W[i] = f ? cnt + 1 : 1;
    G[i] = f ? 0 : cnt;
}
// binstart[b] = first column of bin b (bin of column i: W[i] / MM_BIN; a column heavier than a bin skips bins, which stay empty)
__global__ void mm_bins_k(const i64 *__restrict__ W, i64 n, i64 nbins, i64 *__restrict__ binstart) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const i64 bi = i < n ? W[i] / MM_BIN : nbins;
    const i64 bp = i == 0 ? -1 : W[i - 1] / MM_BIN;
    for (i64 b = bp + 1; b <= bi; b++) binstart[b] = i;
}

// ---- A*B fused tier: one workgroup per bin ---------------------------------------------------------------------------
// key = local column << 44 | 0-based row << 12 | sequence number inside the bin (loop order)
template <bool WRITE>
__global__ __launch_bounds__(MT) void mm_bin_k(Csc64 A, Csc64 B, const i64 *__restrict__ poff, const i64 *__restrict__ W,
                                               const i64 *__restrict__ binstart, i64 *__restrict__ ccount,
                                               const i64 *__restrict__ colptrC, i64 *__restrict__ rowC, double *__restrict__ valC) {
    __shared__ u64 skey[MM_SMAX];
    __shared__ double sval[WRITE ? MM_SMAX : 1];
    __shared__ u32 scol[MM_BIN + 1];  // local product start of every column; then counts (count pass) / first run rank (write pass)
    __shared__ u32 swave[MT / 64];
    const i64 c0 = binstart[blockIdx.x], c1 = binstart[blockIdx.x + 1];
    const int ncol = (int)(c1 - c0);
    if (ncol == 0) return;
    const i64 base = W[c0];
    for (int k = threadIdx.x; k <= ncol; k += MT) scol[k] = (u32)(W[c0 + k] - base - k);
    __syncthreads();
    const int P = (int)scol[ncol];
    if (P == 0) {
        if (!WRITE)
            for (int k = threadIdx.x; k < ncol; k += MT) ccount[c0 + k] = 0;
        return;
    }
    int S = 2;
    while (S < P) S <<= 1;
    // 1. the products in loop order
    for (int t = threadIdx.x; t < S; t += MT) {
        u64 key = ~0ull;
        if (t < P) {
            int lo = 0, hi = ncol - 1;  // the last column whose products start at or before t
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((int)scol[mid] <= t) lo = mid;
                else hi = mid - 1;
            }
            const i64 i = c0 + lo;
            const i64 qs = B.colptr[i] - 1, qe = B.colptr[i + 1] - 1;
            const i64 g = poff[qs] + (t - (int)scol[lo]);
            const i64 q = last_le(poff, qs, qe, g);
            const i64 apos = A.colptr[B.rowval[q] - 1] - 1 + (g - poff[q]);
            key = ((u64)lo << (MM_ROW_BITS + MM_SEQ_BITS)) | ((u64)(A.rowval[apos] - 1) << MM_SEQ_BITS) | (u64)t;
            if (WRITE) sval[t] = A.nzval[apos] * B.nzval[q];
        }
        skey[t] = key;
    }
    __syncthreads();
    // 2. bitonic sort (keys are distinct: the sequence number is part of them)
    for (int size = 2; size <= S; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int x = threadIdx.x; x < (S >> 1); x += MT) {
                const int lo = 2 * stride * (x / stride) + (x % stride), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const u64 a = skey[lo], b = skey[hi];
                if ((a > b) == up) {
                    skey[lo] = b;
                    skey[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    // 3. run heads: every thread owns `per` consecutive sorted positions
    const int per = (P + MT - 1) / MT;
    const int p0 = threadIdx.x * per, p1 = min(P, p0 + per);
    auto head = [&](int p) { return p == 0 || (skey[p] >> MM_SEQ_BITS) != (skey[p - 1] >> MM_SEQ_BITS); };
    if (!WRITE) {
        for (int k = threadIdx.x; k < ncol; k += MT) scol[k] = 0;
        __syncthreads();
        for (int p = p0; p < p1; p++)
            if (head(p)) atomicAdd(&scol[skey[p] >> (MM_ROW_BITS + MM_SEQ_BITS)], 1u);
        __syncthreads();
        for (int k = threadIdx.x; k < ncol; k += MT) ccount[c0 + k] = (i64)scol[k];
        return;
    }
    u32 nh = 0;
    for (int p = p0; p < p1; p++) nh += head(p) ? 1u : 0u;
    u32 tot;
    u32 r = espscan::block_exclusive<u32, false>(nh, swave, &tot);
    // rank of every column's first run (its first sorted position is a head with a new column)
    u32 rr = r;
    for (int p = p0; p < p1; p++) {
        if (!head(p)) continue;
        const u32 col = (u32)(skey[p] >> (MM_ROW_BITS + MM_SEQ_BITS));
        if (p == 0 || (u32)(skey[p - 1] >> (MM_ROW_BITS + MM_SEQ_BITS)) != col) scol[col] = rr;
        rr++;
    }
    __syncthreads();
    // 4. every head folds its run in sequence order: the first product as it is, the others added one by one
    rr = r;
    for (int p = p0; p < p1; p++) {
        if (!head(p)) continue;
        const u64 k = skey[p];
        const u32 col = (u32)(k >> (MM_ROW_BITS + MM_SEQ_BITS));
        double v = sval[k & ((1u << MM_SEQ_BITS) - 1)];
        for (int e = p + 1; e < P && (skey[e] >> MM_SEQ_BITS) == (k >> MM_SEQ_BITS); e++)
            v = v + sval[skey[e] & ((1u << MM_SEQ_BITS) - 1)];
        const i64 dst = colptrC[c0 + col] - 1 + (i64)(rr - scol[col]);
        rowC[dst] = (i64)((k >> MM_SEQ_BITS) & 0xFFFFFFFFull) + 1;
        valC[dst] = v;
        rr++;
    }
}

// ---- A*B generic tier -------------------------------------------------------------------------------------------------
// product g of the generic columns (in loop order) -> an ESP_COO record of the scratch handle
__global__ void mm_expand_k(Csc64 A, Csc64 B, const i64 *__restrict__ poff, const i64 *__restrict__ G, i64 n, i64 total, KeyLayout L,
                            u64 *__restrict__ keys, double *__restrict__ vals) {
    const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const i64 i = last_le(G, 0, n, g);  // (a fused column has G[i+1] == G[i]: never the last one <= g with products)
    const i64 qs = B.colptr[i] - 1, qe = B.colptr[i + 1] - 1;
    const i64 pg = poff[qs] + (g - G[i]);
    const i64 q = last_le(poff, qs, qe, pg);
    const i64 apos = A.colptr[B.rowval[q] - 1] - 1 + (pg - poff[q]);
    keys[g] = esp_pack(L, A.rowval[apos], i + 1, ESP_COO);
    vals[g] = A.nzval[apos] * B.nzval[q];
}
// per column: distinct rows of the tier that ran it (scp: the scratch handle's colptr, or nullptr)
__global__ void mm_count_k(const i64 *__restrict__ colptrB, const i64 *__restrict__ poff, const i64 *__restrict__ ccount,
                           const i64 *__restrict__ scp, i64 n, int tier, i64 *__restrict__ cp) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        cp[i] = 0;
        return;
    }
    const i64 cnt = poff[colptrB[i + 1] - 1] - poff[colptrB[i] - 1];
    cp[i] = mm_fused(cnt, tier) ? ccount[i] : scp ? scp[i + 1] - scp[i] : 0;  // (no scratch: every generic column is empty)
}
__global__ void add_one_k(i64 *__restrict__ p, i64 n) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] += 1;
}
// the scratch handle's columns into place
__global__ void mm_place_k(const i64 *__restrict__ scp, const i64 *__restrict__ srow, const double *__restrict__ sval, i64 n, i64 snnz,
                           const i64 *__restrict__ colptrC, i64 *__restrict__ rowC, double *__restrict__ valC) {
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= snnz) return;
    const i64 c = col_of(scp, p, 0, n - 1);
    const i64 dst = colptrC[c] - 1 + (p - (scp[c] - 1));
    rowC[dst] = srow[p];
    valC[dst] = sval[p];
}

// ---- A+B: merge path ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 add_key(const Csc64 &X, i64 p, i64 clo, i64 chi) {
    return ((u64)col_of(X.colptr, p, clo, chi) << 32) | (u64)(X.rowval[p] - 1);
}
// split[t] = A elements among the first t * MM_TILE merged ones (A first on equal keys)
__global__ void add_split_k(Csc64 A, Csc64 B, i64 ntiles, i64 *__restrict__ split) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > ntiles) return;
    const i64 d = min(t * MM_TILE, A.nnz + B.nnz);
    i64 lo = max((i64)0, d - B.nnz), hi = min(d, A.nnz);
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (add_key(A, mid, 0, A.n - 1) <= add_key(B, d - 1 - mid, 0, B.n - 1)) lo = mid + 1;
        else hi = mid;
    }
    split[t] = lo;
}
__device__ __forceinline__ i64 lower_bound_lds(const u64 *a, i64 n, u64 k) {  // first index with a[i] >= k
    i64 lo = 0, hi = n;
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (a[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ i64 upper_bound_lds(const u64 *a, i64 n, u64 k) {  // first index with a[i] > k
    i64 lo = 0, hi = n;
    while (lo < hi) {
        const i64 mid = (lo + hi) >> 1;
        if (a[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// one tile: count pass (tcount[t] = stored results) or write pass (at toff[t]; ocol = their 0-based columns)
template <bool WRITE>
__global__ __launch_bounds__(MT) void add_tile_k(Csc64 A, Csc64 B, int op, const i64 *__restrict__ split, i64 *__restrict__ tcount,
                                                 const i64 *__restrict__ toff, i64 *__restrict__ rowC, double *__restrict__ valC,
                                                 u32 *__restrict__ ocol) {
    __shared__ u64 ska[MM_TILE + 2], skb[MM_TILE + 1];
    __shared__ u32 sflag[MM_TILE];
    __shared__ i64 srow[WRITE ? MM_TILE : 1];
    __shared__ double sres[WRITE ? MM_TILE : 1];
    __shared__ u32 scolm[WRITE ? MM_TILE : 1];
    __shared__ i64 scr[4];
    __shared__ u32 swave[MT / 64];
    const i64 t = blockIdx.x;
    const i64 d0 = t * MM_TILE, d1 = min(d0 + MM_TILE, A.nnz + B.nnz);
    const i64 i0 = split[t], i1 = split[t + 1], j0 = d0 - i0, j1 = d1 - i1;
    const int na = (int)(i1 - i0), nb = (int)(j1 - j0);
    // A elements [la, ha] (one in front of the tile for a pair split by its start), B elements [j0, hb] (one behind it)
    const i64 la = i0 > 0 ? i0 - 1 : 0, ha = min(i1, A.nnz - 1), hb = min(j1, B.nnz - 1);
    const int nla = A.nnz > 0 ? (int)(ha - la + 1) : 0, nlb = B.nnz > 0 && j0 <= hb ? (int)(hb - j0 + 1) : 0;
    if (threadIdx.x == 0 && nla > 0) scr[0] = col_of(A.colptr, la, 0, A.n - 1);
    if (threadIdx.x == 1 && nla > 0) scr[1] = col_of(A.colptr, ha, 0, A.n - 1);
    if (threadIdx.x == 2 && nlb > 0) scr[2] = col_of(B.colptr, j0, 0, B.n - 1);
    if (threadIdx.x == 3 && nlb > 0) scr[3] = col_of(B.colptr, hb, 0, B.n - 1);
    for (int k = threadIdx.x; k < MM_TILE; k += MT) sflag[k] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < nla; k += MT) ska[k] = add_key(A, la + k, scr[0], scr[1]);
    for (int k = threadIdx.x; k < nlb; k += MT) skb[k] = add_key(B, j0 + k, scr[2], scr[3]);
    __syncthreads();
    const int oa = (int)(i0 - la);  // A element i0 sits at ska[oa]
    const u64 *ta = ska + oa;
    for (int e = threadIdx.x; e < na + nb; e += MT) {
        double v;
        i64 mp;
        u64 key;
        bool emit = true;
        if (e < na) {
            key = ta[e];
            const i64 lb = lower_bound_lds(skb, nb, key);
            mp = e + lb;
            const double a = A.nzval[i0 + e];
            const bool pair = lb < nlb && skb[lb] == key;  // (lb == nb: the partner may be the B element behind the tile)
            v = pair ? (op == ESP_OP_SUB ? a - B.nzval[j0 + lb] : a + B.nzval[j0 + lb]) : (op == ESP_OP_SUB ? a - 0.0 : a + 0.0);
        } else {
            const int f = e - na;
            key = skb[f];
            const i64 ub = upper_bound_lds(ta, na, key);
            mp = f + ub;
            emit = !(ub > 0 ? ta[ub - 1] == key : (oa == 1 && ska[0] == key));  // the B half of a pair: its A element speaks
            const double b = B.nzval[j0 + f];
            v = op == ESP_OP_SUB ? 0.0 - b : 0.0 + b;
        }
        const bool keep = emit && !(v == 0.0);
        sflag[mp] = keep ? 1u : 0u;
        if (WRITE && keep) {
            srow[mp] = (i64)(key & 0xFFFFFFFFull) + 1;
            sres[mp] = v;
            scolm[mp] = (u32)(key >> 32);
        }
    }
    __syncthreads();
    // compaction in merged order: every thread owns MM_TILE / MT consecutive positions
    constexpr int PER = MM_TILE / MT;
    const int p0 = threadIdx.x * PER;
    u32 nk = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) nk += sflag[p0 + k];
    u32 tot;
    u32 r = espscan::block_exclusive<u32, false>(nk, swave, &tot);
    if (!WRITE) {
        if (threadIdx.x == 0) tcount[t] = (i64)tot;
        return;
    }
    const i64 o0 = toff[t];
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int p = p0 + k;
        if (!sflag[p]) continue;
        const i64 o = o0 + r;
        rowC[o] = srow[p];
        valC[o] = sres[p];
        ocol[o] = scolm[p];
        r++;
    }
}
// Z[c] = number of results in the columns <= c, written by the last result of column c (colptr = 1 + exclusive max scan)
__global__ void add_colend_k(const u32 *__restrict__ ocol, i64 nnz, i64 *__restrict__ Z) {
    const i64 o = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nnz) return;
    if (o == nnz - 1 || ocol[o + 1] != ocol[o]) Z[ocol[o]] = o + 1;
}

// ---- Diagonal scaling: one pass writes the pattern (out of place) and the scaled values ------------------------------------
template <int SIDE, bool COPY>
// (in place, valC is A.nzval: no __restrict__ on it)
__global__ __launch_bounds__(MT) void diag_scale_k(Csc64 A, const double *__restrict__ d, i64 *__restrict__ rowC, double *valC) {
    __shared__ i64 scr[2];
    const i64 p0 = (i64)blockIdx.x * DS_TILE, p1 = min(p0 + DS_TILE, A.nnz);
    if (SIDE == 1) {
        if (threadIdx.x == 0) scr[0] = col_of(A.colptr, p0, 0, A.n - 1);
        if (threadIdx.x == 1) scr[1] = col_of(A.colptr, p1 - 1, 0, A.n - 1);
        __syncthreads();
    }
    for (i64 p = p0 + threadIdx.x; p < p1; p += MT) {
        const i64 r = A.rowval[p];
        const double s = SIDE == 0 ? d[r - 1] : d[col_of(A.colptr, p, scr[0], scr[1])];
        valC[p] = s * A.nzval[p];
        if (COPY) rowC[p] = r;
    }
}

}  // namespace

// (check_operand, install and read_i64 are shared with linalg.hip: internal.hpp)
int32_t check_operand(esp_handle *h, const char *what) {
    if (h->count != 0) FAIL(h, ESP_ERR_STATE, "%s: pending entries (flush first, as sparse(A) does)", what);
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "%s: a column window / column shard as an operand", what);
    if (h->m > 0xFFFFFFFFll || h->n > 0xFFFFFFFFll) FAIL(h, ESP_ERR_UNSUPPORTED, "%s: dimensions beyond 2^32", what);
    (void)hipSetDevice(h->device);
    if (!h->csc_valid) CK(init_empty_csc(h));
    CK(fix_tail(h));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}
namespace {
Csc64 csc_of(const esp_handle *h) {
    return Csc64{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (const double *)h->nzval.p, h->n, h->nnz};
}
}  // namespace
// c takes the new CSC (a pattern change, as a flush that rebuilds leaves it)
void install(esp_handle *c, DevBuf &cp, DevBuf &rv, DevBuf &nz, i64 nnz) {
    drop_kept(c);  // (other buffers from here on)
    std::swap(c->colptr, cp);
    std::swap(c->rowval, rv);
    std::swap(c->nzval, nz);
    c->nnz = nnz;
    c->pattern_version++, c->values_version++;
    c->csc_valid = true;
    c->win_excl = false;
    c->tail_stale = false;
    c->ones_pending = false;
}
void add_one_launch(hipStream_t s, i64 *p, i64 n) { hipLaunchKernelGGL(add_one_k, dim3(grid_for(n, MT)), dim3(MT), 0, s, p, n); }
int32_t read_i64(esp_handle *h, const i64 *d_src, i64 *out) {
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, d_src, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    *out = (i64)h->pin_scalar[0];
    return ESP_OK;
}

extern "C" int32_t esp_device(const esp_handle *h, int32_t *device) {
    if (!h || !device) return ESP_ERR_INVALID;
    *device = h->device;
    return ESP_OK;
}

extern "C" int32_t esp_debug_matmul_tier(esp_handle *c, int32_t tier) {
    if (!c || tier < 0 || tier > 2) return ESP_ERR_INVALID;
    c->matmul_tier = tier;
    return ESP_OK;
}

extern "C" int32_t esp_matmul(esp_handle *a, esp_handle *b, esp_handle *c, int64_t *nnz_out) {
    if (!a || !b || !c) return ESP_ERR_INVALID;
    if (c == a || c == b) FAIL(c, ESP_ERR_INVALID, "esp_matmul: the result handle must not be an operand");
    if (a->device != b->device || a->device != c->device) FAIL(c, ESP_ERR_INVALID, "esp_matmul: operands on different devices");
    CK(check_operand(a, "esp_matmul"));
    if (b != a) CK(check_operand(b, "esp_matmul"));
    CK(check_operand(c, "esp_matmul"));
    if (a->n != b->m) FAIL(c, ESP_ERR_INVALID, "esp_matmul: DimensionMismatch (A has %lld columns, B %lld rows)", (long long)a->n, (long long)b->m);
    if (c->m != a->m || c->n != b->n) FAIL(c, ESP_ERR_INVALID, "esp_matmul: the result handle is not %lld x %lld", (long long)a->m, (long long)b->n);
    esp_handle *h = c;
    hipStream_t s = h->stream;
    const Csc64 A = csc_of(a), B = csc_of(b);
    const i64 n = B.n, nB = B.nnz;
    const int tier = c->matmul_tier;
    Temps tmp;
    DevBuf &poff = tmp.b[0], &W = tmp.b[1], &G = tmp.b[2], &bins = tmp.b[3], &ccount = tmp.b[4], &ws = tmp.b[5];
    DevBuf &cp = tmp.b[6], &rv = tmp.b[7], &nz = tmp.b[8];
    int l = 0;
    CK(ensure(h, poff, sizeof(i64) * (size_t)(nB + 1)));
    CK(ensure(h, W, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, G, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, ccount, sizeof(i64) * (size_t)std::max<i64>(n, 1)));
    CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
    // sequence offsets of the products, tiers, bins
    hipLaunchKernelGGL(mm_plen_k, dim3(grid_for(nB + 1, MT)), dim3(MT), 0, s, A.colptr, B.rowval, nB, (i64 *)poff.p);
    CK(scan_inplace<i64, false>(h, (i64 *)poff.p, nB + 1, ws, &l));
    hipLaunchKernelGGL(mm_cols_k, dim3(grid_for(n + 1, MT)), dim3(MT), 0, s, B.colptr, (const i64 *)poff.p, n, tier, (i64 *)W.p, (i64 *)G.p);
    CK(scan_inplace<i64, false>(h, (i64 *)W.p, n + 1, ws, &l));
    CK(scan_inplace<i64, false>(h, (i64 *)G.p, n + 1, ws, &l));
    HIPCK(h, hipGetLastError());
    i64 wtot = 0, gtot = 0;
    CK(read_i64(h, (const i64 *)W.p + n, &wtot));
    CK(read_i64(h, (const i64 *)G.p + n, &gtot));
    const i64 nbins = ceil_div<i64>(wtot, MM_BIN);
    CK(ensure(h, bins, sizeof(i64) * (size_t)(nbins + 1)));
    hipLaunchKernelGGL(mm_bins_k, dim3(grid_for(n + 1, MT)), dim3(MT), 0, s, (const i64 *)W.p, n, nbins, (i64 *)bins.p);
    // fused tier, count pass
    if (nbins > 0)
        hipLaunchKernelGGL(mm_bin_k<false>, dim3((unsigned)nbins), dim3(MT), 0, s, A, B, (const i64 *)poff.p, (const i64 *)W.p,
                           (const i64 *)bins.p, (i64 *)ccount.p, (const i64 *)nullptr, (i64 *)nullptr, (double *)nullptr);
    HIPCK(h, hipGetLastError());
    // generic tier: the products as ESP_COO records of a scratch handle, folded by its flush
    ScratchFlush sf(h, "esp_matmul");
    DevBuf &scp = tmp.b[9], &srv = tmp.b[10], &snz = tmp.b[11];
    if (gtot > 0) {
        CK(sf.open(a->m, n, gtot));
        HIPCK(h, hipStreamSynchronize(s));
        hipLaunchKernelGGL(mm_expand_k, dim3(grid_for(gtot, MT)), dim3(MT), 0, sf.stream(), A, B, (const i64 *)poff.p, (const i64 *)G.p, n, gtot,
                           sf.L(), sf.keys(), (double *)sf.vals());
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipStreamSynchronize(sf.stream()));
        CK(sf.flush(-1));  // (products of one position fold: no count to expect)
        sf.take(scp, srv, snz);
    }
    // colptr of C
    hipLaunchKernelGGL(mm_count_k, dim3(grid_for(n + 1, MT)), dim3(MT), 0, s, B.colptr, (const i64 *)poff.p, (const i64 *)ccount.p, (const i64 *)scp.p, n,
                       tier, (i64 *)cp.p);
    CK(scan_inplace<i64, false>(h, (i64 *)cp.p, n + 1, ws, &l));
    add_one_launch(s, (i64 *)cp.p, n + 1);
    HIPCK(h, hipGetLastError());
    i64 nnzC = 0;
    CK(read_i64(h, (const i64 *)cp.p + n, &nnzC));
    nnzC -= 1;
    CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(nnzC, 1)));
    CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nnzC, 1)));
    if (nbins > 0)
        hipLaunchKernelGGL(mm_bin_k<true>, dim3((unsigned)nbins), dim3(MT), 0, s, A, B, (const i64 *)poff.p, (const i64 *)W.p,
                           (const i64 *)bins.p, (i64 *)nullptr, (const i64 *)cp.p, (i64 *)rv.p, (double *)nz.p);
    if (sf.nnz() > 0)
        hipLaunchKernelGGL(mm_place_k, dim3(grid_for(sf.nnz(), MT)), dim3(MT), 0, s, (const i64 *)scp.p, (const i64 *)srv.p,
                           (const double *)snz.p, n, sf.nnz(), (const i64 *)cp.p, (i64 *)rv.p, (double *)nz.p);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(s));
    install(c, cp, rv, nz, nnzC);
    if (nnz_out) *nnz_out = nnzC;
    return ESP_OK;
}

extern "C" int32_t esp_add(esp_handle *a, esp_handle *b, int32_t op, esp_handle *c, int64_t *nnz_out) {
    if (!a || !b || !c || (op != ESP_OP_ADD && op != ESP_OP_SUB)) return ESP_ERR_INVALID;
    if (c == a || c == b) FAIL(c, ESP_ERR_INVALID, "esp_add: the result handle must not be an operand");
    if (a->device != b->device || a->device != c->device) FAIL(c, ESP_ERR_INVALID, "esp_add: operands on different devices");
    CK(check_operand(a, "esp_add"));
    if (b != a) CK(check_operand(b, "esp_add"));
    CK(check_operand(c, "esp_add"));
    if (a->m != b->m || a->n != b->n) FAIL(c, ESP_ERR_INVALID, "esp_add: DimensionMismatch (%lld x %lld and %lld x %lld)", (long long)a->m,
                                           (long long)a->n, (long long)b->m, (long long)b->n);
    if (c->m != a->m || c->n != a->n) FAIL(c, ESP_ERR_INVALID, "esp_add: the result handle is not %lld x %lld", (long long)a->m, (long long)a->n);
    esp_handle *h = c;
    hipStream_t s = h->stream;
    const Csc64 A = csc_of(a), B = csc_of(b);
    const i64 n = A.n, tot = A.nnz + B.nnz, ntiles = ceil_div<i64>(tot, MM_TILE);
    Temps tmp;
    DevBuf &split = tmp.b[0], &tcount = tmp.b[1], &ocol = tmp.b[2], &ws = tmp.b[3], &cp = tmp.b[6], &rv = tmp.b[7], &nz = tmp.b[8];
    int l = 0;
    CK(ensure(h, split, sizeof(i64) * (size_t)(ntiles + 1)));
    CK(ensure(h, tcount, sizeof(i64) * (size_t)(ntiles + 1)));
    CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
    i64 nnzC = 0;
    if (ntiles > 0) {
        hipLaunchKernelGGL(add_split_k, dim3(grid_for(ntiles + 1, MT)), dim3(MT), 0, s, A, B, ntiles, (i64 *)split.p);
        hipLaunchKernelGGL(add_tile_k<false>, dim3((unsigned)ntiles), dim3(MT), 0, s, A, B, op, (const i64 *)split.p, (i64 *)tcount.p,
                           (const i64 *)nullptr, (i64 *)nullptr, (double *)nullptr, (u32 *)nullptr);
        HIPCK(h, hipMemsetAsync((i64 *)tcount.p + ntiles, 0, 8, s));
        CK(scan_inplace<i64, false>(h, (i64 *)tcount.p, ntiles + 1, ws, &l));
        HIPCK(h, hipGetLastError());
        CK(read_i64(h, (const i64 *)tcount.p + ntiles, &nnzC));
    }
    CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(nnzC, 1)));
    CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nnzC, 1)));
    CK(ensure(h, ocol, sizeof(u32) * (size_t)std::max<i64>(nnzC, 1)));
    HIPCK(h, hipMemsetAsync(cp.p, 0, sizeof(i64) * (size_t)(n + 1), s));
    if (nnzC > 0) {
        hipLaunchKernelGGL(add_tile_k<true>, dim3((unsigned)ntiles), dim3(MT), 0, s, A, B, op, (const i64 *)split.p, (i64 *)nullptr,
                           (const i64 *)tcount.p, (i64 *)rv.p, (double *)nz.p, (u32 *)ocol.p);
        hipLaunchKernelGGL(add_colend_k, dim3(grid_for(nnzC, MT)), dim3(MT), 0, s, (const u32 *)ocol.p, nnzC, (i64 *)cp.p);
        CK(scan_inplace<i64, true>(h, (i64 *)cp.p, n + 1, ws, &l));
    }
    add_one_launch(s, (i64 *)cp.p, n + 1);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(s));
    install(c, cp, rv, nz, nnzC);
    if (nnz_out) *nnz_out = nnzC;
    return ESP_OK;
}

extern "C" int32_t esp_diag_scale(esp_handle *a, const double *d, int32_t side, int32_t on_device, esp_handle *c) {
    if (!a || !d || !c || (side != 0 && side != 1)) return ESP_ERR_INVALID;
    if (a->device != c->device) FAIL(c, ESP_ERR_INVALID, "esp_diag_scale: operands on different devices");
    CK(check_operand(a, "esp_diag_scale"));
    if (c != a) {
        CK(check_operand(c, "esp_diag_scale"));
        if (c->m != a->m || c->n != a->n) FAIL(c, ESP_ERR_INVALID, "esp_diag_scale: the result handle is not %lld x %lld", (long long)a->m, (long long)a->n);
    }
    esp_handle *h = c;
    hipStream_t s = h->stream;
    const Csc64 A = csc_of(a);
    const i64 nd = side == 0 ? a->m : a->n;
    Temps tmp;
    DevBuf &dd = tmp.b[0], &cp = tmp.b[6], &rv = tmp.b[7], &nz = tmp.b[8];
    const double *dp = d;
    if (!on_device) {
        CK(ensure(h, dd, sizeof(double) * (size_t)std::max<i64>(nd, 1)));
        if (nd > 0) CK(h2d_pipelined(h, dd.p, d, sizeof(double) * (size_t)nd));
        dp = (const double *)dd.p;
    }
    const bool inplace = c == a;
    i64 *rowC = nullptr;
    double *valC = (double *)a->nzval.p;
    if (!inplace) {
        CK(ensure(h, cp, sizeof(i64) * (size_t)(A.n + 1)));
        CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(A.nnz, 1)));
        CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(A.nnz, 1)));
        HIPCK(h, hipMemcpyAsync(cp.p, A.colptr, sizeof(i64) * (size_t)(A.n + 1), hipMemcpyDeviceToDevice, s));
        rowC = (i64 *)rv.p;
        valC = (double *)nz.p;
    }
    if (A.nnz > 0) {
        const dim3 g(grid_for(A.nnz, DS_TILE));
        if (side == 0 && inplace) hipLaunchKernelGGL((diag_scale_k<0, false>), g, dim3(MT), 0, s, A, dp, rowC, valC);
        else if (side == 0) hipLaunchKernelGGL((diag_scale_k<0, true>), g, dim3(MT), 0, s, A, dp, rowC, valC);
        else if (inplace) hipLaunchKernelGGL((diag_scale_k<1, false>), g, dim3(MT), 0, s, A, dp, rowC, valC);
        else hipLaunchKernelGGL((diag_scale_k<1, true>), g, dim3(MT), 0, s, A, dp, rowC, valC);
    }
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(s));
    if (inplace) c->values_version++;
    else install(c, cp, rv, nz, A.nnz);
    return ESP_OK;
}
