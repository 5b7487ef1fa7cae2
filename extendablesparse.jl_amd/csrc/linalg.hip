// linalg.hip -- libesparse_hip: transpose (esp_transpose), transpose(A)*x (esp_mul_transpose), issymmetric (esp_issymmetric),
// opnorm (esp_opnorm) and norm (esp_norm) of an assembled matrix on the device CSC.  The reference forwards norm / opnorm /
// issymmetric to SparseArrays (abstractextendablesparsematrixcsc.jl:188-217) and sketches the transpose as
// ExtendableSparseMatrixCSC(transpose(sparse(A))) (extendable.jl:107-116).  (See internal.hpp for the map of the units.)
//
// SparseArrays' documented behaviour, restated as the assumptions this file reproduces (tests/linalg_model.c restates the loops):
//   copy(transpose(A))  halfperm!: every stored entry, explicit zeros included, rows ascending in every column; pure data
//                       movement (-0.0 and NaN payloads kept)
//   transpose(A)*x      _At_or_Ac_mul_B!: r[j] = 0.0; tmp = 0.0; tmp += nzval[k]*x[rowval[k]] over column j in stored order;
//                       r[j] += tmp.  No FMA (the build passes -ffp-contract=off), no reordered sums.
//   issymmetric(A)      issymmetric(Matrix(A)): square, and every stored value v at (i,j) that is not == 0 equals A[j,i]
//                       (0.0 where not stored); a stored zero of either sign counts as absent, a NaN anywhere gives false
//   opnorm(A, 1 / Inf)  opnorm(::AbstractSparseMatrixCSC, p) branch by branch; its general loops: the max over columns of the
//                       column's sum of |v| in stored order, the max over rows of the row's sum in column order; max
//                       propagates NaN.  opnorm(A, 2) with m, n > 1 is refused, as SparseArrays refuses it.
//   norm(A, p)          norm(nonzeros(A), p) over the stored values
//
// The transpose has two paths (esp_debug_transpose_path on the result handle):
//   1 generic    A's entries go, keys swapped, as ESP_COO records into the append buffer of a scratch handle of size (n, m),
//                which is flushed from its empty CSC: the keys are unique, nothing folds, every value is assigned verbatim
//                (fold.hpp).  c takes the scratch handle's CSC over; everything else the flush grew is destroyed with it.
//   2 counting   C's column counts are A's row counts (u32 atomics), one scan gives C's colptr; a scatter puts every entry at
//                its column's cursor (u32 atomics: any order inside a column), and every column is then sorted by row -- one
//                lane in registers (<= TP_LANE entries) or one workgroup in LDS (<= TP_BLOCK).  Rows are unique inside a column,
//                so the result does not depend on the order of the scatter.  A row of A longer than TP_BLOCK: the generic path.
//   Automatic takes the counting path.  Nothing the call allocates outlives it: c keeps its new CSC only.
// Reductions run over a fixed grid, with partial results per workgroup combined in a fixed order: bit-identical run to run.
// The maxima are integer atomicMax on the bit patterns of non-negative doubles (a NaN, after fabs, sorts above +Inf), the
// counts integer atomicAdd: one atomic per workgroup, no float atomics.
#include "internal.hpp"

namespace {

constexpr int MT = 256;            // threads of every kernel here
constexpr int TP_TILE = 2048;      // entries per workgroup of the entry-parallel kernels
constexpr int TP_LANE = 32;        // counting path: a column of at most this many entries is sorted by one lane
constexpr int TP_BLOCK = 4096;     // ... at most this many by one workgroup in LDS (local index: TP_IDX_BITS)
constexpr int TP_IDX_BITS = 12;
constexpr int MV_LONG = 64;        // transpose(A)*x: a longer column is folded by its whole wave
constexpr int RED_GRID = 1024;     // norm: workgroups of a reduction (at most)
constexpr i64 MAX_GRID = 2048;     // grid-stride kernels that end in one atomicMax per workgroup (one word takes ~90 atomics/us)
constexpr u64 ABS_MASK = 0x7FFFFFFFFFFFFFFFull, INF_BITS = 0x7FF0000000000000ull;

struct Csc64 {
    const i64 *colptr, *rowval;
    const double *nzval;
    i64 n, nnz;
};
Csc64 csc_of(const esp_handle *h) {
    return Csc64{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (const double *)h->nzval.p, h->n, h->nnz};
}

// the 0-based column of entry p (largest c in [lo, hi] with colptr[c] - 1 <= p)
__device__ __forceinline__ i64 col_of(const i64 *__restrict__ colptr, i64 p, i64 lo, i64 hi) {
    while (lo < hi) {
        const i64 mid = (lo + hi + 1) >> 1;
        if (colptr[mid] - 1 <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// every thread of the workgroup gets op over all its threads' v: a butterfly in every wave, then the waves in order (sw: MT / 64)
template <typename T, typename F>
__device__ __forceinline__ T block_reduce(T v, F op, T *sw) {
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = sw[0];
    for (int w = 1; w < MT / 64; w++) r = op(r, sw[w]);
    return r;
}
struct MaxU64 {
    __device__ u64 operator()(u64 a, u64 b) const { return a > b ? a : b; }
};
struct MinU64 {
    __device__ u64 operator()(u64 a, u64 b) const { return a < b ? a : b; }
};
struct AddU64 {
    __device__ u64 operator()(u64 a, u64 b) const { return a + b; }
};
struct AddF64 {
    __device__ double operator()(double a, double b) const { return a + b; }
};

// ---- transpose, generic path: A's entries as ESP_COO records (row <- column, column <- row) --------------------------------
__global__ __launch_bounds__(MT) void tp_expand_k(Csc64 A, KeyLayout L, u64 *__restrict__ keys, u64 *__restrict__ vals) {
    __shared__ i64 scr[2];
    const i64 p0 = (i64)blockIdx.x * TP_TILE, p1 = min(p0 + TP_TILE, A.nnz);
    if (threadIdx.x == 0) scr[0] = col_of(A.colptr, p0, 0, A.n - 1);
    if (threadIdx.x == 1) scr[1] = col_of(A.colptr, p1 - 1, 0, A.n - 1);
    __syncthreads();
    const u64 *__restrict__ v = (const u64 *)A.nzval;  // (the bits, moved as they are)
    for (i64 p = p0 + threadIdx.x; p < p1; p += MT) {
        const i64 j = col_of(A.colptr, p, scr[0], scr[1]);
        keys[p] = esp_pack(L, j + 1, A.rowval[p], ESP_COO);
        vals[p] = v[p];
    }
}

// ---- transpose, counting path ------------------------------------------------------------------------------------------------
// cnt[r] = stored entries of A's row r (0-based) = the length of C's column r
__global__ void tp_count_k(const i64 *__restrict__ rowval, i64 nnz, u32 *__restrict__ cnt) {
    const i64 p = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < nnz) atomicAdd(&cnt[rowval[p] - 1], 1u);
}
// cp[c] = cnt[c] (cp[nC] = 0: an exclusive scan follows); columns longer than TP_LANE are listed for the workgroup sort;
// st[0] = listed columns, st[1] = the longest column
__global__ __launch_bounds__(MT) void tp_lens_k(const u32 *__restrict__ cnt, i64 nC, i64 *__restrict__ cp, u32 *__restrict__ list,
                                                unsigned long long *__restrict__ st) {
    __shared__ u64 sw[MT / 64];
    u64 mx = 0;
    for (i64 c = (i64)blockIdx.x * MT + threadIdx.x; c <= nC; c += (i64)gridDim.x * MT) {
        const u32 len = c < nC ? cnt[c] : 0u;
        cp[c] = (i64)len;
        if (len > (u32)TP_LANE) list[atomicAdd(&st[0], 1ull)] = (u32)c;
        mx = len > mx ? len : mx;
    }
    mx = block_reduce<u64>(mx, MaxU64(), sw);
    if (threadIdx.x == 0 && mx > 0) atomicMax(&st[1], (unsigned long long)mx);
}
// every entry to its column's cursor: C row = A column + 1, the value's bits as they are
__global__ __launch_bounds__(MT) void tp_scatter_k(Csc64 A, const i64 *__restrict__ cp, u32 *__restrict__ cur, i64 *__restrict__ rowC,
                                                   u64 *__restrict__ valC) {
    __shared__ i64 scr[2];
    const i64 p0 = (i64)blockIdx.x * TP_TILE, p1 = min(p0 + TP_TILE, A.nnz);
    if (threadIdx.x == 0) scr[0] = col_of(A.colptr, p0, 0, A.n - 1);
    if (threadIdx.x == 1) scr[1] = col_of(A.colptr, p1 - 1, 0, A.n - 1);
    __syncthreads();
    const u64 *__restrict__ v = (const u64 *)A.nzval;
    for (i64 p = p0 + threadIdx.x; p < p1; p += MT) {
        const i64 j = col_of(A.colptr, p, scr[0], scr[1]);
        const i64 r = A.rowval[p] - 1;
        const i64 dst = cp[r] + (i64)atomicAdd(&cur[r], 1u);  // (exactly cnt[r] entries reach column r)
        rowC[dst] = j + 1;
        valC[dst] = v[p];
    }
}
// one lane sorts one column of 2..N entries in registers: a bitonic network, every index a constant (N = 2^LOG)
template <int LOG>
__global__ __launch_bounds__(MT) void tp_sort_lane_k(const i64 *__restrict__ cp, i64 nC, i64 *__restrict__ rowC, u64 *__restrict__ valC) {
    constexpr int N = 1 << LOG;
    const i64 c = (i64)blockIdx.x * MT + threadIdx.x;
    if (c >= nC) return;
    const i64 s = cp[c], len = cp[c + 1] - s;
    if (len < 2 || len > N) return;
    i64 k[N];
    u64 v[N];
#pragma unroll
    for (int t = 0; t < N; t++) {
        k[t] = t < len ? rowC[s + t] : (i64)0x7FFFFFFFFFFFFFFFll;
        v[t] = t < len ? valC[s + t] : 0ull;
    }
#pragma unroll
    for (int a = 1; a <= LOG; a++) {
#pragma unroll
        for (int b = a - 1; b >= 0; b--) {
#pragma unroll
            for (int i = 0; i < N; i++) {
                const int l = i ^ (1 << b);
                if (l > i) {
                    const bool up = (i & (1 << a)) == 0;
                    const bool sw = up ? k[i] > k[l] : k[i] < k[l];
                    const i64 ki = k[i], kl = k[l];
                    const u64 vi = v[i], vl = v[l];
                    k[i] = sw ? kl : ki;
                    k[l] = sw ? ki : kl;
                    v[i] = sw ? vl : vi;
                    v[l] = sw ? vi : vl;
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < N; t++)
        if (t < len) {
            rowC[s + t] = k[t];
            valC[s + t] = v[t];
        }
}
// one workgroup sorts one listed column (TP_LANE < length <= TP_BLOCK) in LDS: key = row << TP_IDX_BITS | local index
__global__ __launch_bounds__(MT) void tp_sort_block_k(const i64 *__restrict__ cp, const u32 *__restrict__ list, i64 *__restrict__ rowC,
                                                      u64 *__restrict__ valC) {
    __shared__ u64 skey[TP_BLOCK];
    __shared__ u64 sval[TP_BLOCK];
    const i64 c = (i64)list[blockIdx.x];
    const i64 s = cp[c];
    const int len = (int)(cp[c + 1] - s);  // (the host checked the longest column against TP_BLOCK)
    int S = 2;
    while (S < len) S <<= 1;
    for (int t = threadIdx.x; t < S; t += MT) {
        skey[t] = t < len ? ((u64)rowC[s + t] << TP_IDX_BITS) | (u64)t : ~0ull;
        if (t < len) sval[t] = valC[s + t];
    }
    __syncthreads();
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
    for (int t = threadIdx.x; t < len; t += MT) {
        const u64 k = skey[t];
        rowC[s + t] = (i64)(k >> TP_IDX_BITS);
        valC[s + t] = sval[k & ((1u << TP_IDX_BITS) - 1)];
    }
}
// the columns of a scanned cp: those longer than COLSORT_LANE are listed for the workgroup sort; st[0] = listed columns, st[1] = the
// longest column
__global__ __launch_bounds__(MT) void col_lens_k(const i64 *__restrict__ cp, i64 n, u32 *__restrict__ list, unsigned long long *__restrict__ st) {
    const i64 c = (i64)blockIdx.x * MT + threadIdx.x;
    const u32 len = c < n ? (u32)min(cp[c + 1] - cp[c], (i64)0xFFFFFFFFll) : 0u;
    if (len > (u32)COLSORT_LANE) list[atomicAdd(&st[0], 1ull)] = (u32)c;
    const u32 m = esp_wave_max(len);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&st[1], (unsigned long long)m);
}

}  // namespace
static_assert(TP_LANE == COLSORT_LANE && TP_BLOCK == COLSORT_BLOCK, "internal.hpp states the column sorts' limits");
void sort_columns_launch(hipStream_t s, const i64 *cp, i64 nC, i64 *rowC, u64 *valC, i64 maxlen, const u32 *list, i64 nlong) {
    const dim3 gc(grid_for(nC, MT));
    if (maxlen >= 2 && maxlen <= 8) hipLaunchKernelGGL(tp_sort_lane_k<3>, gc, dim3(MT), 0, s, cp, nC, rowC, valC);
    else if (maxlen > 8 && maxlen <= 16) hipLaunchKernelGGL(tp_sort_lane_k<4>, gc, dim3(MT), 0, s, cp, nC, rowC, valC);
    else if (maxlen > 16) hipLaunchKernelGGL(tp_sort_lane_k<5>, gc, dim3(MT), 0, s, cp, nC, rowC, valC);
    if (nlong > 0) hipLaunchKernelGGL(tp_sort_block_k, dim3((unsigned)nlong), dim3(MT), 0, s, cp, list, rowC, valC);
}
int32_t ColumnSort::plan(DevBuf &cp, i64 n, i64 nnz, unsigned long long *st, DevBuf &rv, DevBuf &payload) {
    esp_handle *h = h_;
    hipStream_t s = h->stream;
    cp_ = &cp, rv_ = &rv, pay_ = &payload, n_ = n, nnz_ = nnz;
    CK(ensure(h, list_, sizeof(u32) * (size_t)n));
    hipLaunchKernelGGL(col_lens_k, dim3(grid_for(n, MT)), dim3(MT), 0, s, (const i64 *)cp.p, n, (u32 *)list_.p, st);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, st, sizeof(u64) * 2, hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    nlong_ = (i64)h->pin_scalar[0], maxlen_ = (i64)h->pin_scalar[1];
    if (maxlen_ <= COLSORT_BLOCK) {
        CK(ensure(h, rv, sizeof(i64) * (size_t)nnz));
        CK(ensure(h, payload, sizeof(u64) * (size_t)nnz));
        rowB = (i64 *)rv.p;
        pay = (u64 *)payload.p;
        L = h->L;
        return ESP_OK;
    }
    CK(sf_.open(n, n, nnz));
    keys = sf_.keys();
    pay = sf_.vals();
    L = sf_.L();
    return ESP_OK;
}
int32_t ColumnSort::finish(bool *one_based) {
    esp_handle *h = h_;
    *one_based = keys != nullptr;
    if (!keys) {
        sort_columns_launch(h->stream, (const i64 *)cp_->p, n_, rowB, pay, maxlen_, (const u32 *)list_.p, nlong_);
        return ESP_OK;
    }
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(h->stream));
    CK(sf_.flush(nnz_));
    sf_.take(*cp_, *rv_, *pay_);
    return ESP_OK;
}
namespace {

// ---- transpose(A)*x: one lane per column, a wave for a column longer than MV_LONG ---------------------------------------------
__global__ __launch_bounds__(MT) void mv_t_k(Csc64 A, const double *__restrict__ x, double *__restrict__ r) {
    const i64 j = (i64)blockIdx.x * MT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    i64 s = 0, e = 0;
    if (j < A.n) {
        s = A.colptr[j] - 1;
        e = A.colptr[j + 1] - 1;
    }
    const bool longc = e - s > MV_LONG;
    if (j < A.n && !longc) {
        double tmp = 0.0;
        for (i64 k = s; k < e; k++) tmp = tmp + A.nzval[k] * x[A.rowval[k] - 1];
        r[j] = 0.0 + tmp;
    }
    // the wave's long columns one after the other: 64 products at a time in parallel, folded one by one in stored order
    u64 mask = __ballot(longc);
    while (mask) {
        const int src = __builtin_ctzll(mask);
        mask &= mask - 1;
        const i64 ls = __shfl(s, src), le = __shfl(e, src);
        double tmp = 0.0;
        for (i64 b = ls; b < le; b += 64) {
            const i64 k = b + lane;
            const double pr = k < le ? A.nzval[k] * x[A.rowval[k] - 1] : 0.0;
            const int cnt = (int)min((i64)64, le - b);
            for (int t = 0; t < cnt; t++) tmp = tmp + __shfl(pr, t);
        }
        if (lane == src) r[j] = 0.0 + tmp;
    }
}

// ---- issymmetric: every stored value that is not == 0 against its mirror ----------------------------------------------------
__global__ __launch_bounds__(MT) void sym_k(Csc64 A, unsigned long long *__restrict__ flag) {
    __shared__ i64 scr[2];
    __shared__ unsigned long long stop;
    const i64 p0 = (i64)blockIdx.x * TP_TILE, p1 = min(p0 + TP_TILE, A.nnz);
    // a workgroup that starts after a mismatch was found has nothing to do (a benign race: nobody waits for the flag)
    if (threadIdx.x == 0) stop = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 1) scr[0] = col_of(A.colptr, p0, 0, A.n - 1);
    if (threadIdx.x == 2) scr[1] = col_of(A.colptr, p1 - 1, 0, A.n - 1);
    __syncthreads();
    if (stop) return;
    bool bad = false;
    for (i64 p = p0 + threadIdx.x; p < p1; p += MT) {
        const double v = A.nzval[p];
        if (v == 0.0) continue;  // a stored zero of either sign is an absent entry
        const i64 i = A.rowval[p] - 1, j = col_of(A.colptr, p, scr[0], scr[1]);
        double w = v;  // (diagonal: v == v, false for NaN)
        if (i != j) {  // A[j,i]: row j + 1 in column i
            i64 lo = A.colptr[i] - 1, hi = A.colptr[i + 1] - 1;
            while (lo < hi) {
                const i64 mid = (lo + hi) >> 1;
                if (A.rowval[mid] < j + 1) lo = mid + 1;
                else hi = mid;
            }
            w = lo < A.colptr[i + 1] - 1 && A.rowval[lo] == j + 1 ? A.nzval[lo] : 0.0;
        }
        bad |= !(v == w);
    }
    if (bad) __hip_atomic_store(flag, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- opnorm's general branch: the max over segments of the segment's sum of |v| in stored order ----------------------------
// segment c = entries [st[c] - off, st[c + 1] - off): the columns of the CSC (st = colptr, off = 1) or the rows of the
// row-wise index (st = rowptr0 + 1, off = 0); out: the max's bit pattern
__global__ __launch_bounds__(MT) void segsum_max_k(const i64 *__restrict__ st, i64 off, const double *__restrict__ val, i64 nseg,
                                                   unsigned long long *__restrict__ out) {
    __shared__ u64 sw[MT / 64];
    u64 mx = 0;
    for (i64 c = (i64)blockIdx.x * MT + threadIdx.x; c < nseg; c += (i64)gridDim.x * MT) {
        double sum = 0.0;
        for (i64 k = st[c] - off; k < st[c + 1] - off; k++) sum = sum + fabs(val[k]);
        const u64 b = (u64)__double_as_longlong(sum);
        mx = b > mx ? b : mx;
    }
    mx = block_reduce<u64>(mx, MaxU64(), sw);
    if (threadIdx.x == 0 && mx > 0) atomicMax(out, (unsigned long long)mx);
}

// ---- norm over the stored values ------------------------------------------------------------------------------------------
// st[0] = max |v| bits, st[1] = min |v| bits over the values that are not NaN, st[2] = values that are not == 0, st[3] = NaNs
__global__ __launch_bounds__(MT) void nrm_stats_k(const double *__restrict__ x, i64 N, unsigned long long *__restrict__ st) {
    __shared__ u64 sw[MT / 64];
    u64 mx = 0, mn = ~0ull, nz = 0, nan = 0;
    const u64 *__restrict__ xb = (const u64 *)x;
    for (i64 i = (i64)blockIdx.x * MT + threadIdx.x; i < N; i += (i64)gridDim.x * MT) {
        const u64 a = xb[i] & ABS_MASK;
        mx = a > mx ? a : mx;
        if (a > INF_BITS) nan++;
        else mn = a < mn ? a : mn;
        nz += a != 0 ? 1 : 0;  // (!iszero: NaN counts)
    }
    mx = block_reduce<u64>(mx, MaxU64(), sw);
    __syncthreads();
    mn = block_reduce<u64>(mn, MinU64(), sw);
    __syncthreads();
    nz = block_reduce<u64>(nz, AddU64(), sw);
    __syncthreads();
    nan = block_reduce<u64>(nan, AddU64(), sw);
    if (threadIdx.x == 0) {
        atomicMax(&st[0], (unsigned long long)mx);
        atomicMin(&st[1], (unsigned long long)mn);
        if (nz) atomicAdd(&st[2], (unsigned long long)nz);
        if (nan) atomicAdd(&st[3], (unsigned long long)nan);
    }
}
// partial[b] = workgroup b's sum of f(|v|): MODE 1 |v|, 2 (|v|/s)^2, 3 (|v|/s)^p -- every thread in grid-stride order, then the tree
template <int MODE>
__global__ __launch_bounds__(MT) void nrm_sum_k(const double *__restrict__ x, i64 N, double s, double p, double *__restrict__ partial) {
    __shared__ double sw[MT / 64];
    double acc = 0.0;
    for (i64 i = (i64)blockIdx.x * MT + threadIdx.x; i < N; i += (i64)gridDim.x * MT) {
        const double a = fabs(x[i]);
        double t;
        if (MODE == 1) t = a;
        else if (MODE == 2) {
            const double q = a / s;
            t = q * q;
        } else t = pow(a / s, p);
        acc = acc + t;
    }
    acc = block_reduce<double>(acc, AddF64(), sw);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(MT) void nrm_final_k(const double *__restrict__ partial, int G, double *__restrict__ out) {
    __shared__ double sw[MT / 64];
    double acc = 0.0;
    for (int b = threadIdx.x; b < G; b += MT) acc = acc + partial[b];
    acc = block_reduce<double>(acc, AddF64(), sw);
    if (threadIdx.x == 0) out[0] = acc;
}

double from_bits(u64 b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}

// C := transpose(A) through an ESP_COO flush of a scratch handle; cp / rv / nz receive its CSC
int32_t transpose_generic(esp_handle *c, const Csc64 &A, i64 mC, i64 nC, DevBuf &cp, DevBuf &rv, DevBuf &nz) {
    ScratchFlush sf(c, "esp_transpose");
    CK(sf.open(mC, nC, A.nnz, true));  // (esp_debug_fail_next_bucket_stage armed on c: this is the flush it meets)
    hipLaunchKernelGGL(tp_expand_k, dim3(grid_for(A.nnz, TP_TILE)), dim3(MT), 0, sf.stream(), A, sf.L(), sf.keys(), sf.vals());
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipStreamSynchronize(sf.stream()));
    CK(sf.flush(A.nnz));
    sf.take(cp, rv, nz);
    return ESP_OK;
}

// C := transpose(A) by counting sort; *done = false (nothing installed, every buffer released) when a row of A is too long
// seen[0], seen[1]: the columns listed for the workgroup sort and the longest column, as tp_lens_k measured them
int32_t transpose_counting(esp_handle *c, const Csc64 &A, i64 nC, Temps &tmp, bool *done, i64 *seen) {
    esp_handle *h = c;
    hipStream_t s = h->stream;
    DevBuf &cnt = tmp.b[0], &list = tmp.b[1], &stat = tmp.b[2], &ws = tmp.b[3], &cp = tmp.b[6], &rv = tmp.b[7], &nz = tmp.b[8];
    int l = 0;
    *done = false;
    CK(ensure(h, cnt, sizeof(u32) * (size_t)std::max<i64>(nC, 1)));
    CK(ensure(h, list, sizeof(u32) * (size_t)std::max<i64>(nC, 1)));
    CK(ensure(h, stat, sizeof(u64) * 2));
    CK(ensure(h, cp, sizeof(i64) * (size_t)(nC + 1)));
    HIPCK(h, hipMemsetAsync(cnt.p, 0, sizeof(u32) * (size_t)nC, s));
    HIPCK(h, hipMemsetAsync(stat.p, 0, sizeof(u64) * 2, s));
    hipLaunchKernelGGL(tp_count_k, dim3(grid_for(A.nnz, MT)), dim3(MT), 0, s, A.rowval, A.nnz, (u32 *)cnt.p);
    hipLaunchKernelGGL(tp_lens_k, dim3(std::min<i64>(grid_for(nC + 1, MT), MAX_GRID)), dim3(MT), 0, s, (const u32 *)cnt.p, nC, (i64 *)cp.p, (u32 *)list.p,
                       (unsigned long long *)stat.p);
    CK(scan_inplace<i64, false>(h, (i64 *)cp.p, nC + 1, ws, &l));
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, stat.p, sizeof(u64) * 2, hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    const i64 nlong = (i64)h->pin_scalar[0], maxlen = (i64)h->pin_scalar[1];
    seen[0] = nlong;
    seen[1] = maxlen;
    if (maxlen > TP_BLOCK || nlong > 0x7FFFFFFFll) {
        for (DevBuf *b : {&cnt, &list, &stat, &ws, &cp}) release(*b);
        return ESP_OK;
    }
    CK(ensure(h, rv, sizeof(i64) * (size_t)A.nnz));
    CK(ensure(h, nz, sizeof(u64) * (size_t)A.nnz));
    HIPCK(h, hipMemsetAsync(cnt.p, 0, sizeof(u32) * (size_t)nC, s));
    hipLaunchKernelGGL(tp_scatter_k, dim3(grid_for(A.nnz, TP_TILE)), dim3(MT), 0, s, A, (const i64 *)cp.p, (u32 *)cnt.p, (i64 *)rv.p, (u64 *)nz.p);
    sort_columns_launch(s, (const i64 *)cp.p, nC, (i64 *)rv.p, (u64 *)nz.p, maxlen, (const u32 *)list.p, nlong);
    add_one_launch(s, (i64 *)cp.p, nC + 1);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(s));
    *done = true;
    return ESP_OK;
}

// norm(x, p) of N device doubles (norm(view(nonzeros(A), 1:nnz(A)), p)); p is not NaN
int32_t norm_values(esp_handle *h, const double *x, i64 N, double p, double *result) {
    if (N == 0) {  // (norm of an empty collection)
        *result = 0.0;
        return ESP_OK;
    }
    hipStream_t s = h->stream;
    Temps tmp;
    DevBuf &st = tmp.b[0], &part = tmp.b[1];
    const int G = (int)std::min<i64>(RED_GRID, ceil_div<i64>(N, MT));
    const bool inf = std::isinf(p);
    const bool stats = inf || p == 0.0 || p == 2.0 || (p > 1.0 || p < -1.0);
    u64 mx = 0, mn = 0, nzc = 0, nan = 0;
    if (stats) {
        CK(ensure(h, st, sizeof(u64) * 4));
        hipLaunchKernelGGL(set_i64_k, dim3(1), dim3(1), 0, s, (i64 *)st.p, (i64)0, (i64)-1, (i64)0, (i64)0);
        hipLaunchKernelGGL(nrm_stats_k, dim3(G), dim3(MT), 0, s, x, N, (unsigned long long *)st.p);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, st.p, sizeof(u64) * 4, hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        mx = h->pin_scalar[0], mn = h->pin_scalar[1], nzc = h->pin_scalar[2], nan = h->pin_scalar[3];
    }
    const double maxabs = from_bits(mx), minabs = nan ? NAN : from_bits(mn);
    if (inf && p > 0) {  // normInf: the max, NaN propagating
        *result = maxabs;
        return ESP_OK;
    }
    if (inf) {  // normMinusInf
        *result = minabs;
        return ESP_OK;
    }
    if (p == 0.0) {  // count(!iszero, x)
        *result = (double)nzc;
        return ESP_OK;
    }
    int mode = 3;
    double scale = 1.0;
    if (p == 1.0) {
        mode = 1;
    } else if (p == 2.0) {  // nrm2 without over- / underflow: scaled by the largest |v|
        if (std::isnan(maxabs) || maxabs == 0.0 || std::isinf(maxabs)) {
            *result = maxabs;
            return ESP_OK;
        }
        mode = 2;
        scale = maxabs;
    } else if (p > 1.0 || p < -1.0) {  // generic_normp: rescale where length(x) * maxabs^p leaves the finite nonzero range
        const double ma = p > 1.0 ? maxabs : minabs;
        if (ma == 0.0 || std::isinf(ma)) {
            *result = ma;
            return ESP_OK;
        }
        const double t = (double)N * std::pow(ma, p);
        if (!(std::isfinite(t) && t != 0.0)) scale = ma;
    }
    CK(ensure(h, part, sizeof(double) * (size_t)(G + 1)));
    double *pp = (double *)part.p;
    if (mode == 1) hipLaunchKernelGGL(nrm_sum_k<1>, dim3(G), dim3(MT), 0, s, x, N, scale, p, pp);
    else if (mode == 2) hipLaunchKernelGGL(nrm_sum_k<2>, dim3(G), dim3(MT), 0, s, x, N, scale, p, pp);
    else hipLaunchKernelGGL(nrm_sum_k<3>, dim3(G), dim3(MT), 0, s, x, N, scale, p, pp);
    hipLaunchKernelGGL(nrm_final_k, dim3(1), dim3(MT), 0, s, (const double *)pp, G, pp + G);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, pp + G, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    const double sum = from_bits((u64)h->pin_scalar[0]);
    if (mode == 1) *result = sum;
    else if (mode == 2) *result = scale * std::sqrt(sum);
    else *result = scale == 1.0 ? std::pow(sum, 1.0 / p) : scale * std::pow(sum, 1.0 / p);
    return ESP_OK;
}

// max over segments of their |v| sums (opnorm's general loops); nseg > 0
int32_t segsum_max(esp_handle *h, const i64 *st, i64 off, const double *val, i64 nseg, double *result) {
    hipStream_t s = h->stream;
    Temps tmp;
    DevBuf &out = tmp.b[0];
    CK(ensure(h, out, sizeof(u64)));
    HIPCK(h, hipMemsetAsync(out.p, 0, sizeof(u64), s));  // (nA = 0)
    hipLaunchKernelGGL(segsum_max_k, dim3(std::min<i64>(grid_for(nseg, MT), MAX_GRID)), dim3(MT), 0, s, st, off, val, nseg, (unsigned long long *)out.p);
    HIPCK(h, hipGetLastError());
    i64 b = 0;
    CK(read_i64(h, (const i64 *)out.p, &b));
    *result = from_bits((u64)b);
    return ESP_OK;
}

}  // namespace

extern "C" int32_t esp_debug_transpose_path(esp_handle *c, int32_t path) {
    if (!c || path < 0 || path > 2) return ESP_ERR_INVALID;
    c->transpose_path = path;
    return ESP_OK;
}

extern "C" int32_t esp_debug_last_transpose(const esp_handle *c, int64_t out[3]) {
    if (!c || !out) return ESP_ERR_INVALID;
    for (int k = 0; k < 3; k++) out[k] = c->last_transpose[k];
    return ESP_OK;
}

extern "C" int32_t esp_transpose(esp_handle *a, esp_handle *c, int64_t *nnz_out) {
    if (!a || !c) return ESP_ERR_INVALID;
    if (c == a) FAIL(c, ESP_ERR_INVALID, "esp_transpose: the result handle must not be the operand");
    if (a->device != c->device) FAIL(c, ESP_ERR_INVALID, "esp_transpose: operand and result on different devices");
    CK(check_operand(a, "esp_transpose"));
    CK(check_operand(c, "esp_transpose"));
    if (c->m != a->n || c->n != a->m)
        FAIL(c, ESP_ERR_INVALID, "esp_transpose: the result handle is not %lld x %lld", (long long)a->n, (long long)a->m);
    const Csc64 A = csc_of(a);
    const i64 mC = a->n, nC = a->m;
    Temps tmp;
    DevBuf &cp = tmp.b[6], &rv = tmp.b[7], &nz = tmp.b[8];
    i64 took[3] = {0, 0, 0};  // (esp_debug_last_transpose)
    if (A.nnz == 0) {
        CK(ensure(c, cp, sizeof(i64) * (size_t)(nC + 1)));
        CK(ensure(c, rv, sizeof(i64)));
        CK(ensure(c, nz, sizeof(double)));
        hipLaunchKernelGGL(fill_i64_k, dim3(grid_for(nC + 1, MT)), dim3(MT), 0, c->stream, (i64 *)cp.p, nC + 1, (i64)1);
        HIPCK(c, hipGetLastError());
        HIPCK(c, hipStreamSynchronize(c->stream));
    } else {
        bool done = false;
        if (c->transpose_path != 1) CK(transpose_counting(c, A, nC, tmp, &done, took + 1));
        if (!done) CK(transpose_generic(c, A, mC, nC, cp, rv, nz));
        took[0] = done ? 2 : 1;
    }
    install(c, cp, rv, nz, A.nnz);
    for (int k = 0; k < 3; k++) c->last_transpose[k] = took[k];
    if (nnz_out) *nnz_out = A.nnz;
    return ESP_OK;
}

extern "C" int32_t esp_mul_transpose(esp_handle *h, const double *x, double *r, int32_t on_device) {
    if (!h || !x || !r) return ESP_ERR_INVALID;
    CK(check_operand(h, "esp_mul_transpose"));
    const double *dx = x;
    double *dr = r;
    if (!on_device) {
        CK(ensure(h, h->mul_x, sizeof(double) * (size_t)std::max<i64>(h->m, 1)));
        CK(ensure(h, h->mul_r, sizeof(double) * (size_t)std::max<i64>(h->n, 1)));
        HIPCK(h, hipMemcpyAsync(h->mul_x.p, x, sizeof(double) * (size_t)h->m, hipMemcpyHostToDevice, h->stream));
        dx = (const double *)h->mul_x.p;
        dr = (double *)h->mul_r.p;
    }
    if (h->n > 0) hipLaunchKernelGGL(mv_t_k, dim3(grid_for(h->n, MT)), dim3(MT), 0, h->stream, csc_of(h), dx, dr);
    HIPCK(h, hipGetLastError());
    if (!on_device) HIPCK(h, hipMemcpyAsync(r, dr, sizeof(double) * (size_t)h->n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}

extern "C" int32_t esp_issymmetric(esp_handle *h, int32_t *result) {
    if (!h || !result) return ESP_ERR_INVALID;
    CK(check_operand(h, "esp_issymmetric"));
    if (h->m != h->n) {
        *result = 0;
        return ESP_OK;
    }
    if (h->nnz == 0) {
        *result = 1;
        return ESP_OK;
    }
    Temps tmp;
    DevBuf &flag = tmp.b[0];
    CK(ensure(h, flag, sizeof(u64)));
    HIPCK(h, hipMemsetAsync(flag.p, 0, sizeof(u64), h->stream));
    hipLaunchKernelGGL(sym_k, dim3(grid_for(h->nnz, TP_TILE)), dim3(MT), 0, h->stream, csc_of(h), (unsigned long long *)flag.p);
    HIPCK(h, hipGetLastError());
    i64 f = 0;
    CK(read_i64(h, (const i64 *)flag.p, &f));
    *result = f ? 0 : 1;
    return ESP_OK;
}

extern "C" int32_t esp_opnorm(esp_handle *h, double p, double *result) {
    if (!h || !result) return ESP_ERR_INVALID;
    if (std::isnan(p)) FAIL(h, ESP_ERR_INVALID, "esp_opnorm: p is NaN");
    CK(check_operand(h, "esp_opnorm"));
    const i64 m = h->m, n = h->n, N = h->nnz;
    const double *nz = (const double *)h->nzval.p;
    if (m == 0 || n == 0) {
        *result = 0.0;
        return ESP_OK;
    }
    const bool p1 = p == 1.0, p2 = p == 2.0, pinf = p == INFINITY;
    if (m == 1) {
        if (p1) return norm_values(h, nz, N, INFINITY, result);
        if (p2) return norm_values(h, nz, N, 2.0, result);
        if (pinf) return norm_values(h, nz, N, 1.0, result);
    } else if (n == 1 && (p1 || p2 || pinf)) {
        return norm_values(h, nz, N, p, result);
    } else {
        if (p2)
            FAIL(h, ESP_ERR_UNSUPPORTED, "esp_opnorm: 2-norm not yet implemented for sparse matrices. Try opnorm(Array(A)) or opnorm(A, p) where p=1 or Inf.");
        if ((p1 || pinf) && N == 0) {
            *result = 0.0;
            return ESP_OK;
        }
        if (p1) return segsum_max(h, (const i64 *)h->colptr.p, 1, nz, n, result);
        if (pinf) {  // the rows of esp_mul's row-wise index, each in increasing column order
            CK(csr_current(h));
            return segsum_max(h, (const i64 *)h->csr_rowptr.p + 1, 0, (const double *)h->csr_val.p, m, result);
        }
    }
    FAIL(h, ESP_ERR_INVALID, "esp_opnorm: invalid operator norm p=%g. Valid: 1, 2, Inf", p);
}

extern "C" int32_t esp_norm(esp_handle *h, double p, double *result) {
    if (!h || !result) return ESP_ERR_INVALID;
    if (std::isnan(p)) FAIL(h, ESP_ERR_INVALID, "esp_norm: p is NaN");
    CK(check_operand(h, "esp_norm"));
    return norm_values(h, (const double *)h->nzval.p, h->nnz, p, result);
}
