// krylov_many.hpp -- libesparse_hip: what the solvers for several right-hand sides share (krylov_many.hip: esp_cg_many and the
// many-column ldiv! of Jacobi and ILU0; gmres_many.hip: esp_gmres_many): the live mask, level 2 of a chunk's dot products, the
// many-column vector kernels that start a residual and take a dot product, the many-column row kernels and their launches.
// A chunk is ESP_MANY_CHUNK = 8 columns of an n x 8 column-major block; the set of live columns goes to every kernel as a plain
// bit-mask ARGUMENT, a frozen column's loads and stores are skipped (a wave-uniform branch).  Column d of a chunk has its level-0
// partials at p0 + d*nb0 and its level-1 partials at p1 + d*nb1.
// Every translation unit that includes this gets its own copy of the kernels (an unnamed namespace).
#pragma once
#include "krylov.hpp"

namespace {

constexpr int MC = ESP_MANY_CHUNK;
static_assert(MC == 8, "the live mask, the trees and the read-back slots are laid out for 8 columns");

// (is_live and all_live, the mask's two readers, are internal.hpp's: iluam.hip and block.hip take the mask as well)

// level 2 of the live columns at once: column d has its partial1 at p1 + d*nb1; the results in sres[0 .. 7], visible to every
// thread on return (sred is free again).  Lane t adds p1[t], p1[t + 256], ... to 0.0 as level2 does, then the same tree
__device__ __forceinline__ void level2_many(const double *__restrict__ p1, i64 nb1, u32 live, double (*sred)[KT], double *sres) {
#pragma unroll
    for (int d = 0; d < MC; d++) {
        double a = 0.0;
        if (is_live(live, d))
            for (i64 q = threadIdx.x; q < nb1; q += KT) a = a + p1[(i64)d * nb1 + q];
        sred[d][threadIdx.x] = a;
    }
    trees<MC>(sred, sres, 1);
}

// ---- the vector kernels: a lane handles the elements the single kernels give it, for every live column ----------------------------
// r = b (c == nullptr) or r = b - c, with level 0 of dot(r, r)
__global__ __launch_bounds__(KT) void start_many_k(const double *__restrict__ b, i64 ldb, const double *__restrict__ c, double *__restrict__ r,
                                                   i64 ldw, i64 n, i64 nb0, double *__restrict__ p0, u32 live) {
    __shared__ double sred[MC][KT];
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
#pragma unroll
        for (int d = 0; d < MC; d++) {
            double prod = 0.0;
            if (is_live(live, d) && i < n) {
                const double ri = c ? b[(i64)d * ldb + i] - c[(i64)d * ldw + i] : b[(i64)d * ldb + i];
                r[(i64)d * ldw + i] = ri;
                prod = ri * ri;
            }
            sred[d][threadIdx.x] = prod;
        }
        trees<MC>(sred, p0 + q, nb0);
    }
}
// c = invdiag .* b (Jacobi's ldiv!) with level 0 of dot(c, b); inv == nullptr: level 0 of dot(a, b) alone.  p0 == nullptr: the
// ldiv! alone (esp_precon_ldiv_many; c may be b there, so neither is __restrict__)
__global__ __launch_bounds__(KT) void dot_many_k(const double *__restrict__ inv, const double *a, i64 lda, const double *b, i64 ldb, double *c,
                                                 i64 ldc, i64 n, i64 nb0, double *__restrict__ p0, u32 live) {
    __shared__ double sred[MC][KT];
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
#pragma unroll
        for (int d = 0; d < MC; d++) {
            double prod = 0.0;
            if (is_live(live, d) && i < n) {
                if (inv) {
                    const double bi = b[(i64)d * ldb + i];
                    const double ci = inv[i] * bi;
                    c[(i64)d * ldc + i] = ci;
                    prod = ci * bi;
                } else {
                    prod = a[(i64)d * lda + i] * b[(i64)d * ldb + i];
                }
            }
            sred[d][threadIdx.x] = prod;
        }
        if (p0) trees<MC>(sred, p0 + q, nb0);
    }
}

// ---- the row kernels: a workgroup owns 256 consecutive rows and stages their slice of the index and values in LDS ONCE for the
// whole chunk (a slice above KCAP is read from global memory); a lane owns a row and 8 accumulators and runs the single kernel's
// statement for every live column, k ascending, as spmm_rows_k does.  MODE: krylov.hpp's UPPER_DOT, MUL_DOT and MUL_JAC_DOT (the
// row sum times xdiag[i] before the store: Jacobi's ldiv! of mul!, bitwise row_dot_k<MUL_JAC_DOT>), and
constexpr int LOWER_MANY = 3;  // row_chain_k<ILU_LOWER>: dst[i] = u0[i] - sum_{j<i, decreasing} val*u0[j], u0[j] = xdiag[j]*src[j]
// p0 == nullptr: no dot product is wanted (other is not read, the trees do not run).  LDS: 8 KiB of columns + 16 KiB of values
// + 16 KiB of trees = 40 KiB, four workgroups on a CU's 160 KiB (LOWER_MANY has no trees: 24 KiB)
template <int MODE, typename P>
__device__ __forceinline__ void row_many(const P *__restrict__ ptr, const u32 *__restrict__ col, const double *__restrict__ val,
                                         const double *__restrict__ xdiag, const double *__restrict__ src, i64 lds,
                                         const double *__restrict__ other, i64 ldo, double *__restrict__ dst, i64 ldd, i64 n,
                                         double *__restrict__ p0, u32 live) {
    __shared__ u32 scol[KCAP];
    __shared__ double sval[KCAP];
    __shared__ double sred[MODE == LOWER_MANY ? 1 : MC][KT];
    const i64 r0 = (i64)blockIdx.x * KT;
    const i64 i = r0 + threadIdx.x;
    const i64 rend = std::min<i64>(r0 + KT, n);
    const u64 s = (u64)ptr[r0], e = (u64)ptr[rend];
    const bool staged = e - s <= (u64)KCAP;
    if (staged) {
        const int cnt = (int)(e - s);
        for (int t = threadIdx.x; t < cnt; t += KT) {
            scol[t] = col[s + t];
            sval[t] = val[s + t];
        }
    }
    __syncthreads();
    double acc[MC];
#pragma unroll
    for (int d = 0; d < MC; d++) acc[d] = 0.0;
    if (i < n) {
        const u64 kb = (u64)ptr[i], ke = (u64)ptr[i + 1];
        if (MODE == UPPER_DOT || MODE == LOWER_MANY) {
            const double xi = MODE == LOWER_MANY ? xdiag[i] : 1.0;
#pragma unroll
            for (int d = 0; d < MC; d++)
                if (is_live(live, d)) acc[d] = MODE == LOWER_MANY ? xi * src[(i64)d * lds + i] : src[(i64)d * lds + i];
        }
        for (u64 k = kb; k < ke; k++) {
            const u32 c = staged ? scol[k - s] : col[k];
            const double a = staged ? sval[k - s] : val[k];
            const double *sc = src + c;
            const double xc = MODE == LOWER_MANY ? xdiag[c] : 1.0;
#pragma unroll
            for (int d = 0; d < MC; d++) {
                if (!is_live(live, d)) continue;
                if (MODE == LOWER_MANY) acc[d] = acc[d] - a * (xc * sc[(i64)d * lds]);
                else if (MODE == UPPER_DOT) acc[d] = acc[d] - a * sc[(i64)d * lds];
                else acc[d] = acc[d] + a * sc[(i64)d * lds];
            }
        }
        if (MODE == MUL_JAC_DOT) {
            const double inv = xdiag[i];
#pragma unroll
            for (int d = 0; d < MC; d++)
                if (is_live(live, d)) acc[d] = inv * acc[d];
        }
#pragma unroll
        for (int d = 0; d < MC; d++)
            if (is_live(live, d)) dst[(i64)d * ldd + i] = acc[d];
    }
    if (MODE == LOWER_MANY || !p0) return;
#pragma unroll
    for (int d = 0; d < MC; d++) {
        double prod = 0.0;
        if (is_live(live, d) && i < n) prod = acc[d] * other[(i64)d * ldo + i];
        sred[d][threadIdx.x] = prod;
    }
    trees<MC>(sred, p0 + blockIdx.x, (i64)gridDim.x);
}
template <int MODE, typename P>
__global__ __launch_bounds__(KT) void row_dot_many_k(const P *__restrict__ ptr, const u32 *__restrict__ col, const double *__restrict__ val,
                                                     const double *__restrict__ src, i64 lds, const double *__restrict__ other, i64 ldo,
                                                     double *__restrict__ dst, i64 ldd, i64 n, double *__restrict__ p0, u32 live) {
    row_many<MODE, P>(ptr, col, val, nullptr, src, lds, other, ldo, dst, ldd, n, p0, live);
}
__global__ __launch_bounds__(KT) void row_chain_many_k(const u32 *__restrict__ ptr, const u32 *__restrict__ col, const double *__restrict__ val,
                                                       const double *__restrict__ xdiag, const double *__restrict__ src, i64 lds,
                                                       double *__restrict__ dst, i64 ldd, i64 n, u32 live) {
    row_many<LOWER_MANY, u32>(ptr, col, val, xdiag, src, lds, nullptr, 0, dst, ldd, n, nullptr, live);
}
__global__ __launch_bounds__(KT) void row_jac_dot_many_k(const u64 *__restrict__ ptr, const u32 *__restrict__ col, const double *__restrict__ val,
                                                         const double *__restrict__ inv, const double *__restrict__ src, i64 lds,
                                                         const double *__restrict__ other, i64 ldo, double *__restrict__ dst, i64 ldd, i64 n,
                                                         double *__restrict__ p0, u32 live) {
    row_many<MUL_JAC_DOT, u64>(ptr, col, val, inv, src, lds, other, ldo, dst, ldd, n, p0, live);
}

// ---- the launches (they only enqueue on h->stream) ----------------------------------------------------------------------------------
inline unsigned rows_grid(i64 n) { return (unsigned)std::max<i64>(ceil_div<i64>(n, KT), 1); }
inline unsigned vec_grid(i64 n) { return (unsigned)std::min<i64>(std::max<i64>(ceil_div<i64>(n, KT), 1), KGRID); }

// dst = A*src over the row-wise index of esp_mul; p0: level 0 of dot(dst, other), or nullptr
void mul_many(esp_handle *h, const double *src, i64 lds, const double *other, i64 ldo, double *dst, i64 ldd, double *p0, u32 live) {
    hipLaunchKernelGGL((row_dot_many_k<MUL_DOT, u64>), dim3(rows_grid(h->n)), dim3(KT), 0, h->stream, (const u64 *)h->csr_rowptr.p + 1,
                       (const u32 *)h->csr_col.p, (const double *)h->csr_val.p, src, lds, other, ldo, dst, ldd, h->n, p0, live);
}
// dst = invdiag .* (A*src) (Jacobi, SPAI-0: ldiv! of mul! in one launch); p0: level 0 of dot(dst, other), or nullptr.  A is h's
// matrix -- the handle the SOLVE runs on, whose row-wise index csr_current made -- and p gives its diagonal alone: behind a
// BlockPreconditioner on its identity path p is the inner preconditioner and p->h the derived block matrix, which is not A
void mul_jacobi_many(esp_handle *h, esp_precon *p, const double *src, i64 lds, const double *other, i64 ldo, double *dst, i64 ldd, double *p0,
                     u32 live) {
    hipLaunchKernelGGL(row_jac_dot_many_k, dim3(rows_grid(h->n)), dim3(KT), 0, h->stream, (const u64 *)h->csr_rowptr.p + 1,
                       (const u32 *)h->csr_col.p, (const double *)h->csr_val.p, (const double *)p->diag.p, src, lds, other, ldo, dst, ldd, h->n,
                       p0, live);
}
// dst = invdiag .* src (Jacobi, SPAI-0); p0: level 0 of dot(dst, src), or nullptr.  dst may be src
void jacobi_many(esp_precon *p, const double *src, i64 lds, double *dst, i64 ldd, double *p0, u32 live) {
    const i64 n = p->n;
    hipLaunchKernelGGL(dot_many_k, dim3(vec_grid(n)), dim3(KT), 0, p->h->stream, (const double *)p->diag.p, (const double *)nullptr, (i64)0, src,
                       lds, dst, ldd, n, ceil_div<i64>(n, KT), p0, live);
}
// dst = ILU0 \ src: pass 1 into u1 (n x 8, leading dimension ld1; src may be dst), pass 2 with level 0 of dot(dst, other) in p0, or
// nullptr
void ilu0_many(esp_precon *p, const double *src, i64 lds, double *u1, i64 ld1, const double *other, i64 ldo, double *dst, i64 ldd, double *p0,
               u32 live) {
    const i64 n = p->n;
    hipStream_t st = p->h->stream;
    hipLaunchKernelGGL(row_chain_many_k, dim3(rows_grid(n)), dim3(KT), 0, st, (const u32 *)p->lptr.p, (const u32 *)p->lcol.p,
                       (const double *)p->lval.p, (const double *)p->diag.p, src, lds, u1, ld1, n, live);
    hipLaunchKernelGGL((row_dot_many_k<UPPER_DOT, u32>), dim3(rows_grid(n)), dim3(KT), 0, st, (const u32 *)p->uptr.p, (const u32 *)p->ucol.p,
                       (const double *)p->uval.p, (const double *)u1, ld1, other, ldo, dst, ldd, n, p0, live);
}

inline i64 even_ld(i64 n) { return std::max<i64>((n + 1) & ~(i64)1, 2); }

}  // namespace
