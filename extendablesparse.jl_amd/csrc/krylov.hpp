// krylov.hpp -- libesparse_hip: what the Krylov solvers share (krylov.hip: esp_cg; bicgstabl.hip: esp_bicgstabl): the tree of the
// ordered summation shape (krylov.hip states the shape in full), its level kernels, and the row gathers that carry a dot product.
// Every translation unit that includes this gets its own copy of the kernels (an unnamed namespace).
#pragma once
#include "internal.hpp"

namespace {

constexpr int KT = 256;       // threads of every kernel = rows / elements of a chunk of the summation shape
constexpr int KCAP = 2048;    // part entries a workgroup stages in LDS, as precon.hip's row kernels
constexpr unsigned KGRID = 2048;  // workgroups of the grid-stride vector kernels (256 CUs x 8)

// the tree of the summation shape over the 256 values v of a workgroup; the sum in thread 0.  The steps w = 128 and 64 go
// through LDS, w = 32 .. 1 pair the lanes of wave 0 with each other: the same pairs in the same order.
__device__ __forceinline__ double tree256(double v, double *sred) {
    const int t = threadIdx.x;
    sred[t] = v;
    __syncthreads();
    if (t < 128) sred[t] = sred[t] + sred[t + 128];
    __syncthreads();
    double a = 0.0;
    if (t < 64) {
        a = sred[t] + sred[t + 64];
        for (int w = 32; w > 0; w >>= 1) a = a + __shfl_down(a, w, 64);
    }
    return a;
}
// level 2 from the partial1 array, the result in every thread (sred is free again on return)
__device__ __forceinline__ double level2(const double *__restrict__ p1, i64 nb1, double *sred) {
    double a = 0.0;
    for (i64 q = threadIdx.x; q < nb1; q += KT) a = a + p1[q];
    const double s = tree256(a, sred);
    __syncthreads();
    if (threadIdx.x == 0) sred[0] = s;
    __syncthreads();
    const double r = sred[0];
    __syncthreads();
    return r;
}

// level 1: partial1[g] from partial0[256 g .. 256 g + 255]
__global__ __launch_bounds__(KT) void fold_k(const double *__restrict__ p0, i64 nb0, double *__restrict__ p1) {
    __shared__ double sred[KT];
    const i64 q = (i64)blockIdx.x * KT + threadIdx.x;
    const double s = tree256(q < nb0 ? p0[q] : 0.0, sred);
    if (threadIdx.x == 0) p1[blockIdx.x] = s;
}
__global__ __launch_bounds__(KT) void finish_k(const double *__restrict__ p1, i64 nb1, double *__restrict__ out) {
    __shared__ double sred[KT];
    const double s = level2(p1, nb1, sred);
    if (threadIdx.x == 0) out[0] = s;
}

// the ordered row gathers that carry a dot product: a workgroup owns 256 consecutive rows = one chunk of the shape
enum RowDotMode {
    UPPER_DOT = 0,  // pass 2 of ILU0's ldiv!: dst[i] = src[i] - sum_{j>i, increasing} val*src[j];  partial of dst[i]*other[i]
    MUL_DOT = 1,    // mul!: dst[i] = 0 + sum val*src[j], increasing j;                              partial of dst[i]*other[i]
    MUL_JAC_DOT = 2 // Jacobi's ldiv! of mul! in one launch: dst[i] = inv[i]*(0 + sum val*src[j]);           partial of dst[i]*other[i]
};
// p0 == nullptr: no dot product is wanted (other is not read, the tree does not run)
template <int MODE, typename P>
__global__ __launch_bounds__(KT) void row_dot_k(const P *__restrict__ ptr, const u32 *__restrict__ col, const double *__restrict__ val,
                                                const double *__restrict__ src, const double *__restrict__ other,
                                                double *__restrict__ dst, i64 n, double *__restrict__ p0,
                                                const double *__restrict__ inv) {
    __shared__ u32 scol[KCAP];
    __shared__ double sval[KCAP];
    __shared__ double sred[KT];
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
    double prod = 0.0;
    if (i < n) {
        const u64 kb = (u64)ptr[i], ke = (u64)ptr[i + 1];
        double acc = MODE == UPPER_DOT ? src[i] : 0.0;
        for (u64 k = kb; k < ke; k++) {
            const u32 c = staged ? scol[k - s] : col[k];
            const double a = staged ? sval[k - s] : val[k];
            if (MODE == UPPER_DOT) acc = acc - a * src[c];
            else acc = acc + a * src[c];
        }
        if (MODE == MUL_JAC_DOT) acc = inv[i] * acc;
        dst[i] = acc;
        if (p0) prod = acc * other[i];
    }
    if (!p0) return;
    const double t = tree256(prod, sred);
    if (threadIdx.x == 0) p0[blockIdx.x] = t;
}

// the vector kernels: a workgroup takes the chunks blockIdx.x, blockIdx.x + gridDim.x, ...
// c = invdiag .* r (Jacobi's ldiv!) with level 0 of dot(c, r); inv == nullptr: level 0 of dot(a, b) alone (Identity: a = b = r;
// ILUAM: a = c, b = r)
__global__ __launch_bounds__(KT) void dot_k(const double *__restrict__ inv, const double *__restrict__ a, const double *__restrict__ b,
                                            double *__restrict__ c, i64 n, i64 nb0, double *__restrict__ p0) {
    __shared__ double sred[KT];
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
        double prod = 0.0;
        if (i < n) {
            if (inv) {
                const double ci = inv[i] * b[i];
                c[i] = ci;
                prod = ci * b[i];
            } else {
                prod = a[i] * b[i];
            }
        }
        const double t = tree256(prod, sred);
        if (threadIdx.x == 0) p0[q] = t;
        __syncthreads();
    }
}
// r = b (c == nullptr) or r = b - c, with level 0 of dot(r, r)
__global__ __launch_bounds__(KT) void start_k(const double *__restrict__ b, const double *__restrict__ c, double *__restrict__ r, i64 n,
                                              i64 nb0, double *__restrict__ p0) {
    __shared__ double sred[KT];
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
        double prod = 0.0;
        if (i < n) {
            const double ri = c ? b[i] - c[i] : b[i];
            r[i] = ri;
            prod = ri * ri;
        }
        const double t = tree256(prod, sred);
        if (threadIdx.x == 0) p0[q] = t;
        __syncthreads();
    }
}

}  // namespace
