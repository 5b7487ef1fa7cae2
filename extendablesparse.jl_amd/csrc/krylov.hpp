// krylov.hpp -- libesparse_hip: what the Krylov solvers share (krylov.hip: esp_cg; bicgstabl.hip: esp_bicgstabl; gmres.hip:
// esp_gmres): the trees of the ordered summation shape (krylov.hip states the shape in full), its level kernels, the row gathers
// that carry a dot product, and on the host side the ONE place the three take A*v, Pl \ v and Pl \ (A*v) from (PreconProduct: a
// new preconditioner kind is one branch there) and the hand-over of host b / x (stage_vectors, return_x).
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
// ND trees of the summation shape at once: sred[d][t] holds the 256 values of dot d.  The steps w = 128 and 64 go through LDS,
// w = 32 .. 1 pair the lanes of one wave (dot d in wave d mod 4): the same pairs in the same order as tree256.  Lane 0 of that
// wave stores the sum of dot d < nout to out[d*stride].  Ends with a barrier: sred is free again.
template <int ND>
__device__ __forceinline__ void trees(double (*sred)[KT], double *__restrict__ out, i64 stride, int nout = ND) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int d = 0; d < ND; d++) sred[d][t] = sred[d][t] + sred[d][t + 128];
    }
    __syncthreads();
    for (int d = wv; d < ND; d += KT / 64) {
        double a = sred[d][lane] + sred[d][lane + 64];
        for (int w = 32; w > 0; w >>= 1) a = a + __shfl_down(a, w, 64);
        if (lane == 0 && d < nout) out[(i64)d * stride] = a;
    }
    __syncthreads();
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
// level 1 of `gridDim.y` dot products at once: dot d has its partial0 at p0 + d*nb0 and its partial1 at p1 + d*nb1.  gmres.hip's
// gm_fold_batch_k is this body behind the DGKS predicate; the two kernels keep their names, which the recorded traces carry.
__device__ __forceinline__ void fold_batch(const double *__restrict__ p0, i64 nb0, double *__restrict__ p1, i64 nb1, double *sred) {
    p0 += (i64)blockIdx.y * nb0;
    const i64 q = (i64)blockIdx.x * KT + threadIdx.x;
    const double s = tree256(q < nb0 ? p0[q] : 0.0, sred);
    if (threadIdx.x == 0) p1[(i64)blockIdx.y * nb1 + blockIdx.x] = s;
}
__global__ __launch_bounds__(KT) void fold_batch_k(const double *__restrict__ p0, i64 nb0, double *__restrict__ p1, i64 nb1) {
    __shared__ double sred[KT];
    fold_batch(p0, nb0, p1, nb1, sred);
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

// What a solve takes its products from, built once per solve: A through the row-wise index of h; the left preconditioner as the
// fused branches want it (p: fused_precon's, nullptr = Identity; blk: the BlockPreconditioner on its permuted path -- gather, inner
// ldiv!, scatter --, else nullptr); the grids (g0: a workgroup per chunk, gv: the grid-stride vector kernels'); the level-0
// partials p0; the scratch t of pmul (a solver without pmul passes nullptr).  `other` is the second factor of the optional dot
// product: with dot, level 0 of dot(dst, other) goes to p0; without, p0 is left alone -- but for Jacobi's ldiv, see there.  Every
// function only enqueues on h->stream.
struct PreconProduct {
    esp_handle *h;
    esp_precon *p, *blk;
    i64 n, nb0;
    unsigned g0, gv;
    double *p0, *t;

    void dot_launch(const double *inv, const double *a, const double *b, double *c) const {
        hipLaunchKernelGGL(dot_k, dim3(gv), dim3(KT), 0, h->stream, inv, a, b, c, n, nb0, p0);
    }
    template <int MODE>  // the row gather over A: MUL_DOT, or MUL_JAC_DOT with inv = invdiag
    void gather(const double *src, double *dst, const double *other, bool dot, const double *inv) const {
        hipLaunchKernelGGL((row_dot_k<MODE, u64>), dim3(g0), dim3(KT), 0, h->stream, (const u64 *)h->csr_rowptr.p + 1,
                           (const u32 *)h->csr_col.p, (const double *)h->csr_val.p, src, other, dst, n, dot ? p0 : (double *)nullptr, inv);
    }
    // dst = A*src (mul! exactly as esp_mul)
    void mul(const double *src, double *dst, const double *other, bool dot) const { gather<MUL_DOT>(src, dst, other, dot, nullptr); }
    // dst = Pl \ src (src != dst).  Identity launches the dot product alone and leaves dst untouched: the caller reads src in dst's
    // place.  Jacobi is dot_k's fused form, which ALWAYS writes p0 and forms level 0 of dot(dst, src), not of dot(dst, other): right
    // only while every caller passes other == src (esp_cg) or dot == false with a p0 it is about to overwrite (the two others).
    int32_t ldiv(const double *src, double *dst, const double *other, bool dot) const {
        if (!p) {
            if (dot) dot_launch(nullptr, src, other, nullptr);
        } else if (!blk && diag_applied(p)) {
            dot_launch((const double *)p->diag.p, nullptr, src, dst);
        } else if (blk || p->kind == ESP_PRECON_ILUAM || p->kind == ESP_PRECON_AMG || p->kind == ESP_PRECON_SPAI ||
                   p->kind == ESP_PRECON_CHOLESKY) {
            if (blk) CK(block_ldiv_launch(blk, src, dst, false));
            else if (p->kind == ESP_PRECON_AMG) CK(amg_solve(p, src, dst, false));  // the V-cycle's launches
            else if (p->kind == ESP_PRECON_SPAI) CK(spai_apply(p, src, dst, false));  // one product with M
            else if (p->kind == ESP_PRECON_CHOLESKY) CK(chol_solve(p, src, dst, false));  // the depth launches
            else CK(iluam_solve(p, src, dst, false));                              // the level launches
            if (dot) dot_launch(nullptr, dst, other, nullptr);
        } else {  // ILU0: pass 1 into p->u1 (precon.hip, unchanged), pass 2 carries the dot product
            ilu0_lower_launch(p, src);
            hipLaunchKernelGGL((row_dot_k<UPPER_DOT, u32>), dim3(g0), dim3(KT), 0, h->stream, (const u32 *)p->uptr.p, (const u32 *)p->ucol.p,
                               (const double *)p->uval.p, (const double *)p->u1.p, other, dst, n, dot ? p0 : (double *)nullptr,
                               (const double *)nullptr);
        }
        return ESP_OK;
    }
    // dst = Pl \ (A*src): Identity and Jacobi in one launch (Jacobi: the gathered row sum times invdiag[i] before the store,
    // bitwise ldiv! of mul!), every other kind the matvec into t (no dot), then ldiv
    int32_t pmul(const double *src, double *dst, const double *other, bool dot) const {
        if (!p) mul(src, dst, other, dot);
        else if (!blk && diag_applied(p)) gather<MUL_JAC_DOT>(src, dst, other, dot, (const double *)p->diag.p);
        else {
            mul(src, t, other, false);
            CK(ldiv(t, dst, other, dot));
        }
        return ESP_OK;
    }
};

// b and x as the kernels read them: the caller's device vectors, or (enqueued) copies of its host vectors in the handle's hb / hx
inline int32_t stage_vectors(esp_handle *h, i64 n, bool on_device, const double *b, double *x, const double **db, double **dx) {
    *db = b;
    *dx = x;
    if (on_device) return ESP_OK;
    esp_handle::Krylov &w = h->kry;
    CK(ensure(h, w.hb, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    CK(ensure(h, w.hx, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    HIPCK(h, hipMemcpyAsync(w.hb.p, b, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipMemcpyAsync(w.hx.p, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    *db = (const double *)w.hb.p;
    *dx = (double *)w.hx.p;
    return ESP_OK;
}
// the end of a solve: x back to the host when it came from there; returns synchronised
inline int32_t return_x(esp_handle *h, i64 n, bool on_device, double *x, const double *dx) {
    if (!on_device) HIPCK(h, hipMemcpyAsync(x, dx, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}

}  // namespace
