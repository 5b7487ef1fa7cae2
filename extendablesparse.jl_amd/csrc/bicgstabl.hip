// bicgstabl.hip -- libesparse_hip: BiCGStab(l) for non-symmetric systems (esp_bicgstabl) on the device CSC
// (see internal.hpp for the map of the translation units; krylov.hpp for what this shares with esp_cg and esp_gmres)
//
// The algorithm is IterativeSolvers.jl's bicgstabl! with a left preconditioner.  That package is not part of the reference
// tree: the statement sequence below is RESTATED from its documented behaviour, not read from its source.
//
//   bicgstabl!(x, A, b, l; Pl, abstol = 0, reltol = sqrt(eps), max_mv_products = n, initially_zero, r_shadow)
//     mv = 0
//     rs[0] = b                      (initially_zero)   |   rs[0] = b - A*x; mv = 1
//     rs[0] = Pl \ rs[0]             (LEFT preconditioning: every residual and norm below is the preconditioned one)
//     us[0..l] = 0;  omega = sigma = 1;  rt = r_shadow, or a copy of rs[0] when none is given
//     residual = norm(rs[0]);  tol = max(reltol*residual, abstol)
//     while mv < max_mv_products and not residual <= tol:
//         sigma = -omega*sigma
//         for j = 0 .. l-1:
//             rho = dot(rt, rs[j]);  beta = rho/sigma
//             us[k] = rs[k] - beta*us[k]            k = 0..j   (the product rounded, then the difference)
//             us[j+1] = Pl \ (A*us[j])
//             sigma = dot(rt, us[j+1]);  alpha = rho/sigma
//             rs[k] = rs[k] - alpha*us[k+1]         k = 0..j
//             rs[j+1] = Pl \ (A*rs[j])
//             x = x + alpha*us[0]
//         mv += 2l
//         M[i][k] = dot(rs[i], rs[k]) for i <= k, mirrored below the diagonal
//         gamma[1..l] = M[1..l,1..l] \ M[1..l,0]
//             LU without pivoting: for k: inv = 1/G[k][k]; G[i][k] *= inv (i > k); G[i][j] -= G[i][k]*G[k][j] (j > k, i > k);
//             forward substitution with the unit lower factor, back substitution with a true division, inner index increasing
//         us[0] = us[0] - gamma[k]*us[k]    k = 1..l in increasing k, one rounded product and one difference each
//         x     = x     + gamma[k]*rs[k-1]  k = 1..l, the same order rule (rs[0] is still the old one)
//         rs[0] = rs[0] - gamma[k]*rs[k]    k = 1..l, the same order rule
//         omega = gamma[l];  residual = norm(rs[0])     (a fresh dot product, not M's)
//     converged = residual <= tol
//
// mul! is esp_mul's and ldiv! esp_precon_ldiv's, bit for bit; every dot and norm is the ordered summation shape krylov.hip
// states; every division is a true double division, nothing is contracted.  A breakdown (sigma = 0, a singular M) is no error:
// Inf and NaN propagate and the loop runs to max_mv_products, as esp_cg's does.  n = 1 is such a case by construction: the
// first BiCG step solves the system exactly, rs[0] and rs[1] become 0 and the minimal-residual system is 0/0: x and the norms
// are NaN from the first outer iteration on (the package does the same).
// DEVIATIONS from the package: r_shadow is an argument and defaults to the initial preconditioned residual (the package draws
// rand(n)), which makes a solve reproducible; dot, norm and the Gram matrix (BLAS in the package) are the ordered shape;
// Pl = NULL is Identity with no copies.  tests/bicgstabl_model.c restates all of this as plain loops and is normative for the
// order of every operation: x and the whole history are bit-identical to it.
//
// Kernels of one outer iteration (l BiCG steps, then the minimal-residual step):
//   bicg_dir_k      level 2 of rho and of the last sigma redone by every workgroup (j = 0: sigma = -omega*sigma from the
//                   scalar block), beta, us[0..j] = rs[0..j] - beta*us[0..j] in one launch
//   pmul            us[j+1] = Pl \ (A*us[j]) with level 0 of dot(rt, us[j+1]) (krylov.hpp, PreconProduct::pmul):
//                     Identity  row_dot_k<MUL_DOT>, other = rt
//                     Jacobi    row_dot_k<MUL_JAC_DOT>: the gathered row sum times invdiag[i] before the store -- one launch,
//                               bitwise ldiv! of mul!
//                     ILU0      row_dot_k<MUL_DOT> into the scratch (no dot), row_chain_k<ILU_LOWER>, row_dot_k<UPPER_DOT>
//                     ILUAM     the matvec into the scratch, the level launches of iluam_solve, dot_k (AMG: the V-cycle's launches)
//   fold_k          level 1 of sigma
//   bicg_upd_k      level 2 of rho and sigma redone, alpha, rs[0..j] -= alpha*us[1..j+1], x += alpha*us[0] in one launch
//   pmul            rs[j+1] = Pl \ (A*rs[j]) with level 0 of dot(rt, rs[j+1]) = the next rho (not for rs[l]: nothing reads it)
//   fold_k
//   gram_k          ONE pass over rs[0..l]: a lane loads its l+1 values once and forms the (l+1)(l+2)/2 products; the trees of
//                   a chunk run batched through LDS (the same pairs in the same order as tree256, the last six steps of dot d
//                   in wave d mod 4); one level-0 partial per dot and chunk
//   fold_batch_k    level 1 of all the dots in one launch
//   gamma_k         ONE workgroup: level 2 of every dot, the LU, gamma[1..l], omega and the last sigma to the scalar block
//   mr_k            the three updates of the minimal-residual step, level 0 of dot(rs[0], rs[0]) and of dot(rt, rs[0]) (the
//                   next iteration's first rho)
//   fold_batch_k    level 1 of both
//   finish_k        level 2 of dot(rs[0], rs[0]) -> one double, read back through pin_scalar: the ONE host round trip of an
//                   outer iteration; the square root and the stop test run on the host
// gamma in one workgroup rather than redone by every workgroup of mr_k: redoing it costs up to 15 level-2 sums (three barriers
// and a pass over partial1 each) plus the LU in each of up to 2048 workgroups, in front of the streaming part; one launch of one
// workgroup costs a launch gap.  (Chosen by that count; the two were not measured against each other.)
// A value crosses workgroups only at a kernel boundary: no flags, no grid barrier, no fence.
#include "krylov.hpp"

namespace {

constexpr int BL_MAX = 4;  // largest l
// the scalar block: omega, sigma, gamma[k] at SC_GAMMA0 + k (k = 1..4), the squared norm for the read-back
enum { SC_OMEGA = 0, SC_SIGMA = 1, SC_GAMMA0 = 1, SC_OUT = 6, SC_COUNT = 8 };

constexpr int ndots(int l) { return (l + 1) * (l + 2) / 2; }

__global__ void init_scalars_k(double *__restrict__ sc) {
    if (threadIdx.x < SC_COUNT) sc[threadIdx.x] = threadIdx.x <= SC_SIGMA ? 1.0 : 0.0;  // omega = sigma = 1
}

// rt = r_shadow (src; nullptr: a copy of rs[0]; src == rt: already there), level 0 of dot(rs[0], rs[0]) in p0[q] and of
// dot(rt, rs[0]) in p0[nb0 + q]
__global__ __launch_bounds__(KT) void shadow_k(const double *src, const double *__restrict__ r0, double *rt, i64 n, i64 nb0,
                                               double *__restrict__ p0) {
    __shared__ double sred[2][KT];
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
        double pa = 0.0, pb = 0.0;
        if (i < n) {
            const double r = r0[i], s = src ? src[i] : r;
            if (src != rt) rt[i] = s;
            pa = r * r;
            pb = s * r;
        }
        sred[0][threadIdx.x] = pa;
        sred[1][threadIdx.x] = pb;
        trees<2>(sred, p0 + q, nb0);
    }
}

// rho = dot(rt, rs[j]); beta = rho/sigma, sigma the last one (sig_p1) or, for j = 0, -omega*sigma of the scalar block;
// us[k] = rs[k] - beta*us[k] for k = 0..j, two elements per lane (vector k at base + k*ns, ns even)
__global__ __launch_bounds__(KT) void bicg_dir_k(const double *__restrict__ rho_p1, const double *__restrict__ sig_p1,
                                                 const double *__restrict__ sc, i64 nb1, int j, const double *__restrict__ rs,
                                                 double *__restrict__ us, i64 ns, i64 n) {
    __shared__ double sred[KT];
    const double rho = level2(rho_p1, nb1, sred);
    const double sigma = sig_p1 ? level2(sig_p1, nb1, sred) : -sc[SC_OMEGA] * sc[SC_SIGMA];
    const double beta = rho / sigma;
    const i64 n2 = n >> 1;
    for (i64 e = (i64)blockIdx.x * KT + threadIdx.x; e < n2; e += (i64)gridDim.x * KT) {
        for (int k = 0; k <= j; k++) {
            const double2 rv = ((const double2 *)(rs + k * ns))[e];
            double2 uv = ((double2 *)(us + k * ns))[e];
            uv.x = rv.x - beta * uv.x;
            uv.y = rv.y - beta * uv.y;
            ((double2 *)(us + k * ns))[e] = uv;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        for (int k = 0; k <= j; k++) us[k * ns + n - 1] = rs[k * ns + n - 1] - beta * us[k * ns + n - 1];
}

// alpha = rho/sigma; rs[k] = rs[k] - alpha*us[k+1] for k = 0..j; x = x + alpha*us[0]
__global__ __launch_bounds__(KT) void bicg_upd_k(const double *__restrict__ rho_p1, const double *__restrict__ sig_p1, i64 nb1, int j,
                                                 double *__restrict__ rs, const double *__restrict__ us, double *__restrict__ x, i64 ns,
                                                 i64 n) {
    __shared__ double sred[KT];
    const double rho = level2(rho_p1, nb1, sred);
    const double sigma = level2(sig_p1, nb1, sred);
    const double alpha = rho / sigma;
    const i64 n2 = n >> 1;
    // rs and us are the handle's (16-byte aligned: ns is even, the base comes from ensure); x is the CALLER's when the vectors are
    // resident, and a view into a larger array is only 8-byte aligned: plain double accesses then (the same bits, every element
    // is computed by itself; the branch is uniform over the grid)
    const bool xvec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    for (i64 e = (i64)blockIdx.x * KT + threadIdx.x; e < n2; e += (i64)gridDim.x * KT) {
        for (int k = 0; k <= j; k++) {
            const double2 uv = ((const double2 *)(us + (k + 1) * ns))[e];
            double2 rv = ((double2 *)(rs + k * ns))[e];
            rv.x = rv.x - alpha * uv.x;
            rv.y = rv.y - alpha * uv.y;
            ((double2 *)(rs + k * ns))[e] = rv;
        }
        const double2 u0 = ((const double2 *)us)[e];
        if (xvec) {
            double2 xv = ((double2 *)x)[e];
            xv.x = xv.x + alpha * u0.x;
            xv.y = xv.y + alpha * u0.y;
            ((double2 *)x)[e] = xv;
        } else {
            x[2 * e] = x[2 * e] + alpha * u0.x;
            x[2 * e + 1] = x[2 * e + 1] + alpha * u0.y;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        for (int k = 0; k <= j; k++) rs[k * ns + n - 1] = rs[k * ns + n - 1] - alpha * us[(k + 1) * ns + n - 1];
        x[n - 1] = x[n - 1] + alpha * us[n - 1];
    }
}

// level 0 of dot(rs[a], rs[b]) for every a <= b (dot index d in the order (0,0), (0,1), .., (0,L), (1,1), ..) in p0[d*nb0 + q]
template <int L>
__global__ __launch_bounds__(KT) void gram_k(const double *__restrict__ rs, i64 ns, i64 n, i64 nb0, double *__restrict__ p0) {
    constexpr int ND = ndots(L);
    __shared__ double sred[ND][KT];
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
        double v[L + 1];
#pragma unroll
        for (int k = 0; k <= L; k++) v[k] = i < n ? rs[k * ns + i] : 0.0;
        int d = 0;
#pragma unroll
        for (int a = 0; a <= L; a++)
#pragma unroll
            for (int b = a; b <= L; b++) sred[d++][threadIdx.x] = v[a] * v[b];
        trees<ND>(sred, p0 + q, nb0);
    }
}

// one workgroup: M from level 2 of every dot, gamma = M[1..L,1..L] \ M[1..L,0] by the LU stated above, to the scalar block
// with omega = gamma[L] and sigma = the last BiCG step's (level 2 of sig_p1)
template <int L>
__global__ __launch_bounds__(KT) void gamma_k(const double *__restrict__ p1, i64 nb1, const double *__restrict__ sig_p1,
                                              double *__restrict__ sc) {
    __shared__ double sred[KT];
    double M[L + 1][L + 1];
    int d = 0;
#pragma unroll
    for (int a = 0; a <= L; a++)
#pragma unroll
        for (int b = a; b <= L; b++) M[a][b] = M[b][a] = level2(p1 + (d++) * nb1, nb1, sred);
    const double sigma = level2(sig_p1, nb1, sred);
    if (threadIdx.x != 0) return;
    double G[L][L], y[L], z[L];
#pragma unroll
    for (int i = 0; i < L; i++)
#pragma unroll
        for (int k = 0; k < L; k++) G[i][k] = M[i + 1][k + 1];
#pragma unroll
    for (int k = 0; k < L; k++) {
        const double inv = 1.0 / G[k][k];
#pragma unroll
        for (int i = k + 1; i < L; i++) G[i][k] = G[i][k] * inv;
#pragma unroll
        for (int c = k + 1; c < L; c++)
#pragma unroll
            for (int i = k + 1; i < L; i++) G[i][c] = G[i][c] - G[i][k] * G[k][c];
    }
#pragma unroll
    for (int i = 0; i < L; i++) {
        y[i] = M[i + 1][0];
#pragma unroll
        for (int c = 0; c < i; c++) y[i] = y[i] - G[i][c] * y[c];
    }
#pragma unroll
    for (int i = L - 1; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int c = i + 1; c < L; c++) s = s - G[i][c] * z[c];
        z[i] = s / G[i][i];
    }
#pragma unroll
    for (int i = 0; i < L; i++) sc[SC_GAMMA0 + i + 1] = z[i];
    sc[SC_OMEGA] = z[L - 1];
    sc[SC_SIGMA] = sigma;
}

// us[0] -= gamma[k]*us[k]; x += gamma[k]*rs[k-1]; rs[0] -= gamma[k]*rs[k] (k = 1..L in increasing k), with level 0 of
// dot(rs[0], rs[0]) in p0[q] and of dot(rt, rs[0]) in p0[nb0 + q]
template <int L>
__global__ __launch_bounds__(KT) void mr_k(const double *__restrict__ sc, double *__restrict__ rs, double *__restrict__ us,
                                           double *__restrict__ x, const double *__restrict__ rt, i64 ns, i64 n, i64 nb0,
                                           double *__restrict__ p0) {
    __shared__ double sred[2][KT];
    double g[L + 1];
#pragma unroll
    for (int k = 1; k <= L; k++) g[k] = sc[SC_GAMMA0 + k];
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
        double pa = 0.0, pb = 0.0;
        if (i < n) {
            double r[L + 1];
#pragma unroll
            for (int k = 0; k <= L; k++) r[k] = rs[k * ns + i];
            double u0 = us[i];
#pragma unroll
            for (int k = 1; k <= L; k++) u0 = u0 - g[k] * us[k * ns + i];
            us[i] = u0;
            double xi = x[i];
#pragma unroll
            for (int k = 1; k <= L; k++) xi = xi + g[k] * r[k - 1];
            x[i] = xi;
            double r0 = r[0];
#pragma unroll
            for (int k = 1; k <= L; k++) r0 = r0 - g[k] * r[k];
            rs[i] = r0;
            pa = r0 * r0;
            pb = rt[i] * r0;
        }
        sred[0][threadIdx.x] = pa;
        sred[1][threadIdx.x] = pb;
        trees<2>(sred, p0 + q, nb0);
    }
}

template <int L>
void minres_launch(hipStream_t st, unsigned gv, unsigned g1, double *rs, double *us, double *x, const double *rt, i64 ns, i64 n,
                   i64 nb0, i64 nb1, double *p0, double *p1_rr, double *p1_gram, const double *sig_p1, double *sc) {
    constexpr int ND = ndots(L);
    hipLaunchKernelGGL((gram_k<L>), dim3(gv), dim3(KT), 0, st, (const double *)rs, ns, n, nb0, p0);
    hipLaunchKernelGGL(fold_batch_k, dim3(g1, ND), dim3(KT), 0, st, (const double *)p0, nb0, p1_gram, nb1);
    hipLaunchKernelGGL((gamma_k<L>), dim3(1), dim3(KT), 0, st, (const double *)p1_gram, nb1, sig_p1, sc);
    hipLaunchKernelGGL((mr_k<L>), dim3(gv), dim3(KT), 0, st, (const double *)sc, rs, us, x, rt, ns, n, nb0, p0);
    hipLaunchKernelGGL(fold_batch_k, dim3(g1, 2), dim3(KT), 0, st, (const double *)p0, nb0, p1_rr, nb1);  // rr | the next rho
}

}  // namespace

extern "C" int32_t esp_bicgstabl(esp_handle *h, esp_precon *p, int32_t l, const double *b, double *x, const double *r_shadow,
                                 int32_t on_device, int32_t initially_zero, int64_t max_mv_products, double abstol, double reltol,
                                 double *history, int64_t *iterations, int64_t *mv_products, int32_t *converged) {
    if (!h || !b || !x || max_mv_products < 0 || l < 1 || l > BL_MAX) return ESP_ERR_INVALID;
    if (p && p->h != h) FAIL(h, ESP_ERR_INVALID, "esp_bicgstabl: the preconditioner belongs to another matrix");
    CK(solver_ready(h, p, "esp_bicgstabl"));
    CK(csr_current(h));
    const i64 n = h->n;
    const i64 nb0 = ceil_div<i64>(n, KT), nb1 = ceil_div<i64>(nb0, KT);
    const i64 ns = std::max<i64>((n + 31) & ~(i64)31, 32);  // a vector's stride in the block: 256-byte aligned
    const int nd = ndots(l), nvec = 2 * (l + 1) + 1;
    const size_t vbytes = sizeof(double) * (size_t)std::max<i64>(n, 1);
    esp_handle::Krylov &w = h->kry;
    CK(ensure(h, w.bv, sizeof(double) * (size_t)ns * (size_t)nvec));
    if (p) CK(ensure(h, w.t, vbytes));  // A*v in front of ILU0 / ILUAM, the unpreconditioned initial residual
    CK(ensure(h, w.part, sizeof(double) * (size_t)(nd * nb0 + (4 + nd) * nb1 + 8)));
    CK(ensure(h, w.sc, sizeof(double) * SC_COUNT));
    const double *db;
    double *dx;
    CK(stage_vectors(h, n, on_device != 0, b, x, &db, &dx));
    double *rs = (double *)w.bv.p, *us = rs + (l + 1) * ns, *rt = us + (l + 1) * ns, *t = (double *)w.t.p, *sc = (double *)w.sc.p;
    // the partial sums: level 0 of up to nd dots | level 1: rr, rho (neighbours: mr_k's two dots fold in one launch), two places
    // for sigma (bicg_dir_k reads the last one while the next is formed), the Gram matrix
    double *p0 = (double *)w.part.p, *p1 = p0 + nd * nb0;
    double *p1_rr = p1, *p1_rho = p1 + nb1, *p1_sig[2] = {p1 + 2 * nb1, p1 + 3 * nb1}, *p1_gram = p1 + 4 * nb1;
    const unsigned g0 = (unsigned)std::max<i64>(nb0, 1), g1 = (unsigned)std::max<i64>(nb1, 1);
    const unsigned gv = (unsigned)std::min<i64>(std::max<i64>(nb0, 1), KGRID);
    const double *const nil = nullptr;
    auto fold = [&](double *dst) { hipLaunchKernelGGL(fold_k, dim3(g1), dim3(KT), 0, h->stream, (const double *)p0, nb0, dst); };
    // every A*v, Pl \ v and Pl \ (A*v) below, level 0 of dot(dst, rt) when a dot product is wanted
    const PreconProduct pp{h, fused_precon(p), block_permuted(p) ? p : nullptr, n, nb0, g0, gv, p0, t};
    // residual = norm(rs[0]) from its level 1 in p1_rr: one read-back (the stop test runs on the host)
    auto residual = [&](double *out) -> int32_t {
        if (n == 0) {
            *out = 0.0;
            return ESP_OK;
        }
        hipLaunchKernelGGL(finish_k, dim3(1), dim3(KT), 0, h->stream, (const double *)p1_rr, nb1, sc + SC_OUT);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, sc + SC_OUT, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        *out = sqrt(*(const double *)h->pin_scalar);
        return ESP_OK;
    };
    int64_t mv = initially_zero ? 0 : 1;
    if (n > 0) {
        hipLaunchKernelGGL(init_scalars_k, dim3(1), dim3(64), 0, h->stream, sc);
        HIPCK(h, hipMemsetAsync(us, 0, sizeof(double) * (size_t)ns * (size_t)(l + 1), h->stream));  // us = 0
        double *r0 = p ? t : rs;  // the unpreconditioned initial residual
        if (!initially_zero) pp.mul(dx, rs + ns, rt, false);  // A*x in rs[1], which is free until the first BiCG step
        hipLaunchKernelGGL(start_k, dim3(gv), dim3(KT), 0, h->stream, db, initially_zero ? nil : (const double *)(rs + ns), r0, n, nb0,
                           p0);
        if (p) CK(pp.ldiv(r0, rs, rt, false));  // rs[0] = Pl \ r0
        const double *src = nullptr;
        if (r_shadow && on_device) src = r_shadow;
        else if (r_shadow) {
            HIPCK(h, hipMemcpyAsync(rt, r_shadow, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
            src = rt;
        }
        hipLaunchKernelGGL(shadow_k, dim3(gv), dim3(KT), 0, h->stream, src, (const double *)rs, rt, n, nb0, p0);
        hipLaunchKernelGGL(fold_batch_k, dim3(g1, 2), dim3(KT), 0, h->stream, (const double *)p0, nb0, p1_rr, nb1);
    }
    double res = 0.0;
    CK(residual(&res));
    if (history) history[0] = res;
    const double tol = std::max(reltol * res, abstol);
    int64_t it = 0;
    while (mv < max_mv_products && !(res <= tol)) {
        it++;
        if (n > 0) {
            for (int j = 0; j < l; j++) {
                double *sig = p1_sig[j & 1];
                hipLaunchKernelGGL(bicg_dir_k, dim3(gv), dim3(KT), 0, h->stream, (const double *)p1_rho,
                                   j == 0 ? nil : (const double *)p1_sig[(j - 1) & 1], (const double *)sc, nb1, j, (const double *)rs, us,
                                   ns, n);
                CK(pp.pmul(us + j * ns, us + (j + 1) * ns, rt, true));  // us[j+1] = Pl \ (A*us[j]), level 0 of sigma
                fold(sig);
                hipLaunchKernelGGL(bicg_upd_k, dim3(gv), dim3(KT), 0, h->stream, (const double *)p1_rho, (const double *)sig, nb1, j, rs,
                                   (const double *)us, dx, ns, n);
                CK(pp.pmul(rs + j * ns, rs + (j + 1) * ns, rt, j + 1 < l));  // rs[j+1] = Pl \ (A*rs[j]), level 0 of the next rho
                if (j + 1 < l) fold(p1_rho);
            }
            const double *sig_last = p1_sig[(l - 1) & 1];
            switch (l) {
            case 1: minres_launch<1>(h->stream, gv, g1, rs, us, dx, rt, ns, n, nb0, nb1, p0, p1_rr, p1_gram, sig_last, sc); break;
            case 2: minres_launch<2>(h->stream, gv, g1, rs, us, dx, rt, ns, n, nb0, nb1, p0, p1_rr, p1_gram, sig_last, sc); break;
            case 3: minres_launch<3>(h->stream, gv, g1, rs, us, dx, rt, ns, n, nb0, nb1, p0, p1_rr, p1_gram, sig_last, sc); break;
            default: minres_launch<4>(h->stream, gv, g1, rs, us, dx, rt, ns, n, nb0, nb1, p0, p1_rr, p1_gram, sig_last, sc); break;
            }
        }
        mv += 2 * (int64_t)l;
        CK(residual(&res));
        if (history) history[it] = res;
    }
    if (iterations) *iterations = it;
    if (mv_products) *mv_products = mv;
    if (converged) *converged = res <= tol ? 1 : 0;
    return return_x(h, n, on_device != 0, x, dx);
}
