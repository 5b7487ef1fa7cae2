// krylov.hip -- libesparse_hip: preconditioned conjugate gradients (esp_cg) on the device CSC
// (see internal.hpp for the map of the translation units)
//
// The algorithm is IterativeSolvers.jl's cg! with a left preconditioner (its PCGIterable).  That package is not part of the
// reference tree: the statement sequence below is RESTATED from its documented behaviour, not read from its source.
//
//   cg!(x, A, b; Pl, abstol = 0, reltol = sqrt(eps), maxiter = n, initially_zero)
//     u = 0;  rho = 1
//     r = b                     (initially_zero)   |   c = A*x;  r = b - c   (x given)
//     residual = norm(r);  tol = max(reltol*residual, abstol)
//     for iteration = 1, 2, ...   while iteration-1 < maxiter and not residual <= tol:
//         c = Pl \ r
//         rho_prev = rho;  rho = dot(c, r);  beta = rho/rho_prev
//         u = c + beta*u                           (the product rounded, then the sum)
//         c = A*u                                  (mul! exactly as esp_mul: 0 + the row's products in increasing column)
//         alpha = rho / dot(u, c)
//         x = x + alpha*u;   r = r - alpha*c;   residual = norm(r)
//     converged = residual <= tol
//
// `not residual <= tol` is `residual > tol` for every number; a NaN residual (a breakdown: dot(u, c) = 0, an indefinite matrix)
// is no error and does not stop the loop, which then ends at maxiter, as the package's does.  Every division is a true double
// division, no product and sum is contracted.
// DEVIATION: without Pl the package switches to its unpreconditioned iterator (the same in exact arithmetic, not in rounding);
// here Pl = Identity runs the statements above with c = r (no copy is made: the kernels read r in c's place).
//
// The summation shape.  The package's dot and norm are BLAS calls whose order of summation is not defined; here every dot
// product (norm(r) = sqrt(dot(r, r))) is ONE fixed-shape sum that depends on n alone:
//   level 0  the products p[i] = a[i]*b[i] in chunks of 256 consecutive i (the last one padded with +0.0); a chunk is folded by
//            the tree  for w = 128, 64, ..., 1: s[t] = s[t] + s[t + w] (t < w);  partial0[q] = s[0]
//   level 1  the same tree over groups of 256 consecutive partial0 (padded with +0.0): partial1[g]
//   level 2  lane t of 256 adds partial1[t], partial1[t + 256], ... in that order to 0.0, then the same tree over the lanes
// (one value per lane up to n = 2^24).  So x, r and the whole residual history are identical run to run and bit-identical to
// tests/cg_model.c, which restates the statements and this shape as plain loops; against the package itself they agree to
// the rounding of the dot products only.  The sums of squares overflow for entries above about 1e154, where nrm2 would not.
//
// Kernels of one iteration (ILU0; Jacobi and Identity have one launch in place of the first two, ILUAM its level launches
// and a dot kernel -- the branches are krylov.hpp's PreconProduct::ldiv, which esp_bicgstabl and esp_gmres call as well):
//   row_chain_k<ILU_LOWER>   pass 1 of ldiv! (precon.hip, unchanged)
//   row_dot_k<UPPER_DOT>     pass 2, c[i] stored, level 0 of dot(c, r)
//   fold_k                   level 1
//   direction_k              level 2 of rho (and of rho_prev) redone by every workgroup, beta = rho/rho_prev, u = c + beta*u
//   row_dot_k<MUL_DOT>       c = A*u over the row-wise index, level 0 of dot(u, c)
//   fold_k
//   update_k                 level 2 of rho and of dot(u, c) redone, alpha, x += alpha*u, r -= alpha*c, level 0 of dot(r, r)
//   fold_k
//   finish_k                 level 2 of dot(r, r) -> one double, read back through pin_scalar; the host takes the square root
//                            (correctly rounded on both sides of the comparison with the model) and runs the stopping test
// A value crosses workgroups only at a kernel boundary: no flags, no grid barrier, no fence.  rho_prev is not kept in a slot:
// the partial1 array of rho alternates between two places, and the first iteration is told that rho_prev = 1.
#include "krylov.hpp"

namespace {

// beta = rho/rho_prev (rho_prev = 1 in the first iteration: prev == nullptr); u = c + beta*u, two elements per lane
__global__ __launch_bounds__(KT) void direction_k(const double *__restrict__ rho_p1, const double *__restrict__ prev_p1, i64 nb1,
                                                  const double *__restrict__ c, double *__restrict__ u, i64 n) {
    __shared__ double sred[KT];
    const double rho = level2(rho_p1, nb1, sred);
    const double rho_prev = prev_p1 ? level2(prev_p1, nb1, sred) : 1.0;
    const double beta = rho / rho_prev;
    const i64 n2 = n >> 1;
    const double2 *c2 = (const double2 *)c;
    double2 *u2 = (double2 *)u;
    for (i64 k = (i64)blockIdx.x * KT + threadIdx.x; k < n2; k += (i64)gridDim.x * KT) {
        const double2 cv = c2[k];
        double2 uv = u2[k];
        uv.x = cv.x + beta * uv.x;
        uv.y = cv.y + beta * uv.y;
        u2[k] = uv;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) u[n - 1] = c[n - 1] + beta * u[n - 1];
}
// alpha = rho / dot(u, c); x = x + alpha*u; r = r - alpha*c, with level 0 of dot(r, r)
__global__ __launch_bounds__(KT) void update_k(const double *__restrict__ rho_p1, const double *__restrict__ uc_p1, i64 nb1,
                                               const double *__restrict__ u, const double *__restrict__ c, double *__restrict__ x,
                                               double *__restrict__ r, i64 n, i64 nb0, double *__restrict__ p0) {
    __shared__ double sred[KT];
    const double rho = level2(rho_p1, nb1, sred);
    const double uc = level2(uc_p1, nb1, sred);
    const double alpha = rho / uc;
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
        double prod = 0.0;
        if (i < n) {
            x[i] = x[i] + alpha * u[i];
            const double ri = r[i] - alpha * c[i];
            r[i] = ri;
            prod = ri * ri;
        }
        const double t = tree256(prod, sred);
        if (threadIdx.x == 0) p0[q] = t;
        __syncthreads();
    }
}

}  // namespace

extern "C" int32_t esp_cg(esp_handle *h, esp_precon *p, const double *b, double *x, int32_t on_device, int32_t initially_zero,
                          int64_t maxiter, double abstol, double reltol, double *history, int64_t *iterations, int32_t *converged) {
    if (!h || !b || !x || maxiter < 0) return ESP_ERR_INVALID;
    if (p && p->h != h) FAIL(h, ESP_ERR_INVALID, "esp_cg: the preconditioner belongs to another matrix");
    CK(solver_ready(h, p, "esp_cg"));
    CK(csr_current(h));
    const i64 n = h->n;
    const i64 nb0 = ceil_div<i64>(n, KT), nb1 = ceil_div<i64>(nb0, KT);
    const size_t vbytes = sizeof(double) * (size_t)std::max<i64>(n, 1);
    esp_handle::Krylov &w = h->kry;
    CK(ensure(h, w.r, vbytes));
    CK(ensure(h, w.u, vbytes));
    CK(ensure(h, w.c, vbytes));
    CK(ensure(h, w.part, sizeof(double) * (size_t)(nb0 + 4 * nb1 + 8)));
    const double *db;
    double *dx;
    CK(stage_vectors(h, n, on_device != 0, b, x, &db, &dx));
    double *r = (double *)w.r.p, *u = (double *)w.u.p, *c = (double *)w.c.p;
    double *p0 = (double *)w.part.p, *p1_rho[2] = {p0 + nb0, p0 + nb0 + nb1}, *p1_uc = p0 + nb0 + 2 * nb1, *p1_rr = p0 + nb0 + 3 * nb1;
    double *d_out = p0 + nb0 + 4 * nb1;
    const unsigned g0 = (unsigned)std::max<i64>(nb0, 1), g1 = (unsigned)std::max<i64>(nb1, 1);
    const unsigned gv = (unsigned)std::min<i64>(std::max<i64>(nb0, 1), KGRID);
    auto fold = [&](double *p1) { hipLaunchKernelGGL(fold_k, dim3(g1), dim3(KT), 0, h->stream, (const double *)p0, nb0, p1); };
    const PreconProduct pp{h, fused_precon(p), block_permuted(p) ? p : nullptr, n, nb0, g0, gv, p0, nullptr};
    // residual = norm(r) from level 0 in p0: one read-back (the stop test runs on the host)
    auto residual = [&](double *out) -> int32_t {
        if (n == 0) {
            *out = 0.0;
            return ESP_OK;
        }
        fold(p1_rr);
        hipLaunchKernelGGL(finish_k, dim3(1), dim3(KT), 0, h->stream, (const double *)p1_rr, nb1, d_out);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, d_out, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        *out = sqrt(*(const double *)h->pin_scalar);
        return ESP_OK;
    };
    if (n > 0) {
        HIPCK(h, hipMemsetAsync(u, 0, sizeof(double) * (size_t)n, h->stream));  // u = 0
        if (!initially_zero) pp.mul(dx, c, dx, true);                           // c = A*x (its partials are not used)
        hipLaunchKernelGGL(start_k, dim3(gv), dim3(KT), 0, h->stream, db, initially_zero ? (const double *)nullptr : (const double *)c, r,
                           n, nb0, p0);
    }
    double res = 0.0;
    CK(residual(&res));
    if (history) history[0] = res;
    const double tol = std::max(reltol * res, abstol);
    int64_t it = 0;
    const double *z = p ? c : r;  // Pl \ r (Identity: r itself)
    while (it < maxiter && !(res <= tol)) {
        it++;
        if (n > 0) {
            double *rho = p1_rho[it & 1];
            CK(pp.ldiv(r, c, r, true));  // c = Pl \ r with level 0 of dot(c, r)
            fold(rho);
            // rho_prev = rho; rho = dot(c, r); beta = rho/rho_prev; u = c + beta*u
            hipLaunchKernelGGL(direction_k, dim3(gv), dim3(KT), 0, h->stream, (const double *)rho,
                               it == 1 ? (const double *)nullptr : (const double *)p1_rho[(it - 1) & 1], nb1, z, u, n);
            pp.mul(u, c, u, true);  // c = A*u with level 0 of dot(u, c)
            fold(p1_uc);
            // alpha = rho / dot(u, c); x += alpha*u; r -= alpha*c
            hipLaunchKernelGGL(update_k, dim3(gv), dim3(KT), 0, h->stream, (const double *)rho, (const double *)p1_uc, nb1,
                               (const double *)u, (const double *)c, dx, r, n, nb0, p0);
        }
        CK(residual(&res));
        if (history) history[it] = res;
    }
    if (iterations) *iterations = it;
    if (converged) *converged = res <= tol ? 1 : 0;
    return return_x(h, n, on_device != 0, x, dx);
}
