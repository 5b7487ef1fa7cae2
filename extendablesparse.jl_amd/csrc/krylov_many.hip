// krylov_many.hip -- libesparse_hip: conjugate gradients for several right-hand sides (esp_cg_many) and the many-column forms
// of Jacobi's and ILU0's ldiv! (precon_ldiv_many_launch, behind esp_precon_ldiv_many)
// (see internal.hpp for the map of the translation units)
//
// esp_cg_many runs k INDEPENDENT recurrences of krylov.hip's esp_cg in lockstep, ESP_MANY_CHUNK = 8 columns at a time.  This is
// not block CG: every column has its own rho, beta, alpha, residual, tolerance and stopping test, and its chain of separately
// rounded operations is exactly the single call's -- x[:, r], the whole residual history of r, its iteration count and its
// converged flag are bit for bit what esp_cg gives for column r alone.  What the columns share is what does not round: one read of
// A's (or the ILU0 parts') index and values per row for the whole chunk, one launch of every kernel per iteration, one read-back.
//
// The summation shape (krylov.hip states it) is kept per column: level 0 of all the chunk's dot products comes from krylov.hpp's
// trees<8> (the same pairs in the same order as tree256), level 1 from fold_batch_k with the columns on gridDim.y, level 2 is redone
// per workgroup and column through trees<8> again (level2_many).  Every division is a true double division, nothing is contracted.
//
// Lockstep and freezing.  All columns of a chunk share the iteration counter, so the alternating rho slot works per chunk.  After
// each iteration the host reads back the chunk's residual sums of squares in ONE copy of 8*nr bytes, takes the square roots and
// runs each column's stop test.  A column that has stopped is frozen: the set of live columns goes to every kernel of the next
// iteration as a plain bit-mask ARGUMENT (no device flag, no fence), the kernels skip a frozen column's loads and stores (a
// wave-uniform branch), and its x, r and history slots are never written again.  A NaN residual keeps its column live to maxiter,
// as in the single call.  The chunk ends when no column is live or maxiter is reached.
//
// The work vectors R, U and C (and ILU0's pass-1 scratch) are n x 8 column-major in the handle's Krylov workspace with leading
// dimension n rounded up to even: every column starts on a 16-byte boundary and can be handed to the single-vector ldiv branches.
// The caller's B and X may sit at any 8-byte-aligned address with any leading dimension: no 16-byte access touches them.
//
// Kernels of one iteration (ILU0; Jacobi and Identity have dot_many_k in place of the first two; Cholesky and LU's panel form run
// chol_solve_many / lup_solve_many over the chunk -- its first nr columns, so a frozen column is solved as well, into the scratch c
// that nobody reads --, ILUAM and the kinds that end in it precon_levels_many_launch: one pass over the level schedules for the live
// columns --, AMG and SPAI-1 PreconProduct::ldiv per live column, each followed by one dot_many_k):
//   row_chain_many_k          pass 1 of ldiv! for the live columns
//   row_dot_many_k<UPPER_DOT> pass 2, c stored, level 0 of dot(c, r)
//   fold_batch_k              level 1 (gridDim.y = the chunk's columns)
//   direction_many_k          beta = rho/rho_prev per column, u = c + beta*u
//   row_dot_many_k<MUL_DOT>   c = A*u, level 0 of dot(u, c)
//   fold_batch_k
//   update_many_k             alpha per column, x += alpha*u, r -= alpha*c, level 0 of dot(r, r)
//   fold_batch_k
//   finish_many_k             level 2 of dot(r, r) -> 8 doubles, read back in one copy
// The launch count of an iteration does not depend on the number of columns.  Resource usage: NOTES/cg_many.md.
// The live mask, level2_many, start_many_k, dot_many_k, the row kernels and their launches are krylov_many.hpp's, which
// gmres_many.hip includes as well.
#include "krylov_many.hpp"

namespace {

// ---- the vector kernels: a lane handles the elements the single kernels give it, for every live column ----------------------------
// beta = rho/rho_prev per column (rho_prev = 1 in the first iteration: prev == nullptr); u = c + beta*u, two elements per lane
// (work vectors only: their columns start on 16-byte boundaries)
__global__ __launch_bounds__(KT) void direction_many_k(const double *__restrict__ rho_p1, const double *__restrict__ prev_p1, i64 nb1,
                                                       const double *__restrict__ c, double *__restrict__ u, i64 ldw, i64 n, u32 live) {
    __shared__ double sred[MC][KT];
    __shared__ double srho[MC], sprev[MC];
    level2_many(rho_p1, nb1, live, sred, srho);
    if (prev_p1) level2_many(prev_p1, nb1, live, sred, sprev);
    double beta[MC];
#pragma unroll
    for (int d = 0; d < MC; d++) beta[d] = srho[d] / (prev_p1 ? sprev[d] : 1.0);
    const i64 n2 = n >> 1;
    for (i64 k = (i64)blockIdx.x * KT + threadIdx.x; k < n2; k += (i64)gridDim.x * KT) {
#pragma unroll
        for (int d = 0; d < MC; d++) {
            if (!is_live(live, d)) continue;
            const double2 cv = ((const double2 *)(c + (i64)d * ldw))[k];
            double2 *u2 = (double2 *)(u + (i64)d * ldw);
            double2 uv = u2[k];
            uv.x = cv.x + beta[d] * uv.x;
            uv.y = cv.y + beta[d] * uv.y;
            u2[k] = uv;
        }
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int d = 0; d < MC; d++)
            if (is_live(live, d)) u[(i64)d * ldw + n - 1] = c[(i64)d * ldw + n - 1] + beta[d] * u[(i64)d * ldw + n - 1];
    }
}
// alpha = rho / dot(u, c) per column; x = x + alpha*u; r = r - alpha*c, with level 0 of dot(r, r)
__global__ __launch_bounds__(KT) void update_many_k(const double *__restrict__ rho_p1, const double *__restrict__ uc_p1, i64 nb1,
                                                    const double *__restrict__ u, const double *__restrict__ c, double *__restrict__ r, i64 ldw,
                                                    double *__restrict__ x, i64 ldx, i64 n, i64 nb0, double *__restrict__ p0, u32 live) {
    __shared__ double sred[MC][KT];
    __shared__ double srho[MC], suc[MC];
    level2_many(rho_p1, nb1, live, sred, srho);
    level2_many(uc_p1, nb1, live, sred, suc);
    double alpha[MC];
#pragma unroll
    for (int d = 0; d < MC; d++) alpha[d] = srho[d] / suc[d];
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
#pragma unroll
        for (int d = 0; d < MC; d++) {
            double prod = 0.0;
            if (is_live(live, d) && i < n) {
                const i64 w = (i64)d * ldw + i, xi = (i64)d * ldx + i;
                x[xi] = x[xi] + alpha[d] * u[w];
                const double ri = r[w] - alpha[d] * c[w];
                r[w] = ri;
                prod = ri * ri;
            }
            sred[d][threadIdx.x] = prod;
        }
        trees<MC>(sred, p0 + q, nb0);
    }
}
// level 2 of dot(r, r) of the live columns: out[d]
__global__ __launch_bounds__(KT) void finish_many_k(const double *__restrict__ p1, i64 nb1, double *__restrict__ out, u32 live) {
    __shared__ double sred[MC][KT];
    __shared__ double sres[MC];
    level2_many(p1, nb1, live, sred, sres);
    if (threadIdx.x < MC && is_live(live, (int)threadIdx.x)) out[threadIdx.x] = sres[threadIdx.x];
}

}  // namespace

// ldiv! of Jacobi (SPAI-0) and ILU0 for k columns on device arrays (u may be v where ldu == ldv), ESP_MANY_CHUNK columns a launch:
// esp_precon_ldiv_many's branch of these kinds.  Every column is precon.hip's ldiv_launch bit for bit (ILU0's pass-1 scratch p->u1
// grows to a chunk's width)
int32_t precon_ldiv_many_launch(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, i64 k) {
    for (i64 r0 = 0; r0 < k; r0 += MC) {
        const int nr = (int)std::min<i64>(MC, k - r0);
        CK(precon_ldiv_chunk_launch(p, v + r0 * ldv, ldv, u + r0 * ldu, ldu, nr, all_live(nr)));
    }
    return ESP_OK;
}
// ... one chunk's live columns (block.hip's inner Jacobi / ILU0 under a solver's live mask: a frozen column's u is never written)
int32_t precon_ldiv_chunk_launch(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, int nr, u32 live) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    live &= all_live(nr);
    if (n == 0 || nr <= 0) return ESP_OK;
    const i64 ld1 = even_ld(n);
    if (diag_applied(p)) {
        jacobi_many(p, v, ldv, u, ldu, nullptr, live);
    } else {
        CK(ensure(h, p->u1, sizeof(double) * (size_t)ld1 * MC));
        ilu0_many(p, v, ldv, (double *)p->u1.p, ld1, nullptr, 0, u, ldu, nullptr, live);
    }
    HIPCK(h, hipGetLastError());
    return ESP_OK;
}

extern "C" int32_t esp_cg_many(esp_handle *h, esp_precon *p, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k,
                               int32_t on_device, int32_t initially_zero, int64_t maxiter, double abstol, double reltol, double *history,
                               int64_t *iterations, int32_t *converged) {
    if (!h || maxiter < 0) return ESP_ERR_INVALID;
    if (p && p->h != h) FAIL(h, ESP_ERR_INVALID, "esp_cg_many: the preconditioner belongs to another matrix");
    const i64 n = h->n, ldmin = std::max<i64>(n, 1);
    if (k < 0 || ldb < ldmin || ldx < ldmin)
        FAIL(h, ESP_ERR_INVALID, "esp_cg_many: k = %lld, ldb = %lld, ldx = %lld for n = %lld", (long long)k, (long long)ldb, (long long)ldx,
             (long long)n);
    if (k > 0 && n > 0) {
        if (!B || !X) return ESP_ERR_INVALID;
        if (B < X + (k - 1) * ldx + n && X < B + (k - 1) * ldb + n) FAIL(h, ESP_ERR_INVALID, "esp_cg_many: B and X overlap");
    }
    if (k == 1 && n > 0) {  // the single-vector path itself
        if (p) many_note(p, 0, 0, 0);
        return esp_cg(h, p, B, X, on_device, initially_zero, maxiter, abstol, reltol, history, iterations, converged);
    }
    CK(solver_ready(h, p, "esp_cg"));
    CK(csr_current(h));
    if (k == 0) return ESP_OK;
    const i64 hstride = maxiter + 1;
    if (n == 0) {  // norm(r) = 0 <= tol = 0: no iteration, converged
        for (i64 r = 0; r < k; r++) {
            if (history) history[r * hstride] = 0.0;
            if (iterations) iterations[r] = 0;
            if (converged) converged[r] = 1;
        }
        return ESP_OK;
    }
    const i64 nb0 = ceil_div<i64>(n, KT), nb1 = ceil_div<i64>(nb0, KT), ldw = even_ld(n);
    const size_t wbytes = sizeof(double) * (size_t)ldw * MC;
    esp_handle::Krylov &w = h->kry;
    // what Pl \ r is taken from: the branches below, and PreconProduct::ldiv for every kind that has no many-column form
    esp_precon *const fp = fused_precon(p), *const blk = block_permuted(p) ? p : nullptr;
    const bool lup = p && block_built(p) && p->lup;
    const bool jac = !lup && fp && !blk && diag_applied(fp), ilu0 = !lup && fp && !blk && !jac && fp->kind == ESP_PRECON_ILU0;
    const bool chol = !lup && fp && !blk && fp->kind == ESP_PRECON_CHOLESKY;
    esp_precon *const lev = lup ? nullptr : blk ? blk : fp && fp->kind == ESP_PRECON_ILUAM ? fp : nullptr;  // (levels_many's kinds)
    CK(ensure(h, w.r, wbytes));
    CK(ensure(h, w.u, wbytes));
    CK(ensure(h, w.c, wbytes));
    if (ilu0) CK(ensure(h, w.t, wbytes));
    CK(ensure(h, w.part, sizeof(double) * (size_t)(MC * nb0 + 4 * MC * nb1 + MC)));
    if (!on_device) {
        CK(ensure(h, w.hb, sizeof(double) * (size_t)n * MC));
        CK(ensure(h, w.hx, sizeof(double) * (size_t)n * MC));
    }
    double *R = (double *)w.r.p, *U = (double *)w.u.p, *Cw = (double *)w.c.p, *U1 = (double *)w.t.p;
    // the partial sums, every array with its columns side by side: level 0 | level 1 of rho (two places), dot(u, c), dot(r, r) | out
    double *p0 = (double *)w.part.p, *p1_rho[2] = {p0 + MC * nb0, p0 + MC * nb0 + MC * nb1}, *p1_uc = p0 + MC * nb0 + 2 * MC * nb1;
    double *p1_rr = p0 + MC * nb0 + 3 * MC * nb1, *d_out = p0 + MC * nb0 + 4 * MC * nb1;
    const unsigned g0 = (unsigned)nb0, g1 = (unsigned)nb1, gv = (unsigned)std::min<i64>(nb0, KGRID);
    const PreconProduct pp{h, fp, blk, n, nb0, g0, gv, p0, nullptr};
    const double *Z = p ? Cw : R;  // Pl \ r (Identity: r itself)
    hipStream_t st = h->stream;
    for (i64 r0 = 0; r0 < k; r0 += MC) {
        const int nr = (int)std::min<i64>(MC, k - r0);
        const double *dB = B + r0 * ldb;
        double *dX = X + r0 * ldx;
        i64 dldb = ldb, dldx = ldx;
        if (!on_device) {
            HIPCK(h, hipMemcpy2DAsync(w.hb.p, sizeof(double) * (size_t)n, dB, sizeof(double) * (size_t)ldb, sizeof(double) * (size_t)n, (size_t)nr,
                                      hipMemcpyHostToDevice, st));
            HIPCK(h, hipMemcpy2DAsync(w.hx.p, sizeof(double) * (size_t)n, dX, sizeof(double) * (size_t)ldx, sizeof(double) * (size_t)n, (size_t)nr,
                                      hipMemcpyHostToDevice, st));
            dB = (const double *)w.hb.p;
            dX = (double *)w.hx.p;
            dldb = dldx = n;
        }
        auto fold = [&](double *p1) {
            hipLaunchKernelGGL(fold_batch_k, dim3(g1, (unsigned)nr), dim3(KT), 0, st, (const double *)p0, nb0, p1, nb1);
        };
        double res[MC], tol[MC];
        // residual = norm(r) of the live columns from level 0 in p0: ONE read-back (the stop tests run on the host)
        auto residual = [&](u32 live) -> int32_t {
            fold(p1_rr);
            hipLaunchKernelGGL(finish_many_k, dim3(1), dim3(KT), 0, st, (const double *)p1_rr, nb1, d_out, live);
            HIPCK(h, hipGetLastError());
            HIPCK(h, hipMemcpyAsync(h->pin_scalar, d_out, sizeof(double) * (size_t)nr, hipMemcpyDeviceToHost, st));
            HIPCK(h, hipStreamSynchronize(st));
            for (int d = 0; d < nr; d++)
                if (is_live(live, d)) res[d] = sqrt(((const double *)h->pin_scalar)[d]);
            return ESP_OK;
        };
        u32 live = all_live(nr);
        HIPCK(h, hipMemsetAsync(U, 0, wbytes, st));                                                     // u = 0
        if (!initially_zero) mul_many(h, dX, dldx, nullptr, 0, Cw, ldw, nullptr, live);                 // c = A*x
        hipLaunchKernelGGL(start_many_k, dim3(gv), dim3(KT), 0, st, dB, dldb, initially_zero ? (const double *)nullptr : (const double *)Cw, R,
                           ldw, n, nb0, p0, live);
        CK(residual(live));
        int64_t its[MC];
        for (int d = 0; d < nr; d++) {
            if (history) history[(r0 + d) * hstride] = res[d];
            tol[d] = std::max(reltol * res[d], abstol);
            its[d] = 0;
            if (res[d] <= tol[d]) live &= ~(1u << d);
        }
        for (int64_t it = 1; live && it <= maxiter; it++) {
            double *rho = p1_rho[it & 1];
            // c = Pl \ r with level 0 of dot(c, r)
            if (lup || chol || (fp && !jac && !ilu0)) {
                if (lup) CK(lup_solve_many(p, R, ldw, Cw, ldw, nr));
                else if (chol) CK(chol_solve_many(fp, R, ldw, Cw, ldw, nr));
                else if (lev) CK(precon_levels_many_launch(lev, R, ldw, Cw, ldw, nr, live));  // one pass over the level schedules
                else
                    for (int d = 0; d < nr; d++)
                        if (is_live(live, d)) CK(pp.ldiv(R + d * ldw, Cw + d * ldw, R + d * ldw, false));
                hipLaunchKernelGGL(dot_many_k, dim3(gv), dim3(KT), 0, st, (const double *)nullptr, (const double *)Cw, ldw, (const double *)R, ldw,
                                   (double *)nullptr, (i64)0, n, nb0, p0, live);
            } else if (!fp) {
                hipLaunchKernelGGL(dot_many_k, dim3(gv), dim3(KT), 0, st, (const double *)nullptr, (const double *)R, ldw, (const double *)R, ldw,
                                   (double *)nullptr, (i64)0, n, nb0, p0, live);
            } else if (jac) {
                jacobi_many(fp, R, ldw, Cw, ldw, p0, live);
            } else {
                ilu0_many(fp, R, ldw, U1, ldw, R, ldw, Cw, ldw, p0, live);
            }
            if (p) many_note(p, lup || chol || lev || jac || ilu0 ? 2 : 1, nr, r0 / MC + 1);
            fold(rho);
            // rho_prev = rho; rho = dot(c, r); beta = rho/rho_prev; u = c + beta*u
            hipLaunchKernelGGL(direction_many_k, dim3(gv), dim3(KT), 0, st, (const double *)rho,
                               it == 1 ? (const double *)nullptr : (const double *)p1_rho[(it - 1) & 1], nb1, Z, U, ldw, n, live);
            mul_many(h, U, ldw, U, ldw, Cw, ldw, p0, live);  // c = A*u with level 0 of dot(u, c)
            fold(p1_uc);
            // alpha = rho / dot(u, c); x += alpha*u; r -= alpha*c
            hipLaunchKernelGGL(update_many_k, dim3(gv), dim3(KT), 0, st, (const double *)rho, (const double *)p1_uc, nb1, (const double *)U,
                               (const double *)Cw, R, ldw, dX, dldx, n, nb0, p0, live);
            CK(residual(live));
            for (int d = 0; d < nr; d++) {
                if (!is_live(live, d)) continue;
                if (history) history[(r0 + d) * hstride + it] = res[d];
                its[d] = it;
                if (res[d] <= tol[d]) live &= ~(1u << d);
            }
        }
        for (int d = 0; d < nr; d++) {
            if (iterations) iterations[r0 + d] = its[d];
            if (converged) converged[r0 + d] = res[d] <= tol[d] ? 1 : 0;
        }
        if (!on_device)
            HIPCK(h, hipMemcpy2DAsync(X + r0 * ldx, sizeof(double) * (size_t)ldx, dX, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n,
                                      (size_t)nr, hipMemcpyDeviceToHost, st));
    }
    HIPCK(h, hipStreamSynchronize(st));
    return ESP_OK;
}
