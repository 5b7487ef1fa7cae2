// gmres_many.hip -- libesparse_hip: restarted GMRES for several right-hand sides (esp_gmres_many)
// (see internal.hpp for the map of the translation units; gmres.hip states the algorithm, gmres.hpp holds the kernel bodies)
//
// esp_gmres_many runs k INDEPENDENT recurrences of gmres.hip's esp_gmres in lockstep, ESP_MANY_CHUNK = 8 columns at a time.  This is
// not block GMRES: every column has its own Krylov basis, H, nullvec, rhs / y, beta, acc, current, tolerance, DGKS predicate and
// pass counter, and its chain of separately rounded operations is exactly the single call's -- x[:, r], the whole residual history
// of r, its iterations, matrix-vector products, correction passes and converged flag are bit for bit what esp_gmres gives for
// column r alone.  What the columns share is what does not round: one launch of every kernel per iteration, ONE read-back, and in
// the preconditioned product one read of A's (and ILU0's) index and values per row for the whole chunk.  The orthogonalisation
// shares no reads: every column streams its own basis, so lockstep saves launches and synchronisations there, not bytes.
//
// Layout.  Basis vector j of column d sits at V + (j*8 + d)*ns, ns the single call's 256-byte-aligned stride: "vector j of all 8
// columns" is an n x 8 column-major block with leading dimension ns -- the (src, lds) shape the many-column row kernels take -- and
// the basis of one column has the stride vs = 8*ns between its vectors; double2 accesses stay legal.  The scalar state is eight
// copies of gmres.hpp's scalar block side by side (stride SCS); column d's level-0 partials of the batched dot products start at
// p0 + d*restart*nb0, those of a single dot product at p0 + d*nb0 (the shape the product kernels emit), its level-1 places at
// slot + d*nb1 and batch + d*restart*nb1.
//
// Lockstep.  A chunk shares the iteration counter `it` and the position in the cycle `kpos`: all live columns started together,
// so they restart together.  The set of live columns goes to every kernel as a plain bit-mask ARGUMENT (krylov_many.hpp); there is no
// device flag for liveness, no fence, and a value crosses workgroups only at a kernel boundary.  The vector kernels have the
// columns on gridDim.y (gm_fold_many_k: gridDim.z): workgroup (x, d) runs gmres.hpp's body over column d exactly as the single
// kernel's workgroup x does, and returns at once when d is not live or (DGKS correction passes) its device predicate is false.
// A frozen column's basis, scalars, x, history and counters are never touched again; a NaN residual keeps its column live to
// maxiter.  Two launches take no mask and pass over the partial sums of frozen columns as well, which nothing reads afterwards:
// krylov.hpp's fold_batch_k (gridDim.y = the chunk's nr columns) folds a frozen column's stale level-0 partials into its level-1
// place, and the start_many_k that copies a Cholesky / LU-panel solve into the basis writes level 0 of a dot product nobody wants.
// The read-back goes to the handle's pin_many (16 doubles of its own), not to the 8 slots of pin_scalar.
// One iteration for the live columns:
//   1. W = Pl \ (A*V[kpos-1]) into V[kpos], with (MGS) level 0 of dot(V[0], w): Identity row_dot_many_k<MUL_DOT>; Jacobi
//      row_jac_dot_many_k; ILU0 the product into the scratch, then row_chain_many_k and row_dot_many_k<UPPER_DOT>; Cholesky and the
//      LU panels chol_solve_many / lup_solve_many over the chunk's first nr columns (a frozen column is solved into scratch nobody
//      reads); ILUAM and the kinds that end in it precon_levels_many_launch, one pass over the level schedules for the live columns;
//      AMG and SPAI-1 PreconProduct::ldiv per live column; the last three followed by one dot_many_k when MGS wants its dot
//   2. MGS: fold_batch_k, then kpos times mgs_step_many_k + fold_batch_k.  CGS / DGKS: bdot_many_k, gm_fold_many_k, coef_many_k,
//      comb_many_k<true>, gm_fold_many_k; DGKS then pred_many_k and the same five kernels three times, unconditionally
//   3. norm_many_k: H column, nullvec, acc, current; current and the pass count of column d to out[2d], out[2d + 1]
//   4. kpos++, it++, ONE read-back of 16*nr bytes; the host keeps every live column's history, iterations and products
//   5. the ending columns: every live one when kpos == restart+1 or it == maxiter, else those with current <= tol
//   6. for the ending columns alone, m = kpos-1: lsq_many_k (a workgroup's first lane per column), comb_many_k<false> on their x
//   7. converged columns leave the live set; the others keep kpos
//   8. only at kpos == restart+1: kpos = 1 and, if it < maxiter, the init sequence (never "initially zero") for the live columns
// The launch count of an iteration equals one column's.  A column with current <= tol at the start never enters the loop and gets
// no x update.  Resource usage and measurements: NOTES/gmres_many.md.
#include "gmres.hpp"
#include "krylov_many.hpp"

namespace {

constexpr int SCS = (SC_COUNT + 1) & ~1;  // a column's scalar block, rounded up to even

__global__ __launch_bounds__(KT) void gm_scalars_many_k(double *__restrict__ sc) { gm_scalars(sc + (i64)blockIdx.x * SCS); }

// level 1 of gridDim.y dot products of gridDim.z columns: column d has its partial0 at p0 + d*cs0 and its partial1 at p1 + d*cs1
__global__ __launch_bounds__(KT) void gm_fold_many_k(const double *__restrict__ p0, i64 cs0, i64 nb0, double *__restrict__ p1, i64 cs1, i64 nb1,
                                                     const double *__restrict__ sc, int behind, u32 live) {
    __shared__ double sred[KT];
    const int d = blockIdx.z;
    if (!is_live(live, d) || (behind && sc[(i64)d * SCS + SC_FLAG] == 0.0)) return;
    fold_batch(p0 + (i64)d * cs0, nb0, p1 + (i64)d * cs1, nb1, sred);
}

// v: the block of V[0]; p1: a level-1 place.  first: current and a zero pass count to out as well
__global__ __launch_bounds__(KT) void gm_start_many_k(const double *__restrict__ p1, i64 nb1, double *__restrict__ v, i64 ns, i64 n,
                                                      double *__restrict__ sc, int first, double *__restrict__ out, u32 live) {
    __shared__ double sred[KT];
    const int d = blockIdx.y;
    if (!is_live(live, d)) return;
    double *scd = sc + (i64)d * SCS;
    gm_start(p1 + (i64)d * nb1, nb1, v + (i64)d * ns, n, scd, first, sred);
    if (first && blockIdx.x == 0 && threadIdx.x == 0) {
        out[2 * d] = scd[SC_OUT];
        out[2 * d + 1] = scd[SC_PASSES];
    }
}

// vi, w, vnext: the blocks of V[i], V[kpos], V[i+1]; hoff: the place of H[i,kpos] in a scalar block
__global__ __launch_bounds__(KT) void mgs_step_many_k(const double *__restrict__ p1, i64 nb1, const double *__restrict__ vi,
                                                      double *__restrict__ w, const double *__restrict__ vnext, i64 ns, i64 n, i64 nb0,
                                                      double *__restrict__ p0, double *__restrict__ sc, int hoff, u32 live) {
    __shared__ __align__(16) double sred[2][KT];
    const int d = blockIdx.y;
    if (!is_live(live, d)) return;
    gm_mgs_step(p1 + (i64)d * nb1, nb1, vi + (i64)d * ns, w + (i64)d * ns, vnext ? vnext + (i64)d * ns : nullptr, n, nb0, p0 + (i64)d * nb0,
                sc + (i64)d * SCS + hoff, sred);
}

// V: the block of V[0]; w: the block of V[kpos]; one group of GM_GROUP trees (16 KiB of LDS) per workgroup, as the single kernel
__global__ __launch_bounds__(KT) void bdot_many_k(const double *__restrict__ V, i64 ns, i64 vs, int k, const double *__restrict__ w, i64 n,
                                                  i64 nb0, double *__restrict__ p0, i64 cs0, const double *__restrict__ sc, int behind,
                                                  u32 live) {
    __shared__ double sred[GM_GROUP][KT];
    const int d = blockIdx.y;
    if (!is_live(live, d) || (behind && sc[(i64)d * SCS + SC_FLAG] == 0.0)) return;
    gm_bdot(V + (i64)d * ns, vs, k, w + (i64)d * ns, n, nb0, p0 + (i64)d * cs0, sred);
}

__global__ __launch_bounds__(KT) void coef_many_k(const double *__restrict__ p1, i64 cs1, i64 nb1, int k, double *__restrict__ sc, int pass,
                                                  u32 live) {
    __shared__ double sred[KT];
    const int d = blockIdx.y;
    if (!is_live(live, d)) return;
    gm_coef(p1 + (i64)d * cs1, nb1, k, sc + (i64)d * SCS, pass, sred);
}

// a: n x 8 with leading dimension lda (SUB: the block of V[kpos]; else the caller's x); the coefficients at coff of a scalar block
template <bool SUB>
__global__ __launch_bounds__(KT) void comb_many_k(const double *__restrict__ V, i64 ns, i64 vs, int m, int coff, double *__restrict__ a, i64 lda,
                                                  i64 n, i64 nb0, double *__restrict__ p0, i64 cs0, const double *__restrict__ sc, int behind,
                                                  u32 live) {
    __shared__ double sred[KT];
    __shared__ double sco[GM_MAX];
    const int d = blockIdx.y;
    if (!is_live(live, d) || (behind && sc[(i64)d * SCS + SC_FLAG] == 0.0)) return;
    gm_comb<SUB>(V + (i64)d * ns, vs, m, sc + (i64)d * SCS + coff, a + (i64)d * lda, n, nb0, p0 ? p0 + (i64)d * cs0 : nullptr, sred, sco);
}

__global__ __launch_bounds__(KT) void pred_many_k(const double *__restrict__ p1, i64 nb1, double *__restrict__ sc, double eta, int first,
                                                  u32 live) {
    __shared__ double sred[KT];
    const int d = blockIdx.y;
    if (!is_live(live, d)) return;
    gm_pred(p1 + (i64)d * nb1, nb1, sc + (i64)d * SCS, eta, first, sred);
}

// w: the block of V[kpos]; hoff: where a scalar block holds H[0..k-1,k-1]; current and the pass count of column d to out[2d], out[2d+1]
__global__ __launch_bounds__(KT) void norm_many_k(const double *__restrict__ p1, i64 nb1, double *__restrict__ w, i64 ns, i64 n, double *sc, int k,
                                                  int hoff, double *__restrict__ out, u32 live) {
    __shared__ double sred[KT];
    const int d = blockIdx.y;
    if (!is_live(live, d)) return;
    double *scd = sc + (i64)d * SCS;
    gm_norm(p1 + (i64)d * nb1, nb1, w + (i64)d * ns, n, scd, k, scd + hoff, sred);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out[2 * d] = scd[SC_OUT];
        out[2 * d + 1] = scd[SC_PASSES];
    }
}

// workgroup d, one thread: the rotations and the back substitution of column d when it is ending
__global__ void lsq_many_k(double *__restrict__ sc, int m, u32 ending) {
    if (threadIdx.x != 0 || !is_live(ending, (int)blockIdx.x)) return;
    gm_lsq(sc + (i64)blockIdx.x * SCS, m);
}

}  // namespace

extern "C" int32_t esp_gmres_many(esp_handle *h, esp_precon *p, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k,
                                  int32_t on_device, int32_t initially_zero, int32_t restart, int32_t orth_meth, int64_t maxiter,
                                  double abstol, double reltol, double *history, int64_t *iterations, int64_t *mv_products,
                                  int64_t *reorth_passes, int32_t *converged) {
    if (!h || maxiter < 0 || restart < 1 || restart > GM_MAX || orth_meth < ESP_ORTH_MGS || orth_meth > ESP_ORTH_DGKS) return ESP_ERR_INVALID;
    if (p && p->h != h) FAIL(h, ESP_ERR_INVALID, "esp_gmres_many: the preconditioner belongs to another matrix");
    const i64 n = h->n, ldmin = std::max<i64>(n, 1);
    if (k < 0 || ldb < ldmin || ldx < ldmin)
        FAIL(h, ESP_ERR_INVALID, "esp_gmres_many: k = %lld, ldb = %lld, ldx = %lld for n = %lld", (long long)k, (long long)ldb,
             (long long)ldx, (long long)n);
    if (k > 0 && n > 0) {
        if (!B || !X) return ESP_ERR_INVALID;
        if (B < X + (k - 1) * ldx + n && X < B + (k - 1) * ldb + n) FAIL(h, ESP_ERR_INVALID, "esp_gmres_many: B and X overlap");
    }
    if (k == 1 && n > 0 && p) many_note(p, 0, 0, 0);
    if (k == 1 && n > 0)  // the single-vector path itself
        return esp_gmres(h, p, B, X, on_device, initially_zero, restart, orth_meth, maxiter, abstol, reltol, history, iterations, mv_products,
                         reorth_passes, converged);
    CK(solver_ready(h, p, "esp_gmres"));
    CK(csr_current(h));
    if (k == 0) return ESP_OK;
    const i64 hstride = maxiter + 1;
    if (n == 0) {  // current = 0 <= tol = 0: no iteration, converged
        for (i64 r = 0; r < k; r++) {
            if (history) history[r * hstride] = 0.0;
            if (iterations) iterations[r] = 0;
            if (mv_products) mv_products[r] = 0;
            if (reorth_passes) reorth_passes[r] = 0;
            if (converged) converged[r] = 1;
        }
        return ESP_OK;
    }
    const i64 nb0 = ceil_div<i64>(n, KT), nb1 = ceil_div<i64>(nb0, KT);
    const i64 ns = std::max<i64>((n + 31) & ~(i64)31, 32);  // a vector's stride in the block: 256-byte aligned
    const i64 vs = (i64)MC * ns;                            // from a vector of a column to its next: a block of the chunk
    esp_handle::Krylov &w = h->kry;
    // what Pl \ v is taken from: the branches below, and PreconProduct::ldiv for every kind that has no many-column form
    esp_precon *const fp = fused_precon(p), *const blk = block_permuted(p) ? p : nullptr;
    const bool lup = p && block_built(p) && p->lup;
    const bool jac = !lup && fp && !blk && diag_applied(fp), ilu0 = !lup && fp && !blk && !jac && fp->kind == ESP_PRECON_ILU0;
    const bool chol = !lup && fp && !blk && fp->kind == ESP_PRECON_CHOLESKY;
    esp_precon *const lev = lup ? nullptr : blk ? blk : fp && fp->kind == ESP_PRECON_ILUAM ? fp : nullptr;  // (levels_many's kinds)
    const bool mgs = orth_meth == ESP_ORTH_MGS;
    CK(ensure(h, w.bv, sizeof(double) * (size_t)vs * (size_t)(restart + 1)));
    // A*v and the unpreconditioned residual; behind it ILU0's pass 1, or where Cholesky and the LU panels solve the whole chunk
    if (p) CK(ensure(h, w.t, sizeof(double) * (size_t)vs * (ilu0 || lup || chol ? 2 : 1)));
    const i64 cs0 = (i64)restart * nb0, cs1 = (i64)restart * nb1;             // a column's batched partials
    CK(ensure(h, w.part, sizeof(double) * (size_t)(MC * (cs0 + 2 * nb1 + cs1) + 2 * MC)));
    CK(ensure(h, w.sc, sizeof(double) * (size_t)SCS * MC));
    if (!on_device) {
        CK(ensure(h, w.hb, sizeof(double) * (size_t)n * MC));
        CK(ensure(h, w.hx, sizeof(double) * (size_t)n * MC));
    }
    double *V = (double *)w.bv.p, *T = (double *)w.t.p, *U1 = T + vs, *sc = (double *)w.sc.p;
    // the partial sums: level 0 | level 1: two places the single dots alternate between, the batch of the CGS / DGKS passes | out
    double *p0 = (double *)w.part.p, *slot[2] = {p0 + MC * cs0, p0 + MC * cs0 + MC * nb1}, *p1_batch = p0 + MC * cs0 + 2 * MC * nb1;
    double *d_out = p1_batch + MC * cs1;
    const unsigned g0 = (unsigned)nb0, g1 = (unsigned)nb1, gv = (unsigned)std::min<i64>(nb0, KGRID);
    // the grids of the kernels that have the columns on gridDim.y: a quarter of the single call's workgroups per column
    const unsigned gx = (unsigned)std::min<i64>(nb0, KGRID / 4), gx2 = (unsigned)std::min<i64>((nb0 + 1) >> 1, KGRID / 4);
    const PreconProduct pp{h, fp, blk, n, nb0, g0, gv, p0, nullptr};
    const double *const nil = nullptr;
    double *const nilw = nullptr;
    const double eta = 1.0 / sqrt(2.0);
    hipStream_t st = h->stream;
    for (i64 r0 = 0; r0 < k; r0 += MC) {
        const int nr = (int)std::min<i64>(MC, k - r0);
        const unsigned ny = (unsigned)nr;
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
            hipLaunchKernelGGL(fold_batch_k, dim3(g1, ny), dim3(KT), 0, st, (const double *)p0, nb0, p1, nb1);
        };
        // dst = Pl \ src (blocks with leading dimension ns), with level 0 of dot(dst, V[0]) when dot
        auto solve = [&](const double *src, double *dst, bool dot, u32 live) -> int32_t {
            many_note(p, lup || chol || lev || jac || ilu0 ? 2 : 1, nr, r0 / MC + 1);
            if (jac) {
                jacobi_many(fp, src, ns, dst, ns, nilw, live);
            } else if (ilu0) {
                ilu0_many(fp, src, ns, U1, ns, V, ns, dst, ns, dot ? p0 : nilw, live);
                return ESP_OK;
            } else if (lup || chol) {  // the chunk's first nr columns into scratch, the live ones from there into dst (start_many_k: a copy)
                if (lup) CK(lup_solve_many(p, src, ns, U1, ns, nr));
                else CK(chol_solve_many(fp, src, ns, U1, ns, nr));
                hipLaunchKernelGGL(start_many_k, dim3(gv), dim3(KT), 0, st, (const double *)U1, ns, nil, dst, ns, n, nb0, p0, live);
            } else if (lev) {  // one pass over the level schedules
                CK(precon_levels_many_launch(lev, src, ns, dst, ns, nr, live));
            } else {
                for (int d = 0; d < nr; d++)
                    if (is_live(live, d)) CK(pp.ldiv(src + d * ns, dst + d * ns, src + d * ns, false));
            }
            if (dot)
                hipLaunchKernelGGL(dot_many_k, dim3(gv), dim3(KT), 0, st, nil, (const double *)dst, ns, (const double *)V, ns, nilw, (i64)0, n, nb0,
                                   p0, live);
            return ESP_OK;
        };
        // dst = Pl \ (A*src)
        auto product = [&](const double *src, double *dst, bool dot, u32 live) -> int32_t {
            if (!p) {
                mul_many(h, src, ns, V, ns, dst, ns, dot ? p0 : nilw, live);
            } else if (jac) {
                mul_jacobi_many(h, fp, src, ns, V, ns, dst, ns, dot ? p0 : nilw, live);
            } else {
                mul_many(h, src, ns, nil, 0, T, ns, nilw, live);
                CK(solve(T, dst, dot, live));
            }
            return ESP_OK;
        };
        // V[0] = Pl \ b or Pl \ (b - A*x), normalised; beta, acc = 1 (first: current = beta) to the scalar blocks
        auto init = [&](bool zero, bool first, u32 live) -> int32_t {
            double *R0 = p ? T : V;  // the unpreconditioned residual
            if (!zero) mul_many(h, dX, dldx, nil, 0, V + vs, ns, nilw, live);  // A*x in V[1], which is free here
            hipLaunchKernelGGL(start_many_k, dim3(gv), dim3(KT), 0, st, dB, dldb, zero ? nil : (const double *)(V + vs), R0, ns, n, nb0, p0, live);
            if (p) {
                CK(solve(R0, V, false, live));
                hipLaunchKernelGGL(dot_many_k, dim3(gv), dim3(KT), 0, st, nil, (const double *)V, ns, (const double *)V, ns, nilw, (i64)0, n, nb0,
                                   p0, live);
            }
            fold(slot[0]);
            hipLaunchKernelGGL(gm_start_many_k, dim3(gx, ny), dim3(KT), 0, st, (const double *)slot[0], nb1, V, ns, n, sc, first ? 1 : 0, d_out,
                               live);
            return ESP_OK;
        };
        // current and the pass counter of every column of the chunk: the one read-back of an iteration
        double cur[MC], tol[MC];
        int64_t passes[MC], its[MC], mv[MC];
        auto read_back = [&](u32 live) -> int32_t {
            HIPCK(h, hipGetLastError());
            HIPCK(h, hipMemcpyAsync(h->pin_many, d_out, 16 * (size_t)nr, hipMemcpyDeviceToHost, st));
            HIPCK(h, hipStreamSynchronize(st));
            for (int d = 0; d < nr; d++)
                if (is_live(live, d)) {
                    cur[d] = h->pin_many[2 * d];
                    passes[d] = (int64_t)h->pin_many[2 * d + 1];
                }
            return ESP_OK;
        };
        // one CGS pass (pass 0) or DGKS correction pass (1..3, behind each column's device predicate) at position kp
        auto cgs_pass = [&](double *W, int kp, int pass, u32 live) {
            const int behind = pass > 0 ? 1 : 0;
            hipLaunchKernelGGL(bdot_many_k, dim3(gx, ny), dim3(KT), 0, st, (const double *)V, ns, vs, kp, (const double *)W, n, nb0, p0, cs0,
                               (const double *)sc, behind, live);
            hipLaunchKernelGGL(gm_fold_many_k, dim3(g1, (unsigned)kp, ny), dim3(KT), 0, st, (const double *)p0, cs0, nb0, p1_batch, cs1, nb1,
                               (const double *)sc, behind, live);
            hipLaunchKernelGGL(coef_many_k, dim3(1, ny), dim3(KT), 0, st, (const double *)p1_batch, cs1, nb1, kp, sc, pass, live);
            hipLaunchKernelGGL((comb_many_k<true>), dim3(gx, ny), dim3(KT), 0, st, (const double *)V, ns, vs, kp, pass > 0 ? SC_CV : SC_HV, W, ns,
                               n, nb0, p0, cs0, (const double *)sc, behind, live);
            hipLaunchKernelGGL(gm_fold_many_k, dim3(g1, 1, ny), dim3(KT), 0, st, (const double *)p0, cs0, nb0, slot[0], nb1, nb1,
                               (const double *)sc, behind, live);
        };

        u32 live = all_live(nr);
        hipLaunchKernelGGL(gm_scalars_many_k, dim3(ny), dim3(KT), 0, st, sc);
        CK(init(initially_zero != 0, true, live));
        CK(read_back(live));
        for (int d = 0; d < nr; d++) {
            if (history) history[(r0 + d) * hstride] = cur[d];
            tol[d] = std::max(reltol * cur[d], abstol);
            its[d] = 0;
            mv[d] = initially_zero ? 0 : 1;
            if (cur[d] <= tol[d]) live &= ~(1u << d);
        }
        int kpos = 1;
        int64_t it = 0;
        while (live && it < maxiter) {
            double *W = V + (i64)kpos * vs;
            CK(product(V + (i64)(kpos - 1) * vs, W, mgs, live));
            const double *nrm_p1;
            int hoff;
            if (mgs) {
                fold(slot[0]);
                for (int i = 0; i < kpos; i++) {
                    hipLaunchKernelGGL(mgs_step_many_k, dim3(gx2, ny), dim3(KT), 0, st, (const double *)slot[i & 1], nb1,
                                       (const double *)(V + (i64)i * vs), W, i + 1 < kpos ? (const double *)(V + (i64)(i + 1) * vs) : nil, ns, n,
                                       nb0, p0, sc, SC_H + (kpos - 1) * GM_LD + i, live);
                    fold(slot[(i + 1) & 1]);
                }
                nrm_p1 = slot[kpos & 1];
                hoff = SC_H + (kpos - 1) * GM_LD;
            } else {
                cgs_pass(W, kpos, 0, live);
                if (orth_meth == ESP_ORTH_DGKS)
                    for (int pass = 1; pass <= 3; pass++) {
                        hipLaunchKernelGGL(pred_many_k, dim3(1, ny), dim3(KT), 0, st, (const double *)slot[0], nb1, sc, eta, pass == 1 ? 1 : 0,
                                           live);
                        cgs_pass(W, kpos, pass, live);
                    }
                nrm_p1 = slot[0];
                hoff = SC_HV;
            }
            hipLaunchKernelGGL(norm_many_k, dim3(gx, ny), dim3(KT), 0, st, nrm_p1, nb1, W, ns, n, sc, kpos, hoff, d_out, live);
            kpos++;
            it++;
            CK(read_back(live));
            u32 ending = 0;
            for (int d = 0; d < nr; d++) {
                if (!is_live(live, d)) continue;
                if (history) history[(r0 + d) * hstride + it] = cur[d];
                its[d] = it;
                mv[d]++;
                if (kpos == restart + 1 || it == maxiter || cur[d] <= tol[d]) ending |= 1u << d;
            }
            if (ending) {  // y and x = x + V[0..m-1]*y of the ending columns, m = kpos-1
                hipLaunchKernelGGL(lsq_many_k, dim3(ny), dim3(64), 0, st, sc, kpos - 1, ending);
                hipLaunchKernelGGL((comb_many_k<false>), dim3(gx, ny), dim3(KT), 0, st, (const double *)V, ns, vs, kpos - 1, (int)SC_RHS, dX, dldx,
                                   n, nb0, nilw, (i64)0, (const double *)sc, 0, ending);
            }
            for (int d = 0; d < nr; d++)
                if (is_live(live, d) && cur[d] <= tol[d]) live &= ~(1u << d);
            if (kpos == restart + 1) {
                kpos = 1;
                if (live && it < maxiter) {
                    CK(init(false, false, live));
                    for (int d = 0; d < nr; d++)
                        if (is_live(live, d)) mv[d]++;
                }
            }
        }
        for (int d = 0; d < nr; d++) {
            if (iterations) iterations[r0 + d] = its[d];
            if (mv_products) mv_products[r0 + d] = mv[d];
            if (reorth_passes) reorth_passes[r0 + d] = passes[d];
            if (converged) converged[r0 + d] = cur[d] <= tol[d] ? 1 : 0;
        }
        HIPCK(h, hipGetLastError());
        if (!on_device)
            HIPCK(h, hipMemcpy2DAsync(X + r0 * ldx, sizeof(double) * (size_t)ldx, dX, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n,
                                      (size_t)nr, hipMemcpyDeviceToHost, st));
    }
    HIPCK(h, hipStreamSynchronize(st));
    return ESP_OK;
}
