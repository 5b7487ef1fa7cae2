// gmres.hip -- libesparse_hip: restarted GMRES for non-symmetric systems (esp_gmres) on the device CSC
// (see internal.hpp for the map of the translation units; krylov.hpp for what this shares with esp_cg and esp_bicgstabl)
//
// The algorithm is IterativeSolvers.jl's gmres! with a left preconditioner.  That package is not part of the reference tree:
// the statement sequence below is RESTATED from its documented behaviour, not read from its source.
//
//   gmres!(x, A, b; Pl, abstol = 0, reltol = sqrt(eps), restart = min(20, n), maxiter = n, initially_zero, orth_meth)
//     V: n x (restart+1), H: (restart+1) x restart, nullvec: restart+1 entries, all 1.0
//     init:   V1 = b (initially_zero) or b - A*x (mv += 1);  V1 = Pl \ V1;  beta = norm(V1);  V1 = V1 * (1.0/beta)
//     start:  beta = init;  acc = 1;  current = beta;  tol = max(reltol*current, abstol);  k = 1;  it = 0;  history[0] = current
//     while it < maxiter and not current <= tol:
//         w = V[k+1] = Pl \ (A*V[k]);  mv += 1
//         orthogonalise w against V[1..k] -> H[1..k,k], nrm;  w = w * (1.0/nrm);  H[k+1,k] = nrm
//         s = 0;  for i = 1..k increasing: s = s + nullvec[i]*H[i,k]
//         nullvec[k+1] = -(s / H[k+1,k]);  acc = acc + nullvec[k+1]*nullvec[k+1];  current = beta / sqrt(acc)
//         k += 1;  it += 1;  history[it] = current
//         if k == restart+1  or  current <= tol  or  it == maxiter:
//             m = k-1;  rhs = (beta, 0, .., 0) of length k
//             for i = 1..m:                                      (Givens, column by column)
//                 f = H[i,i];  g = H[i+1,i];  g == 0 ? (c,s) = (1,0) : (r = sqrt(f*f + g*g);  c = f/r;  s = g/r)
//                 H[i,i] = c*f + s*g
//                 for j = i+1..m:  t = -s*H[i,j] + c*H[i+1,j];  H[i,j] = c*H[i,j] + s*H[i+1,j];  H[i+1,j] = t
//                 t = -s*rhs[i] + c*rhs[i+1];  rhs[i] = c*rhs[i] + s*rhs[i+1];  rhs[i+1] = t
//             for i = m..1:  z = rhs[i];  for j = i+1..m increasing:  z = z - H[i,j]*rhs[j];  rhs[i] = z / H[i,i]
//             x[e] = (..((x[e] + rhs[1]*V[e,1]) + rhs[2]*V[e,2]) ..) + rhs[m]*V[e,m]
//             k = 1
//             if not current <= tol and it < maxiter:  beta = init (never initially_zero; mv += 1);  acc = 1   (current is NOT reset)
//     converged = current <= tol
//   orthogonalise, orth_meth = ESP_ORTH_MGS:  for i = 1..k:  H[i,k] = dot(V[i], w);  w = w - H[i,k]*V[i];    nrm = norm(w)
//   ESP_ORTH_CGS:   h[j] = dot(V[j], w) for j = 1..k, all from the same w;  w[e] = (..(w[e] - h[1]*V[e,1]) - ..) - h[k]*V[e,k];
//                   nrm = norm(w);  H[1..k,k] = h
//   ESP_ORTH_DGKS:  CGS, then  proj = sqrt(h[1]^2 + .. + h[k]^2) (sequential from 0.0);  eta = 1.0/sqrt(2.0);
//                   while nrm < eta*proj and passes < 3:  c[j] = dot(V[j], w);  proj = that norm of c;  w -= the same ordered
//                   combination with c;  h[j] = h[j] + c[j];  nrm = norm(w);  passes += 1       (a NaN ends the loop)
//
// mul! is esp_mul's and ldiv! esp_precon_ldiv's, bit for bit; dot is esp_cg's ordered sum (krylov.hip states the shape),
// norm(v) = sqrt(dot(v, v)); every product is rounded before its sum, every division and square root is the correctly rounded one.
// A breakdown (nrm = 0 without convergence, a singular H) is no error: Inf and NaN propagate and a NaN residual never stops the
// loop, which ends at maxiter.  A lucky breakdown gives current = 0: converged, x exact (n = 1 always ends so after one iteration).
// b = 0 from x = 0: history = [0], no iteration, x untouched.
// DEVIATIONS from the package: dot, norm and the two gemv's (BLAS in the package) use the stated order; Givens is the plain formula
// above, without LAPACK's scaling (it overflows where f*f does); the DGKS loop is capped at 3 correction passes (no cap in the
// package); x is also formed when maxiter ends a cycle part-way (the package forms x at a restart or on convergence only and
// would return an x that does not belong to the residual it reports); Pl = NULL is Identity with no copies.
// tests/gmres_model.c restates all of this as plain loops and is normative for the order of every operation: x, the whole
// history, the counters and the flag are bit-identical to it.
//
// Kernels of iteration k (w = V[k+1]):
//   pmul            w = Pl \ (A*V[k]) (krylov.hpp, PreconProduct::pmul: the branches esp_bicgstabl takes): Identity / Jacobi / ILU0 end
//                   in a row_dot_k that (MGS) also emits level 0 of dot(V[1], w); ILUAM / AMG / the permuted Block end in dot_k
//   MGS    fold_k, then k times  mgs_step_k + fold_k:  every workgroup finishes H[i,k] from the level-1 partials (workgroup 0
//          stores it), w = w - H[i,k]*V[i] and level 0 of the NEXT dot -- dot(V[i+1], w), or dot(w, w) after the last column -- in
//          the same pass: three streams read, one written, double2 accesses; the dots alternate between two level-1 places.
//          2k + constant launches.
//   CGS / DGKS   bdot_k (w[e] in a register, level 0 of all k dots, the columns in groups of 8 trees), gm_fold_batch_k, coef_k (ONE
//          workgroup: h or c, proj, h += c to the scalar block), comb_k (the ordered combination, level 0 of dot(w, w)), fold;
//          DGKS then enqueues pred_k (ONE workgroup: nrm, the predicate nrm < eta*proj AND every earlier one, to the scalar block)
//          and the same five kernels three times, unconditionally: each reads the device predicate and returns at once when it is
//          false -- no read-back for the decision, a launch count that does not depend on k.
//   norm_k          nrm finished per workgroup, w = w * (1.0/nrm); workgroup 0: H[k+1,k], the nullvec / acc / current recurrence
//   one read-back of 16 bytes (current, the pass counter) through pin_scalar: the ONE host round trip of an iteration
// and at the end of a cycle lsq_k (one thread: Givens and the back substitution over the scalar block, m <= 64), comb_k on x, and
// the init sequence again.  A value crosses workgroups only at a kernel boundary: no flags between workgroups, no grid barrier.
// The statements of every kernel are gmres.hpp's bodies, which esp_gmres_many (gmres_many.hip) runs per column as well.
#include "gmres.hpp"

namespace {

__global__ __launch_bounds__(KT) void gm_scalars_k(double *__restrict__ sc) { gm_scalars(sc); }

// krylov.hpp's fold_batch behind the DGKS predicate
__global__ __launch_bounds__(KT) void gm_fold_batch_k(const double *__restrict__ p0, i64 nb0, double *__restrict__ p1, i64 nb1,
                                                      const double *__restrict__ flag) {
    __shared__ double sred[KT];
    if (flag && flag[0] == 0.0) return;
    fold_batch(p0, nb0, p1, nb1, sred);
}

__global__ __launch_bounds__(KT) void gm_start_k(const double *__restrict__ p1, i64 nb1, double *__restrict__ v, i64 n,
                                                 double *__restrict__ sc, int first) {
    __shared__ double sred[KT];
    gm_start(p1, nb1, v, n, sc, first, sred);
}

__global__ __launch_bounds__(KT) void mgs_step_k(const double *__restrict__ p1, i64 nb1, const double *__restrict__ vi,
                                                 double *__restrict__ w, const double *__restrict__ vnext, i64 n, i64 nb0,
                                                 double *__restrict__ p0, double *__restrict__ hout) {
    __shared__ __align__(16) double sred[2][KT];
    gm_mgs_step(p1, nb1, vi, w, vnext, n, nb0, p0, hout, sred);
}

__global__ __launch_bounds__(KT) void bdot_k(const double *__restrict__ V, i64 ns, int k, const double *__restrict__ w, i64 n,
                                             i64 nb0, double *__restrict__ p0, const double *__restrict__ flag) {
    __shared__ double sred[GM_GROUP][KT];
    if (flag && flag[0] == 0.0) return;
    gm_bdot(V, ns, k, w, n, nb0, p0, sred);
}

__global__ __launch_bounds__(KT) void coef_k(const double *__restrict__ p1, i64 nb1, int k, double *__restrict__ sc, int pass) {
    __shared__ double sred[KT];
    gm_coef(p1, nb1, k, sc, pass, sred);
}

template <bool SUB>
__global__ __launch_bounds__(KT) void comb_k(const double *__restrict__ V, i64 ns, int m, const double *__restrict__ coef,
                                             double *__restrict__ a, i64 n, i64 nb0, double *__restrict__ p0,
                                             const double *__restrict__ flag) {
    __shared__ double sred[KT];
    __shared__ double sco[GM_MAX];
    if (flag && flag[0] == 0.0) return;
    gm_comb<SUB>(V, ns, m, coef, a, n, nb0, p0, sred, sco);
}

__global__ __launch_bounds__(KT) void pred_k(const double *__restrict__ p1, i64 nb1, double *__restrict__ sc, double eta, int first) {
    __shared__ double sred[KT];
    gm_pred(p1, nb1, sc, eta, first, sred);
}

__global__ __launch_bounds__(KT) void norm_k(const double *__restrict__ p1, i64 nb1, double *__restrict__ w, i64 n, double *sc, int k,
                                             const double *hsrc) {
    __shared__ double sred[KT];
    gm_norm(p1, nb1, w, n, sc, k, hsrc, sred);
}

__global__ void lsq_k(double *__restrict__ sc, int m) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    gm_lsq(sc, m);
}

}  // namespace

extern "C" int32_t esp_gmres(esp_handle *h, esp_precon *p, const double *b, double *x, int32_t on_device, int32_t initially_zero,
                             int32_t restart, int32_t orth_meth, int64_t maxiter, double abstol, double reltol, double *history,
                             int64_t *iterations, int64_t *mv_products, int64_t *reorth_passes, int32_t *converged) {
    if (!h || !b || !x || maxiter < 0 || restart < 1 || restart > GM_MAX || orth_meth < ESP_ORTH_MGS || orth_meth > ESP_ORTH_DGKS)
        return ESP_ERR_INVALID;
    if (p && p->h != h) FAIL(h, ESP_ERR_INVALID, "esp_gmres: the preconditioner belongs to another matrix");
    CK(solver_ready(h, p, "esp_gmres"));
    CK(csr_current(h));
    const i64 n = h->n;
    if (n == 0) {
        if (history) history[0] = 0.0;
        if (iterations) *iterations = 0;
        if (mv_products) *mv_products = 0;
        if (reorth_passes) *reorth_passes = 0;
        if (converged) *converged = 1;
        return ESP_OK;
    }
    const i64 nb0 = ceil_div<i64>(n, KT), nb1 = ceil_div<i64>(nb0, KT);
    const i64 ns = std::max<i64>((n + 31) & ~(i64)31, 32);  // a vector's stride in the block: 256-byte aligned
    const size_t vbytes = sizeof(double) * (size_t)n;
    esp_handle::Krylov &w = h->kry;
    CK(ensure(h, w.bv, sizeof(double) * (size_t)ns * (size_t)(restart + 1)));
    if (p) CK(ensure(h, w.t, vbytes));  // A*v in front of ILU0 / ILUAM / AMG / the permuted Block, the unpreconditioned residual
    CK(ensure(h, w.part, sizeof(double) * (size_t)(restart * nb0 + (2 + restart) * nb1 + 8)));
    CK(ensure(h, w.sc, sizeof(double) * SC_COUNT));
    const double *db;
    double *dx;
    CK(stage_vectors(h, n, on_device != 0, b, x, &db, &dx));
    double *V = (double *)w.bv.p, *t = (double *)w.t.p, *sc = (double *)w.sc.p;
    // the partial sums: level 0 of up to `restart` dots | level 1: two places the single dots alternate between (mgs_step_k reads
    // one while the next is formed), the batch of the CGS / DGKS passes
    double *p0 = (double *)w.part.p, *p1 = p0 + (i64)restart * nb0;
    double *slot[2] = {p1, p1 + nb1}, *p1_batch = p1 + 2 * nb1;
    const unsigned g0 = (unsigned)nb0, g1 = (unsigned)nb1;
    const unsigned gv = (unsigned)std::min<i64>(nb0, KGRID), gv2 = (unsigned)std::min<i64>((nb0 + 1) >> 1, KGRID);
    const double *const nil = nullptr;
    double *const nilw = nullptr;
    hipStream_t st = h->stream;
    auto fold = [&](double *dst) { hipLaunchKernelGGL(fold_k, dim3(g1), dim3(KT), 0, st, (const double *)p0, nb0, dst); };
    // every A*v, Pl \ v and Pl \ (A*v) below, level 0 of dot(dst, V[0]) when a dot product is wanted
    const PreconProduct pp{h, fused_precon(p), block_permuted(p) ? p : nullptr, n, nb0, g0, gv, p0, t};
    // V[0] = Pl \ b or Pl \ (b - A*x), normalised; beta, acc = 1 (first: current = beta) to the scalar block
    auto init = [&](bool zero, bool first) -> int32_t {
        double *r0 = p ? t : V;                // the unpreconditioned residual
        if (!zero) pp.mul(dx, V + ns, V, false);  // A*x in V[1], which is free here
        hipLaunchKernelGGL(start_k, dim3(gv), dim3(KT), 0, st, db, zero ? nil : (const double *)(V + ns), r0, n, nb0, p0);
        if (p) {
            CK(pp.ldiv(r0, V, V, false));  // V[0] = Pl \ r0
            hipLaunchKernelGGL(dot_k, dim3(gv), dim3(KT), 0, st, nil, (const double *)V, (const double *)V, nilw, n, nb0, p0);
        }
        fold(slot[0]);
        hipLaunchKernelGGL(gm_start_k, dim3(gv), dim3(KT), 0, st, (const double *)slot[0], nb1, V, n, sc, first ? 1 : 0);
        return ESP_OK;
    };
    // current and the pass counter: the one read-back of an iteration
    double current = 0.0;
    int64_t passes = 0;
    auto read_back = [&]() -> int32_t {
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, sc + SC_OUT, 16, hipMemcpyDeviceToHost, st));
        HIPCK(h, hipStreamSynchronize(st));
        current = ((const double *)h->pin_scalar)[0];
        passes = (int64_t)((const double *)h->pin_scalar)[1];
        return ESP_OK;
    };
    // one CGS pass (pass 0) or DGKS correction pass (1..3, behind the device predicate) of column k: coefficients, combination,
    // level 1 of dot(w, w) in slot[0]
    const double eta = 1.0 / sqrt(2.0);
    auto cgs_pass = [&](double *wv, int k, int pass) {
        const double *flag = pass > 0 ? sc + SC_FLAG : nil;
        hipLaunchKernelGGL(bdot_k, dim3(gv), dim3(KT), 0, st, (const double *)V, ns, k, (const double *)wv, n, nb0, p0, flag);
        hipLaunchKernelGGL(gm_fold_batch_k, dim3(g1, k), dim3(KT), 0, st, (const double *)p0, nb0, p1_batch, nb1, flag);
        hipLaunchKernelGGL(coef_k, dim3(1), dim3(KT), 0, st, (const double *)p1_batch, nb1, k, sc, pass);
        hipLaunchKernelGGL((comb_k<true>), dim3(gv), dim3(KT), 0, st, (const double *)V, ns, k,
                           (const double *)(sc + (pass > 0 ? SC_CV : SC_HV)), wv, n, nb0, p0, flag);
        hipLaunchKernelGGL(gm_fold_batch_k, dim3(g1, 1), dim3(KT), 0, st, (const double *)p0, nb0, slot[0], nb1, flag);
    };

    int64_t mv = initially_zero ? 0 : 1, it = 0;
    hipLaunchKernelGGL(gm_scalars_k, dim3(1), dim3(KT), 0, st, sc);
    CK(init(initially_zero != 0, true));
    CK(read_back());
    if (history) history[0] = current;
    const double tol = std::max(reltol * current, abstol);
    int k = 1;
    while (it < maxiter && !(current <= tol)) {
        double *wv = V + (i64)k * ns;
        CK(pp.pmul(V + (i64)(k - 1) * ns, wv, V, orth_meth == ESP_ORTH_MGS));
        mv++;
        const double *nrm_p1, *hsrc;
        if (orth_meth == ESP_ORTH_MGS) {
            fold(slot[0]);
            for (int i = 0; i < k; i++) {
                hipLaunchKernelGGL(mgs_step_k, dim3(gv2), dim3(KT), 0, st, (const double *)slot[i & 1], nb1, (const double *)(V + (i64)i * ns),
                                   wv, i + 1 < k ? (const double *)(V + (i64)(i + 1) * ns) : nil, n, nb0, p0,
                                   sc + SC_H + (k - 1) * GM_LD + i);
                fold(slot[(i + 1) & 1]);
            }
            nrm_p1 = slot[k & 1];
            hsrc = sc + SC_H + (k - 1) * GM_LD;
        } else {
            cgs_pass(wv, k, 0);
            if (orth_meth == ESP_ORTH_DGKS)
                for (int pass = 1; pass <= 3; pass++) {
                    hipLaunchKernelGGL(pred_k, dim3(1), dim3(KT), 0, st, (const double *)slot[0], nb1, sc, eta, pass == 1 ? 1 : 0);
                    cgs_pass(wv, k, pass);
                }
            nrm_p1 = slot[0];
            hsrc = sc + SC_HV;
        }
        hipLaunchKernelGGL(norm_k, dim3(gv), dim3(KT), 0, st, nrm_p1, nb1, wv, n, sc, k, hsrc);
        k++;
        it++;
        CK(read_back());
        if (history) history[it] = current;
        if (k == restart + 1 || current <= tol || it == maxiter) {
            const int m = k - 1;
            hipLaunchKernelGGL(lsq_k, dim3(1), dim3(64), 0, st, sc, m);
            hipLaunchKernelGGL((comb_k<false>), dim3(gv), dim3(KT), 0, st, (const double *)V, ns, m, (const double *)(sc + SC_RHS), dx, n,
                               nb0, nilw, nil);
            k = 1;
            if (!(current <= tol) && it < maxiter) {
                CK(init(false, false));
                mv++;
            }
        }
    }
    if (iterations) *iterations = it;
    if (mv_products) *mv_products = mv;
    if (reorth_passes) *reorth_passes = passes;
    if (converged) *converged = current <= tol ? 1 : 0;
    HIPCK(h, hipGetLastError());
    return return_x(h, n, on_device != 0, x, dx);
}
