/* precon_model.c -- independent model of the reference's point preconditioners and simple! (test infrastructure).
 *
 * Restates, line by line, with Julia's 1-based CSC arrays (colptr, rowval, idiag hold 1-based values):
 *   - ldiv! of _JacobiPreconditioner   (src/factorizations/jacobi.jl:36-41)
 *   - ldiv! of _ILU0Preconditioner     (src/factorizations/ilu0.jl:66-92) as the LITERAL column loops -- not the row
 *     gathers the device runs, so that bitwise equality with the device checks the two-pass argument of precon.hip
 *   - mul!(r, A, x) as SparseArrays' column loop: r .= 0, then r[rowval[k]] += nzval[k]*x[j] column by column
 *   - simple! (src/factorizations/simple_iteration.jl:21-45) statement by statement; norm is a scaled 2-norm in the
 *     style of the reference BLAS dnrm2 (it cannot be restated bit for bit: the device's fixed-order sum agrees to rounding)
 * Built by the tests with gcc -O1 -ffp-contract=off: every product and sum rounded on its own, as in Julia.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define KIND_JACOBI 0
#define KIND_ILU0 1

/* jacobi.jl:36-41: for i = 1:n, u[i] = p.invdiag[i] * v[i] */
void model_jacobi_ldiv(int64_t n, const double *invdiag, const double *v, double *u) {
    for (int64_t i = 0; i < n; i++) u[i] = invdiag[i] * v[i];
}

/* ilu0.jl:66-92 */
void model_ilu0_ldiv(int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *xdiag,
                     const int64_t *idiag, const double *v, double *u) {
    /* for j = 1:n: u[j] = xdiag[j] * v[j] */
    for (int64_t j = 1; j <= n; j++) u[j - 1] = xdiag[j - 1] * v[j - 1];
    /* for j = n:-1:1, k = (idiag[j] + 1):(colptr[j + 1] - 1): i = rowval[k]; u[i] -= xdiag[i] * nzval[k] * u[j] */
    for (int64_t j = n; j >= 1; j--)
        for (int64_t k = idiag[j - 1] + 1; k <= colptr[j] - 1; k++) {
            const int64_t i = rowval[k - 1];
            u[i - 1] = u[i - 1] - xdiag[i - 1] * nzval[k - 1] * u[j - 1];
        }
    /* for j = 1:n, k = colptr[j]:(idiag[j] - 1): the same statement */
    for (int64_t j = 1; j <= n; j++)
        for (int64_t k = colptr[j - 1]; k <= idiag[j - 1] - 1; k++) {
            const int64_t i = rowval[k - 1];
            u[i - 1] = u[i - 1] - xdiag[i - 1] * nzval[k - 1] * u[j - 1];
        }
}

/* mul!(r, A, x) of SparseArrays: r .= 0; for j, k in nzrange(A, j): r[rowval[k]] += nzval[k] * x[j] */
void model_mul(int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *x, double *r) {
    for (int64_t i = 0; i < n; i++) r[i] = 0.0;
    for (int64_t j = 1; j <= n; j++) {
        const double xj = x[j - 1];
        for (int64_t k = colptr[j - 1]; k <= colptr[j] - 1; k++) r[rowval[k - 1] - 1] = r[rowval[k - 1] - 1] + nzval[k - 1] * xj;
    }
}

/* the 2-norm, scaled (reference BLAS dnrm2): no overflow of the sum of squares */
double model_norm(int64_t n, const double *x) {
    double scale = 0.0, ssq = 1.0;
    for (int64_t i = 0; i < n; i++) {
        if (x[i] != 0.0) {
            const double a = fabs(x[i]);
            if (scale < a) {
                ssq = 1.0 + ssq * (scale / a) * (scale / a);
                scale = a;
            } else {
                ssq = ssq + (a / scale) * (a / scale);
            }
        }
    }
    return scale * sqrt(ssq);
}

/* simple!(u, A, b; abstol, reltol, maxiter, Pl) -- simple_iteration.jl:21-45.  diag = invdiag (Jacobi) or xdiag (ILU0);
 * history: maxiter+1 doubles or NULL; returns the number of ldiv! steps taken */
int64_t model_simple(int32_t kind, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *diag,
                     const int64_t *idiag, const double *b, double *u, int64_t maxiter, double abstol, double reltol,
                     double *history) {
    double *res = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    double *upd = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    /* res = A * u - b */
    model_mul(n, colptr, rowval, nzval, u, res);
    for (int64_t i = 0; i < n; i++) res[i] = res[i] - b[i];
    const double r0 = model_norm(n, res);
    if (history) history[0] = r0;
    int64_t it = 0;
    for (int64_t i = 1; i <= maxiter; i++) {
        if (kind == KIND_JACOBI) model_jacobi_ldiv(n, diag, res, upd); /* ldiv!(upd, Pl, res) */
        else model_ilu0_ldiv(n, colptr, rowval, nzval, diag, idiag, res, upd);
        for (int64_t q = 0; q < n; q++) u[q] = u[q] - upd[q];          /* u .-= upd */
        model_mul(n, colptr, rowval, nzval, u, res);                    /* mul!(res, A, u) */
        for (int64_t q = 0; q < n; q++) res[q] = res[q] - b[q];        /* res .-= b */
        const double r = model_norm(n, res);                            /* r = norm(res) */
        if (history) history[i] = r;                                    /* push!(history, r) */
        it = i;
        if ((r / r0) < reltol || r < abstol) break;
    }
    free(res);
    free(upd);
    return it;
}
