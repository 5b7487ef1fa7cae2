/* iluam_model.c -- independent model of the reference's ILUAMPreconditioner (test infrastructure).
 *
 * Restates, with Julia's 1-based CSC arrays (colptr, rowval, diag hold 1-based values), the loops of
 * src/experimental/ExtendableSparseMatrixParallel/ilu_Al-Kurdi_Mittal.jl:
 *   - iluAM (lines 68-120) as the LITERAL column loops with the `point` array;
 *   - ldiv! (lines 160-175) as the two LITERAL scatter loops forward_subst_old! / backward_subst_old! (122-157);
 *   - simple! (src/factorizations/simple_iteration.jl:21-45) with that ldiv!; mul! and norm are precon_model.c's
 *     (the two files are built into one library).
 * A second set of entry points runs the same factorization column by column in a CALLER-SUPPLIED order and the two
 * solves as ROW GATHERS in caller-supplied orders -- what the device does level by level; tests/test_iluam_model.py
 * holds them to the literal loops bit for bit.
 * Built by the tests with gcc -O1 -ffp-contract=off: every product, sum and quotient rounded on its own, as in Julia.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

void model_mul(int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *x, double *r);
double model_norm(int64_t n, const double *x);

/* lines 78-87: diag[j] = the position of the stored (j,j); returns 0, or the first column j without one (the reference
 * would read an undefined diag[j] there) */
int64_t model_iluam_diag(int64_t n, const int64_t *colptr, const int64_t *rowval, int64_t *diag) {
    for (int64_t j = 1; j <= n; j++) {
        diag[j - 1] = 0;
        for (int64_t v = colptr[j - 1]; v <= colptr[j] - 1; v++)
            if (rowval[v - 1] == j) {
                diag[j - 1] = v;
                break;
            }
        if (diag[j - 1] == 0) return j;
    }
    return 0;
}

/* lines 93-117, the body of `for j = 1:n` */
static void iluam_column(int64_t j, const int64_t *colptr, const int64_t *rowval, const int64_t *diag, double *nzval, int64_t *point) {
    for (int64_t v = colptr[j - 1]; v <= colptr[j] - 1; v++) point[rowval[v - 1] - 1] = v;
    for (int64_t v = colptr[j - 1]; v <= diag[j - 1] - 1; v++) {
        const int64_t i = rowval[v - 1];
        for (int64_t w = diag[i - 1] + 1; w <= colptr[i] - 1; w++) {
            const int64_t k = point[rowval[w - 1] - 1];
            if (k > 0) nzval[k - 1] = nzval[k - 1] - nzval[v - 1] * nzval[w - 1];
        }
    }
    for (int64_t v = diag[j - 1] + 1; v <= colptr[j] - 1; v++) nzval[v - 1] = nzval[v - 1] / nzval[diag[j - 1] - 1];
    for (int64_t v = colptr[j - 1]; v <= colptr[j] - 1; v++) point[rowval[v - 1] - 1] = 0;
}

/* iluAM(A): nzval (in: a copy of A.nzval, out: the factorization), diag from model_iluam_diag.
 * order == NULL: for j = 1:n; else the columns in the order order[0..n-1] (1-based column numbers) */
void model_iluam_factor(int64_t n, const int64_t *colptr, const int64_t *rowval, const int64_t *diag, double *nzval,
                        const int64_t *order) {
    int64_t *point = (int64_t *)calloc((size_t)(n > 0 ? n : 1), sizeof(int64_t));
    for (int64_t t = 1; t <= n; t++) iluam_column(order ? order[t - 1] : t, colptr, rowval, diag, nzval, point);
    free(point);
}

/* ldiv!(x, ILU, b), lines 160-175: y = copy(b); forward_subst_old!(y, b, ...); backward_subst_old!(x, y, ...); x may be b */
void model_iluam_ldiv(int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const int64_t *diag,
                      const double *b, double *x) {
    double *y = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    /* lines 128-138 */
    for (int64_t i = 0; i < n; i++) y[i] = 0.0;
    for (int64_t j = 1; j <= n; j++) {
        y[j - 1] = y[j - 1] + b[j - 1];
        for (int64_t v = diag[j - 1] + 1; v <= colptr[j] - 1; v++)
            y[rowval[v - 1] - 1] = y[rowval[v - 1] - 1] - nzval[v - 1] * y[j - 1];
    }
    /* lines 148-155 */
    for (int64_t j = n; j >= 1; j--) {
        x[j - 1] = y[j - 1] / nzval[diag[j - 1] - 1];
        for (int64_t i = colptr[j - 1]; i <= diag[j - 1] - 1; i++)
            y[rowval[i - 1] - 1] = y[rowval[i - 1] - 1] - nzval[i - 1] * x[j - 1];
    }
    free(y);
}

/* the same ldiv! as row gathers: the rows of the forward solve in the order fwd[0..n-1], those of the backward solve in
 * the order bwd[0..n-1] (1-based row numbers; every row after the rows it reads).  Row i of the forward solve subtracts
 * its stored j < i in increasing order and adds b[i] last; row i of the backward solve subtracts its stored j > i in
 * decreasing order and divides last. */
void model_iluam_ldiv_rows(int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const int64_t *diag,
                           const double *b, double *x, const int64_t *fwd, const int64_t *bwd) {
    const int64_t nnz = colptr[n] - 1;
    /* row-wise index: the positions of every row, columns ascending */
    int64_t *rptr = (int64_t *)calloc((size_t)(n + 2), sizeof(int64_t));
    int64_t *rpos = (int64_t *)malloc(sizeof(int64_t) * (size_t)(nnz > 0 ? nnz : 1));
    int64_t *rcol = (int64_t *)malloc(sizeof(int64_t) * (size_t)(nnz > 0 ? nnz : 1));
    double *y = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    for (int64_t v = 1; v <= nnz; v++) rptr[rowval[v - 1] + 1]++;
    for (int64_t i = 1; i <= n + 1; i++) rptr[i] += rptr[i - 1];
    for (int64_t j = 1; j <= n; j++)
        for (int64_t v = colptr[j - 1]; v <= colptr[j] - 1; v++) {
            const int64_t q = rptr[rowval[v - 1]]++;
            rpos[q] = v;
            rcol[q] = j;
        }
    /* now rptr[i] = end of row i = start of row i+1 (rows 1-based, rptr[0] = 0 = start of row 1) */
    for (int64_t t = 0; t < n; t++) {
        const int64_t i = fwd[t];
        double acc = 0.0;
        for (int64_t q = rptr[i - 1]; q < rptr[i] && rcol[q] < i; q++) acc = acc - nzval[rpos[q] - 1] * y[rcol[q] - 1];
        y[i - 1] = acc + b[i - 1];
    }
    for (int64_t t = 0; t < n; t++) {
        const int64_t i = bwd[t];
        double acc = y[i - 1];
        for (int64_t q = rptr[i] - 1; q >= rptr[i - 1] && rcol[q] > i; q--) acc = acc - nzval[rpos[q] - 1] * x[rcol[q] - 1];
        x[i - 1] = acc / nzval[diag[i - 1] - 1];
    }
    free(rptr);
    free(rpos);
    free(rcol);
    free(y);
}

/* simple!(u, A, b; abstol, reltol, maxiter, Pl = ILUAM) -- simple_iteration.jl:21-45; fval / diag: the factorization.
 * history: maxiter+1 doubles or NULL; returns the number of ldiv! steps taken */
int64_t model_iluam_simple(int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *fval,
                           const int64_t *diag, const double *b, double *u, int64_t maxiter, double abstol, double reltol,
                           double *history) {
    double *res = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    double *upd = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    model_mul(n, colptr, rowval, nzval, u, res);
    for (int64_t i = 0; i < n; i++) res[i] = res[i] - b[i];
    const double r0 = model_norm(n, res);
    if (history) history[0] = r0;
    int64_t it = 0;
    for (int64_t i = 1; i <= maxiter; i++) {
        model_iluam_ldiv(n, colptr, rowval, fval, diag, res, upd);   /* ldiv!(upd, Pl, res) */
        for (int64_t q = 0; q < n; q++) u[q] = u[q] - upd[q];        /* u .-= upd */
        model_mul(n, colptr, rowval, nzval, u, res);                  /* mul!(res, A, u) */
        for (int64_t q = 0; q < n; q++) res[q] = res[q] - b[q];      /* res .-= b */
        const double r = model_norm(n, res);
        if (history) history[i] = r;
        it = i;
        if ((r / r0) < reltol || r < abstol) break;
    }
    free(res);
    free(upd);
    return it;
}
