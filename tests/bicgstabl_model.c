/* bicgstabl_model.c -- independent model of BiCGStab(l) as include/esparse_hip.h states it for esp_bicgstabl (test
 * infrastructure; normative for the order of every operation).
 *
 * The statements are IterativeSolvers.jl's bicgstabl! with a left preconditioner (restated from its documented behaviour; the
 * package is not part of the reference tree), as literal loops over whole vectors.  ldiv!, mul! and the ordered dot product
 * (model_cg_dot) are those of cg_model.c, included below unchanged.  The minimal-residual system is solved by an LU
 * factorization without pivoting, written out.
 * Built by the tests with gcc -O1 -ffp-contract=off: every product, sum and quotient rounded on its own.
 */
#include "cg_model.c"

#define BL_MAX 4

/* w = Pl \ (A*v); t: n doubles of scratch */
static void bl_pmul(int32_t kind, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *diag,
                    const int64_t *idiag, const double *fval, const double *v, double *t, double *w) {
    model_mul(n, colptr, rowval, nzval, v, t);
    cg_ldiv(kind, n, colptr, rowval, nzval, diag, idiag, fval, t, w);
}

/* gamma[1..l] = M[1..l,1..l] \ M[1..l,0]: LU without pivoting, forward substitution with the unit lower factor, back
 * substitution with a true division, the inner index increasing */
void model_bicgstabl_gamma(int32_t l, const double M[BL_MAX + 1][BL_MAX + 1], double *gamma /* [l + 1], gamma[0] unused */) {
    double G[BL_MAX][BL_MAX], y[BL_MAX], z[BL_MAX];
    for (int i = 0; i < l; i++)
        for (int j = 0; j < l; j++) G[i][j] = M[i + 1][j + 1];
    for (int k = 0; k < l; k++) {
        const double inv = 1.0 / G[k][k];
        for (int i = k + 1; i < l; i++) G[i][k] = G[i][k] * inv;
        for (int j = k + 1; j < l; j++)
            for (int i = k + 1; i < l; i++) G[i][j] = G[i][j] - G[i][k] * G[k][j];
    }
    for (int i = 0; i < l; i++) {
        y[i] = M[i + 1][0];
        for (int j = 0; j < i; j++) y[i] = y[i] - G[i][j] * y[j];
    }
    for (int i = l - 1; i >= 0; i--) {
        double s = y[i];
        for (int j = i + 1; j < l; j++) s = s - G[i][j] * z[j];
        z[i] = s / G[i][i];
    }
    gamma[0] = 0.0;
    for (int i = 0; i < l; i++) gamma[i + 1] = z[i];
}

/* history: ceil(max_mv_products / (2 l)) + 1 doubles or NULL; returns the outer iterations run, -1 for an unsupported l */
int64_t model_bicgstabl(int32_t kind, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *diag,
                        const int64_t *idiag, const double *fval, int32_t l, const double *b, double *x, const double *r_shadow,
                        int32_t initially_zero, int64_t max_mv_products, double abstol, double reltol, double *history,
                        int64_t *mv_products, int32_t *converged) {
    if (l < 1 || l > BL_MAX) return -1;
    const size_t bytes = sizeof(double) * (size_t)(n > 0 ? n : 1);
    double *rs[BL_MAX + 1], *us[BL_MAX + 1], *rt = (double *)malloc(bytes), *t = (double *)malloc(bytes);
    for (int k = 0; k <= l; k++) {
        rs[k] = (double *)malloc(bytes);
        us[k] = (double *)malloc(bytes);
        for (int64_t i = 0; i < n; i++) us[k][i] = 0.0;                       /* us = 0 */
    }
    int64_t mv = 0;
    if (initially_zero) {
        for (int64_t i = 0; i < n; i++) t[i] = b[i];                          /* rs[0] = b */
    } else {
        model_mul(n, colptr, rowval, nzval, x, rs[0]);                        /* rs[0] = b - A*x */
        for (int64_t i = 0; i < n; i++) t[i] = b[i] - rs[0][i];
        mv = 1;
    }
    cg_ldiv(kind, n, colptr, rowval, nzval, diag, idiag, fval, t, rs[0]);     /* rs[0] = Pl \ rs[0] */
    double omega = 1.0, sigma = 1.0;
    for (int64_t i = 0; i < n; i++) rt[i] = r_shadow ? r_shadow[i] : rs[0][i];
    double residual = cg_norm(n, rs[0]);
    const double tr = reltol * residual, tol = tr > abstol ? tr : abstol;
    if (history) history[0] = residual;
    int64_t it = 0;
    while (mv < max_mv_products && !(residual <= tol)) {
        it++;
        sigma = -omega * sigma;
        for (int j = 0; j < l; j++) {                                         /* the BiCG part */
            const double rho = model_cg_dot(n, rt, rs[j]);
            const double beta = rho / sigma;
            for (int k = 0; k <= j; k++)
                for (int64_t i = 0; i < n; i++) us[k][i] = rs[k][i] - beta * us[k][i];
            bl_pmul(kind, n, colptr, rowval, nzval, diag, idiag, fval, us[j], t, us[j + 1]);
            sigma = model_cg_dot(n, rt, us[j + 1]);
            const double alpha = rho / sigma;
            for (int k = 0; k <= j; k++)
                for (int64_t i = 0; i < n; i++) rs[k][i] = rs[k][i] - alpha * us[k + 1][i];
            bl_pmul(kind, n, colptr, rowval, nzval, diag, idiag, fval, rs[j], t, rs[j + 1]);
            for (int64_t i = 0; i < n; i++) x[i] = x[i] + alpha * us[0][i];
        }
        mv += 2 * (int64_t)l;
        double M[BL_MAX + 1][BL_MAX + 1], gamma[BL_MAX + 1];                  /* the minimal-residual part */
        for (int i = 0; i <= l; i++)
            for (int k = i; k <= l; k++) M[i][k] = M[k][i] = model_cg_dot(n, rs[i], rs[k]);
        model_bicgstabl_gamma(l, M, gamma);
        for (int k = 1; k <= l; k++)
            for (int64_t i = 0; i < n; i++) us[0][i] = us[0][i] - gamma[k] * us[k][i];
        for (int k = 1; k <= l; k++)
            for (int64_t i = 0; i < n; i++) x[i] = x[i] + gamma[k] * rs[k - 1][i];
        for (int k = 1; k <= l; k++)
            for (int64_t i = 0; i < n; i++) rs[0][i] = rs[0][i] - gamma[k] * rs[k][i];
        omega = gamma[l];
        residual = cg_norm(n, rs[0]);
        if (history) history[it] = residual;
    }
    if (mv_products) *mv_products = mv;
    if (converged) *converged = residual <= tol ? 1 : 0;
    for (int k = 0; k <= l; k++) {
        free(rs[k]);
        free(us[k]);
    }
    free(rt);
    free(t);
    return it;
}
