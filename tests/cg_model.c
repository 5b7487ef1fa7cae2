/* cg_model.c -- independent model of preconditioned conjugate gradients as include/esparse_hip.h states it for esp_cg (test
 * infrastructure).
 *
 * The statements are IterativeSolvers.jl's cg! with a left preconditioner (restated from its documented behaviour; the
 * package is not part of the reference tree), as literal loops over whole vectors.  ldiv! and mul! are the literal column
 * loops of precon_model.c and iluam_model.c, included below unchanged.  dot and norm are the fixed summation shape of the
 * device, restated here on its own: chunks of 256 products folded by a pairwise tree, the same tree over groups of 256 chunk
 * sums, then 256 strided sums and the tree once more.
 * Built by the tests with gcc -O1 -ffp-contract=off: every product and sum rounded on its own.
 */
#include "precon_model.c"
#include "iluam_model.c"

#define KIND_IDENTITY (-1)
#define KIND_ILUAM 2

/* for w = 128, 64, ..., 1: s[t] = s[t] + s[t + w] for t < w; the sum is s[0] */
static double tree256(double *s) {
    for (int w = 128; w >= 1; w /= 2)
        for (int t = 0; t < w; t++) s[t] = s[t] + s[t + w];
    return s[0];
}

/* one level: out[g] = tree of in[256 g .. 256 g + 255], padded with +0.0; returns the number of sums written */
static int64_t fold_level(int64_t cnt, const double *in, double *out) {
    const int64_t groups = (cnt + 255) / 256;
    for (int64_t g = 0; g < groups; g++) {
        double s[256];
        for (int t = 0; t < 256; t++) s[t] = 256 * g + t < cnt ? in[256 * g + t] : 0.0;
        out[g] = tree256(s);
    }
    return groups;
}

double model_cg_dot(int64_t n, const double *a, const double *b) {
    const int64_t nb0 = (n + 255) / 256, nb1 = (nb0 + 255) / 256;
    double *prod = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    double *p0 = (double *)malloc(sizeof(double) * (size_t)(nb0 > 0 ? nb0 : 1));
    double *p1 = (double *)malloc(sizeof(double) * (size_t)(nb1 > 0 ? nb1 : 1));
    for (int64_t i = 0; i < n; i++) prod[i] = a[i] * b[i];
    fold_level(n, prod, p0);   /* level 0 */
    fold_level(nb0, p0, p1);   /* level 1 */
    double s[256];             /* level 2 */
    for (int t = 0; t < 256; t++) {
        s[t] = 0.0;
        for (int64_t q = t; q < nb1; q += 256) s[t] = s[t] + p1[q];
    }
    const double r = tree256(s);
    free(prod);
    free(p0);
    free(p1);
    return r;
}

static double cg_norm(int64_t n, const double *r) { return sqrt(model_cg_dot(n, r, r)); }

/* c = Pl \ r.  diag: invdiag (Jacobi) / xdiag (ILU0); idiag: ILU0's idiag / ILUAM's diag (1-based positions); fval: ILUAM's
 * factorization */
static void cg_ldiv(int32_t kind, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *diag,
                    const int64_t *idiag, const double *fval, const double *r, double *c) {
    if (kind == KIND_IDENTITY) for (int64_t i = 0; i < n; i++) c[i] = r[i];
    else if (kind == KIND_JACOBI) model_jacobi_ldiv(n, diag, r, c);
    else if (kind == KIND_ILU0) model_ilu0_ldiv(n, colptr, rowval, nzval, diag, idiag, r, c);
    else model_iluam_ldiv(n, colptr, rowval, fval, idiag, r, c);
}

/* history: maxiter+1 doubles or NULL; returns the iterations run */
int64_t model_cg(int32_t kind, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *diag,
                 const int64_t *idiag, const double *fval, const double *b, double *x, int32_t initially_zero, int64_t maxiter,
                 double abstol, double reltol, double *history, int32_t *converged) {
    const size_t bytes = sizeof(double) * (size_t)(n > 0 ? n : 1);
    double *r = (double *)malloc(bytes), *u = (double *)malloc(bytes), *c = (double *)malloc(bytes);
    for (int64_t i = 0; i < n; i++) u[i] = 0.0;                  /* u = 0 */
    double rho = 1.0;                                            /* rho = 1 */
    if (initially_zero) {
        for (int64_t i = 0; i < n; i++) r[i] = b[i];             /* r = b */
    } else {
        model_mul(n, colptr, rowval, nzval, x, c);               /* c = A*x */
        for (int64_t i = 0; i < n; i++) r[i] = b[i] - c[i];      /* r = b - c */
    }
    double residual = cg_norm(n, r);
    const double tr = reltol * residual, tol = tr > abstol ? tr : abstol;
    if (history) history[0] = residual;
    int64_t it = 0;
    while (it < maxiter && !(residual <= tol)) {
        it++;
        cg_ldiv(kind, n, colptr, rowval, nzval, diag, idiag, fval, r, c);   /* c = Pl \ r */
        const double rho_prev = rho;
        rho = model_cg_dot(n, c, r);
        const double beta = rho / rho_prev;
        for (int64_t i = 0; i < n; i++) u[i] = c[i] + beta * u[i];          /* u = c + beta*u */
        model_mul(n, colptr, rowval, nzval, u, c);                          /* c = A*u */
        const double alpha = rho / model_cg_dot(n, u, c);
        for (int64_t i = 0; i < n; i++) x[i] = x[i] + alpha * u[i];         /* x = x + alpha*u */
        for (int64_t i = 0; i < n; i++) r[i] = r[i] - alpha * c[i];         /* r = r - alpha*c */
        residual = cg_norm(n, r);
        if (history) history[it] = residual;
    }
    if (converged) *converged = residual <= tol ? 1 : 0;
    free(r);
    free(u);
    free(c);
    return it;
}
