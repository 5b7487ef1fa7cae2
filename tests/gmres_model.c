/* gmres_model.c -- independent model of restarted GMRES as include/esparse_hip.h states it for esp_gmres (test infrastructure;
 * normative for the order of every operation).
 *
 * The statements are IterativeSolvers.jl's gmres! with a left preconditioner (restated from its documented behaviour; the
 * package is not part of the reference tree), as literal loops over whole vectors.  The loop exists once: the operator and the
 * preconditioner are reached through two function pointers.  model_gmres passes the C loops of cg_model.c (included below
 * unchanged: mul!, the four ldiv!s, the ordered dot product); model_gmres_cb takes them from the caller.
 * Built by the tests with gcc -O1 -ffp-contract=off: every product, sum, quotient and square root rounded on its own.
 */
#include <string.h>

#include "cg_model.c"

#define GM_RESTART_MAX 64
#define GM_ORTH_MGS 0
#define GM_ORTH_CGS 1
#define GM_ORTH_DGKS 2
#define GM_DGKS_CAP 3

typedef void (*gm_apply)(void *ctx, const double *v, double *out); /* out = A*v  /  out = Pl \ v  (v != out) */

/* what the loop hands out for inspection (every member may be NULL) */
typedef struct {
    double *H;          /* the Hessenberg matrix of the LAST finished cycle BEFORE its rotations, column-major, leading
                           dimension restart+1 */
    double *V;          /* that cycle's basis, n x (restart+1), column-major */
    int64_t *cycle_m;   /* its number of columns */
    double *restart_x;  /* x after every cycle, one n-vector each (as many as cycles_cap) */
    int64_t *restart_it;/* the iteration count at which each was formed */
    int64_t cycles_cap;
    int64_t *cycles;    /* cycles finished */
} gm_probe;

/* V1 = Pl \ (b - A*x) (or Pl \ b), normalised; returns beta */
static double gm_init(int64_t n, gm_apply mul, void *mctx, gm_apply ldiv, void *lctx, const double *b, const double *x,
                      int32_t initially_zero, double *t, double *u, double *v1, int64_t *mv) {
    if (initially_zero) {
        for (int64_t i = 0; i < n; i++) t[i] = b[i];
    } else {
        mul(mctx, x, u);
        for (int64_t i = 0; i < n; i++) t[i] = b[i] - u[i];
        *mv += 1;
    }
    ldiv(lctx, t, v1);
    const double beta = cg_norm(n, v1);
    const double inv = 1.0 / beta;
    for (int64_t i = 0; i < n; i++) v1[i] = v1[i] * inv;
    return beta;
}

/* w = w - c[0]*V[0] - ... - c[k-1]*V[k-1], element by element in increasing column */
static void gm_subtract(int64_t n, int k, double *const *V, const double *c, double *w) {
    for (int64_t e = 0; e < n; e++) {
        double a = w[e];
        for (int j = 0; j < k; j++) a = a - c[j] * V[j][e];
        w[e] = a;
    }
}

/* orthogonalise w against V[0..k-1]: the coefficients to h[0..k-1], returns norm(w) after it */
static double gm_orthogonalise(int32_t orth, int64_t n, int k, double *const *V, double *w, double *h, int64_t *passes) {
    if (orth == GM_ORTH_MGS) {
        for (int i = 0; i < k; i++) {
            h[i] = model_cg_dot(n, V[i], w);
            for (int64_t e = 0; e < n; e++) w[e] = w[e] - h[i] * V[i][e];
        }
        return cg_norm(n, w);
    }
    for (int j = 0; j < k; j++) h[j] = model_cg_dot(n, V[j], w);
    gm_subtract(n, k, V, h, w);
    double nrm = cg_norm(n, w);
    if (orth == GM_ORTH_CGS) return nrm;
    double s = 0.0, c[GM_RESTART_MAX];
    for (int j = 0; j < k; j++) s = s + h[j] * h[j];
    double proj = sqrt(s);
    const double eta = 1.0 / sqrt(2.0);
    int pass = 0;
    while (nrm < eta * proj && pass < GM_DGKS_CAP) {
        for (int j = 0; j < k; j++) c[j] = model_cg_dot(n, V[j], w);
        s = 0.0;
        for (int j = 0; j < k; j++) s = s + c[j] * c[j];
        proj = sqrt(s);
        gm_subtract(n, k, V, c, w);
        for (int j = 0; j < k; j++) h[j] = h[j] + c[j];
        nrm = cg_norm(n, w);
        pass++;
        *passes += 1;
    }
    return nrm;
}

/* the least-squares problem of a cycle of m columns: Givens rotations column by column over H (leading dimension ld) and
 * rhs = (beta, 0, .., 0), then the back substitution; the solution in rhs[0..m-1] */
void model_gmres_lsq(int m, int ld, double *H, double beta, double *rhs) {
    rhs[0] = beta;
    for (int i = 1; i <= m; i++) rhs[i] = 0.0;
    for (int i = 0; i < m; i++) {
        const double f = H[i + i * ld], g = H[i + 1 + i * ld];
        double c = 1.0, s = 0.0;
        if (!(g == 0.0)) {
            const double r = sqrt(f * f + g * g);
            c = f / r;
            s = g / r;
        }
        H[i + i * ld] = c * f + s * g;
        for (int j = i + 1; j < m; j++) {
            const double t = -s * H[i + j * ld] + c * H[i + 1 + j * ld];
            H[i + j * ld] = c * H[i + j * ld] + s * H[i + 1 + j * ld];
            H[i + 1 + j * ld] = t;
        }
        const double t = -s * rhs[i] + c * rhs[i + 1];
        rhs[i] = c * rhs[i] + s * rhs[i + 1];
        rhs[i + 1] = t;
    }
    for (int i = m - 1; i >= 0; i--) {
        double z = rhs[i];
        for (int j = i + 1; j < m; j++) z = z - H[i + j * ld] * rhs[j];
        rhs[i] = z / H[i + i * ld];
    }
}

/* THE loop.  history: maxiter+1 doubles or NULL; returns the iterations run, -1 for arguments esp_gmres refuses */
static int64_t gm_loop(int64_t n, gm_apply mul, void *mctx, gm_apply ldiv, void *lctx, const double *b, double *x,
                       int32_t initially_zero, int32_t restart, int32_t orth, int64_t maxiter, double abstol, double reltol,
                       double *history, int64_t *mv_products, int64_t *reorth_passes, int32_t *converged, const gm_probe *probe) {
    if (restart < 1 || restart > GM_RESTART_MAX || orth < 0 || orth > GM_ORTH_DGKS || maxiter < 0) return -1;
    int64_t mv = 0, passes = 0, it = 0, cycles = 0;
    if (n == 0) {
        if (history) history[0] = 0.0;
        if (mv_products) *mv_products = 0;
        if (reorth_passes) *reorth_passes = 0;
        if (converged) *converged = 1;
        if (probe && probe->cycles) *probe->cycles = 0;
        return 0;
    }
    const int ld = restart + 1;
    const size_t bytes = sizeof(double) * (size_t)n;
    double *V[GM_RESTART_MAX + 1];
    for (int j = 0; j <= restart; j++) V[j] = (double *)malloc(bytes);
    double *t = (double *)malloc(bytes), *u = (double *)malloc(bytes);
    double *H = (double *)calloc((size_t)ld * (size_t)restart, sizeof(double));
    double nullvec[GM_RESTART_MAX + 1], rhs[GM_RESTART_MAX + 1], h[GM_RESTART_MAX];
    for (int j = 0; j <= restart; j++) nullvec[j] = 1.0;
    double beta = gm_init(n, mul, mctx, ldiv, lctx, b, x, initially_zero, t, u, V[0], &mv);
    double acc = 1.0, current = beta;
    const double tr = reltol * current, tol = tr > abstol ? tr : abstol;
    int k = 1; /* the column being formed, 1-based as in the statement: V[k] (0-based) is the new vector */
    if (history) history[0] = current;
    while (it < maxiter && !(current <= tol)) {
        mul(mctx, V[k - 1], t);
        ldiv(lctx, t, V[k]);
        mv += 1;
        double *w = V[k];
        const double nrm = gm_orthogonalise(orth, n, k, V, w, h, &passes);
        for (int i = 0; i < k; i++) H[i + (k - 1) * ld] = h[i];
        const double inv = 1.0 / nrm;
        for (int64_t e = 0; e < n; e++) w[e] = w[e] * inv;
        H[k + (k - 1) * ld] = nrm;
        double s = 0.0;
        for (int i = 0; i < k; i++) s = s + nullvec[i] * H[i + (k - 1) * ld];
        nullvec[k] = -(s / H[k + (k - 1) * ld]);
        acc = acc + nullvec[k] * nullvec[k];
        current = beta / sqrt(acc);
        k += 1;
        it += 1;
        if (history) history[it] = current;
        if (k == restart + 1 || current <= tol || it == maxiter) {
            const int m = k - 1;
            if (probe) {
                if (probe->H) memcpy(probe->H, H, sizeof(double) * (size_t)ld * (size_t)restart);
                if (probe->V)
                    for (int j = 0; j <= m; j++) memcpy(probe->V + (size_t)j * (size_t)n, V[j], bytes);
                if (probe->cycle_m) *probe->cycle_m = m;
            }
            model_gmres_lsq(m, ld, H, beta, rhs);
            for (int64_t e = 0; e < n; e++) {
                double a = x[e];
                for (int j = 0; j < m; j++) a = a + rhs[j] * V[j][e];
                x[e] = a;
            }
            if (probe && cycles < probe->cycles_cap) {
                if (probe->restart_x) memcpy(probe->restart_x + (size_t)cycles * (size_t)n, x, bytes);
                if (probe->restart_it) probe->restart_it[cycles] = it;
            }
            cycles++;
            k = 1;
            if (!(current <= tol) && it < maxiter) {
                beta = gm_init(n, mul, mctx, ldiv, lctx, b, x, 0, t, u, V[0], &mv);
                acc = 1.0; /* current is NOT reset */
            }
        }
    }
    if (mv_products) *mv_products = mv;
    if (reorth_passes) *reorth_passes = passes;
    if (converged) *converged = current <= tol ? 1 : 0;
    if (probe && probe->cycles) *probe->cycles = cycles;
    for (int j = 0; j <= restart; j++) free(V[j]);
    free(t);
    free(u);
    free(H);
    return it;
}

/* the operator and the four preconditioners of cg_model.c behind the two function pointers */
typedef struct {
    int32_t kind;
    int64_t n;
    const int64_t *colptr, *rowval, *idiag;
    const double *nzval, *diag, *fval;
} gm_csc;

static void gm_csc_mul(void *ctx, const double *v, double *out) {
    const gm_csc *c = (const gm_csc *)ctx;
    model_mul(c->n, c->colptr, c->rowval, c->nzval, v, out);
}
static void gm_csc_ldiv(void *ctx, const double *v, double *out) {
    const gm_csc *c = (const gm_csc *)ctx;
    cg_ldiv(c->kind, c->n, c->colptr, c->rowval, c->nzval, c->diag, c->idiag, c->fval, v, out);
}

int64_t model_gmres(int32_t kind, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, const double *diag,
                    const int64_t *idiag, const double *fval, const double *b, double *x, int32_t initially_zero, int32_t restart,
                    int32_t orth, int64_t maxiter, double abstol, double reltol, double *history, int64_t *mv_products,
                    int64_t *reorth_passes, int32_t *converged, const gm_probe *probe) {
    gm_csc c = {kind, n, colptr, rowval, idiag, nzval, diag, fval};
    return gm_loop(n, gm_csc_mul, &c, gm_csc_ldiv, &c, b, x, initially_zero, restart, orth, maxiter, abstol, reltol, history,
                   mv_products, reorth_passes, converged, probe);
}

/* the same loop over the caller's operator and preconditioner (block_precon_modellib's and amg_modellib's ldiv plug in here) */
int64_t model_gmres_cb(int64_t n, gm_apply mul, gm_apply ldiv, const double *b, double *x, int32_t initially_zero, int32_t restart,
                       int32_t orth, int64_t maxiter, double abstol, double reltol, double *history, int64_t *mv_products,
                       int64_t *reorth_passes, int32_t *converged, const gm_probe *probe) {
    return gm_loop(n, mul, NULL, ldiv, NULL, b, x, initially_zero, restart, orth, maxiter, abstol, reltol, history, mv_products,
                   reorth_passes, converged, probe);
}
