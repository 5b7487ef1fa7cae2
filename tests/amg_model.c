/* amg_model.c -- the smoothed-aggregation AMG preconditioner of include/esparse_hip.h (esp_precon_amg_create), restated as plain
 * loops (test infrastructure).  NORMATIVE for the order of every operation: the strength test, the Luby rounds of the MIS(2)
 * aggregation and the two joining passes, the Gauss-Jordan inverse of the coarsest level, the weighted-Jacobi sweeps and the
 * V-cycle.  The algebra that builds the hierarchy between these pieces (Diagonal scaling, A*B, A+B, transpose, opnorm) is
 * SparseArrays' and has models of its own (matops_model.c, linalg_model.c): tests/amg_modellib.py composes them.
 * Build: gcc -O1 -ffp-contract=off (every product, sum, difference and division rounded on its own).  CSC arrays in Julia layout
 * (colptr and rowval 1-based, rows ascending in every column).  Nothing here knows of the device code. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* position of (row i, column j), both 0-based, or -1 */
static int64_t find(const int64_t *cp, const int64_t *rv, int64_t i, int64_t j) {
    for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++)
        if (rv[k] - 1 == i) return k;
    return -1;
}

/* the checks of level 0: *nodiag = smallest 1-based column without a stored diagonal (0: none), *unsym = smallest 1-based column
 * holding a stored (i,j) without a stored (j,i) (0: none) */
void model_amg_check(int64_t n, const int64_t *cp, const int64_t *rv, int64_t *nodiag, int64_t *unsym) {
    *nodiag = *unsym = 0;
    for (int64_t j = n - 1; j >= 0; j--) {
        if (find(cp, rv, j, j) < 0) *nodiag = j + 1;
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++)
            if (find(cp, rv, j, rv[k] - 1) < 0) *unsym = j + 1;
    }
}

/* strong[k] = 1 iff the stored entry k = (i,j) has i != j, a stored mirror (j,i), m = max(|a_ij|, |a_ji|) != 0 and
 * m*m >= (theta*theta)*(|a_ii|*|a_jj|); a diagonal that is not stored counts as 0.0 */
void model_amg_strength(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, double theta, uint8_t *strong) {
    double *dg = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    for (int64_t j = 0; j < n; j++) {
        const int64_t pos = find(cp, rv, j, j);
        dg[j] = pos >= 0 ? nz[pos] : 0.0;
    }
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) {
            const int64_t i = rv[k] - 1;
            strong[k] = 0;
            if (i == j) continue;
            const int64_t pos = find(cp, rv, j, i);
            if (pos < 0) continue;
            const double x = fabs(nz[k]), y = fabs(nz[pos]);
            double m = x;
            if (y > m || m != m) m = y; /* the larger one; a NaN loses against a number */
            if (m != 0.0 && m * m >= (theta * theta) * (fabs(dg[i]) * fabs(dg[j]))) strong[k] = 1;
        }
    free(dg);
}

static uint64_t key(int64_t i) {
    uint32_t x = (uint32_t)i + 1u;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return ((uint64_t)x << 32) | (uint64_t)(uint32_t)i;
}

/* MIS(2) by Luby rounds, then the two joining passes.  state: 0 undecided, 1 root, 2 excluded.  agg[i] = the aggregate of i
 * (0-based; -1 if the passes left it without one, which maximality excludes); *rounds = rounds run; returns the number of
 * aggregates */
int64_t model_amg_aggregate(int64_t n, const int64_t *cp, const int64_t *rv, const uint8_t *strong, int64_t *agg, int32_t *rounds,
                            uint8_t *state) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    uint64_t *t = (uint64_t *)malloc(8 * nn), *t1 = (uint64_t *)malloc(8 * nn), *t2 = (uint64_t *)malloc(8 * nn);
    int64_t *num = (int64_t *)malloc(8 * nn), *a1 = (int64_t *)malloc(8 * nn);
    int64_t undecided = n;
    *rounds = 0;
    for (int64_t i = 0; i < n; i++) state[i] = 0;
    while (undecided > 0) {
        for (int64_t i = 0; i < n; i++) t[i] = state[i] == 2 ? 0 : state[i] == 1 ? UINT64_MAX : key(i);
        for (int64_t i = 0; i < n; i++) {
            uint64_t m = t[i];
            for (int64_t k = cp[i] - 1; k < cp[i + 1] - 1; k++)
                if (strong[k] && t[rv[k] - 1] > m) m = t[rv[k] - 1];
            t1[i] = m;
        }
        for (int64_t i = 0; i < n; i++) {
            uint64_t m = t1[i];
            for (int64_t k = cp[i] - 1; k < cp[i + 1] - 1; k++)
                if (strong[k] && t1[rv[k] - 1] > m) m = t1[rv[k] - 1];
            t2[i] = m;
        }
        undecided = 0;
        for (int64_t i = 0; i < n; i++) {
            if (state[i] != 0) continue;
            if (t2[i] == key(i)) state[i] = 1;
            else if (t2[i] == UINT64_MAX) state[i] = 2;
            else undecided++;
        }
        (*rounds)++;
    }
    int64_t nc = 0;
    for (int64_t i = 0; i < n; i++) num[i] = state[i] == 1 ? nc++ : -1;
    /* pass 1: the aggregate of the smallest-index strong root neighbour */
    for (int64_t i = 0; i < n; i++) {
        a1[i] = num[i];
        if (a1[i] >= 0) continue;
        for (int64_t k = cp[i] - 1; k < cp[i + 1] - 1; k++)
            if (strong[k] && num[rv[k] - 1] >= 0) {
                a1[i] = num[rv[k] - 1];
                break;
            }
    }
    /* pass 2: what the smallest-index strong neighbour holds after pass 1 (never what pass 2 itself gives) */
    for (int64_t i = 0; i < n; i++) {
        agg[i] = a1[i];
        if (agg[i] >= 0) continue;
        for (int64_t k = cp[i] - 1; k < cp[i + 1] - 1; k++)
            if (strong[k] && a1[rv[k] - 1] >= 0) {
                agg[i] = a1[rv[k] - 1];
                break;
            }
    }
    free(t), free(t1), free(t2), free(num), free(a1);
    return nc;
}

/* inv = the inverse of the dense n x n matrix a (row-major) by Gauss-Jordan with partial pivoting on [a | I] */
void model_amg_gauss_jordan(int64_t n, const double *a, double *inv) {
    const int64_t W = 2 * n;
    double *g = (double *)calloc((size_t)(n * W > 0 ? n * W : 1), sizeof(double));
    for (int64_t i = 0; i < n; i++) {
        for (int64_t j = 0; j < n; j++) g[i * W + j] = a[i * n + j];
        g[i * W + n + i] = 1.0;
    }
    for (int64_t k = 0; k < n; k++) {
        int64_t p = k;
        double best = fabs(g[k * W + k]);
        for (int64_t r = k + 1; r < n; r++) { /* the largest |.|, the smallest row on ties */
            const double v = fabs(g[r * W + k]);
            if (v > best) {
                best = v;
                p = r;
            }
        }
        if (p != k)
            for (int64_t j = 0; j < W; j++) {
                const double s = g[k * W + j];
                g[k * W + j] = g[p * W + j];
                g[p * W + j] = s;
            }
        const double piv = g[k * W + k];
        for (int64_t j = 0; j < W; j++) g[k * W + j] = g[k * W + j] / piv; /* a zero pivot is no error */
        for (int64_t i = 0; i < n; i++) {
            if (i == k) continue;
            const double f = g[i * W + k];
            for (int64_t j = 0; j < W; j++) g[i * W + j] = g[i * W + j] - f * g[k * W + j];
        }
    }
    for (int64_t i = 0; i < n; i++)
        for (int64_t j = 0; j < n; j++) inv[i * n + j] = g[i * W + n + j];
    free(g);
}

/* r = A*x as mul! forms it: r .= 0, then column by column r[row] += nzval*x[col] */
static void mul(int64_t m, int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, const double *x, double *r) {
    for (int64_t i = 0; i < m; i++) r[i] = 0.0;
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) r[rv[k] - 1] += nz[k] * x[j];
}

/* one level of the hierarchy as the cycle needs it; P (n x nc) is unused on the coarsest level */
typedef struct {
    int64_t n, nc;
    const int64_t *acp, *arv;
    const double *anz;
    const int64_t *pcp, *prv;
    const double *pnz;
    const double *w;
} level_t;

static void sweep(const level_t *L, const double *b, double *x, double *t, double *xn) {
    mul(L->n, L->n, L->acp, L->arv, L->anz, x, t);
    for (int64_t i = 0; i < L->n; i++) xn[i] = x[i] + L->w[i] * (b[i] - t[i]); /* from the old x throughout */
    memcpy(x, xn, sizeof(double) * (size_t)L->n);
}

static void cycle(const level_t *lv, int32_t nlev, int32_t l, const double *inv, int32_t pre, int32_t post, const double *b, double *x) {
    const level_t *L = &lv[l];
    const int64_t n = L->n;
    const int last = l == nlev - 1;
    if (last && inv) {
        for (int64_t i = 0; i < n; i++) {
            double s = 0.0;
            for (int64_t j = 0; j < n; j++) s += inv[i * n + j] * b[j];
            x[i] = s;
        }
        return;
    }
    const size_t nn = (size_t)(n > 0 ? n : 1);
    double *t = (double *)malloc(8 * nn), *xn = (double *)malloc(8 * nn);
    for (int64_t i = 0; i < n; i++) x[i] = L->w[i] * b[i]; /* the first pre-sweep from x = 0 */
    for (int32_t k = 1; k < pre; k++) sweep(L, b, x, t, xn);
    if (!last) {
        const int64_t nc = L->nc;
        const size_t ncc = (size_t)(nc > 0 ? nc : 1);
        double *r = (double *)malloc(8 * nn), *bc = (double *)malloc(8 * ncc), *xc = (double *)malloc(8 * ncc);
        mul(n, n, L->acp, L->arv, L->anz, x, t);
        for (int64_t i = 0; i < n; i++) r[i] = b[i] - t[i];
        for (int64_t j = 0; j < nc; j++) { /* transpose(P)*r */
            double tmp = 0.0;
            bc[j] = 0.0;
            for (int64_t k = L->pcp[j] - 1; k < L->pcp[j + 1] - 1; k++) tmp += L->pnz[k] * r[L->prv[k] - 1];
            bc[j] += tmp;
        }
        cycle(lv, nlev, l + 1, inv, pre, post, bc, xc);
        mul(n, nc, L->pcp, L->prv, L->pnz, xc, t); /* e = P*x_c */
        for (int64_t i = 0; i < n; i++) x[i] = x[i] + t[i];
        free(r), free(bc), free(xc);
    }
    for (int32_t k = 0; k < post; k++) sweep(L, b, x, t, xn);
    free(t), free(xn);
}

/* u = the V-cycle applied to v.  Per level l: ns[l], and pointers to colptr / rowval / nzval of A_l, of P_l (NULL on the coarsest)
 * and to w_l; inv: the dense inverse of the coarsest level or NULL (smoothing only) */
void model_amg_cycle(int32_t nlev, const int64_t *ns, const void *const *acp, const void *const *arv, const void *const *anz,
                     const void *const *pcp, const void *const *prv, const void *const *pnz, const void *const *w, const double *inv,
                     int32_t pre, int32_t post, const double *v, double *u) {
    level_t *lv = (level_t *)calloc((size_t)nlev, sizeof(level_t));
    for (int32_t l = 0; l < nlev; l++) {
        lv[l].n = ns[l];
        lv[l].nc = l + 1 < nlev ? ns[l + 1] : 0;
        lv[l].acp = (const int64_t *)acp[l], lv[l].arv = (const int64_t *)arv[l], lv[l].anz = (const double *)anz[l];
        lv[l].pcp = (const int64_t *)pcp[l], lv[l].prv = (const int64_t *)prv[l], lv[l].pnz = (const double *)pnz[l];
        lv[l].w = (const double *)w[l];
    }
    const int64_t n = ns[0];
    double *x = (double *)malloc(8 * (size_t)(n > 0 ? n : 1));
    cycle(lv, nlev, 0, inv, pre, post, v, x);
    memcpy(u, x, sizeof(double) * (size_t)n);
    free(x), free(lv);
}
