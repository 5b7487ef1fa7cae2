/* ilut_model.c -- normative model of ILUTPreconditioner (test infrastructure): the threshold ILU by synchronous sweeps of
 * DESIGN.md 5p / include/esparse_hip.h (esp_precon_ilut_create), entry by entry, with Julia's 1-based CSC arrays.
 *
 * State: a pattern S (scp, srv: rows ascending in every column, every diagonal position stored) and values F on it -- the scaled
 * unit-lower L strictly below the diagonal, U on and above it.
 *   model_ilut         the whole construction from A: initialisation, `steps` rounds of candidates / sweeps / drop / sweeps
 *   model_ilut_sweeps  `count` sweeps on the kept pattern from the current F and A's current values (the warm update; with
 *                      count = 2n the fixed point, which tests/test_ilut_model.py holds to iluam_model.c bit for bit)
 * The application is iluam_model.c's ldiv! over (S, F).
 * Built by the tests with gcc -O1 -ffp-contract=off: every product, difference and quotient rounded on its own.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* the 1-based position of row i in column j of (cp, rv), or 0 */
static int64_t find(const int64_t *cp, const int64_t *rv, int64_t i, int64_t j) {
    int64_t lo = cp[j - 1], hi = cp[j];
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (rv[mid - 1] < i) lo = mid + 1;
        else hi = mid;
    }
    return lo < cp[j] && rv[lo - 1] == i ? lo : 0;
}

/* the row-wise index of a pattern: row i holds rcol / rpos [rptr[i - 1], rptr[i]), columns ascending */
typedef struct {
    int64_t *rptr, *rcol, *rpos;
} Rows;

static Rows rows_of(int64_t n, const int64_t *cp, const int64_t *rv) {
    const int64_t nnz = cp[n] - 1;
    Rows r;
    r.rptr = (int64_t *)calloc((size_t)(n + 2), sizeof(int64_t));
    r.rcol = (int64_t *)malloc(sizeof(int64_t) * (size_t)(nnz > 0 ? nnz : 1));
    r.rpos = (int64_t *)malloc(sizeof(int64_t) * (size_t)(nnz > 0 ? nnz : 1));
    for (int64_t v = 1; v <= nnz; v++) r.rptr[rv[v - 1] + 1]++;
    for (int64_t i = 1; i <= n + 1; i++) r.rptr[i] += r.rptr[i - 1];
    for (int64_t j = 1; j <= n; j++)
        for (int64_t v = cp[j - 1]; v <= cp[j] - 1; v++) {
            const int64_t q = r.rptr[rv[v - 1]]++;
            r.rcol[q] = j;
            r.rpos[q] = v;
        }
    /* now rptr[i] = the end of row i = the start of row i + 1, rptr[0] = the start of row 1 */
    return r;
}

static void rows_free(Rows *r) {
    free(r->rptr);
    free(r->rcol);
    free(r->rpos);
}

/* one synchronous sweep on the pattern (cp, rv): fnew from fold.  For every (i,j): r = a_ij (+0.0 where A stores nothing), then
 * r = r - l_ik*u_kj for every k < min(i,j) with (i,k) and (k,j) in the pattern, k increasing; l_ij = r/u_jj(old), u_ij = r */
static void sweep(int64_t n, const int64_t *acp, const int64_t *arv, const double *anz, const int64_t *cp, const int64_t *rv,
                  const Rows *rows, const double *fold, double *fnew) {
    for (int64_t j = 1; j <= n; j++) {
        const int64_t dj = find(cp, rv, j, j);
        for (int64_t q = cp[j - 1]; q <= cp[j] - 1; q++) {
            const int64_t i = rv[q - 1];
            const int64_t pa = find(acp, arv, i, j);
            double r = pa ? anz[pa - 1] : 0.0;
            const int64_t m = i < j ? i : j;
            int64_t a = rows->rptr[i - 1], c = cp[j - 1];
            while (a < rows->rptr[i] && c <= cp[j] - 1) {
                const int64_t ka = rows->rcol[a], kc = rv[c - 1];
                if (ka >= m || kc >= m) break;
                if (ka < kc) a++;
                else if (kc < ka) c++;
                else {
                    r = r - fold[rows->rpos[a] - 1] * fold[c - 1];
                    a++;
                    c++;
                }
            }
            fnew[q - 1] = i > j ? r / fold[dj - 1] : r;
        }
    }
}

/* `count` sweeps on (scp, srv) in place: f holds the current values and receives the last sweep's */
void model_ilut_sweeps(int64_t n, const int64_t *acp, const int64_t *arv, const double *anz, const int64_t *scp, const int64_t *srv,
                       double *f, int64_t count) {
    const int64_t nnz = scp[n] - 1;
    Rows rows = rows_of(n, scp, srv);
    double *g = (double *)malloc(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1));
    for (int64_t t = 0; t < count; t++) {
        sweep(n, acp, arv, anz, scp, srv, &rows, f, g);
        memcpy(f, g, sizeof(double) * (size_t)nnz);
    }
    free(g);
    rows_free(&rows);
}

/* The construction.  scp (n + 1), srv / f (cap entries each) receive S and F; stats[2 t], stats[2 t + 1] = nnz(C), nnz(S) of step t.
 * Returns nnz(S), or
 *   -1  a column of A stores no diagonal entry (info[0] = the column),
 *   -2  step info[0] (0-based) found nnz(C) = info[1] > info[2] = (int64)(max_fill * nnz(A)),
 *   -3  cap is too small (cap >= (int64)(max_fill * nnz(A)) never is). */
int64_t model_ilut(int64_t n, const int64_t *acp, const int64_t *arv, const double *anz, double tau, int64_t steps, int64_t sweeps,
                   double max_fill, int64_t cap, int64_t *scp, int64_t *srv, double *f, int64_t *stats, int64_t *info) {
    const int64_t nnzA = acp[n] - 1;
    const int64_t limit = (int64_t)(max_fill * (double)nnzA);
    for (int64_t j = 1; j <= n; j++)
        if (!find(acp, arv, j, j)) {
            info[0] = j;
            return -1;
        }
    if (nnzA > cap) return -3;
    /* initialisation: S = pattern(A), u_ij = a_ij, l_ij = a_ij / a_jj */
    memcpy(scp, acp, sizeof(int64_t) * (size_t)(n + 1));
    memcpy(srv, arv, sizeof(int64_t) * (size_t)nnzA);
    for (int64_t j = 1; j <= n; j++) {
        const double piv = anz[find(acp, arv, j, j) - 1];
        for (int64_t q = acp[j - 1]; q <= acp[j] - 1; q++) f[q - 1] = arv[q - 1] > j ? anz[q - 1] / piv : anz[q - 1];
    }
    if (steps == 0) {
        model_ilut_sweeps(n, acp, arv, anz, scp, srv, f, sweeps);
        return nnzA;
    }
    int64_t *ccp = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n + 1));
    int64_t *crv = (int64_t *)malloc(sizeof(int64_t) * (size_t)(cap > 0 ? cap : 1));
    double *cf = (double *)malloc(sizeof(double) * (size_t)(cap > 0 ? cap : 1));
    char *mark = (char *)calloc((size_t)(n + 1), 1);
    int64_t ret = 0;
    for (int64_t t = 0; t < steps; t++) {
        /* 1. C = pattern((L + I) * U): column j holds every row i >= k of column k of S for every stored (k,j), k <= j */
        int64_t nc = 0;
        int over = 0;
        for (int64_t j = 1; j <= n && !over; j++) {
            ccp[j - 1] = nc + 1;
            for (int64_t c = scp[j - 1]; c <= scp[j] - 1 && srv[c - 1] <= j; c++) {
                const int64_t k = srv[c - 1];
                for (int64_t w = scp[k - 1]; w <= scp[k] - 1; w++)
                    if (srv[w - 1] >= k) mark[srv[w - 1]] = 1;
            }
            for (int64_t i = 1; i <= n; i++)
                if (mark[i]) {
                    mark[i] = 0;
                    if (nc < cap) crv[nc] = i;
                    nc++;
                }
        }
        ccp[n] = nc + 1;
        stats[2 * t] = nc;
        /* 3. the fill guard */
        if (nc > limit) {
            info[0] = t;
            info[1] = nc;
            info[2] = limit;
            ret = -2;
            break;
        }
        if (nc > cap) {
            ret = -3;
            break;
        }
        /* 2. F carried to C, +0.0 at the new positions */
        for (int64_t j = 1; j <= n; j++)
            for (int64_t q = ccp[j - 1]; q <= ccp[j] - 1; q++) {
                const int64_t ps = find(scp, srv, crv[q - 1], j);
                cf[q - 1] = ps ? f[ps - 1] : 0.0;
            }
        /* 4. sweeps on C */
        model_ilut_sweeps(n, acp, arv, anz, ccp, crv, cf, sweeps);
        /* 5. / 6. the drop: an off-diagonal (i,j) goes when fabs(l_ij) < tau (i > j) or fabs(u_ij) < tau*fabs(u_ii) (i < j) is true */
        int64_t ns = 0;
        for (int64_t j = 1; j <= n; j++) {
            scp[j - 1] = ns + 1;
            for (int64_t q = ccp[j - 1]; q <= ccp[j] - 1; q++) {
                const int64_t i = crv[q - 1];
                int drop = 0;
                if (i > j) drop = fabs(cf[q - 1]) < tau;
                else if (i < j) drop = fabs(cf[q - 1]) < tau * fabs(cf[find(ccp, crv, i, i) - 1]);
                if (!drop) {
                    srv[ns] = i;
                    f[ns] = cf[q - 1];
                    ns++;
                }
            }
        }
        scp[n] = ns + 1;
        stats[2 * t + 1] = ns;
        /* 7. sweeps on S */
        model_ilut_sweeps(n, acp, arv, anz, scp, srv, f, sweeps);
        ret = ns;
    }
    free(ccp);
    free(crv);
    free(cf);
    free(mark);
    return ret;
}
