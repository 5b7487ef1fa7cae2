/* cholesky_model.c -- the normative model of CholeskyFactorization as plain loops (test infrastructure).
 *
 * The ordering c, the nodes and the pattern are lu_model.c's: column j of L holds, in positions of c, the rows >= j of column j
 * of the filled matrix B.  L comes as a CSC with Julia's 1-based colptr / rowval, rows ascending, the diagonal first.
 * Every product is rounded, then every difference: build with -ffp-contract=off. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* lnz[q] of the entry (i, j) of L = the bits of the stored A[min(c[i], c[j]), max(c[i], c[j])], +0.0 where A stores none: only the
 * entries A[r, s] with r <= s are ever read */
void model_chol_load(int64_t n, const int64_t *acp, const int64_t *arv, const double *anz, const int64_t *c, const int64_t *lcp,
                     const int64_t *lrv, double *lnz) {
    for (int64_t j = 0; j < n; j++)
        for (int64_t q = lcp[j] - 1; q < lcp[j + 1] - 1; q++) {
            const int64_t i = lrv[q] - 1;
            const int64_t r = c[i] < c[j] ? c[i] : c[j], s = c[i] < c[j] ? c[j] : c[i];
            double v = 0.0;
            for (int64_t t = acp[s] - 1; t < acp[s + 1] - 1; t++)
                if (arv[t] - 1 == r) v = anz[t];
            lnz[q] = v;
        }
}

/* the entries of every row of L, k ascending: rp[i] .. rp[i + 1] of (rk = the column, rq = the position in lnz) */
static void rows_of(int64_t n, const int64_t *lcp, const int64_t *lrv, int64_t *rp, int64_t *rk, int64_t *rq) {
    memset(rp, 0, sizeof(int64_t) * (size_t)(n + 2));
    for (int64_t q = 0; q < lcp[n] - 1; q++) rp[lrv[q] + 1]++; /* row i counts at rp[i + 2] */
    for (int64_t i = 0; i < n; i++) rp[i + 2] += rp[i + 1];
    for (int64_t k = 0; k < n; k++)
        for (int64_t q = lcp[k] - 1; q < lcp[k + 1] - 1; q++) {
            const int64_t at = rp[lrv[q]]++; /* (rp[i + 1] runs from the start of row i to the start of row i + 1) */
            rk[at] = k;
            rq[at] = q;
        }
}

/* lnz: a_ij on entry, l_ij on return.  Returns 0, or 1 + the smallest position whose pivot fails (the columns behind it are left
 * as they were loaded) */
int64_t model_chol_factor(int64_t n, const int64_t *lcp, const int64_t *lrv, double *lnz) {
    const int64_t nnz = n > 0 ? lcp[n] - 1 : 0;
    int64_t *rp = malloc(sizeof(int64_t) * (size_t)(n + 2)), *rk = malloc(sizeof(int64_t) * (size_t)(nnz + 1)),
            *rq = malloc(sizeof(int64_t) * (size_t)(nnz + 1));
    int64_t bad = 0;
    rows_of(n, lcp, lrv, rp, rk, rq);
    for (int64_t j = 0; j < n && !bad; j++) {
        double ljj = 0.0;
        for (int64_t q = lcp[j] - 1; q < lcp[j + 1] - 1; q++) {
            const int64_t i = lrv[q] - 1;
            double t = lnz[q];
            int64_t a = rp[i], b = rp[j]; /* the rows i and j of L, merged on their common columns k < j */
            while (a < rp[i + 1] && b < rp[j + 1] && rk[a] < j && rk[b] < j) {
                if (rk[a] < rk[b]) a++;
                else if (rk[b] < rk[a]) b++;
                else {
                    const double pr = lnz[rq[a]] * lnz[rq[b]];
                    t = t - pr;
                    a++;
                    b++;
                }
            }
            if (i == j) {
                if (!(t > 0)) {
                    bad = j + 1;
                    break;
                }
                ljj = sqrt(t);
                lnz[q] = ljj;
            } else {
                lnz[q] = t / ljj;
            }
        }
    }
    free(rp);
    free(rk);
    free(rq);
    return bad;
}

/* y = v[c] on entry, x on return (u[c] = x).  nstart[j] / nsize[j]: the start and the size of the node of position j */
void model_chol_solve(int64_t n, const int64_t *lcp, const int64_t *lrv, const double *lnz, const int64_t *nstart, const int64_t *nsize,
                      double *y) {
    const int64_t nnz = n > 0 ? lcp[n] - 1 : 0;
    int64_t *rp = malloc(sizeof(int64_t) * (size_t)(n + 2)), *rk = malloc(sizeof(int64_t) * (size_t)(nnz + 1)),
            *rq = malloc(sizeof(int64_t) * (size_t)(nnz + 1));
    rows_of(n, lcp, lrv, rp, rk, rq);
    for (int64_t j = 0; j < n; j++) { /* forward */
        double t = y[j];
        for (int64_t a = rp[j]; a < rp[j + 1] && rk[a] < j; a++) {
            const double pr = lnz[rq[a]] * y[rk[a]];
            t = t - pr;
        }
        y[j] = t / lnz[lcp[j] - 1];
    }
    for (int64_t j = n - 1; j >= 0; j--) { /* backward: struct of the node ascending, then the node's positions behind j descending */
        const int64_t end = nstart[j] + nsize[j], q0 = lcp[j] - 1, q1 = lcp[j + 1] - 1;
        double t = y[j];
        int64_t qs = q0 + 1;
        while (qs < q1 && lrv[qs] - 1 < end) qs++;
        for (int64_t q = qs; q < q1; q++) {
            const double pr = lnz[q] * y[lrv[q] - 1];
            t = t - pr;
        }
        for (int64_t q = qs - 1; q > q0; q--) {
            const double pr = lnz[q] * y[lrv[q] - 1];
            t = t - pr;
        }
        y[j] = t / lnz[q0];
    }
    free(rp);
    free(rk);
    free(rq);
}
