/* cholesky_model_main.c -- a stand-alone run of tests/cholesky_model.c for the sanitizers (test infrastructure):
 *   gcc -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all cholesky_model_main.c cholesky_model.c -lm
 * Two tiny systems with hand-written patterns: a path 0 - 2 - 1 ordered as two leaves and their separator, and one dense node of
 * five positions; each loaded, factorized, solved and checked against A x = b; then an indefinite matrix, whose failing position is
 * checked.  Prints "cholesky_model_main: ok" and returns 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>

void model_chol_load(int64_t n, const int64_t *acp, const int64_t *arv, const double *anz, const int64_t *c, const int64_t *lcp,
                     const int64_t *lrv, double *lnz);
int64_t model_chol_factor(int64_t n, const int64_t *lcp, const int64_t *lrv, double *lnz);
void model_chol_solve(int64_t n, const int64_t *lcp, const int64_t *lrv, const double *lnz, const int64_t *nstart, const int64_t *nsize,
                      double *y);

/* |S x - b| with S the symmetric matrix of the upper triangle of the CSC (acp, arv, anz) */
static double residual(int64_t n, const int64_t *acp, const int64_t *arv, const double *anz, const double *x, const double *b) {
    double r[8] = {0}, m = 0.0;
    for (int64_t s = 0; s < n; s++)
        for (int64_t q = acp[s] - 1; q < acp[s + 1] - 1; q++) {
            const int64_t i = arv[q] - 1;
            if (i > s) continue;
            r[i] += anz[q] * x[s];
            if (i != s) r[s] += anz[q] * x[i];
        }
    for (int64_t i = 0; i < n; i++) m = fmax(m, fabs(r[i] - b[i]));
    return m;
}

static int run(const char *name, int64_t n, const int64_t *acp, const int64_t *arv, const double *anz, const int64_t *c, const int64_t *lcp,
               const int64_t *lrv, const int64_t *nstart, const int64_t *nsize, int64_t want_bad) {
    double lnz[32], b[8], y[8], x[8];
    model_chol_load(n, acp, arv, anz, c, lcp, lrv, lnz);
    const int64_t bad = model_chol_factor(n, lcp, lrv, lnz);
    if (bad != want_bad) {
        printf("%s: factor returned %lld, expected %lld\n", name, (long long)bad, (long long)want_bad);
        return 1;
    }
    if (bad) return 0;
    for (int64_t i = 0; i < n; i++) b[i] = 1.0 + 0.5 * (double)i;
    for (int64_t k = 0; k < n; k++) y[k] = b[c[k]];
    model_chol_solve(n, lcp, lrv, lnz, nstart, nsize, y);
    for (int64_t k = 0; k < n; k++) x[c[k]] = y[k];
    const double r = residual(n, acp, arv, anz, x, b);
    if (!(r <= 1e-13)) {
        printf("%s: residual %.3e\n", name, r);
        return 1;
    }
    return 0;
}

int main(void) {
    int fail = 0;
    { /* the path 0 - 2 - 1 in A's numbering 0 - 1 - 2: c = (0, 2, 1); a stored strict lower entry that must not be read */
        const int64_t acp[] = {1, 3, 5, 7}, arv[] = {1, 2, 1, 2, 2, 3};
        const double anz[] = {4.0, 1e300, -1.0, 5.0, -2.0, 6.0};
        const int64_t c[] = {0, 2, 1}, lcp[] = {1, 3, 5, 6}, lrv[] = {1, 3, 2, 3, 3};
        const int64_t nstart[] = {0, 1, 2}, nsize[] = {1, 1, 1};
        fail |= run("path", 3, acp, arv, anz, c, lcp, lrv, nstart, nsize, 0);
    }
    { /* one dense node of five positions, c the identity: the upper triangle of a diagonally dominant matrix */
        int64_t acp[6], arv[15], lcp[6], lrv[15], c[5], nstart[5], nsize[5], q = 0, p = 0;
        double anz[15];
        for (int64_t s = 0; s < 5; s++) {
            acp[s] = q + 1;
            for (int64_t i = 0; i <= s; i++, q++) {
                arv[q] = i + 1;
                anz[q] = i == s ? 6.0 + (double)s : -1.0 / (double)(1 + s - i);
            }
            lcp[s] = p + 1;
            for (int64_t i = s; i < 5; i++) lrv[p++] = i + 1;
            c[s] = s;
            nstart[s] = 0;
            nsize[s] = 5;
        }
        acp[5] = q + 1;
        lcp[5] = p + 1;
        fail |= run("dense", 5, acp, arv, anz, c, lcp, lrv, nstart, nsize, 0);
        anz[5] = -anz[5]; /* A[2,2] negated: the pivot of position 2 fails */
        fail |= run("indefinite", 5, acp, arv, anz, c, lcp, lrv, nstart, nsize, 3);
    }
    if (!fail) printf("cholesky_model_main: ok\n");
    return fail;
}
