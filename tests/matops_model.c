/* matops_model.c -- test infrastructure: SparseArrays' A*B (spmatmul), map(+/-, A, B) and Diagonal scaling restated as the
 * literal loops of the rules include/esparse_hip.h states for esp_matmul / esp_add / esp_diag_scale.  CSC arrays in
 * Julia's layout (1-based Int64 colptr / rowval).  Built with -ffp-contract=off: no FMA. */
#include <stdint.h>
#include <stdlib.h>

static int cmp_i64(const void *a, const void *b) {
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    return x < y ? -1 : x > y;
}

/* C = A*B (A m x k, B k x n).  Gustavson: a dense accumulator with a marker; the first product that reaches a row is
 * assigned, later ones added in arrival order; every reached row stored, rows sorted.  rvC / nzC hold at least the number
 * of products.  Returns nnz(C). */
int64_t model_matmul(int64_t m, int64_t n, const int64_t *cpA, const int64_t *rvA, const double *nzA, const int64_t *cpB,
                     const int64_t *rvB, const double *nzB, int64_t *cpC, int64_t *rvC, double *nzC) {
    double *x = (double *)malloc(sizeof(double) * (size_t)(m > 0 ? m : 1));
    int64_t *mark = (int64_t *)malloc(sizeof(int64_t) * (size_t)(m > 0 ? m : 1));
    for (int64_t r = 0; r < m; r++) mark[r] = -1;
    int64_t nz = 0;
    cpC[0] = 1;
    for (int64_t i = 0; i < n; i++) {
        const int64_t start = nz;
        for (int64_t q = cpB[i] - 1; q < cpB[i + 1] - 1; q++) {
            const int64_t j = rvB[q] - 1;
            const double b = nzB[q];
            for (int64_t p = cpA[j] - 1; p < cpA[j + 1] - 1; p++) {
                const int64_t k = rvA[p] - 1;
                const double prod = nzA[p] * b;
                if (mark[k] != i) {
                    mark[k] = i;
                    x[k] = prod;
                    rvC[nz++] = k + 1;
                } else {
                    x[k] = x[k] + prod;
                }
            }
        }
        qsort(rvC + start, (size_t)(nz - start), sizeof(int64_t), cmp_i64);
        for (int64_t t = start; t < nz; t++) nzC[t] = x[rvC[t] - 1];
        cpC[i + 1] = nz + 1;
    }
    free(x);
    free(mark);
    return nz;
}

/* C = A + B (op 0) or A - B (op 1), both m x n: per column the two sorted row runs merge; both stored f(a,b), one stored
 * f(a,0.0) / f(0.0,b); a result that compares == 0 is not stored.  rvC / nzC hold nnz(A) + nnz(B).  Returns nnz(C). */
static double f(int op, double a, double b) { return op ? a - b : a + b; }
int64_t model_add(int64_t n, int op, const int64_t *cpA, const int64_t *rvA, const double *nzA, const int64_t *cpB,
                  const int64_t *rvB, const double *nzB, int64_t *cpC, int64_t *rvC, double *nzC) {
    int64_t nz = 0;
    cpC[0] = 1;
    for (int64_t i = 0; i < n; i++) {
        int64_t pa = cpA[i] - 1, pb = cpB[i] - 1;
        const int64_t ea = cpA[i + 1] - 1, eb = cpB[i + 1] - 1;
        while (pa < ea || pb < eb) {
            int64_t row;
            double v;
            if (pb >= eb || (pa < ea && rvA[pa] < rvB[pb])) {
                row = rvA[pa];
                v = f(op, nzA[pa++], 0.0);
            } else if (pa >= ea || rvB[pb] < rvA[pa]) {
                row = rvB[pb];
                v = f(op, 0.0, nzB[pb++]);
            } else {
                row = rvA[pa];
                v = f(op, nzA[pa++], nzB[pb++]);
            }
            if (!(v == 0.0)) {
                rvC[nz] = row;
                nzC[nz++] = v;
            }
        }
        cpC[i + 1] = nz + 1;
    }
    return nz;
}

/* Diagonal(d) * A (side 0: nzC[p] = d[row] * nz[p]) or A * Diagonal(d) (side 1: d[col] * nz[p]); the pattern of A */
void model_diag_scale(int side, int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, const double *d, double *nzC) {
    for (int64_t j = 0; j < n; j++)
        for (int64_t p = cp[j] - 1; p < cp[j + 1] - 1; p++) nzC[p] = (side == 0 ? d[rv[p] - 1] : d[j]) * nz[p];
}
