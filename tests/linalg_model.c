/* linalg_model.c -- test infrastructure: SparseArrays' transpose, transpose(A)*x, issymmetric and opnorm restated as the literal
 * loops of their documented behaviour (the stated assumption of include/esparse_hip.h's linalg block).  Built with
 * gcc -O1 -ffp-contract=off (tests/linalg_modellib.py); 1-based CSC arrays as Julia holds them. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* Julia's max(x, y) / maximum for Float64: NaN propagates */
static double jl_max(double x, double y) {
    if (isnan(x)) return x;
    if (isnan(y)) return y;
    return x > y ? x : y;
}

/* halfperm!(X, A, 1:n, identity): X = copy(transpose(A)), A m x n; cpT: m + 1 entries, rvT / nzT: nnz(A).  Values are copied as
 * bits (memcpy), so -0.0 and NaN payloads stay. */
void model_transpose(int64_t m, int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, int64_t *cpT, int64_t *rvT,
                     double *nzT) {
    /* counts of A's rows, shifted by one: cpT[i + 1] = entries of row i, then the cumulative sum */
    for (int64_t i = 0; i <= m; i++) cpT[i] = 0;
    for (int64_t k = 0; k < cp[n] - 1; k++) cpT[rv[k]] += 1;
    cpT[0] = 1;
    for (int64_t i = 1; i <= m; i++) cpT[i] += cpT[i - 1];
    int64_t *next = (int64_t *)malloc(sizeof(int64_t) * (size_t)(m + 1));
    for (int64_t i = 0; i < m; i++) next[i] = cpT[i];
    /* every column of A in order: its entries go behind what earlier columns put into their rows */
    for (int64_t j = 1; j <= n; j++)
        for (int64_t k = cp[j - 1]; k < cp[j]; k++) {
            const int64_t i = rv[k - 1];
            const int64_t q = next[i - 1]++;
            rvT[q - 1] = j;
            memcpy(&nzT[q - 1], &nz[k - 1], sizeof(double));
        }
    free(next);
}

/* _At_or_Ac_mul_B!(r, A, x, true, false): x m entries, r n entries */
void model_mul_transpose(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, const double *x, double *r) {
    for (int64_t j = 0; j < n; j++) r[j] = 0.0;
    for (int64_t j = 1; j <= n; j++) {
        double tmp = 0.0;
        for (int64_t k = cp[j - 1]; k < cp[j]; k++) tmp += nz[k - 1] * x[rv[k - 1] - 1];
        r[j - 1] += tmp;
    }
}

/* opnorm(A, 1), general branch: the max over columns of colSum += abs(v) in stored order, nA starting at 0 */
double model_opnorm1(int64_t n, const int64_t *cp, const double *nz) {
    double nA = 0.0;
    for (int64_t j = 1; j <= n; j++) {
        double colSum = 0.0;
        for (int64_t k = cp[j - 1]; k < cp[j]; k++) colSum += fabs(nz[k - 1]);
        nA = jl_max(nA, colSum);
    }
    return nA;
}

/* opnorm(A, Inf), general branch: rowSum = zeros(m); rowSum[rowval[i]] += abs(nzval[i]) in storage order; maximum(rowSum) */
double model_opnorminf(int64_t m, int64_t n, const int64_t *cp, const int64_t *rv, const double *nz) {
    double *rowSum = (double *)calloc((size_t)(m > 0 ? m : 1), sizeof(double));
    for (int64_t i = 0; i < cp[n] - 1; i++) rowSum[rv[i] - 1] += fabs(nz[i]);
    double mx = rowSum[0];
    for (int64_t i = 1; i < m; i++) mx = jl_max(mx, rowSum[i]);
    free(rowSum);
    return mx;
}

/* issymmetric(Matrix(A)): the dense matrix, then A[i,j] == A[j,i] for every j >= i (LinearAlgebra's loop) */
int32_t model_issymmetric(int64_t m, int64_t n, const int64_t *cp, const int64_t *rv, const double *nz) {
    if (m != n) return 0;
    double *D = (double *)calloc((size_t)(m * n > 0 ? m * n : 1), sizeof(double));
    for (int64_t j = 1; j <= n; j++)
        for (int64_t k = cp[j - 1]; k < cp[j]; k++) D[(j - 1) * m + (rv[k - 1] - 1)] = nz[k - 1];
    int32_t sym = 1;
    for (int64_t i = 0; i < n && sym; i++)
        for (int64_t j = i; j < n; j++)
            if (!(D[j * m + i] == D[i * m + j])) {  /* A[i,j] (column j) against A[j,i] (column i) */
                sym = 0;
                break;
            }
    free(D);
    return sym;
}
