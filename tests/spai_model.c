// spai_model.c -- the normative model of SPAIPreconditioner (include/esparse_hip.h, esp_precon_spai_create; test infrastructure):
// the sparse approximate inverses SPAI-0 and SPAI-1 of a square matrix held column-wise, as plain loops.  M minimises
// |I - A*M|_F over the pattern of A, one column at a time; the device result equals this model bit for bit.
// Julia CSC arrays (colptr and rowval 1-based), indices below 0-based.  Build: gcc -O1 -ffp-contract=off -shared -fPIC ... -lm
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

// the ordered sum of p terms: part[l] adds the terms r = l, l + 64, ... in increasing r, starting from the first one (+0.0 where
// there is none); then the tree s = 32, 16, .., 1: part[l] = part[l] + part[l + s] for l < s; the result is part[0]
static double osum(const double *t, int64_t p) {
    double part[64];
    for (int l = 0; l < 64; l++) {
        if (l < p) {
            part[l] = t[l];
            for (int64_t r = (int64_t)l + 64; r < p; r += 64) part[l] = part[l] + t[r];
        } else {
            part[l] = 0.0;
        }
    }
    for (int s = 32; s >= 1; s >>= 1)
        for (int l = 0; l < s; l++) part[l] = part[l] + part[l + s];
    return part[0];
}

// SPAI-0: d[k] = a_kk / osum(a*a over the stored entries of column k), a_kk = +0.0 where the diagonal is not stored
void model_spai0(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, double *d) {
    for (int64_t k = 0; k < n; k++) {
        const int64_t s = cp[k] - 1, q = cp[k + 1] - 1 - s;
        double *t = (double *)malloc(sizeof(double) * (size_t)(q > 0 ? q : 1));
        double akk = 0.0;
        for (int64_t c = 0; c < q; c++) {
            t[c] = nz[s + c] * nz[s + c];
            if (rv[s + c] - 1 == k) akk = nz[s + c];
        }
        d[k] = akk / osum(t, q);
        free(t);
    }
}

// SPAI-1: m (nnz values, the positions of A) ; pcol (n, may be NULL): p of every column; stats (4, may be NULL): max p, max q,
// max p*q, 0.  Returns 0, or -1 when memory ran out.
int64_t model_spai1(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, double *m, int64_t *pcol, int64_t *stats) {
    int64_t maxp = 0, maxq = 0, maxpq = 0;
    uint8_t *mark = (uint8_t *)calloc((size_t)(n > 0 ? n : 1), 1);
    int64_t *I = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
    int64_t *loc = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
    if (!mark || !I || !loc) return -1;
    for (int64_t k = 0; k < n; k++) {
        // 1. J: the stored rows of column k, ascending
        const int64_t ks = cp[k] - 1, q = cp[k + 1] - 1 - ks;
        const int64_t *J = rv + ks;  // (1-based)
        // 2. I: the ascending union of the stored rows of the columns j in J
        int64_t p = 0;
        for (int64_t c = 0; c < q; c++) {
            const int64_t j = J[c] - 1;
            for (int64_t e = cp[j] - 1; e < cp[j + 1] - 1; e++) mark[rv[e] - 1] = 1;
        }
        int64_t lo = n, hi = -1;
        for (int64_t c = 0; c < q; c++) {
            const int64_t j = J[c] - 1;
            if (cp[j + 1] > cp[j]) {
                if (rv[cp[j] - 1] - 1 < lo) lo = rv[cp[j] - 1] - 1;
                if (rv[cp[j + 1] - 2] - 1 > hi) hi = rv[cp[j + 1] - 2] - 1;
            }
        }
        for (int64_t r = lo; r <= hi; r++)
            if (mark[r]) {
                mark[r] = 0;
                loc[r] = p;
                I[p++] = r;
            }
        if (pcol) pcol[k] = p;
        if (p > maxp) maxp = p;
        if (q > maxq) maxq = q;
        if (p * q > maxpq) maxpq = p * q;
        if (q == 0) continue;
        // 3. B = A[I, J], dense p x q, column-major: A's bits where stored, +0.0 elsewhere
        double *B = (double *)malloc(sizeof(double) * (size_t)(p * q > 0 ? p * q : 1));
        double *R = (double *)malloc(sizeof(double) * (size_t)(q * q));
        double *t = (double *)malloc(sizeof(double) * (size_t)(p > 0 ? p : 1));
        double *y = (double *)malloc(sizeof(double) * (size_t)q);
        if (!B || !R || !t || !y) return -1;
        for (int64_t i = 0; i < p * q; i++) B[i] = 0.0;
        for (int64_t c = 0; c < q; c++) {
            const int64_t j = J[c] - 1;
            for (int64_t e = cp[j] - 1; e < cp[j + 1] - 1; e++) B[loc[rv[e] - 1] + c * p] = nz[e];
        }
        // 5. modified Gram-Schmidt
        for (int64_t c = 0; c < q; c++) {
            for (int64_t r = 0; r < p; r++) t[r] = B[r + c * p] * B[r + c * p];
            R[c * q + c] = sqrt(osum(t, p));
            for (int64_t r = 0; r < p; r++) B[r + c * p] = B[r + c * p] / R[c * q + c];
            for (int64_t d = c + 1; d < q; d++) {
                for (int64_t r = 0; r < p; r++) t[r] = B[r + c * p] * B[r + d * p];
                R[c * q + d] = osum(t, p);
                for (int64_t r = 0; r < p; r++) B[r + d * p] = B[r + d * p] - R[c * q + d] * B[r + c * p];
            }
        }
        // 6. the right-hand side: row k of the normalised columns
        int64_t pos = -1;
        for (int64_t r = 0; r < p; r++)
            if (I[r] == k) pos = r;
        for (int64_t c = 0; c < q; c++) y[c] = pos >= 0 ? B[pos + c * p] : 0.0;
        // 7. back substitution
        for (int64_t c = q - 1; c >= 0; c--) {
            double v = y[c];
            for (int64_t d = c + 1; d < q; d++) v = v - R[c * q + d] * y[d];
            y[c] = v / R[c * q + c];
        }
        // 8.
        for (int64_t c = 0; c < q; c++) m[ks + c] = y[c];
        free(B);
        free(R);
        free(t);
        free(y);
    }
    free(mark);
    free(I);
    free(loc);
    if (stats) {
        stats[0] = maxp;
        stats[1] = maxq;
        stats[2] = maxpq;
        stats[3] = 0;
    }
    return 0;
}
