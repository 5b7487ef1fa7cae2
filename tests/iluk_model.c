/* iluk_model.c -- independent model of ILUKPreconditioner's filled matrix B (test infrastructure).
 *
 * Restates the sequential level-of-fill rule of include/esparse_hip.h (esp_precon_iluk_create) literally, row by row, with indices
 * 0-based inside and Julia's 1-based CSC arrays at the interface:
 *   lev(i,j) = 0 where A stores (i,j) (whatever the value: 0.0, -0.0 and NaN count), infinite elsewhere;
 *   for i = 0..n-1, for k < i in increasing order with lev(i,k) <= K, for j > k with lev(k,j) <= K:
 *       lev(i,j) = min(lev(i,j), lev(i,k) + lev(k,j) + 1);
 *   B holds every position with lev <= K: A's bits where lev = 0, +0.0 elsewhere, rows ascending in every column.
 * Row i is worked in a dense row of levels; of a finished row k only the part the rule reads later -- j > k with lev(k,j) <= K --
 * is kept (the rule changes lev(k,j), j > k, while i = k only, and reads it while i > k only).
 * The numeric side is tests/iluam_model.c applied to B.  Built by the tests with gcc -O1 -ffp-contract=off.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define LEV_INF (INT64_MAX / 4)

typedef struct {
    int64_t *col, *lev, *pos; /* pos: 0-based position in A's nzval of a level-0 entry, -1 for fill */
    int64_t len, up;          /* entries of the row (columns ascending); index of the first one with col > row */
} Row;

/* B of (n, colptr, rowval, nzval) for the level K >= 0.  Returns nnz(B), or -1 without memory.  bcolptr (n + 1, 1-based) is always
 * written; browval (1-based), bnzval and blev (the level of every stored entry) only when cap >= nnz(B): call once with cap = 0 for
 * the size, then again. */
int64_t model_iluk(int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, int64_t K, int64_t *bcolptr,
                   int64_t *browval, double *bnzval, int32_t *blev, int64_t cap) {
    const int64_t nnz = n > 0 ? colptr[n] - 1 : 0;
    int64_t *rptr = (int64_t *)calloc((size_t)(n + 2), sizeof(int64_t));
    int64_t *rcol = (int64_t *)malloc(sizeof(int64_t) * (size_t)(nnz > 0 ? nnz : 1));
    int64_t *rpos = (int64_t *)malloc(sizeof(int64_t) * (size_t)(nnz > 0 ? nnz : 1));
    int64_t *lev = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
    int64_t *pos = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
    Row *rows = (Row *)calloc((size_t)(n > 0 ? n : 1), sizeof(Row));
    if (!rptr || !rcol || !rpos || !lev || !pos || !rows) return -1;
    /* the rows of A: columns ascending */
    for (int64_t v = 0; v < nnz; v++) rptr[rowval[v]]++; /* rowval is 1-based: row r counts into rptr[r + 1] of a 0-based r */
    for (int64_t i = 1; i <= n; i++) rptr[i] += rptr[i - 1];
    {
        int64_t *next = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
        if (!next) return -1;
        for (int64_t i = 0; i < n; i++) next[i] = rptr[i];
        for (int64_t j = 0; j < n; j++)
            for (int64_t v = colptr[j] - 1; v < colptr[j + 1] - 1; v++) {
                const int64_t q = next[rowval[v] - 1]++;
                rcol[q] = j;
                rpos[q] = v;
            }
        free(next);
    }
    int64_t total = 0;
    for (int64_t i = 0; i < n; i++) {
        for (int64_t j = 0; j < n; j++) {
            lev[j] = LEV_INF;
            pos[j] = -1;
        }
        for (int64_t q = rptr[i]; q < rptr[i + 1]; q++) {
            lev[rcol[q]] = 0;
            pos[rcol[q]] = rpos[q];
        }
        for (int64_t k = 0; k < i; k++) {
            if (lev[k] > K) continue;
            const Row *rk = &rows[k];
            for (int64_t t = rk->up; t < rk->len; t++) { /* j > k with lev(k,j) <= K */
                const int64_t j = rk->col[t];
                const int64_t cand = lev[k] + rk->lev[t] + 1;
                if (cand < lev[j]) lev[j] = cand;
            }
        }
        int64_t len = 0;
        for (int64_t j = 0; j < n; j++) len += lev[j] <= K;
        Row *ri = &rows[i];
        ri->col = (int64_t *)malloc(sizeof(int64_t) * (size_t)(len > 0 ? len : 1));
        ri->lev = (int64_t *)malloc(sizeof(int64_t) * (size_t)(len > 0 ? len : 1));
        ri->pos = (int64_t *)malloc(sizeof(int64_t) * (size_t)(len > 0 ? len : 1));
        if (!ri->col || !ri->lev || !ri->pos) return -1;
        ri->len = 0;
        ri->up = -1;
        for (int64_t j = 0; j < n; j++)
            if (lev[j] <= K) {
                if (j > i && ri->up < 0) ri->up = ri->len;
                ri->col[ri->len] = j;
                ri->lev[ri->len] = lev[j];
                ri->pos[ri->len] = pos[j];
                ri->len++;
            }
        if (ri->up < 0) ri->up = ri->len;
        total += len;
    }
    /* the rows in increasing order into the columns: rows ascending in every column */
    for (int64_t j = 0; j <= n; j++) bcolptr[j] = 0;
    for (int64_t i = 0; i < n; i++)
        for (int64_t t = 0; t < rows[i].len; t++) bcolptr[rows[i].col[t] + 1]++;
    bcolptr[0] = 1;
    for (int64_t j = 1; j <= n; j++) bcolptr[j] += bcolptr[j - 1];
    if (cap >= total) {
        int64_t *next = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
        if (!next) return -1;
        for (int64_t j = 0; j < n; j++) next[j] = bcolptr[j] - 1;
        for (int64_t i = 0; i < n; i++)
            for (int64_t t = 0; t < rows[i].len; t++) {
                const int64_t q = next[rows[i].col[t]]++;
                browval[q] = i + 1;
                blev[q] = (int32_t)rows[i].lev[t];
                if (rows[i].pos[t] >= 0) memcpy(&bnzval[q], &nzval[rows[i].pos[t]], sizeof(double)); /* the bits */
                else bnzval[q] = 0.0;
            }
        free(next);
    }
    for (int64_t i = 0; i < n; i++) {
        free(rows[i].col);
        free(rows[i].lev);
        free(rows[i].pos);
    }
    free(rows);
    free(rptr);
    free(rcol);
    free(rpos);
    free(lev);
    free(pos);
    return total;
}
