/* coloring_model.c -- the multicolour ordering of include/esparse_hip.h (esp_graph_coloring, esp_precon_colored_create), restated as
 * plain loops (test infrastructure).  NORMATIVE: the graph, the priority, the rounds, the permutation and the reordered matrix.
 * The preconditioner itself needs no model of its own: it is precon_model.c / iluam_model.c applied to A[c,c] with v[c], scattered
 * back (tests/coloring_modellib.py composes them).
 * Build: gcc -O1 -ffp-contract=off.  CSC arrays in Julia layout (colptr and rowval 1-based, rows ascending in every column).
 * Nothing here knows of the device code. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* key(i) = (u64)mix(i) << 32 | i with the 32-bit mixer of the aggregation's hash (amg_model.c), applied to i + 1 */
static uint64_t key(int64_t i) {
    uint32_t x = (uint32_t)i + 1u;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return ((uint64_t)x << 32) | (uint64_t)(uint32_t)i;
}

/* The rounds.  i and j != i are neighbours when (i,j) or (j,i) is stored; the values are never read.  color[i] = 0-based colour.
 * Returns ncolors = the number of rounds. */
int64_t model_coloring(int64_t n, const int64_t *cp, const int64_t *rv, int64_t *color) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    /* the stored (i, j) row by row: rp[i] .. rp[i + 1] of cj hold the columns j of row i */
    int64_t *rp = (int64_t *)calloc(nn + 1, 8), *cj = (int64_t *)malloc(8 * (size_t)(cp[n] > 1 ? cp[n] - 1 : 1));
    int64_t *fill = (int64_t *)malloc(8 * nn);
    uint8_t *inU = (uint8_t *)malloc(nn), *win = (uint8_t *)malloc(nn);
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) rp[rv[k]]++;
    for (int64_t i = 0; i < n; i++) rp[i + 1] += rp[i];
    for (int64_t i = 0; i < n; i++) fill[i] = rp[i];
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) cj[fill[rv[k] - 1]++] = j;
    for (int64_t i = 0; i < n; i++) color[i] = -1;
    int64_t left = n, r = 0;
    while (left > 0) {
        r++;
        for (int64_t i = 0; i < n; i++) inU[i] = color[i] < 0; /* U: uncoloured at the start of the round */
        for (int64_t i = 0; i < n; i++) {
            win[i] = inU[i];
            if (!inU[i]) continue;
            for (int64_t k = cp[i] - 1; k < cp[i + 1] - 1; k++) { /* (j, i) stored */
                const int64_t j = rv[k] - 1;
                if (j != i && inU[j] && !(key(i) > key(j))) win[i] = 0;
            }
            for (int64_t k = rp[i]; k < rp[i + 1]; k++) { /* (i, j) stored */
                const int64_t j = cj[k];
                if (j != i && inU[j] && !(key(i) > key(j))) win[i] = 0;
            }
        }
        for (int64_t i = 0; i < n; i++)
            if (win[i]) {
                color[i] = r - 1;
                left--;
            }
    }
    free(rp);
    free(cj);
    free(fill);
    free(inU);
    free(win);
    return r;
}

/* c = the vertices sorted by (colour, index), 0-based; ptr[0..ncolors] delimits the colours in c */
void model_color_perm(int64_t n, int64_t ncolors, const int64_t *color, int64_t *c, int64_t *ptr) {
    int64_t k = 0;
    ptr[0] = 0;
    for (int64_t r = 0; r < ncolors; r++) {
        for (int64_t i = 0; i < n; i++)
            if (color[i] == r) c[k++] = i;
        ptr[r + 1] = k;
    }
}

/* B = A[c,c]: B[k,l] = A[c[k],c[l]], every column sorted by row, the values moved as they are.  bcp: n + 1, brv / bnz: nnz(A) */
void model_reorder(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, const int64_t *c, int64_t *bcp, int64_t *brv,
                   double *bnz) {
    int64_t *new_of = (int64_t *)malloc(8 * (size_t)(n > 0 ? n : 1));
    for (int64_t k = 0; k < n; k++) new_of[c[k]] = k;
    int64_t q = 0;
    bcp[0] = 1;
    for (int64_t l = 0; l < n; l++) {
        const int64_t j = c[l], q0 = q;
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) { /* insertion by the new row (distinct) */
            const int64_t row = new_of[rv[k] - 1] + 1;
            int64_t t = q++;
            while (t > q0 && brv[t - 1] > row) {
                brv[t] = brv[t - 1];
                memcpy(&bnz[t], &bnz[t - 1], 8);
                t--;
            }
            brv[t] = row;
            memcpy(&bnz[t], &nz[k], 8);
        }
        bcp[l + 1] = q + 1;
    }
    free(new_of);
}
