/* rsamg_model.c -- the Ruge-Stueben coarsening of RS_AMGPreconditioner (include/esparse_hip.h, esp_precon_rsamg_create), restated
 * as plain loops (test infrastructure).  NORMATIVE for the order of every operation: row-wise strength, the rounds of the PMIS
 * splitting over the fixed hash, the numbering of the C points and direct interpolation.  Everything around it -- dinv, rho, w, the
 * checks of level 0, the Galerkin products, the coarsest level's inverse, the V-cycle -- is amg_model.c's and the algebra models':
 * tests/rsamg_modellib.py composes them.
 * Build: gcc -O1 -ffp-contract=off (every product, sum and division rounded on its own).  CSC arrays in Julia layout (colptr and
 * rowval 1-based, rows ascending in every column).  Nothing here knows of the device code. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* position of (row i, column j), both 0-based, or -1 */
static int64_t find(const int64_t *cp, const int64_t *rv, int64_t i, int64_t j) {
    for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++)
        if (rv[k] - 1 == i) return k;
    return -1;
}

static uint32_t mix(int64_t i) {
    uint32_t x = (uint32_t)i + 1u;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

/* m[i] = the largest |a_ik| over the stored k != i of row i (0.0 for none; a NaN is never larger) */
static void rowmax(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, double *m) {
    for (int64_t i = 0; i < n; i++) m[i] = 0.0;
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) {
            const int64_t i = rv[k] - 1;
            if (i != j && fabs(nz[k]) > m[i]) m[i] = fabs(nz[k]);
        }
}

/* the value a of an off-diagonal entry of a row whose largest is mi: does the row depend on that column? */
static int strong(double a, double theta, double mi) { return fabs(a) != 0.0 && fabs(a) >= theta * mi; }

/* dep[k] = 1 iff the row of the stored entry k = (i,j) strongly depends on j: j in S_i */
void model_rsamg_strength(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, double theta, uint8_t *dep) {
    double *m = (double *)malloc(sizeof(double) * (size_t)(n > 0 ? n : 1));
    rowmax(n, cp, rv, nz, m);
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) {
            const int64_t i = rv[k] - 1;
            dep[k] = (uint8_t)(i != j && strong(nz[k], theta, m[i]));
        }
    free(m);
}

/* The PMIS splitting.  cf[i] = cnum(i) (0-based) for a C point, -1 for an F point with interpolation, -2 for an F point with an
 * empty S_i; *rounds = rounds run; returns the number of C points.  The neighbours of i are what a walk over COLUMN i meets:
 * the entry (r,i) tells "r depends on i" by itself and "i depends on r" by its stored mirror (i,r). */
int64_t model_rsamg_split(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, double theta, int64_t *cf, int32_t *rounds) {
    const size_t nn = (size_t)(n > 0 ? n : 1), zz = (size_t)(cp[n] > 1 ? cp[n] - 1 : 1);
    uint8_t *dep = (uint8_t *)malloc(zz), *state = (uint8_t *)malloc(nn), *next = (uint8_t *)malloc(nn);
    int64_t *mirror = (int64_t *)malloc(8 * zz);
    uint64_t *key = (uint64_t *)malloc(8 * nn);
    model_rsamg_strength(n, cp, rv, nz, theta, dep);
    int64_t undecided = 0;
    for (int64_t i = 0; i < n; i++) { /* state: 0 undecided, 1 C, 2 F, 3 F without interpolation */
        uint64_t lam = 0;
        int64_t ns = 0;
        for (int64_t k = cp[i] - 1; k < cp[i + 1] - 1; k++) {
            mirror[k] = find(cp, rv, i, rv[k] - 1); /* (i, r) in column r */
            if (dep[k]) lam++;
            if (mirror[k] >= 0 && dep[mirror[k]]) ns++;
        }
        key[i] = ((lam < 65535 ? lam : 65535) << 48) | ((uint64_t)(mix(i) >> 16) << 32) | (uint64_t)(uint32_t)i;
        state[i] = ns > 0 ? 0 : 3;
        if (ns > 0) undecided++;
    }
    *rounds = 0;
    while (undecided > 0) {
        /* phase 1, on the state of the round's start */
        for (int64_t i = 0; i < n; i++) {
            next[i] = state[i];
            if (state[i] != 0) continue;
            int beaten = 0;
            for (int64_t k = cp[i] - 1; k < cp[i + 1] - 1; k++) {
                const int64_t r = rv[k] - 1;
                const int nb = dep[k] || (mirror[k] >= 0 && dep[mirror[k]]);
                if (nb && state[r] == 0 && key[r] > key[i]) beaten = 1;
            }
            if (!beaten) next[i] = 1;
        }
        /* phase 2 */
        undecided = 0;
        for (int64_t i = 0; i < n; i++) {
            state[i] = next[i];
            if (next[i] != 0) continue;
            int hasc = 0;
            for (int64_t k = cp[i] - 1; k < cp[i + 1] - 1; k++)
                if (mirror[k] >= 0 && dep[mirror[k]] && next[rv[k] - 1] == 1) hasc = 1;
            if (hasc) state[i] = 2;
            else undecided++;
        }
        (*rounds)++;
    }
    int64_t nc = 0;
    for (int64_t i = 0; i < n; i++) cf[i] = state[i] == 1 ? nc++ : state[i] == 2 ? -1 : -2;
    free(dep), free(state), free(next), free(mirror), free(key);
    return nc;
}

/* Direct interpolation, written down as transpose(P) (nc x n): column i holds row i of P, its rows cnum(j) + 1 ascending.
 * tcp: n + 1, trv / tnz: room for nnz(A) + n entries.  Returns the number of entries. */
int64_t model_rsamg_interp(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, double theta, const int64_t *cf,
                           int64_t *tcp, int64_t *trv, double *tnz) {
    const size_t nn = (size_t)(n > 0 ? n : 1), zz = (size_t)(cp[n] > 1 ? cp[n] - 1 : 1);
    double *m = (double *)malloc(8 * nn), *rval = (double *)malloc(8 * zz);
    int64_t *rp = (int64_t *)calloc(nn + 1, 8), *rcol = (int64_t *)malloc(8 * zz), *fill = (int64_t *)malloc(8 * nn);
    rowmax(n, cp, rv, nz, m);
    /* the rows of A, columns ascending */
    for (int64_t k = 0; k < cp[n] - 1; k++) rp[rv[k]]++;
    for (int64_t i = 0; i < n; i++) rp[i + 1] += rp[i], fill[i] = rp[i];
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) {
            const int64_t q = fill[rv[k] - 1]++;
            rcol[q] = j;
            rval[q] = nz[k];
        }
    int64_t z = 0;
    for (int64_t i = 0; i < n; i++) {
        tcp[i] = z + 1;
        if (cf[i] >= 0) {
            trv[z] = cf[i] + 1;
            tnz[z] = 1.0;
            z++;
            continue;
        }
        if (cf[i] != -1) continue;
        double sn = 0.0, sp = 0.0, snc = 0.0, spc = 0.0, d = 0.0;
        for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
            const int64_t j = rcol[q];
            const double a = rval[q];
            if (j == i) {
                d = a;
                continue;
            }
            const int inc = strong(a, theta, m[i]) && cf[j] >= 0;
            if (a < 0.0) {
                sn = sn + a;
                if (inc) snc = snc + a;
            } else if (a > 0.0) {
                sp = sp + a;
                if (inc) spc = spc + a;
            }
        }
        double beta = 0.0;
        if (spc == 0.0) d = d + sp;
        else beta = sp / spc;
        const double alpha = snc != 0.0 ? sn / snc : 0.0;
        for (int64_t q = rp[i]; q < rp[i + 1]; q++) {
            const int64_t j = rcol[q];
            const double a = rval[q];
            if (j == i || !(strong(a, theta, m[i]) && cf[j] >= 0)) continue;
            trv[z] = cf[j] + 1;
            tnz[z] = (-(a < 0.0 ? alpha : beta) * a) / d;
            z++;
        }
    }
    tcp[n] = z + 1;
    free(m), free(rval), free(rp), free(rcol), free(fill);
    return z;
}
