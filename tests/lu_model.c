/* lu_model.c -- normative model of LUFactorization (include/esparse_hip.h, esp_precon_lu_create), restated as plain
 * loops (test infrastructure).  NORMATIVE: the graph, the dissection rounds, the tree, the permutation and the filled, reordered
 * matrix B.  The numerics need no model of their own: they are iluam_model.c applied to B with v[c], scattered back
 * (tests/lu_modellib.py composes them).
 * Build: gcc -O1 -ffp-contract=off.  CSC arrays in Julia layout (colptr and rowval 1-based, rows ascending in every column).
 * Nothing here knows of the device code. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define UNPLACED (-1)
#define FAR INT64_MAX

/* the colouring's key (coloring_model.c): distinct, so every comparison is strict */
static uint64_t key(int64_t i) {
    uint32_t x = (uint32_t)i + 1u;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return ((uint64_t)x << 32) | (uint64_t)(uint32_t)i;
}

typedef struct {
    int64_t n;
    const int64_t *cp, *rv; /* (j, i) stored: column i */
    int64_t *rp, *cj;       /* (i, j) stored: row i */
} graph;

static void graph_open(graph *g, int64_t n, const int64_t *cp, const int64_t *rv) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    g->n = n;
    g->cp = cp;
    g->rv = rv;
    g->rp = (int64_t *)calloc(nn + 1, 8);
    g->cj = (int64_t *)malloc(8 * (size_t)(cp[n] > 1 ? cp[n] - 1 : 1));
    int64_t *fill = (int64_t *)malloc(8 * nn);
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) g->rp[rv[k]]++;
    for (int64_t i = 0; i < n; i++) g->rp[i + 1] += g->rp[i];
    for (int64_t i = 0; i < n; i++) fill[i] = g->rp[i];
    for (int64_t j = 0; j < n; j++)
        for (int64_t k = cp[j] - 1; k < cp[j + 1] - 1; k++) g->cj[fill[rv[k] - 1]++] = j;
    free(fill);
}
static void graph_close(graph *g) {
    free(g->rp);
    free(g->cj);
}
/* the t-th neighbour slot of i (the column, then the row; i itself and repeats are among them): -1 behind the last */
static int64_t slot(const graph *g, int64_t i, int64_t t) {
    const int64_t nc = g->cp[i + 1] - g->cp[i];
    if (t < nc) return g->rv[g->cp[i] - 1 + t] - 1;
    t -= nc;
    if (t < g->rp[i + 1] - g->rp[i]) return g->cj[g->rp[i] + t];
    return -1;
}

/* a breadth-first search inside every component at once: dist holds 0 at the sources and FAR at every other unplaced vertex of a
 * split candidate; ecc[root of the component] = the largest distance.  comp[v] = the root of v's component */
static void bfs(const graph *g, const int64_t *level, const int64_t *comp, int64_t *dist, int64_t *ecc) {
    for (int64_t step = 1;; step++) {
        int64_t found = 0;
        for (int64_t v = 0; v < g->n; v++) {
            if (level[v] != UNPLACED || dist[v] != FAR) continue;
            int hit = 0;
            for (int64_t t = 0, j; (j = slot(g, v, t)) >= 0; t++)
                if (j != v && level[j] == UNPLACED && dist[j] == step - 1) hit = 1;
            if (hit) {
                dist[v] = step;
                ecc[comp[v]] = step;
                found++;
            }
        }
        if (!found) return;
    }
}

/* The dissection.  level[v] = the depth at which v was placed, anc[d * n + v] = the root of v's component in round d for every
 * d <= level[v] (-1 beyond).  anc holds (max_depth + 1) * n entries.  Returns the number of rounds. */
int64_t model_lu_dissect(int64_t n, const int64_t *cp, const int64_t *rv, int64_t leaf_size, int64_t max_depth, int64_t *level,
                         int64_t *anc) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    graph g;
    graph_open(&g, n, cp, rv);
    uint64_t *lab = (uint64_t *)malloc(8 * nn), *nxt = (uint64_t *)malloc(8 * nn), *best = (uint64_t *)malloc(8 * nn);
    int64_t *comp = (int64_t *)malloc(8 * nn), *size = (int64_t *)malloc(8 * nn), *dist = (int64_t *)malloc(8 * nn);
    int64_t *ecc = (int64_t *)malloc(8 * nn);
    for (int64_t v = 0; v < n; v++) level[v] = UNPLACED;
    for (int64_t k = 0; k < (max_depth + 1) * n; k++) anc[k] = -1;
    int64_t left = n, d = 0;
    while (left > 0) {
        /* 1. the components of the unplaced vertices: the largest key spreads until nothing changes */
        for (int64_t v = 0; v < n; v++) lab[v] = level[v] == UNPLACED ? key(v) : 0;
        for (int changed = 1; changed;) {
            changed = 0;
            for (int64_t v = 0; v < n; v++) {
                nxt[v] = lab[v];
                if (level[v] != UNPLACED) continue;
                for (int64_t t = 0, j; (j = slot(&g, v, t)) >= 0; t++)
                    if (level[j] == UNPLACED && lab[j] > nxt[v]) nxt[v] = lab[j];
                if (nxt[v] != lab[v]) changed = 1;
            }
            memcpy(lab, nxt, 8 * nn);
        }
        for (int64_t v = 0; v < n; v++) size[v] = 0;
        for (int64_t v = 0; v < n; v++)
            if (level[v] == UNPLACED) {
                comp[v] = (int64_t)(uint32_t)lab[v];
                anc[d * n + v] = comp[v];
                size[comp[v]]++;
            }
        /* 2. the leaves by size or depth; every other component is searched from its root */
        for (int64_t v = 0; v < n; v++) {
            if (level[v] != UNPLACED) continue;
            if (size[comp[v]] <= leaf_size || d == max_depth) {
                level[v] = d;
                left--;
            } else {
                dist[v] = v == comp[v] ? 0 : FAR;
                ecc[v] = 0;
                best[v] = 0;
            }
        }
        /* 3. dist0 from the root, r1 = the farthest vertex with the largest key, dist from r1 */
        bfs(&g, level, comp, dist, ecc);
        for (int64_t v = 0; v < n; v++)
            if (level[v] == UNPLACED && dist[v] == ecc[comp[v]] && key(v) > best[comp[v]]) best[comp[v]] = key(v);
        for (int64_t v = 0; v < n; v++)
            if (level[v] == UNPLACED) {
                dist[v] = key(v) == best[comp[v]] ? 0 : FAR;
                ecc[v] = 0;
            }
        bfs(&g, level, comp, dist, ecc);
        for (int64_t v = 0; v < n; v++) { /* (ecc and dist are read for unplaced vertices only: the order of v does not matter) */
            if (level[v] != UNPLACED) continue;
            const int64_t e = ecc[comp[v]];
            if (e < 2 || dist[v] == (e + 1) / 2) dist[v] = -2; /* a clique-like leaf, or the separator */
        }
        for (int64_t v = 0; v < n; v++)
            if (level[v] == UNPLACED && dist[v] == -2) {
                level[v] = d;
                left--;
            }
        d++;
    }
    free(lab);
    free(nxt);
    free(best);
    free(comp);
    free(size);
    free(dist);
    free(ecc);
    graph_close(&g);
    return d;
}

/* c = the vertices sorted by (level descending, anc[v][level[v]] ascending, index ascending); node_root[v] = anc[v][level[v]];
 * nstart[k] = the position in c of the first vertex of the node of c[k], nsize[k] = that node's size.  Returns the number of nodes. */
int64_t model_lu_perm(int64_t n, int64_t rounds, const int64_t *level, const int64_t *anc, int64_t *c, int64_t *node_root,
                      int64_t *nstart, int64_t *nsize) {
    for (int64_t v = 0; v < n; v++) node_root[v] = anc[level[v] * n + v];
    int64_t k = 0, nodes = 0;
    for (int64_t d = rounds - 1; d >= 0; d--)
        for (int64_t r = 0; r < n; r++) { /* (a root names at most one node of depth d) */
            const int64_t k0 = k;
            for (int64_t v = 0; v < n; v++)
                if (level[v] == d && node_root[v] == r) c[k++] = v;
            for (int64_t t = k0; t < k; t++) {
                nstart[t] = k0;
                nsize[t] = k - k0;
            }
            nodes += k > k0;
        }
    return nodes;
}

/* The filled matrix.  pos = the inverse of c.  S[s * n + p] = 1: the vertex at position p belongs to struct of the node that starts
 * at position s.  count only (brv == NULL) or the arrays; returns nnz(B), or -(k + 1) when column k of B has no stored diagonal
 * in A. */
int64_t model_lu_fill(int64_t n, const int64_t *cp, const int64_t *rv, const double *nz, int64_t rounds, const int64_t *level,
                      const int64_t *anc, const int64_t *c, const int64_t *nstart, const int64_t *nsize, int64_t *bcp, int64_t *brv,
                      double *bnz) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    graph g;
    graph_open(&g, n, cp, rv);
    int64_t *pos = (int64_t *)malloc(8 * nn), *start_of = (int64_t *)malloc(8 * nn * (size_t)(rounds > 0 ? rounds : 1));
    uint8_t *S = (uint8_t *)calloc(nn * nn, 1);
    for (int64_t k = 0; k < n; k++) pos[c[k]] = k;
    for (int64_t k = 0; k < rounds * n; k++) start_of[k] = -1;
    for (int64_t v = 0; v < n; v++) start_of[level[v] * n + anc[level[v] * n + v]] = nstart[pos[v]]; /* the node (d, root) */
    for (int64_t u = 0; u < n; u++)
        for (int64_t t = 0, v; (v = slot(&g, u, t)) >= 0; t++) {
            if (!(level[v] < level[u])) continue; /* (another level: another node) */
            for (int64_t e = level[v] + 1; e <= level[u]; e++) {
                const int64_t s = start_of[e * n + anc[e * n + u]];
                if (s >= 0) S[s * n + pos[v]] = 1;
            }
        }
    int64_t q = 0, bad = 0;
    bcp[0] = 1;
    for (int64_t l = 0; l < n && !bad; l++) {
        const int64_t j = c[l];
        for (int64_t k = 0; k < n; k++) {
            int in;
            if (k < l) in = k >= nstart[l] || S[nstart[k] * n + l];  /* transpose(L): l is in column k of L */
            else in = k < nstart[l] + nsize[l] || S[nstart[l] * n + k]; /* L: the dense diagonal block, then struct */
            if (!in) continue;
            int64_t at = -1;
            for (int64_t p = cp[j] - 1; p < cp[j + 1] - 1; p++)
                if (rv[p] - 1 == c[k]) at = p;
            if (k == l && at < 0) bad = l + 1;
            if (brv) {
                brv[q] = k + 1;
                bnz[q] = 0.0;
                if (at >= 0) memcpy(&bnz[q], &nz[at], 8);
            }
            q++;
        }
        bcp[l + 1] = q + 1;
    }
    free(pos);
    free(start_of);
    free(S);
    graph_close(&g);
    return bad ? -bad : q;
}
