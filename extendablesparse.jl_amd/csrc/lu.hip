// lu.hip -- libesparse_hip: LUFactorization (esp_precon_lu_create), the sparse LU without pivoting behind `A \ b`, and the
// nested-dissection ordering it rests on (esp_nested_dissection)
// (see internal.hpp for the map of the translation units)
//
// The rule is stated in full in include/esparse_hip.h and DESIGN.md 5q; tests/lu_model.c restates it as plain loops and is normative.
// In short: the graph and key(i) are the colouring's (color.hip).  Round d = 0, 1, ... finds the connected components of the
// vertices not placed yet (root = the largest key), turns a small component into a leaf of depth d, and splits every other one by
// the middle level set of a breadth-first search from a far vertex: that separator is placed at depth d, the two sides go on.  c =
// the vertices sorted by (level descending, root of the node, index); the filled matrix B takes, per tree node K, a dense diagonal
// block and struct(K) = the ancestors' vertices next to K's subtree; the numerics are ILUAM's on B.
//
//   components   lu_label_k spreads the largest key over the unplaced vertices, every vertex at once from the previous launch's
//                labels (two arrays), until a launch changes nothing: as many launches as the farthest vertex is from its root, the
//                same from run to run.
//   searches     lu_bfs_k, level-synchronous over all components at once: an unplaced vertex without a distance that has a neighbour
//                at distance step - 1 takes distance step (the pull form: no frontier list, no order inside a level to keep).  A
//                vertex set during the launch holds `step`, never step - 1: one array serves.  Eccentricities and the far vertex
//                go through atomicMax on arrays indexed by the component's root vertex: no table of components exists.
//   both         one lane per vertex; a vertex whose column or row holds more than AMG_LONG entries is folded by its whole wave, 64
//                entries at a time (nbr_max), as color_round_k does.  A step is one launch on the handle's stream and one counter
//                read back; steps are separated by kernel boundaries and by nothing else.
//   permutation  a stable LSD sort of the vertices in index order on ((deepest - level) << bits(n) | root of the node): the radix
//                passes of the colouring's permutation.  Node starts by a max-scan of the head positions.
//   fill         anc[e][u] is rewritten to the start position of the node (e, anc[e][u]) through a table per depth; lu_pair_k emits
//                the records (row = position of v, column = start of the node) of the rule, an ESP_COO flush of a scratch handle
//                sorts them and folds the repeats: the pattern matrix S with struct(K) as column start(K).  T = transpose(S)
//                (esp_transpose) lists, per position k, the nodes whose struct holds k.  Column k of B is then written in ascending
//                order with no sort: the whole nodes of T's column k (rows of transpose(L)), the node of k itself (the rows before k
//                belong to transpose(L), from k on to L's dense block), struct of k's node.  lu_bcount_k counts, a scan makes the
//                column starts -- nnz(B) is known before B is allocated --, lu_bfill_k (one wave per column) writes the rows and
//                src[q], the position in A's nzval of A[c[row], c[k]] by bisection or ILUK_FILL.
//   the kind     update!, the value gather and the inner ILUAM are derived.hip's; ldiv! is block.hip's gather / inner ldiv! /
//                scatter over blk_new = the inverse of c (block_built holds for this kind).
//   panel form   esp_precon_lu_create_form(.., ESP_LU_PANELS, ..): build_b as above (B, src, the maps), then the tables and the two panels
//                per node of lu_panels.hip in the inner ILUAM's place; panels_update is derived_update's order of statements with
//                lup_numeric where the inner update! stood; ldiv! and esp_precon_get_factor branch on p->lup (block.hip, iluam.hip).
#include "lu.hpp"

using namespace espamg;
using namespace esplu;

namespace {

constexpr int LT = 256;                   // threads of every kernel here

__device__ __forceinline__ u64 lu_key(i64 i) { return ((u64)amg_mix(i) << 32) | (u64)(u32)i; }
__device__ __forceinline__ u64 lu_max(u64 a, u64 b) { return a > b ? a : b; }

// rp = csr_rowptr + 1: the entries of row i are [rp[i], rp[i+1]) of col
struct Graph {
    const i64 *colptr, *rowval;
    const u64 *rp;
    const u32 *col;
};

// the largest f(j) over the neighbour slots j of vertex i (column i of the CSC, then row i of the row-wise index: i itself and
// repeats are among them), 0 where there is none or the lane is not live.  Every lane of the wave calls it: a long vertex is folded
// by all of them.
template <typename F>
__device__ __forceinline__ u64 nbr_max(const Graph &g, bool live, i64 i, F f) {
    const int lane = threadIdx.x & 63;
    i64 s = 0, e = 0;
    u64 rs = 0, re = 0;
    if (live) {
        s = g.colptr[i] - 1;
        e = g.colptr[i + 1] - 1;
        rs = g.rp[i];
        re = g.rp[i + 1];
    }
    u64 m = 0;
    const bool longv = e - s > AMG_LONG || re - rs > (u64)AMG_LONG;
    if (!longv) {
        for (i64 k = s; k < e; k++) m = lu_max(m, f(g.rowval[k] - 1));
        for (u64 k = rs; k < re; k++) m = lu_max(m, f((i64)g.col[k]));
    }
    u64 mask = __ballot(longv);
    while (mask) {
        const int sl = __builtin_ctzll(mask);
        mask &= mask - 1;
        const i64 ls = __shfl(s, sl), le = __shfl(e, sl);
        const u64 lrs = __shfl(rs, sl), lre = __shfl(re, sl);
        u64 v = 0;
        for (i64 b = ls; b < le; b += 64) {
            const i64 k = b + lane;
            if (k < le) v = lu_max(v, f(g.rowval[k] - 1));
        }
        for (u64 b = lrs; b < lre; b += 64) {
            const u64 k = b + (u64)lane;
            if (k < lre) v = lu_max(v, f((i64)g.col[k]));
        }
        for (int o = 32; o > 0; o >>= 1) v = lu_max(v, (u64)__shfl_xor((unsigned long long)v, o));
        if (lane == sl) m = v;
    }
    return m;
}

// cnt[w] += the lanes of the wave with `yes` (one atomic per wave)
__device__ __forceinline__ void wave_count(u32 *cnt, int w, bool yes) {
    const u64 m = __ballot(yes);
    if (m && (int)(threadIdx.x & 63) == __builtin_ctzll(m)) atomicAdd(&cnt[w], (u32)__popcll(m));
}

// ---- the rounds ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LT) void lu_label_init_k(const u32 *__restrict__ level, i64 n, u64 *__restrict__ lab) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    if (v < n) lab[v] = level[v] == LU_NONE ? lu_key(v) : 0ull;
}
// out[v] = the largest of in[v] and in[j] over the unplaced neighbours j; cnt[0] = the labels that grew
__global__ __launch_bounds__(LT) void lu_label_k(Graph g, const u32 *__restrict__ level, const u64 *__restrict__ in, u64 *__restrict__ out, i64 n,
                                                 u32 *__restrict__ cnt) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    const bool live = v < n && level[v] == LU_NONE;
    const u64 m = nbr_max(g, live, v, [&](i64 j) { return level[j] == LU_NONE ? in[j] : 0ull; });
    bool grew = false;
    if (v < n) {
        const u64 own = in[v], nv = live ? lu_max(own, m) : own;
        out[v] = nv;
        grew = nv != own;
    }
    wave_count(cnt, 0, grew);
}
// anc[v] = the root of v's component (LU_NONE for a placed vertex), size[root] = the component's vertices
__global__ __launch_bounds__(LT) void lu_comp_k(const u32 *__restrict__ level, const u64 *__restrict__ lab, i64 n, u32 *__restrict__ anc,
                                                u32 *__restrict__ size) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    if (v >= n) return;
    if (level[v] != LU_NONE) {
        anc[v] = LU_NONE;
        return;
    }
    const u32 r = (u32)lab[v];
    anc[v] = r;
    atomicAdd(&size[r], 1u);
}
// a component of at most leaf_size vertices (or any, in the last round) is a leaf of depth d; every other one is searched from its
// root.  cnt[0] = the vertices placed, cnt[1] = the vertices of the components that go on.  (level: every lane reads its own entry)
__global__ __launch_bounds__(LT) void lu_seed_k(u32 *level, const u32 *__restrict__ anc, const u32 *__restrict__ size, i64 n, u32 d, u32 leaf_size,
                                                bool last, u32 *__restrict__ dist, u32 *__restrict__ ecc, u64 *__restrict__ best,
                                                u32 *__restrict__ cnt) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    const bool open = v < n && level[v] == LU_NONE;
    bool leaf = false;
    if (open) {
        const u32 r = anc[v];
        leaf = last || size[r] <= leaf_size;
        if (leaf) {
            level[v] = d;
        } else {
            dist[v] = (u32)v == r ? 0u : LU_NONE;
            if ((u32)v == r) {
                ecc[r] = 0u;
                best[r] = 0ull;
            }
        }
    }
    wave_count(cnt, 0, leaf);
    wave_count(cnt, 1, open && !leaf);
}
// one step of the searches.  dist is read and written by the same launch (see above): no __restrict__
__global__ __launch_bounds__(LT) void lu_bfs_k(Graph g, const u32 *__restrict__ level, const u32 *__restrict__ anc, u32 *dist, u32 *__restrict__ ecc,
                                               u32 step, i64 n, u32 *__restrict__ cnt) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    const bool live = v < n && level[v] == LU_NONE && dist[v] == LU_NONE;
    const u32 want = step - 1u;
    const u64 hit = nbr_max(g, live, v, [&](i64 j) { return level[j] == LU_NONE && dist[j] == want ? 1ull : 0ull; });
    const bool found = live && hit != 0;
    if (found) {
        dist[v] = step;
        atomicMax(&ecc[anc[v]], step);
    }
    wave_count(cnt, 0, found);
}
// best[root] = the largest key among the farthest vertices
__global__ __launch_bounds__(LT) void lu_far_k(const u32 *__restrict__ level, const u32 *__restrict__ anc, const u32 *__restrict__ dist,
                                               const u32 *__restrict__ ecc, u64 *__restrict__ best, i64 n) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    if (v >= n || level[v] != LU_NONE) return;
    const u32 r = anc[v];
    if (dist[v] == ecc[r]) atomicMax((unsigned long long *)&best[r], (unsigned long long)lu_key(v));
}
// the second search starts from that vertex
__global__ __launch_bounds__(LT) void lu_reseed_k(const u32 *__restrict__ level, const u32 *__restrict__ anc, const u64 *__restrict__ best,
                                                  u32 *__restrict__ dist, u32 *__restrict__ ecc, i64 n) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    if (v >= n || level[v] != LU_NONE) return;
    const u32 r = anc[v];
    dist[v] = lu_key(v) == best[r] ? 0u : LU_NONE;
    if ((u32)v == r) ecc[r] = 0u;
}
// ecc < 2: a clique-like leaf; else the vertices at distance (ecc + 1) / 2 are the separator.  cnt[0] = the vertices placed
__global__ __launch_bounds__(LT) void lu_split_k(u32 *level, const u32 *__restrict__ anc, const u32 *__restrict__ dist, const u32 *__restrict__ ecc,
                                                 i64 n, u32 d, u32 *__restrict__ cnt) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    bool placed = false;
    if (v < n && level[v] == LU_NONE) {
        const u32 e = ecc[anc[v]];
        placed = e < 2u || dist[v] == (e + 1u) / 2u;
        if (placed) level[v] = d;
    }
    wave_count(cnt, 0, placed);
}

// ---- the permutation and the nodes -----------------------------------------------------------------------------------------------
// root[v] = anc[level[v]][v]; the sort key (deepest - level[v]) << nb | root[v], the payload v
__global__ __launch_bounds__(LT) void lu_keys_k(const u32 *__restrict__ level, const u32 *const *__restrict__ anc, i64 n, u32 deepest, int nb,
                                                u32 *__restrict__ root, u64 *__restrict__ key, double *__restrict__ payload) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    if (v >= n) return;
    const u32 l = min(level[v], deepest), r = anc[l][v];  // (every vertex was placed: the bound keeps a broken count from reading astray)
    root[v] = r;
    key[v] = ((((u64)(deepest - l)) << nb) | (u64)r) << ESP_TAG_BITS;
    payload[v] = __longlong_as_double((long long)v);
}
// c[k] = the k-th vertex of the sorted order, new(c[k]) = k; head[k] = k where a node starts at k (its key differs from the one
// before), else 0
__global__ __launch_bounds__(LT) void lu_maps_k(const u64 *__restrict__ skey, const double *__restrict__ spayload, i64 n, u32 *__restrict__ perm,
                                                u32 *__restrict__ newpos, u32 *__restrict__ head) {
    const i64 k = (i64)blockIdx.x * LT + threadIdx.x;
    if (k >= n) return;
    const u32 i = (u32)__double_as_longlong(spayload[k]);
    perm[k] = i;
    newpos[i] = (u32)k;
    head[k] = k > 0 && skey[k] != skey[k - 1] ? (u32)k : 0u;
}
// before[k] = the largest head below k (the exclusive max-scan of head): nstart[k] = the start of k's node, nsize[start] = its size
// (zeroed before), st[0] = the nodes
__global__ __launch_bounds__(LT) void lu_nodes_k(const u64 *__restrict__ skey, const u32 *__restrict__ before, i64 n, u32 *__restrict__ nstart,
                                                 u32 *__restrict__ nsize, unsigned long long *__restrict__ st) {
    const i64 k = (i64)blockIdx.x * LT + threadIdx.x;
    if (k >= n) return;
    const bool head = k == 0 || skey[k] != skey[k - 1];
    const u32 s = head ? (u32)k : before[k];
    nstart[k] = s;
    atomicAdd(&nsize[s], 1u);
    if (head) atomicAdd(&st[0], 1ull);
}
// tab[root] = the start of the node (e, root), from any of its vertices
__global__ __launch_bounds__(LT) void lu_tab_k(const u32 *__restrict__ level, const u32 *__restrict__ root, const u32 *__restrict__ newpos,
                                               const u32 *__restrict__ nstart, i64 n, u32 e, u32 *__restrict__ tab) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    if (v < n && level[v] == e) tab[root[v]] = nstart[newpos[v]];
}
// anc[v]: the root of v's component at depth e -> the start of the node (e, that root)
__global__ __launch_bounds__(LT) void lu_anc_k(const u32 *__restrict__ level, const u32 *__restrict__ tab, i64 n, u32 e, u32 *__restrict__ anc) {
    const i64 v = (i64)blockIdx.x * LT + threadIdx.x;
    if (v < n && level[v] >= e) anc[v] = tab[anc[v]];
}

// ---- the fill ----------------------------------------------------------------------------------------------------------------------
// an edge (u, v) with level[v] < level[u]: the position of v belongs to struct of the node of u's ancestor at every depth e with
// level[v] < e <= level[u].  Count (FILL = false): cnt[u] = the records of u; fill: the ESP_COO records behind off[u].  One lane per
// vertex, the column and then the row in stored order: both passes meet the same slots
template <bool FILL>
__global__ __launch_bounds__(LT) void lu_pair_k(Graph g, const u32 *__restrict__ level, const u32 *const *__restrict__ anc,
                                                const u32 *__restrict__ newpos, i64 n, i64 *__restrict__ cnt, const i64 *__restrict__ off,
                                                u64 *__restrict__ keys, u64 *__restrict__ vals, KeyLayout L, unsigned long long *__restrict__ err) {
    const i64 u = (i64)blockIdx.x * LT + threadIdx.x;
    if (u >= n) return;
    const u32 lu = level[u];
    i64 q = FILL ? off[u] : 0;
    const i64 qend = FILL ? off[u + 1] : 0;
    auto slot = [&](i64 v) {
        const u32 lv = level[v];
        if (!(lv < lu)) return;
        if (!FILL) {
            q += (i64)(lu - lv);
            return;
        }
        const i64 row = (i64)newpos[v];
        for (u32 e = lv + 1u; e <= lu; e++) {
            const u32 s = anc[e][u];
            if (s == LU_NONE || q >= qend) {  // (no node at an ancestor's depth, or the passes disagree: reported, nothing stray written)
                atomicMax(err, 1ull);
                return;
            }
            keys[q] = esp_pack(L, row + 1, (i64)s + 1, ESP_COO);
            vals[q] = 0x3FF0000000000000ull;  // (1.0: repeats fold to a sum that is never zero)
            q++;
        }
    };
    for (i64 k = g.colptr[u] - 1; k < g.colptr[u + 1] - 1; k++) slot(g.rowval[k] - 1);
    for (u64 k = g.rp[u]; k < g.rp[u + 1]; k++) slot((i64)g.col[k]);
    if (!FILL) cnt[u] = q;
    else if (q != qend) atomicMax(err, 1ull);
}

// cp[k] = the entries of column k of B; st[1] = the largest node
__global__ __launch_bounds__(LT) void lu_bcount_k(Struct x, const u32 *__restrict__ nstart, const u32 *__restrict__ nsize, i64 n, i64 *__restrict__ cp,
                                                  unsigned long long *__restrict__ st) {
    const i64 k = (i64)blockIdx.x * LT + threadIdx.x;
    u32 big = 0;
    if (k < n) {
        const i64 s = (i64)nstart[k];
        i64 c = (i64)nsize[s];
        if (s == k) big = nsize[s];
        if (x.scp) {
            c += x.scp[s + 1] - x.scp[s];
            for (i64 q = x.tcp[k] - 1; q < x.tcp[k + 1] - 1; q++) c += (i64)nsize[x.trv[q] - 1];
        }
        cp[k] = c;
    }
    const u32 m = esp_wave_max(big);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&st[1], (unsigned long long)m);
}
// one wave per column k of B (cp: the 0-based starts): the rows ascending, src[q] = the position in A of A[c[row], c[k]] or ILUK_FILL;
// st[2] = the smallest column whose diagonal A does not store, st[3] = 1 when a column does not end where the count said
__global__ __launch_bounds__(LT) void lu_bfill_k(Struct x, espfold::Csc A, const u32 *__restrict__ perm, const u32 *__restrict__ nstart,
                                                 const u32 *__restrict__ nsize, i64 n, const i64 *__restrict__ cp, i64 *__restrict__ rowB,
                                                 u32 *__restrict__ src, unsigned long long *__restrict__ st) {
    const i64 k = (i64)blockIdx.x * (LT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (k >= n) return;
    const i64 j = (i64)perm[k], end = cp[k + 1];
    i64 q = cp[k];
    auto put = [&](i64 at, i64 row) {  // (at < end: the count pass walked the same lists)
        if (at >= end) return;
        const i64 pos = A.nnz > 0 ? espfold::csc_find(A, j, (i64)perm[row]) : -1;
        rowB[at] = row + 1;
        src[at] = pos >= 0 ? (u32)pos : ILUK_FILL;
        if (row == k && pos < 0) atomicMin(&st[2], (unsigned long long)k);
    };
    if (x.scp)
        for (i64 t = x.tcp[k] - 1; t < x.tcp[k + 1] - 1; t++) {  // the nodes whose struct holds k: their columns of L hold row k
            const i64 s = x.trv[t] - 1, m = (i64)nsize[s];
            for (i64 r = lane; r < m; r += 64) put(q + r, s + r);
            q += m;
        }
    const i64 s = (i64)nstart[k], m = (i64)nsize[s];
    for (i64 r = lane; r < m; r += 64) put(q + r, s + r);  // k's own node: the rows before k of transpose(L), the dense block of L
    q += m;
    if (x.scp) {
        const i64 b = x.scp[s] - 1, len = x.scp[s + 1] - 1 - b;
        for (i64 r = lane; r < len; r += 64) put(q + r, x.srv[b + r] - 1);  // struct of k's node
        q += len;
    }
    if (lane == 0 && q != end) atomicMax(&st[3], 1ull);
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
Graph graph_of(const esp_handle *h) {
    return Graph{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (const u64 *)h->csr_rowptr.p + 1, (const u32 *)h->csr_col.p};
}

// the words of a zeroed counter after the launches in front of it
int32_t read_cnt(esp_handle *h, const DevBuf &cnt, u32 out[2]) {
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, cnt.p, sizeof(u32) * 2, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    out[0] = ((const u32 *)h->pin_scalar)[0];
    out[1] = ((const u32 *)h->pin_scalar)[1];
    return ESP_OK;
}

}  // namespace

// the rounds of h's stored pattern (checked, square, flushed): o.level, o.anc, o.rounds, o.launches
int32_t lu_dissect(esp_handle *h, int leaf_size, int max_depth, Order &o) {
    hipStream_t s = h->stream;
    const i64 n = h->n;
    CK(ensure(h, o.level, sizeof(u32) * (size_t)std::max<i64>(n, 1)));
    if (n == 0) return ESP_OK;
    CK(csr_current(h));
    const Graph g = graph_of(h);
    Temps tmp;
    DevBuf &la = tmp.b[0], &lb = tmp.b[1], &size = tmp.b[2], &dist = tmp.b[3], &ecc = tmp.b[4], &best = tmp.b[5], &cnt = tmp.b[6];
    for (DevBuf *b : {&la, &lb, &best}) CK(ensure(h, *b, sizeof(u64) * (size_t)n));
    for (DevBuf *b : {&size, &dist, &ecc}) CK(ensure(h, *b, sizeof(u32) * (size_t)n));
    CK(ensure(h, cnt, sizeof(u32) * 2));
    HIPCK(h, hipMemsetAsync(o.level.p, 0xFF, sizeof(u32) * (size_t)n, s));
    u32 *level = (u32 *)o.level.p;
    const unsigned grid = grid_for(n, LT);
    i64 left = n;
    u32 got[2];
    // the searches of every component, from the sources lu_seed_k / lu_reseed_k left
    auto search = [&](const u32 *anc) -> int32_t {
        for (i64 step = 1;; step++) {
            if (step > n) FAIL(h, ESP_ERR_HIP, "esp_nested_dissection: a search did not end after %lld steps", (long long)n);
            HIPCK(h, hipMemsetAsync(cnt.p, 0, sizeof(u32) * 2, s));
            hipLaunchKernelGGL(lu_bfs_k, dim3(grid), dim3(LT), 0, s, g, (const u32 *)level, anc, (u32 *)dist.p, (u32 *)ecc.p, (u32)step, n,
                               (u32 *)cnt.p);
            o.launches++;
            CK(read_cnt(h, cnt, got));
            if (got[0] == 0) return ESP_OK;
        }
    };
    for (int d = 0; left > 0; d++) {
        if (d > max_depth) FAIL(h, ESP_ERR_HIP, "esp_nested_dissection: %lld vertices left behind depth %d", (long long)left, max_depth);
        o.anc.emplace_back();
        CK(ensure(h, o.anc.back(), sizeof(u32) * (size_t)n));
        u32 *anc = (u32 *)o.anc.back().p;
        u64 *in = (u64 *)la.p, *out = (u64 *)lb.p;
        hipLaunchKernelGGL(lu_label_init_k, dim3(grid), dim3(LT), 0, s, (const u32 *)level, n, in);
        for (i64 it = 0;; it++) {  // (the largest key of a component reaches its farthest vertex after at most n - 1 launches)
            if (it > n) FAIL(h, ESP_ERR_HIP, "esp_nested_dissection: the components did not settle after %lld launches", (long long)n);
            HIPCK(h, hipMemsetAsync(cnt.p, 0, sizeof(u32) * 2, s));
            hipLaunchKernelGGL(lu_label_k, dim3(grid), dim3(LT), 0, s, g, (const u32 *)level, (const u64 *)in, out, n, (u32 *)cnt.p);
            o.launches++;
            CK(read_cnt(h, cnt, got));
            std::swap(in, out);
            if (got[0] == 0) break;
        }
        HIPCK(h, hipMemsetAsync(size.p, 0, sizeof(u32) * (size_t)n, s));
        hipLaunchKernelGGL(lu_comp_k, dim3(grid), dim3(LT), 0, s, (const u32 *)level, (const u64 *)in, n, anc, (u32 *)size.p);
        HIPCK(h, hipMemsetAsync(cnt.p, 0, sizeof(u32) * 2, s));
        hipLaunchKernelGGL(lu_seed_k, dim3(grid), dim3(LT), 0, s, level, (const u32 *)anc, (const u32 *)size.p, n, (u32)d, (u32)leaf_size,
                           d == max_depth, (u32 *)dist.p, (u32 *)ecc.p, (u64 *)best.p, (u32 *)cnt.p);
        CK(read_cnt(h, cnt, got));
        left -= (i64)got[0];
        if ((i64)got[1] != left) FAIL(h, ESP_ERR_HIP, "esp_nested_dissection: round %d lost count of its vertices", d);
        if (got[1] > 0) {
            CK(search(anc));
            hipLaunchKernelGGL(lu_far_k, dim3(grid), dim3(LT), 0, s, (const u32 *)level, (const u32 *)anc, (const u32 *)dist.p, (const u32 *)ecc.p,
                               (u64 *)best.p, n);
            hipLaunchKernelGGL(lu_reseed_k, dim3(grid), dim3(LT), 0, s, (const u32 *)level, (const u32 *)anc, (const u64 *)best.p, (u32 *)dist.p,
                               (u32 *)ecc.p, n);
            CK(search(anc));
            HIPCK(h, hipMemsetAsync(cnt.p, 0, sizeof(u32) * 2, s));
            hipLaunchKernelGGL(lu_split_k, dim3(grid), dim3(LT), 0, s, level, (const u32 *)anc, (const u32 *)dist.p, (const u32 *)ecc.p, n, (u32)d,
                               (u32 *)cnt.p);
            CK(read_cnt(h, cnt, got));
            if (got[0] == 0 || (i64)got[0] > left) FAIL(h, ESP_ERR_HIP, "esp_nested_dissection: round %d placed %u of %lld vertices", d, got[0], (long long)left);
            left -= (i64)got[0];
        }
        o.rounds = d + 1;
    }
    o.deepest = o.rounds - 1;  // (the last round placed something, at its own depth)
    return ESP_OK;
}

// o.perm = the vertices sorted by (level descending, root of the node, index), o.newpos its inverse, o.root, the nodes
int32_t lu_order(esp_handle *h, Order &o) {
    hipStream_t s = h->stream;
    const i64 n = h->n;
    for (DevBuf *b : {&o.root, &o.perm, &o.newpos, &o.nstart, &o.nsize}) CK(ensure(h, *b, sizeof(u32) * (size_t)std::max<i64>(n, 1)));
    if (n == 0) return ESP_OK;
    std::vector<const u32 *> ptrs;
    for (const DevBuf &b : o.anc) ptrs.push_back((const u32 *)b.p);
    CK(ensure(h, o.ancptr, sizeof(u32 *) * ptrs.size()));
    HIPCK(h, hipMemcpyAsync(o.ancptr.p, ptrs.data(), sizeof(u32 *) * ptrs.size(), hipMemcpyHostToDevice, s));
    HIPCK(h, hipStreamSynchronize(s));  // (ptrs is free from here)
    Temps tmp;
    DevBuf &sortb = tmp.b[0], &head = tmp.b[1], &ws = tmp.b[2], &st = tmp.b[3];
    CK(ensure(h, sortb, (size_t)n * 4 * 8));
    CK(ensure(h, head, sizeof(u32) * (size_t)n));
    CK(ensure(h, st, sizeof(u64)));
    const PingPong d = carve_pingpong(sortb.p, n);
    const unsigned g = grid_for(n, LT);
    int nb = 1, db = 1;
    while (((i64)1 << nb) < n) nb++;
    while (((i64)1 << db) < o.rounds) db++;
    hipLaunchKernelGGL(lu_keys_k, dim3(g), dim3(LT), 0, s, (const u32 *)o.level.p, (const u32 *const *)o.ancptr.p, n, (u32)o.deepest, nb,
                       (u32 *)o.root.p, d.k[0], d.v[0]);
    SortPair r;
    CK(sort_segment_lsd(h, d.half(0), d, n, 0, nb + db, 62, &r));
    hipLaunchKernelGGL(lu_maps_k, dim3(g), dim3(LT), 0, s, r.k, r.v, n, (u32 *)o.perm.p, (u32 *)o.newpos.p, (u32 *)head.p);
    int l = 0;
    CK(scan_inplace<u32, true>(h, (u32 *)head.p, n, ws, &l));
    HIPCK(h, hipMemsetAsync(o.nsize.p, 0, sizeof(u32) * (size_t)n, s));
    HIPCK(h, hipMemsetAsync(st.p, 0, sizeof(u64), s));
    hipLaunchKernelGGL(lu_nodes_k, dim3(g), dim3(LT), 0, s, r.k, (const u32 *)head.p, n, (u32 *)o.nstart.p, (u32 *)o.nsize.p,
                       (unsigned long long *)st.p);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, st.p, sizeof(u64), hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    o.nodes = (i64)h->pin_scalar[0];
    return ESP_OK;
}

// n values of a u32 device array into the caller's host or device array: as int64 (wide) or as they are (int32)
int32_t lu_export(esp_handle *h, const DevBuf &src, void *out, bool wide, int32_t on_device) {
    if (wide) return export_u32_as_i64(h, src.p, h->n, 0u, (int64_t *)out, on_device);
    return copy_out(h, out, src.p, sizeof(u32) * (size_t)h->n, on_device);
}

// the struct lists of the ordered tree (n > 0): anc as node starts, the records of the rule, S by an ESP_COO flush, T its transpose
int32_t lu_structs(esp_handle *h, Order &o, const char *what, Handles &hs, Struct &x) {
    hipStream_t s = h->stream;
    const i64 n = h->n;
    x = Struct{nullptr, nullptr, nullptr, nullptr};
    if (n == 0) return ESP_OK;
    Temps tmp;
    DevBuf &st = tmp.b[0], &ws = tmp.b[1], &tab = tmp.b[2], &off = tmp.b[3], &scp = tmp.b[4], &srv = tmp.b[5], &snz = tmp.b[6];
    CK(ensure(h, st, sizeof(u64)));
    HIPCK(h, hipMemsetAsync(st.p, 0, sizeof(u64), s));
    unsigned long long *stp = (unsigned long long *)st.p;  // a record or node error
    const unsigned g = grid_for(n, LT);
    int l = 0;
    // the ancestors as node starts
    CK(ensure(h, tab, sizeof(u32) * (size_t)n));
    for (i64 e = 0; e < o.rounds; e++) {
        HIPCK(h, hipMemsetAsync(tab.p, 0xFF, sizeof(u32) * (size_t)n, s));
        hipLaunchKernelGGL(lu_tab_k, dim3(g), dim3(LT), 0, s, (const u32 *)o.level.p, (const u32 *)o.root.p, (const u32 *)o.newpos.p,
                           (const u32 *)o.nstart.p, n, (u32)e, (u32 *)tab.p);
        hipLaunchKernelGGL(lu_anc_k, dim3(g), dim3(LT), 0, s, (const u32 *)o.level.p, (const u32 *)tab.p, n, (u32)e, (u32 *)o.anc[(size_t)e].p);
    }
    // the records of struct
    const Graph gr = graph_of(h);
    CK(ensure(h, off, sizeof(i64) * (size_t)(n + 1)));
    HIPCK(h, hipMemsetAsync(off.p, 0, sizeof(i64) * (size_t)(n + 1), s));
    hipLaunchKernelGGL(lu_pair_k<false>, dim3(g), dim3(LT), 0, s, gr, (const u32 *)o.level.p, (const u32 *const *)o.ancptr.p,
                       (const u32 *)o.newpos.p, n, (i64 *)off.p, (const i64 *)nullptr, (u64 *)nullptr, (u64 *)nullptr, h->L, stp);
    CK(scan_inplace<i64, false>(h, (i64 *)off.p, n + 1, ws, &l));
    HIPCK(h, hipGetLastError());
    i64 npairs = 0;
    CK(read_i64(h, (const i64 *)off.p + n, &npairs));
    if (npairs == 0) return ESP_OK;
    ScratchFlush sf(h, what);
    CK(sf.open(n, n, npairs));
    hipLaunchKernelGGL(lu_pair_k<true>, dim3(g), dim3(LT), 0, s, gr, (const u32 *)o.level.p, (const u32 *const *)o.ancptr.p,
                       (const u32 *)o.newpos.p, n, (i64 *)nullptr, (const i64 *)off.p, sf.keys(), sf.vals(), sf.L(), stp);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, stp, sizeof(u64), hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    if (h->pin_scalar[0] != 0) FAIL(h, ESP_ERR_HIP, "%s: the record pass of struct disagrees with its count pass", what);
    CK(sf.flush(-1));
    const i64 nnzS = sf.nnz();
    sf.take(scp, srv, snz);
    hs.v.assign(2, nullptr);
    for (esp_handle *&q : hs.v) CK(amg_make_handle(h, n, n, &q));
    install(hs.v[0], scp, srv, snz, nnzS);
    const int32_t ts = esp_transpose(hs.v[0], hs.v[1], nullptr);
    if (ts != ESP_OK) FAIL(h, ts, "%s: transpose of the struct lists: %s", what, hs.v[1]->err.c_str());
    x = Struct{(const i64 *)hs.v[0]->colptr.p, (const i64 *)hs.v[0]->rowval.p, (const i64 *)hs.v[1]->colptr.p,
               (const i64 *)hs.v[1]->rowval.p};
    return ESP_OK;
}

namespace {

// derived_update's builder: the ordering, the tree and B from A's current CSC; B installed in p->der.bh, src in p->der.src, the maps
// in p.  Everything that can fail comes in front of that: nothing of p changes when it fails
int32_t build_b(esp_precon *p) {
    esp_handle *h = p->h;
    hipStream_t s = h->stream;
    const i64 n = p->n;
    CK(ensure(h, p->blk_t, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    CK(ensure(h, p->blk_s, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    Order o;
    CK(lu_dissect(h, p->lu_leaf, p->lu_depth, o));
    CK(lu_order(h, o));
    Temps tmp;
    DevBuf &cp = tmp.b[0], &rv = tmp.b[1], &nz = tmp.b[2], &src = tmp.b[3], &st = tmp.b[4], &ws = tmp.b[5];
    Handles hs;  // S and transpose(S)
    CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, st, sizeof(u64) * 4));
    HIPCK(h, hipMemsetAsync(cp.p, 0, sizeof(i64) * (size_t)(n + 1), s));
    hipLaunchKernelGGL(set_i64_k, dim3(1), dim3(1), 0, s, (i64 *)st.p, (i64)0, (i64)0, (i64)-1, (i64)0);
    unsigned long long *stp = (unsigned long long *)st.p;  // 0: spare, 1: the largest node, 2: smallest column without a
                                                            // stored diagonal, 3: count and fill of B disagree
    const unsigned g = grid_for(n, LT);
    Struct x{nullptr, nullptr, nullptr, nullptr};
    int l = 0;
    if (n > 0) {
        CK(lu_structs(h, o, "esp_precon_lu", hs, x));
        hipLaunchKernelGGL(lu_bcount_k, dim3(g), dim3(LT), 0, s, x, (const u32 *)o.nstart.p, (const u32 *)o.nsize.p, n, (i64 *)cp.p, stp);
        CK(scan_inplace<i64, false>(h, (i64 *)cp.p, n + 1, ws, &l));
    }
    HIPCK(h, hipGetLastError());
    i64 nnzB = 0;
    CK(read_i64(h, (const i64 *)cp.p + n, &nnzB));
    if (nnzB < n) FAIL(h, ESP_ERR_HIP, "esp_precon_lu: %lld entries of B for %lld columns", (long long)nnzB, (long long)n);
    const i64 cap = h->debug_lu_cap > 0 ? h->debug_lu_cap : 0xFFFFFFF0ll;
    if (nnzB >= cap)
        FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_lu: the factors fill the matrix to %lld entries (the preconditioners' index holds 32-bit positions%s)",
             (long long)nnzB, h->debug_lu_cap > 0 ? "; esp_debug_lu_fill_cap lowered the limit" : "");
    CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(nnzB, 1)));
    CK(ensure(h, src, sizeof(u32) * (size_t)std::max<i64>(nnzB, 1)));
    CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nnzB, 1)));
    i64 largest = 0;
    if (n > 0) {
        const espfold::Csc A{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (double *)h->nzval.p, h->nnz};
        hipLaunchKernelGGL(lu_bfill_k, dim3(grid_for(n, LT / 64)), dim3(LT), 0, s, x, A, (const u32 *)o.perm.p, (const u32 *)o.nstart.p,
                           (const u32 *)o.nsize.p, n, (const i64 *)cp.p, (i64 *)rv.p, (u32 *)src.p, stp);
        add_one_launch(s, (i64 *)cp.p, n + 1);
        derived_gather_launch(s, nullptr, (u32 *)src.p, nullptr, (const u64 *)h->nzval.p, (u64 *)nz.p, nnzB, nullptr);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, stp + 1, sizeof(u64) * 3, hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        largest = (i64)h->pin_scalar[0];
        const unsigned long long missing = h->pin_scalar[1];
        if (h->pin_scalar[2] != 0) FAIL(h, ESP_ERR_HIP, "esp_precon_lu: the fill pass of B disagrees with its count pass");
        if (missing != ~0ull) {
            HIPCK(h, hipMemcpyAsync(h->pin_scalar, (const u32 *)o.perm.p + missing, sizeof(u32), hipMemcpyDeviceToHost, s));
            HIPCK(h, hipStreamSynchronize(s));
            FAIL(h, ESP_ERR_INVALID,
                 "esp_precon_lu: iluam: column %llu has no stored diagonal entry (a column of B: the position in c; A's column is %llu)",
                 missing + 1, (unsigned long long)*(const u32 *)h->pin_scalar + 1);
        }
    } else {
        add_one_launch(s, (i64 *)cp.p, 1);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipStreamSynchronize(s));
    }
    LuPanelData *lp = nullptr;
    if (p->lu_form == ESP_LU_PANELS) CK(lup_symbolic(p, o, hs, x, &lp));  // (the last thing that can fail)
    lup_drop(p->lup);
    p->lup = lp;
    install(p->der.bh, cp, rv, nz, nnzB);
    std::swap(p->der.src, src);
    std::swap(p->blk_new, o.newpos);
    std::swap(p->lu_perm, o.perm);
    std::swap(p->lu_level, o.level);
    std::swap(p->lu_root, o.root);
    p->blk_path = n > 0 ? 1 : 0;
    p->lu_stats[0] = nnzB;
    p->lu_stats[1] = o.rounds;
    p->lu_stats[2] = o.deepest;
    p->lu_stats[3] = o.nodes;
    p->lu_stats[4] += o.launches;
    p->lu_stats[5] = largest;
    return ESP_OK;
}

int32_t lu_current(esp_precon *p, const char *what) {
    esp_handle *h = p->h;
    if (h->pattern_version != p->pattern_version || h->nnz != p->nnz)
        FAIL(h, ESP_ERR_STATE, "%s: the matrix pattern changed since the factorization's last update!", what);
    return ESP_OK;
}

}  // namespace

int32_t lu_check_args(esp_handle *h, const char *what, int32_t leaf_size, int32_t max_depth) {
    if (leaf_size < 1) FAIL(h, ESP_ERR_INVALID, "%s: leaf_size = %d < 1", what, leaf_size);
    if (max_depth < 0 || max_depth > 64) FAIL(h, ESP_ERR_INVALID, "%s: max_depth = %d is outside 0..64", what, max_depth);
    CK(precon_check_handle(h, what));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "%s: a column window / column shard", what);
    return ESP_OK;
}

// the panel form's update!: derived_update's order of statements with the numeric factorization on the panels in the inner
// preconditioner's place (no inner object, no level analysis, no schedules)
static int32_t panels_update(esp_precon *p) {
    esp_handle *h = p->h, *bh = p->der.bh;
    CK(precon_check_handle(h, "esp_precon_update"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_lu: a column window / column shard");
    CK(derived_follow_stream(p));
    if (derived_stale(p)) {
        CK(build_b(p));
        p->pattern_version = 0;
        p->der.rebuild = false;
    } else {
        p->pattern_version = 0;
        if (bh->nnz > 0)
            derived_gather_launch(h->stream, nullptr, (u32 *)p->der.src.p, nullptr, (const u64 *)h->nzval.p, (u64 *)bh->nzval.p, bh->nnz, nullptr);
        HIPCK(h, hipGetLastError());
        bh->values_version++;
    }
    CK(lup_numeric(p));
    HIPCK(h, hipStreamSynchronize(h->stream));
    p->nnz = h->nnz;
    p->pattern_version = h->pattern_version;
    p->values_version = h->values_version;
    return ESP_OK;
}

int32_t lu_update(esp_precon *p) { return p->lu_form == ESP_LU_PANELS ? panels_update(p) : derived_update(p, "esp_precon_lu", build_b, ""); }

void lu_release(esp_precon *p) {
    lup_drop(p->lup);
    p->lup = nullptr;
    for (DevBuf *b : {&p->lu_perm, &p->lu_level, &p->lu_root}) release(*b);
}

extern "C" int32_t esp_nested_dissection(esp_handle *h, int32_t leaf_size, int32_t max_depth, int64_t *c, int32_t *level, int32_t on_device) {
    if (!h) return ESP_ERR_INVALID;
    CK(lu_check_args(h, "esp_nested_dissection", leaf_size, max_depth));
    Order o;
    int32_t st = lu_dissect(h, leaf_size, max_depth, o);
    if (st == ESP_OK) st = lu_order(h, o);
    if (st == ESP_OK && c) st = lu_export(h, o.perm, c, true, on_device);
    if (st == ESP_OK && level) st = lu_export(h, o.level, level, false, on_device);
    (void)hipStreamSynchronize(h->stream);
    return st;
}

extern "C" int32_t esp_precon_lu_create(esp_handle *h, int32_t leaf_size, int32_t max_depth, esp_precon **out) {
    return esp_precon_lu_create_form(h, leaf_size, max_depth, ESP_LU_COLUMNS, out);
}

extern "C" int32_t esp_precon_lu_create_form(esp_handle *h, int32_t leaf_size, int32_t max_depth, int32_t form, esp_precon **out) {
    if (!h || !out) return ESP_ERR_INVALID;
    *out = nullptr;
    if (form != ESP_LU_COLUMNS && form != ESP_LU_PANELS) return ESP_ERR_INVALID;
    CK(lu_check_args(h, "esp_precon_lu_create", leaf_size, max_depth));
    esp_precon *p = precon_new(h, ESP_PRECON_LU);
    p->der.inner_kind = ESP_PRECON_ILUAM;
    p->lu_form = form;
    p->lu_leaf = leaf_size;
    p->lu_depth = max_depth;
    p->der.rebuild = true;
    const int32_t st = [&]() -> int32_t {
        const int32_t cs = esp_create(h->n, h->n, h->device, 0, &p->der.bh);
        if (cs != ESP_OK) FAIL(h, cs, "esp_precon_lu_create: the handle of B: %s", esp_last_error(nullptr));
        return lu_update(p);
    }();
    return precon_finish(p, st, out);
}

extern "C" int32_t esp_precon_lu_perm(esp_precon *p, int64_t *c, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_LU || !c) return ESP_ERR_INVALID;
    CK(lu_current(p, "esp_precon_lu_perm"));
    return lu_export(p->h, p->lu_perm, c, true, on_device);
}

extern "C" int32_t esp_precon_lu_tree(esp_precon *p, int32_t *level, int64_t *node_root, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_LU) return ESP_ERR_INVALID;
    CK(lu_current(p, "esp_precon_lu_tree"));
    if (level) CK(lu_export(p->h, p->lu_level, level, false, on_device));
    if (node_root) CK(lu_export(p->h, p->lu_root, node_root, true, on_device));
    return ESP_OK;
}

extern "C" int32_t esp_precon_lu_matrix(esp_precon *p, esp_handle **b) {
    if (!p || p->kind != ESP_PRECON_LU) return ESP_ERR_INVALID;
    if (b) *b = p->der.bh;
    return ESP_OK;
}

extern "C" int32_t esp_precon_lu_stats(esp_precon *p, int64_t out[6]) {
    if (!p || p->kind != ESP_PRECON_LU || !out) return ESP_ERR_INVALID;
    for (int k = 0; k < 6; k++) out[k] = p->lu_stats[k];
    return ESP_OK;
}

extern "C" int32_t esp_debug_lu_fill_cap(esp_handle *h, int64_t cap) {
    if (!h || cap < 0) return ESP_ERR_INVALID;
    h->debug_lu_cap = cap;
    return ESP_OK;
}
