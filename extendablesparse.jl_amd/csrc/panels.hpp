// panels.hpp -- what the two factorizations on dense panels per tree node share: cholesky.hip (CholeskyFactorization) and
// lu_panels.hip (LUFactorization's panel form).  The node table, the update lists and the depth schedule (host side,
// from lu.hip's ordering and struct lists), struct_find, the gather and scatter of v[c], upload and download.  Nothing here knows what
// a panel holds: a node K (width w, h = |struct(K)|) owns (w + h) x w column-major doubles at `off`.
#pragma once
#include "lu.hpp"

struct CholNode {
    i64 off;      // the panel's first double
    i64 sbase;    // struct(K) = srv[sbase .. sbase + h) (1-based positions, ascending)
    u32 w, h, start, depth;
    u32 ub, ue;   // the update list: ulist[ub .. ue)
};

struct CholLaunch {  // one block column of the wide nodes of a depth: dlist[first .. first + count), tiles per node
    u32 first, count, bc, tiles_u, tiles_f;
};
struct CholDepth {
    u32 all_first = 0, all_count = 0;      // dlist: every node of the depth (the solves)
    u32 small_first = 0, small_count = 0;  // flist: the small nodes, then the wide ones by block columns descending
    std::vector<CholLaunch> wide;
};

// the tables of an ordered tree, on the host (depth) and on the device
struct PanelTree {
    esp_handle *S = nullptr;  // the struct lists (column start(K) = struct(K)); nullptr when no node has one
    DevBuf nodes, ulist, dlist, flist, nodeof;
    std::vector<CholDepth> depth;
    std::vector<CholNode> host_nodes;  // (read by the builders while they size what lies behind the tables; cleared afterwards)
    i64 nnodes = 0, panel_doubles = 0, nnzL = 0, largest = 0, nsmall = 0, nwide = 0, nbcols = 0;
};

namespace esppanel {

using namespace esplu;

constexpr int CT = 256;       // threads of every kernel of the panel forms
constexpr int NB = 32;        // columns of a block column = of the update tile = the factor block width = W_small
constexpr int TR = 64;        // rows of the update tile
constexpr int KB = 16;        // columns of a descendant staged at once
constexpr int FR = 128;       // rows below the diagonal block a workgroup divides at once (one per lane of its first two waves)
constexpr int TRI_LDS = 1024; // rows of a node's triangle the solves keep in LDS
// the solves of several right-hand sides: RC columns share one pass over the panels.  8 = ESP_MANY_CHUNK fills a
// workgroup with 32 rows x 8 columns, which is exactly a leaf of leaf_size 32 (the default), and the 8 lanes of a row read one
// 64-byte line of the work vector
constexpr int RC = ESP_MANY_CHUNK;
constexpr int RR = CT / RC;        // rows of a node a workgroup walks at once
constexpr int TRI_LDS_MANY = 512;  // rows of a node's triangle the chunked solves keep in LDS: 512 x RC doubles = 32 KiB, four workgroups per CU
static_assert(CT % RC == 0 && 64 % RC == 0 && TRI_LDS_MANY * RC * 8 <= 64 * 1024, "a row's lanes lie in one wave; static LDS <= 64 KiB");

// the index of position pos (0-based) in struct(J), or -1
__device__ __forceinline__ int struct_find(const i64 *__restrict__ srv, const CholNode &J, u32 pos) {
    const i64 *s = srv + J.sbase;
    int lo = 0, hi = (int)J.h - 1;
    const i64 want = (i64)pos + 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const i64 v = s[mid];
        if (v == want) return mid;
        if (v < want) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

// y = v[c]
static __global__ __launch_bounds__(CT) void panel_gather_k(const u32 *__restrict__ perm, const double *__restrict__ v, double *__restrict__ y, i64 n) {
    const i64 k = (i64)blockIdx.x * CT + threadIdx.x;
    if (k < n) y[k] = v[perm[k]];
}
// u[c[k]] = x[k], or simple!'s step u[c[k]] = u[c[k]] - x[k]
static __global__ __launch_bounds__(CT) void panel_scatter_k(const u32 *__restrict__ perm, const double *__restrict__ x, double *__restrict__ u, i64 n, bool sub) {
    const i64 k = (i64)blockIdx.x * CT + threadIdx.x;
    if (k >= n) return;
    const u32 i = perm[k];
    u[i] = sub ? u[i] - x[k] : x[k];
}

// the chunked forms over nr <= RC columns: y[k * RC + r] = V[c[k], r] (v: column-major, leading dimension ldv) ...
static __global__ __launch_bounds__(CT) void panel_gather_many_k(const u32 *__restrict__ perm, const double *__restrict__ v, i64 ldv, double *__restrict__ y,
                                                                 i64 n, int nr) {
    const i64 e = (i64)blockIdx.x * CT + threadIdx.x, k = e / RC;
    const int r = (int)(e % RC);
    if (k < n && r < nr) y[e] = v[(i64)r * ldv + perm[k]];
}
// ... and U[c[k], r] = x[k * RC + r]
static __global__ __launch_bounds__(CT) void panel_scatter_many_k(const u32 *__restrict__ perm, const double *__restrict__ x, double *__restrict__ u, i64 ldu,
                                                                  i64 n, int nr) {
    const i64 e = (i64)blockIdx.x * CT + threadIdx.x, k = e / RC;
    const int r = (int)(e % RC);
    if (k < n && r < nr) u[(i64)r * ldu + perm[k]] = x[e];
}
// what a lane of the chunked solves owns: right-hand side r of the row slot `slot` (the RC lanes of a row are neighbours in one wave)
struct ManyLane {
    int r, slot, head;  // head: the wave lane of the row's first right-hand side
    bool on;            // r < nr: a narrower last chunk is masked
};
__device__ __forceinline__ ManyLane many_lane(int nr) {
    const int tid = threadIdx.x;
    return ManyLane{tid % RC, tid / RC, (tid & 63) & ~(RC - 1), tid % RC < nr};
}
// struct_find once per (row, descendant), the RC lanes of a row sharing the work: lane r bisects position pos in the r-th node of
// ulist[u0 .. min(u0 + RC, ue)) (a masked lane too) and every lane of the row reads answer q by many_found.  (With the bisection
// on the row's first lane alone seven lanes of eight wait on its chain of loads: NOTES/multi_rhs.md has that form's times)
__device__ __forceinline__ int struct_find_spread(const CholNode *__restrict__ nodes, const u32 *__restrict__ ulist, const i64 *__restrict__ srv, u32 u0,
                                                  u32 ue, u32 pos, bool valid, const ManyLane &m) {
    const u32 u = u0 + (u32)m.r;
    return (valid && u < ue) ? struct_find(srv, nodes[ulist[u]], pos) : -1;
}
// the answer of the row's lane q.  Every lane of the wave calls it
__device__ __forceinline__ int many_found(int mine, int q, const ManyLane &m) { return __shfl(mine, m.head + q); }

template <typename T>
inline int32_t download(esp_handle *h, std::vector<T> &out, const void *src, size_t count) {
    out.resize(count);
    if (count) HIPCK(h, hipMemcpyAsync(out.data(), src, sizeof(T) * count, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}
template <typename T>
inline int32_t upload(esp_handle *h, DevBuf &b, const std::vector<T> &v) {
    CK(ensure(h, b, sizeof(T) * std::max<size_t>(v.size(), 1)));
    if (!v.empty()) HIPCK(h, hipMemcpyAsync(b.p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));  // (v is free from here)
    return ESP_OK;
}

inline void tree_drop(PanelTree &t) {
    if (t.S) (void)esp_destroy(t.S);
    t.S = nullptr;
    for (DevBuf *b : {&t.nodes, &t.ulist, &t.dlist, &t.flist, &t.nodeof}) release(*b);
}

// the node table, the update lists and the schedule of the ordered tree o with its struct lists (hs, x: lu_structs'; S is taken out
// of hs).  wide_from: the width from which a node takes the wide form.  what: the message prefix.  On failure t holds what it had
// got so far: the caller drops it
inline int32_t tree_build(esp_handle *h, Order &o, espamg::Handles &hs, const Struct &x, const char *what, u32 wide_from, PanelTree &t) {
    const i64 n = h->n;
    std::vector<u32> nstart, nsize, level, perm;
    std::vector<i64> scp, tcp, trv;
    if (n > 0) {
        CK(download(h, nstart, o.nstart.p, (size_t)n));
        CK(download(h, nsize, o.nsize.p, (size_t)n));
        CK(download(h, level, o.level.p, (size_t)n));
        CK(download(h, perm, o.perm.p, (size_t)n));
        if (x.scp) {
            CK(download(h, scp, x.scp, (size_t)n + 1));
            CK(download(h, tcp, x.tcp, (size_t)n + 1));
            CK(download(h, trv, x.trv, (size_t)hs.v[1]->nnz));
        }
    }
    std::vector<CholNode> &nodes = t.host_nodes;
    nodes.clear();
    std::vector<u32> nodeof((size_t)n), ulist;
    i64 off = 0, nnzL = 0, largest = 0;
    for (i64 k = 0; k < n;) {
        CholNode K{};
        K.start = (u32)k;
        K.w = nsize[(size_t)k];
        if (K.w == 0 || nstart[(size_t)k] != (u32)k || k + K.w > n) FAIL(h, ESP_ERR_HIP, "%s: the nodes of the ordering do not tile the positions", what);
        K.depth = level[perm[(size_t)k]];
        K.h = scp.empty() ? 0u : (u32)(scp[(size_t)k + 1] - scp[(size_t)k]);
        K.sbase = scp.empty() ? 0 : scp[(size_t)k] - 1;
        K.off = off;
        off += ((i64)K.w + K.h) * K.w;
        nnzL += (i64)K.w * (K.w + 1) / 2 + (i64)K.w * K.h;
        largest = std::max<i64>(largest, K.w);
        for (u32 q = 0; q < K.w; q++) nodeof[(size_t)k + q] = (u32)nodes.size();
        nodes.push_back(K);
        k += K.w;
    }
    if ((i64)nodes.size() != o.nodes) FAIL(h, ESP_ERR_HIP, "%s: %lld nodes counted, %lld listed", what, (long long)o.nodes, (long long)nodes.size());
    // the update lists: the nodes whose struct holds a position of K, ascending (T's column k lists them by start)
    std::vector<u32> tmp;
    for (CholNode &K : nodes) {
        tmp.clear();
        if (!tcp.empty())
            for (u32 q = 0; q < K.w; q++)
                for (i64 e = tcp[(size_t)K.start + q] - 1; e < tcp[(size_t)K.start + q + 1] - 1; e++) tmp.push_back(nodeof[(size_t)(trv[(size_t)e] - 1)]);
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        K.ub = (u32)ulist.size();
        ulist.insert(ulist.end(), tmp.begin(), tmp.end());
        K.ue = (u32)ulist.size();
        if (ulist.size() >= 0xFFFFFFF0ull) FAIL(h, ESP_ERR_UNSUPPORTED, "%s: the update lists hold 2^32 entries", what);
    }
    // the schedule: the nodes are sorted by depth descending already
    t.depth.assign((size_t)(n > 0 ? o.deepest + 1 : 0), CholDepth());
    std::vector<u32> dlist, flist;
    i64 nsmall = 0, nwide = 0, nbcols = 0;
    for (size_t a = 0; a < nodes.size();) {
        size_t b = a;
        while (b < nodes.size() && nodes[b].depth == nodes[a].depth) b++;
        if (nodes[a].depth >= t.depth.size()) FAIL(h, ESP_ERR_HIP, "%s: a node lies deeper than the deepest level", what);
        CholDepth &D = t.depth[nodes[a].depth];
        if (D.all_count) FAIL(h, ESP_ERR_HIP, "%s: the nodes are not sorted by depth", what);
        D.all_first = (u32)dlist.size();
        D.all_count = (u32)(b - a);
        for (size_t q = a; q < b; q++) dlist.push_back((u32)q);
        D.small_first = (u32)flist.size();
        std::vector<u32> wide;
        for (size_t q = a; q < b; q++) {
            if (nodes[q].w < wide_from) flist.push_back((u32)q);
            else wide.push_back((u32)q);
        }
        D.small_count = (u32)flist.size() - D.small_first;
        nsmall += D.small_count;
        nwide += (i64)wide.size();
        std::stable_sort(wide.begin(), wide.end(), [&](u32 l, u32 r) { return nodes[l].w > nodes[r].w; });
        const u32 wfirst = (u32)flist.size();
        flist.insert(flist.end(), wide.begin(), wide.end());
        const u32 maxbc = wide.empty() ? 0u : (nodes[wide[0]].w + NB - 1) / NB;
        for (u32 bc = 0; bc < maxbc; bc++) {
            CholLaunch Lc{wfirst, 0, bc, 1, 1};
            i64 rows = 0;
            for (u32 q : wide) {
                if ((nodes[q].w + NB - 1) / NB <= bc) break;
                Lc.count++;
                rows = std::max<i64>(rows, (i64)nodes[q].w + nodes[q].h - (i64)bc * NB);
            }
            Lc.tiles_u = (u32)std::max<i64>(1, (rows + TR - 1) / TR);
            Lc.tiles_f = (u32)std::max<i64>(1, (rows + FR - 1) / FR);  // (the rows below a short last block column: a bound)
            if ((i64)Lc.count * std::max(Lc.tiles_u, Lc.tiles_f) > 0x7FFFFFFFll) FAIL(h, ESP_ERR_UNSUPPORTED, "%s: a depth's grid exceeds 2^31 workgroups", what);
            D.wide.push_back(Lc);
        }
        nbcols += maxbc;
        a = b;
    }
    CK(upload(h, t.nodes, nodes));
    CK(upload(h, t.ulist, ulist));
    CK(upload(h, t.dlist, dlist));
    CK(upload(h, t.flist, flist));
    CK(upload(h, t.nodeof, nodeof));
    if (!hs.v.empty()) {
        t.S = hs.v[0];
        hs.v[0] = nullptr;
    }
    t.nnodes = (i64)nodes.size();
    t.panel_doubles = off;
    t.nnzL = nnzL;
    t.largest = largest;
    t.nsmall = nsmall;
    t.nwide = nwide;
    t.nbcols = nbcols;
    return ESP_OK;
}

}  // namespace esppanel
