// cholesky.hip -- libesparse_hip: CholeskyFactorization (esp_precon_cholesky_create), A[c,c] = L L' on dense panels per tree node
// (see internal.hpp for the map of the translation units)
//
// The rule is stated in full in include/esparse_hip.h and DESIGN.md 5r; tests/cholesky_model.c restates it as plain loops and is
// normative.  The ordering c, the nodes and struct(K) are lu.hip's (lu_dissect, lu_order, lu_structs), unchanged.  In short: column j
// of L holds the positions of node(j) from j on, then struct(node(j)); every entry is ONE chain t = a_ij - sum over k < j ascending of
// l_ik l_jk (each product rounded, each difference rounded), l_jj = sqrt(t), l_ij = t / l_jj.  Any schedule that walks every chain in
// that order gives the same bits; this one walks the tree depth by depth.
//
//   panels     node K (width w, h = |struct(K)|) owns a dense (w + h) x w column-major panel, all panels in one allocation (64-bit
//              offsets).  The tables, their builder, struct_find and the gather / scatter of v[c] live in panels.hpp, shared with
//              lu_panels.hip.  CholNode holds offset, w, h, start, depth, where struct(K) lies in S's rowval, and K's update list: the
//              descendants J with struct(J) meeting K, ascending by position (from the transpose of S; built on the host at set-up).
//              A position is found in J's panel by bisection in the sorted struct(J).
//   load       chol_load_k: the panels are zeroed, then one lane per column s of A scatters the stored A[r, s], r <= s.  It is the
//              whole gather of a values-only update.
//   update     update_tile: a workgroup owns a TR x NB tile of a block column (NB columns) of K's panel, 2 x 4 accumulators per
//              lane.  Per descendant J of the update list, in order: the panel rows of the tile's rows and columns in J (bisection,
//              one lane each), then J's columns in ascending k, KB at a time through LDS.  K's own columns in front of the block
//              column come last, as one more "descendant" whose rows are the tile's own.
//   factor     factor_diag: the NB x NB diagonal block right-looking in LDS, by the workgroup that updated the tile holding it; a failing
//              pivot is reported by atomicMin.  factor_rows: one lane per row below, the row in LDS, the chain against the
//              diagonal block (LDS), the division.
//   forms      small (w < wide_from): chol_small_k, a workgroup per node runs its block columns one after the other, every small
//              node of a depth in one launch.  wide: chol_update_k (tiles and diagonal blocks) / chol_factor_k (rows below) per block column for all wide nodes of the depth
//              at once, tiles spread over the grid.  Both call the same two functions: the bits are the same.
//   solve      gather y = v[c]; forward per depth from the deepest up (chol_fwd_k, a workgroup per node: one lane per row gathers
//              from the update list with k ascending, then the triangle right-looking, t in LDS up to TRI_LDS rows, else in a
//              second vector); backward per depth from 0 down (chol_bwd_k: struct first, then the triangle from the last position
//              up); scatter u[c] = x.  Launches on the handle's stream and nothing else.  Several right-hand sides
//              (esp_precon_ldiv_many): chol_fwd_many_k / chol_bwd_many_k carry RC = 8 columns per pass over the panels,
//              a lane per (row of the node, right-hand side) pair, the work vectors stored right-hand-side-fastest.
#include "panels.hpp"

using namespace espamg;
using namespace esplu;
using namespace esppanel;

struct CholData : PanelTree {
    DevBuf panels, fail, y, y2, lcp;
    DevBuf ym, y2m;  // the work vectors of the chunked solves, n * RC doubles each, from the first esp_precon_ldiv_many on
    bool failed = false;
    i64 stats[ESP_CHOL_STATS] = {0};
};

namespace {

struct Dev {
    const CholNode *nodes;
    const u32 *ulist;
    const i64 *srv;
    double *panels;
};

__device__ __forceinline__ int struct_find(const Dev &d, const CholNode &J, u32 pos) { return esppanel::struct_find(d.srv, J, pos); }

// ---- load ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT) void chol_load_k(Dev d, espfold::Csc A, const u32 *__restrict__ newpos, const u32 *__restrict__ nodeof, i64 n) {
    const i64 s = (i64)blockIdx.x * CT + threadIdx.x;
    if (s >= n) return;
    const u32 ps = newpos[s];
    for (i64 q = A.colptr[s] - 1; q < A.colptr[s + 1] - 1; q++) {
        const i64 r = A.rowval[q] - 1;
        if (r > s) continue;  // (the strict lower triangle is never read)
        const u32 pr = newpos[r];
        const u32 lo = pr < ps ? pr : ps, hi = pr < ps ? ps : pr;
        const CholNode K = d.nodes[nodeof[lo]];
        i64 row;
        if (hi < K.start + K.w) row = (i64)(hi - K.start);
        else {
            const int f = struct_find(d, K, hi);
            if (f < 0) continue;  // (an edge of A's graph always lies in the pattern)
            row = (i64)K.w + f;
        }
        d.panels[K.off + (i64)(lo - K.start) * ((i64)K.w + K.h) + row] = A.nzval[q];
    }
}

// ---- update --------------------------------------------------------------------------------------------------------------------------
struct TileLds {
    double a[KB][TR];   // the rows' slice of a descendant's panel
    double b[KB][NB];   // the columns' slice
    int ri[TR], rj[NB]; // the panel row in the descendant of every tile row / column, -1: none
    u32 pos[TR];        // the position of every tile row
};

// acc -= the columns [0, kcount) of the panel (base, ld) over the rows L.ri / L.rj, k ascending
__device__ __forceinline__ void tile_apply(TileLds &L, const double *__restrict__ base, i64 ld, u32 kcount, double (&acc)[2][4]) {
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const bool r0 = L.ri[tx] >= 0, r1 = L.ri[tx + 32] >= 0;
    bool cv[4];
#pragma unroll
    for (int c = 0; c < 4; c++) cv[c] = L.rj[ty * 4 + c] >= 0;
    for (u32 k0 = 0; k0 < kcount; k0 += KB) {
        const int kn = (int)min((u32)KB, kcount - k0);
        __syncthreads();  // (the slices of the chunk before are read)
        for (int e = tid; e < KB * TR; e += CT) {
            const int kk = e / TR, r = e % TR;
            const int row = L.ri[r];
            L.a[kk][r] = (kk < kn && row >= 0) ? base[(i64)(k0 + kk) * ld + row] : 0.0;
        }
        for (int e = tid; e < KB * NB; e += CT) {
            const int kk = e / NB, c = e % NB;
            const int row = L.rj[c];
            L.b[kk][c] = (kk < kn && row >= 0) ? base[(i64)(k0 + kk) * ld + row] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < kn; kk++) {
            const double a0 = L.a[kk][tx], a1 = L.a[kk][tx + 32];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const double b = L.b[kk][ty * 4 + c];
                const double p0 = a0 * b, p1 = a1 * b;
                acc[0][c] = (r0 && cv[c]) ? acc[0][c] - p0 : acc[0][c];
                acc[1][c] = (r1 && cv[c]) ? acc[1][c] - p1 : acc[1][c];
            }
        }
    }
}

// the tile of K's panel: columns [c0, c0 + nc), rows [r0, r0 + TR) (r0 >= c0): every chain up to the columns in front of c0.
// Every lane of the workgroup calls it
__device__ void update_tile(const Dev &d, const CholNode &K, u32 c0, u32 nc, u32 r0, TileLds &L) {
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const i64 ld = (i64)K.w + K.h;
    double *P = d.panels + K.off;
    __syncthreads();  // (whoever used L before is done)
    if (tid < TR) {
        const i64 r = (i64)r0 + tid;
        L.pos[tid] = r >= ld ? LU_NONE : r < (i64)K.w ? K.start + (u32)r : (u32)(d.srv[K.sbase + (r - K.w)] - 1);
    }
    double acc[2][4];
#pragma unroll
    for (int rr = 0; rr < 2; rr++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const i64 r = (i64)r0 + tx + 32 * rr;
            const u32 cc = (u32)(ty * 4 + c);
            acc[rr][c] = (r < ld && cc < nc) ? P[(i64)(c0 + cc) * ld + r] : 0.0;
        }
    __syncthreads();
    for (u32 u = K.ub; u < K.ue; u++) {
        const CholNode J = d.nodes[d.ulist[u]];
        bool mine = false;
        if (tid < TR) {
            const u32 pos = L.pos[tid];
            const int f = pos == LU_NONE ? -1 : struct_find(d, J, pos);
            L.ri[tid] = f < 0 ? -1 : (int)J.w + f;
        } else if (tid < TR + NB) {
            const u32 c = (u32)(tid - TR);
            const int f = c < nc ? struct_find(d, J, K.start + c0 + c) : -1;
            L.rj[c] = f < 0 ? -1 : (int)J.w + f;
            mine = f >= 0;
        }
        if (!__syncthreads_or(mine)) continue;  // (no column of the block column lies in struct(J): nothing to subtract)
        tile_apply(L, d.panels + J.off, (i64)J.w + J.h, J.w, acc);
        __syncthreads();
    }
    if (c0 > 0) {  // K's own columns in front of the block column
        if (tid < TR) L.ri[tid] = L.pos[tid] == LU_NONE ? -1 : (int)(r0 + tid);
        else if (tid < TR + NB) L.rj[tid - TR] = (u32)(tid - TR) < nc ? (int)(c0 + tid - TR) : -1;
        __syncthreads();
        tile_apply(L, P, ld, c0, acc);
    }
#pragma unroll
    for (int rr = 0; rr < 2; rr++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const i64 r = (i64)r0 + tx + 32 * rr;
            const u32 cc = (u32)(ty * 4 + c);
            if (r < ld && cc < nc && r >= (i64)(c0 + cc)) P[(i64)(c0 + cc) * ld + r] = acc[rr][c];
        }
}

// ---- factor --------------------------------------------------------------------------------------------------------------------------
struct FactorLds {
    double D[NB][NB + 1];
};
struct RowLds {
    double X[NB][FR];  // the rows below, one per lane
};

// the diagonal block of the block column [c0, c0 + nc) of K's panel, updated: right-looking in LDS, stored back; a failing pivot
// goes to `fail` by atomicMin.  Every lane of the workgroup calls it
__device__ void factor_diag(const Dev &d, const CholNode &K, u32 c0, u32 nc, FactorLds &F, unsigned long long *__restrict__ fail) {
    const int tid = threadIdx.x;
    const i64 ld = (i64)K.w + K.h;
    double *P = d.panels + K.off;
    __syncthreads();
    for (int e = tid; e < NB * NB; e += CT) {
        const u32 i = (u32)(e % NB), j = (u32)(e / NB);
        F.D[i][j] = (i < nc && j <= i) ? P[(i64)(c0 + j) * ld + c0 + i] : 0.0;
    }
    __syncthreads();
    for (u32 k = 0; k < nc; k++) {
        if (tid == 0) {
            const double t = F.D[k][k];
            if (!(t > 0)) atomicMin(fail, (unsigned long long)(K.start + c0 + k));
            F.D[k][k] = sqrt(t);
        }
        __syncthreads();
        if ((u32)tid > k && (u32)tid < nc) F.D[tid][k] = F.D[tid][k] / F.D[k][k];
        __syncthreads();
        const u32 i = (u32)(tid >> 3);
        if (i > k && i < nc) {
            const double lik = F.D[i][k];
            for (u32 j = (u32)(tid & 7); j <= i; j += 8)
                if (j > k) {
                    const double pr = lik * F.D[j][k];
                    F.D[i][j] = F.D[i][j] - pr;
                }
        }
        __syncthreads();
    }
    for (int e = tid; e < NB * NB; e += CT) {
        const u32 i = (u32)(e % NB), j = (u32)(e / NB);
        if (i < nc && j <= i) P[(i64)(c0 + j) * ld + c0 + i] = F.D[i][j];
    }
}

// the rows [rb, re), re - rb <= FR, below the factored diagonal block (read from the panel): one lane per row, the row
// in LDS, the chain against the block, the division.  Every lane of the workgroup calls it
__device__ void factor_rows(const Dev &d, const CholNode &K, u32 c0, u32 nc, i64 rb, i64 re, FactorLds &F, RowLds &R) {
    const int tid = threadIdx.x;
    const i64 ld = (i64)K.w + K.h;
    double *P = d.panels + K.off;
    __syncthreads();
    for (int e = tid; e < NB * NB; e += CT) {
        const u32 i = (u32)(e % NB), j = (u32)(e / NB);
        F.D[i][j] = (i < nc && j <= i) ? P[(i64)(c0 + j) * ld + c0 + i] : 0.0;
    }
    __syncthreads();
    const i64 r = rb + tid;
    if (tid < FR && r < re) {  // (the row lives in LDS, one column of F.X per lane: registers would need the whole chain unrolled)
        for (u32 j = 0; j < nc; j++) R.X[j][tid] = P[(i64)(c0 + j) * ld + r];
        for (u32 j = 0; j < nc; j++) {
            double t = R.X[j][tid];
            for (u32 k = 0; k < j; k++) {
                const double pr = R.X[k][tid] * F.D[j][k];
                t = t - pr;
            }
            t = t / F.D[j][j];
            R.X[j][tid] = t;
            P[(i64)(c0 + j) * ld + r] = t;
        }
    }
}

// the small form: a workgroup per node of list[0 .. count)
__global__ __launch_bounds__(CT) void chol_small_k(Dev d, const u32 *__restrict__ list, unsigned long long *__restrict__ fail) {
    __shared__ TileLds L;
    __shared__ FactorLds F;
    __shared__ RowLds R;
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    for (u32 c0 = 0; c0 < K.w; c0 += NB) {
        const u32 nc = min((u32)NB, K.w - c0);
        for (i64 r0 = c0; r0 < ld; r0 += TR) update_tile(d, K, c0, nc, (u32)r0, L);
        __threadfence_block();
        factor_diag(d, K, c0, nc, F, fail);
        __threadfence_block();
        for (i64 rb = (i64)c0 + nc; rb < ld; rb += FR) factor_rows(d, K, c0, nc, rb, min(rb + FR, ld), F, R);
        __threadfence_block();
    }
}
// the wide form, block column bc of the nodes list[0 .. count): workgroup (node, tile) = (blockIdx.x / tiles, blockIdx.x % tiles)
__global__ __launch_bounds__(CT) void chol_update_k(Dev d, const u32 *__restrict__ list, u32 bc, u32 tiles, unsigned long long *__restrict__ fail) {
    __shared__ TileLds L;
    __shared__ FactorLds F;
    const CholNode K = d.nodes[list[blockIdx.x / tiles]];
    const u32 c0 = bc * NB, nc = min((u32)NB, K.w - c0);
    const i64 r0 = (i64)c0 + (i64)(blockIdx.x % tiles) * TR;
    if (r0 >= (i64)K.w + K.h) return;
    update_tile(d, K, c0, nc, (u32)r0, L);
    if (r0 != (i64)c0) return;  // the first tile holds the whole diagonal block (NB <= TR) and no other tile touches it
    __threadfence_block();
    factor_diag(d, K, c0, nc, F, fail);
}
__global__ __launch_bounds__(CT) void chol_factor_k(Dev d, const u32 *__restrict__ list, u32 bc, u32 tiles) {
    __shared__ FactorLds F;
    __shared__ RowLds R;
    const CholNode K = d.nodes[list[blockIdx.x / tiles]];
    const u32 c0 = bc * NB, nc = min((u32)NB, K.w - c0), t = blockIdx.x % tiles;
    const i64 ld = (i64)K.w + K.h, rb = (i64)c0 + nc + (i64)t * FR;
    if (rb >= ld) return;
    factor_rows(d, K, c0, nc, rb, min(rb + FR, ld), F, R);
}

// ---- solve ---------------------------------------------------------------------------------------------------------------------------
// forward: a workgroup per node of list.  t lives in LDS (w <= TRI_LDS) or in y2
__global__ __launch_bounds__(CT) void chol_fwd_k(Dev d, const u32 *__restrict__ list, double *__restrict__ y, double *__restrict__ y2) {
    __shared__ double sh[TRI_LDS];
    const int tid = threadIdx.x;
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    const double *P = d.panels + K.off;
    double *t = K.w <= (u32)TRI_LDS ? sh : y2 + K.start;
    for (u32 j = (u32)tid; j < K.w; j += CT) {
        double a = y[K.start + j];
        for (u32 u = K.ub; u < K.ue; u++) {
            const CholNode J = d.nodes[d.ulist[u]];
            const int f = struct_find(d, J, K.start + j);
            if (f < 0) continue;
            const i64 ldj = (i64)J.w + J.h;
            const double *R = d.panels + J.off + J.w + f;
            const double *yj = y + J.start;
            for (u32 k = 0; k < J.w; k++) {
                const double pr = R[(i64)k * ldj] * yj[k];
                a = a - pr;
            }
        }
        t[j] = a;
    }
    for (u32 k = 0; k < K.w; k++) {
        __syncthreads();
        const double yk = t[k] / P[(i64)k * ld + k];
        if (tid == 0) y[K.start + k] = yk;
        for (u32 i = k + 1 + (u32)tid; i < K.w; i += CT) {
            const double pr = P[(i64)k * ld + i] * yk;
            t[i] = t[i] - pr;
        }
    }
}
// backward: struct(K) ascending, then the triangle from the last position up
__global__ __launch_bounds__(CT) void chol_bwd_k(Dev d, const u32 *__restrict__ list, double *__restrict__ y, double *__restrict__ y2) {
    __shared__ double sh[TRI_LDS];
    const int tid = threadIdx.x;
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    const double *P = d.panels + K.off;
    const i64 *st = d.srv + K.sbase;
    double *t = K.w <= (u32)TRI_LDS ? sh : y2 + K.start;
    for (u32 j = (u32)tid; j < K.w; j += CT) {
        double a = y[K.start + j];
        const double *C = P + (i64)j * ld + K.w;
        for (u32 i = 0; i < K.h; i++) {
            const double pr = C[i] * y[st[i] - 1];
            a = a - pr;
        }
        t[j] = a;
    }
    for (u32 k = K.w; k-- > 0;) {
        __syncthreads();
        const double xk = t[k] / P[(i64)k * ld + k];
        if (tid == 0) y[K.start + k] = xk;
        for (u32 j = (u32)tid; j < k; j += CT) {
            const double pr = P[(i64)j * ld + k] * xk;
            t[j] = t[j] - pr;
        }
    }
}

// ---- solve, several right-hand sides -----------------------------------------------------------------------------------
// chol_fwd_k over nr <= RC right-hand sides at once: y and y2 hold RC doubles per position (y[pos * RC + r]); a lane owns right-hand
// side r = tid % RC of the rows slot, slot + RR, ... of the node and walks chol_fwd_k's chain for that pair.  The RC lanes of a row
// read the same panel entry (one fetch) and RC neighbouring doubles of y.  t: w x RC doubles, in LDS up to TRI_LDS_MANY rows
__global__ __launch_bounds__(CT) void chol_fwd_many_k(Dev d, const u32 *__restrict__ list, double *__restrict__ y, double *__restrict__ y2, int nr) {
    __shared__ double sh[TRI_LDS_MANY * RC];
    const ManyLane m = many_lane(nr);
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    const double *P = d.panels + K.off;
    double *t = K.w <= (u32)TRI_LDS_MANY ? sh : y2 + (i64)K.start * RC;
    for (u32 j0 = 0; j0 < K.w; j0 += RR) {  // (uniform over the workgroup: the shuffle of many_found needs every lane)
        const u32 j = j0 + (u32)m.slot;
        const bool valid = j < K.w;
        double a = (valid && m.on) ? y[(i64)(K.start + j) * RC + m.r] : 0.0;
        for (u32 u0 = K.ub; u0 < K.ue; u0 += RC) {
            const int mine = struct_find_spread(d.nodes, d.ulist, d.srv, u0, K.ue, K.start + j, valid, m);
            for (int q = 0; q < RC && u0 + q < K.ue; q++) {  // the update list ascending, as chol_fwd_k walks it
                const int f = many_found(mine, q, m);
                if (f < 0 || !m.on) continue;
                const CholNode J = d.nodes[d.ulist[u0 + q]];
                const i64 ldj = (i64)J.w + J.h;
                const double *R = d.panels + J.off + J.w + f;
                const double *yj = y + (i64)J.start * RC + m.r;
                for (u32 k = 0; k < J.w; k++) {
                    const double pr = R[(i64)k * ldj] * yj[(i64)k * RC];
                    a = a - pr;
                }
            }
        }
        if (valid && m.on) t[(i64)j * RC + m.r] = a;
    }
    for (u32 k = 0; k < K.w; k++) {
        __syncthreads();
        if (!m.on) continue;
        const double yk = t[(i64)k * RC + m.r] / P[(i64)k * ld + k];
        if (m.slot == 0) y[(i64)(K.start + k) * RC + m.r] = yk;
        for (u32 i = k + 1 + (u32)m.slot; i < K.w; i += RR) {
            const double pr = P[(i64)k * ld + i] * yk;
            t[(i64)i * RC + m.r] = t[(i64)i * RC + m.r] - pr;
        }
    }
}
// chol_bwd_k in the same way
__global__ __launch_bounds__(CT) void chol_bwd_many_k(Dev d, const u32 *__restrict__ list, double *__restrict__ y, double *__restrict__ y2, int nr) {
    __shared__ double sh[TRI_LDS_MANY * RC];
    const ManyLane m = many_lane(nr);
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    const double *P = d.panels + K.off;
    const i64 *st = d.srv + K.sbase;
    double *t = K.w <= (u32)TRI_LDS_MANY ? sh : y2 + (i64)K.start * RC;
    if (m.on)
        for (u32 j = (u32)m.slot; j < K.w; j += RR) {
            double a = y[(i64)(K.start + j) * RC + m.r];
            const double *C = P + (i64)j * ld + K.w;
            for (u32 i = 0; i < K.h; i++) {
                const double pr = C[i] * y[(st[i] - 1) * RC + m.r];
                a = a - pr;
            }
            t[(i64)j * RC + m.r] = a;
        }
    for (u32 k = K.w; k-- > 0;) {
        __syncthreads();
        if (!m.on) continue;
        const double xk = t[(i64)k * RC + m.r] / P[(i64)k * ld + k];
        if (m.slot == 0) y[(i64)(K.start + k) * RC + m.r] = xk;
        for (u32 j = (u32)m.slot; j < k; j += RR) {
            const double pr = P[(i64)j * ld + k] * xk;
            t[(i64)j * RC + m.r] = t[(i64)j * RC + m.r] - pr;
        }
    }
}

// ---- L as a CSC ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CT) void chol_export_k(Dev d, const u32 *__restrict__ nodeof, const i64 *__restrict__ lcp, i64 n, i64 *__restrict__ rv,
                                                    double *__restrict__ nz) {
    const i64 j = (i64)blockIdx.x * CT + threadIdx.x;
    if (j >= n) return;
    const CholNode K = d.nodes[nodeof[j]];
    const i64 ld = (i64)K.w + K.h, cj = j - K.start;
    const double *C = d.panels + K.off + cj * ld;
    i64 q = lcp[j] - 1;
    for (i64 r = cj; r < ld; r++, q++) {
        if (rv) rv[q] = r < (i64)K.w ? (i64)K.start + r + 1 : d.srv[K.sbase + (r - K.w)];
        if (nz) nz[q] = C[r];
    }
}

Dev dev_of(const CholData *c) {
    return Dev{(const CholNode *)c->nodes.p, (const u32 *)c->ulist.p, c->S ? (const i64 *)c->S->rowval.p : nullptr, (double *)c->panels.p};
}

void chol_drop(CholData *c) {
    if (!c) return;
    tree_drop(*c);
    for (DevBuf *b : {&c->panels, &c->fail, &c->y, &c->y2, &c->lcp, &c->ym, &c->y2m}) release(*b);
    delete c;
}

// the ordering, the tree, the tables and the panels' layout from A's current pattern: a new CholData, p untouched
int32_t chol_symbolic(esp_precon *p, CholData **out, Order &o) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    CK(lu_dissect(h, p->lu_leaf, p->lu_depth, o));
    CK(lu_order(h, o));
    Handles hs;
    Struct x{nullptr, nullptr, nullptr, nullptr};
    CK(lu_structs(h, o, "esp_precon_cholesky", hs, x));
    CholData *c = new CholData();
    struct Guard {
        CholData *c;
        ~Guard() { chol_drop(c); }
    } guard{c};
    const u32 wide_from = h->debug_chol_wide > 0 ? (u32)std::min<i64>(h->debug_chol_wide, 0xFFFFFFFFll) : (u32)NB + 1;
    CK(tree_build(h, o, hs, x, "esp_precon_cholesky", wide_from, *c));
    // L's column starts
    std::vector<i64> lcp((size_t)n + 1);
    lcp[0] = 1;
    for (const CholNode &K : c->host_nodes)
        for (u32 t = 0; t < K.w; t++) lcp[(size_t)K.start + t + 1] = lcp[(size_t)K.start + t] + (K.w - t) + K.h;
    c->host_nodes.clear();
    const i64 off = c->panel_doubles;
    CK(upload(h, c->lcp, lcp));
    CK(ensure(h, c->panels, sizeof(double) * (size_t)std::max<i64>(off, 1)));
    CK(ensure(h, c->fail, sizeof(u64)));
    CK(ensure(h, c->y, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    CK(ensure(h, c->y2, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    i64 *st = c->stats;
    st[0] = c->nnzL;
    st[1] = o.rounds;
    st[2] = n > 0 ? o.deepest : 0;
    st[3] = c->nnodes;
    st[4] = c->largest;
    st[5] = off;
    st[9] = c->nsmall;
    st[10] = c->nwide;
    st[11] = c->nbcols;
    i64 solve = n > 0 ? 2 : 0;
    for (const CholDepth &D : c->depth) solve += D.all_count ? 2 : 0;
    st[8] = solve;
    guard.c = nullptr;
    *out = c;
    return ESP_OK;
}

// the load and the numeric factorization on c's layout: launches only, then ONE read-back of the failing position
int32_t chol_numeric(esp_precon *p, CholData *c, const u32 *newpos, const u32 *perm) {
    esp_handle *h = p->h;
    hipStream_t s = h->stream;
    const i64 n = p->n;
    i64 launches = 0;
    c->failed = true;
    if (n > 0) {
        const Dev d = dev_of(c);
        unsigned long long *fail = (unsigned long long *)c->fail.p;
        HIPCK(h, hipMemsetAsync(c->panels.p, 0, sizeof(double) * (size_t)c->panel_doubles, s));
        HIPCK(h, hipMemsetAsync(fail, 0xFF, sizeof(u64), s));
        const espfold::Csc A{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (double *)h->nzval.p, h->nnz};
        hipLaunchKernelGGL(chol_load_k, dim3(grid_for(n, CT)), dim3(CT), 0, s, d, A, newpos, (const u32 *)c->nodeof.p, n);
        launches++;
        const u32 *flist = (const u32 *)c->flist.p;
        for (size_t dep = c->depth.size(); dep-- > 0;) {
            const CholDepth &D = c->depth[dep];
            if (D.small_count) {
                hipLaunchKernelGGL(chol_small_k, dim3(D.small_count), dim3(CT), 0, s, d, flist + D.small_first, fail);
                launches++;
            }
            for (const CholLaunch &Lc : D.wide) {
                hipLaunchKernelGGL(chol_update_k, dim3(Lc.count * Lc.tiles_u), dim3(CT), 0, s, d, flist + Lc.first, Lc.bc, Lc.tiles_u, fail);
                hipLaunchKernelGGL(chol_factor_k, dim3(Lc.count * Lc.tiles_f), dim3(CT), 0, s, d, flist + Lc.first, Lc.bc, Lc.tiles_f);
                launches += 2;
            }
        }
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, fail, sizeof(u64), hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        const unsigned long long bad = h->pin_scalar[0];
        c->stats[7] = launches;
        if (bad != ~0ull) {
            HIPCK(h, hipMemcpyAsync(h->pin_scalar, perm + bad, sizeof(u32), hipMemcpyDeviceToHost, s));
            HIPCK(h, hipStreamSynchronize(s));
            FAIL(h, ESP_ERR_NOTPOSDEF, "esp_precon_cholesky: the matrix is not positive definite: the pivot of position %llu in c fails (A's column is %llu)",
                 bad + 1, (unsigned long long)*(const u32 *)h->pin_scalar + 1);
        }
    }
    c->stats[7] = launches;
    c->failed = false;
    return ESP_OK;
}

int32_t chol_current(esp_precon *p, const char *what) {
    esp_handle *h = p->h;
    if (!p->chol || h->pattern_version != p->pattern_version || h->nnz != p->nnz)
        FAIL(h, ESP_ERR_STATE, "%s: the matrix pattern changed since the factorization's last update!", what);
    return ESP_OK;
}

}  // namespace

int32_t chol_update(esp_precon *p) {
    esp_handle *h = p->h;
    CK(lu_check_args(h, "esp_precon_update", p->lu_leaf, p->lu_depth));
    const bool rebuild = !p->chol || p->pattern_version != h->pattern_version || p->nnz != h->nnz;
    p->pattern_version = 0;  // (a failure below leaves an object that refuses ldiv! until the next good update!)
    if (rebuild) {
        Order o;
        CholData *c = nullptr;
        CK(chol_symbolic(p, &c, o));
        c->stats[6] = (p->chol ? p->chol->stats[6] : 0) + o.launches;
        chol_drop(p->chol);
        p->chol = c;
        std::swap(p->blk_new, o.newpos);
        std::swap(p->lu_perm, o.perm);
        std::swap(p->lu_level, o.level);
        std::swap(p->lu_root, o.root);
    }
    CK(chol_numeric(p, p->chol, (const u32 *)p->blk_new.p, (const u32 *)p->lu_perm.p));
    p->nnz = h->nnz;
    p->pattern_version = h->pattern_version;
    p->values_version = h->values_version;
    return ESP_OK;
}

// u = A \ v on device vectors (u may be v; sub: u[i] = u[i] - x[i], simple!'s step): launches on the handle's stream only
int32_t chol_solve(esp_precon *p, const double *v, double *u, bool sub) {
    esp_handle *h = p->h;
    hipStream_t s = h->stream;
    const i64 n = p->n;
    CholData *c = p->chol;
    if (!c || c->failed) FAIL(h, ESP_ERR_STATE, "esp_precon_ldiv: the last update! of the factorization failed");
    if (n == 0) return ESP_OK;
    const Dev d = dev_of(c);
    const u32 *perm = (const u32 *)p->lu_perm.p, *dlist = (const u32 *)c->dlist.p;
    double *y = (double *)c->y.p, *y2 = (double *)c->y2.p;
    const unsigned g = grid_for(n, CT);
    hipLaunchKernelGGL(panel_gather_k, dim3(g), dim3(CT), 0, s, perm, v, y, n);
    for (size_t dep = c->depth.size(); dep-- > 0;) {
        const CholDepth &D = c->depth[dep];
        if (D.all_count) hipLaunchKernelGGL(chol_fwd_k, dim3(D.all_count), dim3(CT), 0, s, d, dlist + D.all_first, y, y2);
    }
    for (size_t dep = 0; dep < c->depth.size(); dep++) {
        const CholDepth &D = c->depth[dep];
        if (D.all_count) hipLaunchKernelGGL(chol_bwd_k, dim3(D.all_count), dim3(CT), 0, s, d, dlist + D.all_first, y, y2);
    }
    hipLaunchKernelGGL(panel_scatter_k, dim3(g), dim3(CT), 0, s, perm, (const double *)y, u, n, sub);
    return ESP_OK;
}

// U[:, r] = A \ V[:, r] for k columns on device arrays (U may be V where ldu == ldv), RC columns per pass over the panels
int32_t chol_solve_many(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, i64 k) {
    esp_handle *h = p->h;
    hipStream_t s = h->stream;
    const i64 n = p->n;
    CholData *c = p->chol;
    if (!c || c->failed) FAIL(h, ESP_ERR_STATE, "esp_precon_ldiv: the last update! of the factorization failed");
    if (n == 0 || k == 0) return ESP_OK;
    CK(ensure(h, c->ym, sizeof(double) * (size_t)n * RC));
    CK(ensure(h, c->y2m, sizeof(double) * (size_t)n * RC));
    const Dev d = dev_of(c);
    const u32 *perm = (const u32 *)p->lu_perm.p, *dlist = (const u32 *)c->dlist.p;
    double *y = (double *)c->ym.p, *y2 = (double *)c->y2m.p;
    const unsigned g = grid_for(n * RC, CT);
    for (i64 r0 = 0; r0 < k; r0 += RC) {
        const int nr = (int)std::min<i64>(RC, k - r0);
        hipLaunchKernelGGL(panel_gather_many_k, dim3(g), dim3(CT), 0, s, perm, v + r0 * ldv, ldv, y, n, nr);
        for (size_t dep = c->depth.size(); dep-- > 0;) {
            const CholDepth &D = c->depth[dep];
            if (D.all_count) hipLaunchKernelGGL(chol_fwd_many_k, dim3(D.all_count), dim3(CT), 0, s, d, dlist + D.all_first, y, y2, nr);
        }
        for (size_t dep = 0; dep < c->depth.size(); dep++) {
            const CholDepth &D = c->depth[dep];
            if (D.all_count) hipLaunchKernelGGL(chol_bwd_many_k, dim3(D.all_count), dim3(CT), 0, s, d, dlist + D.all_first, y, y2, nr);
        }
        hipLaunchKernelGGL(panel_scatter_many_k, dim3(g), dim3(CT), 0, s, perm, (const double *)y, u + r0 * ldu, ldu, n, nr);
    }
    return ESP_OK;
}

void chol_release(esp_precon *p) {
    if (p->kind != ESP_PRECON_CHOLESKY) return;
    chol_drop(p->chol);
    p->chol = nullptr;
    for (DevBuf *b : {&p->lu_perm, &p->lu_level, &p->lu_root, &p->blk_new}) release(*b);
}

extern "C" int32_t esp_precon_cholesky_create(esp_handle *h, int32_t leaf_size, int32_t max_depth, esp_precon **out) {
    if (!h || !out) return ESP_ERR_INVALID;
    *out = nullptr;
    CK(lu_check_args(h, "esp_precon_cholesky_create", leaf_size, max_depth));
    esp_precon *p = precon_new(h, ESP_PRECON_CHOLESKY);
    p->lu_leaf = leaf_size;
    p->lu_depth = max_depth;
    return precon_finish(p, chol_update(p), out);
}

extern "C" int32_t esp_precon_cholesky_perm(esp_precon *p, int64_t *c, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_CHOLESKY || !c) return ESP_ERR_INVALID;
    CK(chol_current(p, "esp_precon_cholesky_perm"));
    return lu_export(p->h, p->lu_perm, c, true, on_device);
}

extern "C" int32_t esp_precon_cholesky_tree(esp_precon *p, int32_t *level, int64_t *node_root, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_CHOLESKY) return ESP_ERR_INVALID;
    CK(chol_current(p, "esp_precon_cholesky_tree"));
    if (level) CK(lu_export(p->h, p->lu_level, level, false, on_device));
    if (node_root) CK(lu_export(p->h, p->lu_root, node_root, true, on_device));
    return ESP_OK;
}

extern "C" int32_t esp_precon_cholesky_factor(esp_precon *p, int64_t *colptr, int64_t *rowval, double *nzval, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_CHOLESKY) return ESP_ERR_INVALID;
    esp_handle *h = p->h;
    CK(chol_current(p, "esp_precon_cholesky_factor"));
    (void)hipSetDevice(h->device);
    CholData *c = p->chol;
    const i64 n = p->n;
    if (colptr) CK(copy_out(h, colptr, c->lcp.p, sizeof(i64) * (size_t)(n + 1), on_device));
    if (n == 0 || (!rowval && !nzval)) return ESP_OK;
    Temps tmp;
    DevBuf &rv = tmp.b[0], &nz = tmp.b[1];
    i64 *drv = nullptr;
    double *dnz = nullptr;
    if (rowval) {
        if (on_device) drv = rowval;
        else {
            CK(ensure(h, rv, sizeof(i64) * (size_t)c->nnzL));
            drv = (i64 *)rv.p;
        }
    }
    if (nzval) {
        if (on_device) dnz = nzval;
        else {
            CK(ensure(h, nz, sizeof(double) * (size_t)c->nnzL));
            dnz = (double *)nz.p;
        }
    }
    hipLaunchKernelGGL(chol_export_k, dim3(grid_for(n, CT)), dim3(CT), 0, h->stream, dev_of(c), (const u32 *)c->nodeof.p, (const i64 *)c->lcp.p, n, drv, dnz);
    HIPCK(h, hipGetLastError());
    if (!on_device) {
        if (rowval) CK(copy_out(h, rowval, drv, sizeof(i64) * (size_t)c->nnzL, 0));
        if (nzval) CK(copy_out(h, nzval, dnz, sizeof(double) * (size_t)c->nnzL, 0));
    }
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}

extern "C" int32_t esp_precon_cholesky_stats(esp_precon *p, int64_t out[ESP_CHOL_STATS]) {
    if (!p || p->kind != ESP_PRECON_CHOLESKY || !out || !p->chol) return ESP_ERR_INVALID;
    for (int k = 0; k < ESP_CHOL_STATS; k++) out[k] = p->chol->stats[k];
    return ESP_OK;
}

extern "C" int32_t esp_debug_cholesky_wide_from(esp_handle *h, int64_t w) {
    if (!h || w < 0) return ESP_ERR_INVALID;
    h->debug_chol_wide = w;
    return ESP_OK;
}
