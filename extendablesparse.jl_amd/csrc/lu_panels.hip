// lu_panels.hip -- libesparse_hip: the panel form of LUFactorization (esp_precon_lu_create_form, ESP_LU_PANELS): ILUAM's chains over
// the filled matrix B, walked on dense panels per tree node instead of column by column
// (see internal.hpp for the map of the translation units)
//
// The rule is stated in include/esparse_hip.h next to esp_precon_lu_create and in DESIGN.md 5s.  Nothing numerical is new: entry (k, j)
// of B is ONE chain t = b_kj - sum over i < min(k, j) ascending, (i, j) and (k, i) in B's pattern, of u_ij * l_ki (each product
// rounded, each difference rounded), and l_kj = t / u_jj below the diagonal (tests/iluam_model.c).  (i, j) and (k, i) lie in the
// pattern exactly when i belongs to a descendant J with j and k in node(J) + struct(J), or to the entry's own node: the predicate
// of cholesky.hip's chain.  Any schedule that walks the chains in this order gives the bits of the column form; this one walks the
// tree depth by depth, as cholesky.hip does, on the tables of panels.hpp.
//
//   panels     node K (width w, h = |struct(K)|) owns TWO (w + h) x w column-major panels at the same offset of two halves of one
//              allocation: PL[r, j] = B[row r, K_j] for r >= j (L, u_jj on the diagonal) and PU[r, j] = B[K_j, row r] for r > j
//              (U transposed); row r < w is K's r-th position, row w + f the f-th entry of struct(K).  The rest stays zero, unread.
//   load       lup_move_k<true>: the panels are zeroed, then one wave per column of B scatters its values; <false> reads them back
//              into B's position order (esp_precon_get_factor).  A position outside struct(K) is skipped, never written.
//   update     update_tile: a workgroup owns a TR x NB tile of a block column of PL or PU (a run-time flag: one body), 2 x 4
//              accumulators per lane.  Per descendant J of the update list, ascending: the panel rows in J of the tile's rows and
//              columns (bisection), then J's columns i ascending, KB at a time through LDS: the rows' slice from the panel of the
//              tile's own kind, the columns' slice from the other one; acc = acc - u * l.  K's own columns in front of the block
//              column come last.  An accumulator whose row or column J does not hold is skipped by a predicate.
//   factor     factor_diag: the NB x NB diagonal block (lower triangle from PL, upper from PU) right-looking in LDS over both
//              triangles, no pivot test, by the workgroup that updated both tiles holding it.  factor_rows: one lane per row
//              below, the row in LDS: PL rows run the chain against the block's U and divide, PU rows against its unit-lower L.
//   forms      small (w < wide_from): lup_small_k, a workgroup per node, every small node of a depth in one launch.  wide:
//              lup_update_k / lup_factor_k per block column for all wide nodes of the depth at once.  The same device functions.
//   solve      ILUAM's orders.  yb = v[c]; forward per depth from the deepest up (lup_fwd_k: acc = 0, the descendants' l_jk y_k
//              in ascending k, the node's triangle right-looking, the right-hand side added last); backward per depth from 0 down
//              (lup_bwd_k: acc = y_j, struct(K) from its last entry down, the triangle from the last position up, the division
//              last); scatter.  Launches on the handle's stream and nothing else.
#include "panels.hpp"

using namespace espamg;
using namespace esplu;
using namespace esppanel;

struct LuPanelData : PanelTree {
    DevBuf panels, y2;  // PL of every node, then PU of every node (2 * panel_doubles); the triangles wider than TRI_LDS
    DevBuf bm, ym, y2m;  // the work vectors of the chunked solves, n * RC doubles each, from the first esp_precon_ldiv_many on
    i64 stats[ESP_LU_PANEL_STATS] = {0};
};

namespace {

struct Dev {
    const CholNode *nodes;
    const u32 *ulist;
    const i64 *srv;
    double *pl, *pu;
};

// the panel row of position pos in K, or -1
__device__ __forceinline__ i64 row_in(const Dev &d, const CholNode &K, u32 pos) {
    if (pos >= K.start && pos < K.start + K.w) return (i64)(pos - K.start);
    const int f = struct_find(d.srv, K, pos);
    return f < 0 ? -1 : (i64)K.w + f;
}

// ---- load / export -------------------------------------------------------------------------------------------------------------------
// one wave per column k of B (bcp, brv: 1-based).  LOAD: the panels take bnz; else out takes the panels, in B's position order
template <bool LOAD>
__global__ __launch_bounds__(CT) void lup_move_k(Dev d, const i64 *__restrict__ bcp, const i64 *__restrict__ brv, const double *__restrict__ bnz,
                                                 const u32 *__restrict__ nodeof, i64 n, double *__restrict__ out) {
    const i64 k = (i64)blockIdx.x * (CT / 64) + (threadIdx.x >> 6);
    if (k >= n) return;
    const int lane = threadIdx.x & 63;
    const CholNode Kc = d.nodes[nodeof[k]];
    for (i64 q = bcp[k] - 1 + lane; q < bcp[k + 1] - 1; q += 64) {
        const i64 r = brv[q] - 1;
        double *slot = nullptr;
        if (r >= k) {  // l_rk, or the diagonal u_kk: column k of its own node's PL
            const i64 row = row_in(d, Kc, (u32)r);
            if (row >= 0) slot = d.pl + Kc.off + (k - Kc.start) * ((i64)Kc.w + Kc.h) + row;
        } else {       // u_rk: column r of PU of r's node, at k's row
            const CholNode K = d.nodes[nodeof[r]];
            const i64 row = row_in(d, K, (u32)k);
            if (row >= 0) slot = d.pu + K.off + (r - K.start) * ((i64)K.w + K.h) + row;
        }
        if (LOAD) {
            if (slot) *slot = bnz[q];
        } else {
            out[q] = slot ? *slot : bnz[q];
        }
    }
}

// ---- update --------------------------------------------------------------------------------------------------------------------------
struct TileLds {
    double a[KB][TR];   // the rows' slice of a descendant's panel
    double b[KB][NB];   // the columns' slice (of its other panel)
    int ri[TR], rj[NB]; // the panel row in the descendant of every tile row / column, -1: none
    u32 pos[TR];        // the position of every tile row
};

// acc -= u * l over the columns [0, kcount) of a descendant, k ascending: the rows' values from baseA, the columns' from baseB (both
// panels of one node: ld).  A PU tile's rows carry u and its columns l, a PL tile's the other way round: one product either way
__device__ __forceinline__ void tile_apply(TileLds &L, const double *__restrict__ baseA, const double *__restrict__ baseB, i64 ld, u32 kcount,
                                           double (&acc)[2][4]) {
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
            L.a[kk][r] = (kk < kn && row >= 0) ? baseA[(i64)(k0 + kk) * ld + row] : 0.0;
        }
        for (int e = tid; e < KB * NB; e += CT) {
            const int kk = e / NB, c = e % NB;
            const int row = L.rj[c];
            L.b[kk][c] = (kk < kn && row >= 0) ? baseB[(i64)(k0 + kk) * ld + row] : 0.0;
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

// the tile of K's PL (up = false) or PU: columns [c0, c0 + nc), rows [r0, r0 + TR) (r0 >= c0): every chain up to the columns in front
// of c0.  Every lane of the workgroup calls it (up is a run-time flag: one body serves both panels)
__device__ void update_tile(const Dev &d, const CholNode &K, u32 c0, u32 nc, u32 r0, TileLds &L, bool up) {
    const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
    const i64 ld = (i64)K.w + K.h;
    double *const rowsP = up ? d.pu : d.pl, *const colsP = up ? d.pl : d.pu;  // where the rows' and the columns' values of a descendant lie
    double *P = rowsP + K.off;
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
            const int f = pos == LU_NONE ? -1 : struct_find(d.srv, J, pos);
            L.ri[tid] = f < 0 ? -1 : (int)J.w + f;
        } else if (tid < TR + NB) {
            const u32 c = (u32)(tid - TR);
            const int f = c < nc ? struct_find(d.srv, J, K.start + c0 + c) : -1;
            L.rj[c] = f < 0 ? -1 : (int)J.w + f;
            mine = f >= 0;
        }
        if (!__syncthreads_or(mine)) continue;  // (no column of the block column lies in struct(J): nothing to subtract)
        tile_apply(L, rowsP + J.off, colsP + J.off, (i64)J.w + J.h, J.w, acc);
        __syncthreads();
    }
    if (c0 > 0) {  // K's own columns in front of the block column
        if (tid < TR) L.ri[tid] = L.pos[tid] == LU_NONE ? -1 : (int)(r0 + tid);
        else if (tid < TR + NB) L.rj[tid - TR] = (u32)(tid - TR) < nc ? (int)(c0 + tid - TR) : -1;
        __syncthreads();
        tile_apply(L, P, colsP + K.off, ld, c0, acc);
    }
#pragma unroll
    for (int rr = 0; rr < 2; rr++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const i64 r = (i64)r0 + tx + 32 * rr;
            const u32 cc = (u32)(ty * 4 + c);
            if (r < ld && cc < nc && r >= (i64)(c0 + cc) + (up ? 1 : 0)) P[(i64)(c0 + cc) * ld + r] = acc[rr][c];
        }
}

// ---- factor --------------------------------------------------------------------------------------------------------------------------
struct FactorLds {
    double D[NB][NB + 1];  // D[i][j] = the block's entry (row i, column j): l_ij below the diagonal, u_ij on and above it
};
struct RowLds {
    double X[NB][FR];  // the rows below, one per lane
};

// F.D = the diagonal block of the block column [c0, c0 + nc) of K, as the panels hold it (tr: transposed)
__device__ __forceinline__ void diag_read(const Dev &d, const CholNode &K, u32 c0, u32 nc, FactorLds &F, bool tr) {
    const i64 ld = (i64)K.w + K.h;
    const double *PL = d.pl + K.off, *PU = d.pu + K.off;
    for (int e = threadIdx.x; e < NB * NB; e += CT) {
        const u32 i = (u32)(e % NB), j = (u32)(e / NB);
        double v = 0.0;
        if (i < nc && j < nc) v = i >= j ? PL[(i64)(c0 + j) * ld + c0 + i] : PU[(i64)(c0 + i) * ld + c0 + j];
        if (tr) F.D[j][i] = v;
        else F.D[i][j] = v;
    }
}

// the diagonal block, updated: right-looking in LDS over both triangles, stored back.  No pivot test: a zero pivot gives the Inf and
// NaN the column form gives.  Every lane of the workgroup calls it
__device__ void factor_diag(const Dev &d, const CholNode &K, u32 c0, u32 nc, FactorLds &F) {
    const int tid = threadIdx.x;
    const i64 ld = (i64)K.w + K.h;
    double *PL = d.pl + K.off, *PU = d.pu + K.off;
    __syncthreads();
    diag_read(d, K, c0, nc, F, false);
    __syncthreads();
    for (u32 k = 0; k + 1 < nc; k++) {
        if ((u32)tid > k && (u32)tid < nc) F.D[tid][k] = F.D[tid][k] / F.D[k][k];
        __syncthreads();
        const u32 i = (u32)(tid >> 3);
        if (i > k && i < nc) {
            const double lik = F.D[i][k];
            for (u32 j = k + 1 + (u32)(tid & 7); j < nc; j += 8) {
                const double pr = F.D[k][j] * lik;
                F.D[i][j] = F.D[i][j] - pr;
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < NB * NB; e += CT) {
        const u32 i = (u32)(e % NB), j = (u32)(e / NB);
        if (i < nc && j < nc) {
            if (i >= j) PL[(i64)(c0 + j) * ld + c0 + i] = F.D[i][j];
            else PU[(i64)(c0 + i) * ld + c0 + j] = F.D[i][j];
        }
    }
}

// the rows [rb, re), re - rb <= FR, below the factored diagonal block (read from the panels) of PL (up = false: the chain against the
// block's U, then the division) or PU (the chain against its unit-lower L): one lane per row, the row in LDS.  For PU the block is
// read transposed, so that both chains run over F.D[k][j].  Every lane of the workgroup calls it
__device__ void factor_rows(const Dev &d, const CholNode &K, u32 c0, u32 nc, i64 rb, i64 re, FactorLds &F, RowLds &R, bool up) {
    const int tid = threadIdx.x;
    const i64 ld = (i64)K.w + K.h;
    double *P = (up ? d.pu : d.pl) + K.off;
    __syncthreads();
    diag_read(d, K, c0, nc, F, up);
    __syncthreads();
    const i64 r = rb + tid;
    if (tid < FR && r < re) {
        for (u32 j = 0; j < nc; j++) R.X[j][tid] = P[(i64)(c0 + j) * ld + r];
        for (u32 j = 0; j < nc; j++) {
            double t = R.X[j][tid];
            for (u32 k = 0; k < j; k++) {
                const double pr = F.D[k][j] * R.X[k][tid];
                t = t - pr;
            }
            if (!up) t = t / F.D[j][j];
            R.X[j][tid] = t;
            P[(i64)(c0 + j) * ld + r] = t;
        }
    }
}

// the small form: a workgroup per node of list[0 .. count)
__global__ __launch_bounds__(CT) void lup_small_k(Dev d, const u32 *__restrict__ list) {
    __shared__ TileLds L;
    __shared__ FactorLds F;
    __shared__ RowLds R;
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    for (u32 c0 = 0; c0 < K.w; c0 += NB) {
        const u32 nc = min((u32)NB, K.w - c0);
        for (i64 r0 = c0; r0 < ld; r0 += TR)
            for (int up = 0; up < 2; up++) update_tile(d, K, c0, nc, (u32)r0, L, up != 0);
        __threadfence_block();
        factor_diag(d, K, c0, nc, F);
        __threadfence_block();
        for (i64 rb = (i64)c0 + nc; rb < ld; rb += FR)
            for (int up = 0; up < 2; up++) factor_rows(d, K, c0, nc, rb, min(rb + FR, ld), F, R, up != 0);
        __threadfence_block();
    }
}
// the wide form, block column bc of the nodes list[0 .. count): 2 * tiles - 1 workgroups per node.  Workgroup 0 owns the first tile
// of BOTH panels -- together they hold the whole diagonal block (NB <= TR) and no other tile touches it -- and factorizes the block;
// 1 .. tiles - 1 own a tile of PL, tiles .. 2 * tiles - 2 one of PU
__global__ __launch_bounds__(CT) void lup_update_k(Dev d, const u32 *__restrict__ list, u32 bc, u32 tiles) {
    __shared__ TileLds L;
    __shared__ FactorLds F;
    const u32 per = 2 * tiles - 1, t = blockIdx.x % per;
    const CholNode K = d.nodes[list[blockIdx.x / per]];
    const u32 c0 = bc * NB, nc = min((u32)NB, K.w - c0);
    const bool up = t >= tiles;
    const i64 r0 = (i64)c0 + (i64)(up ? t - tiles + 1 : t) * TR;
    if (r0 >= (i64)K.w + K.h) return;
    update_tile(d, K, c0, nc, (u32)r0, L, up);
    if (t != 0) return;
    update_tile(d, K, c0, nc, (u32)r0, L, true);
    __threadfence_block();
    factor_diag(d, K, c0, nc, F);
}
// ... the rows below: 2 * tiles workgroups per node, PL's then PU's
__global__ __launch_bounds__(CT) void lup_factor_k(Dev d, const u32 *__restrict__ list, u32 bc, u32 tiles) {
    __shared__ FactorLds F;
    __shared__ RowLds R;
    const u32 per = 2 * tiles, t = blockIdx.x % per;
    const CholNode K = d.nodes[list[blockIdx.x / per]];
    const u32 c0 = bc * NB, nc = min((u32)NB, K.w - c0);
    const bool up = t >= tiles;
    const i64 ld = (i64)K.w + K.h, rb = (i64)c0 + nc + (i64)(up ? t - tiles : t) * FR;
    if (rb >= ld) return;
    factor_rows(d, K, c0, nc, rb, min(rb + FR, ld), F, R, up);
}

// ---- solve ---------------------------------------------------------------------------------------------------------------------------
// forward: a workgroup per node of list; b = v[c], y the result.  t lives in LDS (w <= TRI_LDS) or in y2
__global__ __launch_bounds__(CT) void lup_fwd_k(Dev d, const u32 *__restrict__ list, const double *__restrict__ b, double *y, double *y2) {
    __shared__ double sh[TRI_LDS];
    const int tid = threadIdx.x;
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    const double *P = d.pl + K.off;
    double *t = K.w <= (u32)TRI_LDS ? sh : y2 + K.start;
    for (u32 j = (u32)tid; j < K.w; j += CT) {
        double a = 0.0;
        for (u32 u = K.ub; u < K.ue; u++) {
            const CholNode J = d.nodes[d.ulist[u]];
            const int f = struct_find(d.srv, J, K.start + j);
            if (f < 0) continue;
            const i64 ldj = (i64)J.w + J.h;
            const double *R = d.pl + J.off + J.w + f;
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
        const double yk = t[k] + b[K.start + k];  // (the right-hand side comes last)
        if (tid == 0) y[K.start + k] = yk;
        for (u32 i = k + 1 + (u32)tid; i < K.w; i += CT) {
            const double pr = P[(i64)k * ld + i] * yk;
            t[i] = t[i] - pr;
        }
    }
}
// backward, in place on y: struct(K) from its last entry down, then the triangle from the last position up
__global__ __launch_bounds__(CT) void lup_bwd_k(Dev d, const u32 *__restrict__ list, double *y, double *y2) {
    __shared__ double sh[TRI_LDS];
    const int tid = threadIdx.x;
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    const double *PL = d.pl + K.off, *PU = d.pu + K.off;
    const i64 *st = d.srv + K.sbase;
    double *t = K.w <= (u32)TRI_LDS ? sh : y2 + K.start;
    for (u32 j = (u32)tid; j < K.w; j += CT) {
        double a = y[K.start + j];
        const double *C = PU + (i64)j * ld + K.w;
        for (u32 i = K.h; i-- > 0;) {
            const double pr = C[i] * y[st[i] - 1];
            a = a - pr;
        }
        t[j] = a;
    }
    for (u32 k = K.w; k-- > 0;) {
        __syncthreads();
        const double xk = t[k] / PL[(i64)k * ld + k];
        if (tid == 0) y[K.start + k] = xk;
        for (u32 j = (u32)tid; j < k; j += CT) {
            const double pr = PU[(i64)j * ld + k] * xk;
            t[j] = t[j] - pr;
        }
    }
}

// ---- solve, several right-hand sides -----------------------------------------------------------------------------------
// lup_fwd_k over nr <= RC right-hand sides at once: b, y and y2 hold RC doubles per position (y[pos * RC + r]); a lane owns right-hand
// side r = tid % RC of the rows slot, slot + RR, ... of the node and walks lup_fwd_k's chain for that pair (cholesky.hip's
// chol_fwd_many_k states the layout)
__global__ __launch_bounds__(CT) void lup_fwd_many_k(Dev d, const u32 *__restrict__ list, const double *__restrict__ b, double *y, double *y2, int nr) {
    __shared__ double sh[TRI_LDS_MANY * RC];
    const ManyLane m = many_lane(nr);
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    const double *P = d.pl + K.off;
    double *t = K.w <= (u32)TRI_LDS_MANY ? sh : y2 + (i64)K.start * RC;
    for (u32 j0 = 0; j0 < K.w; j0 += RR) {  // (uniform over the workgroup: the shuffle of many_found needs every lane)
        const u32 j = j0 + (u32)m.slot;
        const bool valid = j < K.w;
        double a = 0.0;
        for (u32 u0 = K.ub; u0 < K.ue; u0 += RC) {
            const int mine = struct_find_spread(d.nodes, d.ulist, d.srv, u0, K.ue, K.start + j, valid, m);
            for (int q = 0; q < RC && u0 + q < K.ue; q++) {  // the update list ascending, as lup_fwd_k walks it
                const int f = many_found(mine, q, m);
                if (f < 0 || !m.on) continue;
                const CholNode J = d.nodes[d.ulist[u0 + q]];
                const i64 ldj = (i64)J.w + J.h;
                const double *R = d.pl + J.off + J.w + f;
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
        const double yk = t[(i64)k * RC + m.r] + b[(i64)(K.start + k) * RC + m.r];  // (the right-hand side comes last)
        if (m.slot == 0) y[(i64)(K.start + k) * RC + m.r] = yk;
        for (u32 i = k + 1 + (u32)m.slot; i < K.w; i += RR) {
            const double pr = P[(i64)k * ld + i] * yk;
            t[(i64)i * RC + m.r] = t[(i64)i * RC + m.r] - pr;
        }
    }
}
// lup_bwd_k in the same way
__global__ __launch_bounds__(CT) void lup_bwd_many_k(Dev d, const u32 *__restrict__ list, double *y, double *y2, int nr) {
    __shared__ double sh[TRI_LDS_MANY * RC];
    const ManyLane m = many_lane(nr);
    const CholNode K = d.nodes[list[blockIdx.x]];
    const i64 ld = (i64)K.w + K.h;
    const double *PL = d.pl + K.off, *PU = d.pu + K.off;
    const i64 *st = d.srv + K.sbase;
    double *t = K.w <= (u32)TRI_LDS_MANY ? sh : y2 + (i64)K.start * RC;
    if (m.on)
        for (u32 j = (u32)m.slot; j < K.w; j += RR) {
            double a = y[(i64)(K.start + j) * RC + m.r];
            const double *C = PU + (i64)j * ld + K.w;
            for (u32 i = K.h; i-- > 0;) {
                const double pr = C[i] * y[(st[i] - 1) * RC + m.r];
                a = a - pr;
            }
            t[(i64)j * RC + m.r] = a;
        }
    for (u32 k = K.w; k-- > 0;) {
        __syncthreads();
        if (!m.on) continue;
        const double xk = t[(i64)k * RC + m.r] / PL[(i64)k * ld + k];
        if (m.slot == 0) y[(i64)(K.start + k) * RC + m.r] = xk;
        for (u32 j = (u32)m.slot; j < k; j += RR) {
            const double pr = PU[(i64)j * ld + k] * xk;
            t[(i64)j * RC + m.r] = t[(i64)j * RC + m.r] - pr;
        }
    }
}

Dev dev_of(const LuPanelData *c) {
    double *pl = (double *)c->panels.p;
    return Dev{(const CholNode *)c->nodes.p, (const u32 *)c->ulist.p, c->S ? (const i64 *)c->S->rowval.p : nullptr, pl, pl + c->panel_doubles};
}

}  // namespace

void lup_drop(LuPanelData *c) {
    if (!c) return;
    tree_drop(*c);
    release(c->panels);
    for (DevBuf *b : {&c->y2, &c->bm, &c->ym, &c->y2m}) release(*b);
    delete c;
}

// the tables and the zero-filled layout of the panels for the ordered tree o (lu.hip's build_b calls it behind its last refusal, in
// front of everything it installs): a new LuPanelData, p untouched
int32_t lup_symbolic(esp_precon *p, Order &o, Handles &hs, const Struct &x, LuPanelData **out) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    LuPanelData *c = new LuPanelData();
    struct Guard {
        LuPanelData *c;
        ~Guard() { lup_drop(c); }
    } guard{c};
    const u32 wide_from = h->debug_lu_wide > 0 ? (u32)std::min<i64>(h->debug_lu_wide, 0xFFFFFFFFll) : (u32)NB + 1;
    CK(tree_build(h, o, hs, x, "esp_precon_lu", wide_from, *c));
    c->host_nodes.clear();
    for (const CholDepth &D : c->depth)
        for (const CholLaunch &Lc : D.wide)
            if (2 * (i64)Lc.count * std::max(Lc.tiles_u, Lc.tiles_f) > 0x7FFFFFFFll) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_lu: a depth's grid exceeds 2^31 workgroups");
    CK(ensure(h, c->panels, sizeof(double) * (size_t)std::max<i64>(2 * c->panel_doubles, 1)));
    CK(ensure(h, c->y2, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    i64 *st = c->stats;
    st[0] = 2 * c->panel_doubles;
    i64 solve = n > 0 ? 2 : 0;
    for (const CholDepth &D : c->depth) solve += D.all_count ? 2 : 0;
    st[2] = solve;
    st[3] = c->nsmall;
    st[4] = c->nwide;
    st[5] = c->nbcols;
    guard.c = nullptr;
    *out = c;
    return ESP_OK;
}

// the load from B's current values and the numeric factorization: launches on the handle's stream only
int32_t lup_numeric(esp_precon *p) {
    esp_handle *h = p->h, *bh = p->der.bh;
    hipStream_t s = h->stream;
    const i64 n = p->n;
    LuPanelData *c = p->lup;
    i64 launches = 0;
    if (n > 0) {
        const Dev d = dev_of(c);
        HIPCK(h, hipMemsetAsync(c->panels.p, 0, sizeof(double) * (size_t)(2 * c->panel_doubles), s));
        hipLaunchKernelGGL(lup_move_k<true>, dim3(grid_for(n, CT / 64)), dim3(CT), 0, s, d, (const i64 *)bh->colptr.p, (const i64 *)bh->rowval.p,
                           (const double *)bh->nzval.p, (const u32 *)c->nodeof.p, n, (double *)nullptr);
        launches++;
        const u32 *flist = (const u32 *)c->flist.p;
        for (size_t dep = c->depth.size(); dep-- > 0;) {
            const CholDepth &D = c->depth[dep];
            if (D.small_count) {
                hipLaunchKernelGGL(lup_small_k, dim3(D.small_count), dim3(CT), 0, s, d, flist + D.small_first);
                launches++;
            }
            for (const CholLaunch &Lc : D.wide) {
                hipLaunchKernelGGL(lup_update_k, dim3(Lc.count * (2 * Lc.tiles_u - 1)), dim3(CT), 0, s, d, flist + Lc.first, Lc.bc, Lc.tiles_u);
                hipLaunchKernelGGL(lup_factor_k, dim3(Lc.count * 2 * Lc.tiles_f), dim3(CT), 0, s, d, flist + Lc.first, Lc.bc, Lc.tiles_f);
                launches += 2;
            }
        }
        HIPCK(h, hipGetLastError());
    }
    c->stats[1] = launches;
    return ESP_OK;
}

// u = B's LU \ v in A's numbering on device vectors (u may be v; sub: u[i] = u[i] - x[i], simple!'s step)
int32_t lup_solve(esp_precon *p, const double *v, double *u, bool sub) {
    esp_handle *h = p->h;
    hipStream_t s = h->stream;
    const i64 n = p->n;
    LuPanelData *c = p->lup;
    if (n == 0) return ESP_OK;
    const Dev d = dev_of(c);
    const u32 *perm = (const u32 *)p->lu_perm.p, *dlist = (const u32 *)c->dlist.p;
    double *b = (double *)p->blk_t.p, *y = (double *)p->blk_s.p, *y2 = (double *)c->y2.p;
    const unsigned g = grid_for(n, CT);
    hipLaunchKernelGGL(panel_gather_k, dim3(g), dim3(CT), 0, s, perm, v, b, n);
    for (size_t dep = c->depth.size(); dep-- > 0;) {
        const CholDepth &D = c->depth[dep];
        if (D.all_count) hipLaunchKernelGGL(lup_fwd_k, dim3(D.all_count), dim3(CT), 0, s, d, dlist + D.all_first, (const double *)b, y, y2);
    }
    for (size_t dep = 0; dep < c->depth.size(); dep++) {
        const CholDepth &D = c->depth[dep];
        if (D.all_count) hipLaunchKernelGGL(lup_bwd_k, dim3(D.all_count), dim3(CT), 0, s, d, dlist + D.all_first, y, y2);
    }
    hipLaunchKernelGGL(panel_scatter_k, dim3(g), dim3(CT), 0, s, perm, (const double *)y, u, n, sub);
    return ESP_OK;
}

// U[:, r] = B's LU \ V[:, r] for k columns on device arrays (U may be V where ldu == ldv), RC columns per pass over the panels
int32_t lup_solve_many(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, i64 k) {
    esp_handle *h = p->h;
    hipStream_t s = h->stream;
    const i64 n = p->n;
    LuPanelData *c = p->lup;
    if (n == 0 || k == 0) return ESP_OK;
    for (DevBuf *w : {&c->bm, &c->ym, &c->y2m}) CK(ensure(h, *w, sizeof(double) * (size_t)n * RC));
    const Dev d = dev_of(c);
    const u32 *perm = (const u32 *)p->lu_perm.p, *dlist = (const u32 *)c->dlist.p;
    double *b = (double *)c->bm.p, *y = (double *)c->ym.p, *y2 = (double *)c->y2m.p;
    const unsigned g = grid_for(n * RC, CT);
    for (i64 r0 = 0; r0 < k; r0 += RC) {
        const int nr = (int)std::min<i64>(RC, k - r0);
        hipLaunchKernelGGL(panel_gather_many_k, dim3(g), dim3(CT), 0, s, perm, v + r0 * ldv, ldv, b, n, nr);
        for (size_t dep = c->depth.size(); dep-- > 0;) {
            const CholDepth &D = c->depth[dep];
            if (D.all_count) hipLaunchKernelGGL(lup_fwd_many_k, dim3(D.all_count), dim3(CT), 0, s, d, dlist + D.all_first, (const double *)b, y, y2, nr);
        }
        for (size_t dep = 0; dep < c->depth.size(); dep++) {
            const CholDepth &D = c->depth[dep];
            if (D.all_count) hipLaunchKernelGGL(lup_bwd_many_k, dim3(D.all_count), dim3(CT), 0, s, d, dlist + D.all_first, y, y2, nr);
        }
        hipLaunchKernelGGL(panel_scatter_many_k, dim3(g), dim3(CT), 0, s, perm, (const double *)y, u + r0 * ldu, ldu, n, nr);
    }
    return ESP_OK;
}

// esp_precon_get_factor of the panel form: nnz(B) doubles in B's position order, exported from the panels
int32_t lup_factor(esp_precon *p, double *nzval, int32_t on_device) {
    esp_handle *h = p->h, *bh = p->der.bh;
    const i64 n = p->n, nnzB = bh->nnz;
    (void)hipSetDevice(h->device);
    if (n == 0 || nnzB == 0) return ESP_OK;
    Temps tmp;
    double *out = nzval;
    if (!on_device) {
        CK(ensure(h, tmp.b[0], sizeof(double) * (size_t)nnzB));
        out = (double *)tmp.b[0].p;
    }
    hipLaunchKernelGGL(lup_move_k<false>, dim3(grid_for(n, CT / 64)), dim3(CT), 0, h->stream, dev_of(p->lup), (const i64 *)bh->colptr.p,
                       (const i64 *)bh->rowval.p, (const double *)bh->nzval.p, (const u32 *)p->lup->nodeof.p, n, out);
    HIPCK(h, hipGetLastError());
    if (!on_device) CK(copy_out(h, nzval, out, sizeof(double) * (size_t)nnzB, 0));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}

extern "C" int32_t esp_precon_lu_panel_stats(esp_precon *p, int64_t out[ESP_LU_PANEL_STATS]) {
    if (!p || p->kind != ESP_PRECON_LU || !out || !p->lup) return ESP_ERR_INVALID;
    for (int k = 0; k < ESP_LU_PANEL_STATS; k++) out[k] = p->lup->stats[k];
    return ESP_OK;
}

extern "C" int32_t esp_debug_lu_wide_from(esp_handle *h, int64_t w) {
    if (!h || w < 0) return ESP_ERR_INVALID;
    h->debug_lu_wide = w;
    return ESP_OK;
}
