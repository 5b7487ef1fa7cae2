// iluam.hip -- libesparse_hip: ILUAMPreconditioner on the device CSC (see internal.hpp for the map of the translation units)
//
// The reference (src/experimental/ExtendableSparseMatrixParallel/iluam.jl, ilu_Al-Kurdi_Mittal.jl) is three sequential loops:
//   iluAM (lines 68-120): nzval = copy(A.nzval); for j = 1:n { for every position v of column j above the diagonal (row
//     i = rowval[v], increasing), for every position w of column i below ITS diagonal whose row is stored in column j at
//     position k: nzval[k] -= nzval[v]*nzval[w];  then nzval[v] /= nzval[diag[j]] for every v of column j below the diagonal }
//   forward  (122-140): y .= 0; for j = 1:n { y[j] += b[j]; y[i] -= nzval[v]*y[j] for the rows i below the diagonal }
//   backward (143-157): for j = n:-1:1 { x[j] = y[j]/nzval[diag[j]]; y[i] -= nzval[v]*x[j] for the rows i above it }
// All three carry true dependencies, so none is a grid-wide pass.  What makes them parallel AND bit-identical:
//   - column j of the factorization writes only its own positions and reads, besides them, only the finished columns i < j
//     with a stored A[i,j]; inside the column the order over v is kept (nzval[v] may have been updated by an earlier v);
//   - seen by row, y[i] = ((0 - l_ij1*y[j1]) - l_ij2*y[j2] - ...) + b[i] with the stored j < i in INCREASING order, and
//     x[i] = ((y[i] - u_ij1*x[j1]) - ...)/u_ii with the stored j > i in DECREASING order: one ordered gather over finished rows.
// So each of the three runs level by level -- a node's level is one more than the highest level it depends on -- in any
// order inside a level.  Levels are separated by kernel boundaries on the handle's stream and by nothing else; consecutive
// levels that together fit one workgroup share a single-workgroup launch with __syncthreads() between them.
//
// Analysis (after a pattern change, all on the device): diagonal positions and the row parts from the split build of
// precon.hip (lower part increasing, upper part decreasing column); then per schedule an in-degree propagation -- one
// launch per level over the level's members, one counter read back per level -- and a stable radix sort of the nodes by
// level, which leaves every level's members ascending; last the row parts are permuted into that order, so that the lanes
// of a level stream one contiguous slice (measured at 256^3: ldiv! 8.3 ms against 11.2 ms with the parts in row order, for
// 2 ms more per factorization, whose value gather then reads the factor scattered).  A values-only update! keeps all of it.
//
// Prefactored mode (esp_precon::prefactored, set by ilut.hip on its inner preconditioner): the handle's values are a factorization
// already.  The diagonal positions, the row parts and the two solve schedules are built as above; the factor schedule is not, and
// FactorOp does not run: fval is a copy of the handle's values, and a values-only update! is that copy and the gather.
//
// Several right-hand sides (iluam_solve_many): a chunk of up to ESP_MANY_CHUNK columns goes through the two solve
// schedules in ONE pass -- the launch lists as they are, ESP_MANY_CHUNK adjacent lanes per row, the scratch interleaved.
//
// esp_debug_iluam_form (a test hook) forces FactorOp or FactorWaveOp at the next update!, and esp_debug_last_iluam_form tells which ran.
#include "internal.hpp"

namespace {

constexpr int LT = 256;  // threads per workgroup; also the most members the levels of one thin launch hold together

enum { S_FACTOR = 0, S_FWD = 1, S_BWD = 2 };

struct Pattern {
    const i64 *colptr, *rowval;  // the CSC, 1-based
    const u32 *dpos;             // position of (j,j), 0-based
    const u32 *lptr, *uptr, *ucol;
};

// ---- level analysis --------------------------------------------------------------------------------------------
// S_FACTOR: node = column j, waits for the columns i < j with a stored (i,j); released by column i: the columns of row i's
//           upper part.  S_FWD: node = row i, waits for the rows j < i with a stored (i,j); released by row j: the rows
//           below the diagonal of column j.  S_BWD: the mirror image.
template <int S>
__device__ __forceinline__ u32 in_degree(const Pattern &g, i64 i) {
    if (S == S_FACTOR) return g.dpos[i] - (u32)(g.colptr[i] - 1);
    if (S == S_FWD) return g.lptr[i + 1] - g.lptr[i];
    return g.uptr[i + 1] - g.uptr[i];
}
template <int S>
__global__ void level_init_k(Pattern g, i64 n, u32 *__restrict__ indeg, u32 *__restrict__ level, u32 *__restrict__ front,
                             u32 *__restrict__ cnt) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 d = in_degree<S>(g, i);
    indeg[i] = d;
    if (d == 0) {
        level[i] = 0;
        front[atomicAdd(cnt, 1u)] = (u32)i;
    }
}
// one round: every member of the frontier releases its successors; a successor whose last dependency this was gets the
// level `lvl` and joins the next frontier (in arrival order: the sort below orders the members)
template <int S>
__global__ void level_expand_k(Pattern g, const u32 *__restrict__ front, u32 count, u32 *__restrict__ next, u32 *__restrict__ cnt_next,
                               u32 *__restrict__ cnt_done, u32 *__restrict__ indeg, u32 *__restrict__ level, u32 lvl) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) *cnt_done = 0;  // (the host has read it: the counter of the round after this one)
    if (t >= count) return;
    const u32 j = front[t];
    i64 b, e;
    if (S == S_FACTOR) b = g.uptr[j], e = g.uptr[j + 1];
    else if (S == S_FWD) b = (i64)g.dpos[j] + 1, e = g.colptr[j + 1] - 1;
    else b = g.colptr[j] - 1, e = g.dpos[j];
    for (i64 k = b; k < e; k++) {
        const u32 s = S == S_FACTOR ? g.ucol[k] : (u32)(g.rowval[k] - 1);
        if (atomicSub(&indeg[s], 1u) == 1u) {
            level[s] = lvl;
            next[atomicAdd(cnt_next, 1u)] = s;
        }
    }
}
__global__ void level_keys_k(const u32 *__restrict__ level, i64 n, u64 *__restrict__ key, double *__restrict__ payload) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = (u64)level[i] << ESP_TAG_BITS;
    payload[i] = __longlong_as_double((long long)i);
}
__global__ void level_order_k(const double *__restrict__ spayload, i64 n, u32 *__restrict__ order) {
    const i64 k = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) order[k] = (u32)__double_as_longlong(spayload[k]);
}

// ---- the work of one node ---------------------------------------------------------------------------------------
// column j of iluAM.  The reference's `point` array (row -> position in column j) is a two-pointer merge here: the rows of
// column i below its diagonal and the rows of column j are both ascending, and only rows > i can match.
// (every Op is called with a SLOT of its schedule: order[slot] is the node)
struct FactorOp {
    const u32 *order;
    const i64 *colptr, *rowval;
    const u32 *dpos;
    double *fval;  // (other columns are read, the own one written: no __restrict__)
    __device__ __forceinline__ void operator()(u32 slot) const {
        const u32 j = order[slot];
        const i64 cb = colptr[j] - 1, ce = colptr[j + 1] - 1, d = dpos[j];
        for (i64 v = cb; v < d; v++) {
            const i64 i = rowval[v] - 1;
            const double a = fval[v];
            i64 k = v + 1;
            const i64 we = colptr[i + 1] - 1;
            for (i64 w = (i64)dpos[i] + 1; w < we; w++) {
                const i64 r = rowval[w];
                while (k < ce && rowval[k] < r) k++;
                if (k == ce) break;
                if (rowval[k] == r) fval[k] = fval[k] - a * fval[w];
            }
        }
        const double piv = fval[d];
        for (i64 v = d + 1; v < ce; v++) fval[v] = fval[v] / piv;
    }
};
// The same column by a whole wave, for matrices whose columns are long (the filled matrices of ILU(k) and LUFactorization: a dense
// front of m columns costs one lane m*m*m/3 dependent steps).  The positions v above the diagonal stay one after the other -- a
// later one may read what an earlier one wrote --, but the updates of one v go to distinct positions k of column j: the lanes take
// the rows w of column i below its diagonal 64 at a time and find k by bisection among the rows of column j behind v (staged in LDS
// while the column holds at most FW_ROWS rows).  Every fval[k] meets the same operands in the same order as in FactorOp: the same
// bits.  Between two v the wave's stores are made visible to its own lanes by a workgroup-scope fence.
constexpr int FW_ROWS = 2048;   // rows of column j a wave stages in LDS (as u32: 8 KiB per wave)
constexpr int FW_MIN_AVG = 24;  // the wave form serves a matrix with at least this many entries per column on average
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
struct FactorWaveOp {
    const u32 *order;
    const i64 *colptr, *rowval;
    const u32 *dpos;
    double *fval;
    __device__ __forceinline__ void operator()(u32 slot, u32 *srow) const {
        const int lane = threadIdx.x & 63;
        const u32 j = order[slot];
        const i64 cb = colptr[j] - 1, ce = colptr[j + 1] - 1, d = dpos[j], len = ce - cb;
        const bool staged = len <= (i64)FW_ROWS;
        if (staged)
            for (i64 t = lane; t < len; t += 64) srow[t] = (u32)rowval[cb + t];
        wave_sync();
        for (i64 v = cb; v < d; v++) {
            const i64 i = rowval[v] - 1;
            const double a = fval[v];
            const i64 we = colptr[i + 1] - 1;
            for (i64 w = (i64)dpos[i] + 1 + lane; w < we; w += 64) {
                const i64 r = rowval[w];
                i64 lo = v + 1 - cb, hi = len;  // the first row of column j behind v that is not below r
                while (lo < hi) {
                    const i64 mid = lo + ((hi - lo) >> 1);
                    const i64 rm = staged ? (i64)srow[mid] : rowval[cb + mid];
                    if (rm < r) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < len && (staged ? (i64)srow[lo] : rowval[cb + lo]) == r) fval[cb + lo] = fval[cb + lo] - a * fval[w];
            }
            wave_sync();
        }
        const double piv = fval[d];
        for (i64 v = d + 1 + lane; v < ce; v += 64) fval[v] = fval[v] / piv;
    }
};
// forward row: y[i] = ((0 - l*y[j1]) - l*y[j2] - ...) + b[i].  The row parts lie in SLOT order (permute_part): the lanes
// of a level read one contiguous slice of pointers, columns and values.
// The statements of both rows are written ONCE, for the single-vector Ops and the many-column ones below: element j of the scratch
// is y[j * S] -- S = 1: the vector itself; S = MC: column d of the interleaved scratch, y = Y + d --, b is the right-hand side's
// own column.
template <int S>
__device__ __forceinline__ void forward_row(const u32 *lptr, const u32 *lcol, const double *lval, u32 slot, u32 i, const double *b, double *y) {
    double acc = 0.0;
    for (u32 k = lptr[slot], e = lptr[slot + 1]; k < e; k++) acc = acc - lval[k] * y[(u64)lcol[k] * S];
    y[(u64)i * S] = acc + b[i];
}
// ... the backward row's x[i], which the caller stores (xs: where the finished x[j] are read)
template <int S>
__device__ __forceinline__ double backward_row(const u32 *uptr, const u32 *ucol, const double *uval, const double *diag, u32 slot, u32 i,
                                               const double *y, const double *xs) {
    double acc = y[(u64)i * S];
    for (u32 k = uptr[slot], e = uptr[slot + 1]; k < e; k++) acc = acc - uval[k] * xs[(u64)ucol[k] * S];
    return acc / diag[slot];
}
struct ForwardOp {
    const u32 *order, *lptr, *lcol;
    const double *lval, *b;
    double *y;
    __device__ __forceinline__ void operator()(u32 slot) const { forward_row<1>(lptr, lcol, lval, slot, order[slot], b, y); }
};
// backward row: x[i] = ((y[i] - u*x[j1]) - ...)/u_ii.  ldiv!: xs == dst.  simple!'s `u .-= upd` fused: x replaces y in the
// scratch (nobody but row i reads y[i]), dst[i] = dst[i] - x[i] with x[i] rounded first.
struct BackwardOp {
    const u32 *order, *uptr, *ucol;
    const double *uval, *diag, *y;  // (diag in slot order as well)
    double *xs, *dst;
    bool sub;
    __device__ __forceinline__ void operator()(u32 slot) const {
        const u32 i = order[slot];
        const double x = backward_row<1>(uptr, ucol, uval, diag, slot, i, y, xs);
        if (sub) {
            xs[i] = x;
            dst[i] = dst[i] - x;
        } else {
            dst[i] = x;
        }
    }
};
// The many-column forms (iluam_solve_many): a lane owns one (slot, column d) pair.  The scratch is interleaved, Y[i * MC + d]: the MC
// lanes of a row are adjacent, gather one 64-byte line per stored entry and read lval[k] / lcol[k] at one address (the layout
// panels.hpp argues for).  V and U are the caller's column-major arrays.  Backward: x replaces y in the scratch, as sub does above
constexpr int MC = ESP_MANY_CHUNK;
static_assert(LT % MC == 0, "the MC lanes of a slot share a workgroup");
struct ForwardManyOp {
    const u32 *order, *lptr, *lcol;
    const double *lval, *V;
    i64 ldv;
    double *Y;
    __device__ __forceinline__ void operator()(u32 slot, int d) const {
        forward_row<MC>(lptr, lcol, lval, slot, order[slot], V + (i64)d * ldv, Y + d);
    }
};
struct BackwardManyOp {
    const u32 *order, *uptr, *ucol;
    const double *uval, *diag;
    double *Y, *U;
    i64 ldu;
    __device__ __forceinline__ void operator()(u32 slot, int d) const {
        const u32 i = order[slot];
        const double x = backward_row<MC>(uptr, ucol, uval, diag, slot, i, Y + d, Y + d);
        Y[(u64)i * MC + d] = x;
        U[(i64)d * ldu + i] = x;
    }
};

template <class Op>
__global__ __launch_bounds__(LT) void level_wide_k(Op op, u32 first, u32 count) {
    const u32 t = blockIdx.x * LT + threadIdx.x;
    if (t < count) op(first + t);
}
// one workgroup, the levels [l0, l1) one after the other (each holds at most LT members)
template <class Op>
__global__ __launch_bounds__(LT) void level_thin_k(Op op, const u32 *__restrict__ loff, u32 l0, u32 l1) {
    for (u32 l = l0; l < l1; l++) {
        const u32 b = loff[l], e = loff[l + 1];
        if (b + threadIdx.x < e) op(b + threadIdx.x);
        __syncthreads();
    }
}
// The many-column launches: the same launch list, MC lanes per member (d = t % MC, member = t / MC).  A lane whose column is not
// live, or whose member lies past the level's end, skips its loads and stores
template <class Op>
__global__ __launch_bounds__(LT) void level_wide_many_k(Op op, u32 first, u32 count, u32 live) {
    const u64 t = (u64)blockIdx.x * LT + threadIdx.x;
    const int d = (int)(t % MC);
    const u64 member = t / MC;
    if (member < count && is_live(live, d)) op(first + (u32)member, d);
}
// ... one workgroup takes the members of a level LT / MC at a time (a level of a thin launch holds up to LT members: up to MC passes,
// independent of each other).  Every lane reaches every barrier: the loop bounds are the workgroup's, there is no early return
template <class Op>
__global__ __launch_bounds__(LT) void level_thin_many_k(Op op, const u32 *__restrict__ loff, u32 l0, u32 l1, u32 live) {
    const int d = threadIdx.x % MC;
    const u32 member = threadIdx.x / MC;
    const bool on = is_live(live, d);
    for (u32 l = l0; l < l1; l++) {
        const u32 e = loff[l + 1];
        for (u32 b = loff[l]; b < e; b += LT / MC)
            if (on && b + member < e) op(b + member, d);
        __syncthreads();
    }
}
// (returns the launches it issued)
template <class Op>
i64 run_schedule_many(const esp_precon *p, const IluamSched &s, const Op &op, u32 live) {
    i64 issued = 0;
    for (const IluamLaunch &L : s.launches) {
        if (L.thin)
            hipLaunchKernelGGL(level_thin_many_k<Op>, dim3(1), dim3(LT), 0, p->h->stream, op, (const u32 *)s.loff.p, L.l0, L.l1, live);
        else
            hipLaunchKernelGGL(level_wide_many_k<Op>, dim3(grid_for((i64)L.count * MC, LT)), dim3(LT), 0, p->h->stream, op, L.first, L.count, live);
        issued++;
    }
    return issued;
}
// the wave form: a wave per member (a wide level: LT / 64 members per workgroup; a thin launch: the waves of the one workgroup take
// the members of a level in turn)
__global__ __launch_bounds__(LT) void factor_wave_wide_k(FactorWaveOp op, u32 first, u32 count) {
    __shared__ u32 srow[LT / 64][FW_ROWS];
    const u32 w = blockIdx.x * (LT / 64) + (threadIdx.x >> 6);
    if (w < count) op(first + w, srow[threadIdx.x >> 6]);
}
__global__ __launch_bounds__(LT) void factor_wave_thin_k(FactorWaveOp op, const u32 *__restrict__ loff, u32 l0, u32 l1) {
    __shared__ u32 srow[LT / 64][FW_ROWS];
    for (u32 l = l0; l < l1; l++) {
        const u32 b = loff[l], e = loff[l + 1];
        for (u32 m = b + (threadIdx.x >> 6); m < e; m += LT / 64) op(m, srow[threadIdx.x >> 6]);
        __syncthreads();
    }
}
void run_factor_waves(const esp_precon *p, const IluamSched &s, const FactorWaveOp &op) {
    for (const IluamLaunch &L : s.launches) {
        if (L.thin)
            hipLaunchKernelGGL(factor_wave_thin_k, dim3(1), dim3(LT), 0, p->h->stream, op, (const u32 *)s.loff.p, L.l0, L.l1);
        else
            hipLaunchKernelGGL(factor_wave_wide_k, dim3(grid_for(L.count, LT / 64)), dim3(LT), 0, p->h->stream, op, L.first, L.count);
    }
}
template <class Op>
void run_schedule(const esp_precon *p, const IluamSched &s, const Op &op) {
    for (const IluamLaunch &L : s.launches) {
        if (L.thin)
            hipLaunchKernelGGL(level_thin_k<Op>, dim3(1), dim3(LT), 0, p->h->stream, op, (const u32 *)s.loff.p, L.l0, L.l1);
        else
            hipLaunchKernelGGL(level_wide_k<Op>, dim3(grid_for(L.count, LT)), dim3(LT), 0, p->h->stream, op, L.first, L.count);
    }
}

// a row part from row order into the slot order of its schedule: slot t holds the part of row order[t]
__global__ void permute_count_k(const u32 *__restrict__ order, const u32 *__restrict__ ptr, i64 n, u32 *__restrict__ nptr) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n) return;
    nptr[t] = t < n ? ptr[order[t] + 1] - ptr[order[t]] : 0u;
}
__global__ void permute_fill_k(const u32 *__restrict__ order, const u32 *__restrict__ ptr, const u32 *__restrict__ col,
                               const u32 *__restrict__ pos, const u32 *__restrict__ nptr, i64 n, u32 *__restrict__ ncol,
                               u32 *__restrict__ npos) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const u32 src = ptr[order[t]], dst = nptr[t], cnt = nptr[t + 1] - dst;
    for (u32 q = 0; q < cnt; q++) {
        ncol[dst + q] = col[src + q];
        npos[dst + q] = pos[src + q];
    }
}
// the row parts' values and the diagonal of U from the factorization, all in slot order (t: a slot of both solves' schedules)
__global__ void iluam_gather_k(const u32 *__restrict__ lptr, const u32 *__restrict__ lpos, const u32 *__restrict__ uptr,
                               const u32 *__restrict__ upos, const u32 *__restrict__ dpos, const u32 *__restrict__ order_bwd,
                               const double *__restrict__ fval, i64 n, double *__restrict__ lval, double *__restrict__ uval,
                               double *__restrict__ diag) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    for (u32 k = lptr[t], e = lptr[t + 1]; k < e; k++) lval[k] = fval[lpos[k]];
    for (u32 k = uptr[t], e = uptr[t + 1]; k < e; k++) uval[k] = fval[upos[k]];
    diag[t] = fval[dpos[order_bwd[t]]];
}

Pattern pattern_of(const esp_precon *p) {
    const esp_handle *h = p->h;
    return Pattern{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (const u32 *)p->dpos.p,
                   (const u32 *)p->lptr.p,   (const u32 *)p->uptr.p,   (const u32 *)p->ucol.p};
}

// the analysis' scratch: gone when the analysis ends, however it ends (after the work that uses it)
struct Scratch {
    esp_handle *h;
    DevBuf b;
    ~Scratch() {
        (void)hipStreamSynchronize(h->stream);
        release(b);
    }
};

template <int S>
int32_t build_schedule(esp_precon *p, IluamSched &s) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    s.levels = 0;
    s.launches.clear();
    if (n == 0) return ESP_OK;
    // scratch: sort keys and payloads (two of each), level, in-degree, two frontiers, two counters
    Scratch tmp{h};
    CK(ensure(h, tmp.b, (size_t)n * (4 * 8 + 4 * 4) + 16));
    void *rest;
    const PingPong d = carve_pingpong(tmp.b.p, n, &rest);
    u32 *level = (u32 *)rest, *indeg = level + n, *front[2] = {indeg + n, indeg + 2 * n}, *cnt = indeg + 3 * n;
    const Pattern g = pattern_of(p);
    std::vector<u32> loff(1, 0u);
    HIPCK(h, hipMemsetAsync(cnt, 0, 8, h->stream));
    hipLaunchKernelGGL(level_init_k<S>, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, g, n, indeg, level, front[0], cnt);
    for (u32 r = 0;; r++) {  // one round per level, one counter read back per round
        u32 *c_cur = cnt + (r & 1), *c_next = cnt + ((r + 1) & 1);
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, c_cur, 4, hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        const u32 count = *(const u32 *)h->pin_scalar;
        if (count == 0) break;
        loff.push_back(loff.back() + count);
        hipLaunchKernelGGL(level_expand_k<S>, dim3(grid_for(count, 256)), dim3(256), 0, h->stream, g, (const u32 *)front[r & 1], count,
                           front[(r + 1) & 1], c_next, c_cur, indeg, level, r + 1);
    }
    if ((i64)loff.back() != n)
        FAIL(h, ESP_ERR_HIP, "iluam: the level analysis reached %lld of %lld nodes", (long long)loff.back(), (long long)n);
    s.levels = (i64)loff.size() - 1;
    // nodes sorted by (level, index): a stable LSD sort on the level bits of the nodes in index order
    hipLaunchKernelGGL(level_keys_k, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, (const u32 *)level, n, d.k[0], d.v[0]);
    int B = 1;
    while (((i64)1 << B) < s.levels) B++;
    SortPair r;
    CK(sort_segment_lsd(h, d.half(0), d, n, 0, B, 62, &r));
    CK(ensure(h, s.order, sizeof(u32) * (size_t)n));
    CK(ensure(h, s.loff, sizeof(u32) * loff.size()));
    hipLaunchKernelGGL(level_order_k, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, r.v, n, (u32 *)s.order.p);
    HIPCK(h, hipMemcpyAsync(s.loff.p, loff.data(), sizeof(u32) * loff.size(), hipMemcpyHostToDevice, h->stream));
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(h->stream));
    // the launch list: a level wider than a workgroup by itself, else as many consecutive levels as fit one workgroup
    for (u32 l = 0; l < (u32)s.levels;) {
        const u32 c = loff[l + 1] - loff[l];
        if (c > (u32)LT) {
            s.launches.push_back(IluamLaunch{l, l + 1, loff[l], c, false});
            l++;
            continue;
        }
        u32 e = l + 1;
        while (e < (u32)s.levels && loff[e + 1] - loff[l] <= (u32)LT) e++;
        s.launches.push_back(IluamLaunch{l, e, loff[l], loff[e] - loff[l], true});
        l = e;
    }
    return ESP_OK;
}

// ptr / col / pos (row order, from split_build) -> the slot order of schedule s; the row-order arrays are released
int32_t permute_part(esp_precon *p, const IluamSched &s, DevBuf &ptr, DevBuf &col, DevBuf &pos) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    if (n == 0) return ESP_OK;
    DevBuf nptr, ncol, npos;
    const int32_t st = [&]() -> int32_t {
        CK(ensure(h, nptr, sizeof(u32) * (size_t)(n + 1)));
        CK(ensure(h, ncol, col.bytes));
        CK(ensure(h, npos, pos.bytes));
        hipLaunchKernelGGL(permute_count_k, dim3(grid_for(n + 1, 256)), dim3(256), 0, h->stream, (const u32 *)s.order.p,
                           (const u32 *)ptr.p, n, (u32 *)nptr.p);
        int l = 0;
        CK(scan_inplace<u32, false>(h, (u32 *)nptr.p, n + 1, p->scanws, &l));
        hipLaunchKernelGGL(permute_fill_k, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, (const u32 *)s.order.p, (const u32 *)ptr.p,
                           (const u32 *)col.p, (const u32 *)pos.p, (const u32 *)nptr.p, n, (u32 *)ncol.p, (u32 *)npos.p);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipStreamSynchronize(h->stream));
        return ESP_OK;
    }();
    if (st != ESP_OK) {
        (void)hipStreamSynchronize(h->stream);
        release(nptr);
        release(ncol);
        release(npos);
        return st;
    }
    std::swap(ptr, nptr);
    std::swap(col, ncol);
    std::swap(pos, npos);
    release(nptr);
    release(ncol);
    release(npos);
    return ESP_OK;
}

}  // namespace

int32_t iluam_update(esp_precon *p, bool rebuild) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "iluam: a column window / column shard");
    if (rebuild) {                // iluAM(A): the analysis
        CK(diag_refresh(p));      // (refuses a missing diagonal before anything is built)
        CK(split_build(p, true));
        CK(ensure(h, p->u1, sizeof(double) * (size_t)std::max<i64>(n, 1)));
        if (!p->prefactored) CK(build_schedule<S_FACTOR>(p, p->sched[S_FACTOR]));
        CK(build_schedule<S_FWD>(p, p->sched[S_FWD]));
        CK(build_schedule<S_BWD>(p, p->sched[S_BWD]));
        CK(permute_part(p, p->sched[S_FWD], p->lptr, p->lcol, p->lpos));  // (the analysis above read them in row order)
        CK(permute_part(p, p->sched[S_BWD], p->uptr, p->ucol, p->upos));
    }
    // the numeric factorization on a copy of the values (prefactored, ilut.hip's inner preconditioner: the values are the factorization
    // already -- the copy and the gather alone)
    p->iluam_form = 0;
    CK(ensure(h, p->fval, sizeof(double) * (size_t)std::max<i64>(h->nnz, 1)));
    if (n == 0) return ESP_OK;
    HIPCK(h, hipMemcpyAsync(p->fval.p, h->nzval.p, sizeof(double) * (size_t)h->nnz, hipMemcpyDeviceToDevice, h->stream));
    if (!p->prefactored) p->iluam_form = p->iluam_force ? p->iluam_force : h->nnz >= (i64)FW_MIN_AVG * n ? 2 : 1;
    if (p->iluam_form == 2)
        run_factor_waves(p, p->sched[S_FACTOR], FactorWaveOp{(const u32 *)p->sched[S_FACTOR].order.p, (const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (const u32 *)p->dpos.p, (double *)p->fval.p});
    else if (p->iluam_form == 1)
        run_schedule(p, p->sched[S_FACTOR], FactorOp{(const u32 *)p->sched[S_FACTOR].order.p, (const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (const u32 *)p->dpos.p, (double *)p->fval.p});
    hipLaunchKernelGGL(iluam_gather_k, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, (const u32 *)p->lptr.p, (const u32 *)p->lpos.p,
                       (const u32 *)p->uptr.p, (const u32 *)p->upos.p, (const u32 *)p->dpos.p, (const u32 *)p->sched[S_BWD].order.p,
                       (const double *)p->fval.p, n,
                       (double *)p->lval.p, (double *)p->uval.p, (double *)p->diag.p);
    HIPCK(h, hipGetLastError());
    return ESP_OK;
}

// ldiv!(dst, ILU, v) on device vectors (dst may be v); sub: dst[i] = dst[i] - x[i] instead (simple!'s step, v = res)
int32_t iluam_solve(esp_precon *p, const double *v, double *dst, bool sub) {
    esp_handle *h = p->h;
    if (p->n == 0) return ESP_OK;
    double *y = (double *)p->u1.p;  // the forward solve writes the scratch: dst may be v
    run_schedule(p, p->sched[S_FWD], ForwardOp{(const u32 *)p->sched[S_FWD].order.p, (const u32 *)p->lptr.p, (const u32 *)p->lcol.p, (const double *)p->lval.p, v, y});
    run_schedule(p, p->sched[S_BWD], BackwardOp{(const u32 *)p->sched[S_BWD].order.p, (const u32 *)p->uptr.p, (const u32 *)p->ucol.p, (const double *)p->uval.p,
                                                (const double *)p->diag.p, (const double *)y, sub ? y : dst, dst, sub});
    HIPCK(h, hipGetLastError());
    return ESP_OK;
}

// ldiv! of the live columns of one chunk: the two launch lists walked once each, whatever nr is (live: bits below nr).  A frozen
// column's u is never written.  The scratch grows to MC * n doubles here: a preconditioner that never sees a many-column call keeps
// the n doubles of update!
int32_t iluam_solve_many(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, int nr, u32 live) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    live &= all_live(nr);
    if (n == 0 || nr <= 0) return ESP_OK;
    CK(ensure(h, p->u1, sizeof(double) * (size_t)n * MC));
    double *Y = (double *)p->u1.p;
    i64 issued = run_schedule_many(p, p->sched[S_FWD], ForwardManyOp{(const u32 *)p->sched[S_FWD].order.p, (const u32 *)p->lptr.p, (const u32 *)p->lcol.p, (const double *)p->lval.p, v, ldv, Y}, live);
    issued += run_schedule_many(p, p->sched[S_BWD], BackwardManyOp{(const u32 *)p->sched[S_BWD].order.p, (const u32 *)p->uptr.p, (const u32 *)p->ucol.p, (const double *)p->uval.p,
                                                                   (const double *)p->diag.p, Y, u, ldu}, live);
    p->many_stats[2] = issued;
    HIPCK(h, hipGetLastError());
    return ESP_OK;
}

void iluam_release(esp_precon *p) {
    release(p->fval);
    for (IluamSched &s : p->sched) {
        release(s.order);
        release(s.loff);
    }
}

extern "C" int32_t esp_precon_get_factor(esp_precon *p, double *nzval, int32_t on_device) {
    if (!p || !nzval) return ESP_ERR_INVALID;
    esp_handle *h = p->h;
    if (holds_derived(p)) {  // the inner factorization: nnz(B) values in B's position order
        if (h->pattern_version != p->pattern_version || h->nnz != p->nnz)
            FAIL(h, ESP_ERR_STATE, "esp_precon_get_factor: the matrix pattern changed since the preconditioner's last update!");
        CK(derived_follow_stream(p));
        if (p->lup) return lup_factor(p, nzval, on_device);  // LUFactorization's panel form: exported from the panels
        const int32_t st = esp_precon_get_factor(p->der.inner, nzval, on_device);
        if (st != ESP_OK) FAIL(h, st, "%s", p->der.bh->err.c_str());
        return ESP_OK;
    }
    const bool spai = p->kind == ESP_PRECON_SPAI;  // the applied M's values in its position order / the n diagonal values of SPAI-0
    if (p->kind != ESP_PRECON_ILUAM && !spai) FAIL(h, ESP_ERR_INVALID, "esp_precon_get_factor: not an ILUAM preconditioner");
    if (h->pattern_version != p->pattern_version || h->nnz != p->nnz)  // (the caller sized nzval by the matrix's nnz)
        FAIL(h, ESP_ERR_STATE, "esp_precon_get_factor: the matrix pattern changed since the preconditioner's last update!");
    (void)hipSetDevice(h->device);
    if (spai) CK(spai_follow_stream(p));
    const void *src = !spai ? p->fval.p : p->spai_order == 0 ? p->diag.p : spai_applied(p)->nzval.p;
    const size_t bytes = sizeof(double) * (size_t)(!spai ? p->nnz : p->spai_order == 0 ? p->n : spai_applied(p)->nnz);
    return copy_out(h, nzval, src, bytes, on_device);
}

extern "C" int32_t esp_precon_levels(esp_precon *p, int64_t out[3]) {
    if (!p || !out) return ESP_ERR_INVALID;
    if (holds_derived(p) && p->der.inner) p = p->der.inner;
    for (int k = 0; k < 3; k++) out[k] = p->kind == ESP_PRECON_ILUAM ? p->sched[k].levels : 0;
    return ESP_OK;
}

// the ILUAM preconditioner the two calls below speak to: p itself, or the inner one of a kind that holds a derived matrix
static esp_precon *iluam_of(esp_precon *p) {
    if (p && holds_derived(p)) p = p->der.inner;
    return p && p->kind == ESP_PRECON_ILUAM ? p : nullptr;
}

extern "C" int32_t esp_debug_iluam_form(esp_precon *p, int32_t form) {
    esp_precon *q = iluam_of(p);
    if (!q || form < 0 || form > 2) return ESP_ERR_INVALID;
    q->iluam_force = form;
    return ESP_OK;
}

extern "C" int32_t esp_debug_last_iluam_form(esp_precon *p, int32_t *form) {
    esp_precon *q = iluam_of(p);
    if (!q || !form) return ESP_ERR_INVALID;
    *form = q->iluam_form;
    return ESP_OK;
}

extern "C" int32_t esp_precon_many_stats(esp_precon *p, int64_t out[4]) {
    if (!p || !out) return ESP_ERR_INVALID;
    if (holds_derived(p) && p->der.inner) p = p->der.inner;
    for (int k = 0; k < 4; k++) out[k] = p->many_stats[k];
    return ESP_OK;
}

extern "C" int32_t esp_precon_launches(esp_precon *p, int64_t out[6]) {
    if (!p || !out) return ESP_ERR_INVALID;
    if (holds_derived(p) && p->der.inner) p = p->der.inner;
    for (int k = 0; k < 3; k++) {
        i64 wide = 0, thin = 0;
        if (p->kind == ESP_PRECON_ILUAM)
            for (const IluamLaunch &L : p->sched[k].launches) (L.thin ? thin : wide)++;
        out[2 * k] = wide;
        out[2 * k + 1] = thin;
    }
    return ESP_OK;
}
