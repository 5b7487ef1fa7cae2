// amg.hip -- libesparse_hip: AMGPreconditioner, a smoothed-aggregation V-cycle on the device CSC
// (see internal.hpp for the map of the translation units)
//
// The reference's SA_AMGPreconditioner (ext/ExtendableSparseAlgebraicMultigridExt.jl) wraps AlgebraicMultigrid.jl, which is not
// part of the reference tree; its aggregation is a sequential greedy sweep and its spectral-radius estimate starts from rand.  The
// algorithm here is stated in full in include/esparse_hip.h and DESIGN.md 5i; tests/amg_model.c restates it as plain loops and is
// normative for the order of every operation.  Everything below is bit-identical to that model.
//
// Setup (esp_precon_update: always the whole hierarchy), level by level from A_0 = a copy of A:
//   dinv, rho, w     esp_jacobi_setup, esp_diag_scale + esp_opnorm(., Inf) on an internal handle, w = ((4/3)/rho)*dinv
//   amg_check_k      level 0 only: every column holds its diagonal, every stored (i,j) has a stored (j,i) (the smallest column named)
//   amg_strength_k   one flag per stored entry: i != j, the mirror stored, m = max(|a_ij|, |a_ji|) != 0, m*m >= theta^2*(|a_ii|*|a_jj|)
//   amg_luby_k<1|2>  one Luby round of MIS(2): T1 = max of t over {i} and its strong neighbours, T2 the same over T1, then the
//                    decision (root / excluded / still undecided: a plain store of 1 to the round's flag, read back by the host).
//                    One lane per column; a column of more than AMG_LONG entries is folded by its whole wave, 64 entries at a time
//   scan             the roots numbered in index order (scan.hpp)
//   amg_join_k<1|2>  the two joining passes (two buffers: pass 2 reads what pass 1 wrote, never itself)
//   T                transpose(T) is a CSC one can write down (column i holds the single row agg(i)); T = esp_transpose of it: a
//                    counting sort by aggregate that keeps index order
//   P, A_{l+1}       esp_diag_scale, esp_matmul, esp_add, esp_transpose, esp_matmul twice, on internal handles the preconditioner owns
//   amg_gj_k         the coarsest level's dense inverse: one workgroup, Gauss-Jordan with partial pivoting on [A | I] in global memory
// With coarsening mode ESP_AMG_COARSEN_RS (esp_precon_rsamg_create) the aggregation and the formation of P are replaced by
// rsamg_coarsen (rsamg.hip: row-wise strength, a PMIS splitting, direct interpolation); everything else here serves both.
// The V-cycle (esp_precon_ldiv, and inside esp_simple / esp_cg / esp_bicgstabl): launches on the handle's stream only, every buffer
// sized at setup -- no copy, no allocation, no synchronisation.
//   amg_scale_k      the first pre-sweep from x = 0: x = w.*b
//   amg_row_k<SWEEP> x_new[i] = x[i] + w[i]*(b[i] - (A x)[i]) over esp_mul's row-wise index, one pass (Jacobi: two buffers)
//   amg_row_k<RESID> r[i] = b[i] - (A x)[i]
//   amg_restrict_k   b_c = transpose(P)*r over P's columns, esp_mul_transpose's rule (tmp accumulation, r[j] = 0.0 + tmp)
//   amg_dense_k      x_c = inv*b_c, one row per wave, the products of 64 columns at a time folded in column order
//   amg_row_k<PROLONG> x[i] = x[i] + (P x_c)[i] over P's row-wise index
// The last kernel of level 0 stores straight into u (u may alias v: every lane reads its own b[i] before it stores u[i]), fused
// with simple!'s `u .-= upd` where that is the caller.
#include "amg.hpp"

using namespace espamg;

int32_t amg_make_handle(esp_handle *h, i64 m, i64 n, esp_handle **out) {
    const int32_t st = esp_create(m, n, h->device, 0, out);
    if (st != ESP_OK) FAIL(h, st == ESP_ERR_HIP ? ESP_ERR_NOMEM : st, "esp_precon_amg: an internal handle: %s", esp_last_error(nullptr));
    CK(esp_set_stream(*out, (void *)h->stream));
    return ESP_OK;
}

namespace {

constexpr int AMG_TLONG = 64;  // restriction: as esp_mul_transpose's MV_LONG
constexpr int GJT = 1024;      // threads of the Gauss-Jordan workgroup

// ---- setup: checks, strength, Luby rounds, joining -----------------------------------------------------------------------------
// st[0] = smallest 1-based column without a stored diagonal, st[1] = smallest 1-based column with a stored (i,j) but no (j,i)
__global__ void amg_check_k(espfold::Csc c, i64 n, unsigned long long *__restrict__ st) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    bool diag = false, sym = true;
    for (i64 k = c.colptr[j] - 1; k < c.colptr[j + 1] - 1; k++) {
        const i64 i = c.rowval[k] - 1;
        if (i == j) diag = true;
        else if (espfold::csc_find(c, i, j) < 0) sym = false;
    }
    if (!diag) atomicMin(&st[0], (unsigned long long)(j + 1));
    if (!sym) atomicMin(&st[1], (unsigned long long)(j + 1));
}
// dg[j] = a_jj (0.0 where not stored), w[j] = omega*dinv[j], nw[j] = -w[j]
__global__ void amg_diag_k(espfold::Csc c, i64 n, const double *__restrict__ dinv, double omega, double *__restrict__ dg,
                           double *__restrict__ w, double *__restrict__ nw) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const i64 pos = c.nnz > 0 ? espfold::csc_find(c, j, j) : -1;
    dg[j] = pos >= 0 ? c.nzval[pos] : 0.0;
    const double wj = omega * dinv[j];
    w[j] = wj;
    nw[j] = -wj;
}
__global__ void amg_strength_k(espfold::Csc c, i64 n, const double *__restrict__ dg, double theta, uint8_t *__restrict__ strong) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double ajj = fabs(dg[j]);
    for (i64 k = c.colptr[j] - 1; k < c.colptr[j + 1] - 1; k++) {
        const i64 i = c.rowval[k] - 1;
        uint8_t s = 0;
        if (i != j) {
            const i64 pos = espfold::csc_find(c, i, j);
            if (pos >= 0) {
                const double x = fabs(c.nzval[k]), y = fabs(c.nzval[pos]);
                double m = x;
                if (y > m || m != m) m = y;
                if (m != 0.0 && m * m >= (theta * theta) * (fabs(dg[i]) * ajj)) s = 1;
            }
        }
        strong[k] = s;
    }
}
__device__ __forceinline__ u64 amg_key(i64 i) { return ((u64)amg_mix(i) << 32) | (u64)(u32)i; }
// state: 0 undecided, 1 root, 2 excluded
__device__ __forceinline__ u64 amg_t(u32 state, i64 i) { return state == 2u ? 0ull : state == 1u ? ~0ull : amg_key(i); }
// PH 1: out[j] = max of t over {j} and its strong neighbours; PH 2: the same max over in[] (= T1), then j's decision
template <int PH>
__global__ __launch_bounds__(AT) void amg_luby_k(const i64 *__restrict__ colptr, const i64 *__restrict__ rowval,
                                                 const uint8_t *__restrict__ strong, i64 n, u32 *state, const u64 *__restrict__ in,
                                                 u64 *__restrict__ out, u32 *__restrict__ flag) {
    const i64 j = (i64)blockIdx.x * AT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    i64 s = 0, e = 0;
    u64 m = 0;
    if (j < n) {
        s = colptr[j] - 1;
        e = colptr[j + 1] - 1;
        m = PH == 1 ? amg_t(state[j], j) : in[j];
    }
    const bool longc = e - s > AMG_LONG;
    if (j < n && !longc) {
        for (i64 k = s; k < e; k++) {
            if (!strong[k]) continue;
            const i64 r = rowval[k] - 1;
            const u64 v = PH == 1 ? amg_t(state[r], r) : in[r];
            m = v > m ? v : m;
        }
    }
    // the wave's long columns one after the other, 64 entries at a time (every lane of the wave gets here: nobody left early)
    u64 mask = __ballot(longc);
    while (mask) {
        const int sl = __builtin_ctzll(mask);
        mask &= mask - 1;
        const i64 ls = __shfl(s, sl), le = __shfl(e, sl);
        u64 v = 0;
        for (i64 b = ls; b < le; b += 64) {
            const i64 k = b + lane;
            if (k < le && strong[k]) {
                const i64 r = rowval[k] - 1;
                const u64 t = PH == 1 ? amg_t(state[r], r) : in[r];
                v = t > v ? t : v;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const u64 t = __shfl_xor(v, o);
            v = t > v ? t : v;
        }
        if (lane == sl) m = v > m ? v : m;
    }
    if (j >= n) return;
    if (PH == 1) {
        out[j] = m;
    } else if (state[j] == 0u) {  // (a lane writes its own state only; the neighbours read T1)
        if (m == amg_key(j)) state[j] = 1u;
        else if (m == ~0ull) state[j] = 2u;
        else *flag = 1u;  // somebody is still undecided: a plain store
    }
}
__global__ void amg_isroot_k(const u32 *__restrict__ state, i64 n, i64 *__restrict__ num) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j <= n) num[j] = j < n && state[j] == 1u ? 1 : 0;
}
// PASS 1: a root takes its number, every other node the aggregate of its smallest-index strong root neighbour (else -1);
// PASS 2: a node still without one takes what its smallest-index strong neighbour holds in `in` (pass 1's result); left = 1
// if somebody stays without (maximality of the independent set excludes it)
template <int PASS>
__global__ void amg_join_k(const i64 *__restrict__ colptr, const i64 *__restrict__ rowval, const uint8_t *__restrict__ strong, i64 n,
                           const u32 *__restrict__ state, const i64 *__restrict__ num, const i64 *__restrict__ in, i64 *__restrict__ out,
                           u32 *__restrict__ left) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    i64 a = PASS == 1 ? (state[j] == 1u ? num[j] : -1) : in[j];
    if (a < 0) {
        for (i64 k = colptr[j] - 1; k < colptr[j + 1] - 1; k++) {
            if (!strong[k]) continue;
            const i64 r = rowval[k] - 1;
            const i64 ar = PASS == 1 ? (state[r] == 1u ? num[r] : -1) : in[r];
            if (ar >= 0) {
                a = ar;
                break;
            }
        }
        if (PASS == 2 && a < 0) *left = 1u;
    }
    out[j] = a;
}
// transpose(T): an nc x n CSC whose column i holds the single row agg(i) with the value 1.0
__global__ void amg_tt_k(const i64 *__restrict__ agg, i64 n, i64 *__restrict__ cp, i64 *__restrict__ rv, double *__restrict__ nz) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) cp[i] = i + 1;
    if (i < n) {
        rv[i] = agg[i] + 1;
        nz[i] = 1.0;
    }
}
// ---- the coarsest level's dense inverse --------------------------------------------------------------------------------------
// aug (n rows of 2n, zeroed): [A | I]
__global__ void amg_aug_k(espfold::Csc c, i64 n, double *__restrict__ aug) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    for (i64 k = c.colptr[j] - 1; k < c.colptr[j + 1] - 1; k++) aug[(c.rowval[k] - 1) * 2 * n + j] = c.nzval[k];
    aug[j * 2 * n + n + j] = 1.0;
}
// One workgroup.  Column by column: the pivot is the largest |.| at or below the diagonal (the smallest row on ties; a NaN is
// never larger, a NaN on the diagonal stays), the rows are swapped, the pivot row is divided by the pivot, every other row i
// becomes a[i][j] - a[i][k]*a[k][j] over the whole width (a zero pivot is no error: Inf / NaN propagate)
__global__ __launch_bounds__(GJT) void amg_gj_k(double *a, int n, double *__restrict__ inv) {
    __shared__ double sv[GJT];
    __shared__ int si[GJT];
    __shared__ double fcol[ESP_AMG_DENSE_MAX];
    __shared__ int spiv;
    const int tid = threadIdx.x, W = 2 * n;
    for (int k = 0; k < n; k++) {
        double best = -1.0;
        int bi = n;
        for (int r = k + tid; r < n; r += GJT) {
            const double v = fabs(a[(size_t)r * W + k]);
            if (v > best) {
                best = v;
                bi = r;
            }
        }
        sv[tid] = best;
        si[tid] = bi;
        __syncthreads();
        for (int w = GJT / 2; w > 0; w >>= 1) {
            if (tid < w) {
                const double v2 = sv[tid + w];
                const int i2 = si[tid + w];
                if (v2 > sv[tid] || (v2 == sv[tid] && i2 < si[tid])) {
                    sv[tid] = v2;
                    si[tid] = i2;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const double akk = fabs(a[(size_t)k * W + k]);
            spiv = (akk != akk || si[0] >= n) ? k : si[0];
        }
        __syncthreads();
        const int pr = spiv;
        if (pr != k) {
            for (int j = tid; j < W; j += GJT) {
                const double t = a[(size_t)k * W + j];
                a[(size_t)k * W + j] = a[(size_t)pr * W + j];
                a[(size_t)pr * W + j] = t;
            }
        }
        __syncthreads();
        const double piv = a[(size_t)k * W + k];
        for (int i = tid; i < n; i += GJT)
            if (i != k) fcol[i] = a[(size_t)i * W + k];
        __syncthreads();
        for (int j = tid; j < W; j += GJT) a[(size_t)k * W + j] = a[(size_t)k * W + j] / piv;
        __syncthreads();
        for (int i = 0; i < n; i++) {
            if (i == k) continue;
            const double f = fcol[i];
            for (int j = tid; j < W; j += GJT) a[(size_t)i * W + j] = a[(size_t)i * W + j] - f * a[(size_t)k * W + j];
        }
        __syncthreads();
    }
    for (int idx = tid; idx < n * n; idx += GJT) {
        const int i = idx / n, j = idx - i * n;
        inv[idx] = a[(size_t)i * W + n + j];
    }
}

// ---- the V-cycle ---------------------------------------------------------------------------------------------------------------
// (dst may be b or sub: no __restrict__ on them; sub != nullptr: dst[i] = sub[i] - value, simple!'s `u .-= upd`)
__global__ void amg_scale_k(const double *__restrict__ w, const double *b, double *dst, const double *sub, i64 n) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = w[i] * b[i];
    dst[i] = sub ? sub[i] - v : v;
}
enum AmgRow { SWEEP = 0, RESID = 1, PROLONG = 2 };
// rp = csr_rowptr + 1: the entries of row i are [rp[i], rp[i+1]) of col / val, columns ascending (esp_mul's index and order)
//   SWEEP    dst[i] = x[i] + w[i]*(b[i] - (A x)[i])        (dst is not x: the neighbours read the old x)
//   RESID    dst[i] = b[i] - (A x)[i]
//   PROLONG  dst[i] = b[i] + (P x)[i]                       (b: the fine iterate, x: the coarse solution; dst may be b)
template <int MODE>
__global__ __launch_bounds__(AT) void amg_row_k(const u64 *__restrict__ rp, const u32 *__restrict__ col, const double *__restrict__ val,
                                                const double *__restrict__ x, const double *b, const double *__restrict__ w, double *dst,
                                                const double *sub, i64 n) {
    const i64 i = (i64)blockIdx.x * AT + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;  // r .= zero(eltype)
    const u64 kb = rp[i], ke = rp[i + 1];
    for (u64 k = kb; k < ke; k++) acc = acc + val[k] * x[col[k]];
    double v;
    if (MODE == SWEEP) v = x[i] + w[i] * (b[i] - acc);
    else if (MODE == RESID) v = b[i] - acc;
    else v = b[i] + acc;
    dst[i] = sub ? sub[i] - v : v;
}
// bc = transpose(P)*r: one lane per column, a wave for a column longer than AMG_TLONG (the same sum in the same order)
__global__ __launch_bounds__(AT) void amg_restrict_k(const i64 *__restrict__ colptr, const i64 *__restrict__ rowval,
                                                     const double *__restrict__ nzval, i64 nc, const double *__restrict__ r,
                                                     double *__restrict__ bc) {
    const i64 j = (i64)blockIdx.x * AT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    i64 s = 0, e = 0;
    if (j < nc) {
        s = colptr[j] - 1;
        e = colptr[j + 1] - 1;
    }
    const bool longc = e - s > AMG_TLONG;
    if (j < nc && !longc) {
        double tmp = 0.0;
        for (i64 k = s; k < e; k++) tmp = tmp + nzval[k] * r[rowval[k] - 1];
        bc[j] = 0.0 + tmp;
    }
    u64 mask = __ballot(longc);
    while (mask) {
        const int src = __builtin_ctzll(mask);
        mask &= mask - 1;
        const i64 ls = __shfl(s, src), le = __shfl(e, src);
        double tmp = 0.0;
        for (i64 b = ls; b < le; b += 64) {
            const i64 k = b + lane;
            const double pr = k < le ? nzval[k] * r[rowval[k] - 1] : 0.0;
            const int cnt = (int)min((i64)64, le - b);
            for (int t = 0; t < cnt; t++) tmp = tmp + __shfl(pr, t);
        }
        if (lane == src) bc[j] = 0.0 + tmp;
    }
}
// x[i] = s with s = 0.0; s += inv[i][j]*b[j] for increasing j: one row per wave
__global__ __launch_bounds__(AT) void amg_dense_k(const double *__restrict__ inv, const double *__restrict__ b, double *__restrict__ x, int n) {
    const int row = blockIdx.x * (AT / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n) return;  // (wave-uniform)
    double s = 0.0;
    for (int b0 = 0; b0 < n; b0 += 64) {
        const int j = b0 + lane;
        const double pr = j < n ? inv[(size_t)row * n + j] * b[j] : 0.0;
        const int cnt = min(64, n - b0);
        for (int t = 0; t < cnt; t++) s = s + __shfl(pr, t);
    }
    if (lane == 0) x[row] = s;
}
__global__ void amg_finish_k(const double *__restrict__ x, double *dst, const double *sub, i64 n) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = sub ? sub[i] - x[i] : x[i];
}

void release_level(AmgLevel &L) {
    if (L.A) (void)esp_destroy(L.A);
    if (L.P) (void)esp_destroy(L.P);
    L.A = L.P = nullptr;
    for (DevBuf *b : {&L.w, &L.agg, &L.x0, &L.x1, &L.b, &L.r}) release(*b);
}
void release_levels(std::vector<AmgLevel> &lv) {
    for (AmgLevel &L : lv) release_level(L);
    lv.clear();
}

// the aggregation of level L (its matrix in L.A): L.agg, L.nc, L.rounds
int32_t aggregate(esp_handle *h, AmgLevel &L, const double *dg, double theta) {
    hipStream_t s = h->stream;
    const i64 n = L.n, nnz = L.A->nnz;
    const espfold::Csc c = csc_of(L.A);
    Temps tmp;
    DevBuf &strong = tmp.b[0], &state = tmp.b[1], &t1 = tmp.b[2], &flag = tmp.b[3], &num = tmp.b[4], &a1 = tmp.b[5], &ws = tmp.b[6];
    const unsigned g = grid_for(n, AT);
    CK(ensure(h, strong, (size_t)std::max<i64>(nnz, 1)));
    CK(ensure(h, state, sizeof(u32) * (size_t)n));
    CK(ensure(h, t1, sizeof(u64) * (size_t)n));
    CK(ensure(h, flag, sizeof(u32) * 2));
    CK(ensure(h, num, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, a1, sizeof(i64) * (size_t)n));
    CK(ensure(h, L.agg, sizeof(i64) * (size_t)n));
    hipLaunchKernelGGL(amg_strength_k, dim3(g), dim3(AT), 0, s, c, n, dg, theta, (uint8_t *)strong.p);
    HIPCK(h, hipMemsetAsync(state.p, 0, sizeof(u32) * (size_t)n, s));
    L.rounds = 0;
    for (;;) {  // the globally largest undecided key decides in every round: at most n rounds
        HIPCK(h, hipMemsetAsync(flag.p, 0, sizeof(u32) * 2, s));
        hipLaunchKernelGGL(amg_luby_k<1>, dim3(g), dim3(AT), 0, s, c.colptr, c.rowval, (const uint8_t *)strong.p, n, (u32 *)state.p,
                           (const u64 *)nullptr, (u64 *)t1.p, (u32 *)nullptr);
        hipLaunchKernelGGL(amg_luby_k<2>, dim3(g), dim3(AT), 0, s, c.colptr, c.rowval, (const uint8_t *)strong.p, n, (u32 *)state.p,
                           (const u64 *)t1.p, (u64 *)nullptr, (u32 *)flag.p);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, flag.p, sizeof(u32), hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        L.rounds++;
        if (*(const u32 *)h->pin_scalar == 0u) break;
        if ((i64)L.rounds > n) FAIL(h, ESP_ERR_HIP, "esp_precon_amg: the aggregation did not end after %lld rounds", (long long)n);
    }
    hipLaunchKernelGGL(amg_isroot_k, dim3(grid_for(n + 1, AT)), dim3(AT), 0, s, (const u32 *)state.p, n, (i64 *)num.p);
    int l = 0;
    CK(scan_inplace<i64, false>(h, (i64 *)num.p, n + 1, ws, &l));
    HIPCK(h, hipMemsetAsync(flag.p, 0, sizeof(u32) * 2, s));
    hipLaunchKernelGGL(amg_join_k<1>, dim3(g), dim3(AT), 0, s, c.colptr, c.rowval, (const uint8_t *)strong.p, n, (const u32 *)state.p,
                       (const i64 *)num.p, (const i64 *)nullptr, (i64 *)a1.p, (u32 *)flag.p);
    hipLaunchKernelGGL(amg_join_k<2>, dim3(g), dim3(AT), 0, s, c.colptr, c.rowval, (const uint8_t *)strong.p, n, (const u32 *)state.p,
                       (const i64 *)num.p, (const i64 *)a1.p, (i64 *)L.agg.p, (u32 *)flag.p);
    HIPCK(h, hipGetLastError());
    CK(read_i64(h, (const i64 *)num.p + n, &L.nc));
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, flag.p, sizeof(u32), hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    if (*(const u32 *)h->pin_scalar != 0u || L.nc < 1 || L.nc > n)
        FAIL(h, ESP_ERR_HIP, "esp_precon_amg: the aggregation left a node without an aggregate (%lld roots of %lld)", (long long)L.nc, (long long)n);
    L.has_agg = true;
    return ESP_OK;
}

// the dense inverse of the coarsest level
int32_t dense_inverse(esp_handle *h, AmgData *D, const AmgLevel &L, DevBuf &inv) {
    hipStream_t s = h->stream;
    const i64 n = L.n;
    CK(ensure(h, inv, sizeof(double) * (size_t)std::max<i64>(n * n, 1)));
    if (n == 0) return ESP_OK;
    Temps tmp;
    DevBuf &aug = tmp.b[0];
    CK(ensure(h, aug, sizeof(double) * (size_t)(2 * n * n)));
    HIPCK(h, hipMemsetAsync(aug.p, 0, sizeof(double) * (size_t)(2 * n * n), s));
    hipLaunchKernelGGL(amg_aug_k, dim3(grid_for(n, AT)), dim3(AT), 0, s, csc_of(L.A), n, (double *)aug.p);
    hipLaunchKernelGGL(amg_gj_k, dim3(1), dim3(GJT), 0, s, (double *)aug.p, (int)n, (double *)inv.p);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(s));
    (void)D;
    return ESP_OK;
}

// the whole hierarchy of h's current matrix into lv / inv
int32_t build(esp_precon *p, std::vector<AmgLevel> &lv, DevBuf &inv, bool *has_inv) {
    esp_handle *h = p->h;
    AmgData *D = p->amg;
    hipStream_t s = h->stream;
    const i64 n0 = h->n;
    *has_inv = false;
    // level 0: the checks on A itself, then its copy
    if (n0 > 0) {
        Temps tmp;
        DevBuf &st = tmp.b[0];
        CK(ensure(h, st, sizeof(u64) * 2));
        HIPCK(h, hipMemsetAsync(st.p, 0xFF, sizeof(u64) * 2, s));
        hipLaunchKernelGGL(amg_check_k, dim3(grid_for(n0, AT)), dim3(AT), 0, s, csc_of(h), n0, (unsigned long long *)st.p);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, st.p, sizeof(u64) * 2, hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        const unsigned long long nodiag = h->pin_scalar[0], unsym = h->pin_scalar[1];
        if (nodiag != ~0ull) FAIL(h, ESP_ERR_INVALID, "esp_precon_amg: column %llu has no stored diagonal entry", nodiag);
        if (unsym != ~0ull)
            FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_amg: the stored pattern is not structurally symmetric: column %llu holds an entry (i,j) without a stored (j,i)",
                 unsym);
    }
    {
        lv.emplace_back();
        AmgLevel &L = lv.back();
        L.n = n0;
        CK(amg_make_handle(h, n0, n0, &L.A));
        Temps tmp;
        DevBuf &cp = tmp.b[0], &rv = tmp.b[1], &nz = tmp.b[2];
        const i64 nnz = h->nnz;
        CK(ensure(h, cp, sizeof(i64) * (size_t)(n0 + 1)));
        CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(nnz, 1)));
        CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nnz, 1)));
        HIPCK(h, hipMemcpyAsync(cp.p, h->colptr.p, sizeof(i64) * (size_t)(n0 + 1), hipMemcpyDeviceToDevice, s));
        if (nnz > 0) {
            HIPCK(h, hipMemcpyAsync(rv.p, h->rowval.p, sizeof(i64) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
            HIPCK(h, hipMemcpyAsync(nz.p, h->nzval.p, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
        }
        HIPCK(h, hipStreamSynchronize(s));
        install(L.A, cp, rv, nz, nnz);
    }
    for (int l = 0;; l++) {
        AmgLevel &L = lv[(size_t)l];
        esp_handle *A = L.A;
        const i64 n = L.n;
        const size_t vb = sizeof(double) * (size_t)std::max<i64>(n, 1);
        Temps tmp;
        Handles hs;
        DevBuf &dinv = tmp.b[0], &dg = tmp.b[1], &nw = tmp.b[2];
        for (DevBuf *b : {&dinv, &dg, &nw, &L.w, &L.x0, &L.x1, &L.r}) CK(ensure(h, *b, vb));
        if (l > 0) CK(ensure(h, L.b, vb));
        // dinv, rho, w
        SUB(h, A, esp_jacobi_setup(A, (double *)dinv.p, 1));
        {
            esp_handle *S = nullptr;
            CK(amg_make_handle(h, n, n, &S));
            hs.v.push_back(S);
            SUB(h, S, esp_diag_scale(A, (const double *)dinv.p, 0, 1, S));
            SUB(h, S, esp_opnorm(S, INFINITY, &L.rho));
        }
        const double omega = (4.0 / 3.0) / L.rho;
        if (n > 0)
            hipLaunchKernelGGL(amg_diag_k, dim3(grid_for(n, AT)), dim3(AT), 0, s, csc_of(A), n, (const double *)dinv.p, omega, (double *)dg.p,
                               (double *)L.w.p, (double *)nw.p);
        HIPCK(h, hipGetLastError());
        SUB(h, A, csr_current(A));  // the row-wise index and values the sweeps stream
        bool coarsest = n <= (i64)D->max_coarse || l + 1 == D->max_levels;
        esp_handle *PT = nullptr;  // transpose(P_l)
        if (!coarsest && D->coarsen == ESP_AMG_COARSEN_RS) {
            // the splitting and, where it leaves 0 < nc < n, P_l and its transpose (rsamg.hip)
            const int32_t st = rsamg_coarsen(h, L, D->theta, &PT);
            hs.v.push_back(PT);
            CK(st);
            if (L.nc == 0 || L.nc == n) coarsest = true;
        } else if (!coarsest) {
            CK(aggregate(h, L, (const double *)dg.p, D->theta));
            if (L.nc == n) coarsest = true;
        }
        if (coarsest) {
            if (n <= (i64)ESP_AMG_DENSE_MAX) {
                CK(dense_inverse(h, D, L, inv));
                *has_inv = true;
            }
            HIPCK(h, hipStreamSynchronize(s));
            return ESP_OK;
        }
        const i64 nc = L.nc;
        esp_handle *AP = nullptr;
        if (D->coarsen == ESP_AMG_COARSEN_SA) {
            // T = transpose of the CSC one can write down
            esp_handle *TT = nullptr, *T = nullptr, *DA = nullptr, *DAT = nullptr;
            CK(amg_make_handle(h, nc, n, &TT));
            hs.v.push_back(TT);
            {
                Temps t2;
                DevBuf &cp = t2.b[0], &rv = t2.b[1], &nz = t2.b[2];
                CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
                CK(ensure(h, rv, sizeof(i64) * (size_t)n));
                CK(ensure(h, nz, sizeof(double) * (size_t)n));
                hipLaunchKernelGGL(amg_tt_k, dim3(grid_for(n + 1, AT)), dim3(AT), 0, s, (const i64 *)L.agg.p, n, (i64 *)cp.p, (i64 *)rv.p,
                                   (double *)nz.p);
                HIPCK(h, hipGetLastError());
                HIPCK(h, hipStreamSynchronize(s));
                install(TT, cp, rv, nz, n);
            }
            CK(amg_make_handle(h, n, nc, &T));
            hs.v.push_back(T);
            SUB(h, T, esp_transpose(TT, T, nullptr));
            // P = T + (Diagonal(-w)*A)*T
            CK(amg_make_handle(h, n, n, &DA));
            hs.v.push_back(DA);
            SUB(h, DA, esp_diag_scale(A, (const double *)nw.p, 0, 1, DA));
            CK(amg_make_handle(h, n, nc, &DAT));
            hs.v.push_back(DAT);
            SUB(h, DAT, esp_matmul(DA, T, DAT, nullptr));
            CK(amg_make_handle(h, n, nc, &L.P));
            SUB(h, L.P, esp_add(T, DAT, ESP_OP_ADD, L.P, nullptr));
        }
        // A_{l+1} = transpose(P)*(A*P)
        CK(amg_make_handle(h, n, nc, &AP));
        hs.v.push_back(AP);
        SUB(h, AP, esp_matmul(A, L.P, AP, nullptr));
        if (!PT) {
            CK(amg_make_handle(h, nc, n, &PT));
            hs.v.push_back(PT);
            SUB(h, PT, esp_transpose(L.P, PT, nullptr));
        }
        esp_handle *An = nullptr;
        CK(amg_make_handle(h, nc, nc, &An));
        lv.emplace_back();  // (L is stale from here)
        lv.back().A = An;
        lv.back().n = nc;
        SUB(h, An, esp_matmul(PT, AP, An, nullptr));
        SUB(h, lv[(size_t)l].P, csr_current(lv[(size_t)l].P));  // the prolongation streams P's row-wise index
    }
}

}  // namespace

int32_t amg_update(esp_precon *p) {
    esp_handle *h = p->h;
    AmgData *D = p->amg;
    CK(precon_check_handle(h, "esp_precon_update"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_amg: a column window / column shard");
    p->n = h->n;
    p->pattern_version = 0;  // (a failure below leaves a preconditioner that refuses ldiv! until the next good update!)
    std::vector<AmgLevel> lv;
    DevBuf inv;
    bool has_inv = false;
    int32_t st = ESP_OK;
    try {
        st = build(p, lv, inv, &has_inv);
    } catch (const std::exception &) {
        g_err = h->err = "esp_precon_amg: no host memory for the hierarchy";
        st = ESP_ERR_NOMEM;
    }
    if (st != ESP_OK) {
        release_levels(lv);
        release(inv);
        return st;
    }
    release_levels(D->lv);
    release(D->inv);
    D->lv.swap(lv);
    D->inv = inv;
    D->has_inv = has_inv;
    HIPCK(h, hipStreamSynchronize(h->stream));
    p->nnz = h->nnz;
    p->pattern_version = h->pattern_version;
    p->values_version = h->values_version;
    return ESP_OK;
}

void amg_release(esp_precon *p) {
    if (!p->amg) return;
    release_levels(p->amg->lv);
    release(p->amg->inv);
    delete p->amg;
    p->amg = nullptr;
}

namespace {

// the cycle on level l with the right-hand side b; fdst (level 0 only): where the level's last kernel stores; -> the result
const double *cycle(esp_precon *p, int l, const double *b, double *fdst, const double *sub) {
    AmgData *D = p->amg;
    hipStream_t s = p->h->stream;
    AmgLevel &L = D->lv[(size_t)l];
    const i64 n = L.n;
    const bool last = l + 1 == (int)D->lv.size();
    const unsigned g = grid_for(n, AT);
    double *x0 = (double *)L.x0.p, *x1 = (double *)L.x1.p;
    const double *w = (const double *)L.w.p;
    if (last && D->has_inv) {
        hipLaunchKernelGGL(amg_dense_k, dim3(grid_for(n, AT / 64)), dim3(AT), 0, s, (const double *)D->inv.p, b, x0, (int)n);
        if (fdst) hipLaunchKernelGGL(amg_finish_k, dim3(g), dim3(AT), 0, s, (const double *)x0, fdst, sub, n);
        return x0;
    }
    const u64 *rp = (const u64 *)L.A->csr_rowptr.p + 1;
    const u32 *col = (const u32 *)L.A->csr_col.p;
    const double *val = (const double *)L.A->csr_val.p;
    const int nops = D->pre + D->post + (last ? 0 : 1);
    int op = 0;
    const double *cur = nullptr;
    const double *nil = nullptr;
    // where the next kernel stores: the caller's vector for the level's last one, else the iterate that is not read
    auto target = [&](bool inplace) -> double * {
        op++;
        if (fdst && op == nops) return fdst;
        if (inplace) return cur == x0 ? x0 : x1;
        return cur == x0 ? x1 : x0;
    };
    auto subof = [&](const double *d) { return d == fdst ? sub : nil; };
    double *d = target(false);
    hipLaunchKernelGGL(amg_scale_k, dim3(g), dim3(AT), 0, s, w, b, d, subof(d), n);  // the first pre-sweep from x = 0
    cur = d;
    auto sweep = [&]() {
        double *t = target(false);
        hipLaunchKernelGGL((amg_row_k<SWEEP>), dim3(g), dim3(AT), 0, s, rp, col, val, cur, b, w, t, subof(t), n);
        cur = t;
    };
    for (int k = 1; k < D->pre; k++) sweep();
    if (!last) {
        AmgLevel &C = D->lv[(size_t)l + 1];
        const esp_handle *P = L.P;
        hipLaunchKernelGGL((amg_row_k<RESID>), dim3(g), dim3(AT), 0, s, rp, col, val, cur, b, nil, (double *)L.r.p, nil, n);
        hipLaunchKernelGGL(amg_restrict_k, dim3(grid_for(C.n, AT)), dim3(AT), 0, s, (const i64 *)P->colptr.p, (const i64 *)P->rowval.p,
                           (const double *)P->nzval.p, C.n, (const double *)L.r.p, (double *)C.b.p);
        const double *xc = cycle(p, l + 1, (const double *)C.b.p, nullptr, nullptr);
        double *t = target(true);
        hipLaunchKernelGGL((amg_row_k<PROLONG>), dim3(g), dim3(AT), 0, s, (const u64 *)P->csr_rowptr.p + 1, (const u32 *)P->csr_col.p,
                           (const double *)P->csr_val.p, xc, cur, nil, t, subof(t), n);
        cur = t;
    }
    for (int k = 0; k < D->post; k++) sweep();
    return cur;
}

}  // namespace

int32_t amg_solve(esp_precon *p, const double *v, double *u, bool sub) {
    esp_handle *h = p->h;
    if (!p->amg || p->amg->lv.empty()) FAIL(h, ESP_ERR_STATE, "esp_precon_amg: no hierarchy (update! first)");
    if (p->n == 0) return ESP_OK;
    (void)cycle(p, 0, v, u, sub ? u : nullptr);
    return ESP_OK;
}

namespace {
// esp_precon_amg_create / esp_precon_rsamg_create: the same arguments and rules, another coarsening and another default of theta
int32_t create(esp_handle *h, int32_t max_levels, int32_t max_coarse, int32_t presweeps, int32_t postsweeps, double theta, int coarsen,
               double theta_default, const char *what, esp_precon **out) {
    if (!h || !out) return ESP_ERR_INVALID;
    *out = nullptr;
    if (max_levels == -1) max_levels = 10;
    if (max_coarse == -1) max_coarse = 64;
    if (presweeps == -1) presweeps = 1;
    if (postsweeps == -1) postsweeps = 1;
    if (theta < 0.0) theta = theta_default;
    if (max_levels < 1) FAIL(h, ESP_ERR_INVALID, "%s: max_levels = %d (>= 1, or -1 for the default)", what, max_levels);
    if (max_coarse < 1 || max_coarse > ESP_AMG_DENSE_MAX)
        FAIL(h, ESP_ERR_INVALID, "%s: max_coarse = %d (1..%d, or -1 for the default)", what, max_coarse, ESP_AMG_DENSE_MAX);
    if (presweeps < 1) FAIL(h, ESP_ERR_INVALID, "%s: presweeps = %d (>= 1, or -1 for the default)", what, presweeps);
    if (postsweeps < 0) FAIL(h, ESP_ERR_INVALID, "%s: postsweeps = %d (>= 0, or -1 for the default)", what, postsweeps);
    if (!std::isfinite(theta)) FAIL(h, ESP_ERR_INVALID, "%s: theta is not finite", what);
    CK(precon_check_handle(h, what));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "%s: a column window / column shard", what);
    esp_precon *p = precon_new(h, ESP_PRECON_AMG);
    p->amg = new AmgData();
    p->amg->max_levels = max_levels;
    p->amg->max_coarse = max_coarse;
    p->amg->pre = presweeps;
    p->amg->post = postsweeps;
    p->amg->theta = theta;
    p->amg->coarsen = coarsen;
    return precon_finish(p, amg_update(p), out);
}
}  // namespace

extern "C" int32_t esp_precon_amg_create(esp_handle *h, int32_t max_levels, int32_t max_coarse, int32_t presweeps, int32_t postsweeps,
                                         double theta, esp_precon **out) {
    return create(h, max_levels, max_coarse, presweeps, postsweeps, theta, ESP_AMG_COARSEN_SA, 0.0, "esp_precon_amg_create", out);
}

extern "C" int32_t esp_precon_rsamg_create(esp_handle *h, int32_t max_levels, int32_t max_coarse, int32_t presweeps, int32_t postsweeps,
                                           double theta, esp_precon **out) {
    return create(h, max_levels, max_coarse, presweeps, postsweeps, theta, ESP_AMG_COARSEN_RS, 0.25, "esp_precon_rsamg_create", out);
}

extern "C" int32_t esp_precon_amg_coarsening(esp_precon *p, int32_t *kind) {
    if (!p || p->kind != ESP_PRECON_AMG || !kind) return ESP_ERR_INVALID;
    *kind = p->amg->coarsen;
    return ESP_OK;
}

extern "C" int32_t esp_precon_amg_levels(esp_precon *p, int32_t *nlevels) {
    if (!p || p->kind != ESP_PRECON_AMG || !nlevels) return ESP_ERR_INVALID;
    *nlevels = (int32_t)p->amg->lv.size();
    return ESP_OK;
}

extern "C" int32_t esp_precon_amg_level(esp_precon *p, int32_t level, esp_handle **a, esp_handle **prolong, int64_t *n, double *rho,
                                        int32_t *rounds) {
    if (!p || p->kind != ESP_PRECON_AMG) return ESP_ERR_INVALID;
    if (level < 0 || level >= (int32_t)p->amg->lv.size()) FAIL(p->h, ESP_ERR_INVALID, "esp_precon_amg_level: no level %d", level);
    const AmgLevel &L = p->amg->lv[(size_t)level];
    if (a) *a = L.A;
    if (prolong) *prolong = L.P;
    if (n) *n = L.n;
    if (rho) *rho = L.rho;
    if (rounds) *rounds = L.rounds;
    return ESP_OK;
}

extern "C" int32_t esp_precon_amg_aggregates(esp_precon *p, int32_t level, int64_t *agg, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_AMG) return ESP_ERR_INVALID;
    if (p->amg->coarsen != ESP_AMG_COARSEN_SA) FAIL(p->h, ESP_ERR_INVALID, "esp_precon_amg_aggregates: a Ruge-Stueben hierarchy has a splitting, no aggregates");
    if (level < 0 || level >= (int32_t)p->amg->lv.size()) FAIL(p->h, ESP_ERR_INVALID, "esp_precon_amg_aggregates: no level %d", level);
    const AmgLevel &L = p->amg->lv[(size_t)level];
    if (!L.has_agg) FAIL(p->h, ESP_ERR_INVALID, "esp_precon_amg_aggregates: level %d was not aggregated", level);
    if (!agg && L.n > 0) return ESP_ERR_INVALID;
    return copy_out(p->h, agg, L.agg.p, sizeof(i64) * (size_t)L.n, on_device);
}

extern "C" int32_t esp_precon_amg_splitting(esp_precon *p, int32_t level, int64_t *cf, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_AMG) return ESP_ERR_INVALID;
    if (p->amg->coarsen != ESP_AMG_COARSEN_RS) FAIL(p->h, ESP_ERR_INVALID, "esp_precon_amg_splitting: a smoothed-aggregation hierarchy has aggregates, no splitting");
    if (level < 0 || level >= (int32_t)p->amg->lv.size()) FAIL(p->h, ESP_ERR_INVALID, "esp_precon_amg_splitting: no level %d", level);
    const AmgLevel &L = p->amg->lv[(size_t)level];
    if (!L.has_split) FAIL(p->h, ESP_ERR_INVALID, "esp_precon_amg_splitting: level %d was not split", level);
    if (!cf && L.n > 0) return ESP_ERR_INVALID;
    return copy_out(p->h, cf, L.agg.p, sizeof(i64) * (size_t)L.n, on_device);
}

extern "C" int32_t esp_precon_amg_coarse_inverse(esp_precon *p, double *inv, int32_t on_device) {
    if (!p || p->kind != ESP_PRECON_AMG) return ESP_ERR_INVALID;
    if (!p->amg->has_inv || p->amg->lv.empty()) FAIL(p->h, ESP_ERR_INVALID, "esp_precon_amg_coarse_inverse: the coarsest level is only smoothed");
    const i64 n = p->amg->lv.back().n;
    if (!inv && n > 0) return ESP_ERR_INVALID;
    return copy_out(p->h, inv, p->amg->inv.p, sizeof(double) * (size_t)(n * n), on_device);
}
