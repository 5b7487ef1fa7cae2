// rsamg.hip -- libesparse_hip: the Ruge-Stueben coarsening of RS_AMGPreconditioner (esp_precon_rsamg_create)
// (see internal.hpp for the map of the translation units; the level container, the checks, the coarsest level and the V-cycle are
// amg.hip's and serve both coarsenings)
//
// The reference's RS_AMGPreconditioner (ext/ExtendableSparseAlgebraicMultigridExt.jl) wraps AlgebraicMultigrid.jl, whose splitting
// is a sequential sweep.  The algorithm here is stated in full in include/esparse_hip.h and DESIGN.md 5k; tests/rsamg_model.c
// restates it as plain loops and is normative for the order of every operation.  Everything below is bit-identical to that model.
//
// rsamg_coarsen, one level (its matrix A in L.A, the row-wise index of esp_mul current):
//   rs_rowmax_k     m_i = the largest |a_ik| over the stored k != i of row i (a NaN is never larger), over the row-wise index
//   rs_strength_k   one byte per CSC position of column i, entry (r,i): bit 0 "r depends on i" (r != i, |a_ri| != 0,
//                   |a_ri| >= theta*m_r), bit 1 "i depends on r" (the same test on the stored a_ir, found by csc_find); so a walk
//                   over column i sees S_i (bit 1), S_i^T (bit 0) and their union without a search.  lambda_i = |S_i^T| gives
//                   key(i) = min(lambda_i, 65535) << 48 | (mix(i) >> 16) << 32 | i; a node with an empty S_i is an F point
//                   without interpolation from the start (state 3), everybody else undecided (a plain store of 1 to the flag)
//   rs_pmis_k<1|2>  one round.  Phase 1 reads the round's start (state) and writes next: an undecided i whose key exceeds the key
//                   of every undecided neighbour in S_i + S_i^T becomes a C point.  Phase 2 reads next and writes state: a node
//                   still undecided with a C point in S_i becomes an F point, else it stays (a plain store of 1 to the round's
//                   flag, read back by the host).  Both are ORs over the column: order-free.  One lane per column; a column of
//                   more than AMG_LONG entries is folded by its whole wave, 64 entries at a time, as amg_luby_k does
//   rs_count_k      per row: is it a C point, and how many entries its row of P holds (C: 1, F: |S_i & C|, else 0); two scans give
//                   cnum and the column pointers of transpose(P)
//   rs_interp_k     direct interpolation, one lane per row over the row-wise index: the four sums in increasing k, then the
//                   entries in increasing k (cnum is monotone: the rows of transpose(P)'s column ascend); the splitting as the
//                   inspector reports it
//   P               transpose(P) is installed as it was written down; P = esp_transpose of it
#include "amg.hpp"

using namespace espamg;

namespace {

enum : u32 { UNDECIDED = 0u, CPOINT = 1u, FPOINT = 2u, FNONE = 3u };

// j in S_i by the row's own measure: not the diagonal, not zero, at least theta times the row's largest (false for a NaN)
__device__ __forceinline__ bool rs_strong(double a, double theta, double mi) {
    const double x = fabs(a);
    return x != 0.0 && x >= theta * mi;
}

// rp = csr_rowptr + 1: the entries of row i are [rp[i], rp[i+1]) of col / val, columns ascending
__global__ __launch_bounds__(AT) void rs_rowmax_k(const u64 *__restrict__ rp, const u32 *__restrict__ col, const double *__restrict__ val,
                                                  i64 n, double *__restrict__ m) {
    const i64 i = (i64)blockIdx.x * AT + threadIdx.x;
    if (i >= n) return;
    double mi = 0.0;
    const u64 kb = rp[i], ke = rp[i + 1];
    for (u64 k = kb; k < ke; k++) {
        if ((i64)col[k] == i) continue;
        const double x = fabs(val[k]);
        if (x > mi) mi = x;
    }
    m[i] = mi;
}

__global__ __launch_bounds__(AT) void rs_strength_k(espfold::Csc c, i64 n, const double *__restrict__ m, double theta,
                                                    uint8_t *__restrict__ flags, u64 *__restrict__ key, u32 *__restrict__ state,
                                                    u32 *__restrict__ flag) {
    const i64 i = (i64)blockIdx.x * AT + threadIdx.x;
    if (i >= n) return;
    const double mi = m[i];
    u32 lam = 0, ns = 0;
    for (i64 k = c.colptr[i] - 1; k < c.colptr[i + 1] - 1; k++) {
        const i64 r = c.rowval[k] - 1;
        uint8_t f = 0;
        if (r != i) {
            if (rs_strong(c.nzval[k], theta, m[r])) {  // a_ri: r depends on i
                f |= 1;
                lam++;
            }
            const i64 pos = espfold::csc_find(c, r, i);  // a_ir, in column r
            if (pos >= 0 && rs_strong(c.nzval[pos], theta, mi)) {  // i depends on r
                f |= 2;
                ns++;
            }
        }
        flags[k] = f;
    }
    key[i] = ((u64)(lam < 65535u ? lam : 65535u) << 48) | ((u64)(amg_mix(i) >> 16) << 32) | (u64)(u32)i;
    state[i] = ns > 0 ? UNDECIDED : FNONE;
    if (ns > 0) *flag = 1u;  // somebody is undecided: a plain store
}

// PH 1: out[j] = C point if the undecided j is not beaten by an undecided neighbour in S_j + S_j^T, else in[j]
// PH 2: out[j] = F point if the undecided j has a C point in S_j, else in[j]; flag = 1 if j stays undecided
// (in and out are two buffers: every lane reads its neighbours' in[] and writes its own out[] only)
template <int PH>
__global__ __launch_bounds__(AT) void rs_pmis_k(const i64 *__restrict__ colptr, const i64 *__restrict__ rowval,
                                                const uint8_t *__restrict__ flags, const u64 *__restrict__ key, i64 n,
                                                const u32 *__restrict__ in, u32 *__restrict__ out, u32 *__restrict__ flag) {
    const i64 j = (i64)blockIdx.x * AT + threadIdx.x;
    const int lane = threadIdx.x & 63;
    i64 s = 0, e = 0;
    u64 kj = 0;
    u32 st = FNONE;
    if (j < n) {
        st = in[j];
        if (st == UNDECIDED) {
            s = colptr[j] - 1;
            e = colptr[j + 1] - 1;
            if (PH == 1) kj = key[j];
        }
    }
    bool hit = false;  // PH 1: beaten; PH 2: a C point in S_j
    const bool longc = e - s > AMG_LONG;
    if (!longc) {
        for (i64 k = s; k < e; k++) {
            const uint8_t f = flags[k];
            if (PH == 1 ? f == 0 : (f & 2) == 0) continue;
            const i64 r = rowval[k] - 1;
            if (PH == 1) hit = hit || (in[r] == UNDECIDED && key[r] > kj);
            else hit = hit || in[r] == CPOINT;
        }
    }
    // the wave's long columns one after the other, 64 entries at a time (every lane of the wave gets here: nobody left early)
    u64 mask = __ballot(longc);
    while (mask) {
        const int sl = __builtin_ctzll(mask);
        mask &= mask - 1;
        const i64 ls = __shfl(s, sl), le = __shfl(e, sl);
        const u64 lk = __shfl(kj, sl);
        bool v = false;
        for (i64 b = ls; b < le; b += 64) {
            const i64 k = b + lane;
            if (k < le) {
                const uint8_t f = flags[k];
                if (PH == 1 ? f != 0 : (f & 2) != 0) {
                    const i64 r = rowval[k] - 1;
                    if (PH == 1) v = v || (in[r] == UNDECIDED && key[r] > lk);
                    else v = v || in[r] == CPOINT;
                }
            }
        }
        const bool any = __ballot(v) != 0ull;
        if (lane == sl) hit = any;
    }
    if (j >= n) return;
    if (st == UNDECIDED) {
        if (PH == 1) {
            if (!hit) st = CPOINT;
        } else {
            if (hit) st = FPOINT;
            else *flag = 1u;  // somebody is still undecided: a plain store
        }
    }
    out[j] = st;
}

// num[i] = 1 for a C point, cnt[i] = the entries of row i of P; both n + 1 long with a zero at the end (for the exclusive scans)
__global__ __launch_bounds__(AT) void rs_count_k(const u64 *__restrict__ rp, const u32 *__restrict__ col, const double *__restrict__ val,
                                                 i64 n, const double *__restrict__ m, double theta, const u32 *__restrict__ state,
                                                 i64 *__restrict__ num, i64 *__restrict__ cnt) {
    const i64 i = (i64)blockIdx.x * AT + threadIdx.x;
    if (i > n) return;
    i64 c = 0, isc = 0;
    if (i < n) {
        const u32 st = state[i];
        if (st == CPOINT) {
            c = isc = 1;
        } else if (st == FPOINT) {
            const double mi = m[i];
            const u64 kb = rp[i], ke = rp[i + 1];
            for (u64 k = kb; k < ke; k++) {
                const i64 j = (i64)col[k];
                if (j != i && rs_strong(val[k], theta, mi) && state[j] == CPOINT) c++;
            }
        }
    }
    num[i] = isc;
    cnt[i] = c;
}

// num, cnt: scanned.  Column i of transpose(P) (nc x n): cp[i] = cnt[i] + 1, its rows cnum(j) + 1 and values; cf[i]: the splitting
__global__ __launch_bounds__(AT) void rs_interp_k(const u64 *__restrict__ rp, const u32 *__restrict__ col, const double *__restrict__ val,
                                                  i64 n, const double *__restrict__ m, double theta, const u32 *__restrict__ state,
                                                  const i64 *__restrict__ num, const i64 *__restrict__ cnt, i64 *__restrict__ cp,
                                                  i64 *__restrict__ rv, double *__restrict__ nz, i64 *__restrict__ cf) {
    const i64 i = (i64)blockIdx.x * AT + threadIdx.x;
    if (i > n) return;
    i64 q = cnt[i];
    cp[i] = q + 1;
    if (i == n) return;
    const u32 st = state[i];
    if (st == CPOINT) {
        rv[q] = num[i] + 1;
        nz[q] = 1.0;
        cf[i] = num[i];
        return;
    }
    cf[i] = st == FPOINT ? -1 : -2;
    if (st != FPOINT) return;
    const double mi = m[i];
    const u64 kb = rp[i], ke = rp[i + 1];
    double sn = 0.0, sp = 0.0, snc = 0.0, spc = 0.0, d = 0.0;
    for (u64 k = kb; k < ke; k++) {
        const i64 j = (i64)col[k];
        const double a = val[k];
        if (j == i) {
            d = a;
            continue;
        }
        const bool inc = rs_strong(a, theta, mi) && state[j] == CPOINT;
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
    for (u64 k = kb; k < ke; k++) {
        const i64 j = (i64)col[k];
        const double a = val[k];
        if (j == i || !(rs_strong(a, theta, mi) && state[j] == CPOINT)) continue;
        rv[q] = num[j] + 1;
        nz[q] = (-(a < 0.0 ? alpha : beta) * a) / d;
        q++;
    }
}

}  // namespace

int32_t rsamg_coarsen(esp_handle *h, AmgLevel &L, double theta, esp_handle **tt) {
    hipStream_t s = h->stream;
    esp_handle *A = L.A;
    const i64 n = L.n, nnz = A->nnz;
    const espfold::Csc c = csc_of(A);
    const u64 *rp = (const u64 *)A->csr_rowptr.p + 1;
    const u32 *col = (const u32 *)A->csr_col.p;
    const double *val = (const double *)A->csr_val.p;
    *tt = nullptr;
    Temps tmp;
    DevBuf &m = tmp.b[0], &flags = tmp.b[1], &key = tmp.b[2], &st0 = tmp.b[3], &st1 = tmp.b[4], &flag = tmp.b[5], &num = tmp.b[6],
           &cnt = tmp.b[7], &ws = tmp.b[8];
    const unsigned g = grid_for(n, AT), g1 = grid_for(n + 1, AT);
    CK(ensure(h, m, sizeof(double) * (size_t)n));
    CK(ensure(h, flags, (size_t)std::max<i64>(nnz, 1)));
    CK(ensure(h, key, sizeof(u64) * (size_t)n));
    CK(ensure(h, st0, sizeof(u32) * (size_t)n));
    CK(ensure(h, st1, sizeof(u32) * (size_t)n));
    CK(ensure(h, flag, sizeof(u32) * 2));
    CK(ensure(h, num, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, cnt, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, L.agg, sizeof(i64) * (size_t)n));
    u32 *state = (u32 *)st0.p, *next = (u32 *)st1.p;
    // strength, keys, the first states
    HIPCK(h, hipMemsetAsync(flag.p, 0, sizeof(u32) * 2, s));
    hipLaunchKernelGGL(rs_rowmax_k, dim3(g), dim3(AT), 0, s, rp, col, val, n, (double *)m.p);
    hipLaunchKernelGGL(rs_strength_k, dim3(g), dim3(AT), 0, s, c, n, (const double *)m.p, theta, (uint8_t *)flags.p, (u64 *)key.p, state,
                       (u32 *)flag.p);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, flag.p, sizeof(u32), hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    L.rounds = 0;
    while (*(const u32 *)h->pin_scalar != 0u) {  // the globally largest undecided key decides in every round: at most n rounds
        if ((i64)L.rounds >= n) FAIL(h, ESP_ERR_HIP, "esp_precon_rsamg: the splitting did not end after %lld rounds", (long long)n);
        HIPCK(h, hipMemsetAsync(flag.p, 0, sizeof(u32) * 2, s));
        hipLaunchKernelGGL(rs_pmis_k<1>, dim3(g), dim3(AT), 0, s, c.colptr, c.rowval, (const uint8_t *)flags.p, (const u64 *)key.p, n,
                           (const u32 *)state, next, (u32 *)nullptr);
        hipLaunchKernelGGL(rs_pmis_k<2>, dim3(g), dim3(AT), 0, s, c.colptr, c.rowval, (const uint8_t *)flags.p, (const u64 *)key.p, n,
                           (const u32 *)next, state, (u32 *)flag.p);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, flag.p, sizeof(u32), hipMemcpyDeviceToHost, s));
        HIPCK(h, hipStreamSynchronize(s));
        L.rounds++;
    }
    // cnum and the column pointers of transpose(P)
    hipLaunchKernelGGL(rs_count_k, dim3(g1), dim3(AT), 0, s, rp, col, val, n, (const double *)m.p, theta, (const u32 *)state, (i64 *)num.p,
                       (i64 *)cnt.p);
    HIPCK(h, hipGetLastError());
    int l = 0;
    CK(scan_inplace<i64, false>(h, (i64 *)num.p, n + 1, ws, &l));
    CK(scan_inplace<i64, false>(h, (i64 *)cnt.p, n + 1, ws, &l));
    i64 nzp = 0;
    CK(read_i64(h, (const i64 *)num.p + n, &L.nc));
    CK(read_i64(h, (const i64 *)cnt.p + n, &nzp));
    if (L.nc < 0 || L.nc > n || nzp < L.nc || nzp > nnz + n)
        FAIL(h, ESP_ERR_HIP, "esp_precon_rsamg: the splitting is inconsistent (%lld C points of %lld, %lld entries)", (long long)L.nc, (long long)n,
             (long long)nzp);
    // the interpolation, written down as transpose(P)
    Temps t2;
    DevBuf &cp = t2.b[0], &rv = t2.b[1], &nz = t2.b[2];
    CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(nzp, 1)));
    CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nzp, 1)));
    hipLaunchKernelGGL(rs_interp_k, dim3(g1), dim3(AT), 0, s, rp, col, val, n, (const double *)m.p, theta, (const u32 *)state,
                       (const i64 *)num.p, (const i64 *)cnt.p, (i64 *)cp.p, (i64 *)rv.p, (double *)nz.p, (i64 *)L.agg.p);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(s));
    L.has_split = true;
    if (L.nc == 0 || L.nc == n) return ESP_OK;  // nothing to coarsen to: the caller makes this the coarsest level
    esp_handle *TT = nullptr;
    CK(amg_make_handle(h, L.nc, n, &TT));
    *tt = TT;  // (the caller's: also where a step below fails)
    install(TT, cp, rv, nz, nzp);
    CK(amg_make_handle(h, n, L.nc, &L.P));
    SUB(h, L.P, esp_transpose(TT, L.P, nullptr));
    return ESP_OK;
}
