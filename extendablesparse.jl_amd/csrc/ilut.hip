// ilut.hip -- libesparse_hip: ILUTPreconditioner, the threshold ILU by synchronous sweeps (ParILUT family), on the device CSC (see
// internal.hpp for the map of the translation units; the algorithm: include/esparse_hip.h, esp_precon_ilut_create)
//
// State: a pattern S and values F on it (the scaled unit-lower L below the diagonal, U on and above it) in the internal handle
// der.bh; der.inner is an ILUAM preconditioner of that handle in its PREFACTORED mode (iluam.hip: the values are the factorization,
// the analysis and both solves are ILUAM's), so ldiv!, the solvers' dispatch, get_factor and levels are ILU(k)'s paths.
//
// One sweep (ilut_sweep_k) computes every entry at once from the previous values -- F_old is read, F_new written, nothing else:
//   r = a_ij (through apos: the position in A, or +0.0 for fill); r = r - l_ik*u_kj for k < min(i,j), k increasing, where the
//   pattern holds (i,k) and (k,j); l_ij = r / u_jj(old) below the diagonal, u_ij = r on and above it.
// Every entry of column j shares the column's part above the diagonal (rows k < j with u_kj), so a column is served by one group of
// lanes that stages those rows and old values in LDS once; each lane then takes entries (i,j) and merges row i's part left of
// min(i,j) -- from the row-wise index of the pattern's handle (build_csr: columns ascending, positions beside them) -- against it.
//   wave tier       one wave per column, four columns per workgroup, up to ESP_ILUT_WAVE_UPPER rows above the diagonal
//   workgroup tier  256 lanes per column, up to ESP_ILUT_GROUP_UPPER rows (48 KiB of LDS)
//   stride tier     256 lanes stride the column and merge against the column in global memory: any length
// The columns of the two upper tiers are listed when the pattern changes (ilut_tiers_k).
// One step: (L+I) and U of the state go to two internal handles with every value 1.0, esp_matmul gives C = pattern((L+I)*U) (its
// values are discarded), F is carried to C by bisection in the column (+0.0 at new positions) together with apos, the fill guard is
// checked, s sweeps run on C, the drop rule marks, a scan over the per-column counts and a compaction give S, s sweeps run on S.
// Nothing of p changes before the last step succeeded: the work lives on the two work handles and goes into der.bh at the end.
#include "internal.hpp"

namespace {

constexpr int WAVE = 64, GROUP = 256;
constexpr int WAVE_COLS = GROUP / WAVE;  // columns per workgroup of the wave tier
constexpr u32 NO_POS = 0xFFFFFFFFu;      // apos of a fill position (every update! refuses nnz(A) >= 2^32 - 16)
static_assert((size_t)ESP_ILUT_GROUP_UPPER * 12 <= 64 * 1024, "rows and values of the workgroup tier in LDS");
static_assert(ESP_ILUT_WAVE_UPPER < ESP_ILUT_GROUP_UPPER, "the tiers follow each other");

struct SweepArgs {
    const i64 *cp, *rv;    // the pattern, Julia's arrays
    const u32 *dpos;       // 0-based position of (j,j)
    const u64 *rp;         // row-wise index: row i = [rp[i], rp[i + 1]) of rcol / rpos, columns ascending
    const u32 *rcol, *rpos;
    const u32 *apos;       // position in A's nzval, or NO_POS
    const double *anz;
    const double *fold;
    double *fnew;
};

// T lanes per column, COLS columns per workgroup, CAP staged rows per column (0: the column is read where it lies).  list == nullptr:
// every column (the wave tier: a column with more than ESP_ILUT_WAVE_UPPER rows above its diagonal is left to the listed tiers);
// else the listed columns
template <int T, int COLS, int CAP>
__global__ __launch_bounds__(T *COLS) void ilut_sweep_k(SweepArgs a, i64 n, const u32 *__restrict__ list, i64 count) {
    __shared__ u32 srow[COLS][CAP > 0 ? CAP : 1];
    __shared__ double sval[COLS][CAP > 0 ? CAP : 1];
    const int w = threadIdx.x / T, t = threadIdx.x % T;
    const i64 idx = (i64)blockIdx.x * COLS + w;
    bool live = idx < count;
    i64 j = 0, cb = 0, ce = 0, d = 0;
    if (live) {
        j = list ? (i64)list[idx] : idx;
        cb = a.cp[j] - 1;
        ce = a.cp[j + 1] - 1;
        d = a.dpos[j];
        if (!list && d - cb > (i64)ESP_ILUT_WAVE_UPPER) live = false;  // (listed: a wider tier writes this column)
    }
    const int up = live ? (int)std::min<i64>(d - cb, CAP > 0 ? CAP : 0x7FFFFFFF) : 0;  // (a listed column never exceeds its tier's CAP)
    if (CAP > 0) {
        for (int x = t; x < up; x += T) {
            srow[w][x] = (u32)(a.rv[cb + x] - 1);
            sval[w][x] = a.fold[cb + x];
        }
        __syncthreads();
    }
    if (!live) return;
    const double piv = a.fold[d];
    for (i64 q = cb + t; q < ce; q += T) {
        const u32 i = (u32)(a.rv[q] - 1);
        const u32 src = a.apos[q];
        double r = src == NO_POS ? 0.0 : a.anz[src];
        const u32 m = i < (u32)j ? i : (u32)j;
        u64 ra = a.rp[i];
        const u64 re = a.rp[i + 1];
        int c = 0;
        if ((re - ra) * 8 < (u64)up) {  // a short row against a long column: the row's columns looked up by bisection, in the same order
            for (; ra < re; ra++) {
                const u32 ka = a.rcol[ra];
                if (ka >= m) break;
                int hi = up;
                while (c < hi) {
                    const int mid = c + ((hi - c) >> 1);
                    const u32 km = CAP > 0 ? srow[w][mid] : (u32)(a.rv[cb + mid] - 1);
                    if (km < ka) c = mid + 1;
                    else hi = mid;
                }
                if (c == up) break;
                const u32 kc = CAP > 0 ? srow[w][c] : (u32)(a.rv[cb + c] - 1);
                if (kc != ka) continue;
                const double u = CAP > 0 ? sval[w][c] : a.fold[cb + c];
                r = r - a.fold[a.rpos[ra]] * u;
                c++;
            }
            ra = re;
        }
        while (ra < re && c < up) {
            const u32 ka = a.rcol[ra];
            const u32 kc = CAP > 0 ? srow[w][c] : (u32)(a.rv[cb + c] - 1);
            if (ka >= m || kc >= m) break;
            if (ka < kc) ra++;
            else if (kc < ka) c++;
            else {
                const double u = CAP > 0 ? sval[w][c] : a.fold[cb + c];
                r = r - a.fold[a.rpos[ra]] * u;
                ra++;
                c++;
            }
        }
        a.fnew[q] = i > (u32)j ? r / piv : r;
    }
}

// ---- what runs when a pattern is new ---------------------------------------------------------------------------------------------
// dpos[j] by bisection; missing: the smallest 1-based column without a stored diagonal
__global__ void ilut_diag_k(espfold::Csc c, i64 n, u32 *__restrict__ dpos, unsigned long long *__restrict__ missing) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const i64 pos = espfold::csc_find(c, j, j);
    if (pos < 0) atomicMin(missing, (unsigned long long)(j + 1));
    dpos[j] = pos < 0 ? 0u : (u32)pos;
}
// the columns of the workgroup tier (list) and of the stride tier (list + n); cnt[0], cnt[1]: how many
__global__ void ilut_tiers_k(const i64 *__restrict__ cp, const u32 *__restrict__ dpos, i64 n, u32 *__restrict__ list,
                             unsigned long long *__restrict__ cnt) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const i64 up = (i64)dpos[j] - (cp[j] - 1);
    if (up > (i64)ESP_ILUT_GROUP_UPPER) list[n + (i64)atomicAdd(&cnt[1], 1ull)] = (u32)j;
    else if (up > (i64)ESP_ILUT_WAVE_UPPER) list[(i64)atomicAdd(&cnt[0], 1ull)] = (u32)j;
}
// initialisation on pattern(A): u_ij = a_ij, l_ij = a_ij / a_jj; apos = the position itself (one wave per column)
__global__ __launch_bounds__(GROUP) void ilut_init_k(const i64 *__restrict__ cp, const i64 *__restrict__ rv, const double *__restrict__ anz,
                                                     const u32 *__restrict__ dpos, i64 n, double *__restrict__ f, u32 *__restrict__ apos) {
    const i64 j = (i64)blockIdx.x * WAVE_COLS + threadIdx.x / WAVE;
    if (j >= n) return;
    const double piv = anz[dpos[j]];
    for (i64 q = cp[j] - 1 + (threadIdx.x % WAVE); q < cp[j + 1] - 1; q += WAVE) {
        f[q] = rv[q] - 1 > j ? anz[q] / piv : anz[q];
        apos[q] = (u32)q;
    }
}
// (L+I) and U of the pattern as matrices of ones: the column counts, then the rows
__global__ void ilut_split_count_k(const i64 *__restrict__ cp, const u32 *__restrict__ dpos, i64 n, i64 *__restrict__ lcp, i64 *__restrict__ ucp) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    lcp[j] = j < n ? (cp[j + 1] - 1) - (i64)dpos[j] : 0;
    ucp[j] = j < n ? (i64)dpos[j] - (cp[j] - 1) + 1 : 0;
}
__global__ __launch_bounds__(GROUP) void ilut_split_fill_k(const i64 *__restrict__ cp, const i64 *__restrict__ rv, const u32 *__restrict__ dpos, i64 n,
                                                           const i64 *__restrict__ lcp, const i64 *__restrict__ ucp, i64 *__restrict__ lrv,
                                                           double *__restrict__ lnz, i64 *__restrict__ urv, double *__restrict__ unz) {
    const i64 j = (i64)blockIdx.x * WAVE_COLS + threadIdx.x / WAVE;
    if (j >= n) return;
    const i64 cb = cp[j] - 1, d = dpos[j];
    for (i64 q = cb + (threadIdx.x % WAVE); q < cp[j + 1] - 1; q += WAVE) {
        if (q >= d) {
            lrv[lcp[j] + (q - d)] = rv[q];
            lnz[lcp[j] + (q - d)] = 1.0;
        }
        if (q <= d) {
            urv[ucp[j] + (q - cb)] = rv[q];
            unz[ucp[j] + (q - cb)] = 1.0;
        }
    }
}
// F carried from S to C (+0.0 at a new position), apos of every position of C: two bisections per entry (one wave per column)
__global__ __launch_bounds__(GROUP) void ilut_carry_k(const i64 *__restrict__ ccp, const i64 *__restrict__ crv, i64 n, espfold::Csc S, espfold::Csc A,
                                                      double *__restrict__ f, u32 *__restrict__ apos) {
    const i64 j = (i64)blockIdx.x * WAVE_COLS + threadIdx.x / WAVE;
    if (j >= n) return;
    for (i64 q = ccp[j] - 1 + (threadIdx.x % WAVE); q < ccp[j + 1] - 1; q += WAVE) {
        const i64 i = crv[q] - 1;
        const i64 ps = espfold::csc_find(S, j, i), pa = espfold::csc_find(A, j, i);
        f[q] = ps >= 0 ? S.nzval[ps] : 0.0;
        apos[q] = pa >= 0 ? (u32)pa : NO_POS;
    }
}
// the drop rule: an off-diagonal (i,j) goes when fabs(l_ij) < tau (i > j) or fabs(u_ij) < tau*fabs(u_ii) (i < j) is true
__device__ __forceinline__ bool ilut_kept(const double *f, const u32 *dpos, i64 i, i64 j, i64 q, double tau) {
    if (i > j) return !(fabs(f[q]) < tau);
    if (i < j) return !(fabs(f[q]) < tau * fabs(f[dpos[i]]));
    return true;
}
__global__ void ilut_drop_count_k(const i64 *__restrict__ cp, const i64 *__restrict__ rv, const double *__restrict__ f, const u32 *__restrict__ dpos,
                                  i64 n, double tau, i64 *__restrict__ ncp) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    i64 c = 0;
    if (j < n)
        for (i64 q = cp[j] - 1; q < cp[j + 1] - 1; q++) c += ilut_kept(f, dpos, rv[q] - 1, j, q, tau) ? 1 : 0;
    ncp[j] = c;
}
// ncp: the scanned 0-based starts.  The kept entries of every column in order: rows, values, apos; the new diagonal positions
__global__ void ilut_compact_k(const i64 *__restrict__ cp, const i64 *__restrict__ rv, const double *__restrict__ f, const u32 *__restrict__ dpos,
                               const u32 *__restrict__ apos, i64 n, double tau, const i64 *__restrict__ ncp, i64 *__restrict__ nrv,
                               double *__restrict__ nf, u32 *__restrict__ napos, u32 *__restrict__ ndpos) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    i64 o = ncp[j];
    for (i64 q = cp[j] - 1; q < cp[j + 1] - 1; q++) {
        const i64 i = rv[q] - 1;
        if (!ilut_kept(f, dpos, i, j, q, tau)) continue;
        if (i == j) ndpos[j] = (u32)o;
        nrv[o] = rv[q];
        nf[o] = f[q];
        napos[o] = apos[q];
        o++;
    }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------
// a pattern with values on a handle (its CSC and row-wise index), and what the sweeps need beside it
struct Work {
    esp_handle *hd = nullptr;
    DevBuf alt, apos, dpos, list;  // the second value array, u32 nnz, u32 n, u32 2 n
    i64 tiers[2] = {0, 0};         // columns of the workgroup / stride tier
    ~Work() {
        for (DevBuf *b : {&alt, &apos, &dpos, &list}) release(*b);
    }
};

espfold::Csc csc_of(const esp_handle *h) { return espfold::Csc{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (double *)h->nzval.p, h->nnz}; }

// behind a pattern change of w.hd (dpos is current): the tier lists, the row-wise index, room for the second value array
int32_t work_ready(esp_precon *p, Work &w, unsigned long long *st) {
    esp_handle *h = p->h, *hd = w.hd;
    const i64 n = p->n;
    hipStream_t s = h->stream;
    CK(ensure(h, w.list, sizeof(u32) * (size_t)std::max<i64>(2 * n, 1)));
    CK(ensure(h, w.alt, sizeof(double) * (size_t)std::max<i64>(hd->nnz, 1)));
    HIPCK(h, hipMemsetAsync(st, 0, sizeof(u64) * 2, s));
    if (n > 0)
        hipLaunchKernelGGL(ilut_tiers_k, dim3(grid_for(n, 256)), dim3(256), 0, s, (const i64 *)hd->colptr.p, (const u32 *)w.dpos.p, n, (u32 *)w.list.p, st);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, st, sizeof(u64) * 2, hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    w.tiers[0] = (i64)h->pin_scalar[0];
    w.tiers[1] = (i64)h->pin_scalar[1];
    if (hd->csr_version != hd->pattern_version) {
        const int32_t cs = build_csr(hd);
        if (cs != ESP_OK) FAIL(h, cs, "esp_precon_ilut: the row-wise index: %s", hd->err.c_str());
        hd->csr_val_version = 0;
    }
    return ESP_OK;
}

// `count` sweeps over the pattern of hd: its nzval holds the current values before and after (the two arrays change places)
int32_t run_sweeps(esp_precon *p, esp_handle *hd, DevBuf &alt, const DevBuf &apos, const DevBuf &dpos, const DevBuf &list, const i64 tiers[2],
                   int count) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    if (n == 0 || hd->nnz == 0) return ESP_OK;
    hipStream_t s = h->stream;
    SweepArgs a{(const i64 *)hd->colptr.p, (const i64 *)hd->rowval.p, (const u32 *)dpos.p,  (const u64 *)hd->csr_rowptr.p + 1,
                (const u32 *)hd->csr_col.p, (const u32 *)hd->csr_perm.p, (const u32 *)apos.p, (const double *)h->nzval.p,
                nullptr,                    nullptr};
    for (int t = 0; t < count; t++) {
        a.fold = (const double *)hd->nzval.p;
        a.fnew = (double *)alt.p;
        hipLaunchKernelGGL((ilut_sweep_k<WAVE, WAVE_COLS, ESP_ILUT_WAVE_UPPER>), dim3(grid_for(n, WAVE_COLS)), dim3(GROUP), 0, s, a, n,
                           (const u32 *)nullptr, n);
        if (tiers[0] > 0)
            hipLaunchKernelGGL((ilut_sweep_k<GROUP, 1, ESP_ILUT_GROUP_UPPER>), dim3((unsigned)tiers[0]), dim3(GROUP), 0, s, a, n,
                               (const u32 *)list.p, tiers[0]);
        if (tiers[1] > 0)
            hipLaunchKernelGGL((ilut_sweep_k<GROUP, 1, 0>), dim3((unsigned)tiers[1]), dim3(GROUP), 0, s, a, n, (const u32 *)list.p + n, tiers[1]);
        std::swap(hd->nzval, alt);
    }
    hd->values_version++;
    HIPCK(h, hipGetLastError());
    return ESP_OK;
}
int32_t run_sweeps(esp_precon *p, Work &w, int count) { return run_sweeps(p, w.hd, w.alt, w.apos, w.dpos, w.list, w.tiers, count); }

// derived_update's builder: the whole construction from A's current CSC; S and F go into p->der.bh, the sweep's companions into p.
// Nothing of p changes when it fails (the work handles are scratch)
int32_t build_f(esp_precon *p) {
    esp_handle *h = p->h, *bh = p->der.bh;
    hipStream_t s = h->stream;
    const i64 n = p->n, nnzA = h->nnz;
    const double tau = p->ilut_tau;
    const int steps = p->ilut_steps, sweeps = p->ilut_sweeps;
    Temps tmp;
    DevBuf &stat = tmp.b[0], &ws = tmp.b[1], &cp = tmp.b[2], &rv = tmp.b[3], &nz = tmp.b[4], &cp2 = tmp.b[5], &rv2 = tmp.b[6], &nz2 = tmp.b[7];
    Work cur, cand;  // the state S and the candidates C
    cur.hd = p->ilut_h[0];
    cand.hd = p->ilut_h[1];
    esp_handle *lh = p->ilut_h[2], *uh = p->ilut_h[3];
    i64 stats[ESP_ILUT_STATS] = {0};
    int l = 0;
    CK(ensure(h, stat, sizeof(u64) * 8));
    unsigned long long *st = (unsigned long long *)stat.p;  // 0 / 1: the tier counters, 2: the smallest column without a diagonal
    // A's diagonal; S = pattern(A) with the initial values
    CK(ensure(h, cur.dpos, sizeof(u32) * (size_t)std::max<i64>(n, 1)));
    hipLaunchKernelGGL(fill_i64_k, dim3(1), dim3(1), 0, s, (i64 *)st + 2, (i64)1, (i64)-1);
    if (n > 0) hipLaunchKernelGGL(ilut_diag_k, dim3(grid_for(n, 256)), dim3(256), 0, s, csc_of(h), n, (u32 *)cur.dpos.p, st + 2);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, st + 2, sizeof(u64), hipMemcpyDeviceToHost, s));
    HIPCK(h, hipStreamSynchronize(s));
    if (h->pin_scalar[0] != ~0ull)
        FAIL(h, ESP_ERR_INVALID, "esp_precon_ilut: column %llu has no stored diagonal entry", (unsigned long long)h->pin_scalar[0]);
    CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(nnzA, 1)));
    CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nnzA, 1)));
    CK(ensure(h, cur.apos, sizeof(u32) * (size_t)std::max<i64>(nnzA, 1)));
    HIPCK(h, hipMemcpyAsync(cp.p, h->colptr.p, sizeof(i64) * (size_t)(n + 1), hipMemcpyDeviceToDevice, s));
    if (nnzA > 0) HIPCK(h, hipMemcpyAsync(rv.p, h->rowval.p, sizeof(i64) * (size_t)nnzA, hipMemcpyDeviceToDevice, s));
    if (n > 0)
        hipLaunchKernelGGL(ilut_init_k, dim3(grid_for(n, WAVE_COLS)), dim3(GROUP), 0, s, (const i64 *)h->colptr.p, (const i64 *)h->rowval.p,
                           (const double *)h->nzval.p, (const u32 *)cur.dpos.p, n, (double *)nz.p, (u32 *)cur.apos.p);
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipStreamSynchronize(s));
    install(cur.hd, cp, rv, nz, nnzA);
    CK(work_ready(p, cur, st));
    i64 run = 0;
    if (steps == 0) {
        CK(run_sweeps(p, cur, sweeps));
        run += sweeps;
    }
    for (int t = 0; t < steps && n > 0; t++) {
        // (L+I) and U as matrices of ones, C = pattern((L+I)*U)
        CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
        CK(ensure(h, cp2, sizeof(i64) * (size_t)(n + 1)));
        hipLaunchKernelGGL(ilut_split_count_k, dim3(grid_for(n + 1, 256)), dim3(256), 0, s, (const i64 *)cur.hd->colptr.p, (const u32 *)cur.dpos.p, n,
                           (i64 *)cp.p, (i64 *)cp2.p);
        CK(scan_inplace<i64, false>(h, (i64 *)cp.p, n + 1, ws, &l));
        CK(scan_inplace<i64, false>(h, (i64 *)cp2.p, n + 1, ws, &l));
        const i64 nS = cur.hd->nnz;  // nnz(L+I) + nnz(U) = nnz(S) + n
        i64 zl = 0, zu = 0;
        CK(read_i64(h, (const i64 *)cp.p + n, &zl));
        CK(read_i64(h, (const i64 *)cp2.p + n, &zu));
        if (zl + zu != nS + n) FAIL(h, ESP_ERR_HIP, "esp_precon_ilut: the split of F holds %lld + %lld entries of %lld", (long long)zl, (long long)zu, (long long)(nS + n));
        CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(zl, 1)));
        CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(zl, 1)));
        CK(ensure(h, rv2, sizeof(i64) * (size_t)std::max<i64>(zu, 1)));
        CK(ensure(h, nz2, sizeof(double) * (size_t)std::max<i64>(zu, 1)));
        if (n > 0)
            hipLaunchKernelGGL(ilut_split_fill_k, dim3(grid_for(n, WAVE_COLS)), dim3(GROUP), 0, s, (const i64 *)cur.hd->colptr.p, (const i64 *)cur.hd->rowval.p,
                               (const u32 *)cur.dpos.p, n, (const i64 *)cp.p, (const i64 *)cp2.p, (i64 *)rv.p, (double *)nz.p, (i64 *)rv2.p, (double *)nz2.p);
        add_one_launch(s, (i64 *)cp.p, n + 1);
        add_one_launch(s, (i64 *)cp2.p, n + 1);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipStreamSynchronize(s));
        install(lh, cp, rv, nz, zl);
        install(uh, cp2, rv2, nz2, zu);
        int64_t nnzC = 0;
        const int32_t ms = esp_matmul(lh, uh, cand.hd, &nnzC);
        if (ms != ESP_OK) FAIL(h, ms, "esp_precon_ilut: the candidate pattern of step %d: %s", t, cand.hd->err.c_str());
        stats[8 + 2 * t] = nnzC;
        const i64 limit = (i64)(p->ilut_max_fill * (double)nnzA);
        if (nnzC > limit)
            FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_ilut: step %d has %lld candidate positions, more than max_fill * nnz(A) = %lld (nnz(A) = %lld)", t,
                 (long long)nnzC, (long long)limit, (long long)nnzA);
        if (nnzC >= 0xFFFFFFF0ll) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_ilut: %lld candidate positions (the index holds 32-bit positions)", (long long)nnzC);
        // F and apos carried to C, its diagonal, tiers and row-wise index; s sweeps
        CK(ensure(h, cand.apos, sizeof(u32) * (size_t)std::max<i64>(nnzC, 1)));
        CK(ensure(h, cand.dpos, sizeof(u32) * (size_t)std::max<i64>(n, 1)));
        if (n > 0) {
            hipLaunchKernelGGL(ilut_carry_k, dim3(grid_for(n, WAVE_COLS)), dim3(GROUP), 0, s, (const i64 *)cand.hd->colptr.p, (const i64 *)cand.hd->rowval.p, n,
                               csc_of(cur.hd), csc_of(h), (double *)cand.hd->nzval.p, (u32 *)cand.apos.p);
            hipLaunchKernelGGL(ilut_diag_k, dim3(grid_for(n, 256)), dim3(256), 0, s, csc_of(cand.hd), n, (u32 *)cand.dpos.p, st + 2);
        }
        HIPCK(h, hipGetLastError());
        CK(work_ready(p, cand, st));
        CK(run_sweeps(p, cand, sweeps));
        // the drop: counts, scan, compaction into the state
        CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
        hipLaunchKernelGGL(ilut_drop_count_k, dim3(grid_for(n + 1, 256)), dim3(256), 0, s, (const i64 *)cand.hd->colptr.p, (const i64 *)cand.hd->rowval.p,
                           (const double *)cand.hd->nzval.p, (const u32 *)cand.dpos.p, n, tau, (i64 *)cp.p);
        CK(scan_inplace<i64, false>(h, (i64 *)cp.p, n + 1, ws, &l));
        i64 nnzS = 0;
        CK(read_i64(h, (const i64 *)cp.p + n, &nnzS));
        stats[9 + 2 * t] = nnzS;
        CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(nnzS, 1)));
        CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nnzS, 1)));
        CK(ensure(h, cur.apos, sizeof(u32) * (size_t)std::max<i64>(nnzS, 1)));
        if (n > 0)
            hipLaunchKernelGGL(ilut_compact_k, dim3(grid_for(n, 256)), dim3(256), 0, s, (const i64 *)cand.hd->colptr.p, (const i64 *)cand.hd->rowval.p,
                               (const double *)cand.hd->nzval.p, (const u32 *)cand.dpos.p, (const u32 *)cand.apos.p, n, tau, (const i64 *)cp.p,
                               (i64 *)rv.p, (double *)nz.p, (u32 *)cur.apos.p, (u32 *)cur.dpos.p);
        add_one_launch(s, (i64 *)cp.p, n + 1);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipStreamSynchronize(s));
        install(cur.hd, cp, rv, nz, nnzS);
        CK(work_ready(p, cur, st));
        CK(run_sweeps(p, cur, sweeps));
        run += 2 * (i64)sweeps;
    }
    HIPCK(h, hipStreamSynchronize(s));
    // the state goes into B's handle with its row-wise index (ILUAM's split build finds it current); the work handle takes what B held
    esp_handle *w = cur.hd;
    const i64 nnzS = w->nnz, old_nnz = bh->nnz;
    const bool old_valid = bh->csc_valid;
    install(bh, w->colptr, w->rowval, w->nzval, nnzS);
    std::swap(bh->csr_rowptr, w->csr_rowptr);
    std::swap(bh->csr_perm, w->csr_perm);
    std::swap(bh->csr_col, w->csr_col);
    bh->csr_version = bh->pattern_version;
    bh->csr_val_version = 0;
    drop_kept(w);
    w->nnz = old_valid ? old_nnz : 0;
    w->csc_valid = old_valid;
    w->pattern_version++, w->values_version++;
    std::swap(p->ilut_alt, cur.alt);
    std::swap(p->ilut_apos, cur.apos);
    std::swap(p->ilut_dpos, cur.dpos);
    std::swap(p->ilut_list, cur.list);
    p->ilut_tiers[0] = cur.tiers[0];
    p->ilut_tiers[1] = cur.tiers[1];
    stats[0] = steps;
    stats[1] = run;
    stats[2] = n - cur.tiers[0] - cur.tiers[1];
    stats[3] = cur.tiers[0];
    stats[4] = cur.tiers[1];
    stats[5] = nnzS;
    memcpy(p->ilut_stats, stats, sizeof stats);
    return ESP_OK;
}

}  // namespace

// update! with A's pattern kept and keep_pattern set (derived_update's values-only branch): s sweeps on the kept S from the current
// F and A's new values -- no index structure is touched
int32_t ilut_warm(esp_precon *p) {
    esp_handle *bh = p->der.bh;
    CK(run_sweeps(p, bh, p->ilut_alt, p->ilut_apos, p->ilut_dpos, p->ilut_list, p->ilut_tiers, p->ilut_sweeps));
    p->ilut_stats[1] = p->ilut_sweeps;
    return ESP_OK;
}

int32_t ilut_update(esp_precon *p) {
    if (!p->ilut_keep) p->der.rebuild = true;  // S depends on the values: the whole construction
    return derived_update(p, "esp_precon_ilut", build_f, "");
}

void ilut_release(esp_precon *p) {
    for (esp_handle *&q : p->ilut_h) {
        if (q) (void)esp_destroy(q);
        q = nullptr;
    }
    for (DevBuf *b : {&p->ilut_alt, &p->ilut_apos, &p->ilut_dpos, &p->ilut_list}) release(*b);
}

extern "C" int32_t esp_precon_ilut_create(esp_handle *h, double droptol, int32_t steps, int32_t sweeps, double max_fill, int32_t keep_pattern,
                                          esp_precon **out) {
    if (!h || !out) return ESP_ERR_INVALID;
    *out = nullptr;
    if (!(droptol >= 0.0)) FAIL(h, ESP_ERR_INVALID, "esp_precon_ilut_create: droptol = %g (>= 0)", droptol);
    if (steps < 0 || steps > ESP_ILUT_STEPS_MAX) FAIL(h, ESP_ERR_INVALID, "esp_precon_ilut_create: steps = %d (0 .. %d)", steps, ESP_ILUT_STEPS_MAX);
    if (sweeps < 1) FAIL(h, ESP_ERR_INVALID, "esp_precon_ilut_create: sweeps = %d (>= 1)", sweeps);
    if (!(max_fill >= 1.0)) FAIL(h, ESP_ERR_INVALID, "esp_precon_ilut_create: max_fill = %g (>= 1)", max_fill);
    CK(precon_check_handle(h, "esp_precon_ilut_create"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_ilut_create: a column window / column shard");
    esp_precon *p = precon_new(h, ESP_PRECON_ILUT);
    p->der.inner_kind = ESP_PRECON_ILUAM;
    p->ilut_tau = droptol;
    p->ilut_steps = steps;
    p->ilut_sweeps = sweeps;
    p->ilut_max_fill = max_fill;
    p->ilut_keep = keep_pattern != 0;
    const int32_t st = [&]() -> int32_t {
        esp_handle **hs[5] = {&p->der.bh, &p->ilut_h[0], &p->ilut_h[1], &p->ilut_h[2], &p->ilut_h[3]};
        for (esp_handle **q : hs) {
            const int32_t cs = esp_create(h->n, h->n, h->device, 0, q);
            if (cs != ESP_OK) FAIL(h, cs, "esp_precon_ilut_create: an internal handle: %s", esp_last_error(nullptr));
        }
        p->der.inner = precon_new(p->der.bh, ESP_PRECON_ILUAM);  // (its first update! analyses F's pattern)
        p->der.inner->prefactored = true;
        return ilut_update(p);
    }();
    return precon_finish(p, st, out);
}

extern "C" int32_t esp_precon_ilut_matrix(esp_precon *p, esp_handle **f) {
    if (!p || p->kind != ESP_PRECON_ILUT) return ESP_ERR_INVALID;
    if (f) *f = p->der.bh;
    return ESP_OK;
}

extern "C" int32_t esp_precon_ilut_stats(esp_precon *p, int64_t out[ESP_ILUT_STATS]) {
    if (!p || p->kind != ESP_PRECON_ILUT || !out) return ESP_ERR_INVALID;
    for (int k = 0; k < ESP_ILUT_STATS; k++) out[k] = p->ilut_stats[k];
    return ESP_OK;
}

extern "C" int32_t esp_precon_ilut_limits(int64_t out[4]) {
    if (!out) return ESP_ERR_INVALID;
    out[0] = ESP_ILUT_WAVE_UPPER;
    out[1] = ESP_ILUT_GROUP_UPPER;
    out[2] = ESP_ILUT_STEPS_MAX;
    out[3] = ESP_ILUT_STATS;
    return ESP_OK;
}
