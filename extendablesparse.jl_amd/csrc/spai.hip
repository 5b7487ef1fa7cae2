// spai.hip -- libesparse_hip: SPAIPreconditioner, the sparse approximate inverses SPAI-0 and SPAI-1, on the device CSC (see
// internal.hpp for the map of the translation units)
//
// M ~ inv(A) minimises |I - A*M|_F over the pattern of A, one column at a time (include/esparse_hip.h states the eight steps,
// tests/spai_model.c restates them as plain loops; the device equals the model bit for bit).  Column k: J = its stored rows
// (q of them), I = the sorted union of the stored rows of the columns j in J (p of them), B = A[I, J] dense, B = Q R by modified
// Gram-Schmidt with every sum in the order `osum` (lane l adds the rows l, l + 64, ... in turn, then the tree 32, 16, .., 1 over
// the lanes), y = row k of Q, R m = y by back substitution.
//   spai_size_k   one source column per workgroup: the rows of its lists gathered into LDS, sorted (bitonic) and counted without
//                 repeats: p.  The wave form (64 lanes) takes every column whose lists hold at most ESP_SPAI_WAVE_DOUBLES rows
//                 together, the workgroup form (512 lanes) the listed ones up to SORT_MAX rows.  Thread 0 files the column: the
//                 wave tier (p q <= ESP_SPAI_WAVE_DOUBLES and q q <= ESP_SPAI_WAVE_DOUBLES), the workgroup tier's list, or refused
//                 (p q > ESP_SPAI_DENSE_MAX; the lists of a column hold at most p q rows, so more than SORT_MAX of them are refused
//                 unsorted, with a lower bound of p).  Nothing of the preconditioner has changed by then.
//   spai1_k       one column per workgroup, the same body for both tiers: I by the size pass's sort, B zeroed and gathered by
//                 bisection of every stored row against I, then the Gram-Schmidt steps.  B is column-major with the leading
//                 dimension p: lane l reads B[l + 64 i + c p], consecutive doubles, no bank conflict.  Wave tier: one wave, B, R
//                 and I in LDS (10.5 KiB: room for 15 single-wave workgroups per CU).  Workgroup tier: eight waves, B (96 KiB) and I (48 KiB)
//                 in LDS, R in the workgroup's slot of a device scratch (q q doubles; it stays in the L2); the waves take the
//                 independent columns d > c round-robin, each with the wave's own sum -- the bits of the wave tier.  The back
//                 substitution is one lane's chain (its order is fixed by step 7).
//   spai0_k       SPAI-0: a wave per column, four per workgroup.
// update! with the pattern kept runs spai1_k / spai0_k alone on the kept p, tiers and list -- bitwise what a fresh create gives.
// ldiv! (order 1) is esp_mul's row gather over M's handle; order 0 is Jacobi's kernel on the n values.
#include "internal.hpp"

namespace {

constexpr int WAVE_T = 64, WIDE_T = 512;
constexpr int WCAP = ESP_SPAI_WAVE_DOUBLES, DCAP = ESP_SPAI_DENSE_MAX;
constexpr int SORT_MAX = 16384;        // rows the workgroup form of the size pass sorts
constexpr int WAVE_Q = 32;             // the wave tier's y / m: q q <= WCAP
constexpr u32 NOROW = 0xFFFFFFFFu;     // (n < 2^32 - 16: no row) pads the sort
constexpr unsigned GRID_MAX = 1u << 20;  // workgroups of a grid-stride launch
enum : uint8_t { TIER_WAVE = 0, TIER_WIDE = 1, TIER_REFUSED = 2, TIER_REFUSED_BOUND = 3 };
// the status words of an update (esp_precon::spai_stat)
enum { ST_NSORT = 0, ST_NWIDE = 1, ST_BAD = 2, ST_MAXP = 3, ST_MAXQ = 4, ST_MAXPQ = 5, ST_WIDEQ = 6, ST_ERR = 7 };
static_assert(WCAP % 64 == 0 && WAVE_Q * WAVE_Q >= WCAP, "the wave tier's q");
static_assert(2 * DCAP >= SORT_MAX && SORT_MAX >= DCAP, "the workgroup tier sorts its rows in B's LDS: at most p q <= DCAP of them");
static_assert((size_t)DCAP * 12 + (WIDE_T + 1) * 4 + 64 <= 160 * 1024, "B and I of the workgroup tier: the LDS of one CU");

__device__ __forceinline__ int pow2_at_least(int x) {
    int v = 1;
    while (v < x) v <<= 1;
    return v;
}

// the tree of osum over the 64 partial sums of a wave; the result in lane 0 (and, through the shuffle, in every lane)
__device__ __forceinline__ double osum_tree(double a) {
    for (int s = 32; s > 0; s >>= 1) a = a + __shfl_down(a, s, 64);
    return __shfl(a, 0, 64);
}

// I (p entries; I == nullptr: the count alone) = the sorted union of the stored rows of the columns j in J = column k's rows.
// tc = the rows of those lists together; cand: LDS for pow2_at_least(tc) <= ccap words; cnt: LDS, T + 1 words.  Every thread
// of the workgroup calls it and gets p; icap bounds the writes to I.
template <int T>
__device__ int union_rows(const i64 *__restrict__ cp, const i64 *__restrict__ rv, i64 ks, int q, int tc, u32 *cand, int ccap, int *cnt,
                          u32 *I, int icap) {
    const int tid = threadIdx.x;
    const int npad = pow2_at_least(tc < 1 ? 1 : tc);
    if (npad > ccap) return -1;
    int off = 0;
    for (int c = 0; c < q; c++) {
        const i64 j = rv[ks + c] - 1;
        const i64 s = cp[j] - 1, e = cp[j + 1] - 1;
        for (i64 x = s + tid; x < e; x += T) {
            const i64 at = (i64)off + (x - s);
            if (at < npad) cand[at] = (u32)(rv[x] - 1);
        }
        off += (int)(e - s);
    }
    for (int i = tc + tid; i < npad; i += T) cand[i] = NOROW;
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < npad; i += T) {
                const int x = i ^ j;
                if (x > i) {
                    const u32 a = cand[i], b = cand[x];
                    if ((a > b) == ((i & k) == 0)) {
                        cand[i] = b;
                        cand[x] = a;
                    }
                }
            }
            __syncthreads();
        }
    // the first of every run of equal rows, counted per thread over a slice, the slices' offsets by one lane
    const int chunk = (npad + T - 1) / T;
    const int lo = tid * chunk, hi = min(lo + chunk, tc);
    int mine = 0;
    for (int i = lo; i < hi; i++) mine += (i == 0 || cand[i] != cand[i - 1]) ? 1 : 0;
    cnt[tid] = mine;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < T; t++) {
            const int v = cnt[t];
            cnt[t] = run;
            run += v;
        }
        cnt[T] = run;
    }
    __syncthreads();
    if (I) {
        int at = cnt[tid];
        for (int i = lo; i < hi; i++)
            if (i == 0 || cand[i] != cand[i - 1]) {
                if (at < icap) I[at] = cand[i];
                at++;
            }
    }
    const int p = cnt[T];
    __syncthreads();
    return p;
}

// q, the rows of the lists together and the longest list of column k, in every thread (red: LDS, 2 words)
template <int T>
__device__ void list_sizes(const i64 *__restrict__ cp, const i64 *__restrict__ rv, i64 ks, i64 q, unsigned long long *red,
                           unsigned long long *tc_out, unsigned long long *maxlen_out) {
    if (threadIdx.x == 0) red[0] = red[1] = 0ull;
    __syncthreads();
    unsigned long long tc = 0, ml = 0;
    for (i64 c = threadIdx.x; c < q; c += T) {
        const i64 j = rv[ks + c] - 1;
        const unsigned long long len = (unsigned long long)(cp[j + 1] - cp[j]);
        tc += len;
        ml = len > ml ? len : ml;
    }
    if (tc) atomicAdd(&red[0], tc);
    if (ml) atomicMax(&red[1], ml);
    __syncthreads();
    *tc_out = red[0];
    *maxlen_out = red[1];
    __syncthreads();
}

__device__ __forceinline__ void stat_max(unsigned long long *w, unsigned long long v) {
    if (v > *(volatile unsigned long long *)w) atomicMax(w, v);
}

// the size pass.  sources == nullptr: every column (the wave form); else the listed ones (the workgroup form)
template <int T, int SCAP>
__global__ __launch_bounds__(T) void spai_size_k(espfold::Csc A, i64 n, const u32 *__restrict__ sources, i64 nsrc, u32 *__restrict__ pcol,
                                                 uint8_t *__restrict__ tier, u32 *__restrict__ sortlist, u32 *__restrict__ widelist,
                                                 unsigned long long *__restrict__ st) {
    __shared__ u32 cand[SCAP];
    __shared__ int cnt[T + 1];
    __shared__ unsigned long long red[2];
    const i64 count = sources ? nsrc : n;
    for (i64 it = blockIdx.x; it < count; it += gridDim.x) {
        const i64 k = sources ? (i64)sources[it] : it;
        const i64 ks = A.colptr[k] - 1, q = A.colptr[k + 1] - 1 - ks;
        if (q == 0) {  // an empty column stays empty
            if (threadIdx.x == 0) {
                pcol[k] = 0u;
                tier[k] = TIER_WAVE;
            }
            continue;
        }
        unsigned long long tc, maxlen;
        list_sizes<T>(A.colptr, A.rowval, ks, q, red, &tc, &maxlen);
        if (tc > (unsigned long long)SCAP) {
            if (threadIdx.x == 0) {
                if (!sources && tc <= (unsigned long long)SORT_MAX) {
                    sortlist[atomicAdd(&st[ST_NSORT], 1ull)] = (u32)k;
                } else {  // p q >= tc > SORT_MAX >= DCAP
                    const unsigned long long lb = max(maxlen, (tc + (unsigned long long)q - 1) / (unsigned long long)q);
                    pcol[k] = (u32)min(lb, 0xFFFFFFFFull);
                    tier[k] = TIER_REFUSED_BOUND;
                    atomicMin(&st[ST_BAD], (unsigned long long)k);
                }
            }
            continue;
        }
        const int p = union_rows<T>(A.colptr, A.rowval, ks, (int)q, (int)tc, cand, SCAP, cnt, nullptr, 0);
        if (threadIdx.x == 0) {
            const unsigned long long pq = (unsigned long long)p * (unsigned long long)q;
            pcol[k] = (u32)p;
            if (p < 0) {
                atomicMax(&st[ST_ERR], 1ull);
            } else if (pq > (unsigned long long)DCAP) {
                tier[k] = TIER_REFUSED;
                atomicMin(&st[ST_BAD], (unsigned long long)k);
            } else {
                if (pq <= (unsigned long long)WCAP && (unsigned long long)q * (unsigned long long)q <= (unsigned long long)WCAP) {
                    tier[k] = TIER_WAVE;
                } else {
                    tier[k] = TIER_WIDE;
                    widelist[atomicAdd(&st[ST_NWIDE], 1ull)] = (u32)k;
                    stat_max(&st[ST_WIDEQ], (unsigned long long)q);
                }
                stat_max(&st[ST_MAXP], (unsigned long long)p);
                stat_max(&st[ST_MAXQ], (unsigned long long)q);
                stat_max(&st[ST_MAXPQ], pq);
            }
        }
    }
}

// column k of M.  list == nullptr: every column of the wave tier (BCAP = WCAP, one wave); else the listed columns of the workgroup
// tier (BCAP = DCAP, R in the workgroup's slot Rg + blockIdx.x * rslot)
template <int T, int BCAP, bool WIDE>
__global__ __launch_bounds__(T) void spai1_k(espfold::Csc A, i64 n, const u32 *__restrict__ pcol, const uint8_t *__restrict__ tier,
                                             const u32 *__restrict__ list, i64 nlist, double *__restrict__ Rg, i64 rslot,
                                             double *__restrict__ out, unsigned long long *__restrict__ st) {
    constexpr int NW = T / 64;
    __shared__ double B[BCAP];
    __shared__ u32 I[BCAP];
    __shared__ double Rl[WIDE ? 1 : BCAP];
    __shared__ double s_ym[WIDE ? 1 : WAVE_Q];
    __shared__ int cnt[T + 1];
    __shared__ unsigned long long red[2];
    __shared__ double s_rcc;
    __shared__ int s_pos;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const i64 count = WIDE ? nlist : n;
    for (i64 it = blockIdx.x; it < count; it += gridDim.x) {
        const i64 k = WIDE ? (i64)list[it] : it;
        if (!WIDE && tier[k] != TIER_WAVE) continue;
        const i64 ks = A.colptr[k] - 1;
        const int q = (int)(A.colptr[k + 1] - 1 - ks);
        if (q == 0) continue;
        const int p = (int)pcol[k];
        unsigned long long tc, maxlen;
        list_sizes<T>(A.colptr, A.rowval, ks, q, red, &tc, &maxlen);
        // (what the size pass filed: anything else means the pattern is not the one it saw)
        const bool fits = (i64)p * q <= BCAP && tc <= (unsigned long long)BCAP &&
                          (WIDE ? (i64)q * q <= rslot : ((i64)q * q <= BCAP && q <= WAVE_Q));
        if (!fits) {
            if (tid == 0) atomicMax(&st[ST_ERR], 1ull);
            continue;
        }
        double *R = WIDE ? Rg + (i64)blockIdx.x * rslot : Rl;
        double *ym = WIDE ? out + ks : s_ym;
        const int pp = union_rows<T>(A.colptr, A.rowval, ks, q, (int)tc, (u32 *)B, 2 * BCAP, cnt, I, BCAP);
        if (pp != p) {
            if (tid == 0) atomicMax(&st[ST_ERR], 1ull);
            continue;
        }
        if (tid == 0) {  // 6: where is row k?
            int lo = 0, hi = p;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (I[mid] < (u32)k) lo = mid + 1;
                else hi = mid;
            }
            s_pos = lo < p && I[lo] == (u32)k ? lo : -1;
        }
        for (int i = tid; i < p * q; i += T) B[i] = 0.0;  // 3
        __syncthreads();
        for (int c = 0; c < q; c++) {
            const i64 j = A.rowval[ks + c] - 1;
            const i64 e = A.colptr[j + 1] - 1;
            for (i64 x = A.colptr[j] - 1 + tid; x < e; x += T) {
                const u32 r = (u32)(A.rowval[x] - 1);
                int lo = 0, hi = p - 1;  // (r is in I)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (I[mid] < r) lo = mid + 1;
                    else hi = mid;
                }
                B[lo + c * p] = A.nzval[x];
            }
        }
        __syncthreads();
        for (int c = 0; c < q; c++) {  // 5
            double *bc = B + c * p;
            if (wv == 0) {
                double a = 0.0;
                if (lane < p) {
                    a = bc[lane] * bc[lane];
                    for (int r = lane + 64; r < p; r += 64) a = a + bc[r] * bc[r];
                }
                a = osum_tree(a);
                if (lane == 0) {
                    const double rcc = sqrt(a);
                    s_rcc = rcc;
                    R[(i64)c * q + c] = rcc;
                }
            }
            __syncthreads();
            const double rcc = s_rcc;
            for (int r = tid; r < p; r += T) bc[r] = bc[r] / rcc;
            __syncthreads();
            for (int d = c + 1 + wv; d < q; d += NW) {
                double *bd = B + d * p;
                double a = 0.0;
                if (lane < p) {
                    a = bc[lane] * bd[lane];
                    for (int r = lane + 64; r < p; r += 64) a = a + bc[r] * bd[r];
                }
                const double dot = osum_tree(a);
                if (lane == 0) R[(i64)c * q + d] = dot;
                for (int r = lane; r < p; r += 64) bd[r] = bd[r] - dot * bc[r];
            }
            __syncthreads();
        }
        const int pos = s_pos;
        for (int c = tid; c < q; c += T) ym[c] = pos >= 0 ? B[pos + c * p] : 0.0;
        __syncthreads();
        if (tid == 0) {  // 7
            for (int c = q - 1; c >= 0; c--) {
                double t = ym[c];
                for (int d = c + 1; d < q; d++) t = t - R[(i64)c * q + d] * ym[d];
                ym[c] = t / R[(i64)c * q + c];
            }
        }
        __syncthreads();
        if (!WIDE)
            for (int c = tid; c < q; c += T) out[ks + c] = ym[c];  // 8
        __syncthreads();
    }
}

// SPAI-0: m_k = a_kk / osum(a*a over column k), a wave per column
__global__ __launch_bounds__(256) void spai0_k(espfold::Csc A, i64 n, double *__restrict__ d) {
    const int lane = threadIdx.x & 63;
    const i64 k = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= n) return;
    const i64 s = A.colptr[k] - 1, q = A.colptr[k + 1] - 1 - s;
    double a = 0.0, mine = 0.0;
    bool has = false;
    for (i64 r = lane; r < q; r += 64) {
        const double v = A.nzval[s + r];
        a = r == lane ? v * v : a + v * v;
        if (A.rowval[s + r] - 1 == k) {
            mine = v;
            has = true;
        }
    }
    a = osum_tree(a);
    const unsigned long long mask = __ballot(has);
    const double akk = mask ? __shfl(mine, __ffsll((long long)mask) - 1, 64) : 0.0;
    if (lane == 0) d[k] = akk / a;
}

__global__ void fill_f64_k(double *p, i64 n, double v) {
    const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) p[g] = v;
}
__global__ void sub_k(double *__restrict__ u, const double *__restrict__ x, i64 n) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) u[i] = u[i] - x[i];
}

unsigned grid_of(i64 count) { return (unsigned)std::max<i64>(1, std::min<i64>(count, (i64)GRID_MAX)); }

int32_t read_status(esp_handle *h, const unsigned long long *st) {
    HIPCK(h, hipGetLastError());
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, st, sizeof(u64) * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}

// the numeric kernels of order 1 over the filed columns: M's values into out
int32_t numeric(esp_precon *p, const u32 *pcol, const uint8_t *tier, const u32 *list, i64 nwide, double *Rg, i64 rslot, i64 rgrid,
                double *out) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    unsigned long long *st = (unsigned long long *)p->spai_stat.p;
    if (n == 0 || h->nnz == 0) return ESP_OK;
    const espfold::Csc A{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (double *)h->nzval.p, h->nnz};
    HIPCK(h, hipMemsetAsync(st + ST_ERR, 0, sizeof(u64), h->stream));
    hipLaunchKernelGGL((spai1_k<WAVE_T, WCAP, false>), dim3(grid_of(n)), dim3(WAVE_T), 0, h->stream, A, n, pcol, tier, (const u32 *)nullptr,
                       (i64)0, (double *)nullptr, (i64)0, out, st);
    if (nwide > 0)
        hipLaunchKernelGGL((spai1_k<WIDE_T, DCAP, true>), dim3((unsigned)rgrid), dim3(WIDE_T), 0, h->stream, A, n, pcol, tier, list, nwide, Rg,
                           rslot, out, st);
    CK(read_status(h, st));
    if (h->pin_scalar[ST_ERR] != 0) FAIL(h, ESP_ERR_HIP, "esp_precon_spai: a column is not what the size pass filed it as");
    return ESP_OK;
}

// after a pattern change: the size pass, the tiers, M's arrays; p changes only when everything succeeded
int32_t rebuild(esp_precon *p) {
    esp_handle *h = p->h, *rh = p->spai_rh;
    hipStream_t s = h->stream;
    const i64 n = p->n, nnz = h->nnz;
    Temps tmp;
    DevBuf &pcol = tmp.b[0], &tier = tmp.b[1], &wlist = tmp.b[2], &slist = tmp.b[3], &rbuf = tmp.b[4], &cp = tmp.b[6], &rv = tmp.b[7],
           &nz = tmp.b[8];
    const size_t n1 = (size_t)std::max<i64>(n, 1);
    CK(ensure(h, pcol, sizeof(u32) * n1));
    CK(ensure(h, tier, n1));
    CK(ensure(h, wlist, sizeof(u32) * n1));
    CK(ensure(h, slist, sizeof(u32) * n1));
    unsigned long long *st = (unsigned long long *)p->spai_stat.p;
    HIPCK(h, hipMemsetAsync(st, 0, sizeof(u64) * 8, s));
    HIPCK(h, hipMemsetAsync(pcol.p, 0, sizeof(u32) * n1, s));
    HIPCK(h, hipMemsetAsync(tier.p, 0, n1, s));
    hipLaunchKernelGGL(fill_i64_k, dim3(1), dim3(1), 0, s, (i64 *)st + ST_BAD, (i64)1, (i64)-1);
    const espfold::Csc A{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (double *)h->nzval.p, nnz};
    i64 stats[4] = {0, 0, 0, 0}, wideq = 0;
    if (n > 0 && nnz > 0) {
        hipLaunchKernelGGL((spai_size_k<WAVE_T, WCAP>), dim3(grid_of(n)), dim3(WAVE_T), 0, s, A, n, (const u32 *)nullptr, (i64)0, (u32 *)pcol.p,
                           (uint8_t *)tier.p, (u32 *)slist.p, (u32 *)wlist.p, st);
        CK(read_status(h, st));
        const i64 nsort = (i64)h->pin_scalar[ST_NSORT];
        if (nsort > 0) {
            hipLaunchKernelGGL((spai_size_k<WIDE_T, SORT_MAX>), dim3(grid_of(nsort)), dim3(WIDE_T), 0, s, A, n, (const u32 *)slist.p, nsort,
                               (u32 *)pcol.p, (uint8_t *)tier.p, (u32 *)nullptr, (u32 *)wlist.p, st);
            CK(read_status(h, st));
        }
        if (h->pin_scalar[ST_ERR] != 0) FAIL(h, ESP_ERR_HIP, "esp_precon_spai: the size pass overran its sort");
        const unsigned long long bad = h->pin_scalar[ST_BAD];
        stats[0] = (i64)h->pin_scalar[ST_MAXP];
        stats[1] = (i64)h->pin_scalar[ST_MAXQ];
        stats[2] = (i64)h->pin_scalar[ST_MAXPQ];
        stats[3] = (i64)h->pin_scalar[ST_NWIDE];
        wideq = (i64)h->pin_scalar[ST_WIDEQ];
        if (bad != ~0ull) {
            i64 c0 = 0, c1 = 0;
            CK(read_i64(h, (const i64 *)h->colptr.p + bad, &c0));
            CK(read_i64(h, (const i64 *)h->colptr.p + bad + 1, &c1));
            HIPCK(h, hipMemcpyAsync(h->pin_scalar, (const u32 *)pcol.p + bad, sizeof(u32), hipMemcpyDeviceToHost, s));
            HIPCK(h, hipMemcpyAsync(h->pin_scalar + 1, (const uint8_t *)tier.p + bad, 1, hipMemcpyDeviceToHost, s));
            HIPCK(h, hipStreamSynchronize(s));
            const unsigned pb = *(const u32 *)h->pin_scalar;
            const bool bound = *(const uint8_t *)(h->pin_scalar + 1) == TIER_REFUSED_BOUND;
            FAIL(h, ESP_ERR_UNSUPPORTED,
                 "esp_precon_spai: column %llu needs a dense problem of p %s %u rows by q = %lld unknowns, more than ESP_SPAI_DENSE_MAX = %d "
                 "doubles (the smallest such column)",
                 bad, bound ? ">=" : "=", pb, (long long)(c1 - c0), (int)DCAP);
        }
    }
    // the R slots of the workgroup tier: as many workgroups as 1 GiB of slots allows
    const i64 rslot = std::max<i64>(wideq * wideq, 1);
    const i64 rgrid = std::max<i64>(1, std::min<i64>(std::min<i64>(stats[3], 1024), ((i64)1 << 27) / rslot));
    if (stats[3] > 0) CK(ensure(h, rbuf, sizeof(double) * (size_t)(rslot * rgrid)));
    CK(ensure(h, cp, sizeof(i64) * (size_t)(n + 1)));
    CK(ensure(h, rv, sizeof(i64) * (size_t)std::max<i64>(nnz, 1)));
    CK(ensure(h, nz, sizeof(double) * (size_t)std::max<i64>(nnz, 1)));
    HIPCK(h, hipMemcpyAsync(cp.p, h->colptr.p, sizeof(i64) * (size_t)(n + 1), hipMemcpyDeviceToDevice, s));
    if (nnz > 0) HIPCK(h, hipMemcpyAsync(rv.p, h->rowval.p, sizeof(i64) * (size_t)nnz, hipMemcpyDeviceToDevice, s));
    CK(numeric(p, (const u32 *)pcol.p, (const uint8_t *)tier.p, (const u32 *)wlist.p, stats[3], (double *)rbuf.p, rslot, rgrid, (double *)nz.p));
    HIPCK(h, hipStreamSynchronize(s));
    install(rh, cp, rv, nz, nnz);
    std::swap(p->spai_p, pcol);
    std::swap(p->spai_tier, tier);
    std::swap(p->spai_list, wlist);
    std::swap(p->spai_r, rbuf);
    p->spai_rslot = rslot;
    p->spai_rgrid = rgrid;
    for (int k = 0; k < 4; k++) p->spai_stats[k] = stats[k];
    return ESP_OK;
}

// an internal handle's call failed: its message under the preconditioner's name
#define SUBCALL(h, q, call)                                                       \
    do {                                                                          \
        const int32_t _st = (call);                                               \
        if (_st != ESP_OK) FAIL(h, _st, "esp_precon_spai: %s", (q)->err.c_str()); \
    } while (0)

}  // namespace

int32_t spai_follow_stream(esp_precon *p) {
    for (esp_handle *q : {p->spai_rh, p->spai_th, p->spai_sh})
        if (q && q->stream != p->h->stream) CK(esp_set_stream(q, (void *)p->h->stream));
    return ESP_OK;
}

// The order of the statements is derived_update's guarantee: everything that can refuse (the size pass, the buffers) comes before
// anything of p changes; once M's values are being written pattern_version = 0 matches no pattern, and the stamps come last.
int32_t spai_update(esp_precon *p) {
    esp_handle *h = p->h;
    CK(precon_check_handle(h, "esp_precon_update"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_spai: a column window / column shard");
    CK(spai_follow_stream(p));
    hipStream_t s = h->stream;
    const i64 n = p->n;
    const size_t n1 = (size_t)std::max<i64>(n, 1);
    const bool stale = p->pattern_version != h->pattern_version || p->nnz != h->nnz;
    if (p->spai_order == 0) {
        CK(ensure(h, p->diag, sizeof(double) * n1));
        p->pattern_version = 0;
        const espfold::Csc A{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (double *)h->nzval.p, h->nnz};
        if (n > 0) hipLaunchKernelGGL(spai0_k, dim3(grid_for(n, 4)), dim3(256), 0, s, A, n, (double *)p->diag.p);
        HIPCK(h, hipGetLastError());
    } else {
        CK(ensure(h, p->spai_stat, sizeof(u64) * 8));
        CK(ensure(h, p->u1, sizeof(double) * n1));
        if (p->spai_sym && !p->spai_half.p) {
            CK(ensure(h, p->spai_half, sizeof(double) * n1));
            hipLaunchKernelGGL(fill_f64_k, dim3(grid_for(n, 256)), dim3(256), 0, s, (double *)p->spai_half.p, n, 0.5);
        }
        esp_handle *rh = p->spai_rh;
        if (stale) {
            CK(rebuild(p));
            p->pattern_version = 0;
        } else {
            p->pattern_version = 0;
            CK(numeric(p, (const u32 *)p->spai_p.p, (const uint8_t *)p->spai_tier.p, (const u32 *)p->spai_list.p, p->spai_stats[3],
                       (double *)p->spai_r.p, p->spai_rslot, p->spai_rgrid, (double *)rh->nzval.p));
            rh->values_version++;
        }
        if (p->spai_sym) {  // 0.5*(M + transpose(M))
            esp_handle *th = p->spai_th, *sh = p->spai_sh;
            SUBCALL(h, th, esp_transpose(rh, th, nullptr));
            SUBCALL(h, sh, esp_add(rh, th, ESP_OP_ADD, sh, nullptr));
            SUBCALL(h, sh, esp_diag_scale(sh, (const double *)p->spai_half.p, 0, 1, sh));
        }
        esp_handle *mh = spai_applied(p);
        SUBCALL(h, mh, csr_current(mh));  // the row-wise index ldiv! streams: nothing is built inside a solve
    }
    HIPCK(h, hipStreamSynchronize(s));
    p->nnz = h->nnz;
    p->pattern_version = h->pattern_version;
    p->values_version = h->values_version;
    return ESP_OK;
}

int32_t spai_apply(esp_precon *p, const double *v, double *u, bool sub) {
    esp_handle *h = p->h, *mh = spai_applied(p);
    const i64 n = p->n;
    if (n == 0) return ESP_OK;
    const bool via = sub || u == v;
    double *dst = via ? (double *)p->u1.p : u;
    mul_rows_launch(mh, v, dst);
    if (sub) hipLaunchKernelGGL(sub_k, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, u, (const double *)dst, n);
    else if (via) HIPCK(h, hipMemcpyAsync(u, dst, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    return ESP_OK;
}

void spai_release(esp_precon *p) {
    for (esp_handle **q : {&p->spai_rh, &p->spai_th, &p->spai_sh}) {
        if (*q) (void)esp_destroy(*q);
        *q = nullptr;
    }
    for (DevBuf *b : {&p->spai_p, &p->spai_tier, &p->spai_list, &p->spai_r, &p->spai_half, &p->spai_stat}) release(*b);
}

extern "C" int32_t esp_precon_spai_create(esp_handle *h, int32_t order, int32_t symmetric, esp_precon **out) {
    if (!h || !out) return ESP_ERR_INVALID;
    *out = nullptr;
    if (order != 0 && order != 1) FAIL(h, ESP_ERR_INVALID, "esp_precon_spai_create: order = %d (0: SPAI-0, 1: SPAI-1)", order);
    if (symmetric && order == 0) FAIL(h, ESP_ERR_INVALID, "esp_precon_spai_create: SPAI-0 is diagonal: symmetric belongs to order 1");
    CK(precon_check_handle(h, "esp_precon_spai_create"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "esp_precon_spai_create: a column window / column shard");
    esp_precon *p = precon_new(h, ESP_PRECON_SPAI);
    p->spai_order = order;
    p->spai_sym = symmetric ? 1 : 0;
    const int32_t st = [&]() -> int32_t {
        if (order == 1)
            for (esp_handle **q : {&p->spai_rh, &p->spai_th, &p->spai_sh}) {
                if (!symmetric && q != &p->spai_rh) continue;
                const int32_t cs = esp_create(h->n, h->n, h->device, 0, q);
                if (cs != ESP_OK) FAIL(h, cs == ESP_ERR_HIP ? ESP_ERR_NOMEM : cs, "esp_precon_spai_create: an internal handle: %s", esp_last_error(nullptr));
            }
        return spai_update(p);
    }();
    return precon_finish(p, st, out);
}

extern "C" int32_t esp_precon_spai_matrix(esp_precon *p, esp_handle **m) {
    if (!p || p->kind != ESP_PRECON_SPAI || p->spai_order == 0) return ESP_ERR_INVALID;
    if (m) *m = spai_applied(p);
    return ESP_OK;
}

extern "C" int32_t esp_precon_spai_stats(esp_precon *p, int64_t out[4]) {
    if (!p || p->kind != ESP_PRECON_SPAI || !out) return ESP_ERR_INVALID;
    for (int k = 0; k < 4; k++) out[k] = p->spai_stats[k];
    return ESP_OK;
}
