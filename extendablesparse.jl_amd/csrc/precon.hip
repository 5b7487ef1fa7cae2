// precon.hip -- libesparse_hip: the point preconditioners' update! / ldiv! and the simple! iteration on the device CSC
// (ILUAM's analysis, factorization and solves: iluam.hip; its create / update! / ldiv! / simple! enter here)
// (see internal.hpp for the map of the translation units)
//
// ldiv! of ILU0 (factorizations/ilu0.jl:66-92) reads like two triangular sweeps, but neither carries a dependency chain:
//   1. u[j] = xdiag[j]*v[j] for every j (call it u0);
//   2. for j = n:-1:1, the entries of column j BELOW the diagonal (rows i > j): u[i] -= xdiag[i]*nzval[k]*u[j].  Row j is
//      written only while a column j' < j is processed, and in the descending loop those come AFTER column j: every read
//      u[j] sees u0[j].  So u1[i] = u0[i] - sum over the stored j < i of (xdiag[i]*a_ij)*u0[j], subtracted in DECREASING j;
//   3. for j = 1:n, the entries ABOVE the diagonal (rows i < j): the same argument with the loop ascending gives
//      u[i] = u1[i] - sum over the stored j > i of (xdiag[i]*a_ij)*u1[j], subtracted in INCREASING j.
// Every row is an independent, ordered gather: two grid-wide passes reproduce the reference loop bit for bit, with no level
// scheduling and no atomics (tests/precon_model.c restates the literal column loops; the GPU tests compare bitwise).  Julia's
// `xdiag[i] * nzval[k] * u[j]` is `(xdiag[i]*nzval[k])*u[j]`, so the pass kernels stream PRE-SCALED values xdiag[i]*a_ij:
// the same single multiplication the reference performs first.
//
// The split layout, built at update! after a pattern change from the row-wise index of esp_mul (build_csr): the strictly
// lower part of every row in decreasing column order, the strictly upper part in increasing column order, each with its own
// row pointers, 4-byte columns, 4-byte CSC positions (to re-gather values) and the pre-scaled 8-byte values.
// The reference's preconditioner holds A.cscmatrix by reference: after an in-place value change without update! its ldiv!
// uses the CURRENT off-diagonal nzval with the OLD xdiag.  So when values_version moved since the scaled copy was made, it is
// re-gathered with the STORED xdiag (ldiv!) or with the new one (update!).
#include "internal.hpp"

namespace {

constexpr int PT = 256;       // threads = rows per workgroup of the row kernels
constexpr int PCAP = 2048;    // part entries a workgroup stages in LDS (24 KiB); a bigger slice reads from global memory

// ---- build of the split layout (pattern changed) -------------------------------------------------------------------
// rp = csr_rowptr + 1: the entries of row i are [rp[i], rp[i+1]) of csr_col / csr_perm, columns ascending
__global__ void split_count_k(const u64 *__restrict__ rp, const u32 *__restrict__ tcol, const u32 *__restrict__ perm, i64 n,
                              u32 *__restrict__ lcnt, u32 *__restrict__ ucnt, u32 *__restrict__ dpos) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 b = rp[i], e = rp[i + 1];
    u32 nl = 0, nd = 0;
    for (u64 k = b; k < e; k++) {
        const u32 c = tcol[k];
        nl += c < (u64)i ? 1u : 0u;
        nd += c == (u64)i ? 1u : 0u;
    }
    lcnt[i] = nl;
    ucnt[i] = (u32)(e - b) - nl - nd;
    dpos[i] = nd ? perm[b + nl] : 0u;  // (ILU0 / ILUAM refused a missing diagonal before the build)
}
__global__ void split_fill_k(const u64 *__restrict__ rp, const u32 *__restrict__ tcol, const u32 *__restrict__ perm, i64 n,
                             const u32 *__restrict__ lptr, const u32 *__restrict__ uptr, u32 *__restrict__ lcol,
                             u32 *__restrict__ lpos, u32 *__restrict__ ucol, u32 *__restrict__ upos, bool reversed) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 b = rp[i], e = rp[i + 1];
    const u32 nl = lptr[i + 1] - lptr[i], nu = uptr[i + 1] - uptr[i];
    // reversed (ILUAM): the forward substitution runs j = 1:n, the backward one j = n:-1:1 (ilu_Al-Kurdi_Mittal.jl:133-155)
    for (u32 t = 0; t < nl; t++) {  // lower part: decreasing column (ilu0.jl:78-83 runs j = n:-1:1)
        const u64 k = reversed ? b + t : b + nl - 1 - t;
        lcol[lptr[i] + t] = tcol[k];
        lpos[lptr[i] + t] = perm[k];
    }
    for (u32 t = 0; t < nu; t++) {  // upper part: increasing column (ilu0.jl:85-90 runs j = 1:n)
        const u64 k = reversed ? e - 1 - t : e - nu + t;
        ucol[uptr[i] + t] = tcol[k];
        upos[uptr[i] + t] = perm[k];
    }
}
// invdiag[j] = one(Tv) / A[j,j] (jacobi.jl:5-12; getindex of a position that is not stored gives zero: Inf) and
// xdiag[j] = 1/nzval[idiag[j]] (what ilu0.jl:8-41 leaves, see diag_setup_k in consumers.hip); missing = smallest 1-based
// column without a stored diagonal
__global__ void precon_diag_k(espfold::Csc c, i64 n, double *__restrict__ inv, unsigned long long *__restrict__ missing) {
    const i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const i64 pos = c.nnz > 0 ? espfold::csc_find(c, j, j) : -1;
    if (pos < 0) atomicMin(missing, (unsigned long long)(j + 1));
    inv[j] = 1.0 / (pos >= 0 ? c.nzval[pos] : 0.0);
}
// the pre-scaled values xdiag[i]*nzval[k] of both parts.  A workgroup owns PT rows: their xdiag and part pointers go to LDS,
// then the lanes walk the slice of each part entry by entry (coalesced positions and values; the row of an entry by binary
// search in LDS).  FRESH (update! with the pattern kept: ilu0!): xdiag[i] = 1/nzval[dpos[i]] is formed (and stored) here.
__device__ __forceinline__ void scale_part(const u32 *sp, int nr, const double *sx, const u32 *__restrict__ pos,
                                           const double *__restrict__ nzval, double *__restrict__ val) {
    for (u32 k = sp[0] + threadIdx.x; k < sp[nr]; k += PT) {
        int lo = 0, hi = nr - 1;  // the last row r with sp[r] <= k
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (sp[mid] <= k) lo = mid;
            else hi = mid - 1;
        }
        val[k] = sx[lo] * nzval[pos[k]];
    }
}
template <bool FRESH>
__global__ __launch_bounds__(PT) void split_scale_k(const u32 *__restrict__ lptr, const u32 *__restrict__ lpos, const u32 *__restrict__ uptr,
                                                    const u32 *__restrict__ upos, const u32 *__restrict__ dpos, double *__restrict__ xdiag,
                                                    const double *__restrict__ nzval, i64 n, double *__restrict__ lval,
                                                    double *__restrict__ uval) {
    __shared__ double sx[PT];
    __shared__ u32 slp[PT + 1], sup[PT + 1];
    const i64 r0 = (i64)blockIdx.x * PT;
    const int nr = (int)(std::min<i64>(r0 + PT, n) - r0);
    const i64 i = r0 + threadIdx.x;
    if ((int)threadIdx.x < nr) {
        double x;
        if (FRESH) {
            x = 1.0 / nzval[dpos[i]];
            xdiag[i] = x;
        } else {
            x = xdiag[i];
        }
        sx[threadIdx.x] = x;
        slp[threadIdx.x] = lptr[i];
        sup[threadIdx.x] = uptr[i];
    }
    if (threadIdx.x == 0) {
        slp[nr] = lptr[r0 + nr];
        sup[nr] = uptr[r0 + nr];
    }
    __syncthreads();
    scale_part(slp, nr, sx, lpos, nzval, lval);
    scale_part(sup, nr, sx, upos, nzval, uval);
}

// ---- the row kernels: a workgroup owns PT consecutive rows, stages their slice of the part (columns, values) in LDS with
// coalesced loads, then every lane runs its row's ordered chain from LDS.  Modes:
enum RowMode {
    ILU_LOWER = 0,   // pass 1: dst[i] = u0[i] - sum_{j<i, decreasing} val*u0[j], u0[j] = xdiag[j]*src[j] formed on the fly
    ILU_UPPER = 1,   // pass 2 (ldiv!): dst[i] = src[i] - sum_{j>i, increasing} val*src[j]
    ILU_UPPER_SUB = 2,  // pass 2 fused into simple!'s `u .-= upd`: dst[i] = dst[i] - upd[i]
    RESIDUAL = 3     // simple!'s mul!(res, A, u); res .-= b: dst[i] = (0 + sum val*src[j], increasing j) - b[i], + sums of squares
};
template <int MODE, typename P>
__global__ __launch_bounds__(PT) void row_chain_k(const P *__restrict__ ptr, const u32 *__restrict__ col, const double *__restrict__ val,
                                                  const double *__restrict__ xdiag, const double *__restrict__ src,
                                                  const double *__restrict__ b, double *__restrict__ dst, i64 n, double *__restrict__ partial) {
    __shared__ u32 scol[PCAP];
    __shared__ double sval[PCAP];
    __shared__ double sred[PT];
    const i64 r0 = (i64)blockIdx.x * PT;
    const i64 i = r0 + threadIdx.x;
    const i64 rend = std::min<i64>(r0 + PT, n);
    const u64 s = (u64)ptr[r0], e = (u64)ptr[rend];
    const bool staged = e - s <= (u64)PCAP;
    if (staged) {
        const int cnt = (int)(e - s);
        for (int t = threadIdx.x; t < cnt; t += PT) {
            scol[t] = col[s + t];
            sval[t] = val[s + t];
        }
    }
    __syncthreads();
    double sq = 0.0;
    if (i < n) {
        const u64 kb = (u64)ptr[i], ke = (u64)ptr[i + 1];
        double acc;
        if (MODE == ILU_LOWER) acc = xdiag[i] * src[i];
        else if (MODE == RESIDUAL) acc = 0.0;                          // res .= zero(eltype)
        else acc = src[i];
        for (u64 k = kb; k < ke; k++) {
            const u32 c = staged ? scol[k - s] : col[k];
            const double a = staged ? sval[k - s] : val[k];
            if (MODE == ILU_LOWER) acc = acc - a * (xdiag[c] * src[c]);
            else if (MODE == RESIDUAL) acc = acc + a * src[c];
            else acc = acc - a * src[c];
        }
        if (MODE == ILU_UPPER_SUB) dst[i] = dst[i] - acc;
        else if (MODE == RESIDUAL) {
            const double r = acc - b[i];
            dst[i] = r;
            sq = r * r;
        } else dst[i] = acc;
    }
    if (MODE == RESIDUAL) {  // fixed-order tree: identical run to run
        sred[threadIdx.x] = sq;
        __syncthreads();
        for (int w = PT / 2; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) sred[threadIdx.x] = sred[threadIdx.x] + sred[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) partial[blockIdx.x] = sred[0];
    }
}
// norm(res) from the per-workgroup sums of squares: lane t adds partials t, t+PT, ... in order, then a fixed tree
__global__ __launch_bounds__(PT) void norm_finish_k(const double *__restrict__ partial, i64 nb, double *__restrict__ out) {
    __shared__ double sred[PT];
    double a = 0.0;
    for (i64 q = threadIdx.x; q < nb; q += PT) a = a + partial[q];
    sred[threadIdx.x] = a;
    __syncthreads();
    for (int w = PT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sred[threadIdx.x] = sred[threadIdx.x] + sred[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sqrt(sred[0]);
}
// Jacobi: ldiv!(u, p, v): u[i] = invdiag[i]*v[i] (jacobi.jl:36-41); simple!'s step fuses `u .-= upd`
__global__ void jacobi_ldiv_k(const double *__restrict__ inv, const double *v, double *u, i64 n) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) u[i] = inv[i] * v[i];
}
__global__ void jacobi_sub_k(const double *__restrict__ inv, const double *__restrict__ res, double *__restrict__ u, i64 n) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) u[i] = u[i] - inv[i] * res[i];
}

int32_t check_handle(esp_handle *h, const char *what) {
    if (h->m != h->n) FAIL(h, ESP_ERR_INVALID, "%s: the matrix must be square", what);
    if (h->count != 0) FAIL(h, ESP_ERR_STATE, "%s: pending entries (flush first, like update! does)", what);
    (void)hipSetDevice(h->device);
    if (!h->csc_valid) CK(init_empty_csc(h));
    CK(fix_tail(h));
    if (h->nnz >= 0xFFFFFFF0ll || h->n >= 0xFFFFFFF0ll)
        FAIL(h, ESP_ERR_UNSUPPORTED, "%s: the preconditioners' index holds 32-bit positions and columns", what);
    return ESP_OK;
}

}  // namespace

// invdiag / xdiag from the current nzval (jacobi! / ilu0!); ILU0 / ILUAM without a stored diagonal -> ESP_ERR_INVALID
int32_t diag_refresh(esp_precon *p) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    CK(ensure(h, p->diag, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    if (n == 0) return ESP_OK;
    CK(ensure(h, h->misc, 256));
    unsigned long long *d_missing = (unsigned long long *)h->misc.p + 21;
    h->pin_scalar[0] = ~0ull;
    HIPCK(h, hipMemcpyAsync(d_missing, h->pin_scalar, 8, hipMemcpyHostToDevice, h->stream));
    espfold::Csc c{(const i64 *)h->colptr.p, (const i64 *)h->rowval.p, (double *)h->nzval.p, h->nnz};
    hipLaunchKernelGGL(precon_diag_k, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, c, n, (double *)p->diag.p, d_missing);
    HIPCK(h, hipGetLastError());
    if (p->kind == ESP_PRECON_JACOBI) return ESP_OK;  // (Inf there, nothing to read back)
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, d_missing, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    if (h->pin_scalar[0] != ~0ull)
        FAIL(h, ESP_ERR_INVALID, "%s: column %llu has no stored diagonal entry (the reference reads an undefined %s there)",
             p->kind == ESP_PRECON_ILU0 ? "ilu0" : "iluam", (unsigned long long)h->pin_scalar[0],
             p->kind == ESP_PRECON_ILU0 ? "idiag" : "diag[j]");
    return ESP_OK;
}

int32_t split_build(esp_precon *p, bool reversed) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    CK(csr_current(h));
    CK(ensure(h, p->lptr, sizeof(u32) * (size_t)(n + 1)));
    CK(ensure(h, p->uptr, sizeof(u32) * (size_t)(n + 1)));
    CK(ensure(h, p->dpos, sizeof(u32) * (size_t)std::max<i64>(n, 1)));
    u32 *lptr = (u32 *)p->lptr.p, *uptr = (u32 *)p->uptr.p;
    HIPCK(h, hipMemsetAsync(lptr, 0, sizeof(u32) * (size_t)(n + 1), h->stream));
    HIPCK(h, hipMemsetAsync(uptr, 0, sizeof(u32) * (size_t)(n + 1), h->stream));
    const u64 *rp = (const u64 *)h->csr_rowptr.p + 1;
    if (n > 0)
        hipLaunchKernelGGL(split_count_k, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, rp, (const u32 *)h->csr_col.p,
                           (const u32 *)h->csr_perm.p, n, lptr, uptr, (u32 *)p->dpos.p);
    int l = 0;
    CK(scan_inplace<u32, false>(h, lptr, n + 1, p->scanws, &l));
    CK(scan_inplace<u32, false>(h, uptr, n + 1, p->scanws, &l));
    HIPCK(h, hipMemcpyAsync(h->pin_scalar, lptr + n, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipMemcpyAsync((char *)h->pin_scalar + 8, uptr + n, 4, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    const i64 zl = (i64) * (u32 *)h->pin_scalar, zu = (i64) * (u32 *)((char *)h->pin_scalar + 8);
    CK(ensure(h, p->lcol, sizeof(u32) * (size_t)std::max<i64>(zl, 1)));
    CK(ensure(h, p->lpos, sizeof(u32) * (size_t)std::max<i64>(zl, 1)));
    CK(ensure(h, p->lval, sizeof(double) * (size_t)std::max<i64>(zl, 1)));
    CK(ensure(h, p->ucol, sizeof(u32) * (size_t)std::max<i64>(zu, 1)));
    CK(ensure(h, p->upos, sizeof(u32) * (size_t)std::max<i64>(zu, 1)));
    CK(ensure(h, p->uval, sizeof(double) * (size_t)std::max<i64>(zu, 1)));
    if (n > 0)
        hipLaunchKernelGGL(split_fill_k, dim3(grid_for(n, 256)), dim3(256), 0, h->stream, rp, (const u32 *)h->csr_col.p,
                           (const u32 *)h->csr_perm.p, n, (const u32 *)lptr, (const u32 *)uptr, (u32 *)p->lcol.p, (u32 *)p->lpos.p,
                           (u32 *)p->ucol.p, (u32 *)p->upos.p, reversed);
    HIPCK(h, hipGetLastError());
    return ESP_OK;
}

namespace {

// fresh: xdiag from the current diagonal as well (ilu0!), else the stored xdiag (ldiv! after an in-place value change)
int32_t split_scale(esp_precon *p, bool fresh) {
    esp_handle *h = p->h;
    if (p->n > 0) {
        if (fresh)
            hipLaunchKernelGGL(split_scale_k<true>, dim3(grid_for(p->n, PT)), dim3(PT), 0, h->stream, (const u32 *)p->lptr.p,
                               (const u32 *)p->lpos.p, (const u32 *)p->uptr.p, (const u32 *)p->upos.p, (const u32 *)p->dpos.p,
                               (double *)p->diag.p, (const double *)h->nzval.p, p->n, (double *)p->lval.p, (double *)p->uval.p);
        else
            hipLaunchKernelGGL(split_scale_k<false>, dim3(grid_for(p->n, PT)), dim3(PT), 0, h->stream, (const u32 *)p->lptr.p,
                               (const u32 *)p->lpos.p, (const u32 *)p->uptr.p, (const u32 *)p->upos.p, (const u32 *)p->dpos.p,
                               (double *)p->diag.p, (const double *)h->nzval.p, p->n, (double *)p->lval.p, (double *)p->uval.p);
    }
    HIPCK(h, hipGetLastError());
    p->values_version = h->values_version;
    return ESP_OK;
}

// in front of every ldiv! / simple!: the layout still describes the stored pattern, the scaled values the current nzval
int32_t precon_ready(esp_precon *p, const char *what) {
    esp_handle *h = p->h;
    CK(check_handle(h, what));
    if (h->pattern_version != p->pattern_version || h->nnz != p->nnz)
        FAIL(h, ESP_ERR_STATE, "%s: the matrix pattern changed since the preconditioner's last update! (update! first)", what);
    if (p->kind == ESP_PRECON_ILU0 && p->values_version != h->values_version) CK(split_scale(p, false));  // current nzval, stored xdiag
    if (holds_derived(p)) CK(derived_follow_stream(p));  // (B holds copies: the values as of the last update!, ILU0 included)
    if (p->kind == ESP_PRECON_SPAI) CK(spai_follow_stream(p));
    return ESP_OK;
}

// ldiv! on device vectors (v may equal u; tmp: n doubles of scratch)
int32_t ldiv_launch(esp_precon *p, const double *v, double *u) {
    esp_handle *h = p->h;
    const i64 n = p->n;
    if (n == 0) return ESP_OK;
    if (block_built(p)) return block_ldiv_launch(p, v, u, false);
    if (p->kind == ESP_PRECON_ILUK || p->kind == ESP_PRECON_ILUT) return ldiv_launch(p->der.inner, v, u);  // ILUAM of B / over F on the caller's vectors
    if (p->kind == ESP_PRECON_ILUAM) return iluam_solve(p, v, u, false);
    if (p->kind == ESP_PRECON_AMG) return amg_solve(p, v, u, false);
    if (p->kind == ESP_PRECON_CHOLESKY) return chol_solve(p, v, u, false);
    if (p->kind == ESP_PRECON_SPAI && p->spai_order != 0) return spai_apply(p, v, u, false);  // u = M*v
    const unsigned g = grid_for(n, PT);
    if (diag_applied(p)) {  // Jacobi's invdiag / SPAI-0's diagonal M
        hipLaunchKernelGGL(jacobi_ldiv_k, dim3(g), dim3(PT), 0, h->stream, (const double *)p->diag.p, v, u, n);
        return ESP_OK;
    }
    double *u1 = (double *)p->u1.p;  // pass 1 writes the scratch: its neighbours still read v (which may be u)
    hipLaunchKernelGGL((row_chain_k<ILU_LOWER, u32>), dim3(g), dim3(PT), 0, h->stream, (const u32 *)p->lptr.p, (const u32 *)p->lcol.p,
                       (const double *)p->lval.p, (const double *)p->diag.p, v, (const double *)nullptr, u1, n, (double *)nullptr);
    hipLaunchKernelGGL((row_chain_k<ILU_UPPER, u32>), dim3(g), dim3(PT), 0, h->stream, (const u32 *)p->uptr.p, (const u32 *)p->ucol.p,
                       (const double *)p->uval.p, (const double *)nullptr, (const double *)u1, (const double *)nullptr, u, n,
                       (double *)nullptr);
    return ESP_OK;
}

}  // namespace

int32_t solver_ready(esp_handle *h, esp_precon *p, const char *what) { return p ? precon_ready(p, what) : check_handle(h, what); }
int32_t precon_check_handle(esp_handle *h, const char *what) { return check_handle(h, what); }
int32_t precon_ldiv_launch(esp_precon *p, const double *v, double *u) { return ldiv_launch(p, v, u); }
// the many-column twin of ldiv_launch's first three branches (levels_many's kinds): one pass over the schedules for the chunk
int32_t precon_levels_many_launch(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, int nr, u32 live) {
    if (block_built(p)) return block_ldiv_many_launch(p, v, ldv, u, ldu, nr, live);
    if (p->kind == ESP_PRECON_ILUK || p->kind == ESP_PRECON_ILUT) p = p->der.inner;  // ILUAM of B / over F on the caller's arrays
    return iluam_solve_many(p, v, ldv, u, ldu, nr, live);
}

void ilu0_lower_launch(esp_precon *p, const double *v) {
    hipLaunchKernelGGL((row_chain_k<ILU_LOWER, u32>), dim3(grid_for(p->n, PT)), dim3(PT), 0, p->h->stream, (const u32 *)p->lptr.p,
                       (const u32 *)p->lcol.p, (const double *)p->lval.p, (const double *)p->diag.p, v, (const double *)nullptr,
                       (double *)p->u1.p, p->n, (double *)nullptr);
}

esp_precon *precon_new(esp_handle *h, int kind) {
    esp_precon *p = new esp_precon();
    p->h = h;
    p->kind = kind;
    p->n = h->n;
    h->live_precons++;
    p->pattern_version = 0;  // never matches: the first update! builds everything
    return p;
}
int32_t precon_finish(esp_precon *p, int32_t st, esp_precon **out) {
    if (st != ESP_OK) {
        (void)esp_precon_destroy(p);
        return st;
    }
    *out = p;
    return ESP_OK;
}

extern "C" int32_t esp_precon_create(esp_handle *h, int32_t kind, esp_precon **out) {
    if (!h || !out || (kind != ESP_PRECON_JACOBI && kind != ESP_PRECON_ILU0 && kind != ESP_PRECON_ILUAM)) return ESP_ERR_INVALID;
    *out = nullptr;
    CK(check_handle(h, "esp_precon_create"));
    esp_precon *p = precon_new(h, kind);
    return precon_finish(p, esp_precon_update(p), out);
}

extern "C" int32_t esp_precon_update(esp_precon *p) {
    if (!p) return ESP_ERR_INVALID;
    if (p->kind == ESP_PRECON_BLOCK) return block_update(p);  // B and the inner preconditioner (block.hip)
    if (p->kind == ESP_PRECON_AMG) return amg_update(p);      // the whole hierarchy (amg.hip)
    if (p->kind == ESP_PRECON_ILUK) return iluk_update(p);    // the filled matrix and the inner ILUAM (iluk.hip)
    if (p->kind == ESP_PRECON_ILUT) return ilut_update(p);    // the pattern S, the values F and the inner prefactored ILUAM (ilut.hip)
    if (p->kind == ESP_PRECON_COLORED) return color_update(p);  // the colouring, A[c,c] and the inner preconditioner (color.hip)
    if (p->kind == ESP_PRECON_SPAI) return spai_update(p);      // the approximate inverse M (spai.hip)
    if (p->kind == ESP_PRECON_LU) return lu_update(p);          // the ordering, the filled matrix and the inner ILUAM (lu.hip)
    if (p->kind == ESP_PRECON_CHOLESKY) return chol_update(p);  // the ordering, the panels and the numeric factorization (cholesky.hip)
    esp_handle *h = p->h;
    CK(check_handle(h, "esp_precon_update"));
    p->n = h->n;
    const bool rebuild = p->pattern_version != h->pattern_version || p->nnz != h->nnz;
    p->pattern_version = 0;  // (a failure below leaves a preconditioner that refuses ldiv! until the next good update!)
    if (p->kind == ESP_PRECON_JACOBI) {
        CK(diag_refresh(p));          // jacobi(A) / jacobi!
    } else if (p->kind == ESP_PRECON_ILUAM) {
        CK(iluam_update(p, rebuild)); // iluAM(A) / the numeric factorization on the kept analysis
    } else if (rebuild) {             // ilu0(A)
        CK(diag_refresh(p));          // (refuses a missing diagonal before the layout is built)
        CK(split_build(p, false));
        CK(ensure(h, p->u1, sizeof(double) * (size_t)std::max<i64>(p->n, 1)));
        CK(split_scale(p, false));
    } else {                          // ilu0!: xdiag and the scaled values in one pass
        CK(split_scale(p, true));
    }
    HIPCK(h, hipStreamSynchronize(h->stream));
    p->nnz = h->nnz;
    p->pattern_version = h->pattern_version;
    return ESP_OK;
}

extern "C" int32_t esp_precon_ldiv(esp_precon *p, const double *v, double *u, int32_t on_device) {
    if (!p || !v || !u) return ESP_ERR_INVALID;
    esp_handle *h = p->h;
    CK(precon_ready(p, "esp_precon_ldiv"));
    const i64 n = p->n;
    const double *dv = v;
    double *du = u;
    if (!on_device) {
        CK(ensure(h, p->hv, sizeof(double) * (size_t)std::max<i64>(n, 1)));
        HIPCK(h, hipMemcpyAsync(p->hv.p, v, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        dv = du = (double *)p->hv.p;
    }
    CK(ldiv_launch(p, dv, du));
    HIPCK(h, hipGetLastError());
    if (!on_device) HIPCK(h, hipMemcpyAsync(u, du, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}

// ldiv! of k columns (include/esparse_hip.h, SEVERAL RIGHT-HAND SIDES).  The two panel kinds run their chunked solves, Jacobi
// (SPAI-0) and ILU0 the many-column kernels of krylov_many.hip, every kind that ends in ILUAM's level schedules or in block.hip's
// gather / inner solve / scatter (levels_many) ONE pass over them per chunk of ESP_MANY_CHUNK columns, a narrower last chunk masked
// (precon_levels_many_launch); AMG and SPAI-1 alone run ldiv_launch column by column.  Host arrays pass through p->hv,
// ESP_MANY_CHUNK columns at a time.  esp_precon_many_stats tells afterwards which form ran
extern "C" int32_t esp_precon_ldiv_many(esp_precon *p, const double *V, int64_t ldv, double *U, int64_t ldu, int64_t k, int32_t on_device) {
    if (!p) return ESP_ERR_INVALID;
    esp_handle *h = p->h;
    const i64 n = p->n, ldmin = std::max<i64>(n, 1);
    if (k < 0 || ldv < ldmin || ldu < ldmin) FAIL(h, ESP_ERR_INVALID, "esp_precon_ldiv_many: k = %lld, ldv = %lld, ldu = %lld for n = %lld", (long long)k, (long long)ldv, (long long)ldu, (long long)n);
    if (k > 0 && n > 0) {
        if (!V || !U) return ESP_ERR_INVALID;
        const double *ve = V + (k - 1) * ldv + n, *ue = U + (k - 1) * ldu + n;
        if (V < ue && U < ve && !(U == V && ldu == ldv))
            FAIL(h, ESP_ERR_INVALID, "esp_precon_ldiv_many: U and V overlap (only U == V with ldu == ldv is an in-place solve)");
    }
    if (k == 1 && n > 0) {  // the single-vector path itself
        many_note(p, 0, 0, 0);
        return esp_precon_ldiv(p, V, U, on_device);
    }
    CK(precon_ready(p, "esp_precon_ldiv"));
    const bool chol = p->kind == ESP_PRECON_CHOLESKY, lup = block_built(p) && p->lup;
    const bool fused = !block_built(p) && (diag_applied(p) || p->kind == ESP_PRECON_ILU0);
    const bool lev = !lup && levels_many(p);
    if (k == 0) return ESP_OK;
    const i64 chunks = ceil_div<i64>(k, ESP_MANY_CHUNK);
    many_note(p, k == 1 ? 0 : chol || lup || fused || lev ? 2 : 1, k == 1 ? 0 : k - (chunks - 1) * ESP_MANY_CHUNK, k == 1 ? 0 : chunks);
    if (n == 0) return ESP_OK;
    if (!on_device) CK(ensure(h, p->hv, sizeof(double) * (size_t)n * ESP_MANY_CHUNK));
    const i64 step = on_device ? k : ESP_MANY_CHUNK;  // (device arrays: one pass; the panel kinds chunk them themselves)
    for (i64 r0 = 0; r0 < k; r0 += step) {
        const i64 nr = std::min<i64>(step, k - r0);
        const double *dv = V + r0 * ldv;
        double *du = U + r0 * ldu;
        i64 dldv = ldv, dldu = ldu;
        if (!on_device) {
            HIPCK(h, hipMemcpy2DAsync(p->hv.p, sizeof(double) * (size_t)n, dv, sizeof(double) * (size_t)ldv, sizeof(double) * (size_t)n, (size_t)nr,
                                      hipMemcpyHostToDevice, h->stream));
            dv = du = (double *)p->hv.p;
            dldv = dldu = n;
        }
        if (chol) CK(chol_solve_many(p, dv, dldv, du, dldu, nr));
        else if (lup) CK(lup_solve_many(p, dv, dldv, du, dldu, nr));
        else if (fused) CK(precon_ldiv_many_launch(p, dv, dldv, du, dldu, nr));
        else if (lev)
            for (i64 c0 = 0; c0 < nr; c0 += ESP_MANY_CHUNK) {
                const int nc = (int)std::min<i64>(ESP_MANY_CHUNK, nr - c0);
                CK(precon_levels_many_launch(p, dv + c0 * dldv, dldv, du + c0 * dldu, dldu, nc, all_live(nc)));
            }
        else
            for (i64 r = 0; r < nr; r++) CK(ldiv_launch(p, dv + r * dldv, du + r * dldu));
        HIPCK(h, hipGetLastError());
        if (!on_device)
            HIPCK(h, hipMemcpy2DAsync(U + r0 * ldu, sizeof(double) * (size_t)ldu, du, sizeof(double) * (size_t)n, sizeof(double) * (size_t)n, (size_t)nr,
                                      hipMemcpyDeviceToHost, h->stream));
    }
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}

extern "C" int32_t esp_precon_destroy(esp_precon *p) {
    if (!p) return ESP_OK;
    esp_handle *h = p->h;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    block_release(p);
    iluk_release(p);
    ilut_release(p);
    color_release(p);
    spai_release(p);
    lu_release(p);
    chol_release(p);
    for (DevBuf *b : {&p->diag, &p->lptr, &p->uptr, &p->lcol, &p->ucol, &p->lpos, &p->upos, &p->dpos, &p->lval, &p->uval, &p->u1, &p->res,
                      &p->partial, &p->scanws, &p->hv, &p->hu})
        release(*b);
    iluam_release(p);
    amg_release(p);
    h->live_precons--;
    delete p;
    return ESP_OK;
}

// simple!(u, A, b; abstol, reltol, maxiter, Pl = p) (simple_iteration.jl:21-45), statement by statement
extern "C" int32_t esp_simple(esp_handle *h, esp_precon *p, const double *b, double *u, int32_t on_device, int64_t maxiter,
                              double abstol, double reltol, double *history, int64_t *iterations) {
    if (!h || !p || !b || !u || maxiter < 0) return ESP_ERR_INVALID;
    if (p->h != h) FAIL(h, ESP_ERR_INVALID, "esp_simple: the preconditioner belongs to another matrix");
    CK(precon_ready(p, "esp_simple"));
    CK(csr_current(h));
    const i64 n = h->n;
    const i64 nb = (i64)grid_for(n, PT);
    CK(ensure(h, p->res, sizeof(double) * (size_t)std::max<i64>(n, 1)));
    CK(ensure(h, p->partial, sizeof(double) * (size_t)(nb + 8)));
    const double *db = b;
    double *du = u;
    if (!on_device) {
        CK(ensure(h, p->hv, sizeof(double) * (size_t)std::max<i64>(n, 1)));
        CK(ensure(h, p->hu, sizeof(double) * (size_t)std::max<i64>(n, 1)));
        HIPCK(h, hipMemcpyAsync(p->hv.p, b, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        HIPCK(h, hipMemcpyAsync(p->hu.p, u, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, h->stream));
        db = (const double *)p->hv.p;
        du = (double *)p->hu.p;
    }
    double *res = (double *)p->res.p, *partial = (double *)p->partial.p, *d_norm = partial + nb;
    const u64 *rp = (const u64 *)h->csr_rowptr.p + 1;
    // res = A*u - b; then norm(res): one read-back per residual (the stop test runs on the host)
    auto residual = [&](double *r) -> int32_t {
        if (n > 0)
            hipLaunchKernelGGL((row_chain_k<RESIDUAL, u64>), dim3((unsigned)nb), dim3(PT), 0, h->stream, rp, (const u32 *)h->csr_col.p,
                               (const double *)h->csr_val.p, (const double *)nullptr, (const double *)du, db, res, n, partial);
        hipLaunchKernelGGL(norm_finish_k, dim3(1), dim3(PT), 0, h->stream, (const double *)partial, n > 0 ? nb : (i64)0, d_norm);
        HIPCK(h, hipGetLastError());
        HIPCK(h, hipMemcpyAsync(h->pin_scalar, d_norm, 8, hipMemcpyDeviceToHost, h->stream));
        HIPCK(h, hipStreamSynchronize(h->stream));
        *r = *(const double *)h->pin_scalar;
        return ESP_OK;
    };
    double r0 = 0.0;
    CK(residual(&r0));
    if (history) history[0] = r0;
    int64_t it = 0;
    esp_precon *const blk = block_permuted(p) ? p : nullptr;  // BlockPreconditioner, permuted path: gather, inner ldiv!, scatter
    p = fused_precon(p);                                      // ... identity path: the inner kind's own branch on its buffers
    for (int64_t i = 1; i <= maxiter; i++) {
        // ldiv!(upd, Pl, res); u .-= upd -- upd[i] rounded, then u[i] - upd[i]
        if (n > 0) {
            if (blk) {
                CK(block_ldiv_launch(blk, res, du, true));
            } else if (diag_applied(p)) {
                hipLaunchKernelGGL(jacobi_sub_k, dim3((unsigned)nb), dim3(PT), 0, h->stream, (const double *)p->diag.p,
                                   (const double *)res, du, n);
            } else if (p->kind == ESP_PRECON_ILUAM) {
                CK(iluam_solve(p, res, du, true));
            } else if (p->kind == ESP_PRECON_AMG) {
                CK(amg_solve(p, res, du, true));
            } else if (p->kind == ESP_PRECON_CHOLESKY) {
                CK(chol_solve(p, res, du, true));
            } else if (p->kind == ESP_PRECON_SPAI) {
                CK(spai_apply(p, res, du, true));
            } else {
                double *u1 = (double *)p->u1.p;
                hipLaunchKernelGGL((row_chain_k<ILU_LOWER, u32>), dim3((unsigned)nb), dim3(PT), 0, h->stream, (const u32 *)p->lptr.p,
                                   (const u32 *)p->lcol.p, (const double *)p->lval.p, (const double *)p->diag.p, (const double *)res,
                                   (const double *)nullptr, u1, n, (double *)nullptr);
                hipLaunchKernelGGL((row_chain_k<ILU_UPPER_SUB, u32>), dim3((unsigned)nb), dim3(PT), 0, h->stream,
                                   (const u32 *)p->uptr.p, (const u32 *)p->ucol.p, (const double *)p->uval.p, (const double *)nullptr,
                                   (const double *)u1, (const double *)nullptr, du, n, (double *)nullptr);
            }
        }
        double r = 0.0;
        CK(residual(&r));  // mul!(res, A, u); res .-= b; r = norm(res)
        if (history) history[i] = r;
        it = i;
        if ((r / r0) < reltol || r < abstol) break;
    }
    if (iterations) *iterations = it;
    if (!on_device) HIPCK(h, hipMemcpyAsync(u, du, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCK(h, hipStreamSynchronize(h->stream));
    return ESP_OK;
}
