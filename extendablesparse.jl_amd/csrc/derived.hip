// derived.hip -- libesparse_hip: what the builders of a derived matrix share (see internal.hpp for the map of the translation units)
//
//   ScratchFlush     entries sorted, and folded where keys repeat, by an ESP_COO flush of a scratch handle: the route of
//                    esp_transpose's generic path, esp_matmul's generic tier and a column above the column sorts' limit (ColumnSort,
//                    linalg.hip: block.hip's permuted path, iluk.hip)
//   derived_update   the update! of the kinds that hold a matrix B made from A and an inner preconditioner of it (esp_precon::Derived:
//                    Block, Colored, ILU(k), ILUT); the kind supplies the builder of B
#include "internal.hpp"

namespace {

constexpr int DT = 256;  // threads of the kernel here

// pay != nullptr: src[q] and lev[q] from the sorted payloads first (maxlev: the largest level); then
// B.nzval[q] = src[q] == ILUK_FILL ? +0.0 : A.nzval[src[q]] (the bits)
__global__ __launch_bounds__(DT) void derived_gather_k(const u64 *__restrict__ pay, u32 *__restrict__ src, int32_t *__restrict__ lev,
                                                       const u64 *__restrict__ nzA, u64 *__restrict__ nzB, i64 nnzB,
                                                       unsigned long long *__restrict__ maxlev) {
    const i64 q = (i64)blockIdx.x * DT + threadIdx.x;
    u32 s = ILUK_FILL, l = 0;
    if (q < nnzB) {
        if (pay) {
            const u64 w = pay[q];
            s = (u32)w;
            l = (u32)(w >> 32);
            src[q] = s;
            lev[q] = (int32_t)l;
        } else {
            s = src[q];
        }
        nzB[q] = s == ILUK_FILL ? 0ull : nzA[s];
    }
    if (pay) {
        const u32 m = esp_wave_max(l);
        if ((threadIdx.x & 63) == 0 && m) atomicMax(maxlev, (unsigned long long)m);
    }
}

// update! with the pattern kept: B's values anew, in place
int32_t refresh_values(esp_precon *p) {
    if (p->kind == ESP_PRECON_ILUT) return ilut_warm(p);  // (F is no gather of A's values: sweeps from the current F)
    esp_handle *h = p->h, *bh = p->der.bh;
    if (bh->nnz > 0)
        derived_gather_launch(h->stream, nullptr, (u32 *)p->der.src.p, nullptr, (const u64 *)h->nzval.p, (u64 *)bh->nzval.p, bh->nnz, nullptr);
    HIPCK(h, hipGetLastError());
    bh->values_version++;
    return ESP_OK;
}

}  // namespace

void derived_gather_launch(hipStream_t s, const u64 *pay, u32 *src, int32_t *lev, const u64 *nzA, u64 *nzB, i64 nnzB,
                           unsigned long long *maxlev) {
    hipLaunchKernelGGL(derived_gather_k, dim3(grid_for(nnzB, DT)), dim3(DT), 0, s, pay, src, lev, nzA, nzB, nnzB, maxlev);
}

int32_t derived_follow_stream(esp_precon *p) {
    for (esp_handle *q : {p->der.bh, p->iluk_th, p->ilut_h[0], p->ilut_h[1], p->ilut_h[2], p->ilut_h[3]})
        if (q && q->stream != p->h->stream) CK(esp_set_stream(q, (void *)p->h->stream));
    return ESP_OK;
}

// The order of the statements is the guarantee "a failed rebuild leaves p as its last good update! made it": everything that can
// fail before B is replaced (the kind's buffers, the whole of build) comes first and changes nothing of p, so p stays usable where
// A's pattern is the one of its last good update!.  Once B is new, or its values are being overwritten in place, the inner
// preconditioner no longer belongs to it: pattern_version = 0 matches no pattern, and a failure from there on refuses ldiv! until
// the next good update!.  The three stamps come last, behind the synchronisation.  (color_update relies on the same order: it
// tells from der.rebuild whether a failed call had replaced B.)
int32_t derived_update(esp_precon *p, const char *what, int32_t (*build)(esp_precon *), const char *hint) {
    esp_handle *h = p->h;
    CK(precon_check_handle(h, "esp_precon_update"));
    if (windowed(h) || h->shard_user) FAIL(h, ESP_ERR_UNSUPPORTED, "%s: a column window / column shard", what);
    CK(derived_follow_stream(p));
    if (derived_stale(p)) {
        CK(build(p));
        p->pattern_version = 0;
        p->der.rebuild = false;
    } else {
        p->pattern_version = 0;
        CK(refresh_values(p));
    }
    const int32_t st = p->der.inner ? esp_precon_update(p->der.inner) : esp_precon_create(p->der.bh, p->der.inner_kind, &p->der.inner);
    if (st != ESP_OK) FAIL(h, st, "%s: %s%s", what, p->der.bh->err.c_str(), st == ESP_ERR_INVALID && p->blk_path ? hint : "");
    HIPCK(h, hipStreamSynchronize(h->stream));
    p->nnz = h->nnz;
    p->pattern_version = h->pattern_version;
    p->values_version = h->values_version;
    return ESP_OK;
}

ScratchFlush::~ScratchFlush() {
    if (sc_) (void)esp_destroy(sc_);
}

int32_t ScratchFlush::open(i64 m, i64 n, i64 count, bool fail_hook) {
    const int32_t st = esp_create(m, n, owner_->device, count, &sc_);
    if (st != ESP_OK) FAIL(owner_, st, "%s: scratch handle: %s", what_, esp_last_error(nullptr));
    if (fail_hook) {
        sc_->debug_fail_bucket = owner_->debug_fail_bucket;
        owner_->debug_fail_bucket = false;
    }
    const int32_t rs = reserve_append(sc_, count);
    if (rs != ESP_OK) FAIL(owner_, rs, "%s: append buffer of the scratch handle: %s", what_, sc_->err.c_str());
    count_ = count;
    return ESP_OK;
}

int32_t ScratchFlush::flush(i64 expected) {
    note_kind(sc_, ESP_COO, count_);
    sc_->count = count_;
    pending_changed(sc_);
    i64 z = 0;
    int32_t ch = 0;
    const int32_t fs = esp_flush(sc_, ESP_FLUSH_ROUTED, &z, &ch);
    if (fs != ESP_OK) FAIL(owner_, fs, "%s: flush of the scratch handle: %s", what_, sc_->err.c_str());
    const int32_t ft = fix_tail(sc_);
    if (ft != ESP_OK) FAIL(owner_, ft, "%s: %s", what_, sc_->err.c_str());
    HIPCK(owner_, hipStreamSynchronize(sc_->stream));
    if (expected >= 0 && sc_->nnz != expected)
        FAIL(owner_, ESP_ERR_HIP, "%s: the flush stored %lld entries of %lld", what_, (long long)sc_->nnz, (long long)expected);
    return ESP_OK;
}

void ScratchFlush::take(DevBuf &cp, DevBuf &rv, DevBuf &nz) {
    drop_kept(sc_);  // (the scratch handle gives its arrays away)
    std::swap(cp, sc_->colptr);
    std::swap(rv, sc_->rowval);
    std::swap(nz, sc_->nzval);
}
