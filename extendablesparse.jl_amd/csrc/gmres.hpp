// gmres.hpp -- libesparse_hip: what esp_gmres (gmres.hip) and esp_gmres_many (gmres_many.hip) share: the layout of the scalar block
// and the bodies of the GMRES kernels.  gmres.hip states the algorithm and what every kernel does; a body here is the statement
// sequence of one kernel over ONE right-hand side, written against blockIdx.x / gridDim.x only, so that the single kernels run it as
// it is and the many-column kernels run it once per column with the columns on another grid dimension -- the same statements in the
// same order, hence the same bits.  `vs` is the distance between two basis vectors of one right-hand side.
// Every translation unit that includes this gets its own copy (an unnamed namespace).
#pragma once
#include "krylov.hpp"

namespace {

constexpr int GM_MAX = ESP_GMRES_RESTART_MAX;  // largest restart
constexpr int GM_LD = GM_MAX + 1;              // leading dimension of H in the scalar block
constexpr int GM_GROUP = 8;                    // trees of bdot_k that run batched through LDS (16 KB)
// the scalar block: H column-major | nullvec | rhs (y after lsq_k) | h | c | beta, acc, proj, the DGKS predicate (1.0 / 0.0) |
// what the host reads back: current, the correction passes so far (a count held as a double: exact)
enum {
    SC_H = 0,
    SC_NULL = SC_H + GM_LD * GM_MAX,
    SC_RHS = SC_NULL + GM_LD,
    SC_HV = SC_RHS + GM_LD,
    SC_CV = SC_HV + GM_MAX,
    SC_BETA = SC_CV + GM_MAX,
    SC_ACC,
    SC_PROJ,
    SC_FLAG,
    SC_OUT,
    SC_PASSES,
    SC_COUNT = SC_PASSES + 3
};
static_assert(SC_OUT % 2 == 0, "the read-back is one aligned 16-byte copy");

__device__ __forceinline__ void gm_scalars(double *__restrict__ sc) {
    for (int i = threadIdx.x; i < SC_COUNT; i += KT) sc[i] = i >= SC_NULL && i < SC_RHS ? 1.0 : 0.0;  // nullvec = 1
}

// beta = norm(v) from its level 1, v = v * (1.0/beta); workgroup 0: beta, acc = 1 and (first: the start of a solve) current = beta
__device__ __forceinline__ void gm_start(const double *__restrict__ p1, i64 nb1, double *__restrict__ v, i64 n, double *__restrict__ sc,
                                         int first, double *sred) {
    const double beta = sqrt(level2(p1, nb1, sred));
    const double inv = 1.0 / beta;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sc[SC_BETA] = beta;
        sc[SC_ACC] = 1.0;
        if (first) sc[SC_OUT] = beta;
    }
    const i64 n2 = n >> 1;
    double2 *v2 = (double2 *)v;
    for (i64 e = (i64)blockIdx.x * KT + threadIdx.x; e < n2; e += (i64)gridDim.x * KT) {
        double2 a = v2[e];
        a.x = a.x * inv;
        a.y = a.y * inv;
        v2[e] = a;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) v[n - 1] = v[n - 1] * inv;
}

// one column of modified Gram-Schmidt: H[i,k] = the dot whose level 1 is p1 (every workgroup finishes it, workgroup 0 stores it
// to hout); w = w - H[i,k]*vi; level 0 of dot(vnext, w) -- vnext == nullptr: of dot(w, w) -- in p0.  A workgroup takes two chunks
// of the summation shape per round, a lane two neighbouring elements (vectors 16-byte aligned).
__device__ __forceinline__ void gm_mgs_step(const double *__restrict__ p1, i64 nb1, const double *__restrict__ vi, double *__restrict__ w,
                                            const double *__restrict__ vnext, i64 n, i64 nb0, double *__restrict__ p0,
                                            double *__restrict__ hout, double (*sred)[KT]) {
    const double hik = level2(p1, nb1, sred[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) hout[0] = hik;
    const i64 nspan = (nb0 + 1) >> 1;
    for (i64 q = blockIdx.x; q < nspan; q += gridDim.x) {
        const i64 e = q * KT + threadIdx.x, i0 = 2 * e;
        double2 pr = {0.0, 0.0};
        if (i0 + 1 < n) {
            const double2 vv = ((const double2 *)vi)[e];
            double2 wv = ((double2 *)w)[e];
            wv.x = wv.x - hik * vv.x;
            wv.y = wv.y - hik * vv.y;
            ((double2 *)w)[e] = wv;
            const double2 nv = vnext ? ((const double2 *)vnext)[e] : wv;
            pr.x = nv.x * wv.x;
            pr.y = nv.y * wv.y;
        } else if (i0 < n) {  // the scalar tail of an odd n
            const double wi = w[i0] - hik * vi[i0];
            w[i0] = wi;
            pr.x = (vnext ? vnext[i0] : wi) * wi;
        }
        ((double2 *)&sred[0][0])[threadIdx.x] = pr;  // element 2t + s of the round = place 2t + s of the two chunks
        trees<2>(sred, p0 + 2 * q, 1, nb0 - 2 * q < 2 ? 1 : 2);
    }
}

// level 0 of dot(V[j], w) for j = 0..k-1 from one read of w: dot j in p0[j*nb0 + q]; the columns in groups of GM_GROUP trees
__device__ __forceinline__ void gm_bdot(const double *__restrict__ V, i64 vs, int k, const double *__restrict__ w, i64 n, i64 nb0,
                                        double *__restrict__ p0, double (*sred)[KT]) {
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
        const double wv = i < n ? w[i] : 0.0;
        for (int g = 0; g < k; g += GM_GROUP) {
#pragma unroll
            for (int d = 0; d < GM_GROUP; d++) sred[d][threadIdx.x] = (g + d < k && i < n) ? V[(i64)(g + d) * vs + i] * wv : 0.0;
            trees<GM_GROUP>(sred, p0 + (i64)g * nb0 + q, nb0, k - g < GM_GROUP ? k - g : GM_GROUP);
        }
    }
}

// ONE workgroup: level 2 of the k dots.  pass 0: h[j] (CGS) and proj = sqrt(h[0]^2 + ..) ; pass > 0, only while the predicate
// holds: c[j], proj = that norm of c, h[j] = h[j] + c[j], one more correction pass counted
__device__ __forceinline__ void gm_coef(const double *__restrict__ p1, i64 nb1, int k, double *__restrict__ sc, int pass, double *sred) {
    if (pass > 0 && sc[SC_FLAG] == 0.0) return;
    double s = 0.0;
    for (int j = 0; j < k; j++) {
        const double d = level2(p1 + (i64)j * nb1, nb1, sred);
        if (threadIdx.x == 0) {
            if (pass == 0) {
                sc[SC_HV + j] = d;
            } else {
                sc[SC_CV + j] = d;
                sc[SC_HV + j] = sc[SC_HV + j] + d;
            }
            s = s + d * d;
        }
    }
    if (threadIdx.x == 0) {
        sc[SC_PROJ] = sqrt(s);
        if (pass > 0) sc[SC_PASSES] = sc[SC_PASSES] + 1.0;
    }
}

// a[e] = (..(a[e] -+ coef[0]*V[e,0]) -+ ..) -+ coef[m-1]*V[e,m-1] (SUB: the differences of the orthogonalisation; else the sums
// of the solution update), with level 0 of dot(a, a) when p0
template <bool SUB>
__device__ __forceinline__ void gm_comb(const double *__restrict__ V, i64 vs, int m, const double *__restrict__ coef, double *__restrict__ a,
                                        i64 n, i64 nb0, double *__restrict__ p0, double *sred, double *sco) {
    if ((int)threadIdx.x < m) sco[threadIdx.x] = coef[threadIdx.x];
    __syncthreads();
    for (i64 q = blockIdx.x; q < nb0; q += gridDim.x) {
        const i64 i = q * KT + threadIdx.x;
        double prod = 0.0;
        if (i < n) {
            double ai = a[i];
            for (int j = 0; j < m; j++) {
                if (SUB) ai = ai - sco[j] * V[(i64)j * vs + i];
                else ai = ai + sco[j] * V[(i64)j * vs + i];
            }
            a[i] = ai;
            prod = ai * ai;
        }
        if (p0) {
            const double t = tree256(prod, sred);
            if (threadIdx.x == 0) p0[q] = t;
            __syncthreads();
        }
    }
}

// ONE workgroup: nrm = norm(w) from its level 1; the DGKS predicate of the next correction pass: nrm < eta*proj and (but for the
// first) every predicate before it
__device__ __forceinline__ void gm_pred(const double *__restrict__ p1, i64 nb1, double *__restrict__ sc, double eta, int first, double *sred) {
    if (!first && sc[SC_FLAG] == 0.0) return;
    const double nrm = sqrt(level2(p1, nb1, sred));
    if (threadIdx.x == 0) sc[SC_FLAG] = nrm < eta * sc[SC_PROJ] ? 1.0 : 0.0;
}

// nrm = norm(w) from its level 1 (every workgroup), w = w * (1.0/nrm); workgroup 0: H[0..k-1,k-1] = hsrc (MGS: already there),
// H[k,k-1] = nrm, then the residual recurrence: nullvec[k], acc, current
__device__ __forceinline__ void gm_norm(const double *__restrict__ p1, i64 nb1, double *__restrict__ w, i64 n, double *sc, int k,
                                        const double *hsrc, double *sred) {
    const double nrm = sqrt(level2(p1, nb1, sred));
    const double inv = 1.0 / nrm;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double *Hc = sc + SC_H + (k - 1) * GM_LD;
        double s = 0.0;
        for (int i = 0; i < k; i++) {
            const double hv = hsrc[i];
            Hc[i] = hv;
            s = s + sc[SC_NULL + i] * hv;
        }
        Hc[k] = nrm;
        const double nv = -(s / nrm);
        sc[SC_NULL + k] = nv;
        const double acc = sc[SC_ACC] + nv * nv;
        sc[SC_ACC] = acc;
        sc[SC_OUT] = sc[SC_BETA] / sqrt(acc);
    }
    const i64 n2 = n >> 1;
    double2 *w2 = (double2 *)w;
    for (i64 e = (i64)blockIdx.x * KT + threadIdx.x; e < n2; e += (i64)gridDim.x * KT) {
        double2 a = w2[e];
        a.x = a.x * inv;
        a.y = a.y * inv;
        w2[e] = a;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) w[n - 1] = w[n - 1] * inv;
}

// one thread: the Givens rotations column by column over H and rhs = (beta, 0, .., 0), the back substitution; y in rhs[0..m-1]
__device__ __forceinline__ void gm_lsq(double *__restrict__ sc, int m) {
    double *H = sc + SC_H, *rhs = sc + SC_RHS;
    rhs[0] = sc[SC_BETA];
    for (int i = 1; i <= m; i++) rhs[i] = 0.0;
    for (int i = 0; i < m; i++) {
        const double f = H[i + i * GM_LD], g = H[i + 1 + i * GM_LD];
        double c = 1.0, s = 0.0;
        if (!(g == 0.0)) {
            const double r = sqrt(f * f + g * g);
            c = f / r;
            s = g / r;
        }
        H[i + i * GM_LD] = c * f + s * g;
        for (int j = i + 1; j < m; j++) {
            const double t = -s * H[i + j * GM_LD] + c * H[i + 1 + j * GM_LD];
            H[i + j * GM_LD] = c * H[i + j * GM_LD] + s * H[i + 1 + j * GM_LD];
            H[i + 1 + j * GM_LD] = t;
        }
        const double t = -s * rhs[i] + c * rhs[i + 1];
        rhs[i] = c * rhs[i] + s * rhs[i + 1];
        rhs[i + 1] = t;
    }
    for (int i = m - 1; i >= 0; i--) {
        double z = rhs[i];
        for (int j = i + 1; j < m; j++) z = z - H[i + j * GM_LD] * rhs[j];
        rhs[i] = z / H[i + i * GM_LD];
    }
}

}  // namespace
