// amg.hpp -- what amg.hip (the level container, smoothed aggregation, the V-cycle) shares with rsamg.hip (Ruge-Stueben coarsening)
#pragma once
#include "internal.hpp"

struct AmgLevel {
    esp_handle *A = nullptr, *P = nullptr;  // A_l (n x n), P_l (n x nc; nullptr on the coarsest level)
    i64 n = 0, nc = 0;
    double rho = 0.0;
    int rounds = 0;
    bool has_agg = false;    // smoothed aggregation: agg holds the aggregate of every unknown
    bool has_split = false;  // Ruge-Stueben: agg holds cnum of a C point, -1 (F, interpolated), -2 (F without interpolation)
    DevBuf w, agg;        // f64 n: omega*dinv; i64 n: see has_agg / has_split
    DevBuf x0, x1, b, r;  // f64 n each: the two iterates, the right-hand side (levels > 0), the residual
};
struct AmgData {
    int max_levels = 10, max_coarse = 64, pre = 1, post = 1;
    int coarsen = ESP_AMG_COARSEN_SA;
    double theta = 0.0;
    std::vector<AmgLevel> lv;
    DevBuf inv;  // n_L*n_L doubles, row-major
    bool has_inv = false;
};

namespace espamg {

constexpr int AT = 256;       // threads of every kernel but the Gauss-Jordan
constexpr int AMG_LONG = 32;  // a column with more stored entries is folded by its whole wave (Luby / PMIS rounds)

// the 32-bit mixer of the fixed hash, applied to i + 1
__device__ __forceinline__ u32 amg_mix(i64 i) {
    u32 x = (u32)i + 1u;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// internal handles of a build step: destroyed when the step ends unless taken over
struct Handles {
    std::vector<esp_handle *> v;
    ~Handles() {
        for (esp_handle *x : v)
            if (x) (void)esp_destroy(x);
    }
};

static inline espfold::Csc csc_of(const esp_handle *a) {
    return espfold::Csc{(const i64 *)a->colptr.p, (const i64 *)a->rowval.p, (double *)a->nzval.p, a->nnz};
}

}  // namespace espamg

#pragma GCC visibility push(hidden)
// amg.hip: an internal m x n handle on h's device and stream
int32_t amg_make_handle(esp_handle *h, i64 m, i64 n, esp_handle **out);
// rsamg.hip: the Ruge-Stueben coarsening of level L (its matrix in L.A, the row-wise index current): L.agg (the splitting), L.nc,
// L.rounds; where 0 < nc < n also L.P (n x nc) and *tt = transpose(P) (nc x n; the caller destroys it)
int32_t rsamg_coarsen(esp_handle *h, AmgLevel &L, double theta, esp_handle **tt);
#pragma GCC visibility pop

// a call of the library on internal handles: its message goes to h
#define SUB(h, sub, ...)                                                                  \
    do {                                                                                  \
        const int32_t _st = (__VA_ARGS__);                                                \
        if (_st != ESP_OK) FAIL(h, _st, "esp_precon_amg: %s", (sub)->err.c_str());       \
    } while (0)
