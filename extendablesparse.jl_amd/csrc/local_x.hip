// local_x.hip -- pair_gen_pred_k: the PREDICTED pair form of the bucket kernel (pair_pred_k, local_w.hip) for a batch of the
// stencil generator that was never written (esp_handle::LazyStencil): the workgroup FORMS the updates of its 512 columns.
//
// The generator is a pure function of (grid, seed, rand_mode, kind) and a node number, and the updates that land in column l
// come from at most four nodes -- l - nx ny, l - nx, l - 1 and l itself.  Sorted by (row, call order), as pair_pred_k sorts a
// column's run, they are
//   rows l - nx ny, l - nx, l - 1 : one update each, -v of the pair the neighbour started towards l
//   row  l                        : +v of those three pairs, then the node's own terms in call order: +vx, the x boundary
//                                   term, +vy, the y boundary term, +vz, the z boundary term
//   rows l + 1, l + nx, l + nx ny : one update each, -v of the node's own pairs
// -- at most 12 updates over at most 7 rows, the rows strictly increasing wherever the pairs exist (no x pair when nx = 1 ...).
// The run is therefore born sorted: no load, no counting sort, no sorting network (dropped), and the LDS holds the dense
// records only (512 x 7 x 12 B = 42 KiB: three workgroups per CU).  The updates are folded as they are formed: through
// espfold::fold_step_update / fold_step_sel where a value can be zero or the kind creates a row whatever the value (rand_mode 2,
// RAWUPDATE), and without either where every update is an UPDATE of a strictly positive value (rand_mode 0 and 1: the FLAGS form
// -- a row is present exactly when its flag is on, an off-diagonal record is -v, the diagonal the sum in call order).
// From "entries the run emits" on the kernel calls the functions pair_pred_k calls (pair.hpp):
// pair_place scans the emitted counts, pair_table_hit is the check against the table -- a miss stores nothing --, pair_store
// the coalesced rowval / nzval stores and the lane's colptr, pair_grand_total the granule of the grand total.  Its own: the
// grand total and a miss (PRED_MISS) go to pinned host memory (Args::host_words).  No ticket, no look-back, nothing that waits
// for another workgroup, no memset in front of the launch and no copy behind it.
//
// A step that repeats the last one's structure stores the values alone (the template parameter KEEP, esp_handle::KeptStructure):
// colptr and rowval -- 8 Z + 8 (N + 1) of the 16 Z + 8 (N + 1) bytes -- already lie where the handle's last fused flush wrote them.
// The kernel was store-limited (393 us at 256^3, 273 without the rowval store; NOTES/round16.md); the KEEP form needs no rows in
// LDS (28 KiB: four workgroups per CU) and took 233 us -- 181 us of them the stores (the kernel with constant values), the rest
// the issue of the draws' arithmetic (NOTES/round20.md).  Two cuts in that arithmetic leave 205 us: a quotient by hx, hy or hz
// goes through a reciprocal the thread forms once, and the x and y pair values of a column's lower neighbours come from the
// lanes that formed them, through 8 KiB of LDS (36 KiB and 50 KiB: still four and three workgroups per CU) and one barrier.
// Round 21 (NOTES/round21.md) went after the instructions that are not a draw: the random mode is a template parameter of the
// source (no select per draw) and the plain division is gone (the launcher refuses spacings outside [2^-100, 2^100] before it
// launches anything), the FLAGS fold above, pair_store's 16-byte stores and pair_place's scalar wave number (pair.hpp, shared
// with pair_k and pair_pred_k): 0.2231 -> 0.2037 ms a step, 212 -> 192 us.  Measured and dropped: unpredicated record writes
// for a wave whose lanes all hold seven rows (its range overlapped its parent's).  Not built: the three reciprocals once per
// plan -- Consts still forms them in every thread; a timing probe puts them at another 2 % of the step.
//
// Where the values come from is the template parameter SRC (FdSource: the built-in generator's draws, the expressions and the
// operation order of espgen::fdrand_part_k -- compiled without FMA contraction like every unit); a source that reads edge
// coefficients from a caller's arrays fills the same StencilColumn in the same two steps: Consts (what a thread forms once),
// upper() (the flags and the node's own pairs, vhi), then -- behind the barrier that publishes vhi[0] and vhi[1] -- lower().
#include "generators.hpp"
#include "local.hpp"
#include "pair.hpp"

namespace esplocal {

namespace {
constexpr int G_ROWS = 7;                  // rows a column of the 7-point stencil can hold
constexpr int G_CAP = THREADS * G_ROWS;    // records of a pair
}  // namespace

// What column l = g + 1 receives.  lo(q) / hi(q): the pair towards l - stride[q] / l + stride[2 - q] exists (q = 0, 1, 2: the
// strides nx ny, nx, 1); v: the pair's value -- the off-diagonal update is -v, the diagonal one +v; b(q) / vb: the node's boundary
// terms in x, y, z.  The flags are compares on the node's (i, j, k), taken where they are used: a compare leaves a lane mask in
// scalar registers, a flag kept from upper() to the fold is a byte in a vector register that every use has to test again.
struct StencilColumn {
    i64 stride[3];
    i64 i, j, k, nx, ny, nz;
    double vlo[3], vhi[3], vb[3];
    __device__ __forceinline__ bool lo(int q) const { return q == 0 ? k > 1 : q == 1 ? j > 1 : i > 1; }
    __device__ __forceinline__ bool hi(int q) const { return q == 0 ? i < nx : q == 1 ? j < ny : k < nz; }
    __device__ __forceinline__ bool b(int q) const {
        return q == 0 ? (i == 1 || i == nx) : q == 1 ? (ny > 2 && (j == 1 || j == ny)) : (nz > 2 && (k == 1 || k == nz));
    }
};

// f() where some active lane of the wave has `on` (a wave-uniform branch: no lane data crosses), else 0.0 -- a value nobody reads
template <class F>
__device__ __forceinline__ double draw_if(bool on, F f) {
    return __ballot(on) != 0 ? f() : 0.0;
}

// the built-in generator (espgen::FdArgs without the producer's tables)
//
// The division.  A pair's value is u h h' / h'' with h'' one of the kernel's three arguments hx, hy, hz, so the reciprocal and its
// refinement -- the part of the compiler's division that depends on the denominator alone -- are formed once per thread
// (espgen::SharedDiv, Consts below) and a quotient is quot_mid()'s product, exact remainder and final fma: the bits of `/` whenever
// denominator and numerator lie in SharedDiv::mid's range [2^-400, 2^400] or the numerator is 0.  u is 1, 0.1 + u' or u' with u' = 0
// or in [2^-53, 1), so a numerator is 0 or lies in [2^-53 h h', 1.1 h h']: with every h in [2^-100, 2^100] that is inside
// [2^-253, 2^201], and no product on the way is subnormal.  The launcher tests the three h once on the host and launches nothing
// for other spacings (it returns false; flush_local then serves the flush unfused), so the kernel holds no plain division.
// h = 1 / n for a grid the API accepts (1 <= n < 2^63): the test always passes there.
//
// The random mode is the template parameter MODE (0: every u is 1; 1: 0.1 + u'; 2: u'), so a draw carries no select.  With MODE 0
// or 1 every u is at least 0.1: every pair value and boundary term is strictly positive (`positive`), which the kernel's fold of
// UPDATE entries uses -- a row is then present exactly when its flag is on.  MODE 2 can draw u' = 0 and keeps the general fold.
//
// Pair values through LDS.  The x pair towards l - 1 is the pair node l - 1 starts towards l -- the vhi[0] lane t - 1 forms, the
// same expression on the same counter, the same bits --, the y pair towards l - nx the vhi[1] of lane t - nx.  upper() forms the
// lane's own three pairs, the kernel leaves vhi[0] and vhi[1] in LDS at slot t, and behind one barrier lower() takes vlo[2] from
// slot t - 1 (t >= 1) and vlo[1] from slot t - nx (t >= nx): the slot's lane owns a lower column of the same pair of buckets, so
// it has a column and wrote.  The first lane's x value, the first nx lanes' y values and every z value are drawn as before.
template <int MODE>
struct FdSource {
    // every pair value and boundary term is strictly positive: u is 1 or at least 0.1 and no product underflows (above)
    static constexpr bool positive = MODE == 0 || MODE == 1;
    i64 nx, ny, nz;
    double hx, hy, hz;
    u64 seed;
    int fast;
    u64 magic_nx, magic_nxny;
    u64 zsub[3];  // 6 d GOLDEN for d = nx ny, nx, 1 (wrapping u64, formed once on the host): draw 0 of node g - d has the counter z0(g) - zsub

    // what a thread forms once, whatever its column: the three denominators' reciprocals
    struct Consts {
        espgen::SharedDiv x, y, z;
        __device__ __forceinline__ explicit Consts(const FdSource &s) : x(s.hx), y(s.hy), z(s.hz) {}
    };
    __device__ __forceinline__ double over(double n, const espgen::SharedDiv &by) const {
        return by.quot_mid(n);
    }
    // draw q of node gg: counter 6 gg + q (espgen::fd_rand_z); z0(g - d) = z0(g) - 6 d GOLDEN exactly (the arithmetic wraps)
    __device__ __forceinline__ u64 z0(i64 g) const { return seed + (6ull * (u64)g + 1ull) * ESP_GOLDEN; }

    // the column's flags and the three pairs its node starts (vhi[0], vhi[1]: what the lanes above take from LDS)
    __device__ __forceinline__ void upper(const Consts &k, i64 g, StencilColumn &c) const {
        espgen::fd_node(*this, g, &c.i, &c.j, &c.k);
        constexpr int md = MODE;
        const u64 zg = z0(g);
        c.stride[0] = nx * ny, c.stride[1] = nx, c.stride[2] = 1;
        c.nx = nx, c.ny = ny, c.nz = nz;
        c.vhi[0] = over(espgen::fd_rand_z(md, zg, 0) * hy * hz, k.x);
        c.vhi[1] = over(espgen::fd_rand_z(md, zg, 2) * hx * hz, k.y);
        c.vhi[2] = over(espgen::fd_rand_z(md, zg, 4) * hx * hy, k.z);
    }
    // the lower neighbours' pairs and the boundary terms; sx / sy: vhi[0] / vhi[1] of the workgroup's lanes, slot = lane.
    // A draw is formed only where some lane of the wave uses it (the kernel's step() does not look at a value whose flag is off:
    // 0.0 stands there).  At 256^3 the y and z boundary draws are skipped in more than 99 % of the waves, the x boundary draw in
    // half of them, the x draw in all but a pair's first wave and the y draw in its upper four.
    __device__ __forceinline__ void lower(const Consts &k, i64 g, int t, const double *sx, const double *sy, StencilColumn &c) const {
        constexpr int md = MODE;
        const u64 zg = z0(g);
        const bool x_in = c.lo(2) && t >= 1, y_in = c.lo(1) && (i64)t >= nx;
        const double x_lds = sx[x_in ? t - 1 : 0], y_lds = sy[y_in ? t - (int)nx : 0];  // (slots 0 .. t - 1)
        c.vlo[0] = draw_if(c.lo(0), [&] { return over(espgen::fd_rand_z(md, zg - zsub[0], 4) * hx * hy, k.z); });
        const double y_drawn = draw_if(c.lo(1) && !y_in, [&] { return over(espgen::fd_rand_z(md, zg - zsub[1], 2) * hx * hz, k.y); });
        const double x_drawn = draw_if(c.lo(2) && !x_in, [&] { return over(espgen::fd_rand_z(md, zg - zsub[2], 0) * hy * hz, k.x); });
        c.vlo[1] = y_in ? y_lds : y_drawn;
        c.vlo[2] = x_in ? x_lds : x_drawn;
        c.vb[0] = draw_if(c.b(0), [&] { return espgen::fd_rand_z(md, zg, 1) * hy * hz; });
        c.vb[1] = draw_if(c.b(1), [&] { return espgen::fd_rand_z(md, zg, 3) * hx * hz; });
        c.vb[2] = draw_if(c.b(2), [&] { return espgen::fd_rand_z(md, zg, 5) * hx * hy; });
    }
};

// KEEP: colptr and rowval hold what the handle's last fused flush of this plan, table, grid and kind wrote, and that flush emitted
// the grid's whole structural pattern (esp_handle::KeptStructure) -- a step that hits the table in every pair then has that very
// pattern, so the kernel stores the values alone: no srow (the LDS holds the values only), no out_row, no colptr.  Everything that
// decides is the writing form's: the fold, pair_place, pair_table_hit, PRED_MISS and the grand total.
template <int KEYS, class SRC, bool KEEP>
__global__ __launch_bounds__(THREADS, 6) void pair_gen_pred_k(Args a, SRC src, const u64 *pred, u64 out_cap) {
    static_assert(KEYS == 1 || KEYS == 2, "one kind: 2 = every update is an UPDATE");
    constexpr bool UPD = KEYS == 2;
    constexpr bool FLAGS = UPD && SRC::positive;  // no value is zero: a row is present exactly when its flag is on
    __shared__ u32 srow[KEEP ? 1 : G_CAP];  // the records' rows (1-based; not kept by the KEEP form) ...
    __shared__ double sval[G_CAP];          // ... and values
    __shared__ double shx[THREADS], shy[THREADS];  // the lanes' vhi[0] / vhi[1] (FdSource: pair values through LDS)
    __shared__ u32 lw[WAVES];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int s = (int)(a.first + (i64)blockIdx.x);
    if (s >= a.S) return;
    const u64 dst = esp_uniform_u64(pred[s]);
    const u64 dst_next = esp_uniform_u64(pred[s + 1]);
    const int ncl = 2 << a.cl_bits;
    const u64 hi = ((u64)s << (a.rem_bits + 1)) + a.base;  // the pair's prefix: that of its first bucket
    const i64 c_lo = (i64)(hi >> a.rb);
    const i64 c_hi = min(c_lo + (i64)ncl, a.col_end);
    const bool has = c_lo + t < c_hi;  // lane t owns column c_lo + t
    // ---- the column's run, folded as it is formed: row q of the seven (rows strictly increasing where they exist)
    bool present[G_ROWS];
    double acc[G_ROWS];
    u32 row[G_ROWS];
#pragma unroll
    for (int q = 0; q < G_ROWS; q++) present[q] = false, acc[q] = 0.0, row[q] = 0u;
    // the node's own pairs first; the x and y ones go through LDS to the lanes whose columns they end in.  The barrier stands
    // outside `has`: every lane of a workgroup that got past the uniform return above reaches it.
    const typename SRC::Consts k(src);
    StencilColumn c;
    if (has) {
        src.upper(k, c_lo + t, c);
        shx[t] = c.vhi[0];
        shy[t] = c.vhi[1];
    }
    __syncthreads();
    if (has) {
        src.lower(k, c_lo + t, t, shx, shy, c);
        const i64 l = c_lo + t + 1;
#pragma unroll
        for (int q = 0; q < 3; q++) row[q] = (u32)(l - c.stride[q]), row[4 + q] = (u32)(l + c.stride[2 - q]);
        row[3] = (u32)l;
        if constexpr (FLAGS) {
            // an off-diagonal record is -v, the bits of 0.0 + (-v) for v != 0; the diagonal takes its terms in call order, 0.0 for
            // a term that is off (x + 0.0 is x: no sum here is -0.0)
#pragma unroll
            for (int q = 0; q < 3; q++) {
                present[q] = c.lo(q), acc[q] = -c.vlo[q];
                present[4 + q] = c.hi(q), acc[4 + q] = -c.vhi[q];
            }
            bool any = false;
            double d = 0.0;
#pragma unroll
            for (int q = 0; q < 3; q++) any = any || c.lo(q), d = d + (c.lo(q) ? c.vlo[q] : 0.0);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                any = any || c.hi(q) || c.b(q);
                d = d + (c.hi(q) ? c.vhi[q] : 0.0);
                d = d + (c.b(q) ? c.vb[q] : 0.0);
            }
            present[3] = any, acc[3] = d;
        } else {
            // (MODE 2 can draw 0, RAWUPDATE creates a row whatever the value: the fold's own state machine)
            auto step = [&](int q, bool on, double v) {
                if (!on) return;
                if constexpr (UPD)
                    espfold::fold_step_update(present[q], acc[q], v);
                else
                    espfold::fold_step_sel(present[q], acc[q], a.kind32, v);
            };
#pragma unroll
            for (int q = 0; q < 3; q++) step(q, c.lo(q), -c.vlo[q]);
#pragma unroll
            for (int q = 0; q < 3; q++) step(3, c.lo(q), c.vlo[q]);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                step(3, c.hi(q), c.vhi[q]);
                step(3, c.b(q), c.vb[q]);
            }
#pragma unroll
            for (int q = 0; q < 3; q++) step(4 + q, c.hi(q), -c.vhi[q]);
        }
    }
    // entries the run emits: one per row that one of its updates creates
    u32 ec = 0;
#pragma unroll
    for (int q = 0; q < G_ROWS; q++) ec += present[q] ? 1u : 0u;
    const PairPlace pl = pair_place(ec, lw, lane, w);
    // ---- place: the table's, or nothing is stored
    if (!pair_table_hit(dst, dst_next, pl.total, out_cap, s)) {
        if (t == 0) a.host_words[1] = (u64)PRED_MISS;  // (the same constant from every missing pair: a plain store)
        return;
    }
    {
        u32 at = pl.at0;
#pragma unroll
        for (int q = 0; q < G_ROWS; q++) {
            if (present[q]) {
                if constexpr (!KEEP) srow[at] = row[q];
                sval[at] = acc[q];
                at++;
            }
        }
    }
    __syncthreads();
    pair_store<KEEP>(a, srow, sval, 0, dst, pl, hi, ncl, s, t);  // (srow holds 1-based rows)
    if (s == a.S - 1 && t == 0) a.host_words[0] = pair_grand_total(dst, pl.total);
}

bool launch_pair_gen_predicted(const Variant &v, unsigned grid, hipStream_t stream, const Args &a, const espgen::FdArgs &fd, const u64 *pred,
                               u64 out_cap, bool keep) {
    // (whole columns, at most 512 of them per pair, rows that fit the records' 32 bits)
    if (!v.fresh || v.pieces || a.cl_bits < 0 || (2 << a.cl_bits) > THREADS || a.rb >= 32 || !a.colptr_out || !a.host_words) return false;
    // (FdSource: the division.  Other spacings are not the fused kernel's: the caller serves the flush unfused)
    auto mid = [](double h) { return h >= 0x1.0p-100 && h <= 0x1.0p100; };
    if (!(mid(fd.hx) && mid(fd.hy) && mid(fd.hz))) return false;
    auto go = [&](auto M) {
        using Src = FdSource<decltype(M)::value>;
        const Src src{fd.nx, fd.ny, fd.nz, fd.hx, fd.hy, fd.hz, fd.seed, fd.fast, fd.magic_nx, fd.magic_nxny,
                      {6ull * (u64)(fd.nx * fd.ny) * ESP_GOLDEN, 6ull * (u64)fd.nx * ESP_GOLDEN, 6ull * ESP_GOLDEN}};
        return pair_for_keys(v.keys, [&](auto K) {
            constexpr int KEYS = decltype(K)::value;
            if (keep)
                hipLaunchKernelGGL((pair_gen_pred_k<KEYS, Src, true>), dim3(grid), dim3(THREADS), 0, stream, a, src, pred, out_cap);
            else
                hipLaunchKernelGGL((pair_gen_pred_k<KEYS, Src, false>), dim3(grid), dim3(THREADS), 0, stream, a, src, pred, out_cap);
        });
    };
    // (the mode as the generator reads it: 0, 1, anything else)
    if (fd.rand_mode == 0) return go(std::integral_constant<int, 0>{});
    if (fd.rand_mode == 1) return go(std::integral_constant<int, 1>{});
    return go(std::integral_constant<int, 2>{});
}

}  // namespace esplocal
