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
// for a wave whose lanes all hold seven rows (its range overlapped its parent's).
// Round 22 (NOTES/round22.md): the march.  Where a plane of the grid is a whole number of pairs (nx ny % ncl == 0, the flush from
// column 0 over the whole grid) a workgroup handles the same 512 (i, j) columns in a.march consecutive z planes: the pairs s,
// s + P, ... with P the pairs of a plane.  Once per march it forms what does not depend on the plane -- the reciprocals (round
// 21's open part: closed by this), the node's (i, j, k), the counter of its draw 0, the strides; the compares on i and j stay lane
// masks across the planes --, per plane k advances by 1 and the counter by 6 nx ny GOLDEN, and the z pair towards l - nx ny is
// the vhi[2] the same lane formed one plane below: a draw in the workgroup's first plane only.  Every other grid runs one plane
// per workgroup through the same body without the loop (the template parameter MARCH).  The march length is the host's
// (pair_gen_march_rule below): 3 planes at 256^3 on 256 compute units, 0.2016 -> 0.1954 ms a step, 188.8 -> 182.6 us in one
// session; longer marches lost to the partly filled last round of workgroups.  The table words must be scalar loads (`pred` is restrict, s a scalar): as a vector load their wait counts the
// stores of the plane below.
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
// (i, j, k) and the extents in 32 bits: the launcher takes grids whose rows fit 32 bits only (a.rb < 32), so every one of them is
// below 2^32 -- and the registers a marching thread carries from plane to plane are half as many.
struct StencilColumn {
    i64 stride[3];
    u32 i, j, k, nx, ny, nz;
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
        // (the same in every lane: the refined reciprocals go to scalar registers, where a march keeps them for nothing)
        __device__ __forceinline__ explicit Consts(const FdSource &s) : x(s.hx), y(s.hy), z(s.hz) {
            x.r = uniform(x.r), y.r = uniform(y.r), z.r = uniform(z.r);
        }
        __device__ __forceinline__ static double uniform(double v) {
            return __longlong_as_double((long long)esp_uniform_u64((u64)__double_as_longlong(v)));
        }
    };
    __device__ __forceinline__ double over(double n, const espgen::SharedDiv &by) const {
        return by.quot_mid(n);
    }
    // draw q of node gg: counter 6 gg + q (espgen::fd_rand_z); z0(g - d) = z0(g) - 6 d GOLDEN exactly (the arithmetic wraps)
    __device__ __forceinline__ u64 z0(i64 g) const { return seed + (6ull * (u64)g + 1ull) * ESP_GOLDEN; }

    // what a thread forms once per march: the node's (i, j, k), the strides and extents, and the counter of the node's draw 0
    __device__ __forceinline__ u64 begin(i64 g, StencilColumn &c) const {
        i64 i, j, k;
        espgen::fd_node(*this, g, &i, &j, &k);
        c.i = (u32)i, c.j = (u32)j, c.k = (u32)k;
        c.stride[0] = nx * ny, c.stride[1] = nx, c.stride[2] = 1;
        c.nx = (u32)nx, c.ny = (u32)ny, c.nz = (u32)nz;
        return z0(g);
    }
    // one plane up, node g + nx ny: the same (i, j), k + 1, and z0(g + nx ny) = z0(g) + 6 nx ny GOLDEN exactly (the arithmetic wraps)
    __device__ __forceinline__ u64 next_plane(u64 zg, StencilColumn &c) const {
        c.k += 1;
        return zg + zsub[0];
    }
    // the three pairs the column's node starts (vhi[0], vhi[1]: what the lanes above take from LDS; vhi[2]: what the same lane
    // takes one plane up)
    __device__ __forceinline__ void upper(const Consts &k, u64 zg, StencilColumn &c) const {
        constexpr int md = MODE;
        c.vhi[0] = over(espgen::fd_rand_z(md, zg, 0) * hy * hz, k.x);
        c.vhi[1] = over(espgen::fd_rand_z(md, zg, 2) * hx * hz, k.y);
        c.vhi[2] = over(espgen::fd_rand_z(md, zg, 4) * hx * hy, k.z);
    }
    // the lower neighbours' pairs and the boundary terms; sx / sy: vhi[0] / vhi[1] of the workgroup's lanes, slot = lane.
    // A draw is formed only where some lane of the wave uses it (the kernel's step() does not look at a value whose flag is off:
    // 0.0 stands there).  At 256^3 the y and z boundary draws are skipped in more than 99 % of the waves, the x boundary draw in
    // half of them, the x draw in all but a pair's first wave and the y draw in its upper four.  The z pair towards l - nx ny is
    // drawn in the first plane of a march only (`first`: the node below belongs to another workgroup); one plane up it is z_below,
    // the vhi[2] this lane formed for that node -- the same expression on the same counter, the same bits.
    __device__ __forceinline__ void lower(const Consts &k, u64 zg, int t, const double *sx, const double *sy, bool first, double z_below,
                                          StencilColumn &c) const {
        constexpr int md = MODE;
        const bool x_in = c.lo(2) && t >= 1, y_in = c.lo(1) && (i64)t >= nx;
        const double x_lds = sx[x_in ? t - 1 : 0], y_lds = sy[y_in ? t - (int)nx : 0];  // (slots 0 .. t - 1)
        if (first)
            c.vlo[0] = draw_if(c.lo(0), [&] { return over(espgen::fd_rand_z(md, zg - zsub[0], 4) * hx * hy, k.z); });
        else
            c.vlo[0] = z_below;
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
//
// MARCH: the workgroup handles a.march > 1 planes.  Without it (a grid that does not conform, or one the rule gives no march) the
// loop below runs once and is none: the kernel is the one-plane kernel of round 21, with its registers and its launch bound --
// the march's prologue, the scalars it keeps across planes and the 8-waves bound of its KEEP form cost a one-plane launch more
// than they give it (NOTES/round22.md).
template <int KEYS, class SRC, bool KEEP, bool MARCH>
__global__ __launch_bounds__(THREADS, KEEP && MARCH ? 8 : 6) void pair_gen_pred_k(Args a, SRC src, const u64 *__restrict__ pred, u64 out_cap) {
    static_assert(KEYS == 1 || KEYS == 2, "one kind: 2 = every update is an UPDATE");
    constexpr bool UPD = KEYS == 2;
    constexpr bool FLAGS = UPD && SRC::positive;  // no value is zero: a row is present exactly when its flag is on
    __shared__ u32 srow[KEEP ? 1 : G_CAP];  // the records' rows (1-based; not kept by the KEEP form) ...
    __shared__ double sval[G_CAP];          // ... and values
    __shared__ double shx[THREADS], shy[THREADS];  // the lanes' vhi[0] / vhi[1] (FdSource: pair values through LDS)
    __shared__ u32 lw[WAVES];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    // ---- the workgroup's march: pairs s, s + s_step, ... -- the same 512 (i, j) in a.march consecutive planes (pair_gen_march)
    const int ncl = 2 << a.cl_bits;
    int s = (int)(a.first + (i64)blockIdx.x), s_step = 0;
    if constexpr (MARCH) {
        const u32 wg = (u32)s, P = (u32)a.march_step, chunk = wg / P;  // (workgroup = (pair in plane, chunk), the pair fastest)
        // (the quotient comes out of vector registers; s must be a scalar: the table words are then scalar loads, which wait for no
        // store of the plane below -- a vector load's wait counts the stores too and would hold every plane behind the last one's)
        s = esp_uniform_i32((int)(chunk * (u32)a.march * P + (wg - chunk * P)));
        s_step = (int)P;
    }
    if (s >= a.S) return;
    // what does not depend on the plane, formed once: the reciprocals, the node's (i, j, k) and the counter of its first plane, the
    // strides.  `has` too: a marching grid has full pairs only (every lane owns a column in every plane), a grid that does not
    // conform runs one plane.
    const typename SRC::Consts k(src);
    StencilColumn c;
    const i64 g = (i64)((((u64)s << (a.rem_bits + 1)) + a.base) >> a.rb) + t;  // lane t owns column g (0-based) of the first plane
    const bool has = g < min(g - t + (i64)ncl, a.col_end);
    u64 zg = 0ull;
    if (has) zg = src.begin(g, c);
    c.vhi[2] = 0.0;
    u32 l = (u32)g + 1u;  // the column, 1-based (the records' rows are 32 bits wide: a.rb < 32)
    // Barriers.  A plane has three: (1) behind the writes of shx / shy, (2) pair_place's behind lw, (3) behind the records in
    // sval / srow.  They are enough from one plane to the next: plane m + 1 writes shx / shy behind barrier 3 of plane m, so behind
    // every lane's reads of them (lower(), in front of barrier 2); it writes lw behind its own barrier 1, so behind every lane's
    // reads of lw (pair_place, in front of barrier 3 of plane m); it writes sval / srow behind its own barrier 2, so behind every
    // lane's pair_store of plane m (in front of barrier 1 of plane m + 1).  The returns are the workgroup's: s, the table words and
    // pl.total are the same in every lane.
#pragma nounroll
    for (int m = 0;;) {
        const u64 dst = esp_uniform_u64(pred[s]);
        const u64 dst_next = esp_uniform_u64(pred[s + 1]);
        const u64 hi = ((u64)s << (a.rem_bits + 1)) + a.base;  // the pair's prefix: that of its first bucket
        // ---- the column's run, folded as it is formed: row q of the seven (rows strictly increasing where they exist)
        bool present[G_ROWS];
        double acc[G_ROWS];
        u32 row[G_ROWS];
#pragma unroll
        for (int q = 0; q < G_ROWS; q++) present[q] = false, acc[q] = 0.0, row[q] = 0u;
        // the node's own pairs first; the x and y ones go through LDS to the lanes whose columns they end in.  The barrier stands
        // outside `has`: every lane of a workgroup that got past the uniform returns reaches it.
        const double z_below = c.vhi[2];  // (the plane below's z pair, in front of upper() forming this plane's)
        if (has) {
            src.upper(k, zg, c);
            shx[t] = c.vhi[0];
            shy[t] = c.vhi[1];
        }
        __syncthreads();
        if (has) {
            src.lower(k, zg, t, shx, shy, m == 0, z_below, c);
#pragma unroll
            for (int q = 0; q < 3; q++) row[q] = l - (u32)c.stride[q], row[4 + q] = l + (u32)c.stride[2 - q];
            row[3] = l;
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
        // ---- one plane up: the pair s_step further, k + 1, the counter a constant further
        if (!MARCH || ++m >= a.march) return;
        s += s_step;
        if (s >= a.S) return;  // (the last chunk of an nz that is no multiple of the march)
        if (has) l += (u32)c.stride[0], zg = src.next_plane(zg, c);
    }
}

// ---- the march length: the one place that decides it
// The automatic rule as a pure function of the grid, the cut and the device.  A grid conforms when a plane is a whole number of
// pairs (nx ny % ncl == 0); P = nx ny / ncl pairs then make a plane, pair s + P holds lane for lane the (i, j) of pair s one
// plane up, and every pair is full.  A longer march saves more of what a thread forms once and more z draws ((L - 1) / L of
// them), but it leaves fewer and longer workgroups, and a launch ends with a round of workgroups that fills the device only in
// part.  Measured at 256^3 on 256 compute units (NOTES/round22.md; R = 1024 workgroups at once, four per compute unit: the LDS
// bounds them): 3 planes (10.75 rounds of R) beat the parent by 3 %; 2 planes (16 rounds) lost 1 to 4 %, 5, 6 and 8 planes (6.5,
// 5.4 and 4 rounds) lost 10 %, 4 planes (8 rounds) went either way from run to run -- a round count just above a whole number
// pays for a whole round more.  So the rule marches only what a run backs: MARCH_PLANES planes, where that leaves at least the
// measured 10.75 rounds and where the planes a slot of the device works through, L ceil(W / R + 1/4) with W = P ceil(nz / L)
// workgroups (the quarter: workgroups drift apart, an exact fit does not stay one), are at most 33 / 32 of what one plane per
// workgroup has -- 33 against 32 was the measured gain.  Everything else runs one plane per workgroup.
namespace {
constexpr int MARCH_PLANES = 3;
constexpr i64 MARCH_RESIDENT_PER_CU = 4;
constexpr i64 MARCH_ROUNDS_X4 = 43;  // 10.75 rounds
i64 march_pairs_per_plane(i64 nx, i64 ny, int cl_bits) {  // P, or 0 for a grid that does not conform
    if (nx < 1 || ny < 1 || cl_bits < 0 || (2 << cl_bits) > THREADS) return 0;
    const i64 ncl = (i64)2 << cl_bits, nxny = nx * ny;
    return nxny % ncl == 0 ? nxny / ncl : 0;
}
}  // namespace

int pair_gen_march_rule(i64 nx, i64 ny, i64 nz, int cl_bits, int compute_units) {
    const i64 P = march_pairs_per_plane(nx, ny, cl_bits);
    if (P == 0 || nz < MARCH_PLANES) return 1;
    const i64 R = MARCH_RESIDENT_PER_CU * (i64)std::max(compute_units, 1);
    auto workgroups = [&](i64 L) { return P * ((nz + L - 1) / L); };
    auto planes_per_slot = [&](i64 L) { return L * ((4 * workgroups(L) + R + 4 * R - 1) / (4 * R)); };  // L ceil(W / R + 1/4)
    const i64 L = MARCH_PLANES;
    return 4 * workgroups(L) >= MARCH_ROUNDS_X4 * R && planes_per_slot(L) * 32 <= planes_per_slot(1) * 33 ? (int)L : 1;
}

// The march of one fused flush: 1 unless the grid conforms, the flush starts at column 0, covers the whole grid and its pairs are
// exactly the grid's (a.S = P nz, so a marching workgroup's pairs are all in the table and all full); then `force` (clamped to
// nz) or the rule.  a.S is the number of pairs.
static int pair_gen_march(const Args &a, const espgen::FdArgs &fd, int compute_units, int force) {
    const i64 P = march_pairs_per_plane(fd.nx, fd.ny, a.cl_bits);
    if (P == 0 || fd.nz < 1 || a.rb >= 32 || (a.base >> a.rb) != 0 || a.col_end != fd.nx * fd.ny * fd.nz || (i64)a.S != P * fd.nz || P > 0x7fffffff)
        return 1;
    if (force > 0) return (int)std::min<i64>(force, fd.nz);
    return pair_gen_march_rule(fd.nx, fd.ny, fd.nz, a.cl_bits, compute_units);
}

// ... written into the argument block (a.march, a.march_step); returns the workgroups of the flush: the pairs, or (pairs of a
// plane) x (chunks of `march` planes) -- the unit of a.first and of a launch's grid
i64 pair_gen_set_march(Args &a, const espgen::FdArgs &fd, int compute_units, int force) {
    a.march = pair_gen_march(a, fd, compute_units, force);
    a.march_step = 0;
    if (a.march <= 1) return (i64)a.S;
    const i64 P = march_pairs_per_plane(fd.nx, fd.ny, a.cl_bits);
    a.march_step = (int)P;
    return P * ((fd.nz + a.march - 1) / a.march);
}

bool launch_pair_gen_predicted(const Variant &v, unsigned grid, hipStream_t stream, const Args &a, const espgen::FdArgs &fd, const u64 *pred,
                               u64 out_cap, bool keep) {
    // (whole columns, at most 512 of them per pair, rows that fit the records' 32 bits)
    if (!v.fresh || v.pieces || a.cl_bits < 0 || (2 << a.cl_bits) > THREADS || a.rb >= 32 || !a.colptr_out || !a.host_words) return false;
    // (FdSource: the division.  Other spacings are not the fused kernel's: the caller serves the flush unfused)
    auto mid = [](double h) { return h >= 0x1.0p-100 && h <= 0x1.0p100; };
    if (!(mid(fd.hx) && mid(fd.hy) && mid(fd.hz))) return false;
    // (a march is pair_gen_set_march's or none: the kernel's mapping holds for a grid that conforms only)
    if (a.march > 1 && (a.march != pair_gen_march(a, fd, 0, a.march) || (i64)a.march_step != march_pairs_per_plane(fd.nx, fd.ny, a.cl_bits)))
        return false;
    auto go = [&](auto M) {
        using Src = FdSource<decltype(M)::value>;
        const Src src{fd.nx, fd.ny, fd.nz, fd.hx, fd.hy, fd.hz, fd.seed, fd.fast, fd.magic_nx, fd.magic_nxny,
                      {6ull * (u64)(fd.nx * fd.ny) * ESP_GOLDEN, 6ull * (u64)fd.nx * ESP_GOLDEN, 6ull * ESP_GOLDEN}};
        return pair_for_keys(v.keys, [&](auto K) {
            constexpr int KEYS = decltype(K)::value;
            auto run = [&](auto KP, auto MA) {
                hipLaunchKernelGGL((pair_gen_pred_k<KEYS, Src, decltype(KP)::value, decltype(MA)::value>), dim3(grid), dim3(THREADS), 0, stream, a,
                                   src, pred, out_cap);
            };
            const bool march = a.march > 1;
            if (keep && march) run(std::true_type{}, std::true_type{});
            else if (keep) run(std::true_type{}, std::false_type{});
            else if (march) run(std::false_type{}, std::true_type{});
            else run(std::false_type{}, std::false_type{});
        });
    };
    // (the mode as the generator reads it: 0, 1, anything else)
    if (fd.rand_mode == 0) return go(std::integral_constant<int, 0>{});
    if (fd.rand_mode == 1) return go(std::integral_constant<int, 1>{});
    return go(std::integral_constant<int, 2>{});
}

}  // namespace esplocal
