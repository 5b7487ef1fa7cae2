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
// records only (512 x 7 x 12 B = 42 KiB: three workgroups per CU).  The updates go through espfold::fold_step_update /
// fold_step_sel as they are formed; from "entries the run emits" on the kernel calls the functions pair_pred_k calls (pair.hpp):
// pair_place scans the emitted counts, pair_table_hit is the check against the table -- a miss stores nothing --, pair_store
// the coalesced rowval / nzval stores and the lane's colptr, pair_grand_total the granule of the grand total.  Its own: the
// grand total and a miss (PRED_MISS) go to pinned host memory (Args::host_words).  No ticket, no look-back, nothing that waits
// for another workgroup, no memset in front of the launch and no copy behind it.
//
// A step that repeats the last one's structure stores the values alone (the template parameter KEEP, esp_handle::KeptStructure):
// colptr and rowval -- 8 Z + 8 (N + 1) of the 16 Z + 8 (N + 1) bytes -- already lie where the handle's last fused flush wrote them.
// The kernel was store-limited (393 us at 256^3, 273 without the rowval store; NOTES/round16.md); the KEEP form needs no rows in
// LDS (28 KiB: four workgroups per CU) and takes 226 us.
//
// Where the values come from is the template parameter SRC (FdSource: the built-in generator's draws, the expressions and the
// operation order of espgen::fdrand_part_k -- compiled without FMA contraction like every unit); a source that reads edge
// coefficients from a caller's arrays fills the same StencilColumn.
#include "generators.hpp"
#include "local.hpp"
#include "pair.hpp"

namespace esplocal {

namespace {
constexpr int G_ROWS = 7;                  // rows a column of the 7-point stencil can hold
constexpr int G_CAP = THREADS * G_ROWS;    // records of a pair
}  // namespace

// What column l = g + 1 receives.  lo[q] / hi[q]: the pair towards l - stride[q] / l + stride[2 - q] exists (q = 0, 1, 2: the
// strides nx ny, nx, 1); v: the pair's value -- the off-diagonal update is -v, the diagonal one +v; b / vb: the node's boundary
// terms in x, y, z.
struct StencilColumn {
    i64 stride[3];
    bool lo[3], hi[3], b[3];
    double vlo[3], vhi[3], vb[3];
};

// f() where some active lane of the wave has `on` (a wave-uniform branch: no lane data crosses), else 0.0 -- a value nobody reads
template <class F>
__device__ __forceinline__ double draw_if(bool on, F f) {
    return __ballot(on) != 0 ? f() : 0.0;
}

// the built-in generator (espgen::FdArgs without the producer's tables)
struct FdSource {
    i64 nx, ny, nz;
    double hx, hy, hz;
    u64 seed;
    int rand_mode;
    int fast;
    u64 magic_nx, magic_nxny;
    u64 zsub[3];  // 6 d GOLDEN for d = nx ny, nx, 1 (wrapping u64, formed once on the host): draw 0 of node g - d has the counter z0(g) - zsub

    __device__ __forceinline__ void column(i64 g, StencilColumn &c) const {
        i64 i, j, k;
        espgen::fd_node(*this, g, &i, &j, &k);
        const i64 nxy = nx * ny;
        const int md = rand_mode;
        // draw q of node gg: counter 6 gg + q (espgen::fd_rand_z); z0(g - d) = z0(g) - 6 d GOLDEN exactly (the arithmetic wraps)
        const u64 zg = seed + (6ull * (u64)g + 1ull) * ESP_GOLDEN;
        c.stride[0] = nxy, c.stride[1] = nx, c.stride[2] = 1;
        c.lo[0] = k > 1, c.lo[1] = j > 1, c.lo[2] = i > 1;
        c.hi[0] = i < nx, c.hi[1] = j < ny, c.hi[2] = k < nz;
        c.b[0] = i == 1 || i == nx;
        c.b[1] = ny > 2 && (j == 1 || j == ny);
        c.b[2] = nz > 2 && (k == 1 || k == nz);
        // A lower neighbour's or a boundary draw is formed only where some lane of the wave uses it (the kernel's step() does
        // not look at a value whose flag is off: 0.0 stands there).  At 256^3 the y and z boundary draws are skipped in more than
        // 99 % of the waves, the x boundary draw in half of them.
        c.vlo[0] = draw_if(c.lo[0], [&] { return espgen::fd_rand_z(md, zg - zsub[0], 4) * hx * hy / hz; });
        c.vlo[1] = draw_if(c.lo[1], [&] { return espgen::fd_rand_z(md, zg - zsub[1], 2) * hx * hz / hy; });
        c.vlo[2] = draw_if(c.lo[2], [&] { return espgen::fd_rand_z(md, zg - zsub[2], 0) * hy * hz / hx; });
        c.vhi[0] = espgen::fd_rand_z(md, zg, 0) * hy * hz / hx;
        c.vb[0] = draw_if(c.b[0], [&] { return espgen::fd_rand_z(md, zg, 1) * hy * hz; });
        c.vhi[1] = espgen::fd_rand_z(md, zg, 2) * hx * hz / hy;
        c.vb[1] = draw_if(c.b[1], [&] { return espgen::fd_rand_z(md, zg, 3) * hx * hz; });
        c.vhi[2] = espgen::fd_rand_z(md, zg, 4) * hx * hy / hz;
        c.vb[2] = draw_if(c.b[2], [&] { return espgen::fd_rand_z(md, zg, 5) * hx * hy; });
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
    __shared__ u32 srow[KEEP ? 1 : G_CAP];  // the records' rows (1-based; not kept by the KEEP form) ...
    __shared__ double sval[G_CAP];          // ... and values
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
    if (has) {
        StencilColumn c;
        src.column(c_lo + t, c);
        const i64 l = c_lo + t + 1;
        auto step = [&](int q, bool on, double v) {
            if (!on) return;
            if constexpr (UPD)
                espfold::fold_step_update(present[q], acc[q], v);
            else
                espfold::fold_step_sel(present[q], acc[q], a.kind32, v);
        };
#pragma unroll
        for (int q = 0; q < 3; q++) {
            row[q] = (u32)(l - c.stride[q]);
            row[4 + q] = (u32)(l + c.stride[2 - q]);
            step(q, c.lo[q], -c.vlo[q]);
        }
        row[3] = (u32)l;
#pragma unroll
        for (int q = 0; q < 3; q++) step(3, c.lo[q], c.vlo[q]);
#pragma unroll
        for (int q = 0; q < 3; q++) {
            step(3, c.hi[q], c.vhi[q]);
            step(3, c.b[q], c.vb[q]);
        }
#pragma unroll
        for (int q = 0; q < 3; q++) step(4 + q, c.hi[q], -c.vhi[q]);
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
    const FdSource src{fd.nx, fd.ny, fd.nz, fd.hx, fd.hy, fd.hz, fd.seed, fd.rand_mode, fd.fast, fd.magic_nx, fd.magic_nxny,
                       {6ull * (u64)(fd.nx * fd.ny) * ESP_GOLDEN, 6ull * (u64)fd.nx * ESP_GOLDEN, 6ull * ESP_GOLDEN}};
    return pair_for_keys(v.keys, [&](auto K) {
        constexpr int KEYS = decltype(K)::value;
        if (keep)
            hipLaunchKernelGGL((pair_gen_pred_k<KEYS, FdSource, true>), dim3(grid), dim3(THREADS), 0, stream, a, src, pred, out_cap);
        else
            hipLaunchKernelGGL((pair_gen_pred_k<KEYS, FdSource, false>), dim3(grid), dim3(THREADS), 0, stream, a, src, pred, out_cap);
    });
}

}  // namespace esplocal
