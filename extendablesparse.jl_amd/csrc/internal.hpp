// internal.hpp -- what the translation units of libesparse_hip share: the handle, the error / timing helpers, the plan
// and partition records, and the prototypes of the functions that cross file boundaries (hidden visibility: nothing
// of this is part of the C ABI, which is include/esparse_hip.h).
//   handle.hip     lifetime, buffers, append (esp_stage_begin / esp_commit / esp_append_*), CSC in and out, timing, debug;
//                  the readouts into a caller's host or device array (copy_out, export_u32_as_i64)
//   produce.hip    device-side producers (esp_generate_*): plain, producer-side partition (run lists), item partition
//   partition.hip  the plan (prefix bits, back-off), radix passes, run-based single pass, sort_msd;
//                  sort_segment_lsd, the one driver of every single-segment LSD sort (pending buffer, run list, tail, rows, levels, colours)
//   flush.hip      esp_flush: bucket kernel launch, join with a stored CSC, batch + tail, general path
//   shard.hip      column shards (esp_shard_*) and the group API (group.hpp: exchange policy + RCCL transport)
//   consumers.hip  what reads or edits the assembled CSC: getindex, dropzeros, pattern hash, mul!, Dirichlet, Jacobi / ILU0
//   precon.hip     the point preconditioners' update! / ldiv! (esp_precon_*) and simple! (esp_simple) on the device CSC
//   iluam.hip      ILUAMPreconditioner: level analysis, level-scheduled ILU(0) factorization and triangular solves
//   derived.hip    what the kinds that hold a derived matrix share (Block, Colored, ILU(k)): the update! cycle, the value gather, the
//                  stream hand-over; ScratchFlush, the sort by an ESP_COO flush of a scratch handle (also esp_transpose, esp_matmul)
//   block.hip      BlockPreconditioner: the masked block matrix B of a partitioning (identity / permuted path) and the object around it
//   color.hip      the multicolour ordering: graph colouring by rounds over a fixed hash (esp_graph_coloring), the permutation by
//                  (colour, index), ColoredPreconditioner = block.hip's permuted path over that one partition
//   spai.hip       SPAIPreconditioner: the sparse approximate inverses SPAI-0 and SPAI-1 (size pass, one wave / one workgroup per
//                  column: sorted row union, dense gather, modified Gram-Schmidt in LDS), M in an internal handle, ldiv! = esp_mul's gather
//   iluk.hip       ILUKPreconditioner: the level-of-fill pattern by one bounded search per column (wave / workgroup form), the filled
//                  matrix B in an internal handle, ILUAM on it
//   lu.hip         LUFactorization: the nested-dissection ordering by level-synchronous component and search launches, the supernodal
//                  symbolic fill from the dissection tree, the filled reordered matrix B with ILUAM as the inner kind
//   lu_panels.hip  LUFactorization's panel form: ILUAM's chains over B on two dense panels per tree node (panels.hpp: the tables it
//                  shares with cholesky.hip), the solves in ILUAM's orders
//   cholesky.hip   CholeskyFactorization: lu.hip's ordering and tree (lu.hpp), dense column-major panels per node, the numeric
//                  factorization and the solves depth by depth (small form: a workgroup per node; wide form: tiles over the grid)
//   ilut.hip       ILUTPreconditioner: the threshold ILU by synchronous sweeps (wave / workgroup / stride tiers of the sweep kernel),
//                  the candidate pattern from esp_matmul, drop and compaction, F in an internal handle, ILUAM's prefactored mode on it
//   amg.hip        AMGPreconditioner: smoothed aggregation (MIS(2) aggregates by Luby rounds, the level hierarchy from the algebra
//                  calls on internal handles, the fused V-cycle kernels); amg.hpp holds what it shares with rsamg.hip
//   rsamg.hip      RS_AMGPreconditioner's coarsening: row-wise strength, the PMIS splitting, direct interpolation (the rest is amg.hip's)
//   krylov.hip     preconditioned conjugate gradients (esp_cg): fused vector kernels, ordered dot products, scalars on the device
//   krylov_many.hip  conjugate gradients for several right-hand sides (esp_cg_many): k independent recurrences in lockstep, 8
//                  columns a launch behind a live mask; the many-column forms of Jacobi's and ILU0's ldiv!
//   bicgstabl.hip  BiCGStab(l) for non-symmetric systems (esp_bicgstabl): the same design with l+1 residuals and search vectors;
//                  krylov.hpp holds what the solvers share: the summation shape's kernels, the preconditioned product
//                  (PreconProduct) and the hand-over of host b / x
//   gmres.hip      restarted GMRES (esp_gmres): fused modified Gram-Schmidt steps, batched classical / DGKS passes behind a device
//                  predicate, H, the residual recurrence, the rotations and y in a scalar block on the device; gmres.hpp holds the
//                  bodies of its kernels
//   gmres_many.hip   restarted GMRES for several right-hand sides (esp_gmres_many): gmres.hpp's bodies per column, the columns on
//                  gridDim.y behind a live mask; krylov_many.hpp holds what it shares with krylov_many.hip
//   matops.hip     the algebra of assembled matrices on the device: A*B (esp_matmul), A+B / A-B (esp_add), Diagonal scaling
//   linalg.hip     transpose (esp_transpose), transpose(A)*x (esp_mul_transpose), issymmetric, opnorm, norm on the device CSC
//   local_*.hip    the instantiations of the bucket kernel (local.hpp; local_h.hip: group3.hpp, the group tier with three workgroups per CU;
//                  local_j.hip: group3_items.hpp, the same fed with the item records of an element-level batch;
//                  local_w.hip: pair_k, the small variant's form with two producer buckets per workgroup)
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <cmath>
#include <thread>

#include "common.hpp"
#include "fold.hpp"
#include "generators.hpp"
#include "femitems.hpp"
#include "elements.hpp"
#include "local_args.hpp"
#include "merge.hpp"
#include "radix.hpp"
#include "runpart.hpp"
#include "scan.hpp"


// ------------------------------------------------------------------------ handle
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct TimedSpan {
    int stage;
    hipEvent_t a, b;
    int launches;
};

struct esp_handle {
    i64 m = 0, n = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    KeyLayout L{1, 1};
    std::string err;

    // COO append buffer
    DevBuf keys, vals;
    i64 cap = 0, count = 0;
    // ping-pong / scratch
    DevBuf keys2, vals2, hist, segs, colend, newkey, newval, heads, misc, seg[2], tilef[2], segcnt, segout, tseg, ttile;
    int force_path = 0, last_path = 0;
    DevBuf runbuf, chunkbuf;
    i64 chunk_cap = 0, hint = 0;
    int chunk_pb = 0;
    int runs_skip = 0, runs_penalty = 0;  // back-off after a stream turned out not to be pre-sorted
    bool g3_off = false;                  // a segment of this handle's matrix did not fit the three-workgroup group kernel: not tried again
    bool pair_off = false;                // ... a pair of buckets did not fit the small variant's pair form (pair_k): not tried again
    int last_cl_bits = -1, last_buckets = 0;  // the cut the last flush's bucket kernel worked on (esp_debug_last_bucket_cut)
    int last_pair = 0;                    // the last flush's bucket kernel was pair_k (esp_debug_last_bucket_pairs)
    bool hits_off = false;                // the re-assembly form of the group kernel met a batch that was no re-assembly of the stored pattern: not tried again (until reset!)
    bool g3_wide = false;                 // ... for its rows alone (spread over more than 2^18): the kernel's wide form serves this handle
    bool debug_fail_bucket = false;       // esp_debug_fail_next_bucket_stage (test hook, one shot)
    i64 debug_chol_wide = 0;              // esp_debug_cholesky_wide_from: the width from which CholeskyFactorization uses its wide form (test hook; 0: the default)
    i64 debug_lu_wide = 0;                // esp_debug_lu_wide_from: the same for LUFactorization's panel form
    i64 debug_lu_cap = 0;                 // esp_debug_lu_fill_cap: LUFactorization refuses nnz(B) >= this (test hook; 0: the 32-bit limit)
    double debug_plan_cap = 0.0;          // esp_debug_plan_cap: plan as if the bucket kernel took segments of this many entries (test hook)
    int last_group3 = 0;                  // the last flush's bucket kernel was group3_k (esp_debug_last_local_small reports 2)
    bool seen_hits = true;                // the last flush over a stored pattern mostly hit stored positions (re-assembly)
    int seen_maxrun = 0;                  // longest column run the bucket kernel met in the last flush
    int last_partition = 0;               // 1 = run-based single pass, 2 = 8-bit passes only, 4 = the producer's, 7 = shard pieces
    // Producer-side partition: a device-side producer appended to the empty buffer with its PART kernel (runpart.hpp,
    // "the append IS the partition"): the pending entries lie bucket by bucket -- a stable permutation of the stream --
    // and the flush starts at the bucket kernel.  Bucket starts: seg[1] (S + 1 entries).
    struct PrePart {
        bool valid = false;
        int K = 0, pb = 0;       // bits of the key window / of the prefix: S = 1 << pb buckets
        int key_bytes = 8;       // 4: `keys` holds u32 keys (the bits below the prefix); every entry has the kind `kind`
        int kind = 0;
        i64 E = 0, maxlen = 0;   // entries, longest bucket
        // FINE partition (round 6): the plan has `fb` more prefix bits than the bucket kernel needs, so that the bits below the
        // prefix fit 4-byte keys (322^3: 33 bits below the planned prefix; 400^3: 34); the flush's bucket kernel takes 2^fb
        // neighbouring buckets as ONE segment (maxlen_c: the longest of those) and tells an entry's bucket by its position.
        // To everybody else the batch is what its fine plan says: 2^pb buckets of 4-byte keys.
        int fb = 0;
        i64 maxlen_c = 0;
        i64 tail = 0;            // packed entries appended BEHIND the E bucket-ordered ones (count = E + tail)
        u64 base = 0, span = 0;  // the key window it was made for
        double Ee = 0.0;         // (plan_entries of the batch: spread bookkeeping)
        // column shards: the batch was partitioned by (owner, digit inside the owner's column range) -- what
        // esp_shard_partition produces; mw_P windows of mw_nb digits, digit width 2^mw_shift, plan made for mw_eps
        int mw_P = 0, mw_me = 0, mw_shift = 0;
        u32 mw_nb = 0;
        i64 mw_eps = 0;
        bool own32 = false;      // ... and the shard's OWN range holds 4-byte keys of kind `kind` (the sent ranges: packed)
        u64 plan_id = 0;         // ... the table build it came from (prepart_finish numbers them; a reused plan keeps its number)
    } pre;
    u64 plan_counter = 0;
    // esp_shard_partition over a producer's batch whose plan was REUSED: the owner ranges and per-digit counts are those of the
    // call that built the tables -- kept, so that nothing runs beside the PART launch (a second queue with three tiny operations
    // cost that launch 90 us of 500: NOTES/round6.md section 7)
    struct ShardOffsets {
        u64 plan_id = 0;
        int P = 0, me = 0;
        i64 eps = 0, NB = 0, E = 0;
        const void *cnt_at = nullptr;
        std::vector<i64> off;
    } shard_offsets;
    bool pre_keep = false;       // reserve_append: the append that follows goes behind the bucket-ordered batch
    // A batch of an item partition whose EXPANSION has not run (group3_items.hpp): `pre` describes it as if its updates lay
    // bucket by bucket in keys / vals -- they do not yet: the sorted item records lie in the keys array (the two ping-pong
    // halves of the item passes), the cell records of an element-level append in the vals array, and the flush's bucket
    // kernel forms the updates itself (fresh matrix, nothing appended behind the batch).  Everybody else -- an append behind
    // the batch, a clone, getindex, a shard call, a flush over a stored pattern, a segment the fused kernel refuses -- calls
    // lazy_expand() first (pending_materialize and reserve_append do), which runs the expansion kernel into the scratch pair,
    // swaps the pairs and leaves the handle as a producer-side partition always left it.  on implies pre.valid.
    struct LazyItems {
        bool on = false;
        bool armed = false;      // set by the item partition; the producer turns it into `on` beside pre.valid = true (after pending_changed)
        int src = 0;             // 1: the built-in generator's items (espitem), 2: an element-level append's (espelem)
        bool k32 = true;         // the expansion writes 4-byte keys (pre.key_bytes == 4)
        espitem::Args it;        // the expansion's argument block (sorted_keys set; keys_out / vals_out filled in by lazy_expand)
        espelem::Args el;
    } lazy;
    DevBuf lazy_hold;            // esp_append_elements_host: the uploaded element matrices of a batch that stayed a list of items (the fused
                                 // bucket kernel or lazy_expand gathers from them); released by the next flush / reset / upload
    // The stencil generator's counterpart (round 13): a full-range batch that repeats the handle's last plan (GenPlan) on a fresh
    // matrix whose last flush of that plan left its offset table (PredTable) is not written at all -- the PART launch is held
    // back, `pre` describes the batch as E entries lying bucket by bucket, and the flush's fused pair kernel (pair_gen_pred_k,
    // local_x.hip) forms every column's updates itself.  Everybody else calls lazy_expand() first, which issues the PART launch
    // with the arguments kept here and finds the handle as it always was.  on implies pre.valid; gen: the plan it was armed
    // under (whatever rewrites the plan's tables expands or drops the descriptor first -- lazy_expand refuses a stale one).
    struct LazyStencil {
        bool on = false;
        bool armed = false;      // set in the generator call; turned into `on` beside pre.valid = true (after pending_changed)
        u64 gen = 0;
        unsigned grid = 0;       // workgroups of the PART launch
        espgen::FdArgs a;        // its argument block (part = GenPlan::out; the output arrays are filled in by lazy_expand)
    } lazyst;
    int last_lazy_stencil = 0;   // esp_debug_last_lazy_stencil: 0 not armed, 1 the fused kernel served the flush, 2 armed, then expanded
    // The structure a served fused flush wrote stays where it is (round 16).  A time loop over a fixed grid has new values every
    // step and the same pattern: when the next fused flush of the same plan, table, grid and kind finds colptr and rowval as that
    // flush left them, the kernel's KEEP form stores the values alone -- 8 Z of the step's 16 Z + 8 (N + 1) bytes.
    // Why the table's `hit` test proves the patterns equal: every step's pattern is a subset of the grid's structural pattern S
    // (an update whose value folds to "not present" drops an entry and can never add one).  The stamp is armed only behind a
    // flush P0 that hit the table in every pair with |P0| = |S|, so P0 = S and every pair's table count is its structural count;
    // a step P1 that hits the table in every pair then has S's count in every pair, and a subset of S with S's count is S.
    // The stamp describes what the buffers physically HOLD, so whatever may write colptr or rowval, or move them, drops it
    // (drop_kept below): esp_flush on entry (only the served fused branch arms it again), ensure / release_all, the fills of
    // colptr, esp_set_csc, the CSC editors, results installed into a handle, clones, shard calls.  Three conditions are checked
    // where it is used as well: the three pointers, that the pattern version is the one the handle's last reset! made from the
    // stamp's (whoever changes the pattern moves it), and that the lazy fill of colptr reset! left is still pending.
    struct KeptStructure {
        bool valid = false;
        bool candidate = false;  // esp_flush moved `valid` here on entry: what its fused branch may use
        u64 plan_gen = 0, pred_gen = 0;
        i64 nx = 0, ny = 0, nz = 0;
        int keys = 0;            // the kind instantiation (1 / 2)
        const void *rowval = nullptr, *colptr = nullptr, *nzval = nullptr;
        i64 nnz = 0;
        unsigned long long pattern_version = 0;
    } kept;
    int last_kept = 0;           // esp_debug_last_kept_structure: 0 stored everything, 1 kept, 2 the kept form missed and the retry rewrote everything
    int last_march = 0;          // esp_debug_last_march: planes per workgroup of the last flush's fused launch (0: not fused)
    int force_march = 0;         // esp_debug_force_march: 0 automatic, else the march of every grid that conforms (clamped to nz)
    int compute_units = 0;       // of the handle's device (esp_create): what the march rule sizes its workgroup count by
    int last_rebuild = 0;        // the last flush's tail rebuilt the matrix (flush_rebuild: the stored CSC as the first piece of a fresh flush)
    int last_lazy_items = 0;     // the last flush's bucket kernel formed its updates from item records (esp_debug_last_lazy_items)
    int last_sum_join = 0;     // esp_debug_last_sum_join
    int last_sum_plan_bits[2] = {0, 0};  // esp_debug_last_sum_plan_bits: smallest / largest prefix the buffers of the last joint esp_flush_sum had planned
    double last_sum_ms[2] = {0.0, 0.0};  // esp_debug_last_sum_ms: host wall-clock of the last esp_flush_sum's folds / gather + combine flush
    // The entries appended behind a batch over a STORED pattern were partitioned as they came (append_tail_partitioned):
    // pre.tail packed keys in bucket order of a plan of their own -- still a pending stream like any other (a stable
    // partition keeps every column's order), so whoever does not know about it loses nothing; esp_flush's split
    // starts their flush at the bucket kernel.  Segment starts in tseg.
    struct TailPart {
        bool valid = false;
        int K = 0, pb = 0;
        i64 T = 0, maxlen = 0;
        u64 base = 0, span = 0;
    } tailpart;
    // A caller that repeats its stream (a time-stepping code: the same triplets' positions every step): the run lists,
    // run offsets and bucket starts of the last append-is-the-partition of caller-supplied triplets (append_partitioned)
    // serve the next one -- no count pass over the columns; the scatter kernel checks every tile against its run list
    // and a stream that is not the same falls back to the full path.  Dropped by whatever rewrites the tables.
    struct RawPlan {
        bool valid = false;
        i64 count = 0, chunks = 0, maxlen = 0, maxlen_c = 0;
        int kind = 0, K = 0, pb = 0, key_bytes = 8, fb = 0;
        u64 base = 0, span = 0;
        double Ee = 0.0;
    } rawplan;
    // The same for the stencil generator (esp_generate_fdrand*): its run lists, run offsets and bucket starts are a function of
    // the grid, the node range and the plan alone -- not of seed, values or kind -- so an assembly that repeats the previous
    // one (a time loop: reset!, fdrand!, flush!) goes straight to the PART launch: no COUNT launch, no ranking launches, no
    // host round trip for their flags.  Dropped by whatever rewrites the tables (chunk_arrays, sort_msd, release_buffers).
    // A caller's triplets of one kind on an empty buffer that are NOT a pre-sorted stream (a shuffled assembly): the first radix
    // pass of their flush ran while they were appended (append_first_pass: keys formed from rows / cols on the fly, values read
    // where the caller holds them -- no packed copy in stream order is written and read again).  The buffer holds packed keys in
    // the order of that pass -- a stable permutation of the stream: to everybody who does not know, an ordinary pending buffer --
    // and sort_msd resumes behind it (segment / tile tables in seg[cur] / tilef[cur]).  Dropped by pending_changed.
    struct PrePass {
        bool valid = false;
        i64 count = 0, maxlen = 0;
        int K = 0, planned = 0, npass = 0, bits0 = 0, cur = 0, S = 0;
        u64 base = 0, span = 0;
        double Ee = 0.0;
    } prepass;
    struct GenPlan {
        bool valid = false;
        i64 nx = 0, ny = 0, nz = 0, g0 = 0, g1 = 0, E = 0;
        int kind = 0;
        u64 base = 0, span = 0;
        const void *keys_at = nullptr;  // (the arrays the stored PartOut wrote to: a reallocation drops the plan)
        esprun::PartOut out;
        PrePart pre;
    } genplan;
    // Both plans above say that the next batch is cut into the same buckets as the last one.  What the bucket kernel's pair form
    // (local_w.hip) resolves by look-back -- where every pair of buckets starts in the output -- then repeats as well unless
    // structural zeros move: the offsets the last look-back flush of the plan found are kept (one tiny launch over the fresh
    // colptr) and the next flush of the same plan runs the kernel's PREDICTED form on them, which checks every pair's count
    // and stores nothing where it differs; the flush then runs again with the look-back kernel and records anew.
    // plan_gen numbers the plans: it moves wherever genplan / rawplan is made or dropped (plan_made / drop_*_plan below).
    u64 plan_gen = 1;
    struct PredTable {
        DevBuf tab;          // Sp + 1 offsets (u64): pair s writes [tab[s], tab[s + 1])
        u64 gen = 0;         // the plan it belongs to (0: none)
        int S = 0;           // buckets of that flush (Sp = (S + 1) / 2 pairs)
        int misses = 0;      // flushes in a row whose prediction missed; 2: not tried again until the plan changes
        int last = 0;        // esp_debug_last_predicted: 0 not tried, 1 served, 2 tried and missed
    } pred;
    // esp_elements_keep_plan: the item order, the cell records and the segment table of the last esp_append_elements on an
    // empty buffer (cells of 3 / 4 nodes) are kept in buffers of their own, so that esp_append_elements_again -- the same
    // connectivity, new element matrices: a time step of an instationary / nonlinear code -- goes straight to the expansion
    struct ElemPlan {
        bool keep = false, valid = false;
        int nloc = 0, W = 0, vrb = 0, rem_real = 0, K = 0, kind = 0;
        bool k32 = false, has_diag = false;
        i64 ncells = 0, S = 0, maxlen = 0;
        u64 base = 0, span = 0;
        DevBuf sorted, cellrec, segtab;
    } elemplan;
    // sort_msd over ITEM records (femitems.hpp): a segment may hold plan_cap records (the bucket kernel's capacity in
    // updates / updates per item), and a shuffled stream need not be tried as a pre-sorted one
    i64 plan_cap = 0;
    bool plan_try_runs = false;  // item records of an element batch whose cell order looked pre-sorted to elem_cells_k: sort_msd tries the run-based pass
    u64 plan_occ_span = 0;       // > 0: the records to partition occupy only this many keys of the window (the columns one band of a mesh touches): the plan counts them as that dense
    int plan_bits = 0;           // > 0: sort_msd resolves exactly this many prefix bits in its planned passes (item partitions whose expansion does the last bits itself: segexpand.hpp)
    // the pending entries start at this entry of keys/vals (behind a batch that esp_flush flushed by itself); else 0
    i64 pend_off = 0;
    bool item_mode = false;
    bool item_keys_only = false;  // ... whose records are single words (the value arrays are not touched)
    bool shard_user = false;     // the handle is driven through esp_shard_*: its flushes partition by owner first
    int last_shard_source = 0;   // esp_shard_partition: 1 = its own pass moved the entries, 2 = the producer had
    int last_local_small = 0;    // the last flush's bucket kernel was the small variant (3 workgroups per CU)
    // esp_shard_plan: the producers that find the buffer empty partition for the next esp_shard_partition(P, me, eps)
    struct ShardPlan {
        bool valid = false;
        int P = 0, me = 0;
        i64 eps = 0;
    } shard_plan;
    // column window of the pending entries (whole matrix by default)
    u64 win_base = 0, win_span = 0;
    // A shard works on its column range only.  When the window [wc0, wc1) (0-based columns) was
    // declared on an empty matrix and kept since, no entry can lie outside it: the per-column work of a
    // flush (colend clear, colptr scan) then runs over the window only -- with P shards the global colptr
    // has P times the columns a shard owns.  colptr[c] = 1 for c <= wc0 always; the part behind the window
    // (= nnz+1) is rewritten only when somebody needs the whole array (tail_stale).
    i64 wc0 = 0, wc1 = 0;
    bool win_excl = false, tail_stale = false;
    // reset! of an unwindowed matrix leaves colptr := 1 to whoever reads it next (fix_tail): the fresh flush that
    // normally follows rewrites every entry
    bool ones_pending = false;
    // device CSC (Julia layout) + spare set for rebuilds
    DevBuf colptr, rowval, nzval, rowval2, nzval2;
    DevBuf colptr2;  // the join writes the new colptr here (its tiles hold both summands), then the two are swapped
    i64 nnz = 0;
    bool csc_valid = false;  // colptr initialised
    // host staging (pinned) + device staging
    // pinned staging areas (+ their device mirrors): `stage` is the one esp_stage_begin hands to the caller
    // (its pointers stay valid until the caller asks for a larger one); `bulk` is private to esp_append_host
    struct StageArea {
        i64 cap = 0;
        i64 *rows = nullptr, *cols = nullptr;
        double *vals = nullptr;
        uint8_t *kinds = nullptr;
        DevBuf d_rows, d_cols, d_vals, d_kinds;
    } stage, bulk;
    // esp_commit of a staged chunk: the chunk is packed on the host (keys + values) into one of two pinned halves and leaves
    // for the append buffer asynchronously -- the caller refills its chunk while the transfer runs
    struct CommitPack {
        i64 cap = 0;  // entries per half
        u64 *keys[2] = {nullptr, nullptr};
        double *vals[2] = {nullptr, nullptr};
        hipEvent_t done[2] = {nullptr, nullptr};
        bool busy[2] = {false, false};
        int next = 0;
    } cpack;
    // two pinned bounce buffers + their events for transfers between PAGEABLE host memory and the device (d2h_pipelined,
    // h2d_pipelined, the narrowed downloads): made on first use, nothing on the device side
    struct Bounce {
        char *pin[2] = {nullptr, nullptr};
        size_t bytes = 0;  // each
        hipEvent_t ev[2] = {nullptr, nullptr};
    } bounce;
    unsigned long long *pin_scalar = nullptr;  // pinned, 8 slots: the target of every small copy to the host
    // ... and, on a 64-byte line of their own behind them, the result words a flush's fused stencil kernel stores straight into
    // host memory (esplocal::Args::host_words: grand total | error bits | spare) -- never a copy target; pin_words_dev is the
    // address the device uses for them
    unsigned long long *pin_words = nullptr;
    unsigned long long *pin_words_dev = nullptr;
    // ... and behind those, 16 doubles of their own: the target of esp_gmres_many's read-back of a chunk (current and the pass count of
    // up to ESP_MANY_CHUNK columns), which would not fit the 8 slots of pin_scalar
    double *pin_many = nullptr;
    u64 *pin_mw = nullptr;  // pinned source of prepart_begin's asynchronous upload of the window bases (<= MW_MAX)
    hipEvent_t pin_mw_done = nullptr;
    // kind bookkeeping of the pending batch: when every pending entry was appended with ONE known kind the run-based
    // partition hands the bucket kernel 4-byte keys (the key bits below the partition prefix) instead of packed keys
    i64 kind_noted = 0;     // pending entries appended with a single known kind
    int kind_uniform = -1;  // that kind; -1 none yet, -2 mixed / an append of unknown kinds (until the buffer is empty again)
    int last_key_bytes = 8;      // esp_debug_last_key_bytes
    // longest segment / average segment of the last bucket-path flush (0: not known): an assembly that repeats on
    // a handle with regular data (spread ~1.0x) is planned one partition bit tighter when the predicted longest
    // segment still fits the bucket kernel -- half-full segments cost that kernel up to 1.8x
    double seen_spread = 0.0;
    int last_fold_update = 0;    // the register tiers of the last flush ran their UPDATE-only fold
    bool part_own32 = false;       // the own range of the partitioned buffer holds 4-byte keys (kind part_kind32)
    int part_kind32 = 0;
    bool part_own_update = false;  // esp_shard_partition: every pending entry was appended as an UPDATE
    bool part_all_update = false;  // esp_shard_assemble: ... and so is every received entry (checked on the device)
    int last_run_order = 0;      // esp_debug_last_run_order
    int last_plan_reused = 0;    // the last append-is-the-partition of caller triplets used the previous assembly's run lists
    int last_colptr_direct = 0;  // the bucket kernel of the last flush wrote colptr itself
    int last_append_route = 0;   // esp_debug_last_append_route: which kernels read the caller's arrays of the last device append
    hipStream_t aux = nullptr;   // second stream + event: small device-to-host reads beside a running kernel
    hipEvent_t aux_ev = nullptr;  // (created on first use, aux_ready)
    // shard cache
    bool shard_valid = false;
    int shard_P = 0;
    // partitioned exchange (esp_shard_partition / esp_shard_assemble)
    bool part_valid = false;      // the pending buffer is partitioned by (owner, digit); tables in parttab
    bool part_assembled = false;  // piece tables are built: the next flush runs the bucket kernel on them
    int part_P = 0, part_me = 0, part_shift = 0;
    u32 part_nb = 0;
    u64 part_base = 0, part_span = 0;
    i64 part_total = 0, part_maxlen = 0, part_own_lo = 0;
    int part_fb = 0;              // the own range came from a producer's FINE partition: 2^part_fb buckets of seg[1] per digit
    DevBuf parttab, piecetab;
    // esp_flush_sum's general path: the buffers' folds as ONE flush of a scratch handle with p n columns (buffer k's entries in the
    // columns [k n, (k + 1) n)); made on first use, destroyed with this handle
    esp_handle *sumtmp = nullptr;
    DevBuf sumrange;                       // ... the buffers' column ranges (device side of one round trip)
    int last_sum_batched = 0;              // the last esp_flush_sum folded its buffers in one flush of sumtmp
    DevBuf asmwork;                        // esp_shard_assemble's kernel: ticket | summary | per-workgroup partial results (zeroed once)
    unsigned long long *pin_asm = nullptr;  // ... and the pinned block its last workgroup writes the results to
    unsigned long long asm_seq = 0;
    // row-wise view of the device CSC for mul! (built on first use after a pattern change)
    unsigned long long pattern_version = 1, csr_version = 0;
    unsigned long long values_version = 1, csr_val_version = 0;  // nzval changed / row-wise copy of the values
    DevBuf csr_rowptr, csr_perm, csr_col, csr_tmp, csr_val, mul_x, mul_r;
    int matmul_tier = 0;   // esp_debug_matmul_tier: 0 automatic, 1 fused where it fits, 2 generic only (matops.hip)
    int transpose_path = 0;  // esp_debug_transpose_path: 0 automatic, 1 the ESP_COO flush, 2 the counting sort (linalg.hip)
    i64 last_transpose[3] = {0, 0, 0};  // esp_debug_last_transpose: path taken, columns listed for the workgroup sort, longest column
    int live_precons = 0;  // esp_precon objects bound to this handle (precon.hip): esp_destroy refuses while any is alive
    // esp_cg's work vectors (krylov.hip), sized on first use: residual, search direction, Pl \ r and A*u, the partial sums of the
    // three dot products, and the device copies of host b / x.  esp_bicgstabl (bicgstabl.hip) shares part, hb and hx and adds
    // bv: its 2(l+1) + 1 vectors (rs[0..l], us[0..l], the shadow residual), t: A*v in front of ILU0 / ILUAM, sc: the scalar block.
    // esp_gmres (gmres.hip) uses the same buffers: bv holds its restart+1 basis vectors, sc its H, nullvec, rhs, h, c and scalars.
    // krylov.hpp holds what the three share on the host side too: stage_vectors / return_x fill hb and hx and copy x back, and
    // PreconProduct issues every A*v, Pl \ v and Pl \ (A*v) of a solve (t is its scratch between the two).
    // esp_cg_many (krylov_many.hip) holds ESP_MANY_CHUNK columns in each of r, u, c, hb and hx (leading dimension n rounded up to
    // even) and the chunk's partial sums side by side in part; t is ILU0's pass-1 scratch there.
    // esp_gmres_many (gmres_many.hip): bv holds (restart+1) x ESP_MANY_CHUNK basis vectors, t one or two n x ESP_MANY_CHUNK blocks of
    // product scratch, sc ESP_MANY_CHUNK scalar blocks, part the chunk's partial sums and what the host reads back.
    struct Krylov {
        DevBuf r, u, c, part, hb, hx, bv, t, sc;
    } kry;
    // timing
    bool timing = false;
    int timing_level = 2;
    std::vector<hipEvent_t> ev_pool;
    std::vector<TimedSpan> spans;
    esp_timing_t acc;
    hipEvent_t flush_a = nullptr, flush_b = nullptr;
};

extern thread_local std::string g_err;

// a kept producer plan is made / dropped: the offsets kept for its flushes (esp_handle::PredTable) belong to no later plan
static inline void plan_made(esp_handle *h) { h->plan_gen++; }
static inline void drop_raw_plan(esp_handle *h) {
    if (h->rawplan.valid) h->plan_gen++;
    h->rawplan.valid = false;
}
static inline void drop_gen_plan(esp_handle *h) {
    if (h->genplan.valid) h->plan_gen++;
    h->genplan.valid = false;
}

// colptr / rowval may be written or moved: they are no longer known to hold what the last fused flush left (esp_handle::KeptStructure)
static inline void drop_kept(esp_handle *h) { h->kept.valid = h->kept.candidate = false; }

// the pending entries changed: whatever was derived from them is stale
static inline void pending_changed(esp_handle *h) {
    if (h->count == 0) {
        h->kind_noted = 0;
        h->kind_uniform = -1;
    } else if (h->kind_noted != h->count) {
        h->kind_uniform = -2;  // (some entries came or went without note_kind: sticky until the buffer is empty)
    }
    h->shard_valid = false;
    h->part_valid = false;
    h->part_assembled = false;
    // (whoever changes a bucket-ordered buffer called pending_materialize first -- or appends behind it)
    if (h->pre.valid && h->pre_keep && h->count >= h->pre.E)
        h->pre.tail = h->count - h->pre.E;
    else
        h->pre.valid = false, h->lazy.on = false, h->lazyst.on = false;
    h->prepass.valid = false;
    h->pre_keep = false;
    h->tailpart.valid = false;  // (append_tail_partitioned sets it after this call)
}

// set-up of a producer-side partition (prepart_* below, next to run_partition)
struct PartSetup {
    bool on = false;
    esprun::PartOut out;   // for the producer's PART kernel
    esprun::RunSink sink;  // for its COUNT kernel
    u32 *err = nullptr;    // window flag of the COUNT kernel
    int K = 0, pb = 0, kind = -1;
    int fb = 0;            // fine partition: pb holds fb bits more than the bucket kernel's segments need
    i64 E = 0, chunks = 0;
    double Ee = 0.0;
    i64 NB = 0;            // buckets (1 << pb, or shards * digits per shard)
    int mw_P = 0, mw_me = 0, mw_shift = 0;
    u32 mw_nb = 0;
    i64 mw_eps = 0;
    i64 *seg_out = nullptr, *runs_off = nullptr;
    const unsigned long long *bucket_count = nullptr;
    u64 *coarse = nullptr;
    const u32 *dcount = nullptr;
    const u64 *dlist = nullptr;
};

// call right before h->count grows by cnt entries that all carry `kind`
static inline void note_kind(esp_handle *h, int kind, i64 cnt) {
    if (h->count == 0 && h->kind_noted == 0 && h->kind_uniform == -1) h->kind_uniform = kind;
    else if (h->kind_uniform != kind) h->kind_uniform = -2;
    h->kind_noted += cnt;
}

#define FAIL(h, code, ...)                                   \
    do {                                                     \
        char _b[512];                                        \
        snprintf(_b, sizeof _b, __VA_ARGS__);                \
        if (h) (h)->err = _b;                                \
        g_err = _b;                                          \
        return (code);                                       \
    } while (0)

#define HIPCK(h, call)                                                                          \
    do {                                                                                        \
        hipError_t _e = (call);                                                                 \
        if (_e != hipSuccess)                                                                   \
            FAIL(h, _e == hipErrorOutOfMemory ? ESP_ERR_NOMEM : ESP_ERR_HIP, "%s failed: %s",   \
                 #call, hipGetErrorString(_e));                                                 \
    } while (0)

#define CK(...)                       \
    do {                              \
        int32_t _s = (__VA_ARGS__);   \
        if (_s != ESP_OK) return _s;  \
    } while (0)


// ---- records of the plan and the partition (partition.hip)
// ------------------------------------------------------------------------ flush
// MSD plan: partition on the top key bits until every segment fits the LDS bucket kernel.
// Returns local_ok=false when the general (global LSD + fold_k) path must be used instead.
struct Sorted {
    const u64 *sk;
    const double *sv;
    bool in_primary;  // data in h->keys/vals (true) or h->keys2/vals2 (false)
    int S;
    const i64 *seg_start;
    int rem_bits;
    bool local_ok;
    bool fits = false;  // every segment is within seg_cap (local_ok without the limit on the remaining key bits)
    bool all_update = false;  // PIECES: every entry of every piece is an UPDATE (esp_shard_assemble checked)
    int key_bytes = 8;  // 4: sk holds 32-bit keys (the bits below the prefix); every entry has the kind `kind`
    int fb = 0;         // 4-byte keys of a FINE partition: seg_start has (S << fb) + 1 entries, segment s = its buckets [s << fb, (s + 1) << fb)
    int k32_passes = 0;  // the 8-bit passes that wrote 4-byte keys (sort_msd): > 0 = the other pair holds no packed copy of the entries
    int kind = 0;
    i64 maxlen = esplocal::CAP;  // longest segment
    i64 total = -1;              // entries of all segments, if the caller knows (lets flush_local drop the segments behind the last column)
    int p32_piece = -1;          // PIECES: the piece that holds 4-byte keys of kind `kind` from position p32_lo on
    bool all32 = false;          // PIECES: EVERY piece holds 4-byte keys of kind `kind`
    i64 p32_lo = 0;
    // PIECES (partitioned shard exchange): segments are concatenations of per-source pieces
    int npieces = 0;
    const i64 *own_fine = nullptr;  // PIECES, fb > 0: the fine table of the piece p32_piece (local_args.hpp, Args::own_fine)
    bool pieces_dense = false;   // PIECES: most segments hold entries of several pieces (a batch and its tail, a stored slice and new entries)
    const i64 *pstart = nullptr;
    const void *const *ptab = nullptr;
    const esp_handle::LazyItems *lazy = nullptr;  // sk holds sorted ITEM records, seg_start counts their updates: the fused bucket kernel or nothing
    const esp_handle::LazyStencil *stencil = nullptr;  // sk / sv hold nothing yet: the fused predicted pair kernel (local_x.hip) or ESP_RETRY_EXPANDED
    bool no_pred = false;  // the flush comes back after a missed prediction of the fused kernel: the look-back form at once
    bool has_base = false;  // the segments' key base, if it is not the handle's window / shard range
    int expect_hits = -1;   // 1 / 0: the caller knows what the entries will mostly do over the stored pattern; -1: the handle's history
    u64 base = 0;
};

// ---- run lists of the pending entries (runpart.hpp) -------------------------------------------
// Persistent per-handle arrays: every chunk's runs, the digits' own run lists, the bucket totals.  They are
// filled by run_hist_k at flush time or by the COUNT launch of a producer whose append is the partition.
struct ChunkArrays {
    u32 *runs_d, *runs_c;
    u64 *nruns;
    unsigned long long *bucket_count;
    u32 *overflow;
    u32 *dcount;  // (directly in front of bucket_count: one memset clears both)
    u64 *dlist;
    u64 *coarse;  // totals of 256 digits each
    size_t clear_bytes;  // dcount .. bucket_count[NB]
};

// Single-pass partition on the top `pb` (9..20) bits of the key window, for pre-sorted streams
// (runpart.hpp).  *ok=false when some chunk holds too many distinct digits: nothing was moved and the
// caller uses the 8-bit passes.  On success kout/vout hold the partitioned entries, seg_out (NB+1
// entries, device) the bucket starts and tile_first_out the tile index of every bucket.
// several key windows side by side (column shards): see esprun::Args
struct MultiWin {
    int P;
    u32 nb;
    const u64 *d_base;
};

struct MwPlan {
    bool ok = false;
    int K = 0, shift = 0, pb = 0;
    u64 nb64 = 0;
    i64 NB = 0;
    // FINE partition of a producer's batch (33 .. 36 key bits below the plan's prefix -- the shards of 512^3 over 8 GPUs: 35): the
    // producer may cut every digit into 2^fb buckets (tables of NB << fb buckets, digit width 2^(shift - fb) = 2^32), so that its
    // OWN range holds 4-byte keys; the exchange, the piece tables and the bucket kernel's segments stay the plan's digits
    int fb = 0;
    std::vector<u64> base;
};

// mw != nullptr: buckets = mw->P * mw->nb (window r = digits [r*nb, (r+1)*nb)), pb = bits covering them
// triplets of one kind as the source of a partition (esprun::Args::raw_*)
struct RawSource {
    const i64 *rows, *cols;
    int kind, negate;
    unsigned long long *d_err;
};

// ---- the preconditioners (precon.hip, iluam.hip)
// One level schedule of ILUAM: the nodes (columns or rows) sorted by (level, index), the level offsets, and the launch
// list: a level wider than one workgroup is one launch of its own; consecutive levels that together fit one workgroup
// are one single-workgroup launch (thin = true) that separates them with __syncthreads().
struct IluamLaunch {
    u32 l0, l1;        // levels [l0, l1)
    u32 first, count;  // their members: order[first, first + count)
    bool thin;
};
struct IluamSched {
    DevBuf order, loff;  // u32 n / u32 levels + 1
    i64 levels = 0;
    std::vector<IluamLaunch> launches;
};
struct esp_precon {
    esp_handle *h = nullptr;
    int kind = 0;
    i64 n = 0, nnz = 0;
    unsigned long long pattern_version = 0;  // the pattern the split layout (and invdiag/xdiag) belongs to
    unsigned long long values_version = 0;   // the nzval the pre-scaled values were gathered from
    DevBuf diag;                             // invdiag (Jacobi) / xdiag (ILU0) / the diagonal of U (ILUAM), n
    DevBuf lptr, uptr;                       // n+1 each (u32)
    DevBuf lcol, ucol, lpos, upos;           // per part entry (u32)
    DevBuf dpos;                             // CSC position of every row's diagonal (u32, ILU0 / ILUAM)
    DevBuf lval, uval;                       // per part entry (f64; ILU0: pre-scaled, ILUAM: gathered from fval)
    DevBuf u1, res, partial, scanws, hv, hu; // scratch: pass-1 result, residual, sums of squares, scan, host staging
    // ILUAM: the factorization's own values (the reference's ILU.nzval, CSC position order) and the three schedules.
    // Its row parts (lptr .. lval / uptr .. uval) and diag lie in the SLOT order of the forward / backward schedule: entry
    // t belongs to row sched[1 / 2].order[t], so a level's slice is contiguous (8.3 against 11.2 ms per ldiv! at 256^3)
    DevBuf fval;
    IluamSched sched[3];  // 0: columns of the factorization, 1: rows of the forward solve, 2: rows of the backward solve
    int iluam_force = 0, iluam_form = 0;  // esp_debug_iluam_form's choice; the form of the last numeric factorization (0 none, 1 lane, 2 wave)
    // esp_precon_many_stats' layout: the most recent many-column solve (form, columns of the last chunk, the level launches
    // iluam_solve_many issued for it, chunks of the call).  A kind that holds a derived matrix keeps them on its inner preconditioner
    i64 many_stats[4] = {0, 0, 0, 0};
    // The kinds that hold a derived matrix (holds_derived: Block, Colored, ILU(k)): h is A; a matrix B made from A's stored CSC --
    // Block: the stored A[i,j] with part(i) == part(j); Colored: A[c,c]; ILU(k): every position of level <= iluk_k -- lives in the
    // internal handle bh (A's device and stream), and inner is an ordinary preconditioner of inner_kind bound to bh.  src[q] is the
    // position in A's nzval entry q of B came from (ILUK_FILL for a fill entry of ILU(k)): update! with the pattern kept is one gather
    // through it and inner's values-only update (derived_update, derived.hip).  rebuild: the next update! builds B anew whatever A's
    // versions say.
    struct Derived {
        esp_handle *bh = nullptr;
        esp_precon *inner = nullptr;
        int inner_kind = 0;
        bool rebuild = false;
        DevBuf src;  // u32 nnz(B)
    } der;
    // BlockPreconditioner (kind ESP_PRECON_BLOCK, block.hip): B is the block matrix.  blk_path 0 (every partition increasing): B keeps
    // A's numbering, ldiv! is inner's on the caller's vectors.  blk_path 1: B is renumbered by blk_new (position in the concatenated
    // partitions); ldiv! gathers into blk_t, solves into blk_s, scatters.
    int blk_path = 0, blk_force = 0;
    bool blk_increasing = false;
    DevBuf blk_new, blk_part;  // u32 n each: new(i), part(i)
    DevBuf blk_t, blk_s;       // f64 n each (permuted path)
    // AMGPreconditioner (kind ESP_PRECON_AMG, amg.hip): the parameters and the level hierarchy (internal handles of every A_l and
    // P_l, the weights, the cycle's vectors, the dense inverse of the coarsest level)
    struct AmgData *amg = nullptr;
    // ILUKPreconditioner (kind ESP_PRECON_ILUK, iluk.hip): B is the filled matrix -- A's bits where A stores an entry, +0.0 elsewhere --
    // and inner its ILUAM preconditioner (blk_path stays 0: ldiv! is inner's on the caller's vectors).
    int iluk_k = 0;
    esp_handle *iluk_th = nullptr;  // transpose(A), the graph of the search for the upper part
    DevBuf iluk_lev;                // i32 nnz(B): the level of every entry of B
    i64 iluk_stats[4] = {0, 0, 0, 0};  // nnz(B), largest stored level, columns redone by the workgroup search (L, U)
    // ColoredPreconditioner (kind ESP_PRECON_COLORED, color.hip): the multicolour ordering c of A's graph -- the vertices sorted by
    // (colour, index) -- is the one partition of a permuted-path block preconditioner: blk_new = the inverse of c, blk_part = 0
    // everywhere, B = A[c,c], inner ILU0 or ILUAM, blk_path = 1 (0 only for n == 0).  A pattern change of A re-colours before B is
    // rebuilt.
    DevBuf col_color, col_perm;      // u32 n each: the colour of every vertex (1-based, as the rounds number them), c
    std::vector<i64> col_ptr;        // ncolors + 1: colour r holds c[col_ptr[r] .. col_ptr[r + 1])
    // SPAIPreconditioner (kind ESP_PRECON_SPAI, spai.hip).  order 0: the n values in diag, applied as Jacobi's invdiag is.  order 1:
    // M lives in the internal handle spai_rh on A's pattern (A's device and stream); symmetric: spai_th holds its transpose and
    // spai_sh 0.5*(M + transpose(M)).  ldiv! is the row gather of esp_mul over the applied handle (spai_applied), through u1 when u
    // aliases v.  Kept for the values-only update: p of every column, its tier, the columns of the workgroup tier and their scratch.
    int spai_order = 0, spai_sym = 0;
    esp_handle *spai_rh = nullptr, *spai_th = nullptr, *spai_sh = nullptr;
    DevBuf spai_p, spai_tier, spai_list;  // u32 n, u8 n, u32 spai_stats[3]
    DevBuf spai_r, spai_half, spai_stat;  // the R slots of the workgroup tier (f64 spai_rgrid * spai_rslot), n halves, 8 status words
    i64 spai_rslot = 0, spai_rgrid = 0;
    i64 spai_stats[4] = {0, 0, 0, 0};     // max p, max q, max p*q, columns of the workgroup tier
    // ILUAM's prefactored mode (iluam.hip): the handle's values ARE the factorization -- no factor schedule, no FactorOp
    bool prefactored = false;
    // ILUTPreconditioner (kind ESP_PRECON_ILUT, ilut.hip): der.bh holds the pattern S with the values F, der.inner its prefactored
    // ILUAM.  Kept for the warm update (keep_pattern): the second value array of the sweeps, the position in A of every entry of S
    // (NO_POS for fill), the diagonal positions, the columns of the workgroup / stride tier.  ilut_h: the work handles of the
    // construction (state, candidates, L+I, U), scratch between updates
    double ilut_tau = 0.0, ilut_max_fill = 0.0;
    int ilut_steps = 0, ilut_sweeps = 0;
    bool ilut_keep = false;
    esp_handle *ilut_h[4] = {nullptr, nullptr, nullptr, nullptr};
    DevBuf ilut_alt, ilut_apos, ilut_dpos, ilut_list;  // f64 nnz(S), u32 nnz(S), u32 n, u32 2 n
    i64 ilut_tiers[2] = {0, 0};
    i64 ilut_stats[ESP_ILUT_STATS] = {0};  // esp_precon_ilut_stats' layout
    // LUFactorization (kind ESP_PRECON_LU, lu.hip): the nested-dissection ordering c of A's graph, B = the reordered matrix with the
    // complete fill of its elimination tree (A's bits where stored, +0.0 elsewhere: der.src holds ILUK_FILL there), inner its ILUAM
    // preconditioner -- the exact LU without pivoting.  ldiv! is the permuted path of block.hip: blk_new = the inverse of c, blk_path = 1
    // (0 only for n == 0).  A pattern change of A orders anew before B is rebuilt.
    int lu_leaf = 32, lu_depth = 48;
    DevBuf lu_perm, lu_level, lu_root;  // u32 n each: c, the depth every vertex was placed at, the root vertex naming its tree node
    i64 lu_stats[6] = {0, 0, 0, 0, 0, 0};  // esp_precon_lu_stats' layout
    // ... its panel form (lu_form == ESP_LU_PANELS, lu_panels.hip): B, src and the maps as above, NO inner preconditioner; the node
    // table, the update lists, the schedule and the two panels per node in lup; ldiv! is lup_solve through blk_t and blk_s
    int lu_form = 0;
    struct LuPanelData *lup = nullptr;
    // CholeskyFactorization (kind ESP_PRECON_CHOLESKY, cholesky.hip): lu_leaf / lu_depth, lu_perm / lu_level / lu_root and blk_new (the
    // inverse of c) as above; the node table, the update lists, the schedule and the panels in chol
    struct CholData *chol = nullptr;
};
// the kinds that block.hip's ldiv! serves (Block and Colored: its builder and update! too; LU builds B itself)
static inline bool block_built(const esp_precon *p) {
    return p->kind == ESP_PRECON_BLOCK || p->kind == ESP_PRECON_COLORED || p->kind == ESP_PRECON_LU;
}
// the kinds that hold a derived matrix B and an inner preconditioner of it (esp_precon::Derived)
static inline bool holds_derived(const esp_precon *p) { return block_built(p) || p->kind == ESP_PRECON_ILUK || p->kind == ESP_PRECON_ILUT; }
// ... whose next update! builds B anew (else: the values only)
static inline bool derived_stale(const esp_precon *p) {
    return p->der.rebuild || p->pattern_version != p->h->pattern_version || p->nnz != p->h->nnz;
}
// the identity-path block preconditioner and the ILU(k) preconditioner stand for their inner one in the solvers' fused branches
static inline esp_precon *fused_precon(esp_precon *p) { return p && holds_derived(p) && p->blk_path == 0 ? p->der.inner : p; }
static inline bool block_permuted(const esp_precon *p) { return p && block_built(p) && p->blk_path != 0; }
// the kinds whose ldiv! is u = diag .* v: Jacobi (invdiag) and SPAI-0 (its diagonal M) -- one branch in precon.hip and krylov.hpp
static inline bool diag_applied(const esp_precon *p) { return p->kind == ESP_PRECON_JACOBI || (p->kind == ESP_PRECON_SPAI && p->spai_order == 0); }
static inline esp_handle *spai_applied(const esp_precon *p) { return p->spai_sym ? p->spai_sh : p->spai_rh; }
// the live columns of a chunk of ESP_MANY_CHUNK right-hand sides: a plain bit mask that goes to every kernel as an argument
__host__ __device__ __forceinline__ bool is_live(u32 live, int d) { return (live >> d) & 1u; }
static inline u32 all_live(i64 nr) { return (1u << nr) - 1u; }
// the kinds whose ldiv! ends in ILUAM's level schedules or in block.hip's gather / inner solve / scatter: precon_levels_many_launch
// carries a chunk through them in one pass (LUFactorization's panel form has lup_solve_many)
static inline bool levels_many(const esp_precon *p) {
    if (block_built(p)) return !p->lup;
    return p->kind == ESP_PRECON_ILUAM || p->kind == ESP_PRECON_ILUK || p->kind == ESP_PRECON_ILUT;
}
// esp_precon_many_stats: the record of the most recent many-column solve, kept where the call reads it (the inner preconditioner of
// a kind that holds a derived matrix).  form 2 over ILUAM keeps the launch count iluam_solve_many left there
static inline void many_note(esp_precon *p, i64 form, i64 cols, i64 chunks) {
    esp_precon *q = holds_derived(p) && p->der.inner ? p->der.inner : p;
    q->many_stats[0] = form;
    q->many_stats[1] = cols;
    if (form != 2 || q->kind != ESP_PRECON_ILUAM || q->n == 0) q->many_stats[2] = 0;
    q->many_stats[3] = chunks;
}
constexpr u32 ILUK_FILL = 0xFFFFFFFFu;  // src of a fill entry of ILU(k): no position (every update! refuses nnz(A) >= 2^32 - 16)

#pragma GCC visibility push(hidden)
// precon.hip: smallest column without a stored diagonal -> ESP_ERR_INVALID (ILU0 / ILUAM), invdiag / xdiag into p->diag;
// the split layout of the row-wise index (reversed: lower part increasing, upper part decreasing column -- ILUAM's order)
int32_t diag_refresh(esp_precon *p);
int32_t split_build(esp_precon *p, bool reversed);
// iluam.hip: analysis (rebuild) + numeric factorization; ldiv! on device vectors (sub: dst[i] = dst[i] - x[i], simple!'s
// step); release of the buffers above
int32_t iluam_update(esp_precon *p, bool rebuild);
int32_t iluam_solve(esp_precon *p, const double *v, double *dst, bool sub);
// ... and of the live columns of one chunk (nr <= ESP_MANY_CHUNK columns; v: n x nr column-major with leading dimension ldv, u with
// ldu; u may be v where ldu == ldv): ONE pass over the two launch lists, the scratch p->u1 grown to ESP_MANY_CHUNK * n; launches only
int32_t iluam_solve_many(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, int nr, u32 live);
void iluam_release(esp_precon *p);
// precon.hip, for the Krylov solvers: the checks in front of a solve (p == nullptr: those of the handle alone); pass 1 of ILU0's
// ldiv! into the scratch p->u1 (pass 2 is krylov.hpp's own, in PreconProduct::ldiv: it carries the dot product)
int32_t solver_ready(esp_handle *h, esp_precon *p, const char *what);
void ilu0_lower_launch(esp_precon *p, const double *v);
// krylov_many.hip, for esp_precon_ldiv_many: ldiv! of Jacobi (SPAI-0) and ILU0 for k columns on device arrays (v: n x k column-major
// with leading dimension ldv, u with ldu; u may be v where ldu == ldv), ESP_MANY_CHUNK columns a launch; launches only
int32_t precon_ldiv_many_launch(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, i64 k);
// ... and the live columns of ONE chunk of nr <= ESP_MANY_CHUNK columns (block.hip's inner Jacobi / ILU0 under a live mask)
int32_t precon_ldiv_chunk_launch(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, int nr, u32 live);
// precon.hip: the live columns of one chunk through a kind that levels_many names -- ILUAM itself, the inner ILUAM of ILU(k) and ILUT,
// block_ldiv_many_launch for the kinds block.hip serves; launches only
int32_t precon_levels_many_launch(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, int nr, u32 live);
// precon.hip, for block.hip: the checks of every preconditioner call on the handle; ldiv! on device vectors (u may be v)
int32_t precon_check_handle(esp_handle *h, const char *what);
int32_t precon_ldiv_launch(esp_precon *p, const double *v, double *u);
// precon.hip: the frame of every esp_precon_*_create.  precon_new: an object of `kind` bound to h whose versions match nothing (the
// first update! builds everything); precon_finish: st is what the kind's set-up and first update! returned -- the object goes to
// *out, or is destroyed
esp_precon *precon_new(esp_handle *h, int kind);
int32_t precon_finish(esp_precon *p, int32_t st, esp_precon **out);
// derived.hip: the update! of the kinds that hold a derived matrix (what: the prefix of its messages; build: B from A's current CSC
// into p->der.bh and p->der.src, nothing of p changed when it fails; hint: appended when the inner preconditioner refuses a column
// on the permuted path), B's handle -- and ILU(k)'s transpose -- moved to the stream A runs on (esp_set_stream may have replaced it)
int32_t derived_update(esp_precon *p, const char *what, int32_t (*build)(esp_precon *), const char *hint);
int32_t derived_follow_stream(esp_precon *p);
// ... nzB[q] = src[q] == ILUK_FILL ? +0.0 : nzA[src[q]] (the bits); pay != nullptr (ILU(k)'s build): src[q] and lev[q] from the
// sorted payloads first, the largest level into *maxlev
void derived_gather_launch(hipStream_t s, const u64 *pay, u32 *src, int32_t *lev, const u64 *nzA, u64 *nzB, i64 nnzB,
                           unsigned long long *maxlev);
// block.hip: update! (derived_update over the masked extraction), ldiv! on device vectors (sub: u[i] = u[i] - x[i], simple!'s
// step), release of B, the inner preconditioner and every buffer
int32_t block_update(esp_precon *p);
int32_t block_ldiv_launch(esp_precon *p, const double *v, double *u, bool sub);
// ... and of the live columns of one chunk (as iluam_solve_many): the identity path is the inner many-column solve on the caller's
// arrays; the permuted path gathers the chunk into blk_t, solves into blk_s and scatters (both grown to ESP_MANY_CHUNK * n here)
int32_t block_ldiv_many_launch(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, int nr, u32 live);
void block_release(esp_precon *p);
// iluk.hip: update! (derived_update over the pattern search), release of the transpose and the level array (B, the inner
// preconditioner and src are block_release's)
int32_t iluk_update(esp_precon *p);
void iluk_release(esp_precon *p);
// ilut.hip: update! (derived_update over the construction; keep_pattern: its values-only branch is ilut_warm, s sweeps on the kept
// pattern), release of the work handles and the sweep's buffers (F, the inner preconditioner: block_release's)
int32_t ilut_update(esp_precon *p);
int32_t ilut_warm(esp_precon *p);
void ilut_release(esp_precon *p);
// color.hip: update! (after a pattern change the colouring and the maps anew, then block_update; else block_update's value gather),
// release of the colour arrays (B, the inner preconditioner and the maps are block_release's)
int32_t color_update(esp_precon *p);
void color_release(esp_precon *p);
// lu.hip: update! (derived_update over the ordering, the tree and the filled matrix), release of the ordering's arrays (B, the inner
// preconditioner, src and the inverse permutation are block_release's)
int32_t lu_update(esp_precon *p);
void lu_release(esp_precon *p);
// lu_panels.hip: ldiv! of LUFactorization's panel form on device vectors (u may be v; sub: u[i] = u[i] - x[i], simple!'s step;
// launches on the handle's stream only); esp_precon_get_factor's answer, nnz(B) doubles in B's position order exported from the
// panels; the rest of its interface is lu.hpp's
int32_t lup_solve(esp_precon *p, const double *v, double *u, bool sub);
// ... and of k columns in chunks of ESP_MANY_CHUNK (v: n x k column-major with leading dimension ldv, u with ldu; u may be v where
// ldu == ldv): per chunk a gather, two launches per depth and a scatter, nothing else
int32_t lup_solve_many(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, i64 k);
int32_t lup_factor(esp_precon *p, double *nzval, int32_t on_device);
// cholesky.hip: update! (after a pattern change the ordering, the tables and the panels anew; else the load and the numeric
// factorization), ldiv! on device vectors (u may be v; sub: u[i] = u[i] - x[i], simple!'s step; launches on the handle's stream only),
// release of everything
int32_t chol_update(esp_precon *p);
int32_t chol_solve(esp_precon *p, const double *v, double *u, bool sub);
int32_t chol_solve_many(esp_precon *p, const double *v, i64 ldv, double *u, i64 ldu, i64 k);  // (as lup_solve_many)
void chol_release(esp_precon *p);
// spai.hip: update! (after a pattern change the size pass, the tiers and M anew; else the numeric kernels alone), M's handles moved
// to the stream A runs on, ldiv! of order 1 on device vectors (u may be v; sub: u[i] = u[i] - x[i], simple!'s step; launches and at
// most one copy on the handle's stream), release of the handles and buffers
int32_t spai_update(esp_precon *p);
int32_t spai_follow_stream(esp_precon *p);
int32_t spai_apply(esp_precon *p, const double *v, double *u, bool sub);
void spai_release(esp_precon *p);
// consumers.hip: the row gather of esp_mul over h's current row-wise index (csr_current ran), enqueued on h's stream
void mul_rows_launch(esp_handle *h, const double *x, double *r);
// amg.hip: update! (the whole hierarchy is rebuilt every time), the V-cycle on device vectors (u may be v; sub: u[i] = u[i] - x[i],
// simple!'s step; launches on the handle's stream only), release of the hierarchy
int32_t amg_update(esp_precon *p);
int32_t amg_solve(esp_precon *p, const double *v, double *u, bool sub);
void amg_release(esp_precon *p);
// linalg.hip: every column of (cp: 0-based starts, rowC, valC) sorted by row, valC carried along; the caller found
// maxlen <= COLSORT_BLOCK and listed the nlong columns longer than COLSORT_LANE
constexpr int COLSORT_LANE = 32, COLSORT_BLOCK = 4096;
void sort_columns_launch(hipStream_t s, const i64 *cp, i64 nC, i64 *rowC, u64 *valC, i64 maxlen, const u32 *list, i64 nlong);
int32_t ensure(esp_handle *h, DevBuf &b, size_t need, bool keep = false);
void release(DevBuf &b);
// every device buffer of a call, released on every way out
struct Temps {
    DevBuf b[12];
    ~Temps() {
        for (DevBuf &x : b) release(x);
    }
};
// matops.hip: p[i] += 1 for i < n (a scanned 0-based colptr becomes Julia's)
void add_one_launch(hipStream_t s, i64 *p, i64 n);
// derived.hip: entries sorted (and folded) by an ESP_COO flush of a scratch handle, in two phases around the caller's own fill:
//   ScratchFlush sf(owner, "esp_xyz");   the scratch handle is destroyed on every way out; errors go to owner under that prefix
//   CK(sf.open(m, n, count));            an m x n scratch handle on owner's device with room for count records
//   ... the caller's launch writes count records to sf.keys() / sf.vals() with the layout sf.L(), and synchronises its stream ...
//   CK(sf.flush(expected));              the flush from the empty CSC, synchronised; expected >= 0: nnz it must store (unique keys)
//   sf.take(cp, rv, nz);                 the scratch handle's CSC (colptr 1-based) against whatever the three buffers held
class ScratchFlush {
  public:
    ScratchFlush(esp_handle *owner, const char *what) : owner_(owner), what_(what) {}
    ScratchFlush(const ScratchFlush &) = delete;
    ~ScratchFlush();
    // fail_hook: owner's armed esp_debug_fail_next_bucket_stage moves to the scratch handle (this is the flush it meets)
    int32_t open(i64 m, i64 n, i64 count, bool fail_hook = false);
    u64 *keys() const { return (u64 *)sc_->keys.p; }
    u64 *vals() const { return (u64 *)sc_->vals.p; }
    const KeyLayout &L() const { return sc_->L; }
    hipStream_t stream() const { return sc_->stream; }
    int32_t flush(i64 expected);
    i64 nnz() const { return sc_ ? sc_->nnz : 0; }
    void take(DevBuf &cp, DevBuf &rv, DevBuf &nz);

  private:
    esp_handle *owner_, *sc_ = nullptr;
    const char *what_;
    i64 count_ = 0;
};
// linalg.hip: "every column of (cp, rows, payload) sorted by row" in two phases around the caller's fill of nnz entries:
//   plan     cp holds the scanned 0-based column starts (n + 1), st two zeroed device words: measures the columns and picks the
//            route; the fill then writes either rowB[q] (1-based) and pay[q] -- rv and pay, sized here -- or, keys != nullptr,
//            the ESP_COO record keys[q] (layout L) and pay[q] of a scratch handle (a column longer than COLSORT_BLOCK)
//   finish   behind the fill on h's stream: the lane / workgroup sorts, or h's stream synchronised and the scratch flush, whose CSC
//            cp / rv / pay then hold (*one_based: cp is 1-based already)
class ColumnSort {
  public:
    ColumnSort(esp_handle *h, const char *what) : h_(h), sf_(h, what) {}
    ~ColumnSort() { release(list_); }
    int32_t plan(DevBuf &cp, i64 n, i64 nnz, unsigned long long *st, DevBuf &rv, DevBuf &pay);
    int32_t finish(bool *one_based);
    i64 *rowB = nullptr;
    u64 *pay = nullptr, *keys = nullptr;
    KeyLayout L{1, 1};

  private:
    esp_handle *h_;
    ScratchFlush sf_;
    DevBuf list_, *cp_ = nullptr, *rv_ = nullptr, *pay_ = nullptr;
    i64 n_ = 0, nnz_ = 0, nlong_ = 0, maxlen_ = 0;
};
void release_all(esp_handle *h);
hipEvent_t ev_get(esp_handle *h);
void timing_collect(esp_handle *h);
int32_t fix_tail(esp_handle *h);
int32_t init_empty_csc(esp_handle *h);
int32_t reserve_append(esp_handle *h, i64 add);
int32_t pack_device(esp_handle *h, const i64 *d_rows, const i64 *d_cols, const double *d_vals,
                           const uint8_t *d_kinds, int kind_all, int op, i64 count);
int32_t ensure_stage(esp_handle *h, esp_handle::StageArea &sa, i64 want);
int32_t ensure_bounce(esp_handle *h);
void par_memcpy(void *dst, const void *src, size_t bytes);
void host_run_parts(int parts, const std::function<void(int)> &fn);
int32_t d2h_pipelined(esp_handle *h, void *dst, const void *d_src, size_t bytes);
// a device array into the caller's host or device array, synchronised / n values of a u32 device array as int64 minus sub likewise
int32_t copy_out(esp_handle *h, void *dst, const void *d_src, size_t bytes, int32_t on_device);
int32_t export_u32_as_i64(esp_handle *h, const void *d_src, i64 n, u32 sub, int64_t *out, int32_t on_device);
// pageable host memory -> device through the same two pinned bounce buffers (the host copy of chunk i+1 overlaps the transfer
// of chunk i); returns when the device holds the data
int32_t h2d_pipelined(esp_handle *h, void *d_dst, const void *src, size_t bytes);
i64 fd_offset_host(i64 nx, i64 ny, i64 nz, i64 g);
int32_t prepart_begin(esp_handle *h, i64 E, i64 chunks, int kind, PartSetup *ps);
int32_t prepart_rank(esp_handle *h, PartSetup *ps);
int32_t prepart_finish(esp_handle *h, PartSetup *ps, bool *took);
int32_t pending_materialize(esp_handle *h);
namespace esplocal {
bool launch_group3_items(const esp_handle::LazyItems &lz, unsigned grid, hipStream_t stream, const Args &a, bool hits = false);  // local_j.hip
bool launch_group3_items_multi(int nloc, bool diag, const u32 *vlist, const MultiBuf *mbuf, i64 *counts, int S_real, unsigned grid,
                               hipStream_t stream, const Args &a);  // local_j.hip
}
constexpr int32_t ESP_RETRY_EXPANDED = 1000;  // flush_local to esp_flush: expand the items (lazy_expand) and call again -- never leaves the library
int32_t lazy_expand(esp_handle *h);   // produce.hip: the expansion of a batch held as sorted items (esp_handle::LazyItems) or as the
                                      // stencil generator's held-back PART launch (esp_handle::LazyStencil)
// may an item partition on this handle leave its batch unexpanded?  (kind: what its updates are; produce.hip)
bool lazy_items_wanted(const esp_handle *h, int kind);
int32_t settle_offset(esp_handle *h);
int32_t item_produce_fem(esp_handle *h, const espgen::FemArgs &fa, i64 E, bool *took);
int32_t partition_pass(esp_handle *h, espradix::Pass &p, i64 max_tiles);
// partition.hip: the stable LSD sort of ONE segment of count (key, payload) pairs on the key bits [shift0, shift0 + bits), 8 bits per
// pass (the last one: what is left).  The passes alternate between the two halves of d.  A source that is one of the halves sends
// the first pass to the other one; a source of its own (read only) is left alone and the last pass lands in half 0.  *out: the pair
// that holds the result (src itself when bits == 0).  err_slot: the u32 word of h->misc that a key outside [base, base + span) sets.
struct SortPair {
    const u64 *k;
    const double *v;
};
struct PingPong {
    u64 *k[2];
    double *v[2];
    SortPair half(int i) const { return SortPair{k[i], v[i]}; }
};
int32_t sort_segment_lsd(esp_handle *h, SortPair src, const PingPong &d, i64 count, int shift0, int bits, int err_slot, SortPair *out,
                         u64 base = 0, u64 span = ~0ull);
// the two halves of n pairs each at the front of one allocation of at least 4 * n * 8 bytes: keys 0, keys 1, payloads 0, payloads 1;
// *rest: where the caller's further arrays begin
static inline PingPong carve_pingpong(void *p, i64 n, void **rest = nullptr) {
    PingPong d;
    d.k[0] = (u64 *)p;
    d.k[1] = d.k[0] + n;
    d.v[0] = (double *)(d.k[1] + n);
    d.v[1] = d.v[0] + n;
    if (rest) *rest = d.v[1] + n;
    return d;
}
int32_t sort_pending_lsd(esp_handle *h, const u64 **sk, const double **sv);
int32_t chunk_arrays(esp_handle *h, i64 Ccap, int pb, ChunkArrays *out, bool keep_plan = false);
double plan_entries(i64 E, int K, u64 span);
int plan_run_bits(i64 E, int K, u64 span);
int plan_prefix_bits(const esp_handle *h, i64 E, int K, double *Ee_out);
int plan_local_bits(esp_handle *h, i64 NI, int W, int K, int *sort_bits);
int window_bits(const esp_handle *h);
int32_t aux_ready(esp_handle *h);
int32_t run_partition(esp_handle *h, const u64 *kin, const double *vin, u64 *kout, double *vout, int K, int pb,
                             i64 *seg_out, u64 *tile_first_out, bool *tiles_ready, bool *ok, i64 *maxlen_out,
                             const MultiWin *mw = nullptr, int mw_shift = 0, bool allow_k32 = false, int *key_bytes_out = nullptr,
                             i64 E_in = -1, const RawSource *raw = nullptr);
int32_t append_first_pass(esp_handle *h, const i64 *d_rows, const i64 *d_cols, const double *d_vals, int kind, int op, i64 count, bool *took);  // partition.hip
int32_t append_tail_partitioned(esp_handle *h, const i64 *d_rows, const i64 *d_cols, const double *d_vals, int kind, int op, i64 count,
                                 bool *took);
int32_t append_partitioned(esp_handle *h, const i64 *d_rows, const i64 *d_cols, const double *d_vals, int kind, int op, i64 count,
                                  bool *took);
int32_t sort_msd(esp_handle *h, Sorted *out);
int32_t finish_csc(esp_handle *h, i64 Z0, i64 Zn, const u64 *new_key, const double *new_val);
int32_t prepare_outputs(esp_handle *h, i64 Z0, i64 Zn);
int32_t flush_local(esp_handle *h, const Sorted &st, int mode, i64 *Zn_out);
int32_t flush_global(esp_handle *h, int mode, i64 *Zn_out);
int32_t flush_pre_tail(esp_handle *h, int mode, i64 *Zn, bool *served);
int32_t build_csr(esp_handle *h);
int32_t csr_current(esp_handle *h);  // build_csr after a pattern change, the row-wise values after a value change
int32_t dirichlet_call(esp_handle *h, uint8_t *marker, int32_t on_device, bool mark, double penalty);
int32_t diag_setup(esp_handle *h, double *inv, int64_t *idiag, int32_t on_device, const char *what);
int32_t shard_prepare(esp_handle *h, int P, espradix::Pass *out);
int32_t shard_offsets(esp_handle *h, int P, int64_t *offsets /* P+1 */);
// matops.hip, shared with linalg.hip: the operand rules of the algebra calls (no pending entries, no column window or shard,
// dimensions below 2^32; synchronised), a result CSC taken over by c (a pattern change), a device i64 read back
int32_t check_operand(esp_handle *h, const char *what);
void install(esp_handle *c, DevBuf &cp, DevBuf &rv, DevBuf &nz, i64 nnz);
int32_t read_i64(esp_handle *h, const i64 *d_src, i64 *out);
#pragma GCC visibility pop

struct Span {
    esp_handle *h;
    int stage;
    hipEvent_t a = nullptr;
    int launches = 0;
    Span(esp_handle *hh, int st) : h(hh), stage(st) {
        // timing level 1 brackets the big kernels only: the ~20 tiny launches of the "scan" stage would cost
        // more in event records (two per span) than they run
        if (h->timing && (h->timing_level == 2 || (h->timing_level == 1 && st != ESP_ST_SCAN) ||
                          (h->timing_level == 3 && (st == ESP_ST_LOCAL || st == ESP_ST_FOLD)))) {
            a = ev_get(h);
            (void)hipEventRecord(a, h->stream);
        }
    }
    void add(int l) { launches += l; }
    ~Span() {
        if (h->timing && a) {
            hipEvent_t b = ev_get(h);
            (void)hipEventRecord(b, h->stream);
            h->spans.push_back({stage, a, b, launches});
            if (h->spans.size() > 2048) timing_collect(h);
        }
    }
};

// ------------------------------------------------------------------------ small kernels
static __global__ void set_i64_k(i64 *p, i64 a, i64 b, i64 c, i64 d) {
    p[0] = a;
    p[1] = b;
    p[2] = c;
    p[3] = d;
}
static __global__ void fill_i64_k(i64 *p, i64 n, i64 v) {
    const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) p[g] = v;
}

// The 64-byte block of partition results (longest bucket + four flag words) goes to pinned HOST memory with plain
// stores: the host then needs neither a copy engine nor a blit kernel -- which may queue behind the kernel that fills
// the chip -- to read it, only the event recorded behind this launch.
static __global__ void publish_block_k(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ host_dst) {
    if (threadIdx.x < 8) __hip_atomic_store(&host_dst[threadIdx.x], src[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the longest run of 2^fb neighbouring buckets (one segment of a fine partition's flush: esp_handle::PrePart::fb)
static __global__ void coarse_seg_max_k(const i64 *__restrict__ seg, i64 S_coarse, int fb, unsigned long long *__restrict__ out) {
    const i64 g = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 len = g < S_coarse ? (u32)min((i64)0xFFFFFFFFll, seg[(g + 1) << fb] - seg[g << fb]) : 0u;
    const u32 m = esp_wave_max(len);
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, (unsigned long long)m);
}

static inline unsigned grid_for(i64 n, int threads) { return (unsigned)std::max<i64>(1, ceil_div<i64>(n, threads)); }


// ---- small helpers
// no force_path, or one that pins the bucket kernel's form alone (42: one bucket per workgroup, 43: no predicted offsets, 44: the
// stencil batch is always written, 45: the fused kernel always stores the structure): every other choice automatic
static inline bool paths_auto(const esp_handle *h) {
    return h->force_path == ESP_PATH_AUTO || h->force_path == ESP_PATH_NO_BUCKET_PAIRS || h->force_path == ESP_PATH_NO_PREDICTED_OFFSETS ||
           h->force_path == ESP_PATH_NO_LAZY_STENCIL || h->force_path == ESP_PATH_NO_KEPT_STRUCTURE;
}
static inline bool windowed(const esp_handle *h) { return h->win_excl && (h->wc0 > 0 || h->wc1 < h->n); }

// first entry and number of entries of the per-column arrays (colptr, colend: n+1 entries) a flush touches
static inline void col_range(const esp_handle *h, i64 *c0, i64 *cnt) {
    *c0 = windowed(h) ? h->wc0 : 0;
    *cnt = windowed(h) ? h->wc1 - h->wc0 + 1 : h->n + 1;
}

// The look-back status area of a bucket-kernel launch over S segments (u64 words; flush.hip and sum.hip): one granule per
// segment | error flag | longest run | one granule per group of 256 segments, rounded up to a 4 KiB page; behind them a page
// of its own for the ticket counter (every workgroup draws from it while others poll the granules: on one line with them the
// draws cost the headline's bucket kernel 0.18 of 1.55 ms) -- one memset of bytes() clears everything
struct StatusLayout {
    i64 S, G, words;
    explicit StatusLayout(i64 S_) : S(S_) {
        const i64 n_gs = (S >> 8) + 2;                     // (local.hpp: LB_SHIFT = 8)
        G = ((S + 2 + n_gs + 511) & ~(i64)511) - (S + 2);  // (granules behind status[S + 1])
        words = S + 2 + G + 512;
    }
    size_t bytes() const { return sizeof(u64) * (size_t)words; }
    void point(esplocal::Args &a, u64 *status) const {
        a.status = status;
        a.gstatus = status + S + 2;
        a.ticket = (u32 *)(status + S + 2 + G + 256);
        a.err = (u32 *)(status + S) + 1;
        a.maxrun_seen = (u32 *)(status + S) + 2;  // (zeroed with the granules)
    }
};

// The digits of a partition cut the 2^K keys of the window's bit range, of which only `span` exist (a matrix
// with 2^k + 1 columns fills half of it): the plan counts the entries as if the empty part were filled as well,
// so that the occupied buckets come out at the planned fill.
// planned average fill of a segment (fraction of the bucket kernel's capacity); ESP_PLAN_FILL overrides (experiments)
static double plan_fill() {
    static const double f = [] {
        const char *e = esp_exp_env("ESP_PLAN_FILL");
        const double v = e ? atof(e) : 0.9;
        return v > 0.1 && v <= 1.0 ? v : 0.9;
    }();
    return f;
}

// records a segment of the partition may hold: the bucket kernel's capacity, or what an item partition says (plan_cap)
static inline i64 seg_cap(const esp_handle *h) { return h->plan_cap > 0 ? h->plan_cap : (i64)esplocal::CAP; }

// The plan of the partition by (owner, digit inside the owner's column range): every rank derives the same one from
// (n, P, entries_per_shard).  ok = false: small or odd problem (the plain exchange serves it).
static inline i64 shard_col0(i64 n, int P, int r) { return (i64)(((__int128)r * (__int128)n + P - 1) / P); }  // ceil(r*n/P)
static MwPlan shard_mw_plan(const esp_handle *h, int P, i64 entries_per_shard) {
    MwPlan m;
    m.base.resize((size_t)P);
    u64 maxspan = 1;
    for (int r = 0; r < P; r++) {
        const i64 c0 = shard_col0(h->n, P, r), c1 = shard_col0(h->n, P, r + 1);
        m.base[(size_t)r] = (u64)c0 << h->L.rb;
        maxspan = std::max(maxspan, (u64)(c1 - c0) << h->L.rb);
    }
    int K = 1;
    while (K < 62 && ((u64)1 << K) < maxspan) K++;
    const int pbw = plan_run_bits(std::max<i64>(entries_per_shard, 1), K, maxspan);
    if (pbw == 0 || K - pbw > esplocal::MAX_REM_BITS) return m;
    m.K = K;
    m.shift = K - pbw;
    m.nb64 = ((maxspan - 1) >> m.shift) + 1;
    m.NB = (i64)m.nb64 * P;
    if (m.NB > ((i64)1 << 24)) return m;
    m.pb = 1;
    while (((i64)1 << m.pb) < m.NB) m.pb++;
    if (m.shift > 32 && m.shift - 32 <= 4 && h->L.rb <= 32 && (m.NB << (m.shift - 32)) <= ((i64)1 << 24)) m.fb = m.shift - 32;
    m.ok = true;
    return m;
}

// in-place exclusive scan with its workspace in a handle buffer
// exclusive scan helpers with scratch carved from h->misc
template <typename T, bool MAX>
static int32_t scan_inplace(esp_handle *h, T *data, i64 n, DevBuf &ws, int *launches) {
    CK(ensure(h, ws, sizeof(T) * (size_t)espscan::workspace_elems(n)));
    *launches += espscan::exclusive<T, MAX>(h->stream, data, data, n, (T *)ws.p);
    return ESP_OK;
}
