/*
 * esparse_hip.h -- C ABI of libesparse_hip.so, the MI355X (gfx950) sparse-assembly
 * backend for ExtendableSparse.jl's ExtendableSparseMatrix.
 *
 * What it replaces (paths relative to the reference repository):
 *   - the CPU insertion buffer SparseMatrixLNK  (src/matrix/sparsematrixlnk.jl:21-253)
 *     becomes a device-resident COO append buffer (packed u64 key + f64 value);
 *   - flush! / `lnk + csc`  (src/matrix/extendable.jl:248-255,
 *     src/matrix/sparsematrixlnk.jl:294-383) becomes a HIP pipeline: stable radix
 *     partition on (col,row) keys, LDS-staged ordered fold of duplicates,
 *     merge-path join with the existing CSC.
 * The entry points are what the reference's plugin slot for extension buffers
 * (src/matrix/abstractsparsematrixextension.jl:6-14, used by
 * src/matrix/genericextendablesparsematrixcsc.jl:14-92 and
 * src/matrix/genericmtextendablesparsematrixcsc.jl:16-114) needs from a foreign
 * buffer; INTEGRATION.md shows the Julia `ccall` shim that binds them.
 *
 * Conventions
 *   - every function returns an int32 status (0 = ok, <0 = esp_status); nothing
 *     throws or aborts across the boundary; esp_last_error() gives the message;
 *   - all matrix indices are 1-based Int64, exactly as Julia passes them;
 *   - output arrays are caller-allocated (Julia Vectors) after a size query;
 *   - one handle = one device + one HIP stream; a handle is not thread-safe
 *     (like one reference buffer per `tid`); distinct handles are independent and may be
 *     driven from different host threads concurrently -- fills, flushes, transfers, first
 *     use included (genericmtextendablesparsematrixcsc.jl:87-99: one buffer per task;
 *     tests/test_concurrent_handles.py; the corruption rounds 4 and 5 saw here was a
 *     missing barrier inside the bucket kernel, NOTES/round6.md section 1).  The library
 *     starts no threads of its own on the flush path, with one exception: when esp_flush_sum
 *     cannot fold its buffers in one flush (esp_debug_last_sum_batched 0: a column window or a
 *     test hook on a buffer) it folds them one by one, side by side on its host-copy pool (at
 *     most eight threads with the caller's; ESP_HOST_THREADS caps it);
 *   - element types: Float64 values, Int64 indices (the reference's default
 *     ExtendableSparseMatrix{Float64,Int64}); other Tv/Ti stay on the CPU path.
 */
#ifndef ESPARSE_HIP_H
#define ESPARSE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct esp_handle esp_handle;

typedef enum {
    ESP_OK = 0,
    ESP_ERR_INVALID = -1,     /* bad argument / NULL handle                       */
    ESP_ERR_BOUNDS = -2,      /* (i,j) outside 1..m x 1..n  -> Julia BoundsError  */
    ESP_ERR_HIP = -3,         /* a HIP runtime call failed                         */
    ESP_ERR_NOMEM = -4,       /* device or pinned allocation failed                */
    ESP_ERR_UNSUPPORTED = -5, /* dimension / count outside the supported range     */
    ESP_ERR_STATE = -6,       /* call not valid in the handle's current state      */
    ESP_ERR_NODEVICE = -7,    /* no usable GPU (the product never falls back)      */
    ESP_ERR_NOTPOSDEF = -8    /* CholeskyFactorization: a pivot is not positive    -> Julia PosDefException */
} esp_status;

/* How an appended entry combines with what is already stored at (i,j).
 * SET       = Base.setindex!      (sparsematrixlnk.jl:178-201, extendable.jl:205-218)
 * UPDATE    = updateindex!(A,+..) (sparsematrixlnk.jl:210-228, extendable.jl:159-174)
 * RAWUPDATE = rawupdateindex!     (sparsematrixlnk.jl:237-253, extendable.jl:181-197)
 * COO       = a triplet of sparse(I,J,V,m,n,+), i.e. of the COO constructors (extendable.jl:85-104) and
 *             fdrand_coo (sprand.jl:134-185): always creates, the first value as it is, duplicates
 *             added in input order */
typedef enum { ESP_SET = 0, ESP_UPDATE = 1, ESP_RAWUPDATE = 2, ESP_COO = 3 } esp_kind;

/* `op` of updateindex!/rawupdateindex!.  Every call site of the reference passes `+`;
 * `-` is exact as `+` of the negated value.  Other functions stay on the CPU path. */
typedef enum { ESP_OP_ADD = 0, ESP_OP_SUB = 1 } esp_op;

/* Which reference operation esp_flush() evaluates:
 * ROUTED = flush!(ExtendableSparseMatrixCSC): every appended update of an (i,j) that
 *          is already in the CSC is applied to csc.nzval in call order
 *          (extendable.jl:164-166,188-189,210-211), the others fold in the buffer and
 *          are merged in (extendable.jl:248-255);
 * PLUS   = Base.:+(buffer, csc) (sparsematrixlnk.jl:294-383): the buffer folds on its
 *          own and equal positions give csc.nzval + buffer value (:363).            */
typedef enum { ESP_FLUSH_ROUTED = 0, ESP_FLUSH_PLUS = 1 } esp_flush_mode;

/* pipeline stages reported by esp_timing() */
enum {
    ESP_ST_APPEND = 0, /* pack / generator kernels (coalesced stores into the buffer) */
    ESP_ST_HIST = 1,   /* digit histograms of the radix partition                      */
    ESP_ST_SCAN = 2,   /* exclusive scans (offsets, colptr)                           */
    ESP_ST_SCATTER = 3,/* stable radix partition passes (global)                      */
    ESP_ST_LOCAL = 4,  /* LDS bucket sort + ordered fold + emit                       */
    ESP_ST_FOLD = 5,   /* ordered segmented fold on globally sorted entries           */
    ESP_ST_COLPTR = 6, /* column ends -> colptr                                       */
    ESP_ST_MERGE = 7,  /* merge-path join with the existing CSC                       */
    ESP_ST_COPY = 8,   /* H2D / D2H copies issued by this library                     */
    ESP_ST_COUNT = 9
};
typedef struct {
    double ms[ESP_ST_COUNT];        /* summed hipEvent time per stage since the last clear */
    int64_t launches[ESP_ST_COUNT]; /* kernel launches (or copies) per stage               */
    double flush_ms;                /* whole esp_flush calls (device time)                 */
    int64_t flushes;
} esp_timing_t;

/* ---- lifetime -------------------------------------------------------------------
 * esp_create: the constructor T_ext(m,n) of the plugin contract
 * (abstractsparsematrixextension.jl:8; SparseMatrixLNK{Tv,Ti}(m,n),
 * sparsematrixlnk.jl:75-77).  capacity_hint = expected number of appended entries. */
int32_t esp_create(int64_t m, int64_t n, int32_t device, int64_t capacity_hint, esp_handle **out);
int32_t esp_destroy(esp_handle *h);
/* Base.copy(ext) (extendable.jl:279-285): same CSC, same pending entries, same window; device-to-device */
int32_t esp_clone(esp_handle *h, esp_handle **out);
/* frees every device and pinned buffer of the handle NOW (the Generic wrappers drop their buffer after every flush!
 * -- genericextendablesparsematrixcsc.jl:34 -- and Julia's GC does not see device memory); the handle stays valid:
 * an empty matrix with an empty buffer.  Staging pointers from esp_stage_begin are invalid afterwards. */
int32_t esp_release_buffers(esp_handle *h);
const char *esp_last_error(const esp_handle *h);
const char *esp_version(void);
/* use an external HIP stream (hipStream_t) instead of the handle's own */
int32_t esp_set_stream(esp_handle *h, void *hip_stream);
int32_t esp_synchronize(esp_handle *h);
/* Base.size(ext) (abstractsparsematrixextension.jl:10) */
int32_t esp_size(const esp_handle *h, int64_t *m, int64_t *n);
/* packed key layout: key = ((col-1) << row_bits | (row-1)) << 2 | kind */
int32_t esp_key_layout(const esp_handle *h, int32_t *row_bits, int32_t *col_bits);

/* ---- append (replaces setindex!/updateindex!/rawupdateindex! on the buffer) -----
 * Host-fed: Julia fills a pinned chunk obtained from esp_stage_begin and commits it;
 * one ccall per chunk, not per entry.  kinds may be left untouched when kind_all>=0.
 * The chunk pointers stay valid until esp_stage_begin is called with a larger `want` (or esp_destroy);
 * no other call moves them (esp_append_host stages through an area of its own).  esp_commit returns
 * when the chunk may be refilled -- after it has been packed on the host (bounds are checked there: ESP_ERR_BOUNDS is
 * immediate and nothing of the chunk is appended) into one of two pinned halves; the transfer to the device runs while the
 * caller fills the chunk again. */
int32_t esp_stage_begin(esp_handle *h, int64_t want, int64_t **rows, int64_t **cols,
                        double **vals, uint8_t **kinds, int64_t *got);
int32_t esp_commit(esp_handle *h, int64_t count, int32_t kind_all, int32_t op);
/* bulk host arrays (COO constructor path extendable.jl:92-104): kinds==NULL -> kind_all */
int32_t esp_append_host(esp_handle *h, const int64_t *rows, const int64_t *cols,
                        const double *vals, const uint8_t *kinds, int32_t kind_all, int32_t op,
                        int64_t count);
/* the same for Int32 index arrays (ExtendableSparseMatrix{Float64,Int32}: extendable.jl:10-25 is generic in Ti; the CSC
 * the library hands back is Int64 all the same).  Both pack (row, col, kind) into keys on the host, whatever the index
 * type: 8-byte keys (16 bytes per entry over PCIe), or -- one kind for the batch (kinds == NULL) and at most 48 row + column
 * bits -- six-byte keys without the kind (14 bytes per entry), which a small kernel per chunk turns into packed keys on the
 * device */
int32_t esp_append_host_i32(esp_handle *h, const int32_t *rows, const int32_t *cols,
                            const double *vals, const uint8_t *kinds, int32_t kind_all, int32_t op,
                            int64_t count);
/* device-side producers: arrays already in HBM on this handle's device.  An index outside the matrix: ESP_ERR_BOUNDS, nothing is
 * appended; the message names AN offending entry -- the first of the batch when the batch was packed in stream order, the
 * smallest position among the tiles examined before the kernels gave up when the append was the partition */
int32_t esp_append_device(esp_handle *h, const int64_t *d_rows, const int64_t *d_cols,
                          const double *d_vals, const uint8_t *d_kinds, int32_t kind_all,
                          int32_t op, int64_t count);
/* entries already packed in this handle's key layout (used by the shard exchange) */
int32_t esp_append_packed(esp_handle *h, const uint64_t *d_keys, const double *d_vals,
                          int64_t count);
/* on-device update streams of the reference's workloads.  Called on an EMPTY buffer with a stream an assembly loop
 * emits (few column blocks per 256 nodes / 128 cells) the append is the partition: the entries are stored bucket by
 * bucket -- a stable permutation of the stream, so every (i,j) keeps its call order -- and esp_flush needs no partition
 * pass.  Any later append, clone or shard call first turns the batch back into an ordinary pending buffer.
 *
 * fdrand!(A,nx,ny,nz;update,rand) hot loop (src/matrix/sprand.jl:87-124); rand_mode
 * 0: ()->1, 1: 0.1+u (fdrand default, :232), 2: u; kind = ESP_UPDATE / ESP_RAWUPDATE;
 * testassemble! (test/femtools.jl:45-72) on a Kuhn grid with npd points per axis.    */
int32_t esp_generate_fdrand(esp_handle *h, int64_t nx, int64_t ny, int64_t nz, uint64_t seed,
                            int32_t rand_mode, int32_t kind);
int32_t esp_generate_fem(esp_handle *h, int32_t dim, int64_t npd, uint64_t seed,
                         int32_t order_mode);
/* the part of the fdrand! stream issued by the nodes [node_begin, node_end) (0-based l-1) of the
 * k,j,i loop nest: one rank's slab of a sharded assembly */
int32_t esp_generate_fdrand_range(esp_handle *h, int64_t nx, int64_t ny, int64_t nz, uint64_t seed,
                                  int32_t rand_mode, int32_t kind, int64_t node_begin,
                                  int64_t node_end);
/* Element-level append: the inner loops of a finite-element assembly (test/femtools.jl:61-69) as ONE call, for element data
 * the caller holds in arrays (Julia layouts, 1-based node numbers):
 *   for icell = 1:ncells, il = 1:nloc:  i = cellnodes[il,icell]
 *       diag != NULL:  update(A, diag[il,icell], i, i)                            (femtools.jl:64)
 *       for jl = 1:nloc:  update(A, elmat[il,jl,icell], i, cellnodes[jl,icell])   (femtools.jl:65-68)
 * with update = setindex! / updateindex! / rawupdateindex! as `kind` says (op as for esp_commit).  cellnodes: Int64
 * nloc x ncells (grid[CellNodes], femtools.jl:47), elmat: Float64 nloc x nloc x ncells (vol * S of femtools.jl:67), diag:
 * Float64 nloc x ncells or NULL; 1 <= nloc <= 16.  Bit-identical to the nloc * (nloc [+ 1]) per-entry calls per cell in
 * that order.  On an EMPTY buffer the library partitions one 8-byte record per (cell, local column) instead of the updates
 * and stores every update once, at its bucket position (the flush starts at the bucket kernel: esp_debug_last_partition 4);
 * a cell that names a node twice, a non-empty buffer or a column window: the updates are appended in stream order.
 * A node number outside 1..min(m,n): ESP_ERR_BOUNDS, nothing is appended.  The device form reads d_elmat (and, without cell
 * records, d_cellnodes / d_diag) AT FLUSH TIME: on a fresh matrix -- and over the pattern the same mesh built -- the batch stays a
 * list of sorted (cell, local column) items and the flush's bucket kernel forms the updates itself (csrc/group3_items.hpp: the
 * updates are never written to the append buffer).  The arrays must stay valid and unchanged until the handle's next esp_flush
 * (or esp_reset / esp_clear_pending / esp_destroy) has returned; the host form keeps its own device copy that long. */
int32_t esp_append_elements(esp_handle *h, int32_t nloc, int64_t ncells, const int64_t *d_cellnodes,
                            const double *d_elmat, const double *d_diag, int32_t kind, int32_t op);
int32_t esp_append_elements_host(esp_handle *h, int32_t nloc, int64_t ncells, const int64_t *cellnodes,
                                 const double *elmat, const double *diag, int32_t kind, int32_t op);
/* A time step of an instationary / nonlinear code assembles the SAME mesh again with new element matrices.
 * esp_elements_keep_plan(h, 1): from now on an esp_append_elements call on an empty buffer (cells of 3 or 4 nodes, the item
 * partition taken) keeps its plan -- the item order, the cell records, the segment table: 8 B per (cell, local column) + 64 B
 * per cell of device memory; on = 0 releases it.  esp_append_elements_again(h, d_elmat, d_diag, kind, op): the element loop
 * over the connectivity of that planned call (diag NULL iff it was then), on an empty buffer: no pass over the connectivity, no
 * item partition; the entries are bit for bit what esp_append_elements with the same cellnodes would append.  Without a plan:
 * ESP_ERR_STATE.  Together with the flush over the stored pattern (every update hits) a time step costs less than the
 * first assembly. */
int32_t esp_elements_keep_plan(esp_handle *h, int32_t on);
/* (d_elmat as for esp_append_elements: read at flush time, valid until the next esp_flush has returned) */
int32_t esp_append_elements_again(esp_handle *h, const double *d_elmat, const double *d_diag, int32_t kind, int32_t op);
int32_t esp_append_elements_again_host(esp_handle *h, const double *elmat, const double *diag, int32_t kind, int32_t op);
/* The element data of esp_generate_fem's grid as DEVICE arrays, for the cells at stream positions [cell_begin, cell_end):
 * what a caller of testassemble! holds (cellnodes) and computes per cell (elmat = vol * S, diag = 0.1 * vol / (dim+1);
 * femtools.jl:58-67) -- the producer of esp_append_elements' input in tests and bench.  node_mode 1: the nodes carry a
 * permuted numbering (a bijection of 1..n made from node_seed): nothing downstream can lean on grid arithmetic.
 * d_diag may be NULL. */
int32_t esp_generate_fem_mesh(esp_handle *h, int32_t dim, int64_t npd, uint64_t seed, int32_t order_mode,
                              int32_t node_mode, uint64_t node_seed, int64_t cell_begin, int64_t cell_end,
                              int64_t *d_cellnodes, double *d_elmat, double *d_diag);
/* number of appended, not yet flushed entries; >0 iff anything is pending
 * (the flush! gate of genericextendablesparsematrixcsc.jl:32 / nnznew :21) */
int32_t esp_pending(const esp_handle *h, int64_t *count);

/* ---- the CSC side ---------------------------------------------------------------
 * esp_set_csc: attach an existing SparseMatrixCSC (the `csc` operand of `ext + csc`). */
int32_t esp_set_csc(esp_handle *h, const int64_t *colptr, const int64_t *rowval,
                    const double *nzval, int64_t nnz);
/* THE flush: sort + ordered fold + join, result stays device-resident.
 * pattern_changed = 1 iff the CSC was rebuilt (the reference recomputes phash then). */
int32_t esp_flush(esp_handle *h, int32_t mode, int64_t *new_nnz, int32_t *pattern_changed);
/* Base.sum(xmatrices, csc) (sparsematrixdilnkc.jl:397-435) = flush! of GenericMTExtendableSparseMatrixCSC
 * (genericmtextendablesparsematrixcsc.jl:45-51) as ONE call: dst holds the CSC (esp_set_csc, or the result of its last
 * flush) and no pending entries; xs[0..p) are the partition buffers -- handles of the same size on the same device whose own
 * matrix is empty.  Result, bit for bit the reference's sparse!(I,J,V,m,n,+) over (csc entries, buffer 1's entries, ...):
 * at (i,j) ((csc + f_1) + f_2) + ... where f_k is the fold of the calls buffer k received at (i,j), buffers that do not
 * hold (i,j) skipped, zeros kept.  Every buffer is folded by itself on the device, the folds meet the stored matrix in ONE
 * routed flush of dst; no CSC travels between host and device whatever p is.  The buffers come back EMPTY (the reference
 * replaces them all, :47-49).  pattern_changed as for esp_flush. */
int32_t esp_flush_sum(esp_handle *dst, esp_handle *const *xs, int32_t p, int64_t *new_nnz,
                      int32_t *pattern_changed);
/* SparseArrays.nnz of the device CSC (does not flush) */
int32_t esp_nnz(const esp_handle *h, int64_t *nnz);
/* D2H into caller arrays: colptr (n+1), rowval (nnz), nzval (nnz); Julia layout.  Large destinations (> 8 MiB) get
 * madvise(MADV_HUGEPAGE) on their 2 MiB-aligned interior before the first byte lands -- a hint that changes no contents: a
 * vector the caller has just allocated is untouched memory, and its first touch otherwise costs ten times the copy */
int32_t esp_get_csc(esp_handle *h, int64_t *colptr, int64_t *rowval, double *nzval);
/* The same transfers for Int32 index arrays (SparseMatrixCSC{Float64,Int32}: extendable.jl:10-25 is generic in Ti).  The
 * device CSC stays Int64; colptr / rowval are narrowed (widened) on the device, so they cross PCIe as 4 bytes.
 * esp_get_csc_i32: ESP_ERR_UNSUPPORTED when m or nnz + 1 exceeds 2^31 - 1 (Julia's own Int32 CSC could not hold it). */
int32_t esp_set_csc_i32(esp_handle *h, const int32_t *colptr, const int32_t *rowval,
                        const double *nzval, int64_t nnz);
int32_t esp_get_csc_i32(esp_handle *h, int32_t *colptr, int32_t *rowval, double *nzval);
/* D2H of nzval only (pattern unchanged since the caller's last esp_get_csc) */
int32_t esp_get_nzval(esp_handle *h, double *nzval);
/* H2D of nzval only: the attached CSC keeps its pattern (the one of the caller's last esp_set_csc / esp_get_csc) and takes
 * these nnz values -- what a plug-in whose CSC stays on the device between flushes uploads when only nonzeros(A) can have
 * been edited on the host (the Generic wrappers edit cscmatrix.nzval in place: genericextendablesparsematrixcsc.jl:44-54) */
int32_t esp_set_nzval(esp_handle *h, const double *nzval);
/* device pointers of the resident CSC (Int64 1-based values), for device consumers; valid until the next esp_flush /
 * esp_reset / esp_set_csc of the handle (a flush that changes the pattern rotates all three arrays) */
int32_t esp_csc_device(esp_handle *h, const int64_t **d_colptr, const int64_t **d_rowval,
                       const double **d_nzval);
/* reset!(ext) (extendable.jl:269-272): empty CSC, empty buffer */
int32_t esp_reset(esp_handle *h);
/* drop the buffer only (a fresh T_ext(m,n), genericextendablesparsematrixcsc.jl:34) */
int32_t esp_clear_pending(esp_handle *h);
/* fdrand!'s zero!(A): nonzeros(A) .= 0 (sprand.jl:82) on the device CSC */
int32_t esp_zero_values(esp_handle *h);
/* dropzeros!(A) on the device CSC (test/test_updates.jl:19,23) */
int32_t esp_dropzeros(esp_handle *h, int64_t *new_nnz);
/* findindex(csc,i,j)+nzval[k] (sparsematrixcsc.jl:7-23) on the device CSC; found=0 if absent */
int32_t esp_getindex(esp_handle *h, int64_t i, int64_t j, double *value, int32_t *found);
/* getindex(buffer,i,j) (sparsematrixlnk.jl:151-171): the value the PENDING entries alone give (i,j) -- their ordered
 * fold -- 0 and found=0 if none creates an entry.  Slow by design (one pass over the pending keys per call); what
 * GenericExtendableSparseMatrixCSC's getindex falls back to for positions not yet in the CSC (genericext...:60-69).
 * More than 2048 pending updates of one position -> ESP_ERR_UNSUPPORTED (flush first). */
int32_t esp_pending_getindex(esp_handle *h, int64_t i, int64_t j, double *value, int32_t *found);
/* stand-in for phash(csc) (sparsematrixcsc.jl:74): a 64-bit function of colptr/rowval only */
int32_t esp_pattern_hash(esp_handle *h, uint64_t *hash);

/* mul!(r, A, x) on the device CSC (abstractextendablesparsematrixcsc.jl:179-181; the coloured loop of
 * genericmtextendablesparsematrixcsc.jl:124-143 visits the columns in the same order): r[i] = the sum of
 * A[i,j]*x[j] over the entries of row i in increasing column order, products and sums rounded
 * separately -- bit-identical to the reference's column loop (no atomics; a row-wise index of the CSC is
 * built on first use after a pattern change).  x has n, r has m elements; on_device != 0: both are
 * device pointers (a consumer that never leaves the GPU); x may be NULL when n == 0 and r when m == 0 (a vector
 * without elements need not have an address).  Pending entries -> ESP_ERR_STATE: flush first.
 *
 * THE HAND-OVER OF DEVICE ARRAYS, here and in every call of this header that takes a device pointer (`on_device != 0`, and
 * the arrays of esp_append_device, esp_append_elements[_again], esp_generate_fem_mesh, esp_shard_export):
 *   - an array needs the NATURAL ALIGNMENT OF ITS ELEMENT TYPE and nothing more (8 bytes for double and int64_t, 4 for int32_t,
 *     1 for uint8_t): a view into the middle of a larger allocation is as good as an allocation of its own.  Where a kernel
 *     uses wider accesses it looks at the pointer first and takes a scalar form otherwise; the results are the same bits;
 *   - an INPUT (a `const` pointer) is never written;
 *   - of an array of n elements only [0, n) is read or written: nothing in front of it, nothing behind it, whatever the
 *     kernels' chunk sizes are.
 * tests/test_device_handover_gpu.py holds every such call to this with arrays at odd offsets between guard bands. */
int32_t esp_mul(esp_handle *h, const double *x, double *r, int32_t on_device);

/* mark_dirichlet(A; penalty) / eliminate_dirichlet!(A, marker) (sparsematrixcsc.jl:97-140) on the device CSC
 * of a square matrix: marker[i] = 1 iff A[i,i] >= penalty; A[:,i] = 0, A[i,:] = 0, A[i,i] = 1 for marked i.
 * marker has n bytes (Julia Vector{Bool}); on_device != 0: a device pointer.  Values only, the pattern stays. */
int32_t esp_mark_dirichlet(esp_handle *h, double penalty, uint8_t *marker, int32_t on_device);
int32_t esp_eliminate_dirichlet(esp_handle *h, const uint8_t *marker, int32_t on_device);

/* set-up of the point preconditioners on the device CSC of a square matrix (pending entries -> ESP_ERR_STATE).
 * esp_jacobi_setup = jacobi(A) (src/factorizations/jacobi.jl:5-12): invdiag[i] = 1 / A[i,i] (Inf where the diagonal
 * is not stored: getindex gives zero).  esp_ilu0_setup = ilu0(A) (src/factorizations/ilu0.jl:8-41): idiag[j] = 1-based
 * index of column j's diagonal entry in rowval/nzval, xdiag[j] = what the reference's loop leaves: 1 / nzval[idiag[j]]
 * (its `xdiag[i] -= ...` updates of rows i > j are overwritten by iteration i); a column without a stored diagonal
 * -> ESP_ERR_INVALID.  n entries each; on_device != 0: device pointers. */
int32_t esp_jacobi_setup(esp_handle *h, double *invdiag, int32_t on_device);
int32_t esp_ilu0_setup(esp_handle *h, double *xdiag, int64_t *idiag, int32_t on_device);

/* ---- the point preconditioners and simple! on the device CSC of a square matrix -----------------------------------
 * An esp_precon is _JacobiPreconditioner / _ILU0Preconditioner (or ILUAMPrecon, below) plus the update! wrapper around them
 * (src/factorizations/jacobi.jl, ilu0.jl), bound to one handle; everything runs on the handle's stream and every call
 * returns synchronised.  Pending entries -> ESP_ERR_STATE (flush first, as update! does); a rectangular matrix ->
 * ESP_ERR_INVALID; nnz or n >= 2^32 - 16 -> ESP_ERR_UNSUPPORTED (32-bit positions and columns, as esp_mul's index).
 * esp_precon_create = jacobi(A) / ilu0(A): ILU0 on a column without a stored diagonal -> ESP_ERR_INVALID, Jacobi gives Inf
 *   there (jacobi.jl:5-12: getindex of a position that is not stored is zero).  The handle refuses esp_destroy
 *   (ESP_ERR_STATE) while a preconditioner bound to it is alive.
 * esp_precon_update = update! (jacobi.jl:54-64, ilu0.jl:120-130): after a pattern change since the last create / update
 *   everything is rebuilt, else the values only (jacobi! / ilu0!).
 * esp_precon_ldiv = ldiv!(u, p, v) (jacobi.jl:36-41, ilu0.jl:66-92), bit-identical; n doubles each, u may equal v;
 *   on_device != 0: device pointers.  Like the reference, whose preconditioner holds A.cscmatrix by reference, ILU0 uses
 *   the CURRENT off-diagonal values with the xdiag of the last update! after an in-place value change (updates of stored
 *   positions, esp_eliminate_dirichlet, esp_set_nzval).  After a pattern change without update! the reference would
 *   still use the old matrix object; here -> ESP_ERR_STATE (update! first). */
typedef struct esp_precon esp_precon;
#define ESP_PRECON_JACOBI 0
#define ESP_PRECON_ILU0 1
int32_t esp_precon_create(esp_handle *h, int32_t kind, esp_precon **out);
int32_t esp_precon_update(esp_precon *p);
int32_t esp_precon_ldiv(esp_precon *p, const double *v, double *u, int32_t on_device);
int32_t esp_precon_destroy(esp_precon *p);
/* ILUAMPreconditioner (src/experimental/ExtendableSparseMatrixParallel/iluam.jl; the loops of ilu_Al-Kurdi_Mittal.jl in the
 * same directory): a real ILU(0) on A's own pattern, bit-identical to the reference's sequential loops.
 * esp_precon_create(h, ESP_PRECON_ILUAM) = iluAM(A) (lines 68-120): nzval = copy(A.nzval); for j = 1:n, for every stored
 *   position v of column j above the diagonal in increasing row i, and every position w of column i below its diagonal whose
 *   row is stored in column j at position k: nzval[k] -= nzval[v]*nzval[w]; then every position of column j below the
 *   diagonal is divided by nzval[diag[j]].  Unit-lower L (scaled, strictly below the diagonal) and U (on and above it).
 *   On the device the columns run level by level (column j after every column i < j with a stored A[i,j]), one kernel
 *   launch per level; a column writes only its own positions and reads only finished columns, so the order inside a level
 *   does not matter.  The analysis (diagonal positions, row parts, three level schedules) runs on the device after a pattern
 *   change only.  A column without a stored diagonal -> ESP_ERR_INVALID (the reference reads an undefined diag[j]); a zero
 *   pivot is no error (Inf / NaN propagate).
 * esp_precon_update: after a pattern change iluAM(A) (iluam.jl:22-31).  DEVIATION: with the pattern kept the reference
 *   calls iluam!, which does not exist (iluAM! at lines 17-66 reads n before defining it and never stores its result); the
 *   device does what was evidently meant: the numeric factorization on the kept analysis.
 * esp_precon_ldiv = ldiv!(x, ILU, b) (lines 160-175 with 122-157): forward y[i] = ((0 - l_ij1*y[j1]) - ...) + b[i], the
 *   stored j < i in INCREASING order; backward x[i] = ((y[i] - u_ij1*x[j1]) - ...)/u_ii, the stored j > i in DECREASING
 *   order, a true division; each level of rows is one launch.  x may alias b (ldiv!(ILU, b)).
 *   The factorization owns a copy of the values: an in-place value change of A without update! does NOT change ldiv!
 *   (unlike ILU0).  A pattern change without update! -> ESP_ERR_STATE.
 * esp_precon_get_factor: the factorization's nnz values in CSC position order (the reference's ILU.nzval), host doubles or,
 *   on_device != 0, device doubles; SPAI answers with the values of M (below); ESP_ERR_INVALID for Jacobi, ILU0 and AMG.
 * esp_precon_levels: out[0..2] = the level counts of the three schedules (factorization columns, forward rows, backward
 *   rows); zeros for the other kinds.
 * esp_precon_launches: read-only; out[2k], out[2k+1] = the wide and the thin kernel launches schedule k runs, in
 *   esp_precon_levels' order.  A level of more than 256 nodes is one wide launch by itself; as many consecutive levels as
 *   together hold at most 256 nodes share one thin, single-workgroup launch.  Block, ILU(k) and Colored answer for the inner
 *   preconditioner; zeros for the other kinds; the errors of esp_precon_levels. */
#define ESP_PRECON_ILUAM 2
int32_t esp_precon_get_factor(esp_precon *p, double *nzval, int32_t on_device);
int32_t esp_precon_levels(esp_precon *p, int64_t out[3]);
int32_t esp_precon_launches(esp_precon *p, int64_t out[6]);
/* test hook, takes effect at the next esp_precon_update (a values-only one is enough: the form is chosen in the numeric phase): which
 * of the two implementations of the column factorization runs -- 0 automatic (the wave form from 24 stored entries per column on
 * average), 1 always a lane per column, 2 always a wave per column.  Results never change, timings do.  Block, ILU(k), Colored, ILUT
 * and LU forward it to their inner ILUAM.  ESP_ERR_INVALID: p == NULL, a form outside 0..2, a kind without an (inner) ILUAM. */
int32_t esp_debug_iluam_form(esp_precon *p, int32_t form);
/* test / inspection, read-only: the form the last numeric factorization ran -- 0 none (n == 0; the prefactored inner ILUAM of ILUT,
 * whatever was forced), 1 lane, 2 wave.  Forwards as esp_debug_iluam_form does, with its errors (and form == NULL). */
int32_t esp_debug_last_iluam_form(esp_precon *p, int32_t *form);
/* BlockPreconditioner (src/factorizations/blockpreconditioner.jl, docs/src/iter.md): the unknowns are split into partitions, every
 * A[part, part] is factorized with Jacobi, ILU0 or ILUAM (inner_kind), and ldiv! solves the partitions independently:
 * u[part] = inner(A[part, part]) \ v[part].  The reference builds np submatrices and runs np factorizations and solves; the device
 * builds ONE matrix B -- exactly the stored entries A[i,j] with part(i) == part(j), explicit zeros, -0.0 and NaN payloads kept
 * bitwise -- and runs ONE inner preconditioner on it: a point factorization of a block-diagonal matrix decouples into the
 * factorizations of its blocks, row by row, the same operations in the same order, so the result is bit-identical to the
 * reference's per-block loops, and ILUAM's level count is the maximum over the blocks instead of their sum.
 *   path 0 (identity: every partition strictly increasing -- ranges and strided ranges, the reference's documented cases): B keeps A's
 *     numbering; ldiv! is exactly the inner kind's launches on v and u: no further launch, copy or scratch.
 *   path 1 (permuted: anything else): B is renumbered by new(i), the position of i in the concatenation of the partitions, every
 *     column sorted by row; ldiv! adds one gather and one scatter through two n-vectors the preconditioner owns.
 * partitions: part_ptr[0..nparts] (part_ptr[0] = 0, non-decreasing, part_ptr[nparts] = n), part_idx[n] 0-based indices that hold
 * every index 0..n-1 exactly once; host arrays, or device arrays when on_device != 0.  The arrays are copied: the caller may free
 * them after the call.  Empty partitions, nparts == 0 with n == 0, and n == 0 are valid.
 * The result is an esp_precon bound to h; esp_precon_update / _ldiv / _destroy, esp_simple, esp_cg and esp_bicgstabl take it
 * unchanged, with the stream use and "returns synchronised" rules of the other kinds.  esp_precon_update after a pattern change of
 * A rebuilds B and the inner preconditioner; with the pattern kept it gathers B's values and runs the inner kind's values-only
 * update (bitwise what a fresh create gives).  esp_precon_get_factor and esp_precon_levels answer for the inner preconditioner (the
 * factor: nnz(B) values in B's position order).
 * VALUE SEMANTICS: the reference factorizes COPIES A[part, part], so ldiv! sees the values as of the last update! -- for ILU0 too.
 * This differs from the unblocked ILU0 above, which reads A's current off-diagonal values.  A pattern change of A without
 * update! -> ESP_ERR_STATE, as for the other kinds.
 * ESP_ERR_INVALID: a rectangular matrix; inner_kind outside the three; nparts < 0; a malformed part_ptr; an index out of range,
 *   repeated or missing (esp_last_error names the first offending one); for ILU0 and ILUAM a column without a stored diagonal (a
 *   block's diagonal is A's).  DEVIATION: the reference only warns when the lengths do not add up to n and then leaves u untouched
 *   there -- undefined memory inside cg.
 * ESP_ERR_STATE: pending entries.  ESP_ERR_UNSUPPORTED: the unblocked kinds' limits; a column window / column shard on h.
 * ESP_ERR_NOMEM leaves A usable, and a failed create or rebuild of B leaves any earlier state of p as it was; once B has been replaced
 * (or its values overwritten by a values-only update!) a failure of the inner update! leaves p refusing ldiv! (ESP_ERR_STATE) until
 * the next good update!, as for the other kinds.  h refuses esp_destroy while the preconditioner lives; esp_precon_destroy releases B, the inner
 * preconditioner and every buffer. */
#define ESP_PRECON_BLOCK 3
int32_t esp_precon_block_create(esp_handle *h, int32_t inner_kind, int64_t nparts, const int64_t *part_ptr, const int64_t *part_idx,
                                int32_t on_device, esp_precon **out);
/* test / inspection: the internal handle holding B (borrowed: read it with esp_get_csc / esp_nnz only); path = 0 identity, 1 permuted */
int32_t esp_precon_block_matrix(esp_precon *p, esp_handle **b, int32_t *path);
/* test hook, takes effect at the next esp_precon_update (which then rebuilds B): 0 automatic, 1 force the permuted path */
int32_t esp_debug_block_path(esp_precon *p, int32_t path);
/* AMGPreconditioner (ext/ExtendableSparseAlgebraicMultigridExt.jl: SA_AMGPreconditioner): a smoothed-aggregation V-cycle.
 * AlgebraicMultigrid.jl is not part of the reference tree, its aggregation is a sequential greedy sweep and its spectral-radius
 * estimate starts from rand: the algorithm here is stated in full, tests/amg_model.c restates it as plain loops
 * and is normative for the order of every operation, and the device result is bit-identical to that model.  In short, level by
 * level from A_0 = a copy of A: dinv = 1/a_ii (esp_jacobi_setup), rho = opnorm(Diagonal(dinv)*A_l, Inf), w = ((4/3)/rho)*dinv;
 * strong edges {i,j} (both entries stored): m = max(|a_ij|, |a_ji|) != 0 and m*m >= (theta*theta)*(|a_ii|*|a_jj|); aggregates = a
 * distance-2 maximal independent set of the strong graph found by Luby rounds over a fixed hash of the index (parallel and
 * reproducible), roots numbered in index order, the other nodes joined in two passes; T[i, agg(i)] = 1; P_l = T + (Diagonal(-w)*A_l)*T
 * and A_{l+1} = transpose(P_l)*(A_l*P_l) by the rules of esp_diag_scale, esp_matmul, esp_add and esp_transpose.  Level l is the
 * coarsest when n_l <= max_coarse, l + 1 == max_levels or the aggregation leaves n_{l+1} == n_l; a coarsest level of at most
 * ESP_AMG_DENSE_MAX unknowns is solved with its dense inverse (Gauss-Jordan, partial pivoting, a zero pivot is no error), a larger
 * one is only smoothed.
 * esp_precon_ldiv = one V-cycle from x = 0: presweeps weighted-Jacobi sweeps x = x + w.*(b - A_l*x) (the first one is x = w.*b),
 *   r = b - A_l*x, b_c = transpose(P_l)*r (esp_mul_transpose's rule), the cycle on level l+1, x = x + P_l*x_c, postsweeps sweeps;
 *   every product A_l*x and P_l*x_c in esp_mul's order.  u may alias v.  With presweeps == postsweeps and a symmetric A the
 *   operator is symmetric (what esp_cg needs).  On device vectors one call is launches on the handle's stream only: no copy, no
 *   allocation, no synchronisation before the end.
 * esp_precon_amg_create: max_levels >= 1, 1 <= max_coarse <= ESP_AMG_DENSE_MAX, presweeps >= 1, postsweeps >= 0, theta >= 0 and
 *   finite; -1 for any of the four integers / a negative theta selects the default: 10, 64, 1, 1, 0.0.  n == 0 and n == 1 are valid.
 *   The result is an esp_precon bound to h; esp_precon_update / _ldiv / _destroy, esp_simple, esp_cg and esp_bicgstabl take it
 *   unchanged, with the stream use and "returns synchronised" rules of the other kinds.
 * esp_precon_update rebuilds the whole hierarchy every time, as the reference's update! does (no values-only form).  The
 *   hierarchy is built from copies: ldiv! sees A as of the last update!; a pattern change of A without update! -> ESP_ERR_STATE.
 * esp_precon_get_factor -> ESP_ERR_INVALID, esp_precon_levels gives zeros; AMG is no inner kind of esp_precon_block_create.
 * ESP_ERR_INVALID: a rectangular matrix; an argument out of range; a column without a stored diagonal (the smallest is named).
 * ESP_ERR_STATE: pending entries.  ESP_ERR_UNSUPPORTED: a column window / column shard on h; n or nnz >= 2^32 - 16; a stored
 *   pattern that is not structurally symmetric (some stored (i,j) without a stored (j,i); the smallest such column is named; only
 *   the pattern is tested, on level 0: convection-diffusion matrices pass).  A stored zero diagonal is no error: Inf / NaN propagate.
 * ESP_ERR_NOMEM from a failed create or rebuild leaves A usable; after a failed rebuild p refuses ldiv! (ESP_ERR_STATE) until the
 *   next good update!.  h refuses esp_destroy while the preconditioner lives.
 * Inspection (tests, tools): the number of levels; per level the BORROWED handles of A_l and P_l (read them with esp_get_csc /
 *   esp_nnz only; P_l is NULL on the coarsest level), n_l, rho_l and the Luby rounds its aggregation took (0 where none ran); the
 *   aggregate of every unknown of a level (n_l int64, 0-based, host or device; ESP_ERR_INVALID for a level that was not
 *   aggregated); the dense inverse of the coarsest level (n_L*n_L doubles, row-major; ESP_ERR_INVALID if it has none). */
#define ESP_PRECON_AMG 4
#define ESP_AMG_DENSE_MAX 512
int32_t esp_precon_amg_create(esp_handle *h, int32_t max_levels, int32_t max_coarse, int32_t presweeps, int32_t postsweeps,
                              double theta, esp_precon **out);
int32_t esp_precon_amg_levels(esp_precon *p, int32_t *nlevels);
int32_t esp_precon_amg_level(esp_precon *p, int32_t level, esp_handle **a, esp_handle **prolong, int64_t *n, double *rho, int32_t *rounds);
int32_t esp_precon_amg_aggregates(esp_precon *p, int32_t level, int64_t *agg, int32_t on_device);
int32_t esp_precon_amg_coarse_inverse(esp_precon *p, double *inv, int32_t on_device);
/* RS_AMGPreconditioner (ext/ExtendableSparseAlgebraicMultigridExt.jl: RS_AMGPreconditioner): the same V-cycle over a hierarchy
 * coarsened the classical (Ruge-Stueben) way, which decides strength per row and so sees the one-directional couplings of upwind
 * convection-diffusion matrices.  AlgebraicMultigrid.jl's splitting is a sequential sweep: the algorithm here is stated in full
 * (DESIGN.md 5k), tests/rsamg_model.c restates it as plain loops and is normative for the order of every operation, and the device
 * result is bit-identical to that model.  Everything of the AMG block above holds -- dinv, rho, w, the checks of level 0, the
 * coarsest level and its dense inverse, the V-cycle -- but for the construction of P_l:
 *   strength: m_i = the largest |a_ik| over the stored k != i; i depends on j (j in S_i) when (i,j) is stored, j != i, |a_ij| != 0
 *     and |a_ij| >= theta*m_i (comparisons with a NaN are false); S_i^T = { j : i in S_j }, lambda_i = |S_i^T|;
 *   splitting (PMIS over the fixed hash): key(i) = min(lambda_i, 65535) << 48 | (mix(i) >> 16) << 32 | i with the 32-bit mixer of
 *     the aggregation's hash; a node with an empty S_i is an F point without interpolation from the start; per round, phase 1 (on
 *     the state of the round's start): an undecided i whose key exceeds that of every undecided node of S_i + S_i^T becomes a C
 *     point, phase 2: a node still undecided with a C point in S_i becomes an F point; until nobody is undecided (at most n
 *     rounds).  C points are numbered in index order (cnum).  Every F point with a non-empty S_i has a C point in S_i;
 *   direct interpolation: row i of P for a C point is P[i, cnum(i)] = 1.0.  For an F point with C_i = S_i & C non-empty, over the
 *     stored k != i of row i in increasing k: sn / sp = the sum of the negative / positive a_ik, snc / spc the same over k in C_i;
 *     d = a_ii; if spc == 0 then d = d + sp and beta = 0, else beta = sp/spc; alpha = snc != 0 ? sn/snc : 0;
 *     P[i, cnum(j)] = (-(a_ij < 0 ? alpha : beta)*a_ij)/d for every j in C_i, stored whatever its value (a zero d is no error);
 *   A_{l+1} = transpose(P_l)*(A_l*P_l) by esp_matmul's rules, P_l being esp_transpose of the transpose one can write down.
 *   Level l is also the coarsest when the splitting leaves no C point or only C points.
 * esp_precon_rsamg_create: the argument rules and error codes of esp_precon_amg_create; -1 / a negative theta selects 10, 64, 1, 1
 *   and theta = 0.25.  The result has kind ESP_PRECON_AMG (esp_precon_amg_coarsening tells the two apart): esp_precon_update / _ldiv
 *   / _destroy, esp_simple, esp_cg, esp_bicgstabl and esp_gmres take it unchanged, and the pattern requirements, the handling of
 *   windows and shards, ESP_ERR_NOMEM and the state rules are those above.
 * Inspection: esp_precon_amg_levels / _level / _coarse_inverse as above (rounds: the rounds of the splitting, 0 where none ran);
 *   esp_precon_amg_splitting: n_l int64 (host or device), the 0-based coarse index of a C point, -1 for an interpolated F point, -2
 *   for an F point without interpolation; ESP_ERR_INVALID for a smoothed-aggregation preconditioner or a level that was not split.
 *   esp_precon_amg_aggregates -> ESP_ERR_INVALID on a Ruge-Stueben preconditioner. */
#define ESP_AMG_COARSEN_SA 0
#define ESP_AMG_COARSEN_RS 1
int32_t esp_precon_rsamg_create(esp_handle *h, int32_t max_levels, int32_t max_coarse, int32_t presweeps, int32_t postsweeps,
                                double theta, esp_precon **out);
int32_t esp_precon_amg_coarsening(esp_precon *p, int32_t *kind);
int32_t esp_precon_amg_splitting(esp_precon *p, int32_t level, int64_t *cf, int32_t on_device);
/* ILUKPreconditioner: the level-of-fill ILU(k), the dialable member of the ILU family (the reference's own dial is the threshold
 * ILUTPreconditioner, docs/src/iter.md, whose pattern depends on the values and whose elimination is sequential -- see
 * esp_precon_ilut_create below for its form by parallel sweeps; ILU(k)'s pattern depends on the structure alone).  Indices 0-based: lev(i,j) = 0 where A stores (i,j) -- a stored 0.0, -0.0 or NaN counts -- and
 * infinite elsewhere; for i = 0..n-1, for k < i in increasing order with lev(i,k) <= K, for j > k with lev(k,j) <= K:
 * lev(i,j) = min(lev(i,j), lev(i,k) + lev(k,j) + 1).  B holds every position with lev <= K: A's bits where lev = 0, +0.0 elsewhere,
 * rows ascending in every column.  esp_precon_iluk_create(h, k) is esp_precon_create(B, ESP_PRECON_ILUAM): ILU(k) of A is ILU(0) of B,
 * so the factorization, the level-scheduled solves and their results are ILUAM's, bit-identical to tests/iluam_model.c applied to the
 * B of tests/iluk_model.c; k = 0 is ESP_PRECON_ILUAM itself, k >= n - 2 the complete LU without pivoting.  ldiv! is ILUAM's on the
 * caller's vectors (no further launch, copy or scratch); esp_simple, esp_cg, esp_bicgstabl and esp_gmres take it as they take ILUAM.
 * The pattern is found on the device by one bounded breadth-first search per column over A (lower part) and over transpose(A)
 * (upper part): one wave per column with a visited set of up to ESP_ILUK_WAVE_VISITS vertices (the column itself, every vertex enqueued
 * and every row emitted as fill; A's own entries do not count, so k = 0 takes any matrix), a workgroup per column up to
 * ESP_ILUK_VISIT_MAX.
 * esp_precon_update: with A's pattern kept one gather (B.nzval[q] = A.nzval[src[q]], +0.0 for fill) and ILUAM's values-only update
 * -- bitwise what a fresh create gives; after a pattern change everything anew.  B holds copies: a value change of A reaches ldiv!
 * only through the update, and a pattern change of A without it is ESP_ERR_STATE.  When an update fails before B is replaced
 * (ESP_ERR_NOMEM, ESP_ERR_UNSUPPORTED) the preconditioner stays what its last good update made it.
 * esp_precon_get_factor and esp_precon_levels answer for the inner ILUAM (nnz(B) values in B's position order).
 * esp_precon_iluk_matrix: B's handle, borrowed and read-only, like esp_precon_block_matrix.  esp_precon_iluk_levels: the level of every
 * stored entry of B, nnz(B) values in B's position order.  esp_precon_iluk_stats: out = nnz(B), the largest stored level, the columns
 * the workgroup search redid (lower part, upper part).
 * ESP_ERR_INVALID: k < 0, a rectangular matrix, a column without a stored diagonal (ILUAM's error, which names it).
 * ESP_ERR_STATE: pending entries.  ESP_ERR_UNSUPPORTED: a column window / column shard on h; n or nnz(B) >= 2^32 - 16; a search that
 * visits more than ESP_ILUK_VISIT_MAX vertices (esp_last_error names the smallest such column and k; refused before B is touched).
 * ILUK is no inner kind of esp_precon_block_create.  A live preconditioner makes h refuse esp_destroy; esp_precon_destroy releases B,
 * the transpose and every buffer. */
#define ESP_PRECON_ILUK 5
#define ESP_ILUK_WAVE_VISITS 512
#define ESP_ILUK_VISIT_MAX 8192
int32_t esp_precon_iluk_create(esp_handle *h, int32_t k, esp_precon **out);
int32_t esp_precon_iluk_matrix(esp_precon *p, esp_handle **b);
int32_t esp_precon_iluk_levels(esp_precon *p, int32_t *lev, int32_t on_device);
int32_t esp_precon_iluk_stats(esp_precon *p, int64_t out[4]);
/* Multicolour ordering (the reference's src/factorizations/parallel_ilu0.jl: graphcol, reordermatrix, reorderlinsys and
 * ParallelILU0Preconditioner).  The reference's colouring draws rand(); the rule here replaces the draw by the fixed hash of the AMG
 * aggregation and the PMIS splitting, which makes it parallel and reproducible.  The rule is normative, tests/coloring_model.c states it
 * as plain loops, and the device result equals that model exactly.
 *   graph     vertices 0..n-1; i and j (i != j) are neighbours when A[i,j] or A[j,i] is stored.  Only the pattern counts: a stored 0.0,
 *             -0.0 or NaN is an entry.  (The pattern of A + transpose(A) in graphcol; the sum is never formed: column i of the CSC
 *             and row i of esp_mul's row-wise index are read.)  No symmetric pattern is required.
 *   priority  key(i) = (uint64)mix(i) << 32 | i with the 32-bit mixer of the aggregation's hash (applied to i + 1).  The keys are
 *             distinct: every comparison is strict.
 *   rounds    r = 1, 2, ...: U = the vertices without a colour at the start of the round; i in U receives colour r iff
 *             key(i) > key(j) for every neighbour j in U.  The colouring ends when U is empty.  (indset / graphcol with the fixed key in
 *             place of rand(lenW) and > in place of >=.)  The vertex with the largest key of U is always chosen: at most n rounds.
 *   result    ncolors = the number of rounds; color[i] is 0-based; the permutation c = the vertices sorted by (colour, index), the
 *             reference's flatten(coloring); color_ptr[0..ncolors] delimits the colours in c.
 * On the device a round is one launch on the handle's stream and one counter read back, the Luby / PMIS shape: one lane per uncoloured
 * vertex (a vertex whose column or row holds more than 32 entries is folded by its whole wave), the vertices a round leaves uncoloured
 * are the next round's list.  Rounds are separated by kernel boundaries and by nothing else: no flag is polled across workgroups,
 * there is no grid barrier and no persistent kernel.  The permutation comes from stable radix passes over the colour bits.
 * esp_graph_coloring: the colouring of a flushed square matrix without a preconditioner: *ncolors, and color[n] (int64, 0-based; host,
 *   or device when on_device != 0; may be NULL).  The checks are esp_precon_colored_create's.
 * esp_precon_colored_create(h, inner_kind): inner_kind is ESP_PRECON_ILU0 or ESP_PRECON_ILUAM.  The kind colours A, builds
 *   B = A[c,c] (B[k,l] = A[c[k],c[l]]: every column sorted by row, the values bitwise A's) in an internal handle and creates the inner
 *   kind on B.  No two unknowns of one colour are coupled, so a row of colour r meets only rows of colours < r in B's strictly lower
 *   part and only rows of colours > r in its strictly upper part: every level schedule of ILUAM on B has at most ncolors levels.
 *   esp_precon_ldiv is u[c] = inner(B) \ v[c]: one gather, the inner kind's own launches, one scatter; u may alias v.  It is exactly
 *   esp_precon_block_create's permuted path over the single partition c, whose builder, value gather and vector kernels it runs; the
 *   permutation stays on the device.  The result is an esp_precon bound to h; esp_precon_update / _ldiv / _destroy, esp_simple, esp_cg,
 *   esp_bicgstabl and esp_gmres take it unchanged.
 *   DEVIATION: the reference's ParallelILU0Preconditioner(A) preconditions the REORDERED system -- its ldiv! takes vectors in the
 *   coloured numbering and the caller runs reorderlinsys first.  This one acts in A's numbering: a drop-in Pl for A.
 * esp_precon_update: with A's pattern kept one gather of B's values and the inner values-only update (the colouring, B's pattern and
 *   ILUAM's analysis are kept; bitwise what a fresh create gives); after a pattern change the colouring, B and the inner preconditioner
 *   anew.  B holds copies, for ILU0 too (the block kind's value semantics): a value change of A reaches ldiv! only through the update,
 *   and a pattern change of A without it is ESP_ERR_STATE.  A rebuild that fails before B is replaced leaves the earlier state usable.
 * esp_precon_get_factor and esp_precon_levels answer for the inner preconditioner (nnz(B) values in B's position order).
 * Inspection: esp_precon_colored_info: out = ncolors, nnz(B).  esp_precon_colored_colors: color[n] (int64, 0-based).
 *   esp_precon_colored_perm: c[n] (int64, 0-based).  Both host, or device when on_device != 0.  esp_precon_colored_matrix: B's handle,
 *   borrowed and read-only, like esp_precon_block_matrix.
 * ESP_ERR_INVALID: a rectangular matrix; inner_kind outside the two; a column without a stored diagonal (the inner kind's error; it names
 *   the column of B, the position in c).  ESP_ERR_STATE: pending entries.  ESP_ERR_UNSUPPORTED: a column window / column shard on h; the
 *   preconditioners' 32-bit limits.  n == 0 is valid.  ILU(k) and AMG are no inner kinds.  A live preconditioner makes h refuse
 *   esp_destroy; esp_precon_destroy releases B, the inner preconditioner and every buffer. */
#define ESP_PRECON_COLORED 6
int32_t esp_graph_coloring(esp_handle *h, int64_t *ncolors, int64_t *color, int32_t on_device);
int32_t esp_precon_colored_create(esp_handle *h, int32_t inner_kind, esp_precon **out);
int32_t esp_precon_colored_info(esp_precon *p, int64_t out[2]);
int32_t esp_precon_colored_colors(esp_precon *p, int64_t *color, int32_t on_device);
int32_t esp_precon_colored_perm(esp_precon *p, int64_t *c, int32_t on_device);
int32_t esp_precon_colored_matrix(esp_precon *p, esp_handle **b);
/* SPAIPreconditioner: the sparse approximate inverses SPAI-0 and SPAI-1 (the relaxations `spai0` and `spai1` of the reference's
 * AMGCL_RLXPreconditioner, ext/ExtendableSparseAMGCLWrapExt.jl; AMGCLWrap is not part of the reference tree, so the algorithm below
 * is normative, tests/spai_model.c states it as plain loops, and the device equals that model bit for bit).  M ~ inv(A) minimises
 * |I - A*M|_F over the pattern of A, one column at a time from independent small least-squares problems: no ordering, no levels, no
 * colouring, and ldiv! is one sparse product.  Indices 0-based; no FMA contraction anywhere; sqrt and / correctly rounded.  Column k:
 *   1. J = the stored rows of column k of A, ascending: the unknowns of column k of M, q = |J|.  M stores exactly A's positions
 *      (a stored 0.0, -0.0 or NaN counts as an entry): colptr and rowval of M are A's.
 *   2. I = the ascending union of the stored rows of the columns j in J, p = |I|.
 *   3. B = A[I, J], dense p x q: A's bits where stored, +0.0 elsewhere.
 *   4. osum, the ordered sum of p terms: part[l], l = 0..63, adds the terms with local row r = l, l + 64, ... in increasing r,
 *      starting from the first one (+0.0 where there is none); then for s = 32, 16, 8, 4, 2, 1: part[l] = part[l] + part[l + s] for
 *      l < s; the result is part[0].
 *   5. modified Gram-Schmidt, c = 0..q-1 in order: R[c][c] = sqrt(osum_r B[r][c]*B[r][c]); B[r][c] = B[r][c] / R[c][c]; for every
 *      d > c: R[c][d] = osum_r B[r][c]*B[r][d], then B[r][d] = B[r][d] - R[c][d]*B[r][c].
 *   6. y[c] = B[pos][c] of the normalised columns where I[pos] == k; +0.0 where k is not in I.
 *   7. back substitution, c = q-1..0: t = y[c]; for d = c+1..q-1 ascending t = t - R[c][d]*m[d]; m[c] = t / R[c][c].
 *   8. the values of column k of M are m[0..q-1].
 *   A zero or NaN pivot is no error: Inf and NaN propagate (a rank-deficient local problem, an empty row set, p < q).  A column
 *   without a stored diagonal is valid; an empty column stays empty.
 * order = 0, SPAI-0, is the diagonal member: m_k = a_kk / osum(a*a over the stored entries of column k), a_kk = +0.0 where the
 *   diagonal is not stored; an n-vector, applied as Jacobi's invdiag is.
 * symmetric != 0 (order 1 only) replaces M by 0.5*(M + transpose(M)), formed by esp_transpose, esp_add and esp_diag_scale on
 *   internal handles (their rules: a sum that is zero is not stored); bitwise symmetric, the form esp_cg needs.
 * On the device a size pass finds p of every column (the sorted union in LDS) and sorts the columns into tiers before M is touched:
 *   one wave per column with B, R and I in LDS while p*q <= ESP_SPAI_WAVE_DOUBLES (and q*q <= ESP_SPAI_WAVE_DOUBLES, which p >= q
 *   implies); one workgroup of eight waves per listed column with B and I in LDS and R in a scratch slot of device memory up to
 *   p*q <= ESP_SPAI_DENSE_MAX, the waves taking the independent columns d > c in turn, each with the wave form's sum: both tiers
 *   give the same bits.  A column with p*q > ESP_SPAI_DENSE_MAX -> ESP_ERR_UNSUPPORTED before anything of the preconditioner
 *   changes; esp_last_error names the smallest such column with its p and q (p as a lower bound, marked ">=", where the lists of
 *   the column hold more than 16384 rows together).
 * esp_precon_spai_create(h, order, symmetric): the result is an esp_precon bound to h; esp_precon_update / _ldiv / _destroy,
 *   esp_simple, esp_cg, esp_bicgstabl and esp_gmres take it unchanged.
 * esp_precon_ldiv: u = M*v in esp_mul's order on M's internal handle, on h's stream; no allocation, no synchronisation inside the
 *   solvers; u may alias v (one copy through an n-vector the preconditioner owns).  order 0: u = m.*v.
 * esp_precon_update: with A's pattern kept only the numeric kernels run on the kept p, tiers and pattern of M -- bitwise what a
 *   fresh create gives (symmetric: the three algebra calls run again); after a pattern change everything anew.  M holds results: a
 *   value change of A reaches ldiv! only through the update; a pattern change of A without it -> ESP_ERR_STATE.  An update that is
 *   refused (ESP_ERR_UNSUPPORTED, ESP_ERR_NOMEM in the set-up) leaves the preconditioner what its last good update made it.
 * esp_precon_get_factor: the values of the applied M in its position order (order 0: the n diagonal values); esp_precon_levels and
 *   esp_precon_launches give zeros.  esp_precon_spai_matrix: the applied M's handle, borrowed and read-only, like
 *   esp_precon_block_matrix; order 0 -> ESP_ERR_INVALID.  esp_precon_spai_stats: out = max p, max q, max p*q, the columns the
 *   workgroup tier handled (zeros for order 0).
 * ESP_ERR_INVALID: a rectangular matrix, order outside {0, 1}, symmetric with order 0.  ESP_ERR_STATE: pending entries.
 * ESP_ERR_UNSUPPORTED: a column window / column shard on h; n or nnz >= 2^32 - 16; a too-large column.  n == 0 and n == 1 are
 * valid.  SPAI is no inner kind of esp_precon_block_create or esp_precon_colored_create.  A live preconditioner makes h refuse
 * esp_destroy; esp_precon_destroy releases M, its internal handles and every buffer. */
#define ESP_PRECON_SPAI 7
#define ESP_SPAI_WAVE_DOUBLES 512
#define ESP_SPAI_DENSE_MAX 12288
int32_t esp_precon_spai_create(esp_handle *h, int32_t order, int32_t symmetric, esp_precon **out);
int32_t esp_precon_spai_matrix(esp_precon *p, esp_handle **m);
int32_t esp_precon_spai_stats(esp_precon *p, int64_t out[4]);
/* ILUTPreconditioner (ext/ExtendableSparseIncompleteLUExt.jl; docs/src/iter.md builds ILUTPreconditioner(; droptol = 1.0e-2)): a
 * threshold ILU.  IncompleteLU.jl is not part of the reference tree and its row-by-row elimination is sequential with a pattern that
 * depends on the values, so the algorithm here is stated in full: the ParILUT family of Anzt, Chow and Dongarra --
 * the factorization as the fixed point of l_ij = (a_ij - sum_{k<j} l_ik u_kj)/u_jj, u_ij = a_ij - sum_{k<i} l_ik u_kj, every entry
 * updated at once from the previous values, candidates added and small entries dropped between sweeps.  tests/ilut_model.c restates
 * it entry by entry and is normative; the device result is bit-identical to it.
 *   state   A is n x n and stores every diagonal entry (a stored 0.0, -0.0 or NaN counts).  A pattern S containing the diagonal and
 *           values F on it: strictly below the diagonal the unit-lower L, scaled; on and above it U; rows ascending in every column.
 *   init    S = pattern(A); u_ij = a_ij for i <= j, l_ij = a_ij / a_jj for i > j.
 *   sweep   on a pattern P, synchronous (F_old read, F_new written): for every (i,j) in P, r = a_ij (+0.0 where A stores nothing);
 *           for every k < min(i,j) with (i,k) and (k,j) in P, k increasing: r = r - l_ik*u_kj (the product rounded first, no fused
 *           multiply-add); then l_ij = r / u_jj(old) for i > j, u_ij = r for i <= j.
 *   step    1. C = pattern((L+I)*U), structural (it contains S); 2. F carried to C, +0.0 at the new positions; 3. nnz(C) >
 *           (int64)(max_fill*nnz(A)) -> ESP_ERR_UNSUPPORTED (esp_last_error names the step and both counts; the preconditioner stays
 *           as its last good update! made it); 4. `sweeps` sweeps on C; 5. every off-diagonal (i,j) is dropped for which
 *           fabs(l_ij) < droptol is true (i > j) or fabs(u_ij) < droptol*fabs(u_ii) is true (i < j) -- a NaN is kept, positions A
 *           stores are droppable like any other, the diagonal never goes; 6. S = what is left; 7. `sweeps` sweeps on S.
 *   esp_precon_ilut_create runs init and `steps` steps (steps = 0: `sweeps` sweeps on pattern(A)).  The upper part is measured against
 *   its row's pivot so that for symmetric A the rule is symmetric (u_ij/u_ii = l_ji at the fixed point).  On a fixed pattern the
 *   values stop changing after at most 2n sweeps, and the fixed point is bit for bit ILUAM's factorization of the matrix holding A's
 *   values on the pattern and +0.0 elsewhere (the subtraction order is iluAM's).  DEVIATION from IncompleteLU.jl's ilu(A; tau):
 *   that rule drops against tau times the norm of A's column or row during a sequential elimination.
 * ldiv! is ILUAM's forward and backward level-scheduled solve over (S, F) on the caller's vectors (u may be v; no further launch,
 * copy or scratch); esp_simple, esp_cg, esp_bicgstabl and esp_gmres take it as they take ILUAM.  esp_precon_get_factor gives F
 * (nnz(S) values in S's position order), esp_precon_levels the forward and backward level counts (the factor schedule does not
 * exist: 0).
 * esp_precon_update: after a pattern change of A, and with keep_pattern == 0 always (S depends on the values), the whole
 * construction.  With A's pattern kept and keep_pattern != 0: S and every index structure stay, F starts from its CURRENT values,
 * A's new values are read and `sweeps` sweeps run on S (the state is carried by the model too, so any sequence of updates is
 * defined).  A pattern change of A without update! -> ESP_ERR_STATE from ldiv! and the solvers.
 * The sweep kernel serves a column with one wave while at most ESP_ILUT_WAVE_UPPER rows lie above its diagonal (they are staged in
 * LDS), with one workgroup up to ESP_ILUT_GROUP_UPPER, and by lanes striding the column in global memory beyond: no column is
 * refused.  esp_precon_ilut_limits: out = ESP_ILUT_WAVE_UPPER, ESP_ILUT_GROUP_UPPER, ESP_ILUT_STEPS_MAX, ESP_ILUT_STATS.
 * esp_precon_ilut_matrix: the internal handle holding S with F as its values, borrowed and read-only (esp_get_csc / esp_nnz).
 * esp_precon_ilut_stats: out[0] = steps, out[1] = the sweeps the last update! ran, out[2..4] = the columns of S the wave / workgroup /
 * stride tier serves, out[5] = nnz(S), out[8 + 2 t], out[9 + 2 t] = nnz(C), nnz(S) of step t (the rest 0).
 * ESP_ERR_INVALID: droptol < 0 or NaN, steps < 0 or > ESP_ILUT_STEPS_MAX, sweeps < 1, max_fill < 1 or NaN, a rectangular matrix, a
 * column without a stored diagonal.  ESP_ERR_STATE: pending entries.  ESP_ERR_UNSUPPORTED: a column window / column shard on h; the
 * fill guard; n or nnz >= 2^32 - 16.  ILUT is no inner kind of esp_precon_block_create or esp_precon_colored_create.  A live
 * preconditioner makes h refuse esp_destroy; esp_precon_destroy releases F, the work handles and every buffer. */
#define ESP_PRECON_ILUT 8
#define ESP_ILUT_WAVE_UPPER 256
#define ESP_ILUT_GROUP_UPPER 4096
#define ESP_ILUT_STEPS_MAX 16
#define ESP_ILUT_STATS 40
int32_t esp_precon_ilut_create(esp_handle *h, double droptol, int32_t steps, int32_t sweeps, double max_fill, int32_t keep_pattern,
                               esp_precon **out);
int32_t esp_precon_ilut_matrix(esp_precon *p, esp_handle **f);
int32_t esp_precon_ilut_stats(esp_precon *p, int64_t out[ESP_ILUT_STATS]);
int32_t esp_precon_ilut_limits(int64_t out[4]);
/* LUFactorization and `A \ b` (src/factorizations/umfpack_lu.jl, sparspak.jl; docs/src/linearsolve.md): a sparse LU WITHOUT pivoting.
 * The reference wraps UMFPACK / Sparspak, which are not part of its tree, so the algorithm is stated in full here and in DESIGN.md 5q:
 * a nested-dissection ordering found on the device, a supernodal symbolic factorization that predicts a superset of the fill from the
 * dissection tree alone, and ILUAM's factorization and level-scheduled solves on the filled, reordered matrix B.  tests/lu_model.c
 * restates it as plain loops and is normative; the device equals it bit for bit.  Indices 0-based.
 *   graph       i and j (i != j) are neighbours when A[i,j] or A[j,i] is stored: the colouring's graph (a stored 0.0, -0.0 or NaN is an
 *               entry, the sum A + transpose(A) is never formed, no symmetric pattern is required).  key(i) is the colouring's key:
 *               distinct, every comparison strict.
 *   dissection  d = 0, one remaining part holding every vertex.  A round: 1. the connected components of every remaining part; the
 *               root of a component is its vertex with the largest key; anc[v][d] = the root of v's component for every vertex still
 *               unplaced.  2. a component C is a leaf of depth d when |C| <= leaf_size, or d == max_depth, or the eccentricity of
 *               step 3 is below 2; every vertex of a leaf gets level[v] = d.  3. every other component: dist0 = the breadth-first
 *               distances inside C from its root, e0 their maximum, r1 = the vertex with dist0 == e0 of the largest key, dist = the
 *               distances inside C from r1, ecc their maximum; with ecc >= 2 and mid = (ecc + 1) div 2 the vertices with dist == mid
 *               are C's separator and get level[v] = d, {dist < mid} and {dist > mid} are remaining parts of depth d + 1 (an edge joins
 *               equal or adjacent distances only: the separator separates).  4. d = d + 1; stop when no part remains.
 *   tree        a node is a pair (d, root): the vertices with level == d and anc[.][d] == root -- a leaf, or the separator of a split
 *               component.  The nodes (e, anc[v][e]), e < level[v], are v's ancestors.  c = the vertices sorted by (level descending,
 *               anc[v][level[v]] ascending, index ascending): every node is contiguous in c, every ancestor behind its descendants.
 *   fill        for an edge (u, v) with level[v] < level[u], v belongs to struct of the node (e, anc[u][e]) for every e with
 *               level[v] < e <= level[u]: struct(K) = the vertices of K's ancestors next to K or to a descendant of K.  In positions of
 *               c, column u of L holds the vertices of u's node from u on (a dense diagonal block) and struct(node(u)).  B's pattern
 *               is L + transpose(L); B[k,l] = A[c[k],c[l]] bitwise where stored, +0.0 elsewhere, rows ascending.  The pattern contains
 *               the fill of P*A*transpose(P), so ILU(0) of B is the exact LU; entries outside the true fill stay +-0.0.
 *   numerics    esp_precon_create(B, ESP_PRECON_ILUAM), unchanged.  esp_precon_ldiv is u[c] = ILUAM(B) \ v[c]: the coloured kind's gather,
 *               inner solve and scatter; u may alias v.  No pivoting (a zero or NaN pivot propagates as in ILUAM), no refinement;
 *               esp_simple with this kind is iterative refinement.  DEVIATION: the order is the one above, not AMD / MMD / COLAMD.
 * On the device the components (the largest key spreads, every vertex at once from the labels of the launch before) and the searches
 * (an unplaced vertex without a distance that has a neighbour at distance step - 1 takes distance step) run over all components at
 * once, one lane per vertex, a vertex whose column or row holds more than 32 entries folded by its whole wave; the maxima per
 * component go through atomics on arrays indexed by the root vertex.  A step is one launch on the handle's stream and one counter
 * read back; steps are separated by kernel boundaries and by nothing else.  c comes from stable radix passes; the struct lists from
 * an ESP_COO flush of a scratch handle (the nodes as columns) and its transpose; B's columns are written in order by one wave each.
 * esp_nested_dissection: the ordering of a flushed square matrix without a factorization: c[n] (int64) and level[n] (int32), host, or
 *   device when on_device != 0; either may be NULL.  The checks are esp_precon_lu_create's.
 * esp_precon_lu_create(h, leaf_size, max_depth): the result is an esp_precon bound to h; esp_precon_update / _ldiv / _destroy,
 *   esp_simple, esp_cg, esp_bicgstabl and esp_gmres take it unchanged; esp_precon_get_factor / _levels / _launches answer for the inner
 *   ILUAM (nnz(B) values in B's position order).
 * esp_precon_update: with A's pattern kept one gather of B's values and ILUAM's values-only update (the ordering, the tree, B's pattern
 *   and the schedules are kept; bitwise what a fresh create gives); after a pattern change everything anew.  B holds copies: a value
 *   change of A reaches ldiv! only through the update, a pattern change of A without it is ESP_ERR_STATE.  A rebuild that fails before
 *   B is replaced leaves the earlier state usable.
 * Inspection: esp_precon_lu_perm: c[n] (int64).  esp_precon_lu_tree: level[n] (int32) and node_root[n] (int64, anc[v][level[v]]), per
 *   vertex; either may be NULL.  All host, or device when on_device != 0.  esp_precon_lu_matrix: B's handle, borrowed and read-only.
 *   esp_precon_lu_stats: out = nnz(B), the rounds, the deepest level, the nodes, the component and search launches this object has
 *   run since its create (an update! with the pattern kept adds none), the largest node.
 * ESP_ERR_INVALID: a rectangular matrix; leaf_size < 1; max_depth outside 0..64; a column of B whose diagonal A does not store
 *   (ILUAM's condition; the message names the column of B, the position in c, and A's column).  ESP_ERR_STATE: pending entries.
 *   ESP_ERR_UNSUPPORTED: a column window / column shard on h; n or nnz(B) >= 2^32 - 16 -- nnz(B) is known from the count pass: refused
 *   before B is allocated, esp_last_error gives nnz(B) (esp_debug_lu_fill_cap(h, cap) lowers that limit for the factorizations created
 *   on h afterwards, a test hook; 0 restores it).  n == 0 is valid.  LU is no inner kind of esp_precon_block_create or
 *   esp_precon_colored_create.  A live factorization makes h refuse esp_destroy; esp_precon_destroy releases B, the inner
 *   preconditioner and every buffer.
 * esp_precon_lu_create_form(h, leaf_size, max_depth, form): form ESP_LU_COLUMNS is esp_precon_lu_create, unchanged.  ESP_LU_PANELS is a
 *   second schedule of the SAME numerics on dense panels per tree node; any other form is ESP_ERR_INVALID.  The rule: the
 *   ordering, the tree, B (built as above: the missing-diagonal refusal, the fill guard, esp_precon_lu_matrix and the values-only
 *   gather are the column form's) and every bit of the factor and of ldiv! are those of the column form, because ILUAM's factorization
 *   of B is one fixed chain per entry (k, j) of B's pattern: t = b_kj; for every i < min(k, j) ascending with (i, j) and (k, i) in B's
 *   pattern: t = t - u_ij*l_ki (the product rounded, then the difference); k > j: l_kj = t / u_jj, a true division.  (i, j) and (k, i)
 *   lie in the pattern exactly when i belongs to a descendant J with j and k in node(J) + struct(J), or to the entry's own node: the
 *   panel form walks these chains node by node from the deepest depth up.  Node K (width w, h = |struct(K)|) owns two column-major
 *   (w + h) x w panels, PL[r, j] = B[row r, K_j] for r >= j and PU[r, j] = B[K_j, row r] for r > j: twice CholeskyFactorization's memory.
 *   A load kernel scatters B's values into the zeroed panels; per depth the nodes narrower than the wide-form width (default 33) are
 *   finished by one workgroup each in one launch, the others block column by block column (32 columns), two launches per block column;
 *   plain FP64 multiplies and subtractions, no matrix instructions, no pivot test (a zero or NaN pivot propagates as in ILUAM).  The
 *   solves are ILUAM's orders on the panels: forward acc = 0, the stored k < j ascending, the right-hand side added last; backward
 *   acc = y_j, the stored i > j DESCENDING, the division last.  esp_precon_ldiv only enqueues launches: a gather, at most 4 per depth,
 *   a scatter.  The object is an ESP_PRECON_LU one: esp_precon_update / _ldiv / _destroy, esp_simple, esp_cg, esp_bicgstabl, esp_gmres,
 *   esp_precon_lu_perm / _tree / _matrix / _stats take it unchanged.  esp_precon_get_factor gives nnz(B) doubles in B's position order
 *   exported from the panels (bitwise the column form's); esp_precon_levels / _launches give zeros (there is no inner ILUAM, no level
 *   analysis and no schedule), esp_debug_iluam_form / esp_debug_last_iluam_form -> ESP_ERR_INVALID.  esp_precon_update with A's pattern
 *   kept: the values gather of B, the load kernel and the numeric factorization (no ordering launch; bitwise a fresh create).
 * esp_precon_lu_panel_stats: out = the panel doubles allocated, the launches of the last numeric factorization, the launches of one
 *   ldiv!, the nodes taken by the small and by the wide form, the block-column steps of the wide form (per depth the block columns of
 *   its widest wide node, summed).  ESP_ERR_INVALID on a column-form object.
 * esp_debug_lu_wide_from(h, w): a test hook; the panel-form factorizations created on h afterwards use the wide form from width w on
 *   (0 restores the default). */
#define ESP_PRECON_LU 9
#define ESP_LU_COLUMNS 0
#define ESP_LU_PANELS 1
#define ESP_LU_PANEL_STATS 6
int32_t esp_precon_lu_create(esp_handle *h, int32_t leaf_size, int32_t max_depth, esp_precon **out);
int32_t esp_precon_lu_create_form(esp_handle *h, int32_t leaf_size, int32_t max_depth, int32_t form, esp_precon **out);
int32_t esp_precon_lu_panel_stats(esp_precon *p, int64_t out[ESP_LU_PANEL_STATS]);
int32_t esp_debug_lu_wide_from(esp_handle *h, int64_t w);
int32_t esp_precon_lu_perm(esp_precon *p, int64_t *c, int32_t on_device);
int32_t esp_precon_lu_tree(esp_precon *p, int32_t *level, int64_t *node_root, int32_t on_device);
int32_t esp_precon_lu_matrix(esp_precon *p, esp_handle **b);
int32_t esp_precon_lu_stats(esp_precon *p, int64_t out[6]);
int32_t esp_nested_dissection(esp_handle *h, int32_t leaf_size, int32_t max_depth, int64_t *c, int32_t *level, int32_t on_device);
int32_t esp_debug_lu_fill_cap(esp_handle *h, int64_t cap);
/* CholeskyFactorization (src/factorizations/cholmod_cholesky.jl; test/test_default_cholesky.jl): A[c,c] = L*transpose(L) on the
 * device, on dense column-major panels per node of LUFactorization's dissection tree.  The reference wraps CHOLMOD, which is not part
 * of its tree: the rule is stated in full here and in DESIGN.md 5r; tests/cholesky_model.c restates it as plain loops and is normative;
 * the device equals it bit for bit.  Indices 0-based.
 *   input     as Symmetric(A.cscmatrix) does, only stored entries A[r,s] with r <= s are read; the strict lower triangle of A is never
 *             read.  Its pattern still takes part in the graph (above), which gives a superset.
 *   ordering  c, level, the nodes and struct(K) are LUFactorization's for the same leaf_size / max_depth.
 *   pattern   in positions of c, column j of L has the rows pat(j) = the positions of node(j) from j on, then struct(node(j)),
 *             ascending: the lower half of B.
 *   values    a_ij for i >= j in pat(j) is the bits of the stored A[min(c[i],c[j]), max(c[i],c[j])]; an entry that is not stored is
 *             +0.0 (a missing diagonal therefore fails the pivot test and is no error of its own).
 *   factor    every entry is one chain, each product rounded, then each difference rounded (no contraction): t = a_ij; for every
 *             k < j ascending with i in pat(k) and j in pat(k): t = t - l_ik*l_jk; i == j: the column fails when !(t > 0), else
 *             l_jj = sqrt(t) correctly rounded; i > j: l_ij = t / l_jj, a true division.
 *   failure   the factorization reports the smallest position j whose pivot fails and A's column c[j]: ESP_ERR_NOTPOSDEF (the chain
 *             is fixed, so j does not depend on the schedule).
 *   solve     y = v[c].  Forward, j ascending: t = y_j; for k < j ascending with j in pat(k): t = t - l_jk*y_k; y_j = t / l_jj.
 *             Backward, j descending: t = y_j; first for i in struct(node(j)) ascending: t = t - l_ij*x_i; then for the positions
 *             i > j of node(j) DESCENDING: t = t - l_ij*x_i; x_j = t / l_jj (a node's triangle can then run right-looking, one lane
 *             per row).  u[c] = x; u may alias v.
 * Any schedule that respects these chains gives the same bits.  The device walks the tree depth by depth, from the deepest nodes to
 * depth 0 (nodes of equal depth are independent: a chain only reaches into a node's own descendants): a load kernel scatters A's
 * upper triangle into the zeroed panels; per depth, the nodes narrower than the wide-form width (default 33) are finished by one
 * workgroup each in one launch (the small form), the others block column by block column (32 columns) for all of them at once, two
 * launches per block column with the tiles spread over the grid (the wide form); plain FP64 multiplies and subtractions, no matrix
 * instructions.  A failing pivot goes to one device word by atomicMin, read back once after the last depth.
 * esp_precon_cholesky_create(h, leaf_size, max_depth): the result is an esp_precon bound to h; esp_precon_update / _ldiv / _destroy,
 *   esp_simple, esp_cg, esp_bicgstabl and esp_gmres take it unchanged; esp_precon_get_factor -> ESP_ERR_INVALID, esp_precon_levels /
 *   _launches give zeros (as for AMG).  esp_precon_ldiv only enqueues launches: a gather, at most 4 per depth, a scatter.
 * esp_precon_update: with A's pattern kept the load kernel and the numeric factorization alone (the ordering, the tree, the tables and
 *   the panels' layout are kept; bitwise what a fresh create gives); after a pattern change everything anew.  The panels hold copies: a
 *   value change of A reaches ldiv! only through the update, a pattern change of A without it is ESP_ERR_STATE.  After an update that
 *   fails (ESP_ERR_NOTPOSDEF included) the object refuses ldiv! with ESP_ERR_STATE until an update succeeds.
 * Inspection: esp_precon_cholesky_perm / _tree: as esp_precon_lu_perm / _tree.  esp_precon_cholesky_factor: L as a CSC in positions of c
 *   (colptr[n + 1] and rowval[nnz(L)] int64, 1-based; nzval[nnz(L)]), host, or device when on_device != 0; any pointer may be NULL.
 *   esp_precon_cholesky_stats: out = nnz(L), the rounds, the deepest level, the nodes, the largest node, the panel doubles allocated,
 *   the ordering launches since the create (an update! with the pattern kept adds none), the launches of the last numeric
 *   factorization, the launches of one ldiv!, the nodes taken by the small and by the wide form, the block-column steps of the wide
 *   form (per depth the block columns of its widest wide node, summed).
 *   esp_debug_cholesky_wide_from(h, w): a test hook; the factorizations created on h afterwards use the wide form from width w on
 *   (0 restores the default).
 * ESP_ERR_INVALID: a rectangular matrix; leaf_size < 1; max_depth outside 0..64.  ESP_ERR_STATE: pending entries.
 *   ESP_ERR_UNSUPPORTED: a column window / column shard on h; n >= 2^32 - 16.  n == 0 is valid.  Cholesky is no inner kind of
 *   esp_precon_block_create or esp_precon_colored_create.  A live factorization makes h refuse esp_destroy. */
#define ESP_PRECON_CHOLESKY 10
#define ESP_CHOL_STATS 12
int32_t esp_precon_cholesky_create(esp_handle *h, int32_t leaf_size, int32_t max_depth, esp_precon **out);
int32_t esp_precon_cholesky_perm(esp_precon *p, int64_t *c, int32_t on_device);
int32_t esp_precon_cholesky_tree(esp_precon *p, int32_t *level, int64_t *node_root, int32_t on_device);
int32_t esp_precon_cholesky_factor(esp_precon *p, int64_t *colptr, int64_t *rowval, double *nzval, int32_t on_device);
int32_t esp_precon_cholesky_stats(esp_precon *p, int64_t out[ESP_CHOL_STATS]);
int32_t esp_debug_cholesky_wide_from(esp_handle *h, int64_t w);
/* simple!(u, A, b; abstol, reltol, maxiter, Pl = p) (src/factorizations/simple_iteration.jl:21-45) statement by
 * statement: res = A*u - b; then per step ldiv!(upd, Pl, res), u .-= upd, mul!(res, A, u), res .-= b, r = norm(res),
 * stop when (r / r0) < reltol || r < abstol (literally: r0 = 0 gives NaN or Inf there).  u (in/out) is bit-identical to
 * the reference loop for any number of steps run (mul! as esp_mul).  norm is a fixed-order sum of squares (identical run to
 * run) rather than BLAS nrm2: history and the stopping step agree with the reference to rounding of the norm only, and the
 * sum of squares overflows for residual entries above about 1e154, where nrm2 would not.  history: maxiter+1 host doubles
 * or NULL; *iterations = number of ldiv! steps taken (history holds iterations+1 norms).  b, u: n doubles; on_device != 0:
 * device pointers.  p must be bound to h. */
int32_t esp_simple(esp_handle *h, esp_precon *p, const double *b, double *u, int32_t on_device, int64_t maxiter,
                   double abstol, double reltol, double *history, int64_t *iterations);
/* cg / cg!(x, A, b; Pl = p, abstol, reltol, maxiter, initially_zero) of IterativeSolvers.jl (its preconditioned iterator,
 * restated from the package's documented behaviour: the package is not part of the reference tree) on the device CSC:
 *   u = 0; rho = 1; r = b (initially_zero != 0: x is taken to hold zeros) or r = b - A*x; residual = norm(r);
 *   tol = max(reltol*residual, abstol); then, while fewer than maxiter iterations ran and not residual <= tol:
 *   c = Pl \ r; rho_prev = rho; rho = dot(c, r); beta = rho/rho_prev; u = c + beta*u; c = A*u; alpha = rho/dot(u, c);
 *   x = x + alpha*u; r = r - alpha*c; residual = norm(r).  *converged = residual <= tol.
 * p == NULL is Identity (c = r).  DEVIATION: the package runs its unpreconditioned iterator there, equal in exact arithmetic,
 * not in rounding.  A breakdown (dot(u, c) = 0, an indefinite matrix) is no error: Inf / NaN propagate, a NaN residual does
 * not stop the loop, which ends at maxiter.  ldiv! and mul! are those of esp_precon_ldiv and esp_mul, bit for bit.  dot and
 * norm (BLAS in the package, order undefined) are one fixed-shape ordered sum that depends on n alone -- chunks of 256
 * products folded by a pairwise tree, the same tree over groups of 256 chunk sums, then a strided sum and the tree once more
 * (csrc/krylov.hip states it in full) -- so x and the history are identical run to run and bit-identical to a model that
 * restates the statements and that shape; against the package they agree to the rounding of the dot products only.
 * history: maxiter+1 host doubles or NULL: history[0] the initial residual norm, history[k] the norm after iteration k;
 * *iterations = iterations run.  b, x: n doubles, device pointers when on_device != 0; x is updated in place.
 * Errors as esp_simple: p bound to another handle -> ESP_ERR_INVALID; pending entries, or a pattern change since p's last
 * update! -> ESP_ERR_STATE; a rectangular matrix -> ESP_ERR_INVALID; nnz or n >= 2^32 - 16 -> ESP_ERR_UNSUPPORTED.
 * Runs on the handle's stream, returns synchronised.  The work vectors (3 n doubles, the partial sums, 2 n more for host
 * vectors) belong to the handle: sized on first use, released with it. */
int32_t esp_cg(esp_handle *h, esp_precon *p, const double *b, double *x, int32_t on_device, int32_t initially_zero,
               int64_t maxiter, double abstol, double reltol, double *history, int64_t *iterations, int32_t *converged);
/* bicgstabl / bicgstabl!(x, A, b, l; Pl = p, abstol, reltol, max_mv_products, initially_zero) of IterativeSolvers.jl for
 * NON-SYMMETRIC systems (restated from the package's documented behaviour: the package is not part of the reference tree;
 * docs/src/iter.md:97-102 solves with it) on the device CSC, 1 <= l <= 4 (anything else -> ESP_ERR_INVALID):
 *   mv = 0; rs[0] = b (initially_zero != 0: x is taken to hold zeros) or rs[0] = b - A*x, mv = 1; rs[0] = Pl \ rs[0] (LEFT
 *   preconditioning: every residual and norm is the preconditioned one); us[0..l] = 0; omega = sigma = 1; rt = r_shadow, or a
 *   copy of rs[0]; residual = norm(rs[0]); tol = max(reltol*residual, abstol); then, while mv < max_mv_products and not
 *   residual <= tol (mv is tested before an outer iteration, not inside it):
 *     sigma = -omega*sigma; for j = 0..l-1: rho = dot(rt, rs[j]); beta = rho/sigma; us[k] = rs[k] - beta*us[k] (k = 0..j);
 *       us[j+1] = Pl \ (A*us[j]); sigma = dot(rt, us[j+1]); alpha = rho/sigma; rs[k] = rs[k] - alpha*us[k+1] (k = 0..j);
 *       rs[j+1] = Pl \ (A*rs[j]); x = x + alpha*us[0];
 *     mv += 2l; M[i][k] = dot(rs[i], rs[k]); gamma[1..l] = M[1..l,1..l] \ M[1..l,0] by an LU factorization WITHOUT pivoting
 *       (inv = 1/G[k][k]; G[i][k] *= inv; G[i][j] -= G[i][k]*G[k][j]), forward substitution with the unit lower factor, back
 *       substitution with a true division, the inner index increasing;
 *     us[0] -= gamma[k]*us[k]; x += gamma[k]*rs[k-1]; rs[0] -= gamma[k]*rs[k], each for k = 1..l in increasing k, one rounded
 *       product and one sum or difference per term; omega = gamma[l]; residual = norm(rs[0]) (a fresh dot product).
 *   *converged = residual <= tol.
 * ldiv! and mul! are those of esp_precon_ldiv and esp_mul, bit for bit; dot, norm and M are esp_cg's ordered sum; every division
 * is a true double division: x and the history are identical run to run and bit-identical to tests/bicgstabl_model.c, which
 * restates the statements as plain loops and is normative for the order of every operation.
 * DEVIATIONS from the package: r_shadow (n doubles on the same side as b, or NULL) is an argument and defaults to the initial
 * preconditioned residual -- the package draws rand(n) --, so a solve is reproducible; dot, norm and the Gram matrix (BLAS in
 * the package, the system solved by a pivoting LU) are as stated; p == NULL is Identity with no copies.
 * A breakdown (sigma = 0, a singular M) is no error: Inf / NaN propagate, a NaN residual does not stop the loop, which ends at
 * max_mv_products.  n = 1 always breaks down: the first BiCG step solves the system exactly, rs[0] = rs[1] = 0, the
 * minimal-residual system is 0/0 and x and the norms are NaN from the first outer iteration on (as in the package).
 * history: ceil(max_mv_products/(2l)) + 1 host doubles or NULL: history[0] the initial norm, history[k] the norm after outer
 * iteration k; *iterations = outer iterations run, *mv_products = mv.  b, x: n doubles, device pointers when on_device != 0; x
 * is updated in place.  Errors, stream use and "returns synchronised" exactly as esp_cg (max_mv_products < 0 ->
 * ESP_ERR_INVALID).  The work vectors (2(l+1) + 1 vectors of n doubles, n more in front of ILU0 / ILUAM and for the initial
 * residual, the partial sums, 8 scalars; 2 n more for host vectors) belong to the handle: sized on first use, released with it;
 * ESP_ERR_NOMEM leaves the handle usable. */
int32_t esp_bicgstabl(esp_handle *h, esp_precon *p, int32_t l, const double *b, double *x, const double *r_shadow,
                      int32_t on_device, int32_t initially_zero, int64_t max_mv_products, double abstol, double reltol,
                      double *history, int64_t *iterations, int64_t *mv_products, int32_t *converged);
/* gmres / gmres!(x, A, b; Pl = p, abstol, reltol, restart, maxiter, initially_zero, orth_meth) of IterativeSolvers.jl: restarted
 * GMRES(m) for NON-SYMMETRIC systems, the robust fallback where BiCGStab(l) breaks down (restated from the package's documented
 * behaviour: the package is not part of the reference tree; test/test_parilu0.jl:16-17 solves with it) on the device CSC.  LEFT
 * preconditioning: every residual and norm is the preconditioned one.  V is n x (restart+1), H (restart+1) x restart, nullvec
 * has restart+1 entries, all 1.0 at the start:
 *   init:  V1 = b (initially_zero != 0: x is taken to hold zeros) or b - A*x (mv += 1); V1 = Pl \ V1; beta = norm(V1);
 *          V1 = V1 * (1.0/beta)
 *   start: beta = init; acc = 1; current = beta; tol = max(reltol*current, abstol); k = 1; it = 0; history[0] = current
 *   while it < maxiter and not current <= tol:
 *     w = V[k+1] = Pl \ (A*V[k]); mv += 1
 *     orthogonalise w against V[1..k] -> H[1..k,k], nrm (below); w = w * (1.0/nrm); H[k+1,k] = nrm
 *     s = 0; for i = 1..k increasing: s = s + nullvec[i]*H[i,k]
 *     nullvec[k+1] = -(s / H[k+1,k]); acc = acc + nullvec[k+1]*nullvec[k+1]; current = beta / sqrt(acc)
 *     k += 1; it += 1; history[it] = current
 *     if k == restart+1 or current <= tol or it == maxiter:
 *       m = k-1; rhs = (beta, 0, .., 0) of length k
 *       for i = 1..m (Givens, column by column):
 *         f = H[i,i]; g = H[i+1,i]; g == 0 ? (c,s) = (1,0) : (r = sqrt(f*f + g*g); c = f/r; s = g/r)
 *         H[i,i] = c*f + s*g
 *         for j = i+1..m: t = -s*H[i,j] + c*H[i+1,j]; H[i,j] = c*H[i,j] + s*H[i+1,j]; H[i+1,j] = t
 *         t = -s*rhs[i] + c*rhs[i+1]; rhs[i] = c*rhs[i] + s*rhs[i+1]; rhs[i+1] = t
 *       for i = m..1: z = rhs[i]; for j = i+1..m increasing: z = z - H[i,j]*rhs[j]; rhs[i] = z / H[i,i]
 *       x[e] = (..((x[e] + rhs[1]*V[e,1]) + rhs[2]*V[e,2]) ..) + rhs[m]*V[e,m]
 *       k = 1
 *       if not current <= tol and it < maxiter: beta = init (never initially_zero; mv += 1); acc = 1  (current is NOT reset)
 *   *converged = current <= tol.
 * orth_meth, the package's three:
 *   ESP_ORTH_MGS (the default of the package): for i = 1..k: H[i,k] = dot(V[i], w); w = w - H[i,k]*V[i];  nrm = norm(w)
 *   ESP_ORTH_CGS:  h[j] = dot(V[j], w) for j = 1..k, all from the same w; w[e] = (..(w[e] - h[1]*V[e,1]) - ..) - h[k]*V[e,k];
 *                  nrm = norm(w); H[1..k,k] = h
 *   ESP_ORTH_DGKS: CGS first, then proj = sqrt(h[1]^2 + .. + h[k]^2) (sequential from 0.0, increasing j); eta = 1.0/sqrt(2.0);
 *                  while nrm < eta*proj and passes < 3: c[j] = dot(V[j], w) for j = 1..k; proj = that norm of c; w -= the same
 *                  ordered combination with c; h[j] = h[j] + c[j]; nrm = norm(w); passes += 1.  A NaN makes the test false.
 * ldiv! and mul! are those of esp_precon_ldiv and esp_mul, bit for bit; dot is esp_cg's ordered sum, norm(v) = sqrt(dot(v, v));
 * every product is rounded before its sum, every division and square root is the correctly rounded one: x, the whole history,
 * the counters and the flag are identical run to run and bit-identical to tests/gmres_model.c, which restates the statements as
 * plain loops and is normative for the order of every operation.
 * DEVIATIONS from the package: dot, norm and the two gemv's (BLAS in the package) use the stated order; Givens is the plain formula
 * above, without LAPACK's scaling: it overflows where f*f does; the DGKS loop is capped at 3 correction passes (the package has no
 * cap); x is also formed when maxiter ends a cycle part-way (by its documented behaviour the package forms x only at a restart or
 * on convergence and would return an x that does not belong to the residual it reports); p == NULL is Identity with no copies.
 * No errors: a breakdown (nrm == 0 without convergence, a singular H) -- Inf / NaN propagate, a NaN residual never stops the
 * loop, which ends at maxiter; a lucky breakdown -- current = 0, converged, x exact (n = 1 always ends so after one iteration);
 * b = 0 from x = 0 -- history = [0], no iteration, x untouched.
 * restart outside 1..ESP_GMRES_RESTART_MAX, an unknown orth_meth or maxiter < 0 -> ESP_ERR_INVALID.  n == 0 returns at once with
 * history[0] = 0.  history: maxiter+1 host doubles or NULL: history[0] the initial norm, history[k] the norm after iteration k;
 * *iterations = iterations run, *mv_products = mv, *reorth_passes = the DGKS correction passes of the whole solve (0 for the other
 * methods); every out pointer is optional.  b, x: n doubles, device pointers when on_device != 0; x is updated in place.  Errors,
 * stream use and "returns synchronised" exactly as esp_bicgstabl.  The work space (the basis block of restart+1 vectors, n more
 * doubles in front of ILU0 / ILUAM / AMG / a permuted Block, the partial sums, a scalar block for H, nullvec, rhs, h, c, beta,
 * acc, current and the pass counter; 2 n more for host vectors) belongs to the handle: sized on first use, released with it;
 * ESP_ERR_NOMEM leaves the handle usable. */
#define ESP_ORTH_MGS 0
#define ESP_ORTH_CGS 1
#define ESP_ORTH_DGKS 2
#define ESP_GMRES_RESTART_MAX 64
int32_t esp_gmres(esp_handle *h, esp_precon *p, const double *b, double *x, int32_t on_device, int32_t initially_zero,
                  int32_t restart, int32_t orth_meth, int64_t maxiter, double abstol, double reltol, double *history,
                  int64_t *iterations, int64_t *mv_products, int64_t *reorth_passes, int32_t *converged);

/* ---- the algebra of assembled matrices on the device CSC (abstractextendablesparsematrixcsc.jl:224-280) -----------
 * The reference evaluates these through SparseArrays; the device reproduces its documented rules bit for bit:
 *   A*B   Gustavson (spmatmul): for every column i of B, every stored B[j,i] in stored order, every stored A[k,j] in stored
 *         order, p = A[k,j]*B[j,i]; the first product reaching row k is assigned, later ones added in arrival order; every
 *         reached row is stored (zeros kept), rows sorted; no FMA, no reordered sums.
 *   A+B, A-B  map(f, A, B): both stored f(a,b), one stored f(a,0.0) / f(0.0,b); a result == 0 is not stored.
 *   D*A, A*D  the pattern of A exactly; nzval[p] = d[row]*nzval[p] / d[col]*nzval[p].
 * The operands must hold no pending entries (the reference's sparse(A) flushes first: flush them).  The result handle c
 * is left as a flush that changed the pattern leaves it (a preconditioner bound to c needs update!); every call returns
 * synchronised.  Operands and c on one device; a column window or column-shard use on any of them -> ESP_ERR_UNSUPPORTED;
 * m or n above 2^32 -> ESP_ERR_UNSUPPORTED.  A failed allocation returns ESP_ERR_NOMEM and leaves c as it was. */
/* C := A*B.  c: an empty handle of size (a.m, b.n) on the same device, no pending entries; its CSC is replaced.
 * a == b is allowed; c must be neither.  Pending entries on a or b -> ESP_ERR_STATE (flush first);
 * a.n != b.m -> ESP_ERR_INVALID; a column window / shard use on any operand -> ESP_ERR_UNSUPPORTED.
 * Columns of at most 2048 products run in the fused tier (sorted and folded in LDS), longer ones through an ESP_COO flush of
 * a scratch handle (the generic tier); *nnz_out = nnz(C). */
int32_t esp_matmul(esp_handle *a, esp_handle *b, esp_handle *c, int64_t *nnz_out);
/* C := A + B (op ESP_OP_ADD) or A - B (ESP_OP_SUB); zero results are not stored.  Same rules; sizes equal. */
int32_t esp_add(esp_handle *a, esp_handle *b, int32_t op, esp_handle *c, int64_t *nnz_out);
/* C := Diagonal(d) * A (side 0) or A * Diagonal(d) (side 1); the pattern of A.  c may equal a (in place: values only).
 * d: a.m (side 0) or a.n (side 1) doubles; on_device != 0: a device pointer. */
int32_t esp_diag_scale(esp_handle *a, const double *d, int32_t side, int32_t on_device, esp_handle *c);
/* the device the handle lives on (a result handle of the calls above goes on its operands' device) */
int32_t esp_device(const esp_handle *h, int32_t *device);
/* test hook: 0 automatic, 1 every column through the fused tier where it fits, 2 every column through the generic tier.
 * Set on the RESULT handle c of esp_matmul (automatic takes the fused tier wherever it fits: 1 behaves as 0). */
int32_t esp_debug_matmul_tier(esp_handle *c, int32_t tier);

/* ---- transpose, transpose(A)*x, issymmetric, opnorm, norm on the device CSC (abstractextendablesparsematrixcsc.jl:188-217) ----
 * The reference evaluates these through SparseArrays; the device reproduces its documented rules:
 *   copy(transpose(A))  halfperm!: an n x m CSC of every stored entry, explicit zeros included, rows ascending in every column;
 *                       bitwise (-0.0 and NaN payloads kept).
 *   transpose(A)*x      r[j] = 0.0; tmp = 0.0; tmp += nzval[k]*x[rowval[k]] over column j in stored order; r[j] += tmp; bitwise.
 *   issymmetric(A)      issymmetric(Matrix(A)): false for a rectangular matrix; a stored zero of either sign counts as absent;
 *                       every other stored v at (i,j), the diagonal included, needs v == A[j,i] (0.0 where not stored), so a
 *                       stored NaN gives false.  Exact.
 *   opnorm(A, p)        opnorm(::AbstractSparseMatrixCSC, p) branch by branch (m == 0 or n == 0: 0.0; m == 1 and n == 1: the
 *                       norms of the stored values; otherwise the column-sum (p = 1) and row-sum (p = Inf) loops, max
 *                       propagating NaN).  Bitwise, except the 1-row / 1-column norm(nzval, 1 or 2) cases (BLAS asum / nrm2 in
 *                       the reference): relative error <= 1e-13, identical run to run.
 *   norm(A, p)          norm(nonzeros(A), p) over the stored values (none: 0.0).  p = Inf, -Inf, 0: bitwise; p = 1, 2 and every
 *                       other p: relative error <= 1e-13, identical run to run; norm(A, 2) is scaled by the largest |v| and neither
 *                       overflows nor underflows where nrm2 does not.  NaN among the values gives NaN (its payload is not pinned).
 * The operand must hold no pending entries (ESP_ERR_STATE: flush first, as sparse(A) does); a column window or column-shard use
 * -> ESP_ERR_UNSUPPORTED; m or n above 2^32 -> ESP_ERR_UNSUPPORTED.  Every call returns synchronised.
 * Deviation: p NaN -> ESP_ERR_INVALID (SparseArrays would return 0.0 for an empty matrix and throw otherwise). */
/* C := copy(transpose(A)).  c: an empty handle of size (a.n, a.m) on a's device, c != a (else ESP_ERR_INVALID), no pending entries;
 * its CSC is replaced (a pattern change: a preconditioner bound to c needs update!).  A failed call (ESP_ERR_NOMEM included)
 * leaves c as it was.  Nothing else the call allocates outlives it.  *nnz_out = nnz(A). */
int32_t esp_transpose(esp_handle *a, esp_handle *c, int64_t *nnz_out);
/* test hook on the RESULT handle c of esp_transpose: 0 automatic (= 2), 1 the generic path (the entries as ESP_COO records with the
 * keys swapped, flushed into an empty CSC of a scratch handle; an esp_debug_fail_next_bucket_stage armed on c is met by that flush),
 * 2 the counting sort (row counts, a scatter, every column sorted by row; a row of A longer than 4096 entries takes path 1) */
int32_t esp_debug_transpose_path(esp_handle *c, int32_t path);
/* read-only: what the last successful esp_transpose into c did.  out[0] = the path taken (1 generic, 2 counting; 0: no transpose yet,
 * or an operand without stored entries); out[1], out[2] = the columns of C listed for the workgroup sort (longer than 32 entries) and
 * the longest column of C, as the counting path measured them (0 where it did not run: path 1 forced).  A row of A longer than 4096
 * entries reports path 1 with these counts.  Changes nothing. */
int32_t esp_debug_last_transpose(const esp_handle *c, int64_t out[3]);
/* r := transpose(A)*x (= adjoint(A)*x for real A); x: m doubles, r: n doubles; on_device != 0: device pointers (as esp_mul) */
int32_t esp_mul_transpose(esp_handle *h, const double *x, double *r, int32_t on_device);
/* *result = 1 if issymmetric(A) (= ishermitian(A) for real A), else 0 */
int32_t esp_issymmetric(esp_handle *h, int32_t *result);
/* *result = opnorm(A, p); p = 2 with m, n > 1 -> ESP_ERR_UNSUPPORTED ("2-norm not yet implemented"); p outside 1, 2, Inf where the
 * branch needs one of them -> ESP_ERR_INVALID.  p = Inf uses esp_mul's row-wise index (built on first use after a pattern change). */
int32_t esp_opnorm(esp_handle *h, double p, double *result);
/* *result = norm(A, p) */
int32_t esp_norm(esp_handle *h, double p, double *result);

/* ---- column-range shards (multi-GPU, one process per GPU) ------------------------
 * owner(col) = floor((col-1)*nshards/n).  esp_shard_counts: pending entries per owner.
 * esp_shard_export: stable partition of the pending entries by owner into the caller's
 * device buffers (send buffer of the all-to-all); offsets has nshards+1 entries.       */
int32_t esp_shard_counts(esp_handle *h, int32_t nshards, int64_t *counts);
int32_t esp_shard_export(esp_handle *h, int32_t nshards, uint64_t *d_keys, double *d_vals,
                         int64_t *offsets);
/* In-place form of the exchange: what this rank owns itself is not copied twice.  After the counts
 * were exchanged the caller knows how many entries arrive from lower / higher ranks.  The pending
 * entries are partitioned by owner; the own chunk lands at its final position recv_lower, the other
 * chunks (compacted, owner order; send_offsets has nshards+1 entries, the own chunk counts 0) in a
 * send region returned as device pointers that stay valid until the next append or flush.  The
 * received chunks are then dropped in with esp_shard_exchange_place (lower ranks at position 0,
 * higher ranks behind the own chunk). */
int32_t esp_shard_exchange_begin(esp_handle *h, int32_t nshards, int32_t self, int64_t recv_lower,
                                 int64_t recv_higher, uint64_t **d_send_keys, double **d_send_vals,
                                 int64_t *send_offsets);
int32_t esp_shard_exchange_place(esp_handle *h, int64_t position, const uint64_t *d_keys,
                                 const double *d_vals, int64_t count);

/* Partitioned exchange (the fast path for streams an assembly loop emits; the calls above remain the
 * general one).  ONE stable pass partitions the pending entries by (owner, digit inside the owner's
 * column range) -- the owner split and the first partition pass of the local flush at once.
 *   esp_shard_partition: entries_per_shard = (global number of pending entries) / nshards, the SAME
 *     value on every rank (it fixes the digit width, which all ranks must agree on).  *ok = 0: not
 *     applicable (stream not pre-sorted, tiny problem, > 64 shards) -- use esp_shard_exchange_begin;
 *     the pending entries are intact (possibly permuted in a way that keeps the order per entry).
 *     *ok = 1: owner r's entries are d_keys/d_vals[entry_offsets[r] .. entry_offsets[r+1]) and its
 *     per-digit counts d_counts[r*digits .. (r+1)*digits) (device pointers, valid until the next
 *     append or flush).  Send every OTHER owner its range and its counts.  entry_offsets and d_counts are
 *     final on return; the kernel that moves the entries into d_keys/d_vals may still be running on the
 *     handle's stream (the callers' consensus round fits beside it): esp_synchronize(h) before reading them.
 *   esp_shard_assemble: device pointers of the blocks received from every source rank (index = source;
 *     the own index is ignored; recv_entries[q] = entries in block q, counts blocks hold `digits`
 *     values).  The buffers must stay alive until esp_flush returns: the bucket kernel reads a segment
 *     as the concatenation of one piece per source (rank order), nothing is copied.  *ok = 0: a merged
 *     segment is too long for the bucket kernel; the entries were copied into a plain pending buffer
 *     (rank order) instead and esp_flush works as usual.  *ok = 1: until that esp_flush no append is accepted
 *     (ESP_ERR_STATE): the pending entries live in the caller's receive buffers.
 * esp_set_column_window(own column range) must be in force, as for the other exchange. */
int32_t esp_shard_partition(esp_handle *h, int32_t nshards, int32_t self, int64_t entries_per_shard,
                            int32_t *ok, uint64_t **d_keys, double **d_vals, int64_t **d_counts,
                            int64_t *entry_offsets /* nshards+1 */, int64_t *digits_per_shard);
/* esp_shard_plan announces the next esp_shard_partition(nshards, self, entries_per_shard): a device-side producer
 * (esp_generate_*) that finds the buffer empty then writes every entry straight to its (owner, digit) bucket -- the
 * append is the partition, as on one GPU -- and that esp_shard_partition call, given exactly these arguments, has nothing
 * left to move.  entries_per_shard < 0: no announcement.  esp_group_flush does this for the flush after it. */
int32_t esp_shard_plan(esp_handle *h, int32_t nshards, int32_t self, int64_t entries_per_shard);
/* 1: the last esp_shard_partition moved the entries in a pass of its own, 2: the producer had partitioned them, 0: neither */
int32_t esp_debug_last_shard_source(const esp_handle *h, int32_t *kind);
int32_t esp_shard_assemble(esp_handle *h, const uint64_t *const *d_recv_keys,
                           const double *const *d_recv_vals, const int64_t *const *d_recv_counts,
                           const int64_t *recv_entries /* nshards */, int32_t *ok);

/* ---- esp_group: the sharded flush as ONE call per rank (one process per GPU) --------------------------
 * What GenericMTExtendableSparseMatrixCSC does with threads (one buffer per tid, flush! = Base.sum(xmatrices, csc):
 * src/matrix/genericmtextendablesparsematrixcsc.jl:45-51,87-99) across the GPUs of a node: every rank appends whatever
 * its part of the assembly loop produces to ITS handle (any column), esp_group_flush routes every pending entry to the
 * rank that owns its column and runs the local flush.  It drives the esp_shard_* calls above; the transport is RCCL
 * (grouped ncclSend/ncclRecv on the handle's stream, loaded with dlopen: no link-time dependency) or a callback table
 * of the host (MPI, a test harness).  Every esp_group_flush / _nnz / _get_csc is COLLECTIVE: all ranks call it.
 *
 *   rank 0:  esp_group_unique_id(id)  ->  the host broadcasts the 128 bytes (MPI_Bcast, a socket, Distributed.jl)
 *   all:     esp_create(m, n, device, hint, &h); esp_group_create(h, nranks, rank, id, &g)
 *   loop:    appends on h (esp_commit / esp_append_* / esp_generate_*);  esp_group_flush(g, mode, &local_nnz, &changed)
 *   result:  esp_group_nnz (global nnz, this rank's offset), esp_group_get_csc (own column range, global colptr values),
 *            or the device CSC of the handle (esp_csc_device) for consumers that stay on the GPU.                    */
typedef struct esp_group esp_group;
typedef struct {
    void *ctx;
    /* all-gather of `count` int64 per rank through HOST memory; recv holds nranks * count values, rank-major */
    int32_t (*allgather_i64)(void *ctx, const int64_t *send, int32_t count, int64_t *recv);
    /* all-to-all-v on DEVICE memory of the handle's device: for every peer q (the own index is ignored) send
     * send_bytes[q] bytes from send[q] and receive recv_bytes[q] bytes into recv[q]; must be complete, or ordered on
     * hip_stream (the handle's hipStream_t) in front of whatever is enqueued there next, when it returns */
    int32_t (*alltoallv_dev)(void *ctx, const void *const *send, const int64_t *send_bytes, void *const *recv,
                             const int64_t *recv_bytes, void *hip_stream);
} esp_comm_t;
int32_t esp_group_unique_id(uint8_t *id128 /* 128 bytes: an ncclUniqueId */);
/* the handle must be empty; its column window becomes the rank's own column range */
int32_t esp_group_create(esp_handle *h, int32_t nranks, int32_t rank, const uint8_t *id128, esp_group **out);
int32_t esp_group_create_comm(esp_handle *h, int32_t nranks, int32_t rank, const esp_comm_t *comm, esp_group **out);
int32_t esp_group_destroy(esp_group *g);   /* (the handle stays the caller's) */
int32_t esp_group_handle(esp_group *g, esp_handle **out);
const char *esp_group_last_error(const esp_group *g);
/* the rank's own columns, 1-based inclusive: owner(col) = floor((col-1)*nranks/n) */
int32_t esp_group_column_range(const esp_group *g, int64_t *col_lo, int64_t *col_hi);
int32_t esp_group_flush(esp_group *g, int32_t mode, int64_t *local_nnz, int32_t *pattern_changed);
int32_t esp_group_nnz(esp_group *g, int64_t *global_nnz, int64_t *nnz_before_me);
/* colptr_own: col_hi - col_lo + 2 entries = the GLOBAL colptr[col_lo .. col_hi + 1]; rowval, nzval: local_nnz entries */
int32_t esp_group_get_csc(esp_group *g, int64_t *colptr_own, int64_t *rowval, double *nzval);
/* kind: 1 = partitioned exchange (pre-sorted streams), 2 = in-place exchange; entries sent to other ranks */
int32_t esp_group_last_exchange(const esp_group *g, int32_t *kind, int64_t *sent_off_rank);
/* Test hook for one-GPU boxes (a single-rank group made with esp_group_create, i.e. over the library's own RCCL
 * transport): on = 1 -- every esp_group_flush sends the rank's own partitioned ranges to ITSELF through the all-to-all-v
 * (grouped ncclSend / ncclRecv, 1 GiB rounds, on the handle's stream), wipes them and restores them from what arrived,
 * and the flush's small agreements run as a real ncclAllGather on the second stream; on = 0 -- off; on < 0 -- query only.
 * bytes_last_flush: what travelled through RCCL in the last flush.  Results never change. */
int32_t esp_debug_group_loopback(esp_group *g, int32_t on, int64_t *bytes_last_flush);

/* promise: every pending entry of the following flushes has its column in [col_lo, col_hi]
 * (1-based); the partition then works on that window only.  Violations -> ESP_ERR_STATE from esp_flush: the
 * stored pattern is untouched and the batch stays pending (esp_clear_pending / esp_reset), but updates of the
 * batch that hit stored positions may already have been applied to their values. */
int32_t esp_set_column_window(esp_handle *h, int64_t col_lo, int64_t col_hi);

/* ---- measurement ---------------------------------------------------------------- */
/* on = 1: HIP events around the big kernels (append, hist, scatter, local, fold, colptr, merge, copy);
 * on = 2: also around the small launches of the "scan" stage (costs about 3 % of a 256^3 step);
 * on = 3: around the bucket kernel (general path: the fold kernel) only -- every bracketed kernel costs two event
 * records of about 6 us on the stream; 0: off */
int32_t esp_timing_enable(esp_handle *h, int32_t on);
int32_t esp_timing(esp_handle *h, esp_timing_t *out, int32_t clear);
/* Test hooks: esp_debug_force_path(h, path) pins ONE implementation where the library has two (results never change,
 * timings do); path 0 = automatic.  The numbers are part of the ABI (the tests and tools pass them). */
typedef enum {
    ESP_PATH_AUTO = 0,
    ESP_PATH_GENERAL = 2,            /* the general path: global LSD sort + global fold (no bucket kernel)                  */
    ESP_PATH_RADIX_TAIL_ONLY = 3,    /* bucket kernel with its radix tier only (no column tiers, no small variant)          */
    ESP_PATH_MANY_LAUNCHES = 4,      /* bucket kernel issued in launches of 64 workgroups (carry-over of the look-back state) */
    ESP_PATH_NO_RUN_PARTITION = 5,   /* never the run-based single-pass partition: 8/9-bit passes only; producers append in
                                        stream order                                                                        */
    ESP_PATH_SHARD_NOT_APPLICABLE = 11, /* esp_shard_partition reports "not applicable" (consensus fall-back of the exchange) */
    ESP_PATH_RUN_LIST_BY_RADIX = 12, /* the run-based partition orders its run list with radix passes (several small launches
                                        and a host round trip) instead of the one ranking kernel                            */
    ESP_PATH_COLPTR_BY_SCAN = 13,    /* fresh matrix: the bucket kernel marks column ends and a scan over all columns builds
                                        colptr (instead of every segment writing the colptr of its own columns)             */
    ESP_PATH_PACKED_KEYS = 14,       /* packed 8-byte keys for the bucket kernel always (never 4-byte keys)                  */
    ESP_PATH_GENERIC_FOLD = 15,      /* 4-byte keys but the generic fold (no UPDATE-only / one-kind variants)                */
    ESP_PATH_PRODUCER_STREAM_ORDER = 16, /* device-side producers and bulk appends always write in stream order (never the
                                        producer-side partition); the flush partitions                                      */
    ESP_PATH_MERGE_PATH_JOIN = 17,   /* the join with a stored CSC as a merge-path over a per-entry column array (a second
                                        implementation of the column-tiled join)                                            */
    ESP_PATH_NO_SMALL_VARIANT = 18,  /* never the small variant of the bucket kernel (see esp_debug_last_local_small)        */
    ESP_PATH_NO_BATCH_TAIL = 19,     /* an append behind a producer's bucket-ordered batch turns it back into packed keys
                                        (no "batch + tail" flush)                                                           */
    ESP_PATH_BATCH_TAIL_ONE_FLUSH = 22, /* a batch + tail over a stored pattern is ONE flush over two pieces (as on a fresh
                                        matrix) instead of two flushes                                                      */
    ESP_PATH_EIGHT_BIT_PASSES = 23,  /* partition passes of at most 8 bits (no 9-bit digits where they would save a pass)    */
    ESP_PATH_NO_GROUP_TIER = 24,     /* bucket kernel: column runs of more than 24 entries through the radix tier, never the
                                        group tier (2 .. 16 lanes per column)                                               */
    ESP_PATH_NO_ITEM_PARTITION = 25, /* esp_generate_fem in a shuffled order appends in stream order (no item partition)     */
    ESP_PATH_NO_BIG_VARIANT = 26,    /* never the bucket-kernel variant with the 24-input register tier                      */
    ESP_PATH_NO_APPEND_PARTITION = 27, /* esp_append_device / esp_commit of one kind on an empty buffer pack in stream order (the
                                        append is not the partition; esp_append_host always arrives in stream order)       */
    ESP_PATH_TWO_WORD_ITEMS = 28,    /* the item partition of esp_generate_fem moves 16-byte records (key | cell and vertex)
                                        even where the cell's number fits into the key                                      */
    ESP_PATH_TAIL_TO_FRONT = 29,     /* the entries behind a batch that was flushed by itself are copied to the front of
                                        the buffer before their partition (instead of being read where they lie)            */
    ESP_PATH_NO_GROUP3 = 30,         /* never the group-tier kernel with three workgroups per CU (group3_k)                  */
    ESP_PATH_LOCAL_BITS = 32,        /* item partitions (esp_generate_fem in a shuffled order, esp_append_elements): the passes
                                        stop up to three bits early and the expansion orders every segment of up to 4096 items
                                        by the last bits itself (segexpand.hpp) -- one pass less, a slower expansion: measured
                                        slower at config 4's sizes, so not the default                                      */
    ESP_PATH_NO_WIDE_GROUP3 = 33,    /* never the wide form of group3_k (rows of a segment spread over more than 2^18: full rows
                                        in LDS, every column run sorted twice); such segments go to local_k's kernels         */
    ESP_PATH_NO_HITS_KERNEL = 34,    /* never group3_k's re-assembly form (additions over a stored pattern the same mesh built:
                                        every (col,row) of a column run is the stored entry of its rank, sums to a second value
                                        array, all-or-nothing); such flushes take local_k's group-tier kernels               */
    ESP_PATH_LATE_TOTAL = 36,        /* group3_k publishes a segment's total for the look-back after the fold (instead of right
                                        after the sort, which a segment of RAWUPDATEs allows)                                */
    ESP_PATH_NO_CELL_RECORDS = 37,   /* esp_append_elements with cells of 3 / 4 nodes: no 64-byte cell records, the expansion gathers
                                        rows and diagonal terms from the caller's arrays (as it does for other cell sizes)     */
    ESP_PATH_HOST_KEYS8 = 38,        /* esp_append_host of one kind: packed eight-byte keys over PCIe (never six-byte keys)      */
    ESP_PATH_NO_REBUILD = 40,        /* the entries behind a re-assembly's batch never REBUILD the matrix (a fresh flush whose segments start with
                                        the stored entries of their columns as a first piece: no look-ups, no join): always the bucket kernel
                                        against the stored columns + the column-tiled join                                      */
    ESP_PATH_NO_LAZY_ITEMS = 39,     /* item partitions (esp_generate_fem in a shuffled order, esp_append_elements) always run their
                                        expansion at append time: the updates are stored bucket by bucket and the flush's bucket
                                        kernel reads them -- never the fused form that forms them from the sorted item records  */
    ESP_PATH_NO_FINE_PARTITION = 41, /* more than 32 key bits below the planned prefix (a stencil above 256^3): never the FINE partition
                                        (up to 4 more prefix bits, so that 4-byte keys serve, with the bucket kernel taking 2 .. 16
                                        neighbouring buckets as one segment): packed 8-byte keys as before round 6 -- for a
                                        shard's producer too (its own range: 2^fb buckets per digit of the exchange plan)      */
    ESP_PATH_NO_BUCKET_PAIRS = 42,   /* never the PAIR form of the small bucket kernel (two producer buckets per workgroup, see
                                        esp_debug_last_bucket_pairs): one bucket per workgroup, local_k's small variant       */
    ESP_PATH_NO_PREDICTED_OFFSETS = 43, /* never the PREDICTED form of the pair kernel (a flush that repeats the producer plan of
                                        the handle's last flush takes every pair's output offset from the table that flush left, see
                                        esp_debug_last_predicted): always the ticket + look-back form; no table is recorded.  Counts
                                        as automatic for every other choice, like 42                                          */
    ESP_PATH_NO_LAZY_STENCIL = 44,   /* the stencil generator always writes its batch (the PART launch runs in the generator call):
                                        never the fused form in which a repeated full-range batch on a fresh matrix stays unwritten
                                        and the predicted pair kernel forms every column's updates itself (see
                                        esp_debug_last_lazy_stencil).  Counts as automatic for every other choice, like 42 and 43 */
    ESP_PATH_NO_KEPT_STRUCTURE = 45, /* the fused stencil flush always stores colptr and rowval: never its KEEP form, in which a
                                        repeated step whose structure the handle's last fused flush left in these very buffers stores
                                        the values alone (see esp_debug_last_kept_structure).  Counts as automatic for every other
                                        choice, like 42, 43 and 44                                                             */
    ESP_PATH_NO_PLAN_REUSE = 31     /* esp_append_device / esp_commit of one kind on an empty buffer always count their columns
                                        (never the run lists of the previous, identical-looking batch)                      */
} esp_debug_path;
/* last_path reports which pipeline the last flush took (1 = LDS bucket path, 2 = general).
 * Environment: the product library reads ESP_HOST_THREADS (host threads the transfers from / to pageable host arrays --
 * esp_append_host, esp_set_csc / esp_set_nzval, esp_get_csc / esp_get_nzval, esp_append_elements_host -- may use beside the
 * caller's: they go through two pinned bounce buffers, the host copy of one chunk overlapping the PCIe transfer of the other), ESP_RCCL_LIB (path of the RCCL library esp_group_create loads) and, as test hooks, ESP_DEBUG_FORCE_PATH (the
 * path every new handle starts with) and ESP_DEBUG_FAIL_COMM_INIT (esp_group_create fails as with a broken fabric) --
 * nothing else: the switches of the measurement tools exist in a -DESP_EXPERIMENTS build only (csrc/common.hpp). */
int32_t esp_debug_force_path(esp_handle *h, int32_t path);
/* test hook: plan the partition as if the bucket kernel took segments of `cap` entries (many prefix bits -- the 9-bit passes,
 * several rounds -- at sizes a CPU oracle can follow); 0: off */
int32_t esp_debug_plan_cap(esp_handle *h, double cap);
/* test hook: the NEXT flush that reaches its bucket stage reports ESP_ERR_STATE there instead of running it (once) -- the batch
 * must stay pending, whatever the partition left in the buffers (4-byte keys in both pairs ...), and the next flush must finish it */
int32_t esp_debug_fail_next_bucket_stage(esp_handle *h);
int32_t esp_debug_last_path(const esp_handle *h, int32_t *path);
/* how the last run-based partition turned its run lists into offsets: 1 = one ranking kernel over per-digit run
 * lists, 2 = radix-ordered run list, 3 = ranking kernel given up (a digit with more runs than its list holds),
 * radix-ordered run list used */
int32_t esp_debug_last_run_order(const esp_handle *h, int32_t *kind);
/* 1 when the bucket kernel of the last flush wrote colptr itself (fresh matrix, full key window, segments = whole
 * blocks of at most 2048 columns), 0 when column-end marks + a scan over the columns did */
int32_t esp_debug_last_colptr_direct(const esp_handle *h, int32_t *direct);
/* bytes per key the bucket kernel of the last flush read: 4 when every pending entry had been appended with one
 * known kind, at most 32 key bits were left below the partition prefix and the run-based partition served the
 * flush (it then writes only those bits), else 8 (packed keys) */
int32_t esp_debug_last_key_bytes(const esp_handle *h, int32_t *bytes);
/* 1 when the register tiers of the last flush's bucket kernel ran the UPDATE-only fold (every entry known to be an
 * updateindex! call: the batch's bookkeeping, for a shard also a device check of the received blocks) */
int32_t esp_debug_last_fold_update(const esp_handle *h, int32_t *on);
/* 1 when the bucket kernel of the last flush was its small variant: segments of at most 3072 entries over at most 256
 * columns, no radix tier, 51 KiB of LDS = three workgroups per CU instead of two (column runs longer than its register
 * tiers take go through a slow tier and send the handle's next flushes to the regular kernel); esp_debug_force_path(18):
 * never.  2 when it was the group tier's kernel with three workgroups per CU (group3_k: long column runs on a fresh matrix,
 * 4-byte keys; esp_debug_force_path(30): never); 3 when it was that kernel's WIDE form (rows of a segment spread over more than
 * 2^18 -- a mesh numbered without locality: every run sorted twice; esp_debug_force_path(33): never); 4 / 5 when it was that
 * kernel's re-assembly form over a stored pattern (plain / wide; esp_debug_force_path(34): never) */
int32_t esp_debug_last_local_small(const esp_handle *h, int32_t *small);
/* 1 when the bucket kernel of the last flush was the small variant's PAIR form (esp_debug_last_local_small then reports 1): one
 * workgroup took two neighbouring producer buckets -- up to 512 columns and 6144 entries -- as one segment (a fresh matrix, 4-byte
 * keys of one kind, at most 12 pending entries per column; a pair with a longer column run or rows spread over 2^19 or more sends
 * the flush, and the handle's later ones, to the one-bucket kernel); esp_debug_force_path(42): never */
int32_t esp_debug_last_bucket_pairs(const esp_handle *h, int32_t *on);
/* the cut the bucket kernel of the last flush worked on: column bits of one bucket of the table (a bucket holds 2^cl_bits columns;
 * -1: the buckets are no whole columns) and the number of buckets -- the pair form takes two neighbouring ones per workgroup */
int32_t esp_debug_last_bucket_cut(const esp_handle *h, int32_t *cl_bits, int32_t *buckets);
/* what the last flush did with the pair kernel's PREDICTED form: 0 not tried (no table for the batch's plan: the plan was not
 * reused, entries lie behind the batch, the table belongs to another plan, two predictions in a row missed), 1 served (every pair
 * emitted the count the table of the handle's last flush of this plan says: no ticket, no look-back), 2 tried and missed (some
 * pair's count differs -- structural zeros moved; the pairs that differ stored nothing, the flush ran again with the look-back
 * form and left a new table).  esp_debug_last_bucket_pairs reports 1 in all three cases; esp_debug_force_path(43): never tried */
int32_t esp_debug_last_predicted(const esp_handle *h, int32_t *state);
/* test hook: adds 1 to the middle entry of the kept offset table, so that the next flush that tries it misses (ESP_ERR_STATE
 * when the handle holds no table) */
int32_t esp_debug_spoil_predicted(esp_handle *h);
/* 1 when the bucket kernel of the last flush formed its updates from the sorted ITEM records of an item partition
 * (esp_generate_fem in a shuffled order, esp_append_elements on an empty buffer of a fresh matrix): the expansion -- every
 * update stored once at its bucket position, read again by the bucket kernel -- never ran (csrc/group3_items.hpp);
 * esp_debug_force_path(39): never.  2 (on the destination of esp_flush_sum): the folds of all buffers ran as ONE launch over their
 * item records and the combine flush read the folded records as pieces (every buffer held an element batch with the same plan) */
int32_t esp_debug_last_lazy_items(const esp_handle *h, int32_t *on);
/* what became of the last esp_generate_fdrand batch's held-back PART launch: 0 not armed (the batch was written in the generator
 * call: not a repeat of the handle's last plan over the full node range on a fresh matrix, no offset table for the plan, a shard,
 * a column window, esp_debug_force_path(43 / 44)), 1 the flush's fused pair kernel formed the updates itself and the batch was
 * never written (esp_debug_last_predicted and _last_bucket_pairs then report 1), 2 armed and then written after all (something
 * other than that flush needed the entries -- an append behind the batch, a read of the pending buffer, a clone, a shard call, a
 * second generator call -- or the prediction missed) */
int32_t esp_debug_last_lazy_stencil(const esp_handle *h, int32_t *state);
/* what the last flush did with the structure (colptr, rowval): 0 it stored everything (every flush but the one below), 1 KEPT -- the
 * fused stencil flush found colptr and rowval as the handle's last fused flush of the same plan, offset table, grid and kind left
 * them, that flush had emitted the grid's whole structural pattern, and every pair hit the table: the pattern is the stored one and
 * the kernel stored the values alone (n > 4096, no column window; esp_reset and esp_zero_values in between keep the structure,
 * whatever else may write or move colptr / rowval -- a read that resolves reset!'s lazy colptr, esp_set_csc, an editor of the CSC, a
 * result installed into the handle, esp_clone, a shard call, esp_release_buffers -- makes the next flush store everything), 2 the
 * KEEP form missed (some pair's count differs from the table's) and the retry rewrote everything.  esp_debug_force_path(45): never 1 */
int32_t esp_debug_last_kept_structure(const esp_handle *h, int32_t *state);
/* the march of the fused stencil kernel: a workgroup handles `planes` consecutive z planes of the same 512 (i, j) columns, forms
 * what does not depend on the plane once and takes each z pair value from the register that formed it one plane below.  A grid
 * conforms when nx ny is a multiple of the columns of a pair (2 << cl_bits, esp_debug_last_bucket_cut); every other grid runs one
 * plane per workgroup.  last_march: planes per workgroup of the last flush's fused launch, 0 when the last flush was not fused (or
 * the fused kernel missed and the flush was served again without it) */
int32_t esp_debug_last_march(const esp_handle *h, int32_t *planes);
/* test hook: 0 the automatic rule; planes > 0: that march wherever the grid conforms, clamped to nz (a grid that does not conform
 * still runs one plane per workgroup) */
int32_t esp_debug_force_march(esp_handle *h, int32_t planes);
/* the automatic rule as a pure function (no handle, no device): 3 planes where the grid conforms, nz >= 3, that leaves at least
 * 10.75 rounds of the workgroups the device holds at once (four per compute unit) and the last, partly filled round costs no more
 * than 1 / 32 of the launch -- the one march a measurement backs, see pair_gen_march_rule (csrc/local_x.hip); else 1 */
int32_t esp_debug_march_rule(int64_t nx, int64_t ny, int64_t nz, int32_t cl_bits, int32_t compute_units, int32_t *planes);
/* how many neighbouring segments of the folds' plan the combine flush of the last esp_flush_sum of that kind (last_lazy_items 2)
 * joined into one (1, 2, 4 or 8: as many as keep the longest joined segment within the bucket kernel's capacity); 0 otherwise */
int32_t esp_debug_last_sum_join(const esp_handle *h, int32_t *segments);
/* host wall-clock split of the destination's last esp_flush_sum, in ms: the buffers' folds (one launch over their item records, or
 * every buffer's own flush) | everything behind them (gather, combine flush, its completion) -- what a bench line reports beside
 * esp_debug_last_lazy_items / _sum_join so that a slow run can be told from a run that took the other path */
int32_t esp_debug_last_sum_ms(const esp_handle *h, double *folds_ms, double *combine_ms);
/* 1 when the destination's last esp_flush_sum folded its buffers -- not element batches with one plan: per-entry calls, mixed kinds,
 * anything -- in ONE flush of a scratch matrix with p n columns (buffer k in the columns [k n, (k + 1) n): no column is shared, every
 * buffer is folded by itself) instead of one flush per buffer; 0: one by one (a single buffer, a window or test hook on a buffer) */
int32_t esp_debug_last_sum_batched(const esp_handle *h, int32_t *batched);
/* the smallest / largest number of prefix bits the buffers of the destination's last joint esp_flush_sum (last_lazy_items 2) had planned
 * for their item partitions: every handle plans from its own history, the joint path takes the coarsest plan (test hook) */
int32_t esp_debug_last_sum_plan_bits(const esp_handle *h, int32_t *pb_min, int32_t *pb_max);
/* 1 when the last flush REBUILT the matrix for the entries behind a re-assembly's batch (a fresh flush whose segments start
 * with the stored entries of their columns: no look-ups against the stored columns, no join); esp_debug_force_path(40): never */
int32_t esp_debug_last_rebuild(const esp_handle *h, int32_t *on);
/* 1 when the last append-is-the-partition of caller-supplied triplets (esp_append_device / esp_commit of one kind on an
 * empty buffer) used the run lists of the previous assembly instead of counting its columns again: a batch of the same
 * length and kind is scattered straight away, every tile checked against its run list by the scatter kernel (a stream
 * that turns out different is partitioned the full way; results never change) */
/* ... likewise 1 when the last esp_generate_fdrand[_range] repeated the handle's previous call (same grid, node range and kind on
 * the same empty buffer: a time loop of reset! / fdrand! / flush!) and went straight to its PART launch: the run lists, run
 * offsets and bucket starts are a function of the grid and the plan, not of seed or values (esp_debug_force_path(31): never) */
int32_t esp_debug_last_plan_reused(const esp_handle *h, int32_t *reused);
/* which partition the last flush used: 1 = run-based single pass (pre-sorted stream), 2 = 8-bit passes,
 * 4 = none: the producer wrote every entry straight to its bucket (esp_generate_* on an empty buffer: a COUNT launch
 *     of the producer, then its stores go to `bucket start + stable rank`; the flush starts at the bucket kernel),
 * 5 = such a batch with entries appended behind it: the run-based pass over those entries only, the bucket kernel
 *     reads every segment as two pieces (batch, tail),
 * 6 = such a batch + tail over a stored pattern: the batch flushed by itself (as 4), then the tail as a flush of its own,
 * 7 = none: the segments came assembled from esp_shard_assemble,
 * 8 = as 6, and the tail had been partitioned as it was appended (one kind, a pre-sorted stream): both flushes start at the
 *     bucket kernel */
int32_t esp_debug_last_partition(const esp_handle *h, int32_t *kind);
/* which kernels read the CALLER's arrays in the handle's last device-side append (read-only; 0: none yet):
 * esp_append_device / esp_commit -- 1 = packed in stream order (pack_k), 2 = the append was the partition (the run-based pass
 *     counted the columns and scattered rows, columns and values), 3 = the same over the previous assembly's run lists
 *     (esp_debug_last_plan_reused 1), 4 = partitioned as a tail behind a batch over a stored pattern, 5 = the first radix pass of
 *     the flush ran from the caller's arrays (a shuffled stream of 2^18 entries or more);
 * esp_append_elements -- 6 = the item partition, one thread per item (elem_items_k), 7 = the item partition, one thread per cell,
 *     which leaves cell records (elem_cells_k: cells of 3 or 4 nodes), 8 = the updates written in stream order (elem_stream_k: 4096
 *     updates or fewer, a non-empty buffer, a cell that names a node twice) */
int32_t esp_debug_last_append_route(const esp_handle *h, int32_t *route);

/* SEVERAL RIGHT-HAND SIDES: mul!(R, ext, X) and ldiv!(U, fact, V) with matrices (the reference forwards both to SparseArrays
 * and to the factorization, which take them).  esp_mul_many: R[:, r] = A * X[:, r], r = 0 .. k-1; X is n x k column-major with
 * leading dimension ldx, R is m x k with ldr.  esp_precon_ldiv_many: U[:, r] = ldiv!(p, V[:, r]); n x k column-major, leading
 * dimensions ldv and ldu.  on_device != 0: device pointers (the hand-over rules of esp_mul), else host arrays.
 * CONTRACT: column r of the result is bit for bit what esp_mul / esp_precon_ldiv gives for column r alone -- for every kind of
 *   esp_precon and every stored value (+-0.0, NaN, Inf).  A NaN or Inf of one column never reaches another column.  Rows
 *   n .. ld-1 between the columns of X and V are never read, those of R and U never written.
 * ALIASING: U == V with ldu == ldv is the in-place solve.  Any other overlap of the two ranges ([V, V + (k-1)*ldv + n) and U's),
 *   and any overlap of X and R, is refused with ESP_ERR_INVALID before anything is launched.
 * ARGUMENTS: k == 0 returns ESP_OK after the state checks.  ESP_ERR_INVALID: k < 0; a leading dimension below max(n, 1) (max(m, 1)
 *   for ldr); a NULL array that would hold an element.  Every state check and message of the single-vector call applies unchanged:
 *   pending entries, a pattern changed since the last update!, a failed last update! (ESP_ERR_STATE).
 * HOW: k == 1 IS the single-vector call: the same launches of the same kernels.  Otherwise the columns go in chunks of
 *   ESP_MANY_CHUNK, a narrower last chunk masked; everything is enqueued on the handle's stream, which is synchronised ONCE at the
 *   end.  The library's scratch grows with ESP_MANY_CHUNK, never with k: host arrays are staged ESP_MANY_CHUNK columns at a time.
 *   - esp_mul_many: one launch per chunk over the row-wise index of esp_mul; a lane owns a row and ESP_MANY_CHUNK accumulators,
 *     reads every stored value and column once and runs esp_mul's statement acc_r = acc_r + a_ij * x_r[j] per column, j ascending.
 *   - CholeskyFactorization and LUFactorization's panel form: per chunk a gather into work vectors stored right-hand-side-fastest
 *     (y[pos * ESP_MANY_CHUNK + r]), ONE launch per depth of the tree per direction, a scatter; a lane owns one (row of the node,
 *     right-hand side) pair and walks exactly the single call's chain for it, so one read of a panel entry serves the whole chunk.
 *     No allocation, copy or synchronisation in between; esp_precon_cholesky_stats / esp_precon_lu_panel_stats do not change.
 *   - Jacobi (SPAI-0) and ILU0: the many-column kernels of esp_cg_many, one or two launches per chunk.
 *   - ILUAM and every kind whose ldiv! ends in its two triangular solves (ILU(k), ILUT, Colored, Block, LU's column form): per chunk
 *     ONE pass over the forward and the backward launch list -- as many level launches as a single ldiv!, whatever the chunk's
 *     width.  A lane owns one (row, right-hand side) pair, the ESP_MANY_CHUNK lanes of a row are adjacent and the scratch is stored
 *     right-hand-side-fastest (y[i * ESP_MANY_CHUNK + r]; it grows to ESP_MANY_CHUNK * n doubles at the first such call), so one
 *     read of a factor entry serves the chunk.  Block, Colored and LU's column form add one gather and one scatter per chunk on
 *     their permuted path and nothing on the identity path; an inner Jacobi / ILU0 runs the kernels of the line above.
 *   - SPAI-1, AMG and RS-AMG: the single call's launches column after column inside the one call.
 * esp_precon_many_stats: read-only; the most recent many-column solve this preconditioner ran, through esp_precon_ldiv_many or as
 *   the last preconditioner application inside esp_cg_many / esp_gmres_many.  out[0] = its form: 0 none yet or k == 1 (the
 *   single-vector path), 1 column by column, 2 one pass over the schedules or panels for the chunk; out[1] = the columns of the last
 *   chunk; out[2] = the level launches that chunk issued, forward plus backward (0 for a kind without level schedules);
 *   out[3] = the chunks of the last call.  A kind that holds a derived matrix answers with its inner preconditioner's record, as
 *   esp_precon_launches does. */
#define ESP_MANY_CHUNK 8
int32_t esp_mul_many(esp_handle *h, const double *X, int64_t ldx, double *R, int64_t ldr, int64_t k, int32_t on_device);
int32_t esp_precon_ldiv_many(esp_precon *p, const double *V, int64_t ldv, double *U, int64_t ldu, int64_t k, int32_t on_device);
int32_t esp_precon_many_stats(esp_precon *p, int64_t out[4]);
/* CONJUGATE GRADIENTS FOR SEVERAL RIGHT-HAND SIDES: esp_cg for the k columns of B (n x k column-major, leading dimension ldb) into
 * the k columns of X (ldx), as k INDEPENDENT recurrences run in lockstep, ESP_MANY_CHUNK columns at a time.  This is not block CG.
 * CONTRACT: for every column r, X[:, r], the whole residual history of r, iterations[r] and converged[r] are bit for bit what
 *   esp_cg gives for B[:, r] alone with the same arguments, whatever the other columns hold and whenever they stop.  Every column
 *   has its own rho, beta, alpha, residual, tolerance and stopping test; the summation shape of every dot product, the true
 *   divisions and the absence of contraction are esp_cg's, per column.
 * ARGUMENTS: history is (maxiter+1) x k column-major host doubles or NULL (column r holds iterations[r]+1 norms); iterations and
 *   converged hold k entries or are NULL.  ESP_ERR_INVALID: k < 0, a leading dimension below max(n, 1), any overlap of the ranges
 *   of B and X, a NULL array that would hold an element, maxiter < 0, p bound to another handle.  Every state check of esp_cg
 *   applies unchanged.  k == 1 IS esp_cg.  k == 0 returns after the state checks; for n == 0 every column has 0 iterations, is
 *   converged and has residual 0.  Rows n .. ld-1 between the columns are never read or written; B is never written.
 * HOW: all columns of a chunk share the iteration counter.  After each iteration ONE copy of 8 bytes per column brings the chunk's
 *   residual sums of squares to the host, which takes the square roots and runs every column's stop test.  A column that has
 *   stopped is frozen: the live columns go to every kernel of the next iteration as a bit mask in an argument, a frozen column's
 *   x, r and history are never written again, and the chunk ends when no column is live or at maxiter (a NaN residual keeps its
 *   column live to maxiter, as in esp_cg).  A's index and values are read once per chunk and product, and the launches of an
 *   iteration do not depend on the number of columns for Identity, Jacobi and ILU0 (many-column kernels, csrc/krylov_many.hip);
 *   CholeskyFactorization and LUFactorization's panel form run their chunked solves, ILUAM and the kinds that end in it one pass
 *   over the level schedules for the live columns (see esp_precon_ldiv_many), SPAI-1 and the AMG kinds their single ldiv! per live
 *   column.  Host arrays are staged a chunk at a time; the work vectors (4 x ESP_MANY_CHUNK x n doubles) belong to the handle. */
int32_t esp_cg_many(esp_handle *h, esp_precon *p, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k, int32_t on_device,
                    int32_t initially_zero, int64_t maxiter, double abstol, double reltol, double *history, int64_t *iterations,
                    int32_t *converged);
/* RESTARTED GMRES FOR SEVERAL RIGHT-HAND SIDES: esp_gmres for the k columns of B (n x k column-major, leading dimension ldb) into
 * the k columns of X (ldx), as k INDEPENDENT recurrences run in lockstep, ESP_MANY_CHUNK columns at a time.  This is not block
 * GMRES: every column has its own Krylov basis, H, nullvec, rhs / y, beta, acc, current, tolerance, DGKS predicate and pass counter.
 * CONTRACT: for every column r, X[:, r], the whole residual history of r, iterations[r], mv_products[r], reorth_passes[r] and
 *   converged[r] are bit for bit what esp_gmres gives for B[:, r] alone with the same arguments, whatever the other columns hold and
 *   whenever they stop.  The summation shape of every dot product, the true divisions and square roots and the absence of
 *   contraction are esp_gmres's, per column; tests/gmres_model.c stays the normative statement of the order of every operation.
 * ARGUMENTS: history is (maxiter+1) x k column-major host doubles or NULL (column r at history + r*(maxiter+1) holds
 *   iterations[r]+1 norms); iterations, mv_products, reorth_passes and converged hold k entries or are NULL.  ESP_ERR_INVALID: k < 0,
 *   a leading dimension below max(n, 1), any overlap of the ranges of B and X, a NULL array that would hold an element, p bound to
 *   another handle, and what esp_gmres refuses: restart outside 1..ESP_GMRES_RESTART_MAX, an unknown orth_meth, maxiter < 0.  Every
 *   state check of esp_gmres applies unchanged.  k == 1 with n > 0 IS esp_gmres.  k == 0 returns after the state checks; for n == 0
 *   every column has 0 iterations and products, is converged and has residual 0.  Rows n .. ld-1 between the columns are never read
 *   or written; B is never written.  Stream use and "returns synchronised" as esp_cg_many; ESP_ERR_NOMEM leaves the handle usable.
 * LOCKSTEP: the columns of a chunk share the iteration counter and the position in the cycle: they start together, so they
 *   restart together.  After each iteration ONE copy of 16 bytes per column (current, the pass count) reaches the host, which
 *   keeps every column's history and counters and runs its stop test.  The live columns go to every kernel as a bit mask in an
 *   argument (no device flag, no fence); a kernel skips a column that is not live or, in a DGKS correction pass, whose device
 *   predicate is false.  The columns that END after an iteration are all live ones when the cycle is full or at maxiter, else
 *   those with current <= tol; for them alone y is solved and x updated, with the shared m = position - 1.  Converged columns are
 *   frozen: their basis, scalars, x, history and counters are never touched again.  The others keep their position: a neighbour's
 *   convergence does not restart them.  Only a full cycle sets the position back and runs the init sequence for the columns still
 *   live.  A NaN residual keeps its column live to maxiter.  A column with current <= tol at the start (b = 0 from x = 0, a tiny b
 *   under abstol) never enters the loop: history = [r0], 0 iterations, x untouched.  maxiter == 0 touches no x.
 * HOW: the launches of an iteration equal one column's (csrc/gmres_many.hip).  Every column has its own basis, so the
 *   orthogonalisation shares no reads across columns; only Pl \ (A*v) reads A's and ILU0's index and values once per chunk
 *   (Identity, Jacobi, ILU0: many-column row kernels; CholeskyFactorization and LUFactorization's panel form: their chunked solves,
 *   a frozen column solved into scratch; ILUAM and the kinds that end in it: one pass over the level schedules for the live
 *   columns; SPAI-1 and the AMG kinds: the single ldiv! per live column).
 * WORK SPACE (the handle's, sized on first use, released with it): the basis block of (restart+1) x ESP_MANY_CHUNK vectors of n
 *   doubles rounded up to 32 -- 8.6 GB at n = 2e6 with restart 64, 2.8 GB with restart 20 --, n x ESP_MANY_CHUNK doubles of product
 *   scratch behind a preconditioner (twice that for ILU0, Cholesky and the LU panels), the partial sums (ESP_MANY_CHUNK times the
 *   single call's), ESP_MANY_CHUNK scalar blocks, and 2 n x ESP_MANY_CHUNK for host arrays, which are staged a chunk at a time. */
int32_t esp_gmres_many(esp_handle *h, esp_precon *p, const double *B, int64_t ldb, double *X, int64_t ldx, int64_t k,
                       int32_t on_device, int32_t initially_zero, int32_t restart, int32_t orth_meth, int64_t maxiter,
                       double abstol, double reltol, double *history, int64_t *iterations, int64_t *mv_products,
                       int64_t *reorth_passes, int32_t *converged);

#ifdef __cplusplus
}
#endif
#endif
