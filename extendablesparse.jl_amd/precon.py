"""The preconditioners (src/factorizations/jacobi.jl, ilu0.jl; ILUAMPreconditioner of
src/experimental/ExtendableSparseMatrixParallel/iluam.jl) and simple! (simple_iteration.jl) on the device CSC.

JacobiPreconditioner(A) / ILU0Preconditioner(A) / ILUAMPreconditioner(A) bind an esp_precon to the matrix's handle: construction is factorize!
(create + update!), .update() is update!, .ldiv(v, out) is ldiv!(out, p, v) -- bit-identical to the reference loops.
simple(A, b, Pl=...) is simple / simple!; u is bit-identical to the reference's loop, the residual norms agree to rounding
(include/esparse_hip.h, esp_simple).  Vectors: NumPy arrays (copied through the device) or CUDA float64 torch tensors (used
in place).  There is no CPU path: without a GPU the matrix itself raises NoDeviceError.
cg(A, b, Pl=...) is IterativeSolvers' cg / cg! with any of the preconditioners (or none) as the left preconditioner: x and the
residual history are identical run to run and bit-identical to the statement-by-statement model (include/esparse_hip.h, esp_cg).
bicgstabl(A, b, l, Pl=...) is IterativeSolvers' bicgstabl / bicgstabl! for non-symmetric matrices, held to its model in the same
way (include/esparse_hip.h, esp_bicgstabl).
gmres(A, b, Pl=..., restart=..., orth_meth=...) is IterativeSolvers' gmres / gmres!, restarted GMRES with modified or classical
Gram-Schmidt or DGKS re-orthogonalisation, the fallback where BiCGStab(l) breaks down, held to its model in the same way
(include/esparse_hip.h, esp_gmres).
BlockPreconditioner(A, partitioning, factorization) (src/factorizations/blockpreconditioner.jl) solves every A[part, part] with one
of the three point kinds: one block matrix and one inner preconditioner on the device, bit-identical to the per-block loops.
AMGPreconditioner(A) (= SA_AMGPreconditioner, ext/ExtendableSparseAlgebraicMultigridExt.jl) is a smoothed-aggregation V-cycle whose
hierarchy is built on the device; the algorithm is the one include/esparse_hip.h states (esp_precon_amg_create), bit-identical to
tests/amg_model.c.  RS_AMGPreconditioner(A) is the same V-cycle over a hierarchy coarsened the classical (Ruge-Stueben) way -- row-wise
strength, a PMIS splitting, direct interpolation (esp_precon_rsamg_create) -- bit-identical to tests/rsamg_model.c.
ILUKPreconditioner(A, k) is the level-of-fill ILU(k): the filled pattern found on the device by one bounded search per column, then
ILUAMPreconditioner of the filled matrix (esp_precon_iluk_create) -- bit-identical to tests/iluam_model.c on the B of tests/iluk_model.c.
ColoredPreconditioner(A, factorization) colours A's graph on the device (rounds over a fixed hash, esp_graph_coloring), reorders A by
(colour, index) and runs ILU0 or ILUAM on A[c,c]: at most ncolors levels per schedule.  ParallelILU0Preconditioner(A) is the ILU0 form,
the reference's src/factorizations/parallel_ilu0.jl acting in A's numbering; graphcol, reordermatrix and reorderlinsys are its helpers.
SPAIPreconditioner(A, order, symmetric) is the sparse approximate inverse SPAI-0 / SPAI-1 (esp_precon_spai_create): M ~ inv(A) on A's
pattern from one small least-squares problem per column, ldiv! one sparse product -- bit-identical to tests/spai_model.c.
AMGCL_RLXPreconditioner(A, type="spai0" | "spai1" | "ilut") is the reference-named constructor over it (ext/ExtendableSparseAMGCLWrapExt.jl).
ILUTPreconditioner(A, droptol, steps, sweeps, max_fill, keep_pattern) is the threshold ILU (ext/ExtendableSparseIncompleteLUExt.jl) as
synchronous sweeps with candidates and drops between them (esp_precon_ilut_create), applied by ILUAM's solves -- bit-identical to
tests/ilut_model.c.
LUFactorization(A, leaf_size, max_depth) (= SparspakLU; lu, lu_, factorize_, issolver, and A.solve(b) for `A \\ b`) is the direct solver:
a nested-dissection ordering found on the device, a supernodal symbolic fill from the dissection tree and ILUAM's factorization and
solves on the filled, reordered matrix (esp_precon_lu_create) -- no pivoting; bit-identical to tests/iluam_model.c on the B of
tests/lu_model.c.  nested_dissection(A) gives the ordering alone.
"""
import ctypes as C
import math

import numpy as np

from ._lib import ESP_ORTH_CGS, ESP_ORTH_DGKS, ESP_ORTH_MGS, ESP_PRECON_AMG, ESP_PRECON_BLOCK, ESP_PRECON_COLORED, ESP_PRECON_ILU0, ESP_PRECON_ILUAM, ESP_PRECON_ILUK, ESP_PRECON_ILUT, ESP_PRECON_JACOBI, ESP_PRECON_LU, ESP_PRECON_SPAI, ESP_CHOL_STATS, ESP_PRECON_CHOLESKY
from .matrix import ExtendableSparseMatrix, _is_cuda, _many_ptr, _many_result, _vp, many_layout


def _check_cuda(t, n):
    import torch
    assert t.is_cuda and t.dtype == torch.float64 and t.numel() == n and t.is_contiguous()


def _handover(n, b, x, what, zeros=True, r_shadow=None):
    """The vector hand-over of every call.  b: a NumPy array (copied through the device) or a CUDA float64 tensor (used in place);
    x: the result vector, `what` in the messages, or None for a new one where b lives (zeros, or uninitialised); r_shadow:
    bicgstabl's.  Returns (pointer of b, of x, of r_shadow or None, on_device, x)."""
    if _is_cuda(b):
        import torch
        _check_cuda(b, n)
        if x is None:
            x = (torch.zeros if zeros else torch.empty)(n, dtype=torch.float64, device=b.device)
        _check_cuda(x, n)
        if r_shadow is not None:
            if not _is_cuda(r_shadow):
                raise ValueError("r_shadow must live where b does")
            if r_shadow.numel() != n:
                raise ValueError("DimensionMismatch")
            _check_cuda(r_shadow, n)
        torch.cuda.current_stream(b.device).synchronize()   # the library runs on its own stream
        return [None if t is None else C.c_void_p(t.data_ptr()) for t in (b, x, r_shadow)] + [1, x]
    b = np.ascontiguousarray(b, np.float64)
    if b.shape != (n,):
        raise ValueError("DimensionMismatch")
    if x is None:
        x = (np.zeros if zeros else np.empty)(n, np.float64)
    if not (isinstance(x, np.ndarray) and x.dtype == np.float64 and x.shape == (n,) and x.flags.c_contiguous):
        raise ValueError("%s must be a contiguous float64 array of length n" % what)
    if r_shadow is not None:
        if _is_cuda(r_shadow):
            raise ValueError("r_shadow must live where b does")
        r_shadow = np.ascontiguousarray(r_shadow, np.float64)
        if r_shadow.shape != (n,):
            raise ValueError("DimensionMismatch")
    return [None if a is None else _vp(a) for a in (b, x, r_shadow)] + [0, x]   # (a pointer keeps its array alive)


def _check_solver(name, A, Pl):
    if not isinstance(A, ExtendableSparseMatrix):
        raise TypeError("%s(A, b): A must be an ExtendableSparseMatrix" % name)
    if Pl is not None and (not isinstance(Pl, _PointPreconditioner) or Pl.A is not A):
        raise ValueError("%s: Pl must be a preconditioner of A, or None" % name)


class _PointPreconditioner:
    KIND = None

    def __init__(self, A):
        if not isinstance(A, ExtendableSparseMatrix):
            raise TypeError("%s(A): A must be an ExtendableSparseMatrix" % type(self).__name__)
        self._bind(A, "esp_precon_create", self.KIND)  # factorize!: jacobi(A) / ilu0(A)

    def _bind(self, A, create, *args):
        """factorize!: flush!, then the library's `create`(A's handle, *args, &p) -- the new esp_precon is bound to A"""
        self.A = A
        self._p = None
        A.flush()
        d = A._d
        p = C.c_void_p()
        d.ck(getattr(d.lib, create)(d.h, *args, C.byref(p)))
        self._p = p

    def _ck(self, rc):
        self.A._d.ck(rc)

    def _live(self):
        if self._p is None:
            raise ValueError("the preconditioner was closed")
        return self._p

    def update(self):
        """update! (jacobi.jl:54-64, ilu0.jl:120-130): flush! first (host edits of a handed-out copy go up as well), then a
        rebuild after a pattern change, else the values only."""
        p = self._live()
        self.A.flush()
        self._ck(self.A._d.lib.esp_precon_update(p))
        return self

    def ldiv(self, v, out=None):
        """ldiv!(out, p, v); out may be v.  NumPy arrays or CUDA torch tensors (float64, contiguous, n elements).
        A 2-D (n, k) v solves k right-hand sides in one call (esp_precon_ldiv_many: every column is ldiv's bits): a NumPy array of
        any order, brought to column-major once, gives an F-ordered (n, k) array; a tensor needs stride(0) == 1 and
        stride(1) >= n and is used in place.  out=v is the in-place solve."""
        p = self._live()
        A = self.A
        A._push_edits()   # (a device consumer: host edits of a handed-out copy go up first, as for mul)
        if getattr(v, "ndim", 1) != 1:
            V, ldv, k = many_layout(A.n, v)
            U, ldu = _many_result(A.n, k, V, out, "out")
            if _is_cuda(V):
                import torch
                torch.cuda.current_stream(V.device).synchronize()   # the library runs on its own stream
            self._ck(A._d.lib.esp_precon_ldiv_many(p, _many_ptr(V), ldv, _many_ptr(U), ldu, k, 1 if _is_cuda(V) else 0))
            return U
        pv, pu, _, dev, u = _handover(A.n, v, out, "out", zeros=False)
        self._ck(A._d.lib.esp_precon_ldiv(p, pv, pu, dev))
        return u

    def _host_csc(self, h, n):
        """the matrix of handle h (n columns) as host CSC arrays (colptr, rowval, nzval), Julia layout"""
        lib = self.A._d.lib
        nnz = C.c_int64()
        self._ck(lib.esp_nnz(h, C.byref(nnz)))
        cp, rv, nz = np.empty(n + 1, np.int64), np.empty(nnz.value, np.int64), np.empty(nnz.value, np.float64)
        self._ck(lib.esp_get_csc(h, _vp(cp), _vp(rv), _vp(nz)))
        return cp, rv, nz

    def close(self):
        if self._p is not None:
            self.A._d.lib.esp_precon_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class JacobiPreconditioner(_PointPreconditioner):
    """JacobiPreconditioner(A) (src/factorizations/jacobi.jl): ldiv! is u = invdiag .* v."""
    KIND = ESP_PRECON_JACOBI


class ILU0Preconditioner(_PointPreconditioner):
    """ILU0Preconditioner(A) (src/factorizations/ilu0.jl): ldiv! as two row-parallel passes, bit-identical to the
    reference's column loops."""
    KIND = ESP_PRECON_ILU0


class _ILUAMFactors:
    """factor() and levels() of the kinds that hold an ILUAM factorization: ILUAMPreconditioner (of A itself), BlockPreconditioner,
    ILUKPreconditioner and ColoredPreconditioner (of their matrix B: the inner preconditioner answers)"""

    def _factored(self):
        """the handle of the matrix the factorization belongs to"""
        self.A.flush()
        return self.A._d.h

    def factor(self):
        """the factorization's values in the position order of the factored CSC (ILUAM: A's, the reference's ILU.nzval; Block,
        ILU(k) and Colored: the inner ILUAM's, B's): unit-lower L scaled below the diagonal, U on and above it"""
        p = self._live()
        nnz = C.c_int64()
        self._ck(self.A._d.lib.esp_nnz(self._factored(), C.byref(nnz)))
        out = np.empty(nnz.value, np.float64)
        self._ck(self.A._d.lib.esp_precon_get_factor(p, _vp(out), 0))
        return out

    def levels(self):
        """level counts of the three schedules: (factorization columns, forward rows, backward rows); Block: the inner
        preconditioner's (ILUAM: the maximum over the blocks, not their sum)"""
        out = (C.c_int64 * 3)()
        self._ck(self.A._d.lib.esp_precon_levels(self._live(), out))
        return tuple(int(x) for x in out)

    def launches(self):
        """(wide, thin) kernel launches of the three schedules, in levels()' order: a level of more than 256 nodes is one wide
        launch, consecutive levels that together hold at most 256 nodes share one thin, single-workgroup launch"""
        out = (C.c_int64 * 6)()
        self._ck(self.A._d.lib.esp_precon_launches(self._live(), out))
        return tuple((int(out[2 * k]), int(out[2 * k + 1])) for k in range(3))

    def many_stats(self):
        """(form, columns of the last chunk, level launches of that chunk, chunks of the call) of the most recent solve with
        several right-hand sides (esp_precon_many_stats) -- ldiv with a 2-D v, or the last preconditioner application inside
        cg / gmres with a 2-D b.  form: 0 none yet or one column, 1 column by column, 2 one pass over the level schedules for a
        chunk of ESP_MANY_CHUNK columns; the level launches then equal launches()' forward plus backward entries"""
        out = (C.c_int64 * 4)()
        self._ck(self.A._d.lib.esp_precon_many_stats(self._live(), out))
        return tuple(int(x) for x in out)

    def debug_factor_form(self, form):
        """test hook (esp_debug_iluam_form), takes effect at the next update(): 0 the automatic choice between the two forms of the
        column factorization, 1 always a lane per column, 2 always a wave per column -- the results never change"""
        self._ck(self.A._d.lib.esp_debug_iluam_form(self._live(), int(form)))
        return self

    def last_factor_form(self):
        """the form the last numeric factorization ran (esp_debug_last_iluam_form): 0 none, 1 lane, 2 wave"""
        form = C.c_int32()
        self._ck(self.A._d.lib.esp_debug_last_iluam_form(self._live(), C.byref(form)))
        return form.value


class ILUAMPreconditioner(_ILUAMFactors, _PointPreconditioner):
    """ILUAMPreconditioner(A) (src/experimental/ExtendableSparseMatrixParallel/iluam.jl): a real ILU(0) on A's pattern, the
    factorization and both triangular solves level by level on the device, bit-identical to the reference's sequential
    loops.  It owns a copy of the values: a value change of A reaches ldiv only through update()."""
    KIND = ESP_PRECON_ILUAM


class BlockPreconditioner(_ILUAMFactors, _PointPreconditioner):
    """BlockPreconditioner(A; partitioning, factorization) (src/factorizations/blockpreconditioner.jl, docs/src/iter.md):
    ldiv! is u[part] = factorization(A[part, part]) \\ v[part] for every partition, bit-identical to the reference's per-block
    loops (include/esparse_hip.h, esp_precon_block_create).

    partitioning: a sequence of index sequences or ranges in the index base of A[i, j] (1-based, like Julia's 1:2:n), which
    together hold every index 1..n exactly once.  factorization: JacobiPreconditioner, ILU0Preconditioner or
    ILUAMPreconditioner; it is required.  .path is 0 when every partition is increasing (nothing is permuted), else 1.
    The blocks are factorized from copies: a value change of A reaches ldiv only through update(), for ILU0 too."""
    KIND = ESP_PRECON_BLOCK

    def __init__(self, A, partitioning=None, factorization=None):
        if not isinstance(A, ExtendableSparseMatrix):
            raise TypeError("BlockPreconditioner(A, ...): A must be an ExtendableSparseMatrix")
        if factorization is None:
            raise TypeError("BlockPreconditioner: factorization is required -- the reference's default, LUFactorization, is not "
                            "on the device; pass JacobiPreconditioner, ILU0Preconditioner or ILUAMPreconditioner")
        if not (isinstance(factorization, type) and issubclass(factorization, _PointPreconditioner)
                and factorization.KIND in (ESP_PRECON_JACOBI, ESP_PRECON_ILU0, ESP_PRECON_ILUAM)):
            raise TypeError("BlockPreconditioner: factorization must be JacobiPreconditioner, ILU0Preconditioner or "
                            "ILUAMPreconditioner (the reference's default, LUFactorization, is not on the device)")
        self.factorization = factorization
        if partitioning is None:            # blockpreconditioner.jl:46-48: one partition 1:n
            partitioning = [range(1, A.n + 1)]
        parts = [np.asarray(part, np.int64).reshape(-1) for part in partitioning]
        ptr = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(part) for part in parts], out=ptr[1:])
        idx = np.ascontiguousarray(np.concatenate(parts) - 1 if parts else np.empty(0, np.int64), np.int64)
        self._bind(A, "esp_precon_block_create", factorization.KIND, len(parts), _vp(ptr), _vp(idx), 0)

    def _block(self):
        b, path = C.c_void_p(), C.c_int32()
        self._ck(self.A._d.lib.esp_precon_block_matrix(self._live(), C.byref(b), C.byref(path)))
        return b, path.value

    @property
    def path(self):
        """0: the identity path (every partition increasing), 1: the permuted path"""
        return self._block()[1]

    def block_matrix(self):
        """the block matrix B as host CSC arrays (colptr, rowval, nzval), Julia layout -- for tests and inspection"""
        return self._host_csc(self._factored(), self.A.n)

    def _factored(self):
        return self._block()[0]


class ILUKPreconditioner(_ILUAMFactors, _PointPreconditioner):
    """ILUKPreconditioner(A, k=1): the level-of-fill ILU(k) (include/esparse_hip.h, esp_precon_iluk_create).  The filled matrix B
    holds every position of level <= k -- A's entries at level 0, +0.0 where elimination creates an entry -- and the
    preconditioner is ILUAMPreconditioner of B: k = 0 is ILUAMPreconditioner(A), a larger k trades memory for fewer iterations,
    k >= n - 2 is the complete LU without pivoting.  The pattern depends on A's structure alone; unlike the AMG kinds it needs no
    symmetric pattern.  B holds copies: a value change of A reaches ldiv only through update(), which keeps the pattern, the
    analysis and the schedules when only values changed."""
    KIND = ESP_PRECON_ILUK

    def __init__(self, A, k=1):
        if not isinstance(A, ExtendableSparseMatrix):
            raise TypeError("ILUKPreconditioner(A, k): A must be an ExtendableSparseMatrix")
        if int(k) != k or k < 0:
            raise ValueError("ILUKPreconditioner: k = %r (an integer >= 0)" % (k,))
        self.k = min(int(k), 2 ** 31 - 1)     # (a level never exceeds n - 2 < 2^32 - 16)
        self._bind(A, "esp_precon_iluk_create", self.k)

    def stats(self):
        """dict: nnz (of B), max_level (the largest stored level), wide_lower / wide_upper (the columns whose search outgrew
        the one-wave form and was redone by a workgroup)"""
        out = (C.c_int64 * 4)()
        self._ck(self.A._d.lib.esp_precon_iluk_stats(self._live(), out))
        return {"nnz": int(out[0]), "max_level": int(out[1]), "wide_lower": int(out[2]), "wide_upper": int(out[3])}

    def fill_matrix(self):
        """the filled matrix B as host CSC arrays (colptr, rowval, nzval), Julia layout -- for tests and inspection"""
        return self._host_csc(self._factored(), self.A.n)

    def _factored(self):
        b = C.c_void_p()
        self._ck(self.A._d.lib.esp_precon_iluk_matrix(self._live(), C.byref(b)))
        return b

    def fill_levels(self):
        """the level of every stored entry of B (int32, B's position order): 0 for A's entries"""
        out = np.empty(self.stats()["nnz"], np.int32)
        self._ck(self.A._d.lib.esp_precon_iluk_levels(self._live(), _vp(out), 0))
        return out


class ColoredPreconditioner(_ILUAMFactors, _PointPreconditioner):
    """ColoredPreconditioner(A, factorization=ILUAMPreconditioner): the multicolour ordering (include/esparse_hip.h,
    esp_precon_colored_create).  A's graph -- i and j are neighbours when A[i,j] or A[j,i] is stored -- is coloured on the device by
    rounds over a fixed hash, c holds the unknowns sorted by (colour, index), and ldiv! is u[c] = factorization(A[c,c]) \\ v[c]: one
    gather, the inner kind's launches, one scatter.  No two unknowns of one colour are coupled, so ILUAM's schedules on A[c,c] have at
    most ncolors levels.  factorization: ILU0Preconditioner or ILUAMPreconditioner.  It acts in A's numbering (a drop-in Pl for A;
    the reference's ParallelILU0Preconditioner wants the reordered system).  A[c,c] holds copies: a value change of A reaches ldiv
    only through update(), which keeps the colouring and the analysis when only values changed and re-colours after a pattern change."""
    KIND = ESP_PRECON_COLORED

    def __init__(self, A, factorization=None):
        if not isinstance(A, ExtendableSparseMatrix):
            raise TypeError("%s(A, ...): A must be an ExtendableSparseMatrix" % type(self).__name__)
        if factorization is None:
            factorization = ILUAMPreconditioner
        if not (isinstance(factorization, type) and issubclass(factorization, _PointPreconditioner)
                and factorization.KIND in (ESP_PRECON_ILU0, ESP_PRECON_ILUAM)):
            raise TypeError("ColoredPreconditioner: factorization must be ILU0Preconditioner or ILUAMPreconditioner")
        self.factorization = factorization
        self._bind(A, "esp_precon_colored_create", factorization.KIND)

    def _info(self):
        out = (C.c_int64 * 2)()
        self._ck(self.A._d.lib.esp_precon_colored_info(self._live(), out))
        return int(out[0]), int(out[1])

    @property
    def ncolors(self):
        """the number of colours (= the rounds of the colouring)"""
        return self._info()[0]

    def colors(self):
        """the colour of every unknown: int64, 0-based"""
        out = np.empty(self.A.n, np.int64)
        if self.A.n:
            self._ck(self.A._d.lib.esp_precon_colored_colors(self._live(), _vp(out), 0))
        return out

    def permutation(self):
        """c, the unknowns sorted by (colour, index), in the index base of A[i, j] (1-based): flatten(coloring)"""
        out = np.empty(self.A.n, np.int64)
        if self.A.n:
            self._ck(self.A._d.lib.esp_precon_colored_perm(self._live(), _vp(out), 0))
        return out + 1

    def coloring(self):
        """the colours as a list of 1-based index arrays, each ascending: the shape of the reference's `coloring`"""
        col, c = self.colors(), self.permutation()
        cuts = np.cumsum(np.bincount(col, minlength=self.ncolors))[:-1] if len(col) else []
        return [np.ascontiguousarray(a) for a in np.split(c, cuts)] if len(col) else []

    def reordered_matrix(self):
        """A[c,c] as host CSC arrays (colptr, rowval, nzval), Julia layout -- for tests and inspection"""
        return self._host_csc(self._factored(), self.A.n)

    def _factored(self):
        b = C.c_void_p()
        self._ck(self.A._d.lib.esp_precon_colored_matrix(self._live(), C.byref(b)))
        return b


class ParallelILU0Preconditioner(ColoredPreconditioner):
    """ParallelILU0Preconditioner(A) (src/factorizations/parallel_ilu0.jl): ColoredPreconditioner(A, ILU0Preconditioner)"""

    def __init__(self, A):
        super().__init__(A, ILU0Preconditioner)


def graphcol(A):
    """graphcol(A) (parallel_ilu0.jl): the multicolouring of A's graph as a list of 1-based index arrays, found on the device by
    esp_graph_coloring's rule (rounds over a fixed hash in place of the reference's rand)"""
    if not isinstance(A, ExtendableSparseMatrix):
        raise TypeError("graphcol(A): A must be an ExtendableSparseMatrix")
    A.flush()
    d = A._d
    nc = C.c_int64()
    col = np.empty(A.n, np.int64)
    d.ck(d.lib.esp_graph_coloring(d.h, C.byref(nc), _vp(col) if A.n else None, 0))
    return [np.flatnonzero(col == r).astype(np.int64) + 1 for r in range(nc.value)]


def _flatten(coloring, n):
    c = np.concatenate([np.asarray(a, np.int64).reshape(-1) for a in coloring]) - 1 if len(coloring) else np.empty(0, np.int64)
    if len(c) != n or not np.array_equal(np.sort(c), np.arange(n)):
        raise ValueError("coloring must hold every index 1..n exactly once")
    return c


def reordermatrix(A, coloring):
    """reordermatrix(A, coloring) (parallel_ilu0.jl): A[c,c] with c = flatten(coloring) as a new ExtendableSparseMatrix, every column
    sorted by row, the values bitwise A's.  A host-side helper, no hot path."""
    if not isinstance(A, ExtendableSparseMatrix) or A.m != A.n:
        raise TypeError("reordermatrix(A, coloring): A must be a square ExtendableSparseMatrix")
    from .matrix import SparseMatrixCSC
    n = A.n
    c = _flatten(coloring, n)
    cp, rv, nz = (np.asarray(a) for a in A.sparse().arrays())
    new = np.empty(n, np.int64)
    new[c] = np.arange(n)
    lens = np.diff(cp)[c]
    ncp = np.ones(n + 1, np.int64)
    np.cumsum(lens, out=ncp[1:])
    ncp[1:] += 1
    src = np.concatenate([np.arange(cp[j] - 1, cp[j + 1] - 1) for j in c]) if n else np.empty(0, np.int64)
    src = src.astype(np.int64)
    rows = new[rv[src] - 1]
    colof = np.repeat(np.arange(n), lens)
    order = np.lexsort((rows, colof))
    return ExtendableSparseMatrix(SparseMatrixCSC(n, n, ncp, rows[order] + 1, np.asarray(nz, np.float64)[src[order]]))


def reorderlinsys(A, b, coloring):
    """reorderlinsys(A, b, coloring) (parallel_ilu0.jl): (A[c,c], b[c]) with c = flatten(coloring)"""
    b = np.asarray(b, np.float64)
    return reordermatrix(A, coloring), np.ascontiguousarray(b[_flatten(coloring, A.n)])


class SPAIPreconditioner(_PointPreconditioner):
    """SPAIPreconditioner(A, order=1, symmetric=False): the sparse approximate inverse (include/esparse_hip.h,
    esp_precon_spai_create).  M minimises |I - A*M|_F over the pattern of A, column by column from independent small least-squares
    problems (modified Gram-Schmidt on the device), and ldiv! is u = M*v: one sparse product, no triangular solve, no levels.
    order=0 is the diagonal member SPAI-0 (ldiv! is u = m .* v).  symmetric=True (order 1) applies 0.5*(M + transpose(M)), the form
    cg needs.  The pattern of M depends on A's pattern alone; M holds results: a value change of A reaches ldiv only through
    update(), which keeps every index structure when only values changed."""
    KIND = ESP_PRECON_SPAI

    def __init__(self, A, order=1, symmetric=False):
        if not isinstance(A, ExtendableSparseMatrix):
            raise TypeError("%s(A, ...): A must be an ExtendableSparseMatrix" % type(self).__name__)
        if order not in (0, 1):
            raise ValueError("SPAIPreconditioner: order = %r (0: SPAI-0, 1: SPAI-1)" % (order,))
        if symmetric and order == 0:
            raise ValueError("SPAIPreconditioner: SPAI-0 is diagonal; symmetric belongs to order 1")
        self.order, self.symmetric = int(order), bool(symmetric)
        self._bind(A, "esp_precon_spai_create", self.order, int(self.symmetric))

    def _applied(self):
        m = C.c_void_p()
        self._ck(self.A._d.lib.esp_precon_spai_matrix(self._live(), C.byref(m)))
        return m

    def matrix(self):
        """the applied M (order 1) as host CSC arrays (colptr, rowval, nzval), Julia layout -- for tests and inspection"""
        return self._host_csc(self._applied(), self.A.n)

    def factor(self):
        """the values of the applied M in its position order; order 0: the n diagonal values"""
        p = self._live()
        if self.order == 0:
            count = self.A.n
        else:
            nnz = C.c_int64()
            self._ck(self.A._d.lib.esp_nnz(self._applied(), C.byref(nnz)))
            count = nnz.value
        out = np.empty(count, np.float64)
        self._ck(self.A._d.lib.esp_precon_get_factor(p, _vp(out), 0))
        return out

    def issymmetric(self):
        """issymmetric of the applied M (order 1), on the device"""
        r = C.c_int32()
        self._ck(self.A._d.lib.esp_issymmetric(self._applied(), C.byref(r)))
        return bool(r.value)

    def stats(self):
        """dict: max_p / max_q (the largest row set / column of a local problem), max_pq (its largest size in doubles), wide (the
        columns the workgroup tier handled); zeros for order 0"""
        out = (C.c_int64 * 4)()
        self._ck(self.A._d.lib.esp_precon_spai_stats(self._live(), out))
        return {"max_p": int(out[0]), "max_q": int(out[1]), "max_pq": int(out[2]), "wide": int(out[3])}


class ILUTPreconditioner(_ILUAMFactors, _PointPreconditioner):
    """ILUTPreconditioner(A, droptol=1e-3, steps=3, sweeps=3, max_fill=32.0, keep_pattern=False): the threshold ILU
    (ext/ExtendableSparseIncompleteLUExt.jl; include/esparse_hip.h, esp_precon_ilut_create).  The factorization is the fixed point of
    l_ij = (a_ij - sum l_ik u_kj)/u_jj, u_ij = a_ij - sum l_ik u_kj; every entry is updated at once from the previous values
    (`sweeps` sweeps per phase), and each of the `steps` rounds adds the positions of pattern(L*U) as candidates, sweeps, drops every
    l_ij with |l_ij| < droptol and every u_ij with |u_ij| < droptol*|u_ii|, and sweeps again.  The set-up has no sequential dependency;
    ldiv is ILUAMPreconditioner's level-scheduled solves over the result.  max_fill bounds the candidates (times nnz(A)): beyond it
    the update raises and the previous factorization stays.  update() repeats the construction -- the pattern depends on the values --
    unless keep_pattern is set and A's pattern is unchanged: then the pattern and every index stay, and `sweeps` sweeps start from
    the current factors and A's new values (a Newton step's update).  DEVIATION from IncompleteLU.jl: its drop rule measures against
    the norms of A's rows and columns inside a sequential elimination."""
    KIND = ESP_PRECON_ILUT

    def __init__(self, A, droptol=1e-3, steps=3, sweeps=3, max_fill=32.0, keep_pattern=False):
        if not isinstance(A, ExtendableSparseMatrix):
            raise TypeError("ILUTPreconditioner(A, ...): A must be an ExtendableSparseMatrix")
        if not float(droptol) >= 0.0:
            raise ValueError("ILUTPreconditioner: droptol = %r (>= 0)" % (droptol,))
        if int(steps) != steps or not 0 <= steps <= 16:
            raise ValueError("ILUTPreconditioner: steps = %r (an integer in 0..16)" % (steps,))
        if int(sweeps) != sweeps or not 1 <= sweeps < 2 ** 31:
            raise ValueError("ILUTPreconditioner: sweeps = %r (an integer >= 1)" % (sweeps,))
        if not float(max_fill) >= 1.0:
            raise ValueError("ILUTPreconditioner: max_fill = %r (>= 1)" % (max_fill,))
        self.droptol, self.steps, self.sweeps = float(droptol), int(steps), int(sweeps)
        self.max_fill, self.keep_pattern = float(max_fill), bool(keep_pattern)
        self._bind(A, "esp_precon_ilut_create", C.c_double(self.droptol), self.steps, self.sweeps, C.c_double(self.max_fill),
                   int(self.keep_pattern))

    def _factored(self):
        f = C.c_void_p()
        self._ck(self.A._d.lib.esp_precon_ilut_matrix(self._live(), C.byref(f)))
        return f

    def matrix(self):
        """the pattern S with the factors F as host CSC arrays (colptr, rowval, nzval), Julia layout: the scaled unit-lower L below
        the diagonal, U on and above it -- for tests and inspection"""
        return self._host_csc(self._factored(), self.A.n)

    def stats(self):
        """dict: nnz (of S), sweeps (run by the last update), steps: [(nnz(C), nnz(S)) of every step], wave / group / stride: the
        columns of S each tier of the sweep kernel serves"""
        out = (C.c_int64 * 40)()
        self._ck(self.A._d.lib.esp_precon_ilut_stats(self._live(), out))
        return {"nnz": int(out[5]), "sweeps": int(out[1]), "steps": [(int(out[8 + 2 * t]), int(out[9 + 2 * t])) for t in range(int(out[0]))],
                "wave": int(out[2]), "group": int(out[3]), "stride": int(out[4])}


class LUFactorization(_ILUAMFactors, _PointPreconditioner):
    """LUFactorization(A, leaf_size=32, max_depth=48) (src/factorizations/umfpack_lu.jl, sparspak.jl; docs/src/linearsolve.md): a
    sparse LU without pivoting (include/esparse_hip.h, esp_precon_lu_create).  A's graph is ordered by nested dissection on the device
    -- components, two breadth-first searches and a middle level set as the separator, round by round --, the dissection tree predicts
    a superset of the fill (a dense block per node plus the ancestors next to its subtree), and the factorization is
    ILUAMPreconditioner of the filled, reordered matrix B: the exact LU of A[c,c].  solve(b) = ldiv is u[c] = ILUAM(B) \\ v[c], the
    mirror of `lufact \\ b`; as Pl of simple it is iterative refinement.  A smaller leaf_size gives a deeper tree and less fill;
    max_depth caps the rounds (what is left becomes dense leaves).  B holds copies: a value change of A reaches solve only through
    update(), which keeps the ordering, the tree, B's pattern and the schedules when only values changed and orders anew after a
    pattern change.  DEVIATIONS from UMFPACK / Sparspak: no pivoting -- a zero or NaN pivot propagates as in ILUAM --, and the
    ordering is the one above, not AMD / MMD.
    form="columns" (the default) runs ILUAM's column kernel over B; form="panels" walks the same chains on two dense panels per tree
    node (esp_precon_lu_create_form): the permutation, the tree, B, factor() and every bit of ldiv are the same, the
    numeric factorization and the solves take a launch or two per depth of the tree instead of one per level of B's dependency
    graph.  In the panel form levels() and launches() give zeros, debug_factor_form() / last_factor_form() raise (there is no inner
    ILUAM), and panel_stats() tells what ran."""
    KIND = ESP_PRECON_LU
    FORMS = {"columns": 0, "panels": 1}

    def __init__(self, A, leaf_size=32, max_depth=48, form="columns"):
        if not isinstance(A, ExtendableSparseMatrix):
            raise TypeError("LUFactorization(A, ...): A must be an ExtendableSparseMatrix")
        if int(leaf_size) != leaf_size or not 1 <= leaf_size < 2 ** 31:
            raise ValueError("LUFactorization: leaf_size = %r (an integer >= 1)" % (leaf_size,))
        if int(max_depth) != max_depth or not 0 <= max_depth <= 64:
            raise ValueError("LUFactorization: max_depth = %r (an integer in 0..64)" % (max_depth,))
        if form not in self.FORMS:
            raise ValueError("LUFactorization: form = %r (\"columns\" or \"panels\")" % (form,))
        self.leaf_size, self.max_depth, self.form = int(leaf_size), int(max_depth), form
        self._bind_form(A)

    def _bind_form(self, A):
        if self.form == "columns":
            self._bind(A, "esp_precon_lu_create", self.leaf_size, self.max_depth)
        else:
            self._bind(A, "esp_precon_lu_create_form", self.leaf_size, self.max_depth, self.FORMS[self.form])

    def panel_stats(self):
        """the panel form's dict (esp_precon_lu_panel_stats): panel_doubles (allocated), factor_launches (of the last numeric
        factorization), ldiv_launches (of one ldiv), small_nodes / wide_nodes (taken by either form), wide_block_columns (the
        block-column steps of the wide form); an error on a column-form object"""
        out = (C.c_int64 * 6)()
        self._ck(self.A._d.lib.esp_precon_lu_panel_stats(self._live(), out))
        names = ("panel_doubles", "factor_launches", "ldiv_launches", "small_nodes", "wide_nodes", "wide_block_columns")
        return dict(zip(names, (int(x) for x in out)))

    def _factored(self):
        b = C.c_void_p()
        self._ck(self.A._d.lib.esp_precon_lu_matrix(self._live(), C.byref(b)))
        return b

    def permutation(self):
        """c, the unknowns sorted by (level descending, node, index), in the index base of A[i, j] (1-based)"""
        out = np.empty(self.A.n, np.int64)
        if self.A.n:
            self._ck(self.A._d.lib.esp_precon_lu_perm(self._live(), _vp(out), 0))
        return out + 1

    def tree(self):
        """(level, node_root) per unknown: the depth it was placed at (int32) and the 1-based unknown naming its tree node -- the
        root of its component in that round (int64); the node of v is the pair (level[v], node_root[v])"""
        level, root = np.empty(self.A.n, np.int32), np.empty(self.A.n, np.int64)
        if self.A.n:
            self._ck(self.A._d.lib.esp_precon_lu_tree(self._live(), _vp(level), _vp(root), 0))
        return level, root + 1

    def fill_matrix(self):
        """the filled, reordered matrix B as host CSC arrays (colptr, rowval, nzval), Julia layout -- for tests and inspection"""
        return self._host_csc(self._factored(), self.A.n)

    def stats(self):
        """dict: nnz (of B), rounds, deepest (level), nodes (of the tree), launches (component and search launches since the create:
        an update() with the pattern kept adds none), largest_node"""
        out = (C.c_int64 * 6)()
        self._ck(self.A._d.lib.esp_precon_lu_stats(self._live(), out))
        return dict(zip(("nnz", "rounds", "deepest", "nodes", "launches", "largest_node"), (int(x) for x in out)))

    def solve(self, b, out=None):
        """lufact \\ b: an alias of ldiv"""
        return self.ldiv(b, out)


SparspakLU = LUFactorization


class CholeskyFactorization(_PointPreconditioner):
    """CholeskyFactorization(A, leaf_size=32, max_depth=48) (src/factorizations/cholmod_cholesky.jl): A[c,c] = L L' on the device
    (include/esparse_hip.h, esp_precon_cholesky_create).  As Symmetric(A.cscmatrix) does, only A's stored upper triangle is read.
    The ordering and the tree are LUFactorization's; every tree node owns a dense column-major panel, and the numeric factorization
    and the solves walk the tree depth by depth.  solve(b) = ldiv is u[c] = L' \\ (L \\ v[c]).  The panels hold copies: a value
    change of A reaches solve only through update(), which keeps the ordering, the tables and the panels' layout when only values
    changed.  A matrix that is not positive definite raises PosDefError (it names the position in c and A's column); after such an
    update() the object refuses ldiv until an update succeeds.  DEVIATIONS from CHOLMOD: the ordering is nested dissection, not AMD;
    no LDL' fallback."""
    KIND = ESP_PRECON_CHOLESKY

    def __init__(self, A, leaf_size=32, max_depth=48):
        if not isinstance(A, ExtendableSparseMatrix):
            raise TypeError("CholeskyFactorization(A, ...): A must be an ExtendableSparseMatrix")
        if int(leaf_size) != leaf_size or not 1 <= leaf_size < 2 ** 31:
            raise ValueError("CholeskyFactorization: leaf_size = %r (an integer >= 1)" % (leaf_size,))
        if int(max_depth) != max_depth or not 0 <= max_depth <= 64:
            raise ValueError("CholeskyFactorization: max_depth = %r (an integer in 0..64)" % (max_depth,))
        self.leaf_size, self.max_depth = int(leaf_size), int(max_depth)
        self._bind(A, "esp_precon_cholesky_create", self.leaf_size, self.max_depth)

    def permutation(self):
        """c, the unknowns sorted by (level descending, node, index), in the index base of A[i, j] (1-based)"""
        out = np.empty(self.A.n, np.int64)
        if self.A.n:
            self._ck(self.A._d.lib.esp_precon_cholesky_perm(self._live(), _vp(out), 0))
        return out + 1

    def tree(self):
        """(level, node_root) per unknown, as LUFactorization.tree()"""
        level, root = np.empty(self.A.n, np.int32), np.empty(self.A.n, np.int64)
        if self.A.n:
            self._ck(self.A._d.lib.esp_precon_cholesky_tree(self._live(), _vp(level), _vp(root), 0))
        return level, root + 1

    def factor(self):
        """L as host CSC arrays (colptr, rowval, nzval) in positions of c, Julia layout -- for tests and inspection"""
        lib, n = self.A._d.lib, self.A.n
        cp = np.empty(n + 1, np.int64)
        self._ck(lib.esp_precon_cholesky_factor(self._live(), _vp(cp), None, None, 0))
        nnz = int(cp[n]) - 1
        rv, nz = np.empty(nnz, np.int64), np.empty(nnz, np.float64)
        if nnz:
            self._ck(lib.esp_precon_cholesky_factor(self._live(), None, _vp(rv), _vp(nz), 0))
        return cp, rv, nz

    def stats(self):
        """dict: nnz (of L), rounds, deepest (level), nodes, largest_node, panel_doubles, ordering_launches (since the create: an
        update() with the pattern kept adds none), factor_launches (of the last numeric factorization), ldiv_launches (of one ldiv),
        small_nodes / wide_nodes (taken by either form), wide_block_columns (the block-column steps of the wide form)"""
        out = (C.c_int64 * ESP_CHOL_STATS)()
        self._ck(self.A._d.lib.esp_precon_cholesky_stats(self._live(), out))
        names = ("nnz", "rounds", "deepest", "nodes", "largest_node", "panel_doubles", "ordering_launches", "factor_launches",
                 "ldiv_launches", "small_nodes", "wide_nodes", "wide_block_columns")
        return dict(zip(names, (int(x) for x in out)))

    def solve(self, b, out=None):
        """cholfact \\ b: an alias of ldiv"""
        return self.ldiv(b, out)


def cholesky(A, **kw):
    """cholesky(A): CholeskyFactorization(A, **kw)"""
    return CholeskyFactorization(A, **kw)


def cholesky_(fact, A):
    """cholesky!(fact, A): the factorization of A in fact -- bound anew when A is another matrix, else update()"""
    if not isinstance(fact, CholeskyFactorization):
        raise TypeError("cholesky_(fact, A): fact must be a CholeskyFactorization")
    return lu_(fact, A)


def lu(A, **kw):
    """lu(A) (docs/src/linearsolve.md): LUFactorization(A, **kw)"""
    return LUFactorization(A, **kw)


def lu_(fact, A):
    """lu!(fact, A): the factorization of A in fact -- bound anew when A is another matrix, else update().  A CholeskyFactorization
    is taken too (the reference's tests call lu!(CholeskyFactorization(), A))"""
    if not isinstance(fact, (LUFactorization, CholeskyFactorization)):
        raise TypeError("lu_(fact, A): fact must be an LUFactorization or a CholeskyFactorization")
    if not isinstance(A, ExtendableSparseMatrix):
        raise TypeError("lu_(fact, A): A must be an ExtendableSparseMatrix")
    if A is fact.A and fact._p is not None:
        return fact.update()
    fact.close()
    if isinstance(fact, CholeskyFactorization):
        fact._bind(A, "esp_precon_cholesky_create", fact.leaf_size, fact.max_depth)
    else:
        fact._bind_form(A)   # (the object keeps its form)
    return fact


def factorize_(fact, A):
    """factorize!(fact, A) (src/factorizations/factorizations.jl): lu_ for an LUFactorization; a preconditioner is bound to its
    matrix and takes update()"""
    if isinstance(fact, (LUFactorization, CholeskyFactorization)):
        return lu_(fact, A)
    if not isinstance(fact, _PointPreconditioner):
        raise TypeError("factorize_(fact, A): fact must be a factorization or a preconditioner")
    if A is not fact.A:
        raise ValueError("factorize_: a preconditioner is bound to its matrix; create a new one for another matrix")
    return fact.update()


def issolver(f):
    """issolver(f) (factorizations.jl): True for the direct solvers LUFactorization and CholeskyFactorization (an instance or the
    class), False for every preconditioner"""
    direct = (LUFactorization, CholeskyFactorization)
    return isinstance(f, direct) or (isinstance(f, type) and issubclass(f, direct))


def nested_dissection(A, leaf_size=32, max_depth=48):
    """the nested-dissection ordering of A's graph alone (esp_nested_dissection) -> (perm, level): the 1-based permutation c and the
    depth every unknown was placed at (int32)"""
    if not isinstance(A, ExtendableSparseMatrix):
        raise TypeError("nested_dissection(A): A must be an ExtendableSparseMatrix")
    A.flush()
    d = A._d
    c, level = np.empty(A.n, np.int64), np.empty(A.n, np.int32)
    d.ck(d.lib.esp_nested_dissection(d.h, int(leaf_size), int(max_depth), _vp(c) if A.n else None, _vp(level) if A.n else None, 0))
    return c + 1, level


def solve(A, b, form="columns"):
    """A \\ b: A.solve(b, form=form)"""
    if not isinstance(A, ExtendableSparseMatrix):
        raise TypeError("solve(A, b): A must be an ExtendableSparseMatrix")
    return A.solve(b, form=form)


def AMGCL_RLXPreconditioner(A, type="spai0"):
    """AMGCL_RLXPreconditioner(A; type) (ext/ExtendableSparseAMGCLWrapExt.jl): the relaxation preconditioners of AMGCL.  On the
    device: "spai0" and "spai1", as SPAIPreconditioner(A, order=0 / 1), and "ilut", as ILUTPreconditioner(A) with its defaults --
    whose drop rule (|l_ij| < droptol, |u_ij| < droptol*|u_ii|, between parallel sweeps) is not AMGCL's (the p largest entries of a
    row above tau times the row's norm, inside a sequential elimination)."""
    orders = {"spai0": 0, "spai1": 1}
    if type == "ilut" and isinstance(A, ExtendableSparseMatrix):
        return ILUTPreconditioner(A)
    if type not in orders:
        raise NotImplementedError("AMGCL_RLXPreconditioner: type = %r is not on the device; \"spai0\", \"spai1\" and \"ilut\" are" % (type,))
    return SPAIPreconditioner(A, order=orders[type])


class AMGPreconditioner(_PointPreconditioner):
    """AMGPreconditioner(A; max_levels, max_coarse, presweeps, postsweeps, theta) (the reference's SA_AMGPreconditioner,
    ext/ExtendableSparseAlgebraicMultigridExt.jl): ldiv! is one smoothed-aggregation V-cycle (include/esparse_hip.h,
    esp_precon_amg_create): MIS(2) aggregates, P = (I - w.*A)*T, Galerkin coarse matrices, weighted-Jacobi sweeps, a dense
    inverse on the coarsest level.  The stored pattern must be structurally symmetric and hold every diagonal entry.  The
    hierarchy is built from copies: a value change of A reaches ldiv only through update(), which rebuilds everything."""
    KIND = ESP_PRECON_AMG
    CREATE = "esp_precon_amg_create"

    def __init__(self, A, max_levels=10, max_coarse=64, presweeps=1, postsweeps=1, theta=0.0):
        name = type(self).__name__
        if not isinstance(A, ExtendableSparseMatrix):
            raise TypeError("%s(A): A must be an ExtendableSparseMatrix" % name)
        for what, v, lo in (("max_levels", max_levels, 1), ("max_coarse", max_coarse, 1), ("presweeps", presweeps, 1),
                            ("postsweeps", postsweeps, 0)):
            if int(v) != v or v < lo:
                raise ValueError("%s: %s = %r (an integer >= %d)" % (name, what, v, lo))
        if not (theta >= 0.0 and math.isfinite(theta)):
            raise ValueError("%s: theta = %r (finite, >= 0)" % (name, theta))
        self._bind(A, self.CREATE, int(max_levels), int(max_coarse), int(presweeps), int(postsweeps), float(theta))

    @property
    def coarsening(self):
        """ESP_AMG_COARSEN_SA (0, smoothed aggregation) or ESP_AMG_COARSEN_RS (1, Ruge-Stueben)"""
        k = C.c_int32()
        self._ck(self.A._d.lib.esp_precon_amg_coarsening(self._live(), C.byref(k)))
        return k.value

    @property
    def levels(self):
        """the number of levels of the hierarchy"""
        k = C.c_int32()
        self._ck(self.A._d.lib.esp_precon_amg_levels(self._live(), C.byref(k)))
        return k.value

    def level(self, l):
        """level l as a dict: n, rho, rounds (the Luby rounds of its aggregation, 0 where none ran), A and P as host CSC arrays
        (colptr, rowval, nzval), Julia layout; P is None on the coarsest level -- for tests and inspection"""
        a, pr = C.c_void_p(), C.c_void_p()
        n, rho, rounds = C.c_int64(), C.c_double(), C.c_int32()
        self._ck(self.A._d.lib.esp_precon_amg_level(self._live(), int(l), C.byref(a), C.byref(pr), C.byref(n), C.byref(rho),
                                                    C.byref(rounds)))
        out = {"n": n.value, "rho": rho.value, "rounds": rounds.value, "A": self._host_csc(a, n.value), "P": None}
        if pr.value:
            m, nc = C.c_int64(), C.c_int64()
            self._ck(self.A._d.lib.esp_size(pr, C.byref(m), C.byref(nc)))
            out["P"] = self._host_csc(pr, nc.value)
        return out

    def aggregates(self, l):
        """the aggregate (0-based) of every unknown of level l"""
        a, n = C.c_void_p(), C.c_int64()
        self._ck(self.A._d.lib.esp_precon_amg_level(self._live(), int(l), C.byref(a), None, C.byref(n), None, None))
        out = np.empty(n.value, np.int64)
        self._ck(self.A._d.lib.esp_precon_amg_aggregates(self._live(), int(l), _vp(out), 0))
        return out

    def coarse_inverse(self):
        """the dense inverse of the coarsest level (n_L x n_L); raises if that level is only smoothed"""
        a, n = C.c_void_p(), C.c_int64()
        self._ck(self.A._d.lib.esp_precon_amg_level(self._live(), self.levels - 1, C.byref(a), None, C.byref(n), None, None))
        out = np.empty((n.value, n.value), np.float64)
        self._ck(self.A._d.lib.esp_precon_amg_coarse_inverse(self._live(), _vp(out), 0))
        return out


SA_AMGPreconditioner = AMGPreconditioner


class RS_AMGPreconditioner(AMGPreconditioner):
    """RS_AMGPreconditioner(A; max_levels, max_coarse, presweeps, postsweeps, theta) (the reference's RS_AMGPreconditioner,
    ext/ExtendableSparseAlgebraicMultigridExt.jl): AMGPreconditioner's V-cycle over a hierarchy coarsened the classical way
    (include/esparse_hip.h, esp_precon_rsamg_create): strength decided per row (|a_ij| >= theta * the row's largest off-diagonal
    magnitude), a PMIS splitting into C and F points over a fixed hash, direct interpolation.  Made for the non-symmetric
    M-matrices of upwind convection-diffusion schemes; the requirements on the stored pattern and update() are AMGPreconditioner's.
    rounds in level(l) are the rounds of the splitting; aggregates() raises."""
    CREATE = "esp_precon_rsamg_create"

    def __init__(self, A, max_levels=10, max_coarse=64, presweeps=1, postsweeps=1, theta=0.25):
        super().__init__(A, max_levels, max_coarse, presweeps, postsweeps, theta)

    def splitting(self, l):
        """the C/F splitting of level l: the 0-based coarse index of a C point, -1 for an interpolated F point, -2 for an F point
        without interpolation (no strong dependence)"""
        a, n = C.c_void_p(), C.c_int64()
        self._ck(self.A._d.lib.esp_precon_amg_level(self._live(), int(l), C.byref(a), None, C.byref(n), None, None))
        out = np.empty(n.value, np.int64)
        self._ck(self.A._d.lib.esp_precon_amg_splitting(self._live(), int(l), _vp(out), 0))
        return out


def simple(A, b, u=None, Pl=None, maxiter=100, reltol=math.sqrt(np.finfo(np.float64).eps), abstol=0.0, log=False):
    """simple / simple!(u, A, b; abstol, reltol, log, maxiter, Pl) (simple_iteration.jl:21-47): u <- u - Pl \\ (A u - b)
    until norm(res)/r0 < reltol or norm(res) < abstol.  u = None starts from zeros (simple); a given u is updated in
    place (simple!).  log=True returns (u, {"resnorm": history})."""
    if Pl is None:
        raise TypeError("simple: Pl is required (the reference's default `nothing` has no ldiv!)")
    if not isinstance(Pl, _PointPreconditioner) or Pl.A is not A:
        raise ValueError("simple: Pl must be a preconditioner of A")
    p = Pl._live()
    A.flush()
    d = A._d
    n = A.n
    maxiter = int(maxiter)
    if maxiter < 0:
        raise ValueError("maxiter < 0")
    hist = np.empty(maxiter + 1, np.float64)
    its = C.c_int64()
    pb, pu, _, dev, u = _handover(n, b, u, "u")
    d.ck(d.lib.esp_simple(d.h, p, pb, pu, dev, maxiter, float(abstol), float(reltol), _vp(hist), C.byref(its)))
    if log:
        return u, {"resnorm": hist[:its.value + 1].copy()}
    return u


def cg(A, b, Pl=None, x=None, abstol=0.0, reltol=math.sqrt(np.finfo(np.float64).eps), maxiter=None, log=False):
    """cg / cg!(x, A, b; Pl, abstol, reltol, maxiter, log) of IterativeSolvers.jl (include/esparse_hip.h, esp_cg): preconditioned
    conjugate gradients until norm(r) <= max(reltol*norm(r0), abstol) or maxiter (None: n) iterations.  x = None starts from zeros
    (cg); a given x is updated in place (cg!).  Pl: a preconditioner of A, or None (Identity).
    log=True returns (x, {"resnorm": the norm after every iteration, "r0": the initial one, "iters": k, "isconverged": bool}).
    A 2-D (n, k) b solves k right-hand sides in one call (esp_cg_many: k independent recurrences in lockstep, every column the
    single call's bits).  The layout rules are many_layout's; the result is an F-ordered (n, k) array, or a tensor with
    stride(0) == 1, living where b lives.  A given x is an (n, k) array of that layout living where b lives, updated in place.
    log=True then returns (X, logs): a list of k dicts with the single call's keys and values."""
    _check_solver("cg", A, Pl)
    p = Pl._live() if Pl is not None else None
    A.flush()
    d = A._d
    n = A.n
    maxiter = n if maxiter is None else int(maxiter)
    if maxiter < 0:
        raise ValueError("maxiter < 0")
    if getattr(b, "ndim", 1) != 1:
        return _cg_many(d, p, n, b, x, float(abstol), float(reltol), maxiter, log)
    hist = np.empty(maxiter + 1, np.float64)
    its = C.c_int64()
    conv = C.c_int32()
    zero = 1 if x is None else 0
    pb, px, _, dev, x = _handover(n, b, x, "x")
    d.ck(d.lib.esp_cg(d.h, p, pb, px, dev, zero, maxiter, float(abstol), float(reltol), _vp(hist), C.byref(its), C.byref(conv)))
    if log:
        k = its.value
        return x, {"resnorm": hist[1:k + 1].copy(), "r0": float(hist[0]), "iters": k, "isconverged": bool(conv.value)}
    return x


def _cg_many(d, p, n, b, x, abstol, reltol, maxiter, log):
    """cg with a 2-D b: the hand-over of the (n, k) arrays, esp_cg_many, the k logs"""
    B, ldb, k = many_layout(n, b)
    zero = 1 if x is None else 0
    if x is None:
        if _is_cuda(B):
            import torch
            x = torch.zeros((k, n), dtype=torch.float64, device=B.device).t()
        else:
            x = np.zeros((n, k), np.float64, order="F")
    X, ldx = _many_result(n, k, B, x, "x")
    if _is_cuda(B):
        import torch
        torch.cuda.current_stream(B.device).synchronize()   # the library runs on its own stream
    hist = np.empty((maxiter + 1, k), np.float64, order="F")
    its = np.zeros(k, np.int64)
    conv = np.zeros(k, np.int32)
    d.ck(d.lib.esp_cg_many(d.h, p, _many_ptr(B), ldb, _many_ptr(X), ldx, k, 1 if _is_cuda(B) else 0, zero, maxiter, abstol, reltol,
                           _vp(hist), _vp(its), _vp(conv)))
    if log:
        return X, [{"resnorm": hist[1:int(its[r]) + 1, r].copy(), "r0": float(hist[0, r]), "iters": int(its[r]),
                    "isconverged": bool(conv[r])} for r in range(k)]
    return X


def bicgstabl(A, b, l=2, Pl=None, x=None, abstol=0.0, reltol=math.sqrt(np.finfo(np.float64).eps), max_mv_products=None,
              r_shadow=None, log=False):
    """bicgstabl / bicgstabl!(x, A, b, l; Pl, abstol, reltol, max_mv_products, log) of IterativeSolvers.jl for non-symmetric
    systems (include/esparse_hip.h, esp_bicgstabl): BiCGStab(l), 1 <= l <= 4, with Pl as the LEFT preconditioner, until the
    preconditioned norm(r) <= max(reltol*norm(r0), abstol) or max_mv_products (None: n) matrix-vector products, tested before
    every outer iteration of 2l products.  x = None starts from zeros; a given x is updated in place.  Pl: a preconditioner of A,
    or None (Identity).  r_shadow: the shadow residual (None: the initial preconditioned residual; the package draws rand(n)).
    log=True returns (x, {"resnorm": the norm after every outer iteration, "r0": the initial one, "iters": outer iterations,
    "mvps": matrix-vector products, "isconverged": bool})."""
    _check_solver("bicgstabl", A, Pl)
    p = Pl._live() if Pl is not None else None
    A.flush()
    d = A._d
    n = A.n
    l = int(l)
    max_mv_products = n if max_mv_products is None else int(max_mv_products)
    if max_mv_products < 0:
        raise ValueError("max_mv_products < 0")
    hist = np.empty(-(-max_mv_products // (2 * l)) + 1 if l >= 1 else 1, np.float64)   # (l < 1: the call refuses)
    its, mvs = C.c_int64(), C.c_int64()
    conv = C.c_int32()
    zero = 1 if x is None else 0
    pb, px, prs, dev, x = _handover(n, b, x, "x", r_shadow=r_shadow)
    d.ck(d.lib.esp_bicgstabl(d.h, p, l, pb, px, prs, dev, zero, max_mv_products, float(abstol), float(reltol), _vp(hist),
                             C.byref(its), C.byref(mvs), C.byref(conv)))
    if log:
        k = its.value
        return x, {"resnorm": hist[1:k + 1].copy(), "r0": float(hist[0]), "iters": k, "mvps": mvs.value,
                   "isconverged": bool(conv.value)}
    return x


_ORTH = {"mgs": ESP_ORTH_MGS, "cgs": ESP_ORTH_CGS, "dgks": ESP_ORTH_DGKS}


def gmres(A, b, Pl=None, x=None, restart=None, maxiter=None, abstol=0.0, reltol=math.sqrt(np.finfo(np.float64).eps), orth_meth="mgs",
          log=False):
    """gmres / gmres!(x, A, b; Pl, abstol, reltol, restart, maxiter, orth_meth, log) of IterativeSolvers.jl for non-symmetric
    systems (include/esparse_hip.h, esp_gmres): restarted GMRES with Pl as the LEFT preconditioner, until the preconditioned
    residual norm <= max(reltol*norm(r0), abstol) or maxiter (None: n) iterations.  restart (None: max(1, min(20, n)); at most 64)
    is the length of a cycle; orth_meth is "mgs" (modified Gram-Schmidt, the package's default), "cgs" (classical) or "dgks"
    (classical with up to three correction passes).  x = None starts from zeros; a given x is updated in place.  Pl: a
    preconditioner of A, or None (Identity).
    log=True returns (x, {"resnorm": the norm after every iteration, "r0": the initial one, "iters": iterations, "mvps":
    matrix-vector products, "reorth": DGKS correction passes, "isconverged": bool}).
    A 2-D (n, k) b solves k right-hand sides in one call (esp_gmres_many: k independent recurrences in lockstep, every column the
    single call's bits; not block GMRES).  The layout rules are many_layout's; the result is an F-ordered (n, k) array, or a tensor
    with stride(0) == 1, living where b lives.  A given x is an (n, k) array of that layout living where b lives, updated in place.
    log=True then returns (X, logs): a list of k dicts with the single call's keys and values."""
    _check_solver("gmres", A, Pl)
    if orth_meth not in _ORTH:
        raise ValueError("gmres: orth_meth = %r (one of 'mgs', 'cgs', 'dgks')" % (orth_meth,))
    p = Pl._live() if Pl is not None else None
    A.flush()
    d = A._d
    n = A.n
    restart = max(1, min(20, n)) if restart is None else int(restart)
    maxiter = n if maxiter is None else int(maxiter)
    if maxiter < 0:
        raise ValueError("maxiter < 0")
    if getattr(b, "ndim", 1) != 1:
        return _gmres_many(d, p, n, b, x, restart, _ORTH[orth_meth], maxiter, float(abstol), float(reltol), log)
    hist = np.empty(maxiter + 1, np.float64)
    its, mvs, reorth = C.c_int64(), C.c_int64(), C.c_int64()
    conv = C.c_int32()
    zero = 1 if x is None else 0
    pb, px, _, dev, x = _handover(n, b, x, "x")
    d.ck(d.lib.esp_gmres(d.h, p, pb, px, dev, zero, restart, _ORTH[orth_meth], maxiter, float(abstol), float(reltol), _vp(hist),
                         C.byref(its), C.byref(mvs), C.byref(reorth), C.byref(conv)))
    if log:
        k = its.value
        return x, {"resnorm": hist[1:k + 1].copy(), "r0": float(hist[0]), "iters": k, "mvps": mvs.value, "reorth": reorth.value,
                   "isconverged": bool(conv.value)}
    return x


def _gmres_many(d, p, n, b, x, restart, orth, maxiter, abstol, reltol, log):
    """gmres with a 2-D b: the hand-over of the (n, k) arrays, esp_gmres_many, the k logs"""
    B, ldb, k = many_layout(n, b)
    zero = 1 if x is None else 0
    if x is None:
        if _is_cuda(B):
            import torch
            x = torch.zeros((k, n), dtype=torch.float64, device=B.device).t()
        else:
            x = np.zeros((n, k), np.float64, order="F")
    X, ldx = _many_result(n, k, B, x, "x")
    if _is_cuda(B):
        import torch
        torch.cuda.current_stream(B.device).synchronize()   # the library runs on its own stream
    hist = np.empty((maxiter + 1, k), np.float64, order="F")
    its, mvs, reorth = np.zeros(k, np.int64), np.zeros(k, np.int64), np.zeros(k, np.int64)
    conv = np.zeros(k, np.int32)
    d.ck(d.lib.esp_gmres_many(d.h, p, _many_ptr(B), ldb, _many_ptr(X), ldx, k, 1 if _is_cuda(B) else 0, zero, restart, orth, maxiter,
                              abstol, reltol, _vp(hist), _vp(its), _vp(mvs), _vp(reorth), _vp(conv)))
    if log:
        return X, [{"resnorm": hist[1:int(its[r]) + 1, r].copy(), "r0": float(hist[0, r]), "iters": int(its[r]), "mvps": int(mvs[r]),
                    "reorth": int(reorth[r]), "isconverged": bool(conv[r])} for r in range(k)]
    return X
