"""extendablesparse.jl_amd -- MI355X-native sparse-assembly backend for ExtendableSparseMatrix.

Only what the hot path needs: csrc/ (HIP kernels + the C ABI of include/esparse_hip.h) and the
host-side mirror of the reference's operator interface.  Importing the package never touches the
oracle and never falls back to a CPU implementation.
"""
from . import _lib
from ._lib import (ESP_AMG_COARSEN_RS, ESP_AMG_COARSEN_SA, ESP_COO, ESP_FLUSH_PLUS, ESP_FLUSH_ROUTED, ESP_OP_ADD, ESP_OP_SUB, ESP_ORTH_CGS, ESP_ORTH_DGKS, ESP_ORTH_MGS, ESP_PATH_NO_KEPT_STRUCTURE, ESP_PRECON_AMG, ESP_PRECON_BLOCK, ESP_PRECON_CHOLESKY, ESP_PRECON_COLORED, ESP_PRECON_ILU0, ESP_PRECON_ILUAM, ESP_PRECON_ILUK, ESP_PRECON_ILUT, ESP_PRECON_JACOBI, ESP_PRECON_LU, ESP_PRECON_SPAI,
                   ESP_RAWUPDATE, ESP_SET, ESP_UPDATE, BoundsError, EspError, NoDeviceError, PosDefError)
from .matrix import (Diagonal, ExtendableSparseMatrix, GenericExtendableSparseMatrixCSC,
                     GenericMTExtendableSparseMatrixCSC, SparseMatrixCSC, SparseMatrixHIPCOO, many_layout)
from . import fdrand as fdrand_module
from .fdrand import fdrand, fdrand_, fdrand_coo, fdrand_device_
from .sharded import GroupShardedMatrix, owner_ranges
from .precon import (AMGCL_RLXPreconditioner, SPAIPreconditioner, AMGPreconditioner, RS_AMGPreconditioner, SA_AMGPreconditioner, BlockPreconditioner, CholeskyFactorization, ColoredPreconditioner, ParallelILU0Preconditioner, ILU0Preconditioner, ILUAMPreconditioner, ILUKPreconditioner, ILUTPreconditioner, JacobiPreconditioner, LUFactorization, SparspakLU, bicgstabl, cg, cholesky, cholesky_,
                     factorize_, gmres, graphcol, issolver, lu, lu_, nested_dissection, reorderlinsys, reordermatrix, simple, solve)

# aliases mirroring src/ExtendableSparse.jl:34-39
ExtendableSparseMatrixCSC = ExtendableSparseMatrix
HIPExtendableSparseMatrixCSC = GenericExtendableSparseMatrixCSC
MTHIPExtendableSparseMatrixCSC = GenericMTExtendableSparseMatrixCSC


def library_path():
    return _lib.SO
