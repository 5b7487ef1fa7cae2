"""Model of RS_AMGPreconditioner (include/esparse_hip.h, esp_precon_rsamg_create; test infrastructure).  tests/rsamg_model.c is the
normative restatement of what is new -- row-wise strength, the PMIS splitting, direct interpolation; everything around it is
taken, by import, from amg_modellib: dinv, rho and w, the checks of level 0, the Galerkin products through the algebra models,
Gauss-Jordan, the V-cycle and the solver loops.  Built with gcc -O1 -ffp-contract=off into a directory the caller chooses (a
pytest temp directory)."""
import ctypes as C
import os
import subprocess

import numpy as np

import amg_modellib as am
from amg_modellib import DENSE_MAX, _csc, _p

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rsamg_model.c")


class Model(am.Model):
    """rsamg_model.c's library beside amg_modellib.Model (and, through it, the algebra models)"""

    def __init__(self, outdir):
        super().__init__(outdir)
        so = os.path.join(str(outdir), "rsamg_model.so")
        subprocess.check_call(["gcc", "-O1", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, SRC, "-lm"])
        R = C.CDLL(so)
        i64, f64, vp, i32 = C.c_int64, C.c_double, C.c_void_p, C.c_int32
        R.model_rsamg_strength.argtypes = [i64, vp, vp, vp, f64, vp]
        R.model_rsamg_strength.restype = None
        R.model_rsamg_split.argtypes = [i64, vp, vp, vp, f64, vp, C.POINTER(i32)]
        R.model_rsamg_split.restype = i64
        R.model_rsamg_interp.argtypes = [i64, vp, vp, vp, f64, vp, vp, vp, vp]
        R.model_rsamg_interp.restype = i64
        self.R = R

    def rs_strength(self, csc, theta):
        """dep[k] = 1 iff the row of the stored entry k depends on its column"""
        cp, rv, nz = _csc(csc)
        out = np.zeros(max(len(rv), 1), np.uint8)
        self.R.model_rsamg_strength(len(cp) - 1, _p(cp), _p(rv), _p(nz), float(theta), _p(out))
        return out[:len(rv)]

    def rs_split(self, csc, theta):
        """-> (cf: cnum of a C point, -1 an interpolated F point, -2 an F point without interpolation; C points; rounds)"""
        cp, rv, nz = _csc(csc)
        n = len(cp) - 1
        cf = np.empty(max(n, 1), np.int64)
        rounds = C.c_int32()
        nc = self.R.model_rsamg_split(n, _p(cp), _p(rv), _p(nz), float(theta), _p(cf), C.byref(rounds))
        return cf[:n].copy(), int(nc), rounds.value

    def rs_interp_t(self, csc, theta, cf):
        """transpose(P) (nc x n) as CSC arrays"""
        cp, rv, nz = _csc(csc)
        n = len(cp) - 1
        cf = np.ascontiguousarray(np.concatenate([cf, np.zeros(1, np.int64)]), np.int64)
        cap = len(rv) + n + 1
        tcp, trv, tnz = np.empty(n + 1, np.int64), np.empty(cap, np.int64), np.empty(cap, np.float64)
        z = self.R.model_rsamg_interp(n, _p(cp), _p(rv), _p(nz), float(theta), _p(cf), _p(tcp), _p(trv), _p(tnz))
        return tcp, trv[:z].copy(), tnz[:z].copy()


class RSAMGModel(am.AMGModel):
    """the Ruge-Stueben hierarchy of a matrix given as host CSC arrays (update! at construction); ldiv and the solver loops are
    AMGModel's"""

    def __init__(self, model, csc, max_levels=10, max_coarse=64, presweeps=1, postsweeps=1, theta=0.25):
        self.m = model.krylov
        self.model = model
        self.csc = tuple(np.array(a, copy=True) for a in _csc(csc))
        self.n = len(self.csc[0]) - 1
        self.pre, self.post = presweeps, postsweeps
        assert model.check(self.csc) == (0, 0)
        mo, la = model.matops, model.linalg
        self.levels, self.inv = [], None
        A = self.csc
        n = self.n
        while True:
            L = am.Level(n, A)
            L.cf = None
            self.levels.append(L)
            cp, rv, nz = A
            with np.errstate(all="ignore"):
                diag = np.zeros(n)
                for j in range(n):
                    for k in range(cp[j] - 1, cp[j + 1] - 1):
                        if rv[k] - 1 == j:
                            diag[j] = nz[k]
                dinv = np.float64(1.0) / diag
                L.rho = float(model.opnorm_inf(n, mo.diag_scale(A, dinv, 0)))
                omega = np.float64(4.0 / 3.0) / np.float64(L.rho)
                L.w = omega * dinv
            coarsest = n <= max_coarse or len(self.levels) == max_levels
            if not coarsest:
                L.cf, L.nc, L.rounds = model.rs_split(A, theta)
                coarsest = L.nc == 0 or L.nc == n
            if coarsest:
                if n <= DENSE_MAX:
                    with np.errstate(all="ignore"):
                        self.inv = model.gauss_jordan(am.dense_of(n, A))
                break
            nc = L.nc
            with np.errstate(all="ignore"):
                PT = model.rs_interp_t(A, theta, L.cf)
                L.P = la.transpose(nc, PT)
                AP = mo.matmul(n, A, L.P)
                A = mo.matmul(nc, PT, AP)
            n = nc

    # gmres_modellib.Model.gmres_cb(M, ...) calls M.mul and M.ldiv: both are AMGModel's


# ---- the graphs of the splitting tests ------------------------------------------------------------------------------------------
def posmix(fd, seed=3):
    """fd(9, 8, 1) with about a fifth of its off-diagonal pairs made positive and unequal: rows with positive couplings, some of them
    to C points and some not (both branches of the interpolation's positive part)"""
    cp, rv, nz = (np.array(a, copy=True) for a in fd(9, 8, 1))
    n = len(cp) - 1
    rng = np.random.default_rng(seed)
    for j in range(n):
        for k in range(cp[j] - 1, cp[j + 1] - 1):
            i = rv[k] - 1
            if i < j and rng.random() < 0.2:
                lo = cp[i] - 1 + int(np.searchsorted(rv[cp[i] - 1:cp[i + 1] - 1], j + 1))
                assert rv[lo] == j + 1
                nz[k] = abs(nz[k]) * 0.5
                nz[lo] = abs(nz[lo]) * 0.25
    return cp, rv, nz


def positive_branches(model, csc, theta):
    """(rows of level 0 with sp > 0 and spc == 0, rows with spc != 0) among the interpolated F points"""
    cp, rv, nz = _csc(csc)
    n = len(cp) - 1
    cf, _, _ = model.rs_split(csc, theta)
    dep = model.rs_strength(csc, theta)
    cols = np.repeat(np.arange(n), np.diff(cp))
    rows = rv - 1
    off = rows != cols
    sp, spc = np.zeros(n), np.zeros(n)
    np.add.at(sp, rows[off & (nz > 0)], nz[off & (nz > 0)])
    inc = off & (nz > 0) & (dep != 0) & (cf[cols] >= 0)
    np.add.at(spc, rows[inc], nz[inc])
    f = cf == -1
    return int(np.sum(f & (sp > 0) & (spc == 0))), int(np.sum(f & (spc != 0)))


THETA = 0.25
GRAPH_CASES = [(name, THETA) for name in am.GRAPH_NAMES] + [("convdiff_pe50", THETA), ("posmix", THETA), ("path200", 0.0),
                                                             ("fd5x5x5", 0.0)]


def graphs(fd):
    """name -> CSC arrays: the graphs of amg_modellib, convection-diffusion at Pe 50 and posmix"""
    g = {name: csc for name, (csc, _) in am.graphs(fd).items()}
    g["convdiff_pe50"] = am.convdiff(6, 5, 4, 50.0)
    g["posmix"] = posmix(fd)
    return g
