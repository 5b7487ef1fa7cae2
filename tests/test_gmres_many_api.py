"""CPU: esp_gmres_many is declared by the header, exported by the built library and bound by _lib.py with the header's arity.
No device is touched."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["esp_handle *h", "esp_precon *p", "const double *B", "int64_t ldb", "double *X", "int64_t ldx", "int64_t k", "int32_t on_device",
        "int32_t initially_zero", "int32_t restart", "int32_t orth_meth", "int64_t maxiter", "double abstol", "double reltol",
        "double *history", "int64_t *iterations", "int64_t *mv_products", "int64_t *reorth_passes", "int32_t *converged"]


def declaration():
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    m = re.search(r"int32_t\s+esp_gmres_many\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, "include/esparse_hip.h does not declare esp_gmres_many"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_esp_gmres_many():
    args = declaration()
    assert len(args) == 19
    assert args == ARGS


def test_library_exports_esp_gmres_many(esp):
    lib = C.CDLL(esp._lib.SO)
    assert hasattr(lib, "esp_gmres_many")


def test_binding_matches_the_header(esp):
    res, args = esp._lib.SIGNATURES["esp_gmres_many"]
    decl = declaration()
    assert res is C.c_int32 and len(args) == len(decl)
    want = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    for a, d in zip(args, decl):
        if "*" in d:
            assert a is C.c_void_p, d
        else:
            assert a is want[d.split()[0]], d
    assert esp._lib.load().esp_gmres_many.argtypes == args
