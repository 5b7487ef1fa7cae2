"""CPU: esp_cg_many is declared by the header, exported by the built library and bound by _lib.py with the header's arity.
No device is touched."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declaration():
    text = open(os.path.join(ROOT, "include", "esparse_hip.h")).read()
    m = re.search(r"int32_t\s+esp_cg_many\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, "include/esparse_hip.h does not declare esp_cg_many"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_esp_cg_many():
    args = declaration()
    assert len(args) == 15
    assert args[0] == "esp_handle *h" and args[1] == "esp_precon *p"
    assert args[2] == "const double *B" and args[4] == "double *X" and args[6] == "int64_t k"
    assert args[-3:] == ["double *history", "int64_t *iterations", "int32_t *converged"]


def test_library_exports_esp_cg_many(esp):
    lib = C.CDLL(esp._lib.SO)
    assert hasattr(lib, "esp_cg_many")


def test_binding_matches_the_header(esp):
    res, args = esp._lib.SIGNATURES["esp_cg_many"]
    decl = declaration()
    assert res is C.c_int32 and len(args) == len(decl)
    want = {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}
    for a, d in zip(args, decl):
        if "*" in d:
            assert a is C.c_void_p, d
        else:
            assert a is want[d.split()[0]], d
    assert esp._lib.load().esp_cg_many.argtypes == args
