"""CPU: esp_precon_many_stats -- the observable of the many-column solves -- is declared by the header in its SEVERAL
RIGHT-HAND SIDES section, bound by _lib.py as (i32, [vp, P(i64)]) and exported by the built library; the Python classes that have
launches() have many_stats().  No device is touched."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "esparse_hip.h")).read()


def test_header_declares_esp_precon_many_stats():
    text = header()
    m = re.search(r"int32_t\s+esp_precon_many_stats\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, "include/esparse_hip.h does not declare esp_precon_many_stats"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ["esp_precon *p", "int64_t out[4]"]
    # in the section of the calls it describes: behind esp_precon_ldiv_many, in front of esp_cg_many
    section = text.index("SEVERAL RIGHT-HAND SIDES")
    assert section < text.index("int32_t esp_precon_ldiv_many") < m.start() < text.index("int32_t esp_cg_many")


def test_binding(esp):
    res, args = esp._lib.SIGNATURES["esp_precon_many_stats"]
    assert res is C.c_int32 and len(args) == 2
    assert args[0] is C.c_void_p and args[1] is C.POINTER(C.c_int64)
    assert (res, args) == esp._lib.SIGNATURES["esp_precon_launches"]       # the same shape as its neighbour
    assert esp._lib.load().esp_precon_many_stats.argtypes == args


def test_library_exports_esp_precon_many_stats(esp):
    lib = C.CDLL(esp._lib.SO)
    assert hasattr(lib, "esp_precon_many_stats")


def test_python_classes_with_launches_have_many_stats(esp):
    names = ["ILUAMPreconditioner", "BlockPreconditioner", "ILUKPreconditioner", "ILUTPreconditioner", "ColoredPreconditioner",
             "ParallelILU0Preconditioner", "LUFactorization"]
    for name in names:
        cls = getattr(esp, name)
        assert hasattr(cls, "launches") and callable(getattr(cls, "many_stats", None)), name
