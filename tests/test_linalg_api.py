"""CPU: the transpose / transpose(A)*x / issymmetric / opnorm / norm interface exists at every layer -- the header declares the six
calls, the Python binding and class carry them, the Julia shim defines the methods and ccalls the entry points (whose signatures
test_julia_shim.test_every_ccall_matches_the_header then checks)."""
import os
import re

from test_julia_shim import HDR, JL, ROOT, header_prototypes, shim_ccalls

CALLS = ("esp_transpose", "esp_debug_transpose_path", "esp_mul_transpose", "esp_issymmetric", "esp_opnorm", "esp_norm")


def test_header_declares_the_calls():
    protos = header_prototypes()
    for name in CALLS:
        assert name in protos, name
    assert protos["esp_transpose"][1] == ["ptr", "ptr", "ptr"]
    assert protos["esp_mul_transpose"][1] == ["ptr", "ptr", "ptr", "Int32"]
    assert protos["esp_opnorm"][1] == ["ptr", "Float64", "ptr"]
    assert protos["esp_norm"][1] == ["ptr", "Float64", "ptr"]


def test_python_binding_and_class():
    src = open(os.path.join(ROOT, "extendablesparse.jl_amd", "_lib.py")).read()
    for name in CALLS:
        assert '"%s"' % name in src, name
    msrc = open(os.path.join(ROOT, "extendablesparse.jl_amd", "matrix.py")).read()
    cls = msrc.split("class ExtendableSparseMatrix", 1)[1].split("\nclass ", 1)[0]
    for meth in ("transpose", "adjoint", "mul_transpose", "issymmetric", "ishermitian", "opnorm", "norm"):
        assert re.search(r"\n    def %s\(" % meth, cls), meth
    assert re.search(r"@property\n    def T\(", cls)


def test_julia_shim_methods_and_ccalls():
    src = re.sub(r"#.*", "", open(JL).read())
    called = {c[0] for c in shim_ccalls()}
    for name in ("esp_transpose", "esp_mul_transpose", "esp_issymmetric", "esp_opnorm", "esp_norm"):
        assert name in called, name
    for pat in (r"Base\.copy\(\w+::Transpose\{Float64,\s*<:HIPResidentSparseMatrixCSC",
                r"Base\.copy\(\w+::Adjoint\{Float64,\s*<:HIPResidentSparseMatrixCSC",
                r"Base\.permutedims\(\w+::HIPResidentSparseMatrixCSC",
                r"HIPResidentSparseMatrixCSC\(\w+::Union\{Transpose|HIPResidentSparseMatrixCSC\(\w+::Transpose",
                r"LinearAlgebra\.mul!\(\w+::\w+\{Float64\},\s*\w+::(Transpose|Union\{Transpose)",
                r"Base\.:\*\(\w+::(Transpose|Union\{Transpose|TransposeOrAdjointHIP)",
                r"LinearAlgebra\.issymmetric\(\w+::HIPResidentSparseMatrixCSC",
                r"LinearAlgebra\.ishermitian\(\w+::HIPResidentSparseMatrixCSC",
                r"LinearAlgebra\.norm\(\w+::HIPResidentSparseMatrixCSC",
                r"LinearAlgebra\.opnorm\(\w+::HIPResidentSparseMatrixCSC"):
        assert re.search(pat, src), pat
    assert "2-norm not yet implemented" in src and "ArgumentError" in src


def test_docs_list_the_calls():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("esp_transpose", "esp_mul_transpose", "esp_issymmetric", "esp_opnorm", "esp_norm"):
        assert name in doc, name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 5d." in design
    assert os.path.exists(HDR)
