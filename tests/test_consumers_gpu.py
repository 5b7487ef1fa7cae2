"""GPU: the readers and editors of the assembled CSC (csrc/consumers.hip and the entry points that share its caches) against the
CPU ORACLE at their edges, on the cases of tests/consumer_cases.py (tests/test_consumer_cases.py checks on the CPU that every case
sits on the edge it is named for).

  dropzeros!         drops in the middle of the arrays, across the scan's chunks of 2048 flags, emptied columns, everything
                     dropped, -0.0 / NaN / subnormal / -Inf, 1 x n and m x 1, a second call, the flush that follows
  getindex           every column type, first / last / neighbouring / absent rows, stored zeros, nnz = 0
  pending getindex   k = 1 .. 2048 matches of one position among 2 10^5 calls (many workgroups, every stride of the rank sort),
                     the refusal at 2049, a bucket-ordered batch followed by per-entry calls
  mul! / opnorm Inf  every pass count of the row sort (row bits 1, 8, 9, 16, 17, 25), Z around a sort tile, one row, one dense
                     column, empty edge rows, Inf / NaN in x over stored zeros, +0.0 from -0.0 products, n = 0 and m = 0
  editors x readers  the row-wise index primed, one editor, then every reader; the lazy colptr after reset! and behind a column
                     window, one reader per fresh handle
  Dirichlet, diagonal set-up   n = 1, 255, 256, 257 with missing / penalty / NaN / zero diagonals

Integer arrays are equal, values and vectors equal bit for bit; a NaN compares as "NaN at the same position" (the payload of a
NaN that an operation creates is the platform's)."""
import ctypes as C
import math

import numpy as np
import pytest

import consumer_cases as cc
import pair_streams as ps
from linalg_modellib import Model, norm_exact, norm_ref
from refmodel import bits

pytestmark = pytest.mark.gpu

ESP_ERR_INVALID, ESP_ERR_UNSUPPORTED, ESP_ERR_STATE = -1, -5, -6
INF = math.inf

DROPS = cc.drop_cases()
MULS = cc.mul_cases()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    return Model(tmp_path_factory.mktemp("consumers_linalg_model"))


# ------------------------------------------------------------------------------------------------------------ helpers
def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def same_vec(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what + " shape %s != %s" % (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), what + " NaN at other positions (first at %s)" % np.flatnonzero(gn != wn)[:5]
    bad = np.flatnonzero(bits(got)[~gn] != bits(want)[~wn])
    assert len(bad) == 0, what + " %d values differ, first at %d: %r != %r" % (len(bad), bad[0], got[~gn][bad[0]], want[~wn][bad[0]])


def same_scalar(got, want, what=""):
    same_vec(np.array([got]), np.array([want]), what)


def same_csc(got, want, what=""):
    (cp1, rv1, nz1), (cp2, rv2, nz2) = got, want
    assert np.array_equal(cp1, cp2), what + " colptr differs (first at column %s)" % (np.flatnonzero(np.asarray(cp1) != np.asarray(cp2))[:3] + 1)
    assert np.array_equal(rv1, rv2), what + " rowval differs"
    same_vec(nz1, nz2, what + " nzval:")


def host_csc(esp, case):
    return esp.SparseMatrixCSC(case.m, case.n, case.colptr.copy(), case.rowval.copy(), case.nzval.copy())


def install(esp, case):
    A = esp.ExtendableSparseMatrix(case.m, case.n)
    A.cscmatrix = host_csc(esp, case)
    return A


def orc_csc(orc, case_or_arrays, m=None, n=None):
    if isinstance(case_or_arrays, cc.Case):
        c = case_or_arrays
        return orc.CSC(c.m, c.n, c.colptr, c.rowval, c.nzval)
    cp, rv, nz = case_or_arrays
    return orc.CSC(m, n, cp, rv, nz)


def device_arrays(d):
    """(colptr, rowval, nzval) of handle d as esp_get_csc hands them out"""
    return d.get_csc().arrays()


def resident(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# raw readers on a _Handle (an ExtendableSparseMatrix' or a SparseMatrixHIPCOO's)
def raw_mul(d, x):
    r = np.full(max(d.m, 1), -7.0)[:d.m]
    d.ck(d.lib.esp_mul(d.h, _vp(np.ascontiguousarray(x, np.float64)), _vp(r), 0))
    return r


def raw_opnorm_inf(d):
    res = C.c_double()
    d.ck(d.lib.esp_opnorm(d.h, INF, C.byref(res)))
    return res.value


def raw_jacobi(d):
    out = np.full(d.n, -7.0)
    d.ck(d.lib.esp_jacobi_setup(d.h, _vp(out), 0))
    return out


def raw_mark(d, penalty=cc.PENALTY):
    out = np.full(d.n, 9, np.uint8)
    d.ck(d.lib.esp_mark_dirichlet(d.h, float(penalty), _vp(out), 0))
    return out.astype(bool)


def raw_getindex(d, i, j):
    val, found = C.c_double(-7.0), C.c_int32(-7)
    d.ck(d.lib.esp_getindex(d.h, i, j, C.byref(val), C.byref(found)))
    return val.value, found.value


def raw_pending_getindex(d, i, j):
    d.commit()
    val, found = C.c_double(-7.0), C.c_int32(-7)
    rc = d.lib.esp_pending_getindex(d.h, i, j, C.byref(val), C.byref(found))
    return rc, val.value, found.value


def raw_phash(d):
    hsh = C.c_uint64()
    d.ck(d.lib.esp_pattern_hash(d.h, C.byref(hsh)))
    return hsh.value


def opnorm_inf_want(model, m, n, arrays):
    """opnorm(A, Inf) of SparseArrays: the general branch's loop, sum |v| for one row, max |v| for one column, 0 for no extent"""
    nz = arrays[2]
    if m == 0 or n == 0:
        return 0.0, True
    if m == 1:
        return norm_ref(nz, 1), False          # (BLAS in the reference: within 1e-13, tests/test_linalg_gpu.py)
    if n == 1:
        return norm_exact(nz, INF), True
    if len(nz) == 0:
        return 0.0, True
    return model.opnorm_general(m, arrays, INF), True


def check_opnorm_inf(model, got, m, n, arrays, what=""):
    want, exact = opnorm_inf_want(model, m, n, arrays)
    if exact:
        same_scalar(got, want, what + " opnorm(Inf):")
    else:
        assert abs(got - want) <= 1e-13 * abs(want), (what, got, want)


def lookups_of(m, n, arrays, count, seed):
    """some stored and some arbitrary positions"""
    cp, rv, _ = arrays
    rng = np.random.default_rng([seed, m, n])
    out = [(int(rng.integers(1, m + 1)), int(rng.integers(1, n + 1))) for _ in range(count)]
    if len(rv):
        cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
        for k in rng.integers(0, len(rv), count).tolist() + [0, len(rv) - 1]:
            out.append((int(rv[k]), int(cols[k])))
    return out


def check_readers(esp, orc, model, d, want, what):
    """every reader on handle d against the oracle on the arrays `want`"""
    m, n = d.m, d.n
    O = orc_csc(orc, want, m, n)
    x = np.random.default_rng([77, n]).standard_normal(n)
    same_vec(raw_mul(d, x), O.mul(x), what + " mul:")
    check_opnorm_inf(model, raw_opnorm_inf(d), m, n, want, what)
    same_csc(device_arrays(d), want, what + " arrays:")
    same_vec(raw_jacobi(d), O.jacobi(), what + " jacobi:")
    assert np.array_equal(raw_mark(d), O.mark_dirichlet()), what + " mark_dirichlet"
    for (i, j) in lookups_of(m, n, want, 12, 5):
        k = O.findindex(i, j)
        val, found = raw_getindex(d, i, j)
        assert found == (1 if k > 0 else 0), (what, i, j, found, k)
        same_scalar(val, want[2][k - 1] if k > 0 else 0.0, what + " A[%d,%d]:" % (i, j))
    assert raw_phash(d) == O.pattern_hash(), what + " pattern hash"
    xt = resident(x)
    import torch
    rt = torch.full((m,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    d.ck(d.lib.esp_mul(d.h, C.c_void_p(xt.data_ptr()), C.c_void_p(rt.data_ptr()), 1))
    same_vec(rt.cpu().numpy(), O.mul(x), what + " mul (device vectors):")


# ------------------------------------------------------------------------------------------------------------ dropzeros!
@pytest.mark.parametrize("name", sorted(DROPS))
def test_dropzeros(esp, orc, name):
    """colptr, rowval, the raw bits of nzval and new_nnz against CSC.dropzeros(); a second dropzeros! changes nothing; nothing
    dropped: phash and the primed mul! stay; then the next flush joins removed, kept and new positions onto the compacted pattern"""
    case, p = DROPS[name]
    A = install(esp, case)
    d = A._d
    x = cc.mul_x(case)
    ph0 = A._pattern_hash()
    r0 = A.mul(x)                                            # (primes the row-wise index)
    same_vec(r0, orc_csc(orc, case).mul(x), name + " mul before:")
    O = orc_csc(orc, case)
    O.dropzeros()
    want = O.arrays()
    A.dropzeros()
    print(name, "Z", p["Z"], "kept", p["kept"], "chunks", p["chunks"], "emptied", len(p["emptied"]))
    assert d.nnz() == p["kept"] == O.nnz()
    got = device_arrays(d)
    same_csc(got, want, name + ":")
    assert np.array_equal(bits(got[2]), bits(want[2])), name + ": dropzeros! moves values, their bits stay (NaN payloads too)"
    same_vec(A.mul(x), O.mul(x), name + " mul after:")
    if len(p["drop"]) == 0:
        assert A._pattern_hash() == ph0 and np.array_equal(bits(A.mul(x)), bits(r0))
    assert A._pattern_hash() == O.pattern_hash()
    z = C.c_int64(-1)
    d.ck(d.lib.esp_dropzeros(d.h, C.byref(z)))               # a second dropzeros! right after the first
    assert z.value == p["kept"]
    same_csc(device_arrays(d), want, name + " second dropzeros!:")
    kinds, I, J, V = cc.join_stream(case)
    A.append(esp.ESP_UPDATE, I, J, V, kinds=kinds)
    A.flush()
    OE = orc.ExtendableSparseMatrix(O)
    OE.apply(kinds, I, J, V)
    OE.flush()
    same_csc(device_arrays(d), OE.arrays(), name + " flush after dropzeros!:")
    same_vec(A.mul(x), OE.sparse().mul(x), name + " mul after the flush:")


def test_dropzeros_on_both_sides_of_reset(esp, orc):
    """a batch the pair bucket kernel serves (tests/pair_streams.py: ragged, as RAWUPDATE -- its zeros are stored), on ONE handle:
    flush, dropzeros!, the same batch again (joined onto the compacted pattern), reset!, and all of it once more -- the plan and the
    offsets kept from the first flush must not be applied to a pattern they were not made for.  Every state against the oracle."""
    s, _ = ps.ragged(1)
    kinds = np.full(len(s.I), cc.RAWUPDATE, np.uint8)
    A = esp.ExtendableSparseMatrix(s.m, s.n)
    O = orc.ExtendableSparseMatrix(s.m, s.n)
    import torch
    dev = tuple(torch.from_numpy(a).cuda() for a in (s.I, s.J, s.V))
    seen = []
    for side in ("before reset!", "after reset!"):
        for step in ("fresh", "joined"):
            A.append_device(esp.ESP_RAWUPDATE, *dev)
            A.flush()
            O.apply(kinds, s.I, s.J, s.V)
            O.flush()
            seen.append((A.debug_last_bucket_pairs(), A.debug_last_plan_reused(), A.debug_last_predicted()))
            print(side, step, "pairs / plan reused / predicted", seen[-1], "nnz", A.nnz())
            same_csc(device_arrays(A._d), O.arrays(), "%s %s flush:" % (side, step))
            if step == "fresh":
                z0 = A.nnz()
                A.dropzeros()
                O.dropzeros()
                assert 0 < A._d.nnz() < z0
                same_csc(device_arrays(A._d), O.arrays(), "%s dropzeros!:" % side)
        A.reset()
        O.reset()
    assert seen[0][0] == 1, "the first flush is what the pair kernel takes"


# -------------------------------------------------------------------------------------------------------------- getindex
def test_getindex_every_column_type(esp, orc):
    case, p = cc.getindex_case()
    A = install(esp, case)
    O = orc_csc(orc, case)
    for (i, j) in cc.getindex_lookups(case):
        k = O.findindex(i, j)
        val, found = raw_getindex(A._d, i, j)
        assert found == (1 if k > 0 else 0), (i, j, found, k)
        assert bits(np.array([val]))[0] == (bits(case.nzval)[k - 1] if k > 0 else 0), (i, j, val)
        same_scalar(A[i, j], val)
    for at, want in ((p["zero_at"], 0.0), (p["negzero_at"], -0.0), (p["dense_zero_at"], 0.0)):
        val, found = raw_getindex(A._d, *at)                  # a stored zero is found, -0.0 keeps its sign
        assert found == 1 and bits(np.array([val]))[0] == bits(np.array([want]))[0]
    with pytest.raises(IndexError):
        A[case.m + 1, 1]
    with pytest.raises(IndexError):
        A[1, 0]


def test_getindex_empty_matrix(esp):
    for m, n in ((1, 1), (200, 15), (7, 5000)):
        A = esp.ExtendableSparseMatrix(m, n)
        for (i, j) in ((1, 1), (m, n), (1, n), (m, 1)):
            assert raw_getindex(A._d, i, j) == (0.0, 0)
    A = install(esp, cc.getindex_case()[0])
    A.reset()
    assert raw_getindex(A._d, 57, 4) == (0.0, 0) and raw_getindex(A._d, 200, 11) == (0.0, 0)


# ------------------------------------------------------------------------------------------------ getindex of the pending buffer
def _pending_pair(esp, orc, k):
    (kinds, I, J, V), p = cc.pending_stream(k)
    A = esp.ExtendableSparseMatrix(cc.PENDING_M, cc.PENDING_N)
    A.append(esp.ESP_UPDATE, I, J, V, kinds=kinds)            # ONE batch: many workgroups of pending_matches_k
    O = orc.ExtendableSparseMatrix(cc.PENDING_M, cc.PENDING_N)
    O.apply(kinds, I, J, V)
    return A, O, p, len(I)


OTHERS = ((1, 1), (50, 60), (24, 41), (23, 40), (7, 33))


@pytest.mark.parametrize("k", cc.PENDING_K)
def test_pending_getindex_matches(esp, orc, k):
    """k calls of the target among 2 10^5 others: the oracle's O[i, j] on the same pending calls, then the same value in the CSC"""
    A, O, p, E = _pending_pair(esp, orc, k)
    i, j = p["target"]
    rc, val, found = raw_pending_getindex(A._d, i, j)
    want = O[i, j]
    print("k", k, "value", val, "oracle", want, "workgroups", p["groups"])
    assert rc == 0 and found == 1
    same_scalar(val, want, "k = %d:" % k)
    assert A.nnznew() == E and O.pending() > 0                # (the buffer counts calls, the oracle's list positions)
    for (a, b) in OTHERS:
        rc, v, f = raw_pending_getindex(A._d, a, b)
        assert rc == 0 and f == 1
        same_scalar(v, O[a, b], "(%d,%d):" % (a, b))
    A.flush()
    O.flush()
    same_csc(device_arrays(A._d), O.arrays(), "k = %d flush:" % k)
    v, f = raw_getindex(A._d, i, j)
    assert f == 1
    same_scalar(v, want, "k = %d after the flush:" % k)
    assert raw_pending_getindex(A._d, i, j) == (0, 0.0, 0)    # (nothing pending any more)


def test_pending_getindex_refuses_more_than_the_cap(esp, orc):
    """2049 calls of one position: ESP_ERR_UNSUPPORTED with the documented message, the handle as it was"""
    A, O, p, E = _pending_pair(esp, orc, cc.PENDING_MATCH_CAP + 1)
    i, j = p["target"]
    rc, _, _ = raw_pending_getindex(A._d, i, j)
    assert rc == ESP_ERR_UNSUPPORTED
    msg = A._d.lib.esp_last_error(A._d.h).decode()
    assert msg == "esp_pending_getindex: more than %d pending updates of (%d,%d); flush first" % (cc.PENDING_MATCH_CAP, i, j), msg
    B = esp.SparseMatrixHIPCOO(cc.PENDING_M, cc.PENDING_N)    # (the same refusal through the buffer's own getindex)
    (kinds, I, J, V), _ = cc.pending_stream(cc.PENDING_MATCH_CAP + 1)
    B.append(esp.ESP_UPDATE, I, J, V, kinds=kinds)
    with pytest.raises(esp._lib.EspError, match="more than 2048 pending updates") as e:
        B[i, j]
    assert e.value.code == ESP_ERR_UNSUPPORTED and B.nnz() == E
    assert A.nnznew() == E                                    # pending() unchanged
    for (a, b) in OTHERS:                                     # a lookup of another position still answers
        rc, v, f = raw_pending_getindex(A._d, a, b)
        assert rc == 0 and f == 1
        same_scalar(v, O[a, b])
        same_scalar(B[a, b], O[a, b])
    A.flush()
    O.flush()
    same_csc(device_arrays(A._d), O.arrays(), "flush after the refusal:")


def test_pending_getindex_no_match(esp, orc):
    A, O, p, E = _pending_pair(esp, orc, 0)
    i, j = p["target"]
    assert raw_pending_getindex(A._d, i, j) == (0, 0.0, 0) and O[i, j] == 0.0
    E0 = esp.ExtendableSparseMatrix(cc.PENDING_M, cc.PENDING_N)
    assert raw_pending_getindex(E0._d, i, j) == (0, 0.0, 0)   # nothing pending at all
    E0.updateindex("+", 0.0, i, j)                            # an UPDATE of 0.0 creates nothing
    E0[i, j] = -0.0                                           # nor does a SET of -0.0
    assert raw_pending_getindex(E0._d, i, j) == (0, 0.0, 0)
    E0.rawupdateindex("+", -0.0, i, j)                        # a RAWUPDATE does: 0.0 + -0.0
    rc, v, f = raw_pending_getindex(E0._d, i, j)
    assert (rc, f) == (0, 1) and bits(np.array([v]))[0] == 0
    with pytest.raises(IndexError):
        esp.SparseMatrixHIPCOO(cc.PENDING_M, cc.PENDING_N)[cc.PENDING_M + 1, 1]


def test_pending_getindex_bucket_ordered_batch(esp, orc):
    """a batch the device generator leaves bucket-ordered (fdrand 20^3), followed by per-entry calls on the same handle"""
    g = 20
    N = g ** 3
    A = esp.ExtendableSparseMatrix(N, N)
    A.generate_fdrand(g, g, g)
    O = orc.ExtendableSparseMatrix(N, N)
    I, J, V = orc.fdrand_stream(g, g, g)
    O.apply(np.full(len(I), cc.UPDATE, np.uint8), I, J, V)
    mid = g * g * 7 + g * 9 + 11
    calls = [("update", 2.5, mid, mid), ("set", -1.25, mid, mid + 1), ("update", 2.0 ** -60, mid, mid + 1), ("raw", 0.0, 5, 4000),
             ("update", 1e300, 1, 1), ("update", -1e300, 1, 1), ("set", 0.0, N, N), ("update", 3.0, N, N), ("update", 0.0, 9, 4001)]
    for what, v, i, j in calls:
        if what == "set":
            A[i, j] = v
            O[i, j] = v
        elif what == "update":
            A.updateindex("+", v, i, j)
            O.updateindex(0, v, i, j)
        else:
            A.rawupdateindex("+", v, i, j)
            O.rawupdateindex(0, v, i, j)
    look = [(i, j) for _, _, i, j in calls] + [(mid + 1, mid), (mid - g, mid), (2, 1), (N - 1, N), (17, 3000), (mid, mid + 2)]
    for (i, j) in look:
        rc, v, f = raw_pending_getindex(A._d, i, j)
        want = O[i, j]
        assert rc == 0, (i, j, rc)
        same_scalar(v, want, "(%d,%d):" % (i, j))
        if want != 0.0:
            assert f == 1
    assert raw_pending_getindex(A._d, 17, 3000)[2] == 0 and raw_pending_getindex(A._d, 9, 4001)[2] == 0
    assert raw_pending_getindex(A._d, 5, 4000)[2] == 1       # (RAWUPDATE 0.0: a stored zero to be)
    assert A.nnznew() == len(I) + len(calls) and O.pending() > 0
    A.flush()
    O.flush()
    same_csc(device_arrays(A._d), O.arrays(), "fdrand + per-entry calls:")


# ----------------------------------------------------------------------------------------- mul! and the row-wise index
def _check_mul(esp, orc, model, case, x, what):
    A = install(esp, case)
    O = orc_csc(orc, case)
    want = O.mul(x)
    same_vec(A.mul(x), want, what + " mul (NumPy):")
    import torch
    xt = resident(x)
    print(what, "m", case.m, "n", case.n, "nnz", len(case.nzval), "x.data_ptr", xt.data_ptr())
    rt = A.mul(xt)
    assert rt.is_cuda and rt.numel() == case.m
    same_vec(rt.cpu().numpy(), want, what + " mul (device tensors):")
    out = torch.full((case.m,), -7.0, dtype=torch.float64, device="cuda")
    assert A.mul(xt, out=out) is out
    same_vec(out.cpu().numpy(), want, what + " mul (device tensors, out=):")
    same_vec(A @ x, want, what + " A @ x:")
    check_opnorm_inf(model, A.opnorm(INF), case.m, case.n, (case.colptr, case.rowval, case.nzval), what)
    return A, want


@pytest.mark.parametrize("name", list(MULS))
def test_mul_row_index(esp, orc, model, name):
    case, p = MULS[name]
    _check_mul(esp, orc, model, case, cc.mul_x(case), name)


def test_mul_nonfinite_x_over_stored_zeros(esp, orc, model):
    (case, x), p = cc.mul_nonfinite()
    A, want = _check_mul(esp, orc, model, case, x, "mul_nonfinite")
    assert np.isnan(want[p["zero_rows"] - 1]).all()
    assert np.isnan(A.mul(x)[p["zero_rows"] - 1]).all(), "0 * Inf must give NaN: stored zeros take part in the product"


def test_mul_negative_zero_products(esp, orc, model):
    (case, x), p = cc.mul_negzero()
    A, want = _check_mul(esp, orc, model, case, x, "mul_negzero")
    assert (bits(A.mul(x)[p["rows"] - 1]) == 0).all(), "r .= 0 first: a sum of -0.0 products is +0.0"


def test_mul_refuses_wrong_sizes_and_pending(esp):
    case, _ = MULS["mul_Z4097"]
    A = install(esp, case)
    with pytest.raises(ValueError):
        A.mul(np.zeros(case.n + 1))
    A._d.push(esp.ESP_UPDATE, 1.0, 1, 1)
    A._d.commit()
    r = np.empty(case.m)
    assert A._d.lib.esp_mul(A._d.h, _vp(np.zeros(case.n)), _vp(r), 0) == ESP_ERR_STATE


# ------------------------------------------------------------------------------------------- every editor x every reader
def _empty_arrays(n):
    return np.ones(n + 1, np.int64), np.empty(0, np.int64), np.empty(0, np.float64)


def _apply_editor(esp, orc, editor, A, base, O):
    """one editor on the device matrix and on the oracle: the arrays the oracle holds afterwards"""
    d = A._d
    n = base.n
    rng = np.random.default_rng([91, cc.EDITORS.index(editor)])
    if editor in ("flush_hits", "flush_adds"):
        kinds, I, J, V = cc.editor_hits(base) if editor == "flush_hits" else cc.editor_adds(base)
        z0 = A.nnz()
        A.append(int(kinds[0]), I, J, V)
        A.flush()
        assert (A.nnz() == z0) == (editor == "flush_hits")
        O.apply(kinds, I, J, V)
        O.flush()
        return O.arrays()
    if editor == "set_nzval":
        host = A.cscmatrix                                    # (the host copy, handed out: its nzval may be edited in place)
        new = rng.standard_normal(len(base.nzval))
        host.nzval[:] = new
        A.flush()                                             # esp_set_nzval in front of the next consumer
        return base.colptr, base.rowval, new
    if editor == "zero_values":
        A.zero_values()
        O.zero_values()
        return O.arrays()
    if editor == "eliminate_dirichlet":
        marker = orc_csc(orc, base).mark_dirichlet()
        assert marker.sum() > 100
        A.eliminate_dirichlet(marker)
        return orc_csc(orc, base).eliminate_dirichlet(marker).arrays()
    if editor in ("dropzeros_drops", "dropzeros_nothing"):
        z0 = A.nnz()
        A.dropzeros()
        O.dropzeros()
        assert (d.nnz() < z0) == (editor == "dropzeros_drops")
        return O.arrays()
    if editor == "diag_scale_inplace":
        dv = rng.standard_normal(n)
        assert A.diag_scale(dv, side="left", inplace=True) is A
        return base.colptr, base.rowval, dv[base.rowval - 1] * base.nzval
    other, _ = cc.editor_other()
    if editor == "set_csc":
        A.cscmatrix = host_csc(esp, other)
        return other.colptr, other.rowval, other.nzval
    if editor == "set_csc_i32":
        cp, rv = other.colptr.astype(np.int32), other.rowval.astype(np.int32)
        d.ck(d.lib.esp_set_csc_i32(d.h, _vp(cp), _vp(rv), _vp(other.nzval), len(other.nzval)))
        return other.colptr, other.rowval, other.nzval
    if editor == "reset":
        A.reset()
        return _empty_arrays(n)
    if editor == "release":
        d._st, d._nst = None, 0
        d.ck(d.lib.esp_release_buffers(d.h))
        return _empty_arrays(n)
    raise KeyError(editor)


@pytest.mark.parametrize("editor", cc.EDITORS)
def test_every_editor_then_every_reader(esp, orc, model, editor):
    """the row-wise index primed by mul! on a matrix with n = 5000 (above the lazy-colptr threshold) and a Jacobi preconditioner
    made, then ONE editor, then every reader against the oracle on the edited arrays: no reader may meet a cache the editor left
    behind.  The preconditioner refuses ldiv! after an editor that changes the pattern, and answers with its old diagonal after one
    that changes values only."""
    base, _ = cc.editor_base(zeros=editor != "dropzeros_nothing")
    n = base.n
    x = np.random.default_rng([77, n]).standard_normal(n)
    lib = None
    p = C.c_void_p()
    keep = []
    try:
        if editor == "sum_home":
            # the home handle of Base.sum(buffers, csc): a first sum installs the matrix, the second is the editor
            home = esp.SparseMatrixHIPCOO(n, n)
            b1, b2 = esp.SparseMatrixHIPCOO(n, n), esp.SparseMatrixHIPCOO(n, n)
            keep += [home, b1, b2]
            i0, j0 = int(base.rowval[100]), int(cc.coo_of(base)[1][100])
            b1.rawupdateindex("+", 0.5, i0, j0)
            csc1 = esp.SparseMatrixHIPCOO.sum([b1, b2], host_csc(esp, base), home=home)
            L = orc.SparseMatrixLNK(n, n)
            L.rawupdateindex(0, 0.5, i0, j0)
            C1 = L + orc_csc(orc, base)
            same_csc(csc1.arrays(), C1.arrays(), "sum_home first sum:")
            d = home._d
            start = C1.arrays()
        else:
            A = install(esp, base)
            keep.append(A)
            A.flush()        # (the installed host copy counts as handed out: its values go up once more NOW, not behind the editor)
            d = A._d
            O = orc.ExtendableSparseMatrix(orc_csc(orc, base))
            start = (base.colptr, base.rowval, base.nzval)
        lib = d.lib
        O0 = orc_csc(orc, start, n, n)
        same_vec(raw_mul(d, x), O0.mul(x), editor + " mul before:")      # primes csr_version / csr_val_version
        d.ck(lib.esp_precon_create(d.h, esp._lib.ESP_PRECON_JACOBI, C.byref(p)))
        old_inv = O0.jacobi()
        v = np.random.default_rng([78, n]).standard_normal(n)
        u = np.empty(n)
        assert lib.esp_precon_ldiv(p, _vp(v), _vp(u), 0) == 0
        same_vec(u, old_inv * v, editor + " ldiv! before:")
        if editor == "sum_home":
            kinds, I, J, V = cc.editor_adds(base)
            half = len(I) // 2
            b1.append(esp.ESP_RAWUPDATE, I[:half], J[:half], V[:half])
            b2.append(esp.ESP_RAWUPDATE, I[half:], J[half:], V[half:])
            csc2 = esp.SparseMatrixHIPCOO.sum([b1, b2], csc1, home=home)
            L1, L2 = orc.SparseMatrixLNK(n, n), orc.SparseMatrixLNK(n, n)
            for Lk, sl in ((L1, slice(0, half)), (L2, slice(half, None))):
                for i, j, val in zip(I[sl].tolist(), J[sl].tolist(), V[sl].tolist()):
                    Lk.rawupdateindex(0, val, i, j)
            want = (L2 + (L1 + C1)).arrays()
            same_csc(csc2.arrays(), want, "sum_home second sum:")
            assert b1.nnz() == 0 and b2.nnz() == 0
        else:
            want = _apply_editor(esp, orc, editor, A, base, O)
        want = tuple(np.array(a, copy=True) for a in want)
        print(editor, "nnz", len(start[1]), "->", len(want[1]))
        check_readers(esp, orc, model, d, want, editor)
        rc = lib.esp_precon_ldiv(p, _vp(v), _vp(u), 0)
        if cc.EDITOR_EFFECT[editor] == "pattern":
            assert rc == ESP_ERR_STATE, (editor, rc)
            assert "pattern changed" in lib.esp_last_error(d.h).decode()
            assert lib.esp_precon_update(p) == 0                      # update! rebuilds: the new diagonal
            assert lib.esp_precon_ldiv(p, _vp(v), _vp(u), 0) == 0
            same_vec(u, orc_csc(orc, want, n, n).jacobi() * v, editor + " ldiv! after update!:")
        else:
            assert rc == 0, (editor, rc, lib.esp_last_error(d.h).decode())
            same_vec(u, old_inv * v, editor + " ldiv! with the old diagonal:")
        check_readers(esp, orc, model, d, want, editor + " (second round)")
    finally:
        if p and lib is not None:
            lib.esp_precon_destroy(p)


STATES = ("reset_%d" % cc.LAZY_COLPTR_N, "reset_%d" % (cc.LAZY_COLPTR_N + 1), "window")


def _lazy_state(esp, orc, state):
    """(A, arrays the oracle holds): a matrix whose colptr the last state change left to the next reader"""
    if state.startswith("reset_"):
        n = int(state.split("_")[1])
        case, _ = cc.diagonal_case(n)
        A = install(esp, case)
        assert A.nnz() == n
        A.reset()
        return A, _empty_arrays(n)
    n = cc.EDITOR_N
    kinds, I, J, V = cc.window_stream()
    A = esp.ExtendableSparseMatrix(n, n)
    A.set_column_window(*cc.WINDOW)
    A.append(esp.ESP_RAWUPDATE, I, J, V)
    A.flush()
    O = orc.ExtendableSparseMatrix(n, n)
    O.apply(kinds, I, J, V)
    O.flush()
    return A, O.arrays()


def _issymmetric(m, n, arrays):
    """issymmetric(Matrix(A)): stored zeros count as absent"""
    if m != n:
        return False
    cp, rv, nz = arrays
    cols = np.repeat(np.arange(1, n + 1), np.diff(cp))
    val = {(int(i), int(j)): v for i, j, v in zip(rv, cols, nz)}
    return all(val.get((j, i), 0.0) == v for (i, j), v in val.items())


# the algebra's readers take no matrix with a column window (check_operand: ESP_ERR_UNSUPPORTED, documented): behind a window they
# refuse, and read once the window is the whole matrix again (esp_set_column_window refreshes the tail it leaves)
REFUSE_WINDOW = ("opnorm_inf", "transpose", "norm", "issymmetric")


def _read(esp, orc, model, A, want, reader, what):
    m = n = A.n
    O = orc_csc(orc, want, m, n)
    if reader == "mul":
        x = np.random.default_rng([79, n]).standard_normal(n)
        same_vec(A.mul(x), O.mul(x), what)
    elif reader == "opnorm_inf":
        check_opnorm_inf(model, A.opnorm(INF), m, n, want, what)
    elif reader == "jacobi":
        same_vec(A.jacobi(), O.jacobi(), what)
    elif reader == "mark_dirichlet":
        assert np.array_equal(A.mark_dirichlet(), O.mark_dirichlet()), what
    elif reader == "getindex":
        for (i, j) in lookups_of(m, n, want, 3, 6):
            k = O.findindex(i, j)
            same_scalar(A[i, j], want[2][k - 1] if k > 0 else 0.0, what)
    elif reader == "pattern_hash":
        assert A._pattern_hash() == O.pattern_hash(), what
    elif reader == "copy":
        B = A.copy()
        same_csc(device_arrays(B._d), want, what)
    elif reader == "transpose":
        T = A.transpose()
        same_csc(device_arrays(T._d), model.transpose(m, want), what)
    elif reader == "norm":
        same_scalar(A.norm(INF), norm_exact(want[2], INF), what)
    elif reader == "issymmetric":
        assert A.issymmetric() == _issymmetric(m, n, want), what
    elif reader == "arrays":
        same_csc(A.arrays(), want, what)
    else:
        raise KeyError(reader)


@pytest.mark.parametrize("reader", cc.READERS)
@pytest.mark.parametrize("state", STATES)
def test_first_reader_sees_the_whole_colptr(esp, orc, model, state, reader):
    """right after reset! (n = 4096: colptr written at once, n = 4097: left to the next reader) and right after a flush inside a
    column window that ends before n, each reader as the FIRST call on a fresh handle"""
    A, want = _lazy_state(esp, orc, state)
    what = "%s, first reader %s:" % (state, reader)
    if state == "window" and reader in REFUSE_WINDOW:
        with pytest.raises((esp.EspError, ValueError)) as e:
            _read(esp, orc, model, A, want, reader, what)
        assert getattr(e.value, "code", ESP_ERR_UNSUPPORTED) == ESP_ERR_UNSUPPORTED
        assert "a column window / column shard as an operand" in A._d.lib.esp_last_error(A._d.h).decode()
        A.set_column_window(1, A.n)
    _read(esp, orc, model, A, want, reader, what)
    if state == "window":
        A.set_column_window(1, A.n)
    check_readers(esp, orc, model, A._d, want, what + " then every reader")


# -------------------------------------------------------------------------------------- Dirichlet helpers, diagonal set-up
@pytest.mark.parametrize("n", cc.DIRICHLET_N)
def test_dirichlet_and_diagonal_setup(esp, orc, n):
    """mark_dirichlet (>= penalty, NaN not marked, a large off-diagonal entry marks nothing), eliminate_dirichlet! (rows and columns,
    stored zeros stay structural), with the marker in host and in device memory; jacobi: Inf for a missing and a 0.0 diagonal, -Inf
    for -0.0, NaN for NaN; ilu0 names the smallest column without a diagonal"""
    import torch
    case, p = cc.dirichlet_case(n)
    A = install(esp, case)
    d = A._d
    O = orc_csc(orc, case)
    marker = O.mark_dirichlet()
    assert np.array_equal(A.mark_dirichlet(), marker)
    for pen in (cc.PENALTY, 2.5e20, 2.6e20, 0.0, -INF, INF):
        assert np.array_equal(A.mark_dirichlet(penalty=pen), O.mark_dirichlet(penalty=pen)), pen
    mt = torch.full((n,), 9, dtype=torch.uint8, device="cuda")            # the marker in device memory
    torch.cuda.synchronize()
    d.ck(d.lib.esp_mark_dirichlet(d.h, cc.PENALTY, C.c_void_p(mt.data_ptr()), 1))
    assert np.array_equal(mt.cpu().numpy().astype(bool), marker)
    same_vec(A.jacobi(), O.jacobi(), "jacobi n = %d:" % n)
    jt = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    d.ck(d.lib.esp_jacobi_setup(d.h, C.c_void_p(jt.data_ptr()), 1))
    same_vec(jt.cpu().numpy(), O.jacobi(), "jacobi (device vector) n = %d:" % n)
    if len(p["missing"]):
        with pytest.raises(esp._lib.EspError, match="column %d has no stored diagonal" % p["missing"][0]) as e:
            A.ilu0()
        assert e.value.code == ESP_ERR_INVALID
        with pytest.raises(ValueError, match="column %d " % p["missing"][0]):
            O.ilu0()
    # eliminate: host marker on one handle, device marker on another
    B = install(esp, case)
    want = orc_csc(orc, case).eliminate_dirichlet(marker).arrays()
    A.eliminate_dirichlet(marker)
    same_csc(device_arrays(d), want, "eliminate_dirichlet! n = %d:" % n)
    mk = resident(marker.astype(np.uint8))
    torch.cuda.synchronize()
    B._d.ck(B._d.lib.esp_eliminate_dirichlet(B._d.h, C.c_void_p(mk.data_ptr()), 1))
    same_csc(device_arrays(B._d), want, "eliminate_dirichlet! (device marker) n = %d:" % n)
    assert np.array_equal(want[0], case.colptr) and np.array_equal(want[1], case.rowval), "stored zeros stay structural"
    assert d.nnz() == len(case.nzval)
    same_vec(A.jacobi(), orc_csc(orc, want, n, n).jacobi(), "jacobi after the elimination:")
    # every node marked / none marked
    for mk_all in (np.ones(n, bool), np.zeros(n, bool)):
        Cm = install(esp, case)
        Cm.eliminate_dirichlet(mk_all)
        same_csc(device_arrays(Cm._d), orc_csc(orc, case).eliminate_dirichlet(mk_all).arrays(), "eliminate all / none:")
    # a full diagonal: ilu0 against the oracle
    full, _ = cc.dirichlet_case(n, full_diagonal=True)
    F = install(esp, full)
    xd, idg = F.ilu0()
    wxd, widg = orc_csc(orc, full).ilu0()
    same_vec(xd, wxd, "ilu0 xdiag n = %d:" % n)
    assert np.array_equal(idg, widg)
    same_vec(F.jacobi(), orc_csc(orc, full).jacobi(), "jacobi (full diagonal):")


def test_dirichlet_and_diagonal_setup_refusals_and_no_extent(esp):
    R = esp.ExtendableSparseMatrix(3, 4)
    for call in (R.mark_dirichlet, R.jacobi, R.ilu0, lambda: R.eliminate_dirichlet(np.zeros(4, bool))):
        with pytest.raises(esp._lib.EspError, match="must be square") as e:
            call()
        assert e.value.code == ESP_ERR_INVALID
    Z = esp.ExtendableSparseMatrix(0, 0)
    assert Z.mark_dirichlet().shape == (0,) and Z.jacobi().shape == (0,)
    xd, idg = Z.ilu0()
    assert xd.shape == (0,) and idg.shape == (0,)
    Z.eliminate_dirichlet(np.zeros(0, bool))
    assert Z.nnz() == 0
    E = esp.ExtendableSparseMatrix(5, 5)                      # nothing stored: every diagonal is missing
    assert np.isposinf(E.jacobi()).all() and not E.mark_dirichlet().any()
    with pytest.raises(esp._lib.EspError, match="column 1 has no stored diagonal"):
        E.ilu0()
