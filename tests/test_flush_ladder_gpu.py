"""The rungs of flush_local's ladder (csrc/flush.hip) that no other test of the suite takes (NOTES/round17.md has the table of
which test takes which rung): the re-assembly form of group3_k accepted in its WIDE form, and a held-back stencil batch that
finds no usable table at flush time.

Every flush is compared by the arrays' raw bytes with the same calls on a handle pinned to the general path
(esp_debug_force_path 2) and with the CPU oracle; the readouts of the flush that took the rung and of the next flush on the same
handle are asserted."""
import numpy as np
import pytest

import pair_streams as ps
from test_bucket_pairs_gpu import _assert_same

pytestmark = pytest.mark.gpu

GENERAL = 2                 # ESP_PATH_GENERAL
NO_PREDICTED_OFFSETS = 43
NO_LAZY_STENCIL = 44


def test_hits_form_accepted_wide(esp, orc):
    """A P1 mesh of 520^2 = 270 400 nodes (just above 2^18) with permuted node numbers: a segment's rows spread over the whole
    matrix.  The fresh assembly is refused by group3_k for its rows alone and taken by its wide form, which the handle keeps
    (readout 3).  The second assembly, over the pattern the first one built, is the re-assembly form, wide at once (readout 5:
    esp_handle::last_group3 == 4) -- its item records are expanded first, the fused item kernel has no wide form -- and so is
    the third."""
    dim, npd = 2, 520
    nn = npd ** dim
    assert nn > (1 << 18)
    cn, em, dg = orc.fem_mesh(dim, npd, seed=0x5EED0004, order_mode=1, node_mode=1)
    A = esp.ExtendableSparseMatrix(nn, nn)
    G = esp.ExtendableSparseMatrix(nn, nn)
    G.debug_force_path(GENERAL)
    O = orc.ExtendableSparseMatrix(nn, nn)
    seen = []
    for step, f in enumerate((1.0, -0.5, 1.75)):
        emf, dgf = np.asfortranarray(em * f), np.asfortranarray(dg * f)
        I, J, V = orc.elements_stream(cn, emf, dgf)
        for X in (A, G):
            X.append_elements(cn, emf, dgf)
            X.flush()
        O.apply(np.full(len(I), ps.RAWUPDATE, np.uint8), I, J, V)
        O.flush()
        seen.append((A.debug_last_local_small(), A.debug_last_lazy_items(), A.debug_last_key_bytes(), A.debug_last_path()))
        print("step", step, "local_small, lazy_items, key_bytes, path", seen[-1], "general path", G.debug_last_path())
        assert G.debug_last_path() == 2
        got = A.arrays()
        _assert_same(got, G.arrays(), "general path, step %d" % step)
        _assert_same(got, O.arrays(), "oracle, step %d" % step)
    assert seen[0] == (3, 0, 4, 1), seen      # (refused for its rows alone: the wide form, over the expanded entries)
    assert seen[1] == (5, 0, 4, 1), seen      # the rung: the re-assembly form accepted in its wide form
    assert seen[2] == (5, 0, 4, 1), seen      # ... and the handle stays there


def test_stencil_batch_without_a_table(esp, orc):
    """A 44^3 fdrand! batch is held back (the handle's last flush was served by the fused kernel and left its table); before the
    flush the predicted form is switched off (esp_debug_force_path 43): flush_local finds no table to use, the held-back PART
    launch is issued (esp_debug_last_lazy_stencil 2) and pair_k's look-back form serves the flush.  With the hook off again the
    next assembly does what a handle that always writes its batch (44) does."""
    g = (44, 44, 44)
    N = 44 ** 3
    A = esp.ExtendableSparseMatrix(N, N)
    B = esp.ExtendableSparseMatrix(N, N)
    B.debug_force_path(NO_LAZY_STENCIL)
    G = esp.ExtendableSparseMatrix(N, N)
    G.debug_force_path(GENERAL)

    def what(X):
        return (X.debug_last_predicted(), X.debug_last_bucket_pairs(), X.debug_last_plan_reused())

    def assemble(seed, hook=None):
        for X in (A, B, G):
            X.reset()
            X.generate_fdrand(*g, seed=seed, rand_mode=1)
        if hook is not None:
            assert A.debug_last_lazy_stencil() == 0      # (armed, nothing written yet)
            A.debug_force_path(hook)
        for X in (A, B, G):
            X.flush()
        if hook is not None:
            A.debug_force_path(0)
        got = A.arrays()
        _assert_same(got, B.arrays(), "batch always written, seed %x" % seed)
        _assert_same(got, G.arrays(), "general path, seed %x" % seed)
        I, J, V = orc.fdrand_stream(*g, rand_mode=1, seed=seed)
        _assert_same(got, ps.oracle_csc(orc, N, N, ps.UPDATE, I, J, V), "oracle, seed %x" % seed)
        print("seed %x" % seed, "auto", what(A), A.debug_last_lazy_stencil(), "written", what(B), "general path", G.debug_last_path())
        assert G.debug_last_path() == 2 and B.debug_last_lazy_stencil() == 0

    assemble(0x5EED0002)
    assemble(0x5EED0002)
    assert A.debug_last_lazy_stencil() == 1 and what(A) == (1, 1, 1)      # served by the fused kernel
    assemble(0x5EED0B0B, hook=NO_PREDICTED_OFFSETS)
    assert A.debug_last_lazy_stencil() == 2                               # the rung: armed, then written after all
    assert what(A) == (0, 1, 1), what(A)                                  # ... and pair_k's look-back form took the entries
    assert A.debug_last_local_small() == 1 and A.debug_last_key_bytes() == 4 and A.debug_last_colptr_direct() == 1
    assemble(0x5EED0002)
    assert what(A) == what(B), (what(A), what(B))
    assert A.debug_last_lazy_stencil() == (1 if what(B) == (1, 1, 1) else 0)
