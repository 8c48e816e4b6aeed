"""CPU: the patterns whose panels the reference's BlockYTY row layout cannot express are refused by the product's analysis
(qrk_bb_analyze_host; qrk_bb_plan_create shares the code) and by the oracle, and the rule is neither too wide nor too narrow.

The reference places the rows of a panel's Q block as numCols rows at rowIndex, numZeros skipped rows, then the rest
(BlockYTY.h:152-172).  For dense strips of ms x n stepping by s columns the panels after the second skip rows, and their own
strip's rows land on their matrix rows only if the ms - s carried rows fill the first segment: ms - s >= n (the general rule:
include/qrkit_amd.h at qrk_bb_plan_create).  R is right either way; Q, and the least-squares solution through it, are not.

The sweep runs a few hundred strip patterns through analyze_host.  Every accepted one satisfies the reference's invariants
Q R = J and Q^T J = R in the oracle at 1e-12; every refused one violates them in `unguarded_factorize` below, a private copy of the
oracle's chain without the refusal (the arithmetic is the oracle's own: householder_qr, block_triangular_factor, bb_apply_q).
"""
import types

import numpy as np
import pytest
import scipy.sparse as sp

from banded_cases import CASES, REJECTED, case_id, dense_strips
from helpers import rel_fro
from oracle import oracle as orc


def unguarded_factorize(J, suggested=2):
    """oracle.bb_factorize as it was before it refused anything (identity row permutation: the strips are sorted)"""
    M = sp.csr_matrix(J); M.sort_indices()
    blocks = orc.block_info_from_csr(M.shape[0], M.shape[1], M.indptr, M.indices, suggested)
    pmat = M.toarray()
    rows, cols = pmat.shape
    Rd = np.zeros((rows, cols))
    yty = []
    bi = blocks[0]
    Ji = pmat[bi[0]:bi[0] + bi[2], bi[1]:bi[1] + bi[3]].copy()
    activeRows, numZeros = int(bi[2]), 0
    for i in range(len(blocks)):
        idxRow, idxCol, numRows, numCols = (int(v) for v in blocks[i])
        qr, hc = orc.householder_qr(Ji)
        Y = np.eye(activeRows, numCols)
        for bc in range(numCols):
            Y[bc + 1:, bc] = qr[bc + 1:, bc]
        yty.append((Y, -orc.block_triangular_factor(Y, hc[:numCols]), idxCol, numZeros))
        V = np.triu(qr)
        solved = numRows if i == len(blocks) - 1 else int(blocks[i + 1][1]) - idxCol
        for br in range(min(solved, V.shape[0])):
            Rd[idxCol + br, idxCol:idxCol + numCols] = V[br, :numCols]
        if i < len(blocks) - 1:
            nRow, nCol, nRows, nCols = (int(v) for v in blocks[i + 1])
            overlap = (idxCol + numCols) - nCol
            colInc = numCols - overlap
            activeRows = numRows + nRows - colInc
            numZeros = max((nRow + nRows) - activeRows - nCol, 0)
            ncols = nCols if nCols >= overlap else overlap
            Ji = pmat[idxRow + colInc:idxRow + colInc + activeRows, nCol:nCol + ncols].copy()
            if overlap > 0:
                lr = activeRows - nRows
                Ji[:lr, :overlap] = V[colInc:colInc + lr, colInc:colInc + overlap]
    return types.SimpleNamespace(row_perm=np.arange(rows, dtype=np.int32), blocks=blocks, yty=yty, R_dense=Rd)


def invariants(res, Jd):
    """(Q R = J, Q^T J = R) as rel_fro (test/test-qrkit.cpp:251-252)"""
    R = res.R_dense
    return rel_fro(orc.bb_apply_q(res, R, transpose=False), Jd), rel_fro(orc.bb_apply_q(res, Jd, transpose=True), R)


def accepted(J):
    from qrkit_amd import QrkError
    from qrkit_amd.banded import analyze_host
    try:
        analyze_host(J, 2)
        return True
    except QrkError as e:
        assert e.status == 1 and "Q row layout" in str(e), e          # QRK_STATUS_INVALID_ARGUMENT, and it says why
        return False


def sweep():
    """(N, ms, n, s): ms in 8..40, n <= ms, s < n: every pair (n, s) of a coarse grid, with its edges"""
    out = []
    for N in (2, 3, 4):
        for ms in (8, 13, 24, 31, 40):
            ns = sorted({2, 3, ms // 3, ms // 2, ms // 2 + 1, ms - 3, ms - 1} & set(range(2, ms)))      # (portrait strips: n < ms)
            for n in ns:
                for s in sorted({1, 2, n // 2, ms - n - 1, ms - n, ms - n + 1, n - 1} & set(range(1, n))):
                    out.append((N, ms, n, s))
    return out


def test_sweep_accepts_exactly_the_expressible_layouts():
    pats = sweep()
    assert len(pats) >= 200
    n_acc = n_rej = 0
    for key in pats:
        N, ms, n, s = key
        J = dense_strips(*key, seed=11)
        Jd = J.toarray()
        ok = accepted(J)
        assert ok == (N == 2 or ms - s >= n), key                      # the rule for strips, stated in the header
        if ok:
            n_acc += 1
            res = orc.bb_factorize(J, 2)
            np.testing.assert_array_equal(res.R_dense, unguarded_factorize(J).R_dense)     # (the private copy is the oracle's chain)
            e1, e2 = invariants(res, Jd)
            assert e1 <= 1e-12 and e2 <= 1e-12, (key, e1, e2)
        else:
            n_rej += 1
            with pytest.raises(ValueError, match="Q row layout"):      # the oracle refuses what the product refuses
                orc.bb_factorize(J, 2)
            e1, e2 = invariants(unguarded_factorize(J), Jd)
            assert e1 > 1e-6 and e2 > 1e-6, (key, e1, e2)              # the refusal is not too wide: Q really is wrong there
    assert n_acc >= 100 and n_rej >= 50, (n_acc, n_rej)


@pytest.mark.parametrize("key", REJECTED, ids=case_id)
def test_named_patterns_are_refused(key):
    J = dense_strips(*key)
    assert not accepted(J)
    with pytest.raises(ValueError, match="Q row layout"):
        orc.bb_analyze(J, 2)
    res = unguarded_factorize(J)
    e1, e2 = invariants(res, J.toarray())
    assert e1 > 1e-3 and e2 > 1e-3, (e1, e2)
    # R is right all the same: against LAPACK after aligning the row signs
    n = J.shape[1]
    R = res.R_dense[:n]
    Rl = np.linalg.qr(J.toarray(), mode="r")
    Rl = Rl * (np.sign(np.diag(Rl)) * np.sign(np.diag(R)))[:, None]
    assert np.max(np.linalg.norm(R - Rl, axis=1) / np.linalg.norm(Rl, axis=1)) <= 1e-11


def test_existing_inputs_are_still_accepted():
    """Every input of tests/test_banded.py and tests/test_oracle_blockmap.py, the golden banded_overlap_32.npz and the table of
    tests/test_banded_classes_gpu.py: product and oracle accept them."""
    import os
    from test_banded import banded_matrix, strip_matrix
    from test_oracle_blockmap import block_diag_pattern, shuffled
    mats = [(banded_matrix(64, ov, sh), sug) for ov, sh in ((False, None), (True, None), (True, 3)) for sug in (2, 8)]
    mats += [(banded_matrix(nv, ov, sh), sug) for nv, ov, sh, sug in ((256, False, None, 8), (256, True, None, 8), (256, True, 3, 8),
                                                                      (100, True, 7, 2), (64, True, None, 4), (64, True, 5, 3))]
    mats += [(shuffled(block_diag_pattern(256, False)), 2), (shuffled(block_diag_pattern(256, True), 1), 2)]
    mats += [(strip_matrix(6, 256, 192, 64), 2), (strip_matrix(6, 600, 192, 64), 2), (strip_matrix(5, 256, 192, 64), 2)]
    mats += [(dense_strips(*c[0]), 2) for c in CASES]
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "banded_overlap_32.npz"))
    mats.append((sp.csr_matrix((g["data"], g["indices"], g["indptr"]), shape=tuple(g["shape"])), int(g["suggested"])))
    assert orc.bb_q_layout_error(g["blocks"]) is None                 # (the reference's own block map of that matrix)
    from qrkit_amd.banded import analyze_host
    for J, sug in mats:
        _, blocks, _ = analyze_host(J, sug)
        np.testing.assert_array_equal(blocks, orc.bb_analyze(J, sug)[1])
