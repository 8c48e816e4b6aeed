"""GPU: the caller-owned device arrays of the banded CSR calls (qrk_bb_factorize, qrk_bb_apply_q, qrk_bb_solve_r) guard-banded at
the extents include/qrkit_amd.h documents (tests/guarded.py), as tests/test_guarded_gpu.py does for the other solvers: a store past
y_len or t_len from the padded tiles of a partial last block, a read past an input's extent that reaches an output, a write into an
input, an output element left unwritten.

Cases (tests/banded_cases.py::GUARDED): a partial block of 17 columns with odd m; blocks 32 + 1; NR 3 then NR 4 with four blocks
and one column; the in-place T recurrence at n = 201; bb_chain_kernel at n = 257.  Each at shift 0 (16-byte aligned arrays) and
shift 1 (8 bytes off).  The values are judged as in tests/test_banded_classes_gpu.py: R, Y and T of every panel against the
oracle at 1e-12, Q^T J = R and Q R = J on three columns at 1e-12, the back substitution against a host triangular solve at 1e-11.
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spl

from banded_cases import CASES, GUARDED, case_id, matrix_and_oracle
from guarded import Net
from helpers import rel_fro

pytestmark = pytest.mark.gpu


def sync():
    """A GPU fault ends the session here: nothing more is started on a device that has faulted"""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, no further case is run: {e}", returncode=3)


@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("key", GUARDED, ids=case_id)
def test_banded_calls_stay_inside_their_arrays(key, shift):
    import qrkit_amd
    from qrkit_amd import _capi as capi
    L = capi.lib()
    J, ref = matrix_and_oracle(key)
    rows, cols = J.shape
    qr = qrkit_amd.BandedBlockedSparseQR(suggestedBlockCols=2)
    qr.analyzePattern(J)
    want_name = {c[0]: c[1] for c in CASES}[key]
    assert L.qrk_bb_kernel_name(qr._plan, len(qr.blocks) - 1).decode() == want_name
    h = qr._ctx.handle
    qr._ctx.use_current_stream()

    # ---- qrk_bb_factorize: csr_vals[nnz] in; r_vals[nnz_r], y_vals[y_len], t_vals[t_len] out (extents: qrk_bb_plan_info)
    net = Net("cuda", shift)
    vals = net.inp("csr_vals", J.data)
    r = net.out("r_vals", qr._nnz_r)
    y = net.out("y_vals", qr._ylen)
    t = net.out("t_vals", qr._tlen)
    capi.check(L.qrk_bb_factorize(qr._plan, vals.ptr, J.nnz, r.ptr, y.ptr, t.ptr, capi.MEM_DEVICE), h)
    sync()
    net.check()
    R = ref.R.copy()
    R.data = r.get()                                                    # (the pattern is the oracle's: asserted by the class tests)
    assert rel_fro(R.toarray(), ref.R.toarray()) <= 1e-12
    yv, tv = y.get(), t.get()
    for k, (Yo, To, rowo, nzo) in enumerate(ref.yty):
        row, nz, m, n, yo, to = (int(v) for v in qr.yty[k])
        assert (row, nz, m, n) == (rowo, nzo) + Yo.shape
        Y = np.tril(yv[yo:yo + m * n].reshape(m, n), -1) + np.eye(m, n)
        T = tv[to:to + n * n].reshape(n, n).T
        assert rel_fro(Y, Yo) <= 1e-12 and rel_fro(T, To) <= 1e-12, (k, rel_fro(Y, Yo), rel_fro(T, To))
        assert np.abs(np.tril(T, -1)).max() == 0                        # the strict lower triangle is written, as zeros

    # ---- qrk_bb_apply_q, both directions: y_vals, t_vals in; v (rows x 3, ld = rows) in place
    Jd, Rd = J.toarray(), R.toarray()
    pick = [0, cols // 2, cols - 1]
    for transpose, src, want in ((1, Jd[:, pick], Rd[:, pick]), (0, Rd[:, pick], Jd[:, pick])):
        net = Net("cuda", shift)
        yi, ti = net.inp("y_vals", yv), net.inp("t_vals", tv)
        v = net.panel_in("v", src, rows, role="inout")
        capi.check(L.qrk_bb_apply_q(qr._plan, yi.ptr, ti.ptr, transpose, v.ptr, 3, capi.MEM_DEVICE), h)
        sync()
        net.check()
        assert rel_fro(v.get(), want) <= 1e-12, (transpose, rel_fro(v.get(), want))

    # ---- qrk_bb_solve_r: v a strided panel with ldv = rows; the rows cols..rows of every column are not touched
    B = np.random.default_rng(5).uniform(-1, 1, (rows, 3))
    net = Net("cuda", shift)
    v = net.panel_in("v", B, rows, role="inout")
    capi.check(L.qrk_bb_solve_r(qr._plan, v.ptr, rows, 3, capi.MEM_DEVICE), h)
    sync()
    net.check()
    got = v.get()
    want = spl.spsolve_triangular(R.tocsr()[:cols, :], B[:cols], lower=False)
    assert rel_fro(got[:cols], want) <= 1e-11
    np.testing.assert_array_equal(got[cols:].view(np.int64), B[cols:].view(np.int64))
