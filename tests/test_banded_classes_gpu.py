"""GPU: the banded CSR chain (qrk_bb_*, qrkit_amd/csrc/banded.hip) at every panel class it chooses its code by.

bb_chain2_kernel / bb_chain_kernel, 32- or 16-column blocks, 3 / 4 / 8 / 16 row registers, a partial last block behind a block
update, T packed in LDS or built in place, odd and nearly square panels: tests/banded_cases.py lists one matrix of dense strips
per class, each on the edge of its threshold.  Every case first asserts that the plan's panels are exactly the shapes it was
made for, that they are the oracle's, and that qrk_bb_kernel_name names the code it was made for: a case that no longer reaches
its class fails instead of passing vacuously.

Judges and bounds are those of tests/test_banded.py::test_hip_banded_baseline_shaped_panels (the oracle: structure bit-exact, R, Y,
T, Q R = J, Q^T J = R at 1e-12, LS recovery at 1e-10), plus one judge that shares nothing with the oracle: R against
numpy.linalg.qr after aligning the row signs, largest relative row error <= 1e-11 (the bound of tests/test_banded_strips_gpu.py;
the oracle itself stays below 3e-15 there).  Every case factorizes twice on one plan, the values of the second run being new ones,
so that nothing left in LDS or scratch by the first can stand in.

The two cases of more than 256 columns are the ones that found bb_apply_q_kernel leaving out the columns beyond the 256 it holds
in registers (Q R = J off by 1e-2 with a right R): panels that wide now run the kernel's WIDE variant.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spl

from banded_cases import CASES, CLASSES, REJECTED, case_id, dense_strips, matrix_and_oracle, panel_shapes
from helpers import rel_fro
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SOLVE_R = {(3, 96, 17, 9), (2, 130, 129, 65), (2, 210, 201, 100)}       # `solved` no multiple of 64: 9 / 17, 65 / 129, 100 / 201


@pytest.fixture(autouse=True)
def stop_after_a_device_error():
    """A GPU fault ends the session: nothing more is started on a device that has faulted (as tests/test_guarded_gpu.py::sync)"""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, no further case is run: {e}", returncode=3)


def kernel_names(qr):
    from qrkit_amd import _capi as capi
    return [capi.lib().qrk_bb_kernel_name(qr._plan, k).decode() for k in range(len(qr.blocks))]


def rows_vs_lapack(R, Jd):
    n = Jd.shape[1]
    Rl = np.linalg.qr(Jd, mode="r")
    Rl = Rl * (np.sign(np.diag(Rl)) * np.sign(np.diag(R[:n])))[:, None]
    return float(np.max(np.linalg.norm(R[:n] - Rl, axis=1) / np.linalg.norm(Rl, axis=1)))


def judge(qr, J, ref, tag):
    """every judge of the module docstring on a factorised solver; prints each figure before it is asserted"""
    np.testing.assert_array_equal(qr.blocks, ref.blocks)
    np.testing.assert_array_equal(qr.rowsPermutation(), ref.row_perm)
    np.testing.assert_array_equal(qr.rowsPermutation(), np.arange(J.shape[0]))
    R = qr.matrixR()
    np.testing.assert_array_equal(R.indptr, ref.R.indptr)
    np.testing.assert_array_equal(R.indices, ref.R.indices)
    Jd, Rd = J.toarray(), R.toarray()
    fig = {"R": rel_fro(Rd, ref.R.toarray()), "R_lapack": rows_vs_lapack(Rd, Jd)}
    for k in (0, len(ref.yty) - 1):
        Y, T, row, nz = qr.blockYTY(k)
        Yo, To, rowo, nzo = ref.yty[k]
        assert (row, nz) == (rowo, nzo) and Y.shape == Yo.shape and T.shape == To.shape
        fig[f"Y{k}"], fig[f"T{k}"] = rel_fro(Y, Yo), rel_fro(T, To)
    fig["QR=J"] = rel_fro(qr.applyQ(Rd), Jd)
    fig["QtJ=R"] = rel_fro(qr.applyQt(Jd), Rd)
    rng = np.random.default_rng(0)
    x1, x3 = rng.uniform(-1, 1, J.shape[1]), rng.uniform(-1, 1, (J.shape[1], 3))
    fig["ls1"], fig["ls3"] = rel_fro(qr.solve(J @ x1), x1), rel_fro(qr.solve(J @ x3), x3)
    print(tag, " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        bound = 1e-11 if k == "R_lapack" else 1e-10 if k.startswith("ls") else 1e-12
        assert v <= bound, (tag, k, v, fig)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_panel_class(case):
    import qrkit_amd
    key, want_name, what = case
    J, ref = matrix_and_oracle(key)
    qr = qrkit_amd.BandedBlockedSparseQR(suggestedBlockCols=2)
    qr.compute(J)
    # the case reaches the class it is there for
    shapes = panel_shapes(*key)
    assert [(int(r[2]), int(r[3])) for r in qr.yty] == shapes, what
    assert [Y.shape for Y, *_ in ref.yty] == shapes, what
    np.testing.assert_array_equal(qr.blocks, ref.blocks)
    names = kernel_names(qr)
    assert names[-1] == want_name, (what, names)
    judge(qr, J, ref, f"{case_id(case)} [{names[-1]}] first run:")
    # a second factorisation on the same plan, new values
    J2, ref2 = matrix_and_oracle(key, seed=17)
    qr.factorize(J2)
    judge(qr, J2, ref2, f"{case_id(case)} second run:")
    if key in SOLVE_R:
        solve_r_on_device(qr, J2)


def solve_r_on_device(qr, J):
    """qrk_bb_solve_r with ldv = rows and 3 right-hand sides against a host triangular solve with the same R, as
    tests/test_banded.py::test_hip_banded_solve_r_on_device"""
    import torch
    from qrkit_amd import _capi as capi
    rows, cols = J.shape
    R = qr.matrixR().tocsr()[:cols, :]
    Y = np.random.default_rng(5).uniform(-1, 1, (rows, 3))
    want = spl.spsolve_triangular(R, Y[:cols], lower=False)
    v = torch.as_tensor(Y.T.copy(), device="cuda")                      # [nrhs, rows] = column-major, ld = rows
    capi.check(capi.lib().qrk_bb_solve_r(qr._plan, v.data_ptr(), rows, 3, capi.MEM_DEVICE), qr._ctx.handle)
    torch.cuda.synchronize()
    got = v.cpu().numpy()
    e = rel_fro(got[:, :cols].T, want)
    print(f"solve_r {rows}x{cols}: {e:.2e}")
    assert e <= 1e-11
    np.testing.assert_array_equal(got[:, cols:].T, Y[cols:])            # rows beyond cols untouched
    h = np.asfortranarray(Y.copy())
    capi.check(capi.lib().qrk_bb_solve_r(qr._plan, h.ctypes.data_as(C.POINTER(C.c_double)), rows, 3, capi.MEM_HOST), qr._ctx.handle)
    np.testing.assert_array_equal(h[:cols], got[:, :cols].T)


def test_every_class_is_hit(monkeypatch):
    """The names qrk_bb_kernel_name gives over all panels of the table -- the same plans, no launch -- are exactly CLASSES: a class
    added later without a case fails here, and so does a case that no longer reaches its class.  The one name no matrix reaches
    without a switch (T in place needs more than 200 columns, NR 3 at most 192 rows) is reached with QRK_BB_T_GLOBAL."""
    import qrkit_amd
    from qrkit_amd import _capi as capi
    for k in ("QRK_BB_T_GLOBAL", "QRK_BB_CHAIN_V1"):
        monkeypatch.delenv(k, raising=False)
    hit = set()
    for key, want_name, _ in CASES:
        qr = qrkit_amd.BandedBlockedSparseQR(suggestedBlockCols=2)
        qr.analyzePattern(matrix_and_oracle(key)[0])
        names = kernel_names(qr)
        assert names[-1] == want_name
        hit.update(names)
        assert capi.lib().qrk_bb_kernel_name(qr._plan, len(names)) == b"" and capi.lib().qrk_bb_kernel_name(qr._plan, -1) == b""
    assert capi.lib().qrk_bb_kernel_name(None, 0) == b""
    assert sorted(hit) == CLASSES, (sorted(hit - set(CLASSES)), sorted(set(CLASSES) - hit))
    qr = qrkit_amd.BandedBlockedSparseQR(suggestedBlockCols=2)
    qr.analyzePattern(matrix_and_oracle((3, 24, 16, 8))[0])
    monkeypatch.setenv("QRK_BB_T_GLOBAL", "1")
    assert kernel_names(qr)[-1] == "bb_chain2_kernel ob32 nr3 t_global"
    monkeypatch.setenv("QRK_BB_CHAIN_V1", "1")
    assert kernel_names(qr)[-1] == "bb_chain_kernel"


@pytest.mark.parametrize("key", REJECTED, ids=case_id)
def test_inexpressible_q_layout_is_refused(key):
    """Panels whose rows the reference's BlockYTY layout cannot express (include/qrkit_amd.h, qrk_bb_plan_create): compute() raises
    instead of returning a wrong Q with QRK_STATUS_OK."""
    import qrkit_amd
    qr = qrkit_amd.BandedBlockedSparseQR(suggestedBlockCols=2)
    with pytest.raises(qrkit_amd.QrkError, match="Q row layout") as e:
        qr.compute(dense_strips(*key))
    assert e.value.status == 1                                          # QRK_STATUS_INVALID_ARGUMENT
