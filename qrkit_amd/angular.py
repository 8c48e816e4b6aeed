"""Host-side mirror of the block-angular composition.

  QRKit::BlockMatrix1x2          (src/QRKit/BlockMatrix1x2.h:31-67)       -> BlockMatrix1x2
  QRKit::BlockAngularSparseQR    (src/QRKit/BlockAngularSparseQR.h:79-419) -> BlockAngularSparseQR
  its right-block solver, Eigen::ColPivHouseholderQR<MatrixXd> in the reference tests
  (test/test-qrkit.cpp:46-48)                                             -> DenseColPivQR

All arithmetic runs in the HIP library through the C ABI (qrk_bd_*, qrk_dense_*); torch holds the device
buffers and moves the J2 strips around (slicing / column permutation of the strip in makeR).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _capi as capi
from .solvers import BlockDiagonalSparseQR, Context, SparseBlockDiagonal


class BlockMatrix1x2:
    """Non-owning pair [left | right] (BlockMatrix1x2.h:31-67): left is a SparseBlockDiagonal,
    right a dense (rows x m2) column-major matrix (numpy or a float64 torch tensor)."""

    def __init__(self, left: SparseBlockDiagonal, right):
        self._left, self._right = left, right

    def leftBlock(self):
        return self._left

    def rightBlock(self):
        return self._right

    def rows(self) -> int:
        return int(self._right.shape[0])

    def cols(self) -> int:
        return self._left.cols() + int(self._right.shape[1])

def sparse_to_device_dense(context: Context, mat, row0: int = 0, nrows: Optional[int] = None, row_map=None) -> torch.Tensor:
    """Rows [row0, row0 + nrows) of a scipy sparse matrix as a dense COLUMN-major float64 tensor on the device
    (qrk_sparse_window_to_dense: the nonzeros cross PCIe, the dense copy the reference makes - BlockedThinSparseQR.h:131
    "m_R = mat" - is written on the device).  row_map (nrows integers, a permutation) sends source row row0 + i to row_map[i]."""
    import scipy.sparse as sp
    M = mat if sp.isspmatrix_csr(mat) or sp.isspmatrix_csc(mat) else sp.csc_matrix(mat)
    if not M.has_canonical_format:
        M = M.copy(); M.sum_duplicates()
    rows, cols = M.shape
    nrows = rows - row0 if nrows is None else int(nrows)
    dev = context.device
    outer = torch.from_numpy(np.ascontiguousarray(M.indptr, dtype=np.int32)).to(dev)
    inner = torch.from_numpy(np.ascontiguousarray(M.indices, dtype=np.int32)).to(dev)
    vals = torch.from_numpy(np.ascontiguousarray(M.data, dtype=np.float64)).to(dev)
    rmap = None if row_map is None else torch.as_tensor(np.asarray(row_map, dtype=np.int32)).to(dev)
    out = torch.empty(cols, max(nrows, 1), dtype=torch.float64, device=dev)[:, :nrows].t()   # column-major (nrows, cols)
    context.use_current_stream()
    capi.check(capi.lib().qrk_sparse_window_to_dense(
        context.handle, 1 if sp.isspmatrix_csr(M) else 0, rows, cols, outer.data_ptr(), inner.data_ptr(), vals.data_ptr(),
        int(row0), nrows, rmap.data_ptr() if rmap is not None else None, out.data_ptr(), max(nrows, 1)), context.handle)
    return out


def _sparse_window_into(context: Context, mat, out: torch.Tensor):
    """Every row of a scipy sparse matrix, dense, into the leading columns of the column-major device tensor `out`
    (qrk_sparse_window_to_dense with out's leading dimension)."""
    import scipy.sparse as sp
    M = mat if sp.isspmatrix_csr(mat) or sp.isspmatrix_csc(mat) else sp.csc_matrix(mat)
    if not M.has_canonical_format:
        M = M.copy(); M.sum_duplicates()
    rows, cols = M.shape
    dev = context.device
    outer = torch.from_numpy(np.ascontiguousarray(M.indptr, dtype=np.int32)).to(dev)
    inner = torch.from_numpy(np.ascontiguousarray(M.indices, dtype=np.int32)).to(dev)
    vals = torch.from_numpy(np.ascontiguousarray(M.data, dtype=np.float64)).to(dev)
    context.use_current_stream()
    capi.check(capi.lib().qrk_sparse_window_to_dense(
        context.handle, 1 if sp.isspmatrix_csr(M) else 0, rows, cols, outer.data_ptr(), inner.data_ptr(), vals.data_ptr(),
        0, rows, None, out.data_ptr(), _ld(out)), context.handle)


class DenseColPivQR:
    """Dense Householder QR with implicit Q (Eigen::ColPivHouseholderQR / HouseholderQR interface)."""

    def __init__(self, context: Context, solver: int = capi.COLPIV_HOUSEHOLDER):
        self._ctx, self._solver = context, solver
        self._plan = C.c_void_p()
        self._shape = None

    def compute(self, A: torch.Tensor):
        """A: (rows, cols) float64 torch tensor on the device in COLUMN-major storage, i.e. A.t() contiguous, or a window of
        such a matrix (unit row stride, column stride = its leading dimension).  It is factorised in place (becomes the
        packed QR)."""
        rows, cols = A.shape
        assert A.dtype == torch.float64
        self._lda = _ld(A)
        if self._shape != (rows, cols):
            if self._plan:
                capi.lib().qrk_dense_plan_destroy(self._plan)
            self._plan = C.c_void_p()
            capi.check(capi.lib().qrk_dense_plan_create(self._ctx.handle, rows, cols, self._solver, C.byref(self._plan)),
                       self._ctx.handle)
            self._shape = (rows, cols)
        self._qr = A
        self._hc = torch.empty(max(min(rows, cols), 1), dtype=torch.float64, device=A.device)
        self._perm = torch.empty(max(cols, 1), dtype=torch.int32, device=A.device)
        self._ctx.use_current_stream()
        capi.check(capi.lib().qrk_dense_factorize(self._plan, A.data_ptr(), self._lda, self._hc.data_ptr(),
                                                  self._perm.data_ptr(), capi.MEM_DEVICE), self._ctx.handle)
        return self

    def rows(self):
        return self._shape[0]

    def cols(self):
        return self._shape[1]

    def rank(self):
        return min(self._shape)     # the composition only uses cols() of the right solver's rank on full-rank input

    def colsPermutation(self) -> torch.Tensor:
        return self._perm[:self._shape[1]]

    def matrixR(self) -> torch.Tensor:
        """Upper-triangular min(rows,cols) x cols (dense, device)."""
        k = min(self._shape)
        return torch.triu(self._qr[:k, :])

    def applyQ(self, B: torch.Tensor, transpose: bool) -> torch.Tensor:
        """B: (rows, nrhs) column-major device tensor, updated in place: B <- Q^T B or Q B."""
        rows = self._shape[0]
        assert B.shape[0] == rows
        self._ctx.use_current_stream()
        capi.check(capi.lib().qrk_dense_apply_q(self._plan, self._qr.data_ptr(), self._lda, self._hc.data_ptr(),
                                                1 if transpose else 0, B.data_ptr(), _ld(B), B.shape[1], capi.MEM_DEVICE),
                   self._ctx.handle)
        return B

    def solveR(self, B: torch.Tensor) -> torch.Tensor:
        """B: (cols, nrhs) column-major device tensor, updated in place: B <- R^-1 B with the upper triangle of the
        packed QR (qrk_dense_solve_r; the column permutation is the caller's)."""
        rows, cols = self._shape
        assert B.shape[0] == cols
        self._ctx.use_current_stream()
        capi.check(capi.lib().qrk_dense_solve_r(self._plan, self._qr.data_ptr(), self._lda, B.data_ptr(), _ld(B), B.shape[1],
                                                capi.MEM_DEVICE), self._ctx.handle)
        return B

    def __del__(self):
        try:
            if self._plan:
                capi.lib().qrk_dense_plan_destroy(self._plan)
        except Exception:
            pass


class DenseTSQR:
    """Un-pivoted communication-avoiding QR of a tall dense block on this GPU (qrk_tsqr_*): the per-rank stage of the sharded
    right solver (BlockAngularSparseQR.h:361-369 with the rows of J2 spread over GPUs)."""

    def __init__(self, context: Context):
        self._ctx = context
        self._plan = C.c_void_p()
        self._shape = None

    def compute(self, A: torch.Tensor):
        """A: (rows, cols), rows >= cols, float64, column-major on the device; factorised in place (R0 in the upper triangle of the
        first cols rows)."""
        rows, cols = A.shape
        assert A.dtype == torch.float64 and A.t().is_contiguous() and rows >= cols
        if self._shape != (rows, cols):
            if self._plan:
                capi.lib().qrk_tsqr_plan_destroy(self._plan)
            self._plan = C.c_void_p()
            capi.check(capi.lib().qrk_tsqr_plan_create(self._ctx.handle, rows, cols, C.byref(self._plan)), self._ctx.handle)
            self._shape = (rows, cols)
        self._qr = A
        self._ctx.use_current_stream()
        capi.check(capi.lib().qrk_tsqr_factorize(self._plan, A.data_ptr(), rows, capi.MEM_DEVICE), self._ctx.handle)
        return self

    def matrixR(self) -> torch.Tensor:
        return torch.triu(self._qr[:self._shape[1], :])

    def applyQ(self, B: torch.Tensor, transpose: bool) -> torch.Tensor:
        rows = self._shape[0]
        assert B.shape[0] == rows and B.t().is_contiguous()
        self._ctx.use_current_stream()
        capi.check(capi.lib().qrk_tsqr_apply_q(self._plan, self._qr.data_ptr(), rows, 1 if transpose else 0, B.data_ptr(), rows,
                                               B.shape[1], capi.MEM_DEVICE), self._ctx.handle)
        return B

    def __del__(self):
        try:
            if self._plan:
                capi.lib().qrk_tsqr_plan_destroy(self._plan)
        except Exception:
            pass


class DenseQlessR:
    """The R factor of a tall-skinny dense device matrix without Q (qrk_dense_qless_r): R^T R = A^T A by a tree of
    Householder factorisations whose reflectors are never stored.  A is only read.  At most 32 columns; deterministic; nothing is
    allocated between calls of one shape, and the call enqueues only (it can be captured once the workspace exists)."""

    def __init__(self, context: Context):
        self._ctx = context
        self._shape = None
        self._r = self._work = None

    def compute(self, A: torch.Tensor):
        """A: (rows, cols) float64 device tensor in COLUMN-major storage (A.t() contiguous) or a window of one, cols <= 32; any
        rows >= 0 (missing rows count as zero)."""
        rows, cols = A.shape
        assert A.dtype == torch.float64
        lda = _ld(A)
        if self._shape != (rows, cols):
            dev = A.device
            self._work = torch.empty(int(capi.lib().qrk_dense_qless_r_work(rows, cols)), dtype=torch.float64, device=dev)
            self._r = torch.zeros(cols, max(cols, 1), dtype=torch.float64, device=dev).t()      # column-major cols x cols
            self._shape = (rows, cols)
        self._ctx.use_current_stream()
        capi.check(capi.lib().qrk_dense_qless_r(self._ctx.handle, A.data_ptr(), lda, rows, cols, self._r.data_ptr(), max(cols, 1),
                                                self._work.data_ptr()), self._ctx.handle)
        return self

    def rows(self):
        return self._shape[0]

    def cols(self):
        return self._shape[1]

    def matrixR(self) -> torch.Tensor:
        """Upper-triangular cols x cols (dense, device; exact zeros below the diagonal; the sign of the diagonal is not specified)."""
        return self._r.clone()


class BlockedThinDenseQR(DenseColPivQR):
    """QRKit::BlockedThinDenseQR (BlockedThinDenseQR.h:53-176): Householder QR of a thin dense matrix without column
    pivoting, Q implicit, identity permutations (:139-142).  The reference walks panels of SuggestedBlockCols columns
    (HouseholderQR of the panel at (solvedCols, solvedCols), Y/T, block-reflector update of the columns from the panel on,
    BlockedThinQRBase.h:309-333).  The reflectors of that chain ARE the reflectors of one HouseholderQR of the whole matrix
    (a panel's columns arrive updated by every earlier reflector, and inside the panel HouseholderQR is the same recurrence),
    so the device computes that factorisation (qrk_dense_*, QRK_HOUSEHOLDER) and keeps Q as essential vectors + tau instead
    of per-panel (Y, T): R and every product with Q agree with the panel chain to rounding (tests/test_thin_gpu.py compares
    with a CPU restatement of the chain); `suggestedBlockCols` therefore does not change the result."""

    def __init__(self, context: Context, suggestedBlockCols: int = 2):
        super().__init__(context, capi.HOUSEHOLDER)
        self.suggestedBlockCols = suggestedBlockCols

    def compute(self, A):
        if hasattr(A, "tocsc"):
            A = sparse_to_device_dense(self._ctx, A)              # (densified on the device: the nonzeros cross PCIe)
        if not isinstance(A, torch.Tensor):
            A = _colmajor(torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).to(self._ctx.device))
        return super().compute(A)

    def rank(self):
        return self._shape[1]            # m_nonzeroPivots = m_R.cols() (BlockedThinDenseQR.h:132)

    def colsPermutation(self) -> torch.Tensor:
        return torch.arange(self._shape[1], dtype=torch.int32, device=self._qr.device)   # identity (:139)

    def rowsPermutation(self) -> torch.Tensor:
        return torch.arange(self._shape[0], dtype=torch.int32, device=self._qr.device)   # identity (:142)

    def _applyAny(self, v, transpose: bool):
        was_np = not isinstance(v, torch.Tensor)
        t = torch.as_tensor(np.asarray(v, dtype=np.float64)) if was_np else v
        y = _colmajor(t.to(self._ctx.device, torch.float64).reshape(self._shape[0], -1).clone())
        self.applyQ(y, transpose=transpose)
        out = y if np.ndim(v) > 1 else y[:, 0]
        return out.cpu().numpy() if was_np else out

    def matrixQ(self):
        """Product expression (BlockedThinQRBase.h:335-470)."""
        from .qproduct import QProduct
        slv = self

        class _Ops:          # applyQ / applyQt with the (rows, nrhs) calling convention of the expression
            def rows(self_inner): return slv.rows()
            def applyQ(self_inner, v): return slv._applyAny(v, False)
            def applyQt(self_inner, v): return slv._applyAny(v, True)
        return QProduct(_Ops())

    def solve(self, b: torch.Tensor) -> torch.Tensor:
        """BlockedThinQRBase::_solve_impl (BlockedThinQRBase.h:223-247): x = R(0:n,0:n)^-1 (Q^T b)(0:n)."""
        rows, cols = self._shape
        y = _colmajor(b.reshape(rows, -1).clone())
        self.applyQ(y, transpose=True)
        z = _colmajor(y[:cols, :].clone())
        return self.solveR(z)


def column_density_indices(mat) -> np.ndarray:
    """SparseQROrdering::ColumnDensity (SparseQROrdering.h:21-50): columns stable-sorted by their number of nonzeros, as the
    indices of the Eigen permutation it builds (indices[original column] = sorted rank); (A * P)(:, j) = A(:, indices[j])."""
    import scipy.sparse as sp
    M = sp.csc_matrix(mat)
    order = np.argsort(np.diff(M.indptr), kind="stable")
    idx = np.empty(M.shape[1], dtype=np.int32)
    idx[order] = np.arange(M.shape[1], dtype=np.int32)
    return idx


def as_banded_as_possible_indices(mat):
    """SparseQROrdering::AsBandedAsPossible (SparseQROrdering.h:52-120): rows stable-sorted by the column of their first
    nonzero (empty rows last); returns (indices, hasPermutation) with indices[original row] = new row."""
    import scipy.sparse as sp
    M = sp.csr_matrix(mat)
    M.sort_indices()
    rows, cols = M.shape
    start = np.full(rows, cols, dtype=np.int64)
    nz = np.diff(M.indptr) > 0
    start[nz] = M.indices[M.indptr[:-1][nz]]
    has = bool(np.any(start[1:] < start[:-1]))
    order = np.argsort(start, kind="stable") if has else np.arange(rows)
    idx = np.empty(rows, dtype=np.int32)
    idx[order] = np.arange(rows, dtype=np.int32)
    return idx, has


class BlockedThinSparseQR:
    """QRKit::BlockedThinSparseQR (src/QRKit/BlockedThinSparseQR.h:105-283) on the device, through the C entry both language
    mirrors share (qrk_thin_sparse_factorize, include/qrkit_amd.h): analyzePattern (:168-201: ColumnDensity column ordering,
    AsBandedAsPossible row ordering), compute (:105-165: the permuted matrix made dense on the device and factorised panel by
    panel -- a panel of SuggestedBlockCols columns takes the rows its sparsity pattern says, updateBlockInfo :203-238, is
    factorised by the column-pivoted dense solver, its reflectors are applied to the columns to the right, and its columns of R
    are the rows above the diagonal position plus the panel's upper triangle, :271-279).  colsPermutation() = ColumnDensity
    permutation * Householder column permutation with the zero-pivot columns last (:151-159, :250-256); rank() = nonzero pivots
    (Eigen's threshold on the panel's pivots)."""

    def __init__(self, context: Context, suggestedBlockCols: int = 2):
        self._ctx = context
        self.suggestedBlockCols = int(suggestedBlockCols)
        self._plan = C.c_void_p()
        self.m_isInitialized = False

    def _release(self):
        if self._plan:
            capi.lib().qrk_thin_destroy(self._plan)
            self._plan = C.c_void_p()

    def compute(self, mat):
        import scipy.sparse as sp
        M = sp.csc_matrix(mat)
        if not M.has_canonical_format:
            M = M.copy(); M.sum_duplicates()
        M.sort_indices()
        rows, cols = M.shape
        self._release()
        cp = np.ascontiguousarray(M.indptr, dtype=np.int32)
        ri = np.ascontiguousarray(M.indices, dtype=np.int32)
        vv = np.ascontiguousarray(M.data, dtype=np.float64)
        self._ctx.use_current_stream()
        capi.check(capi.lib().qrk_thin_sparse_factorize(self._ctx.handle, rows, cols, self.suggestedBlockCols, cp.ctypes.data,
                                                        ri.ctypes.data, vv.ctypes.data, C.byref(self._plan)), self._ctx.handle)
        rk = C.c_int32()
        cperm = np.empty(cols, np.int32); rperm = np.empty(rows, np.int32)
        capi.check(capi.lib().qrk_thin_info(self._plan, C.byref(rk), cperm.ctypes.data, rperm.ctypes.data), self._ctx.handle)
        dev = self._ctx.device
        self.m_outputPerm_c = torch.from_numpy(cperm).to(dev)
        self.m_rowPerm = torch.from_numpy(rperm).to(dev)
        self.m_nonzeroPivots = int(rk.value)
        self._shape = (rows, cols)
        self._R = None
        self.m_isInitialized = True
        return self

    def rows(self):
        return self._shape[0]

    def cols(self):
        return self._shape[1]

    def rank(self):
        return self.m_nonzeroPivots

    def colsPermutation(self) -> torch.Tensor:
        return self.m_outputPerm_c

    def rowsPermutation(self) -> torch.Tensor:
        return self.m_rowPerm

    def matrixR(self) -> torch.Tensor:
        """rows x cols, dense on the device (the reference keeps it sparse, column by column)."""
        if self._R is None:
            rows, cols = self._shape
            top = torch.empty(cols, cols, dtype=torch.float64, device=self._ctx.device)      # column-major cols x cols
            capi.check(capi.lib().qrk_thin_matrix_r(self._plan, top.data_ptr(), cols, capi.MEM_DEVICE), self._ctx.handle)
            R = torch.zeros(rows, cols, dtype=torch.float64, device=self._ctx.device)
            R[:cols] = top.t()
            self._R = R
        return self._R

    def _padded(self, v):
        """(2 rows, nrhs) column-major work copy of v with zero rows appended (the panels are applied with zero rows below them)."""
        rows = self._shape[0]
        t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float64))
        t = t.to(self._ctx.device, torch.float64).reshape(rows, -1)
        y = torch.zeros(t.shape[1], 2 * rows, dtype=torch.float64, device=self._ctx.device)
        y[:, :rows] = t.t()
        return y                                                     # y.t() is the column-major (2 rows, nrhs) matrix

    def _applyAny(self, v, transpose: bool):
        """SparseBlockYTY sequence (SparseBlockYTY.h:111-138): Q^T v = panels in order, Q v = in reverse; a panel acts on its
        row range only."""
        was_np = not isinstance(v, torch.Tensor)
        rows = self._shape[0]
        y = self._padded(v)
        self._ctx.use_current_stream()
        capi.check(capi.lib().qrk_thin_apply_q(self._plan, 1 if transpose else 0, y.data_ptr(), 2 * rows, y.shape[0]), self._ctx.handle)
        out = y[:, :rows].t()
        out = out if np.ndim(v) > 1 else out[:, 0]
        return out.cpu().numpy() if was_np else out

    def matrixQ(self):
        from .qproduct import QProduct
        slv = self

        class _Ops:
            def rows(self_inner): return slv.rows()
            def applyQ(self_inner, v): return slv._applyAny(v, False)
            def applyQt(self_inner, v): return slv._applyAny(v, True)
        return QProduct(_Ops())

    def solve(self, b):
        """BlockedThinQRBase::_solve_impl (BlockedThinQRBase.h:223-247): y = Q^T b; x(0:rank) = R(0:rank,0:rank)^-1 y(0:rank),
        the rest zero (the caller applies the permutations, as with the reference)."""
        rows, cols = self._shape
        was_np = not isinstance(b, torch.Tensor)
        y = self._padded(b)
        self._ctx.use_current_stream()
        capi.check(capi.lib().qrk_thin_solve(self._plan, y.data_ptr(), 2 * rows, y.shape[0]), self._ctx.handle)
        x = y[:, :cols].t()
        x = x if np.ndim(b) > 1 else x[:, 0]
        return x.cpu().numpy() if was_np else x.clone()

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def _ld(t: torch.Tensor) -> int:
    """Leading dimension of a 2-D device tensor in column-major storage (t.t() contiguous) or of a window of one."""
    rows, cols = t.shape
    assert rows <= 1 or t.stride(0) == 1, "column-major storage expected"
    ld = int(t.stride(1)) if cols > 1 else rows
    assert ld >= rows, "column-major storage expected"
    return max(ld, 1)


def _colmajor(t: torch.Tensor) -> torch.Tensor:
    """Device tensor with column-major storage and the same logical shape."""
    return t.t().contiguous().t()


class BlockAngularSparseQR:
    """QRKit::BlockAngularSparseQR<BlockDiagonalSparseQR<...>, ColPivHouseholderQR<MatrixXd>>:
    QR of [J1 | J2] with J1 block diagonal and J2 dense (BlockAngularSparseQR.h:459-514)."""

    def __init__(self, context: Optional[Context] = None, device: int = 0,
                 leftBlockSolver: int = capi.COLPIV_HOUSEHOLDER, rightSolver: int = capi.COLPIV_HOUSEHOLDER):
        self._ctx = context or Context(device)
        self.m_leftSolver = BlockDiagonalSparseQR(blockSolver=leftBlockSolver, qFormat=capi.FULL_Q, context=self._ctx)
        self.m_rightSolver = DenseColPivQR(self._ctx, rightSolver)
        self.m_isInitialized = False
        self._qless = False          # the last factorisation was factorizeAndSolve(): Q1 was never formed
        self._W = self._Win = None   # rows x (m2 + 1) work matrices of factorizeAndSolve(), kept between calls of one shape
        self._lm_ready = False       # factorizeAndSolve() took the fused route: W holds the factors lmSolve() works on
        self._lm_np = True           # ... and b was a numpy array
        self._lm = None              # work arrays and dense plan of lmSolve() on the route in use, kept between calls of one shape
        self._lm_base = None         # ... the arrays both routes share, and the per-route sets
        self._lm_routes = {}
        self._lm_route = "auto"      # setLmRoute()

    def compute(self, mat: BlockMatrix1x2):
        self.analyzePattern(mat)
        self.factorize(mat)

    def computeAndSolve(self, mat: BlockMatrix1x2, b, returnQtB: bool = False):
        """analyzePattern() + factorizeAndSolve(): compute() followed by solve(b), without Q1."""
        self.analyzePattern(mat)
        return self.factorizeAndSolve(mat, b, returnQtB=returnQtB)

    def factorizeAndSolve(self, mat: BlockMatrix1x2, b, returnQtB: bool = False):
        """factorize(mat) and solve(b) for ONE right-hand side in one pass that never owns Q1: the Levenberg-Marquardt step of
        examples/ellipse_fitting.cpp:117-142 (BlockAngularSparseQR.h:361-369, 459-514, 202-227).  Runs after analyzePattern().

        One device matrix W (rows x (m2 + 1), leading dimension rows) carries the step: the panel [J2.top(n1) | b.top(n1)]
        goes through qrk_bd_factorize_apply_qt into W's top n1 rows, the rows below are copied, the right solver factorizes
        W(m1:, 0:m2) in place, its Q^T updates rows m1.. of the last column, and the back substitution reads the strip
        S = W(0:m1, 0:m2) where it lies.  Returns x, or (x, Q^T b) with returnQtB.  Afterwards matrixR / colsPermutation /
        rowsPermutation / rank / info work; matrixQ / applyQ / applyQt / solve raise until the next compute().

        With fewer bottom rows than right columns (rows - m1 < m2) the call takes the compute() + solve() route."""
        dev = self._ctx.device
        left, right = mat.leftBlock(), mat.rightBlock()
        m1, n1 = self.m_leftCols, self.m_leftRows
        rows, m2 = int(right.shape[0]), int(right.shape[1])
        n2 = rows - n1
        was_np = not isinstance(b, torch.Tensor)
        bt = (torch.as_tensor(np.asarray(b, dtype=np.float64)) if was_np else b).reshape(-1)
        assert bt.shape[0] == rows, "SparseQR::solve() : invalid number of rows in the right hand side matrix"
        self._lm_ready = False
        if rows - m1 < m2:
            self.factorize(mat)
            x = self.solve(b)
            return (x, self.applyQt(b)) if returnQtB else x
        if self._W is None or tuple(self._W.shape) != (rows, m2 + 1):
            self._W = torch.empty(m2 + 1, rows, dtype=torch.float64, device=dev).t()       # column-major
            self._Win = torch.empty(m2 + 1, rows, dtype=torch.float64, device=dev).t()
        W, Win = self._W, self._Win
        self._ctx.use_current_stream()
        if hasattr(right, "tocsc"):          # sparse right block: only its nonzeros cross PCIe, made dense in W's input
            _sparse_window_into(self._ctx, right, Win)
        else:
            J2 = torch.as_tensor(np.asarray(right, dtype=np.float64)) if not isinstance(right, torch.Tensor) else right
            Win[:, :m2].copy_(J2)
        Win[:, m2].copy_(bt)
        self._qless = True
        self.m_isInitialized = False
        # J1 = Q1 R1 and [J2.top(n1) | b.top(n1)] <- Q1^T of it (:472-475, :361-369); the left solver's row permutation is the identity
        self.m_leftSolver.analyzePattern(left)
        self.m_leftSolver.factorizeApplyQtDevice(left, Win.data_ptr(), rows, m2 + 1, W.data_ptr(), rows)
        assert self.m_leftSolver.info() == capi.INFO_SUCCESS
        if n2 > 0:
            W[n1:, :].copy_(Win[n1:, :])
        # rightSolver.compute(J2.bottomRows(rows - m1)) in place in W, then Q2^T on rows m1.. of the right-hand side
        self.m_rightSolver.compute(W[m1:, :m2])
        self.m_rightSolver.applyQ(W[m1:, m2:], transpose=True)
        self._J2 = W[:, :m2]
        self._P2 = self.m_rightSolver.colsPermutation().long()
        self._m1, self._m2, self._n1, self._n2 = m1, m2, n1, n2
        p1 = torch.as_tensor(self.m_leftSolver.colsPermutation(), device=dev).long()
        self.m_outputPerm_c = torch.cat([p1, m1 + self._P2]).to(torch.int32)
        self.m_rowPerm = np.arange(self._rows, dtype=np.int32)
        self.m_nonzeropivots = self.m_leftSolver.rank() + min(rows - m1, m2)
        self.m_isInitialized = True
        self.m_info = capi.INFO_SUCCESS
        # _solve_impl (:202-227) on y = Q^T b = W(:, m2): z2 = R2^-1 y2, y1 -= S(:, P2) z2, z1 = R1^-1 y1
        y = W[:, m2]
        qtb = y.clone() if returnQtB else None
        z2 = self.m_rightSolver.solveR(y[m1:m1 + m2].clone().reshape(m2, 1))
        rhs1 = y[:m1].clone().reshape(m1, 1)
        p2 = self.m_rightSolver.colsPermutation()
        capi.check(capi.lib().qrk_dense_gemv_sub(self._ctx.handle, W.data_ptr(), rows, m1, m2, p2.data_ptr(), z2.data_ptr(),
                                                 rhs1.data_ptr()), self._ctx.handle)
        z1 = self.m_leftSolver.solveR(rhs1)
        x = torch.empty(m1 + m2, dtype=torch.float64, device=dev)
        x[self.m_outputPerm_c.long()] = torch.cat([z1.reshape(-1), z2.reshape(-1)])
        self._lm_ready, self._lm_np = True, was_np
        if was_np:
            x = x.cpu().numpy()
            qtb = qtb.cpu().numpy() if returnQtB else None
        return (x, qtb) if returnQtB else x

    def lmSolve(self, diag, par: float, returnDxNorm2: bool = False):
        """x = argmin || J x - b ||^2 + par || D x ||^2 on the factors the last factorizeAndSolve() / computeAndSolve() left on
        the device (the damped solve MINPACK's lmpar repeats for every trial par, examples/ellipse_fitting.cpp:257-280): nothing
        is re-factorised, no Q is read, W is not modified -- the call can be repeated with any par >= 0, and matrixR() etc. keep
        working.  diag: cols() positive scale factors in J's column order (left part first), None = ones.

        qrk_bd_lm_panel triangularises [R1; sqrt(par) D1] tile by tile and takes the reflectors over W(0:m1, [P2, m2]): the
        damped left factors, the top panel and the fill, which lands in the right stack G = [R2 y2; fill; sqrt(par) D2(P2) 0]
        (qrk_dense_lm_stack writes the other rows); G(:, 0:m2) is factorised without pivoting (Householder dense plan), Q^T
        goes over its last column, and the back substitution is factorizeAndSolve()'s with the damped factors.  The work
        arrays and the dense plan are kept between calls of one shape.

        On the reduced route (lmRoute(); the default for m2 <= 31) the fill goes to a buffer of its own,
        qrk_dense_qless_r reduces [fill | its right-hand side] (m1 x (m2 + 1)) to one triangle T = [T11 t; 0 rho], and the stack is
        G2 = [R2 y2; T; sqrt(par) D2(P2) 0], (3 m2 + 1) x (m2 + 1): the same minimiser (rho^2 is a constant of the residual), a
        dense factorisation that no longer depends on m1, and no zero rows at par = 0.

        Returns x in J's column order, numpy or tensor as `b` was given to factorizeAndSolve(); with returnDxNorm2 also
        || D x ||^2 (a float, from the returned x).  On the stacked route the dense factorisation of G synchronises the stream when
        (m1 + 2 m2) * m2 >= 2^18 (qrk_dense_factorize): the call cannot be captured into a graph at those sizes.  The reduced
        stack has at most 94 x 31 entries and never gets there.
        Raises before a factorizeAndSolve() / computeAndSolve() that took the fused route (rows - m1 >= m2)."""
        self._lm_require("lmSolve()")
        par = float(par)
        if not par >= 0.0:
            raise ValueError("lmSolve(): par must be >= 0")
        d = self._lm_diag(diag)
        x, _ = self._lm_evaluate(d, par, False)
        dx2 = None
        if returnDxNorm2:
            dx2 = float(torch.sum((x * d) ** 2 if d is not None else x ** 2).item())
        xo = x.cpu().numpy() if self._lm_np else x
        return (xo, dx2) if returnDxNorm2 else xo

    LM_REDUCED_MAX_COLS = 32         # qrk_dense_qless_r's column limit: the reduced route needs m2 + 1 <= 32

    def setLmRoute(self, route: str):
        """How lmSolve() / lmpar() finish the right part: "stacked" factorises the (m1 + 2 m2) x m2 stack with the fill in it (K11),
        "reduced" first reduces the fill to one triangle (K13: needs m2 + 1 <= 32, raises at the next evaluation otherwise),
        "auto" (the default) takes the reduced route where it can.  Both give the same minimiser; each route repeats its own bits."""
        if route not in ("auto", "reduced", "stacked"):
            raise ValueError('setLmRoute(): expected "auto", "reduced" or "stacked"')
        self._lm_route = route

    def lmRoute(self) -> str:
        """The route the next evaluation takes: "reduced" or "stacked".  Under "auto" it depends on m2, so it needs the kept factors."""
        if self._lm_route != "auto":
            return self._lm_route
        self._lm_require("lmRoute()")
        return "reduced" if 1 <= self._m2 < self.LM_REDUCED_MAX_COLS else "stacked"

    def _lm_require(self, who: str):
        if not (self.m_isInitialized and self._qless and self._lm_ready):
            raise RuntimeError(f"{who}: no kept factors; call factorizeAndSolve() or computeAndSolve() first "
                               "(with rows - m1 >= m2: the explicit route keeps none)")

    def _lm_diag(self, diag):
        """diag as cols() float64 entries on the device (None stays None)."""
        if diag is None:
            return None
        d = (torch.as_tensor(np.asarray(diag, dtype=np.float64)) if not isinstance(diag, torch.Tensor) else diag)
        d = d.reshape(-1).to(self._ctx.device, torch.float64).contiguous()
        assert d.numel() == self._m1 + self._m2, "diag: expected cols() entries"
        return d

    def _lm_arrays(self):
        """The work arrays and the dense plan of the damped evaluation on the route in use, kept between calls of one shape.  top, s
        and colidx are shared by the two routes; the stack G (and the reduced route's fill F and workspace) are the route's own, so
        the big G exists only once the stacked route has run."""
        dev = self._ctx.device
        m1, m2, left = self._m1, self._m2, self.m_leftSolver
        route = self.lmRoute()
        key = (m1, m2, left._nnz_r)
        if self._lm_base is None or self._lm_base["key"] != key:
            self._lm_base = {
                "key": key,
                "top": torch.empty(m2 + 1, max(m1, 1), dtype=torch.float64, device=dev).t(),      # column-major m1 x (m2 + 1)
                "s": torch.empty(max(left._nnz_r, 1), dtype=torch.float64, device=dev),
                "colidx": torch.empty(m2 + 1, dtype=torch.int32, device=dev),
            }
            self._lm_routes = {}
        lm = self._lm_routes.get(route)
        if lm is None:
            lm = self._lm_routes[route] = dict(self._lm_base)
            lm["route"] = route
            lm["dense"] = DenseColPivQR(self._ctx, capi.HOUSEHOLDER)
            if route == "reduced":
                ldg = 3 * m2 + 1
                lm["F"] = torch.empty(m2 + 1, max(m1, 1), dtype=torch.float64, device=dev).t()    # column-major m1 x (m2 + 1)
                lm["qwork"] = torch.empty(int(capi.lib().qrk_dense_qless_r_work(m1, m2 + 1)), dtype=torch.float64, device=dev)
            else:
                ldg = m1 + 2 * m2
            lm["G"] = torch.empty(m2 + 1, ldg, dtype=torch.float64, device=dev).t()              # column-major ldg x (m2 + 1)
        self._lm = lm
        return lm

    def _lm_transposed_arrays(self):
        """What the transposed pass and the gradient add to _lm_arrays(): w1, the right vector, the sums and gemv_t's workspace."""
        lm = self._lm_arrays()
        if "w1" not in lm:
            dev = self._ctx.device
            m1, m2 = self._m1, self._m2
            lm["w1"] = torch.empty(max(m1, 1), dtype=torch.float64, device=dev)
            lm["t2"] = torch.empty(max(m2, 1), dtype=torch.float64, device=dev)
            lm["sums2"] = torch.empty(2, dtype=torch.float64, device=dev)
            lm["work"] = torch.empty(int(capi.lib().qrk_dense_gemv_t_work(m1, m2)), dtype=torch.float64, device=dev)
        return lm

    def _lm_evaluate(self, d, par: float, transposed: bool):
        """One damped evaluation on the kept factors: lmSolve()'s chain (on the route lmRoute() names: the stack G is the reduced
        G2 or the stacked G, everything after it is the same), and with `transposed` the forward substitution with the
        damped factor S^ = [S1 Top; 0 Rg] behind it: u = D~^2 z in pivoted order, w1 = S1^-T u1 (qrk_bd_solve_rt
        on s_vals), w2 = Rg^-T (u2 - Top^T w1) (qrk_dense_gemv_t on top, qrk_dense_solve_rt on G's upper triangle).  d: the device
        diag or None.  Returns (x, None), x on the device in J's column order, or (x, (s0, s1, zeros)) with s0 = || D x ||^2,
        s1 = || S^-T u ||^2 and the number of S1's tiles with a zero on the diagonal, brought over in one read-back."""
        dev = self._ctx.device
        m1, m2, rows, W = self._m1, self._m2, self._rows, self._W
        left = self.m_leftSolver
        reduced = self.lmRoute() == "reduced"
        if reduced and not 1 <= m2 < self.LM_REDUCED_MAX_COLS:
            raise RuntimeError(f"the reduced LM route needs 1 <= m2 <= {self.LM_REDUCED_MAX_COLS - 1} (m2 = {m2}); "
                               'setLmRoute("auto") or "stacked"')
        ldg = 3 * m2 + 1 if reduced else m1 + 2 * m2
        lm = self._lm_transposed_arrays() if transposed else self._lm_arrays()
        top, G, s_vals, colidx = lm["top"], lm["G"], lm["s"], lm["colidx"]
        p2 = self.m_rightSolver.colsPermutation()
        colidx[:m2].copy_(p2)
        colidx[m2] = m2
        L, h = capi.lib(), self._ctx.handle
        self._ctx.use_current_stream()
        if reduced:
            # the fill to F, [F | f] to the triangle T in rows m2 .. 2 m2 + 1 of G2; the stack kernel sees a "fill" of m2 + 1 rows
            F = lm["F"]
            capi.check(L.qrk_bd_lm_panel(left._plan, left._r.data_ptr(), left._perm.data_ptr(), d.data_ptr() if d is not None else None,
                                         par, W.data_ptr(), rows, m2 + 1, colidx.data_ptr(), s_vals.data_ptr(), top.data_ptr(), max(m1, 1),
                                         F.data_ptr(), max(m1, 1)), h)
            capi.check(L.qrk_dense_qless_r(h, F.data_ptr(), max(m1, 1), m1, m2 + 1, G.data_ptr() + 8 * m2, ldg, lm["qwork"].data_ptr()), h)
        else:
            capi.check(L.qrk_bd_lm_panel(left._plan, left._r.data_ptr(), left._perm.data_ptr(), d.data_ptr() if d is not None else None,
                                         par, W.data_ptr(), rows, m2 + 1, colidx.data_ptr(), s_vals.data_ptr(), top.data_ptr(), max(m1, 1),
                                         G.data_ptr() + 8 * m2, ldg), h)
        capi.check(L.qrk_dense_lm_stack(h, W.data_ptr() + 8 * m1, rows, m2, W.data_ptr() + 8 * (m2 * rows + m1),
                                        d[m1:].data_ptr() if d is not None else None, p2.data_ptr(), par, m2 + 1 if reduced else m1,
                                        G.data_ptr(), ldg), h)
        dense = lm["dense"].compute(G[:, :m2])
        dense.applyQ(G[:, m2:], transpose=True)
        z2 = dense.solveR(G[:m2, m2].clone().reshape(m2, 1))
        rhs1 = top[:, m2].clone().reshape(m1, 1)
        capi.check(L.qrk_dense_gemv_sub(h, top.data_ptr(), max(m1, 1), m1, m2, None, z2.data_ptr(), rhs1.data_ptr()), h)
        z1 = torch.empty_like(rhs1)
        capi.check(L.qrk_bd_solve_r(left._plan, s_vals.data_ptr(), rhs1.data_ptr(), 1, z1.data_ptr(), capi.MEM_DEVICE), h)
        x = torch.empty(m1 + m2, dtype=torch.float64, device=dev)
        pc = self.m_outputPerm_c.long()
        zz = torch.cat([z1.reshape(-1), z2.reshape(-1)])
        x[pc] = zz
        if not transposed:
            return x, None
        u = zz * d[pc] ** 2 if d is not None else zz                 # (contiguous: u1 = its first m1 entries, u2 the rest)
        w1, t2, sums2, work = lm["w1"], lm["t2"], lm["sums2"], lm["work"]
        capi.check(L.qrk_bd_solve_rt(left._plan, s_vals.data_ptr(), u.data_ptr(), w1.data_ptr(), sums2.data_ptr()), h)
        capi.check(L.qrk_dense_gemv_t(h, top.data_ptr(), max(m1, 1), m1, m2, None, w1.data_ptr(), -1.0, u.data_ptr() + 8 * m1,
                                      t2.data_ptr(), work.data_ptr()), h)
        capi.check(L.qrk_dense_solve_rt(h, G.data_ptr(), ldg, m2, t2.data_ptr()), h)
        s0 = torch.sum((x * d) ** 2 if d is not None else x ** 2)
        s = torch.cat([s0.reshape(1), sums2, torch.sum(t2[:m2] ** 2).reshape(1)]).cpu().numpy()     # the one read-back
        return x, (float(s[0]), float(s[1]) + float(s[3]), float(s[2]))

    def lmGradient(self, diag=None):
        """(g, gnorm): g = J^T b in J's column order and gnorm = || D^-1 g ||, from the UNDAMPED kept factors (what lmpar's upper
        bound needs): g = P R^^T y with R^ = [R1 Strip(:, P2); 0 R2] and y = Q^T b, so g1 = R1^T y1 (qrk_bd_lm_gradient on the left
        plan) and g2 = Strip(:, P2)^T y1 + R2^T y2 (qrk_dense_gemv_t on W's strip, qrk_dense_trmv_t on R2).  diag as for lmSolve().
        g is numpy or a tensor as `b` was given to factorizeAndSolve(); gnorm is a float."""
        self._lm_require("lmGradient()")
        g, gnorm2 = self._lm_gradient(self._lm_diag(diag))
        return (g.cpu().numpy() if self._lm_np else g), float(np.sqrt(gnorm2))

    def _lm_gradient(self, d):
        dev = self._ctx.device
        m1, m2, rows, W = self._m1, self._m2, self._rows, self._W
        left = self.m_leftSolver
        lm = self._lm_transposed_arrays()
        L, h = capi.lib(), self._ctx.handle
        self._ctx.use_current_stream()
        y1 = W.data_ptr() + 8 * m2 * rows                   # y = Q^T b = W(:, m2); R2 = the upper triangle of W(m1:, 0:m2)
        g = torch.empty(m1 + m2, dtype=torch.float64, device=dev)
        g2 = torch.empty(max(m2, 1), dtype=torch.float64, device=dev)
        n2 = torch.empty(1, dtype=torch.float64, device=dev)
        capi.check(L.qrk_bd_lm_gradient(left._plan, left._r.data_ptr(), left._perm.data_ptr(), y1, d.data_ptr() if d is not None else None,
                                        g.data_ptr(), n2.data_ptr(), capi.MEM_DEVICE), h)
        p2 = self.m_rightSolver.colsPermutation()
        capi.check(L.qrk_dense_gemv_t(h, W.data_ptr(), rows, m1, m2, p2.data_ptr(), y1, 1.0, None, g2.data_ptr(), lm["work"].data_ptr()), h)
        capi.check(L.qrk_dense_trmv_t(h, W.data_ptr() + 8 * m1, rows, m2, y1 + 8 * m1, g2.data_ptr()), h)
        g[m1 + self._P2] = g2[:m2]
        q2 = g[m1:] / d[m1:] if d is not None else g[m1:]
        gnorm2 = float((n2[0] + torch.sum(q2 ** 2)).item())
        return g, gnorm2

    def lmpar(self, diag, delta: float, par: float = 0.0, returnTrace: bool = False):
        """MINPACK's lmpar on the kept factors (what Eigen::LevenbergMarquardt calls between two factorisations,
        examples/ellipse_fitting.cpp:257-280): finds par with | || D x || - delta | <= 0.1 delta, or par = 0 when the Gauss-Newton
        step is inside the region.  A host loop: every evaluation is lmSolve()'s chain and the transposed pass behind it
        (_lm_evaluate) with one read-back of the sums, the scalar rule is qrk_lmpar_begin / qrk_lmpar_next (steps 1-5 of
        qrk_bd_lmpar, include/qrkit_amd.h), the gradient of the upper bound is lmGradient()'s.  At most 11 evaluations.

        diag as for lmSolve(); delta > 0; par >= 0 is the start value.  Returns (x, par, iters), x as lmSolve(diag, par) returns
        it -- the same bits --, and with returnTrace also the (iters + 1) x 3 array of (par, || D x ||^2, || S^-T D^2 z ||^2) per
        evaluation.  Rank-deficient undamped factors are not handled: a zero on the diagonal at par = 0 raises."""
        self._lm_require("lmpar()")
        delta, par = float(delta), float(par)
        if not delta > 0.0:
            raise ValueError("lmpar(): delta must be > 0")
        if not par >= 0.0:
            raise ValueError("lmpar(): par must be >= 0")
        d = self._lm_diag(diag)
        L = capi.lib()
        x, (s0, s1, zeros) = self._lm_evaluate(d, 0.0, True)
        if zeros > 0 or not np.isfinite(s1):
            raise RuntimeError("lmpar(): the undamped factors have a zero on the diagonal (rank-deficient J is not supported)")
        _, gnorm2 = self._lm_gradient(d)
        st = capi.LmparState()
        rc = L.qrk_lmpar_begin(C.byref(st), delta, par, s0, s1, 0.0, gnorm2)
        while rc == 1:
            x, (s0, s1, _) = self._lm_evaluate(d, st.par, True)
            rc = L.qrk_lmpar_next(C.byref(st), s0, s1)
        if rc != 0:
            raise RuntimeError("lmpar(): the scalar rule refused its arguments")
        xo = x.cpu().numpy() if self._lm_np else x
        out = (xo, float(st.par), int(st.iters))
        if returnTrace:
            out += (np.array(st.trace[:3 * (st.iters + 1)], dtype=np.float64).reshape(-1, 3),)
        return out

    def _need_q(self, what: str):
        if self._qless:
            raise RuntimeError(f"{what}: factorised without Q (factorizeAndSolve); call factorize() or compute() for the explicit Q")

    def analyzePattern(self, mat: BlockMatrix1x2):
        """:431-449: identity permutations, left block size."""
        left, right = mat.leftBlock(), mat.rightBlock()
        assert left.cols() > right.shape[1], "the left block should be the bigger one"
        assert left.rows() <= right.shape[0]
        self.m_leftRows, self.m_leftCols = left.rows(), left.cols()
        self._rows, self._cols = mat.rows(), mat.cols()

    def factorize(self, mat: BlockMatrix1x2):
        dev = self._ctx.device
        left, right = mat.leftBlock(), mat.rightBlock()
        m1, n1 = self.m_leftCols, self.m_leftRows
        m2 = int(right.shape[1])
        n2 = int(right.shape[0]) - n1
        self._qless = False
        self._lm_ready = False
        # J1 = Q1 R1 (:472-475)
        self.m_leftSolver.compute(left)
        assert self.m_leftSolver.info() == capi.INFO_SUCCESS
        # solveRightBlock (:361-369): J2.top(n1) = Q1^T (rowPerm * J2.top(n1)); bottom n2 rows as they are;
        # rightSolver.compute(J2.bottomRows(n1 + n2 - m1)).  The left solver's row permutation is the identity.
        if hasattr(right, "tocsc"):          # sparse right block (test/test-qrkit.cpp:335): only its nonzeros cross PCIe
            J2 = sparse_to_device_dense(self._ctx, right)
        else:
            J2 = torch.as_tensor(np.asarray(right, dtype=np.float64)) if not isinstance(right, torch.Tensor) else right
            J2 = J2.to(dev, torch.float64)
        top = self.m_leftSolver.applyQt(J2[:n1, :])                    # device, (n1, m2)
        self._J2 = torch.cat([top, J2[n1:, :]], dim=0) if n2 > 0 else top
        bottom = torch.empty((m2, self._J2.shape[0] - m1), dtype=torch.float64, device=dev).t()    # column-major, one strided copy
        bottom.copy_(self._J2[m1:, :])
        self.m_rightSolver.compute(bottom)
        self._P2 = self.m_rightSolver.colsPermutation().long()
        self._m1, self._m2, self._n1, self._n2 = m1, m2, n1, n2
        # column permutation (:498-503) and rank (:510)
        p1 = torch.as_tensor(self.m_leftSolver.colsPermutation(), device=dev).long()
        self.m_outputPerm_c = torch.cat([p1, m1 + self._P2]).to(torch.int32)
        self.m_rowPerm = np.arange(self._rows, dtype=np.int32)
        self.m_nonzeropivots = self.m_leftSolver.rank() + min(bottom.shape)
        self.m_isInitialized = True
        self.m_info = capi.INFO_SUCCESS

    # -- accessors ----------------------------------------------------------------------------
    def rows(self):
        return self._rows

    def cols(self):
        return self._cols

    def rank(self):
        return self.m_nonzeropivots

    def info(self):
        return self.m_info

    def colsPermutation(self) -> np.ndarray:
        return self.m_outputPerm_c.cpu().numpy()

    def rowsPermutation(self) -> np.ndarray:
        return self.m_rowPerm

    def matrixR(self):
        """makeR (:285-308): R = [R1, (Q1^T J2)(0:m1, P2); 0, R2] as scipy CSC (rows x cols)."""
        import scipy.sparse as sp
        m1, m2 = self._m1, self._m2
        R1 = self.m_leftSolver.matrixR()[:, :]                            # (n1 x m1) CSC, nonzero in the top m1 rows
        strip = self._J2[:m1, :][:, self._P2].cpu().numpy()              # J2(r, P2(c)) for r < m1
        R2 = self.m_rightSolver.matrixR().cpu().numpy()                  # (min x m2)
        k2 = R2.shape[0]
        top = sp.hstack([R1[:m1, :], sp.csc_matrix(strip)], format="csc")
        mid = sp.hstack([sp.csc_matrix((k2, m1)), sp.csc_matrix(np.triu(R2))], format="csc")
        pad = sp.csc_matrix((self._rows - m1 - k2, m1 + m2))
        return sp.vstack([top, mid, pad], format="csc")

    def applyQt(self, v):
        """matrixQ().transpose() * v (:607-625): top n1 rows <- Q1^T v_top, then rows m1.. <- Q2^T of them."""
        self._need_q("applyQt()")
        was_np = not isinstance(v, torch.Tensor)
        t = torch.as_tensor(np.asarray(v, dtype=np.float64)) if was_np else v
        t = t.to(self._ctx.device, torch.float64).reshape(self._rows, -1).clone()
        n1, m1 = self._n1, self._m1
        t[:n1, :] = self.m_leftSolver.applyQt(t[:n1, :].contiguous())
        bot = _colmajor(t[m1:, :].clone())
        self.m_rightSolver.applyQ(bot, transpose=True)
        t[m1:, :] = bot
        out = t if np.ndim(v) > 1 else t[:, 0]
        return out.cpu().numpy() if was_np else out

    def applyQ(self, v):
        """matrixQ() * v (:627-645): rows m1.. <- Q2 of them, then the top n1 rows <- Q1 of them."""
        self._need_q("applyQ()")
        was_np = not isinstance(v, torch.Tensor)
        t = torch.as_tensor(np.asarray(v, dtype=np.float64)) if was_np else v
        t = t.to(self._ctx.device, torch.float64).reshape(self._rows, -1).clone()
        n1, m1 = self._n1, self._m1
        bot = _colmajor(t[m1:, :].clone())
        self.m_rightSolver.applyQ(bot, transpose=False)
        t[m1:, :] = bot
        t[:n1, :] = self.m_leftSolver.applyQ(t[:n1, :].contiguous())
        out = t if np.ndim(v) > 1 else t[:, 0]
        return out.cpu().numpy() if was_np else out

    def matrixQ(self):
        """Product expression (BlockAngularSparseQR.h:651-701): matrixQ() @ v, .transpose() @ v, .toSparse()."""
        from .qproduct import QProduct
        self._need_q("matrixQ()")
        return QProduct(self)

    def solve(self, b):
        """_solve_impl (:202-227): x = P [R(0:rank,0:rank)^-1 (Q^T b)(0:rank)] (dense back substitution on the host
        side of the mirror is avoided: the triangular solve uses the block structure on the device)."""
        self._need_q("solve()")
        was_np = not isinstance(b, torch.Tensor)
        y = self.applyQt(torch.as_tensor(np.asarray(b, dtype=np.float64)) if was_np else b)
        y = y.reshape(self._rows, -1)
        m1, m2 = self._m1, self._m2
        y2 = self.m_rightSolver.solveR(_colmajor(y[m1:m1 + m2, :].clone()))       # R2^-1 y2 on the device (qrk_dense_solve_r)
        # y1 -= S(:, P2) z2 with the strip S = (Q1^T J2)(0:m1, :) as it lies on the device (qrk_dense_gemv_sub, one column at a time:
        # the kernel reads the strip once per right-hand side), not a library GEMM on a permuted copy
        rhs1 = _colmajor(y[:m1, :].clone())
        strip = self._J2[:m1, :]
        if not strip.t().is_contiguous():
            strip = _colmajor(strip)
        p2 = self._P2.to(torch.int32).contiguous()
        self._ctx.use_current_stream()
        for k in range(rhs1.shape[1]):
            capi.check(capi.lib().qrk_dense_gemv_sub(self._ctx.handle, strip.data_ptr(), strip.stride(1), m1, m2, p2.data_ptr(),
                                                     y2[:, k].contiguous().data_ptr(), rhs1[:, k].data_ptr()), self._ctx.handle)
        # R1 is block upper triangular: solve it tile by tile with the left solver's packed R
        y1 = self.m_leftSolver.solveR(rhs1)
        yy = torch.cat([y1, y2], dim=0)
        x = torch.empty_like(yy)
        x[self.m_outputPerm_c.long(), :] = yy
        x = x if np.ndim(b) > 1 else x[:, 0]
        return x.cpu().numpy() if was_np else x
