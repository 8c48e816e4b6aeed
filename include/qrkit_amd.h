/*
 * qrkit_amd.h -- C ABI of the MI355X (gfx950) structured sparse QR engine.
 *
 * This is the drop-in boundary for QRKit's block-diagonal hot path.  QRKit has
 * no FFI of its own (header-only C++ templates); the seam these entry points
 * replace is the body of
 *     QRKit::BlockDiagonalSparseQR<BlockQRSolver,QFormat>::analyzePattern
 *         (src/QRKit/BlockDiagonalSparseQR.h:392-405)
 *     QRKit::BlockDiagonalSparseQR<...>::factorize   (:415-547)
 *     QRKit::BlockDiagonalSparseQR<...>::_solve_impl (:257-280)
 * i.e. everything between "tiles of a SparseBlockDiagonal in" and
 * "values of m_Q / m_R / m_outputPerm_c out".  The C++ facade in
 * include/qrkit/ keeps the reference's class and method names on top of it;
 * INTEGRATION.md shows the binding a QRKit maintainer would add.
 *
 * Conventions
 *  - plain C types only; the caller owns every buffer; the library never frees
 *    or retains caller memory beyond the call (device work is enqueued on the
 *    handle's HIP stream and has completed when the stream has);
 *  - all matrices are double, tiles column-major (Eigen::Matrix default);
 *  - index arrays are int32 (QRKit's StorageIndex = int);
 *  - one handle per host thread (no internal locking);
 *  - every function returns qrk_status; qrk_last_error() gives the text;
 *  - there is NO CPU fallback: without a HIP device qrk_create() fails with
 *    QRK_STATUS_NO_DEVICE and nothing else can be called.
 */
#ifndef QRKIT_AMD_H
#define QRKIT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QRK_VERSION_MAJOR 0
#define QRK_VERSION_MINOR 1

typedef enum qrk_status {
    QRK_STATUS_OK = 0,
    QRK_STATUS_INVALID_ARGUMENT = 1,
    QRK_STATUS_NO_DEVICE = 2,
    QRK_STATUS_HIP_ERROR = 3,
    QRK_STATUS_ALLOC_FAILED = 4,
    QRK_STATUS_UNSUPPORTED = 5,
    QRK_STATUS_NOT_FACTORIZED = 6
} qrk_status;

/* Eigen::ComputationInfo, as returned by QRKit's info() (BlockDiagonalSparseQR.h:309-313). */
typedef enum qrk_info {
    QRK_INFO_SUCCESS = 0,
    QRK_INFO_NUMERICAL_ISSUE = 1,
    QRK_INFO_NO_CONVERGENCE = 2,
    QRK_INFO_INVALID_INPUT = 3
} qrk_info;

/* BlockDiagonalSparseQR::MatrixQFormat (BlockDiagonalSparseQR.h:59-62). */
typedef enum qrk_q_format { QRK_FULL_Q = 0, QRK_BLOCK_DIAGONAL_Q = 1 } qrk_q_format;

/* Which Eigen dense solver stands behind the _BlockQRSolver template parameter
 * (BlockDiagonalSparseQR.h:37): ColPivHouseholderQR (test/test-qrkit.cpp:32-38,
 * 49-51) or HouseholderQR (examples/ellipse_fitting.cpp:153). */
typedef enum qrk_block_solver { QRK_COLPIV_HOUSEHOLDER = 0, QRK_HOUSEHOLDER = 1 } qrk_block_solver;

/* Where the caller's buffers live. */
typedef enum qrk_memspace { QRK_MEM_DEVICE = 0, QRK_MEM_HOST = 1 } qrk_memspace;

typedef struct qrk_context_s* qrk_handle;
typedef struct qrk_bd_plan_s* qrk_bd_plan;

/* ------------------------------------------------------------------ context */

/* Library version as major*1000+minor. */
int qrk_version(void);

/* Number of HIP devices visible (0 when there is none; never initialises a context). */
int qrk_device_count(void);

/* Create a context on HIP device `device`.  `stream` is a hipStream_t (or NULL
 * for the device's default stream) on which all work of this handle is enqueued. */
qrk_status qrk_create(qrk_handle* out, int device, void* stream);
qrk_status qrk_destroy(qrk_handle h);
qrk_status qrk_set_stream(qrk_handle h, void* stream);
/* Block until everything enqueued on the handle's stream has finished. */
qrk_status qrk_synchronize(qrk_handle h);
/* Text of the last error on this handle (h may be NULL for creation errors). */
const char* qrk_last_error(qrk_handle h);

/* ------------------------------------------------------- device memory helpers */

/* For callers without a HIP toolchain of their own (the C++ facade in include/qrkit/QRKit.hpp keeps the
 * factors on the device between factorize() and solve() with these): plain device memory on the
 * context's device, and copies ordered on the context's stream that return when the data has arrived.
 * direction: 0 = host -> device, 1 = device -> host. */
qrk_status qrk_device_alloc(qrk_handle h, int64_t bytes, void** out);
qrk_status qrk_device_free(qrk_handle h, void* ptr);
qrk_status qrk_memcpy(qrk_handle h, void* dst, const void* src, int64_t bytes, int direction);
/* `height` runs of `width_bytes` bytes, `dst_pitch` / `src_pitch` bytes apart (a block of columns of a column-major matrix, e.g.
 * the top or bottom rows of the dense right block J2, BlockAngularSparseQR.h:361-369).  direction: 0 = host -> device,
 * 1 = device -> host, 2 = device -> device. */
qrk_status qrk_memcpy_2d(qrk_handle h, void* dst, int64_t dst_pitch, const void* src, int64_t src_pitch, int64_t width_bytes,
                         int64_t height, int direction);

/* Dense column-major copy of the row window [row0, row0 + nrows) of a compressed sparse matrix whose arrays are on the device
 * (CSR when row_major != 0, else CSC; Eigen's outerIndexPtr / innerIndexPtr / valuePtr of a compressed matrix):
 * d_out[c * ld + (d_row_map ? d_row_map[r - row0] : r - row0)] = value of entry (r, c); every other element of the nrows x cols
 * window is zero.  d_row_map (device, nrows entries, a permutation of 0..nrows-1) or NULL.  Replaces the dense copy the
 * reference makes of a sparse right block - BlockedThinSparseQR::compute, BlockedThinSparseQR.h:131 "m_R = mat", reached from
 * BlockAngularSparseQR::solveRightBlock (BlockAngularSparseQR.h:361-369) - so that a sparse J2 crosses PCIe as its nonzeros. */
qrk_status qrk_sparse_window_to_dense(qrk_handle h, int row_major, int64_t rows, int64_t cols, const int32_t* d_outer,
                                      const int32_t* d_inner, const double* d_values, int64_t row0, int64_t nrows,
                                      const int32_t* d_row_map, double* d_out, int64_t ld);

/* -------------------------------------------- block-diagonal: analyzePattern */

/* The block structure of a QRKit::SparseBlockDiagonal (SparseBlockDiagonal.h:43-163):
 * num_blocks dense tiles on the diagonal, tile i being rows[i] x cols[i].  When
 * rows == cols == NULL every tile is block_rows x block_cols (the
 * fromBlockDiagonalPattern case, SparseBlockDiagonal.h:71-89).  mat_rows /
 * mat_cols are SparseBlockDiagonal::rows()/cols(); mat_rows may exceed the sum
 * of tile rows (trailing identity rows of Q, BlockDiagonalSparseQR.h:530-533);
 * mat_cols must equal the sum of tile cols.  rows/cols are HOST arrays. */
typedef struct qrk_bd_layout {
    int64_t num_blocks;
    int32_t block_rows;
    int32_t block_cols;
    const int32_t* rows;
    const int32_t* cols;
    int32_t mat_rows;
    int32_t mat_cols;
} qrk_bd_layout;

/* analyzePattern(): validates the layout, computes the prefix sums the hot loop
 * carries (base_row, base_col, m1; BlockDiagonalSparseQR.h:428-431,524-525),
 * uploads the per-tile descriptors and bins tiles by size class.  A landscape
 * tile (rows < cols) is accepted here and reported by factorize() through
 * info = QRK_INFO_INVALID_INPUT, as the reference does (:509-516). */
qrk_status qrk_bd_plan_create(qrk_handle h, const qrk_bd_layout* layout, qrk_q_format q_format,
                              qrk_block_solver solver, qrk_bd_plan* out);
qrk_status qrk_bd_plan_destroy(qrk_bd_plan plan);

/* Element counts of the caller-owned arrays:
 *   tiles_len = sum rows_i*cols_i          (input tiles, packed back to back)
 *   nnz_q     = sum rows_i^2 + (mat_rows - sum rows_i)   (m_Q values / column indices)
 *   nnz_r     = sum cols_i*(cols_i+1)/2    (m_R values / row indices)
 * perm and hcoeffs have mat_cols entries. */
qrk_status qrk_bd_plan_sizes(qrk_bd_plan plan, int64_t* tiles_len, int64_t* nnz_q, int64_t* nnz_r);

/* Sparse patterns exactly as factorize() assembles them: m_Q is RowMajor CSR
 * (mat_rows+1 row pointers, nnz_q column indices; BlockDiagonalSparseQR.h:455-492,
 * 530-536), m_R is ColMajor CSC (mat_cols+1 column pointers, nnz_r row indices;
 * :475-479,496-500,538-541).  Pure functions of the layout and q_format. */
qrk_status qrk_bd_pattern(qrk_bd_plan plan, int32_t* q_rowptr, int32_t* q_colidx, int32_t* r_colptr,
                          int32_t* r_rowidx, qrk_memspace space);

/* ------------------------------------------- block-diagonal: cutting the tiles */

/* SparseBlockDiagonal::fromBlockDiagonalPattern (SparseBlockDiagonal.h:71-89): tile i =
 * dense copy of mat.block(base_row_i, base_col_i, rows_i, cols_i), the block map being
 * BlockBandedMatrixInfo::fromBlockDiagonalPattern (SparseQRUtils.h:255-272; base_row / base_col
 * are the running sums of the plan's layout, = i*blockRows / i*blockCols for equal blocks).
 * `mat` is a compressed sparse matrix with int32 indices: column-major (CSC: mat_cols+1 outer
 * pointers, row indices) when row_major == 0, row-major (CSR: mat_rows+1 outer pointers, column
 * indices) otherwise.  Entries of `mat` outside the blocks are ignored, as block() ignores them.
 *   tiles [tiles_len] out: tile i column-major at the running offset (the input of qrk_bd_factorize) */
qrk_status qrk_bd_tiles_from_sparse(qrk_bd_plan plan, int row_major, const int32_t* outer_ptr,
                                    const int32_t* inner_idx, const double* vals, int64_t nnz, double* tiles,
                                    qrk_memspace space);

/* ------------------------------------------------- block-diagonal: factorize */

/* factorize(): per tile A_i P_i = Q_i R_i (BlockDiagonalSparseQR.h:432-526).
 *   tiles   [tiles_len]  in : tile i column-major at the running offset
 *   q_vals  [nnz_q]      out: values of m_Q in CSR order (row j of Q_i = [U_i(j,:), N_i(j,:)])
 *   r_vals  [nnz_r]      out: values of m_R in CSC order (upper triangle of R_i by columns)
 *   perm    [mat_cols]   out: m_outputPerm_c.indices() (:519-521)
 *   hcoeffs [mat_cols]   out, may be NULL: Householder coefficients tau of every tile
 * Asynchronous on the handle's stream for QRK_MEM_DEVICE; for QRK_MEM_HOST the
 * call stages through device buffers and returns after the results are on the host. */
qrk_status qrk_bd_factorize(qrk_bd_plan plan, const double* tiles, double* q_vals, double* r_vals,
                            int32_t* perm, double* hcoeffs, qrk_memspace space);

/* info() and rank() after factorize() (BlockDiagonalSparseQR.h:161-165,309-313):
 * rank = sum of tile cols (the solver is not rank revealing, :439-444). */
qrk_status qrk_bd_info(qrk_bd_plan plan, qrk_info* info, int64_t* rank);

/* ----------------------------------------------------- block-diagonal: solve */

/* y = Q^T b, the product the reference forms at BlockDiagonalSparseQR.h:266 and the
 * tests at test/test-qrkit.cpp:187.  b, y: mat_rows x nrhs column-major (ld = mat_rows). */
qrk_status qrk_bd_apply_qt(qrk_bd_plan plan, const double* q_vals, const double* b, int64_t nrhs,
                           double* y, qrk_memspace space);

/* y = Q b, matrixQ() * b with the explicit m_Q (BlockDiagonalSparseQR.h:235-237; the reference forms this
 * product as a sparse matrix-vector product, e.g. test/test-qrkit.cpp:201 and BlockAngularSparseQR.h:627-645).
 * b, y: nrhs columns of mat_rows entries; b and y must not alias. */
qrk_status qrk_bd_apply_q(qrk_bd_plan plan, const double* q_vals, const double* b, int64_t nrhs,
                          double* y, qrk_memspace space);

/* _solve_impl (BlockDiagonalSparseQR.h:257-280), FullQ only:
 * x = P * [ R(0:rank,0:rank)^-1 (Q^T b)(0:rank) ];  b: mat_rows x nrhs, x: mat_cols x nrhs. */
qrk_status qrk_bd_solve(qrk_bd_plan plan, const double* q_vals, const double* r_vals,
                        const int32_t* perm, const double* b, int64_t nrhs, double* x,
                        qrk_memspace space);

/* The triangular step of _solve_impl alone (BlockDiagonalSparseQR.h:271):
 * z = R(0:cols,0:cols).triangularView<Upper>().solve(y);  y, z: mat_cols x nrhs.  Used by the angular
 * composition, whose R = [R1, S; 0, R2] is solved block by block. */
qrk_status qrk_bd_solve_r(qrk_bd_plan plan, const double* r_vals, const double* y, int64_t nrhs, double* z,
                          qrk_memspace space);

/* factorize() + the Q^T b and back substitution of _solve_impl (BlockDiagonalSparseQR.h:257-280) in one pass, Q never
 * formed in device memory: what a Levenberg-Marquardt caller needs every iteration (R, the column permutation, Q^T f;
 * examples/ellipse_fitting.cpp:126-142).
 *   tiles   [tiles_len]         in : as qrk_bd_factorize
 *   b       [mat_rows x nrhs]   in : column-major, ld = mat_rows
 *   r_vals, perm, hcoeffs       out: what qrk_bd_factorize writes for this plan (hcoeffs may be NULL)
 *   qtb     [mat_rows x nrhs]   out, may be NULL: what qrk_bd_apply_qt gives (the plan's Q format decides the row order:
 *                                    FullQ [U.. | N..]); trailing identity rows copy b.  Must not overlap b.
 *   x       [mat_cols x nrhs]   out, may be NULL: what qrk_bd_solve gives (FullQ plans only: QRK_STATUS_UNSUPPORTED otherwise)
 * At least one of qtb / x must be given.  qrk_bd_info afterwards as after qrk_bd_factorize.
 * Uniform plans of tiles with 1 or 2 columns and at most 16 rows (up to 4 right-hand sides) and uniform 32 x 32 plans
 * (up to 32 right-hand sides, 16-byte aligned arrays) run kernels that never form Q; every other plan factorizes into a
 * Q scratch owned by the plan (nnz_q doubles, allocated by the first such call: QRK_STATUS_ALLOC_FAILED if that fails)
 * and applies it.  QRK_MEM_DEVICE: enqueued on the handle's stream; QRK_MEM_HOST: staged like qrk_bd_factorize. */
qrk_status qrk_bd_factorize_rhs(qrk_bd_plan plan, const double* tiles, const double* b, int64_t nrhs,
                                double* r_vals, int32_t* perm, double* hcoeffs, double* qtb, double* x,
                                qrk_memspace space);

/* Name of the kernel qrk_bd_factorize_rhs runs on this plan for nrhs right-hand sides (aligned arrays), or a string
 * that contains "fallback" when the plan takes the explicit-Q route.  The pointer is static, like qrk_bd_kernel_name. */
const char* qrk_bd_rhs_kernel_name(qrk_bd_plan plan, int64_t nrhs);

/* factorize() and Q^T C for a panel C of ncols columns, Q never formed in device memory on the thin route: the left half
 * of BlockAngularSparseQR::factorize (BlockAngularSparseQR.h:459-514), the panel being J2's top rows with the right-hand
 * side of a Levenberg-Marquardt step as one more column.
 *   c    [ (ncols-1)*ldc + mat_rows ]  in : column j at c + j*ldc, ldc >= mat_rows
 *   qtc  [ (ncols-1)*ldq + mat_rows ]  out: column j at qtc + j*ldq, ldq >= mat_rows; rows in the plan's Q-format order
 *                                           exactly as qrk_bd_apply_qt orders them (FullQ: [U.. | N.. | trailing identity
 *                                           rows copy c]); rows mat_rows..ldq of a column are not touched.
 *                                           The spans of c and qtc must not overlap.
 *   r_vals, perm, hcoeffs              out: what qrk_bd_factorize writes for this plan (hcoeffs may be NULL)
 * ncols >= 0 (0: the factors only).  qrk_bd_info afterwards as after qrk_bd_factorize; landscape plans as there.
 * Uniform plans of tiles with 1 or 2 columns and at most 16 rows run one kernel that never forms Q, for a panel of any
 * width (bdqr_thin_panel.hip); every other plan, and any plan under QRK_EXACT=1 or QRK_THIN=0, factorizes into the Q
 * scratch owned by the plan (nnz_q doubles, allocated by the first such call) and applies it with qrk_bd_apply_qt's
 * kernels striding by ldc / ldq.  QRK_MEM_DEVICE: enqueued on the handle's stream, no host synchronisation;
 * QRK_MEM_HOST: staged like qrk_bd_factorize_rhs. */
qrk_status qrk_bd_factorize_apply_qt(qrk_bd_plan plan, const double* tiles, const double* c, int64_t ldc, int64_t ncols,
                                     double* r_vals, int32_t* perm, double* hcoeffs, double* qtc, int64_t ldq,
                                     qrk_memspace space);

/* Name of the kernel qrk_bd_factorize_apply_qt runs on this plan for a panel of ncols columns, or a string that contains
 * "fallback" on the explicit-Q route.  The pointer is static, like qrk_bd_kernel_name. */
const char* qrk_bd_panel_kernel_name(qrk_bd_plan plan, int64_t ncols);

/* ------------------------------------ block-diagonal: the Levenberg-Marquardt step on the factors */

/* What Eigen::LevenbergMarquardt does between two factorisations (examples/ellipse_fitting.cpp:257-280,
 * bench/bench_sparse_qr_extra.cpp:303-346): MINPACK's lmpar on matrixR(), colsPermutation() and Q^T f -- no tile, no Q, no
 * reflector is read, so these work after qrk_bd_factorize_rhs / qrk_bd_factorize_apply_qt as after qrk_bd_factorize.  Common arguments:
 *   r_vals [nnz_r], perm [mat_cols]  in : as qrk_bd_factorize wrote them (perm holds global column indices); the arrays are the
 *                                         caller's, the plan's factorised state is not consulted
 *   y      [mat_cols]                in : the first mat_cols entries of Q^T b in FullQ order (qtb[0:mat_cols] of
 *                                         qrk_bd_factorize_rhs; what qrk_bd_apply_qt gives): tile t's entries at its base_col
 *   diag   [mat_cols]                in : positive scale factors in the matrix's own column order; NULL = all ones
 * FullQ plans whose tiles have at most 32 columns; otherwise QRK_STATUS_UNSUPPORTED (BlockDiagonalQ as qrk_bd_solve).  The first
 * three are enqueue-only for QRK_MEM_DEVICE (no host synchronisation; par travels as a kernel argument) and stage like qrk_bd_solve
 * for QRK_MEM_HOST.  Every sum is formed in a fixed order (one partial per workgroup in a scratch the plan owns -- allocated by the
 * first call that asks for a sum, QRK_STATUS_ALLOC_FAILED if that fails -- then one workgroup over the partials; no floating-point
 * atomics; the grid depends on the plan alone): two identical calls give identical bits. */

/* The damped solve of MINPACK's qrsolv, tile by tile: x = argmin || R P^T x - y ||^2 + par || D x ||^2, par >= 0.  In the pivoted
 * order of a tile, with Dt = D permuted: z = argmin || R_t z - y_t ||^2 + par || Dt z ||^2, x[perm[base_col + k]] = z_k.
 *   sums[0] = || D x ||^2
 *   sums[1] = sum over the tiles of || S_t^-T (Dt^2 z) ||^2, S_t^T S_t = R_t^T R_t + par Dt^2 (the derivative lmpar's Newton step needs)
 *   sums[2] = number of tiles with an exact zero on R's diagonal
 * sums (3 doubles) may be NULL.  A tile whose S has its first exact zero diagonal entry at k0 (par = 0: S = R) gets z_k = 0 for
 * k >= k0 and the solution of the leading k0 x k0 block -- MINPACK's nsing rule per tile -- and adds nothing to sums[1]. */
qrk_status qrk_bd_lm_solve(qrk_bd_plan plan, const double* r_vals, const int32_t* perm, const double* y, const double* diag,
                           double par, double* x, double* sums, qrk_memspace space);

/* g = P R^T y = J^T f in the matrix's column order, g[perm[base_col + k]] = sum_{i <= k} R(i, k) y_i, and *gnorm2 =
 * sum (g_j / diag_j)^2 (lmpar's upper bound is sqrt(gnorm2) / delta).  g [mat_cols] or gnorm2 may be NULL, not both. */
qrk_status qrk_bd_lm_gradient(qrk_bd_plan plan, const double* r_vals, const int32_t* perm, const double* y, const double* diag,
                              double* g, double* gnorm2, qrk_memspace space);

/* norms[perm[base_col + k]] = || R_t(0:k, k) || = the norm of column perm[base_col + k] of J: the diag an LM driver starts from
 * (LevenbergMarquardt::minimizeInit takes them from colsPermutation() and matrixR()).  An exact zero is written as zero; the
 * caller decides what to put in its place. */
qrk_status qrk_bd_r_col_norms(qrk_bd_plan plan, const double* r_vals, const int32_t* perm, double* norms, qrk_memspace space);

/* MINPACK's lmpar (what LevenbergMarquardt::minimizeOneStep calls for the step, examples/ellipse_fitting.cpp:257-280) run on the
 * host over the calls above: finds par with | || D x || - delta | <= 0.1 delta, or par = 0 when the Gauss-Newton step is inside
 * the region.  DEVICE pointers only (r_vals, perm, y, diag, x); par (in: start value, out: result), iters and trace are HOST.
 * Every evaluation reads the sums back into a pinned buffer of the plan, so the call SYNCHRONISES the handle's stream once per
 * evaluation (at most 11 times) and cannot be captured into a hipGraph (qrk_bd_lmpar_device below can).  x holds the step of the returned par on return.
 *   1  evaluate at par = 0: s = sums; dxnorm = sqrt(s0), fp = dxnorm - delta; fp <= 0.1 delta: par = 0, iters = 0, return
 *   2  parl = 0 if s2 > 0, else fp / (delta s1 / s0)
 *   3  gnorm = sqrt(gnorm2) of qrk_bd_lm_gradient; paru = gnorm / delta; paru = 0: paru = DBL_MIN / min(delta, 0.1)
 *   4  par = min(max(par, parl), paru); par = 0: par = gnorm / dxnorm
 *   5  for iter = 1, 2, ...: par = 0: par = max(DBL_MIN, 0.001 paru); evaluate at par; dxnorm = sqrt(s0), temp = fp,
 *      fp = dxnorm - delta; stop if |fp| <= 0.1 delta, or (parl = 0 and fp <= temp and temp < 0), or iter = 10; else
 *      parc = fp / (delta s1 / s0); fp > 0: parl = max(parl, par); fp < 0: paru = min(paru, par); par = max(parl, par + parc)
 * trace (3 x 11 doubles, may be NULL) receives (par, s0, s1) of every evaluation, the one at par = 0 first; *iters (may be NULL) =
 * the number of passes of the loop.  delta > 0, *par >= 0. */
qrk_status qrk_bd_lmpar(qrk_bd_plan plan, const double* r_vals, const int32_t* perm, const double* y, const double* diag,
                        double delta, double* par, double* x, int32_t* iters, double* trace);

/* qrk_bd_lmpar as ONE ENQUEUE: the same steps 1-5 with every stopping rule, the parl / paru bounds, the DBL_MIN cases and the cap of
 * 10 passes, but the scalar part of each step runs in one lane on the device behind the sums of the evaluation.  The call
 * enqueues a fixed chain on the handle's stream -- a memset of a small control block in the plan's scratch, the evaluation at
 * par = 0 with the gradient sum, ten damped evaluations that return at once after the search has stopped -- and returns: no
 * stream synchronisation, no copy to the host, no event query, so it can be captured into a hipGraph and replayed.
 * ALL pointers are DEVICE pointers:
 *   delta          in     : one double, the radius.  In device memory (not a kernel argument) so that a replayed graph sees a new one
 *   par            in/out : one double: the start value on entry, the result once the stream has run the call
 *   x   [mat_cols] out    : the step of the returned par once the stream has run the call
 *   iters          out    : one int32, the number of passes of the loop (0 .. 10); may be NULL
 *   trace [3 x 11] out    : (par, s0, s1) of every evaluation that ran, the one at par = 0 first; the rows of evaluations that did
 *                           not run are zero; may be NULL
 * The values of delta and par can only be checked on the device: if !(*delta > 0) or !(*par >= 0) (NaN included) the call writes
 * *iters = -1, leaves *par as it was, runs no damped evaluation, and x HAS NO MEANING (it holds the undamped solve).  A NULL plan,
 * r_vals, perm, y, delta, par or x is QRK_STATUS_INVALID_ARGUMENT before a device is touched; plan support is that of
 * qrk_bd_lm_solve (QRK_STATUS_UNSUPPORTED otherwise).
 * The only allocation is the plan's scratch of the LM calls, made by the first of them on the plan.  If it does not exist yet and
 * the handle's stream is being captured the call fails with QRK_STATUS_INVALID_ARGUMENT: make one LM call on the plan outside
 * the capture first.  The scratch (the control block included) belongs to the plan: calls on one plan must be ordered on one
 * stream, as for every qrk_bd_lm_* call that asks for a sum.
 * The sums are those of qrk_bd_lm_solve / qrk_bd_lm_gradient (same kernels' arithmetic, same grid, same order) and the scalar
 * steps are the host loop's correctly rounded operations in the same order: par, iters, trace and x are qrk_bd_lmpar's. */
qrk_status qrk_bd_lmpar_device(qrk_bd_plan plan, const double* r_vals, const int32_t* perm, const double* y, const double* diag,
                               const double* delta, double* par, double* x, int32_t* iters, double* trace);

/* Name of the kernel qrk_bd_lm_solve runs on this plan, or a string that contains "unsupported" where it would refuse.  The
 * pointer is static, like qrk_bd_kernel_name. */
const char* qrk_bd_lm_kernel_name(qrk_bd_plan plan);

/* The reflectors of the damped solve applied to a PANEL: the left half of the damped solve on the factors the block-angular solver
 * keeps (BlockAngularSparseQR.h:459-514).  Per tile t (c columns, first column base_col, Dt = diag in the tile's
 * pivoted order) the stack [R_t; sqrt(par) Dt] is triangularised by qrk_bd_lm_solve's reflectors and the same reflectors go over the
 * tile's rows of the panel stacked on c zero rows:
 *     H [R_t  C_t; sqrt(par) Dt  0] = [S_t  top_t; 0  fill_t],     S_t^T S_t = R_t^T R_t + par Dt^2
 * DEVICE pointers only; enqueue-only on the handle's stream: no synchronisation, no allocation.
 *   r_vals, perm, diag                 in  : as for qrk_bd_lm_solve (diag in the matrix's own column order; NULL = all ones)
 *   c, ldc, ncols, colidx              in  : panel column j is c + colidx[j] ldc (c + j ldc when colidx is NULL), mat_cols rows, tile
 *                                            t's rows at its base_col; ldc >= mat_cols; ncols >= 0
 *   s_vals [nnz_r]                     out : the packed S_t in r_vals' layout (what qrk_bd_solve_r takes)
 *   top, ldt / fill, ldf               out : column j at top + j ldt / fill + j ldf, mat_cols rows each (ldt, ldf >= mat_cols); the rows
 *                                            beyond mat_cols of a column are not touched
 * With ncols = 0 only s_vals is written (c, top and fill may be NULL).  Output spans must not overlap the inputs.
 * Plan support is that of qrk_bd_lm_solve (QRK_STATUS_UNSUPPORTED otherwise); a NULL plan / r_vals / perm / s_vals, NULL panel
 * pointers with ncols > 0, par < 0 or NaN are QRK_STATUS_INVALID_ARGUMENT before a device is touched.
 * par = 0 makes every reflector the identity: s_vals = r_vals, top = the gathered panel, fill = +0.0, bit for bit.  No atomics; the
 * grid is a function of the plan and ncols: two identical calls give identical bits. */
qrk_status qrk_bd_lm_panel(qrk_bd_plan plan, const double* r_vals, const int32_t* perm, const double* diag, double par,
                           const double* c, int64_t ldc, int64_t ncols, const int32_t* colidx,
                           double* s_vals, double* top, int64_t ldt, double* fill, int64_t ldf);

/* Name of the kernel qrk_bd_lm_panel runs on this plan, or a string that contains "unsupported" where it would refuse ("" for a
 * NULL plan).  The pointer is static. */
const char* qrk_bd_lm_panel_kernel_name(qrk_bd_plan plan, int64_t ncols);

/* The 2 m2 rows of the right stack G of the block-angular damped solve that qrk_bd_lm_panel does not write.  G is (m2 + m1 + m2) x
 * (m2 + 1), column-major with leading dimension ldg; rows m2 .. m2 + m1 are the panel's fill (qrk_bd_lm_panel writes it there).
 *   rows 0 .. m2        : [triu(qr) | y2] -- qr is the packed QR of the right block (m2 columns, leading dimension lda): the
 *                         reflectors below the diagonal are not copied, the rows below it are zero
 *   rows m2 + m1 ..     : sqrt(par) diag2[perm2[k]] on the diagonal (diag2 NULL = ones, perm2 NULL = identity), zero elsewhere, the
 *                         last column included
 * DEVICE pointers, enqueue-only on the handle's stream.  m2 = 0 writes nothing.
 * The reduced route passes m1 = m2 + 1: qrk_bd_lm_panel writes its fill to a buffer of its own, qrk_dense_qless_r
 * reduces [fill | its right-hand side] to one (m2 + 1) x (m2 + 1) triangle in rows m2 .. 2 m2 + 1 of a (3 m2 + 1) x (m2 + 1) stack,
 * and this call writes the rows around it. */
qrk_status qrk_dense_lm_stack(qrk_handle h, const double* qr, int64_t lda, int32_t m2, const double* y2,
                              const double* diag2, const int32_t* perm2, double par, int64_t m1, double* g, int64_t ldg);

/* ------------------------------------ block-angular: lmpar on the kept factors */

/* In the pivoted order the damped triangular factor of [J1 | J2] is S^ = [S1 Top; 0 Rg]: S1 = the tiles qrk_bd_lm_panel writes to
 * s_vals, Top = top(:, 0:m2), Rg = the upper triangle of the factorised right stack G(0:m2, 0:m2).  One evaluation of lmpar needs
 * s1 = || S^-T u ||^2 with u = D~^2 z (z = the solution in pivoted order), by forward substitution:
 *     w1 = S1^-T u1 (qrk_bd_solve_rt),  w2 = Rg^-T (u2 - Top^T w1) (qrk_dense_gemv_t, qrk_dense_solve_rt),  s1 = |w1|^2 + |w2|^2
 * and once per lmpar the gradient of the undamped factors, g1 = R1^T y1 (qrk_bd_lm_gradient), g2 = Strip(:, P2)^T y1 + R2^T y2
 * (qrk_dense_gemv_t, qrk_dense_trmv_t).  The four calls are DEVICE-pointer, enqueue-only calls on the handle's stream. */

/* Per tile t: w_t = R_t^-T u_t, r_vals in the packed layout of qrk_bd_solve_r (s_vals of qrk_bd_lm_panel is passed here).
 *   u, w [mat_cols]  : tile t's entries at its base_col; distinct arrays
 *   sums2 [2]        : may be NULL.  sums2[0] = || w ||^2, sums2[1] = the number of tiles with an exact zero on the diagonal; such a
 *                      tile gets w_t = 0 and adds nothing to sums2[0]
 * Plan support is that of qrk_bd_lm_solve (QRK_STATUS_UNSUPPORTED otherwise); a NULL plan, r_vals, u or w is
 * QRK_STATUS_INVALID_ARGUMENT before a device is touched.  The sums follow the rule of the qrk_bd_lm_* calls: one partial per workgroup
 * in the plan's LM scratch, one workgroup adds them in a fixed order, no floating-point atomics, the grid depends on the plan alone:
 * two identical calls give identical bits.  If sums2 is given, the scratch does not exist yet and the stream is being captured, the
 * call fails with QRK_STATUS_INVALID_ARGUMENT instead of allocating (as qrk_bd_lmpar_device). */
qrk_status qrk_bd_solve_rt(qrk_bd_plan plan, const double* r_vals, const double* u, double* w, double* sums2);

/* Name of the kernel qrk_bd_solve_rt runs on this plan, or a string that contains "unsupported" where it would refuse ("" for a
 * NULL plan).  The pointer is static. */
const char* qrk_bd_solve_rt_kernel_name(qrk_bd_plan plan);

/* out[j] = alpha sum_{i < rows} A(i, colidx[j]) w[i] + (add ? add[j] : 0) for j < cols: a tall-skinny A^T w read once.  A is
 * column-major with leading dimension lda >= rows; rows rows .. lda of a column are never read; colidx NULL = column j.  alpha is
 * +1 or -1.  rows = 0 gives out = add (0 when add is NULL); cols = 0 writes nothing.  out, add and w are distinct.
 *   work : qrk_dense_gemv_t_work(rows, cols) doubles of the caller's (the call allocates nothing and can be captured): one partial
 *          per chunk of rows and column; a second kernel adds the chunks of a column in a fixed order.
 * No atomics; the grid and the order depend on (rows, cols) alone: two identical calls give identical bits. */
int64_t    qrk_dense_gemv_t_work(int64_t rows, int64_t cols);
qrk_status qrk_dense_gemv_t(qrk_handle h, const double* A, int64_t lda, int64_t rows, int64_t cols, const int32_t* colidx,
                            const double* w, double alpha, const double* add, double* out, double* work);

/* b(0:n) <- R^-T b(0:n), R = the upper triangle of qr (column-major, leading dimension lda >= n): nothing below the diagonal is
 * read (a packed QR keeps reflectors there).  A zero on the diagonal gives non-finite entries.  n = 0 writes nothing. */
qrk_status qrk_dense_solve_rt(qrk_handle h, const double* qr, int64_t lda, int32_t n, double* b);
/* out[j] += sum_{i <= j} R(i, j) y[i] for j < n (out and y distinct), R as above. */
qrk_status qrk_dense_trmv_t(qrk_handle h, const double* qr, int64_t lda, int32_t n, const double* y, double* out);

/* The scalar rule of lmpar -- steps 1-5 of qrk_bd_lmpar above with every stopping rule, the parl / paru bounds, the DBL_MIN cases
 * and the cap of 10 passes, the same correctly rounded operations in the same order -- as a host state machine for a caller that
 * owns the evaluation (the block-angular facades).  No device is touched.
 *   qrk_lmpar_begin : behind the evaluation at par = 0 (s0 = || D x ||^2, s1 = || S^-T D^2 z ||^2, s2 > 0 = a zero on R's
 *                     diagonal, gnorm2 = | D^-1 g |^2).  delta > 0, par0 >= 0.
 *   qrk_lmpar_next  : behind the evaluation at state->par.
 * Both return 1 = evaluate at state->par and call qrk_lmpar_next, 0 = stop: state->par is the result, or -1 for a NULL state,
 * delta <= 0, par0 < 0 or NaN, or a call after the stop.  state->iters = the passes of the loop so far, state->trace = (par, s0, s1)
 * of every evaluation, the one at par = 0 first, the rows of evaluations that did not run zero. */
typedef struct qrk_lmpar_state {
    double par;            /* the par to evaluate next; the result after the stop */
    double delta, parl, paru, fp, gnorm;
    int32_t iters;
    int32_t done;
    double trace[33];
} qrk_lmpar_state;
int qrk_lmpar_begin(qrk_lmpar_state* state, double delta, double par0, double s0, double s1, double s2, double gnorm2);
int qrk_lmpar_next(qrk_lmpar_state* state, double s0, double s1);

/* ------------------------------------ the R factor of a tall-skinny matrix without Q */

/* r <- an upper triangle R with R^T R = A^T A, by Householder reflectors that are never stored (a tree of QR factorisations: the
 * condition number is A's, not its square).  The block-angular damped solve reduces the fill [F | f] of qrk_bd_lm_panel with it.
 *   A    : rows x cols, column-major, leading dimension lda >= rows; rows rows .. lda of a column are never read.  rows >= 0; with
 *          fewer rows than columns the missing rows count as zero.
 *   r    : cols x cols, column-major, leading dimension ldr >= cols; exact +0.0 below the diagonal; rows cols .. ldr of a column
 *          are not touched.  The sign of R's diagonal is not specified.  A column whose remaining part is exactly zero (or has
 *          a squared norm below DBL_MIN) gets the identity reflector and keeps its diagonal entry, zero if nothing was there: never a NaN; an all-zero A, or rows = 0, gives R = +0.0 everywhere.
 *   work : qrk_dense_qless_r_work(rows, cols) doubles of the caller's (at least 1): the triangles of level 1 (level_rows[1] * cols
 *          doubles) followed by those of level 2 (level_rows[2] * cols).
 * 1 <= cols <= 32; cols = 0 writes nothing; cols > 32 is QRK_STATUS_UNSUPPORTED.  A NULL handle or buffer, a negative size,
 * lda < rows or ldr < cols is QRK_STATUS_INVALID_ARGUMENT before a device is touched.  DEVICE pointers, enqueue-only on the handle's
 * stream, no allocation, no synchronisation: the call can be captured.  No atomics; the grid, the chunks and the order of every
 * operation are a function of (rows, cols) alone, not of the device: two identical calls give identical bits.
 *
 * qrk_dense_qless_r_levels reports the schedule: level l reads level_rows[l] rows in chunks of level_chunk[l] rows (a positive
 * multiple of 256), one workgroup per chunk, each leaving one triangle of cols rows; the triangles of a level are the next level's
 * rows; the last level has one chunk and writes r.  It returns the number of levels (at most 3; 0 for cols = 0; -1 for a negative
 * size, cols > 32 or cap < 0) and writes the first min(levels, cap) entries of each array (either may be NULL).  No device is touched.
 * qrk_dense_qless_r_kernel_name: the kernel of these sizes, or a string that contains "unsupported" ("" for a negative size). */
int64_t     qrk_dense_qless_r_work(int64_t rows, int32_t cols);
qrk_status  qrk_dense_qless_r(qrk_handle h, const double* A, int64_t lda, int64_t rows, int32_t cols,
                              double* r, int64_t ldr, double* work);
int32_t     qrk_dense_qless_r_levels(int64_t rows, int32_t cols, int64_t* level_rows, int64_t* level_chunk, int32_t cap);
const char* qrk_dense_qless_r_kernel_name(int64_t rows, int32_t cols);

/* --------------------------------------------- dense right-block solver (angular) */

/* A single dense Householder QR with implicit Q: the _BlockQRSolverRight of
 * QRKit::BlockAngularSparseQR (src/QRKit/BlockAngularSparseQR.h:79), which the reference tests
 * instantiate with Eigen::ColPivHouseholderQR<MatrixXd> (test/test-qrkit.cpp:46-48).  It is called at
 * BlockAngularSparseQR.h:361-369 (compute on the bottom rows of Q1^T J2), :488 (matrixR()), :498-503
 * (colsPermutation()) and :619-622 / :636-638 (matrixQ() products).  Q stays a sequence of reflectors. */
typedef struct qrk_dense_plan_s* qrk_dense_plan;

qrk_status qrk_dense_plan_create(qrk_handle h, int32_t rows, int32_t cols, qrk_block_solver solver,
                                 qrk_dense_plan* out);
qrk_status qrk_dense_plan_destroy(qrk_dense_plan plan);

/* compute(): a (rows x cols, column-major, leading dimension lda) is overwritten by the packed QR
 * (R in the upper triangle, essential Householder vectors below); hcoeffs[min(rows,cols)];
 * perm[cols] = colsPermutation().indices().
 *
 * Large tall pivoted problems (rows >= 4 cols, cols >= 128, rows * cols >= 2^22; QRK_DENSE_TWO_STAGE=0/1 overrides) are
 * factorised in two stages: A = Q0 R0 without pivoting on the matrix cores (communication-avoiding QR), then R0 P = Q1 R with
 * Eigen's pivot rule on the n x n triangle.  Same permutation; R equal to Eigen's up to the sign of each ROW (the sign of a
 * Householder beta follows the pivot entry, which the change of basis alters); Q = Q0 diag(Q1, I).  After such a factorisation the
 * upper triangle of `a` holds R as always, but what lies below are the reflectors of Q0, not Eigen's essential vectors, and
 * hcoeffs are those of Q1: use qrk_dense_apply_q / qrk_dense_solve_r with the same plan (the factors of Q1 stay in the plan),
 * do not interpret the lower part yourself.  A pivot decision inside its rounding margin still sends the whole matrix through
 * the exact path, which leaves Eigen's format; decisions that only fix the sign of a row of R (leading entry of a reflector at the
 * noise level, zero tail) do not, since that sign is open in this form anyway.
 *
 * Synchronisation: plans of at most 2^18 entries only enqueue (the exact path is queued behind the fast one and decides on the
 * device).  Two-stage plans and plans with rows * cols >= 2^18 SYNCHRONISE the handle's stream before they return: the host reads
 * one flag word (into a pinned buffer of the plan) to know which format the factors are in / whether the exact path has to be
 * launched over the whole chip.  Such a call cannot be captured into a hipGraph. */
qrk_status qrk_dense_factorize(qrk_dense_plan plan, double* a, int64_t lda, double* hcoeffs, int32_t* perm,
                               qrk_memspace space);

/* The two-stage format keeps part of Q (the T factors of Q0 and the packed Q1) IN THE PLAN, for the array factorised last:
 * qrk_dense_apply_q with any other array fails with QRK_STATUS_INVALID_ARGUMENT while that state is live (it would otherwise
 * apply the wrong Q without a sign of it).  A caller that factorises several matrices with one plan and applies their Qs later
 * (the panel chain of BlockedThinSparseQR, src/QRKit/BlockedThinSparseQR.h:105-165) switches the format off: every
 * factorisation then leaves Eigen's self-contained packed format in the caller's own arrays.  enable = 1 switches it back on
 * for a plan whose shape qualified at creation.  qrk_dense_plan_two_stage returns the current setting. */
qrk_status qrk_dense_plan_set_two_stage(qrk_dense_plan plan, int enable);
int qrk_dense_plan_two_stage(qrk_dense_plan plan);

/* b (rows x nrhs, leading dimension ldb) <- Q^T b (transpose != 0) or Q b. */
qrk_status qrk_dense_apply_q(qrk_dense_plan plan, const double* qr, int64_t lda, const double* hcoeffs,
                             int transpose, double* b, int64_t ldb, int64_t nrhs, qrk_memspace space);

/* b(0:cols, :) <- R^-1 b(0:cols, :) in place, R = the upper triangle of the packed QR (rows >= cols): the back
 * substitution of ColPivHouseholderQR::solve / of BlockAngularSparseQR::_solve_impl on its R2 block
 * (src/QRKit/BlockAngularSparseQR.h:202-227); the column permutation is the caller's. */
qrk_status qrk_dense_solve_r(qrk_dense_plan plan, const double* qr, int64_t lda, double* b, int64_t ldb, int64_t nrhs,
                             qrk_memspace space);

/* y(0:rows) -= sum_c S(:, colidx[c]) z[c]  for c = 0..cols-1 (colidx == NULL: column c), all device pointers, S column-major with
 * leading dimension lds: the strip term of the block back substitution of BlockAngularSparseQR::_solve_impl
 * (src/QRKit/BlockAngularSparseQR.h:202-227), z1 = R1^-1 (y1 - S z2) with S = (Q1^T J2)(0:m1, P2) kept on the device. */
qrk_status qrk_dense_gemv_sub(qrk_handle h, const double* S, int64_t lds, int64_t rows, int64_t cols, const int32_t* colidx,
                              const double* z, double* y);

/* ------------------------------------------------ thin sparse right solver (BlockedThinSparseQR) */

/* QRKit::BlockedThinSparseQR (src/QRKit/BlockedThinSparseQR.h:105-283): analyzePattern (:168-201: ColumnDensity column ordering,
 * SparseQROrdering.h:21-50, and as-banded-as-possible row ordering, :52-120) and compute (:105-165) of a thin sparse matrix given
 * in CSC on the host (colptr[cols + 1], rowidx / vals[nnz], row indices strictly increasing inside a column).  The permuted matrix
 * is made dense on the device (its nonzeros cross PCIe) and factorised panel by panel: a panel of block_cols columns takes the rows
 * its sparsity pattern says (updateBlockInfo, :203-238), is factorised by the column-pivoted dense solver (qrk_dense_factorize:
 * decisions inside rounding go through the exact path as everywhere), its reflectors are applied to the columns on the right, and
 * its columns of R are written (:271-279).  The number of nonzero pivots of a panel (:250-256, Eigen's nonzeroPivots(): counted on the
 * device from the downdated column norms -- the exact path's own table when a pivot is anywhere near the threshold) decides the rows
 * of the next one, so one word per panel travels to the host.  Both language mirrors (include/qrkit/QRKit.hpp, qrkit_amd/angular.py) call this. */
typedef struct qrk_thin_plan_s* qrk_thin_plan;
qrk_status qrk_thin_sparse_factorize(qrk_handle h, int32_t rows, int32_t cols, int32_t block_cols, const int32_t* colptr,
                                     const int32_t* rowidx, const double* vals, qrk_thin_plan* out);
qrk_status qrk_thin_destroy(qrk_thin_plan plan);
/* rank() = nonzero pivots; col_perm[cols] = colsPermutation().indices() (ColumnDensity permutation * Householder column
 * permutations, zero-pivot columns last, :151-159, :250-256); row_perm[rows] = rowsPermutation().indices().  Any pointer may be NULL. */
qrk_status qrk_thin_info(qrk_thin_plan plan, int32_t* rank, int32_t* col_perm, int32_t* row_perm);
/* matrixR(): the cols x cols upper triangle (rows rank.. are zero), column-major with leading dimension ldr */
qrk_status qrk_thin_matrix_r(qrk_thin_plan plan, double* r, int64_t ldr, qrk_memspace space);
/* v <- Q^T v (transpose != 0) or Q v, device pointer, nrhs columns of `rows` entries with leading dimension ldv >= 2 rows
 * (the panels are applied with zero rows appended; the entries rows..2 rows of a column must be zero and stay zero) */
qrk_status qrk_thin_apply_q(qrk_thin_plan plan, int transpose, double* v, int64_t ldv, int64_t nrhs);
/* BlockedThinQRBase::_solve_impl (BlockedThinQRBase.h:223-247) in place: v holds b (rows entries per column, ldv as above) and on
 * return x(0:cols) = [R(0:rank,0:rank)^-1 (Q^T b)(0:rank); 0] (the caller applies the permutations, as with the reference) */
qrk_status qrk_thin_solve(qrk_thin_plan plan, double* v, int64_t ldv, int64_t nrhs);

/* --------------------------------- banded matrix given as dense strips: two-stage factorisation */

/* BandedBlockedSparseQR::factorize (src/QRKit/BandedBlockedSparseQR.h:463-508) for a block-banded matrix whose block rows are
 * handed over as DENSE STRIPS: strip i is strip_rows x strip_cols and covers the rows [i strip_rows, (i+1) strip_rows) and the
 * columns [i col_step, i col_step + strip_cols) (BASELINE configs[2]: 50 000 strips of 256 x 192, step 64 -- 2.46e9 stored
 * entries, more than the int32 StorageIndex of the reference's SparseMatrix, and of qrk_bb_plan_create's CSR, can index; here
 * every offset is 64-bit).  The factorisation runs in two stages:
 *   A  every strip is triangularised on its own, A_i = Q_i [R_i; 0]: one workgroup per strip over all CUs (the block-diagonal
 *      solver's kernels, HouseholderQR);
 *   B  a chain over the strips merges the carried triangle (the strip_cols - col_step columns the next strip shares) with R_i:
 *      the two triangles are stacked with their rows interleaved, which makes the stack a staircase whose zeros the
 *      Householder sweep never visits; col_step rows of R leave per step, the rest is carried on.
 * The reference re-factorises (leftover + strip_rows) x strip_cols per step (:503-506).  R is the reference's up to the sign of
 * each ROW (R is unique up to row signs for a fixed column order; the signs follow the elimination order);
 * Q is kept as the two sequences of reflectors, not as the reference's Y / T blocks.  All pointers are device pointers.
 *
 * Layout of Q^T b / of the argument of Q (rows = num_strips strip_rows entries): first the cols = (num_strips - 1) col_step +
 * strip_cols entries that belong to the rows of R, then per strip i the components orthogonal to the columns: (strip_cols -
 * col_step) of the chain (strips 1..), then strip_rows - strip_cols of stage A. */
typedef struct qrk_bbs_plan_s* qrk_bbs_plan;
qrk_status qrk_bbs_plan_create(qrk_handle h, int64_t num_strips, int32_t strip_rows, int32_t strip_cols, int32_t col_step,
                               qrk_bbs_plan* out);
qrk_status qrk_bbs_plan_destroy(qrk_bbs_plan plan);
/* rows, cols of the matrix; r_len = doubles of R kept by the plan (col_step x strip_cols per strip, strip_cols^2 for the last) */
qrk_status qrk_bbs_plan_sizes(qrk_bbs_plan plan, int64_t* rows, int64_t* cols, int64_t* r_len);
/* strips: strip i column-major (leading dimension strip_rows) at strips + i strip_rows strip_cols.
 * Stage A is enqueued on the handle's stream.  When stage B takes the pipelined chain (three workgroups, more than two strips) the call
 * then SYNCHRONISES that stream: it reads the chain's abort word on the host and, if a hand-off wait ran out, runs stage B again on one
 * workgroup before it returns -- so the factors are complete on return in that case (the one-workgroup chain stays enqueue-only).
 * A caller that overlaps host work or other streams with this call should issue that work first. */
qrk_status qrk_bbs_factorize(qrk_bbs_plan plan, const double* strips);
/* the rows of R emitted by strip i: rows [i col_step, ..) x columns [i col_step, i col_step + strip_cols), column-major with
 * leading dimension = the number of rows (col_step; strip_cols for the last strip), upper trapezoidal */
qrk_status qrk_bbs_r_rows(qrk_bbs_plan plan, int64_t strip, double* r_rows);
/* out = Q^T v (transpose != 0) or Q v; v, out: rows x nrhs (ld = rows), distinct; work: rows x nrhs doubles.  v is not modified
 * logically (the Q v direction reads it only).
 * The chain from strip to strip carries strip_cols - col_step numbers and every strip acts on them linearly, so the first product
 * (or solve) after a factorisation forms one small matrix per strip on all CUs (qrkit_amd/csrc/banded_maps.hip: 2 x 8 (strip_cols -
 * col_step)^2 bytes per strip, kept by the plan until the next factorisation) and the products then run every strip at once plus a
 * two-level chain of those matrices: 0.8 us per strip instead of 70 at the BASELINE configs[2] shape.  QRK_BBS_MAPS=0, more than
 * 65 535 right-hand sides, or no memory for the matrices: one workgroup walks the strips as before (same result to rounding). */
qrk_status qrk_bbs_apply_q(qrk_bbs_plan plan, int transpose, const double* v, double* out, int64_t nrhs, double* work);
/* least squares: x (cols x nrhs, ld = cols) = R^-1 (Q^T b)(0:cols) (BandedBlockedSparseQR::_solve_impl, :290-311);
 * b: rows x nrhs; work: 2 rows nrhs doubles */
qrk_status qrk_bbs_solve(qrk_bbs_plan plan, const double* b, double* x, int64_t nrhs, double* work);

/* ------------------------------------- right block sharded over GPUs: local TSQR stage */

/* rightSolver.compute(J2.bottomRows(...)) (src/QRKit/BlockAngularSparseQR.h:361-369) when the rows of J2 live on several
 * GPUs (BASELINE configs[3], "8 x MI355X sharded"): every rank reduces ITS rows to an n x n triangle without pivoting,
 * A_rank = Q0 R0 (communication-avoiding QR on the matrix cores, the first stage of the two-stage form above), the root gathers
 * the triangles (n^2 doubles per rank instead of rows_rank * n), stacks them and runs qrk_dense_factorize on the stack; Q^T b
 * follows the same route with one n-vector per rank (qrkit_amd/sharding.py, ShardedBlockAngularQR).  Device memory only, rows >= cols.
 * factorize: a (rows x cols, column-major) <- R0 in the upper triangle of its first cols rows, reflectors of Q0 elsewhere.
 * apply_q:   b (rows x nrhs) <- Q0^T b (transpose != 0) or Q0 b. */
typedef struct qrk_tsqr_plan_s* qrk_tsqr_plan;
qrk_status qrk_tsqr_plan_create(qrk_handle h, int32_t rows, int32_t cols, qrk_tsqr_plan* out);
qrk_status qrk_tsqr_plan_destroy(qrk_tsqr_plan plan);
qrk_status qrk_tsqr_factorize(qrk_tsqr_plan plan, double* a, int64_t lda, qrk_memspace space);
qrk_status qrk_tsqr_apply_q(qrk_tsqr_plan plan, const double* a, int64_t lda, int transpose, double* b, int64_t ldb,
                            int64_t nrhs, qrk_memspace space);

/* ------------------------------------------------------------ block-banded solver */

/* QRKit::BandedBlockedSparseQR<SparseMatrix, HouseholderQR<MatrixXd>, Dynamic, SuggestedBlockCols>
 * (src/QRKit/BandedBlockedSparseQR.h:122-366), generic-pattern path.
 *
 * qrk_bb_plan_create = analyzePattern (:391-433): AsBandedAsPossible row ordering
 * (src/QRKit/SparseQROrdering.h:66-119), band detection and mergeBlocks
 * (src/QRKit/SparseQRUtils.h:186-253,308-385) on the CSR pattern of the matrix (HOST arrays), plus
 * the panel chain of factorize() (:457-508) as device descriptors.  Fails with
 * QRK_STATUS_INVALID_ARGUMENT where the reference itself is outside its domain: its mergeBlocks reads
 * back() of an empty vector for non-portrait strips (SparseQRUtils.h:375), and its BlockYTY row layout
 * (BlockYTY.h:152-172: numCols rows at rowIndex, numZeros rows skipped, then the rest) cannot express
 * every panel of the chain.  Panel i >= 1 consists of `carried` = numRows(i-1) - (idxCol(i) - idxCol(i-1))
 * rows taken over from panel i-1 followed by the numRows(i) rows of its own block, and its unclamped
 * numZeros is z = idxRow(i) - idxCol(i) - carried.  The block's own rows land on their matrix rows only
 * if z == 0, or z > 0 and carried >= numCols(i); any other pattern is refused (also by
 * qrk_bb_plan_create_fixed and qrk_bb_analyze_host), because the reference computes the right R but a
 * wrong Q on it.  For strips of ms rows and n columns stepping by s columns: ms - s >= n once there are
 * more than two panels. */
typedef struct qrk_bb_plan_s* qrk_bb_plan;

qrk_status qrk_bb_plan_create(qrk_handle h, int32_t rows, int32_t cols, const int32_t* csr_rowptr,
                              const int32_t* csr_colidx, int32_t suggested_block_cols, qrk_bb_plan* out);
qrk_status qrk_bb_plan_destroy(qrk_bb_plan plan);

/* The fixed-pattern path of BandedBlockedSparseQR::analyzePattern (src/QRKit/BandedBlockedSparseQR.h:398-408, taken when the
 * block type is fixed-size and _BlockOverlap != Dynamic): identity row permutation and the block map of
 * BlockBandedMatrixInfo::fromBlockBandedPattern (src/QRKit/SparseQRUtils.h:274-302) + mergeBlocks (:308-385) instead of the
 * row ordering and band detection of qrk_bb_plan_create.  csr_*: pattern of the matrix, as there. */
qrk_status qrk_bb_plan_create_fixed(qrk_handle h, int32_t rows, int32_t cols, const int32_t* csr_rowptr,
                                    const int32_t* csr_colidx, int32_t block_rows, int32_t block_cols, int32_t block_overlap,
                                    int32_t suggested_block_cols, qrk_bb_plan* out);

/* Host-only: the merged block map of that fixed pattern (blocks: 4 ints each, idxRow idxCol numRows numCols; at most cap).
 * Reproduces the reference's known answer test/test-utils.cpp:228-241 (7x4 blocks, overlap 2 -> 255 blocks, the last 14x4). */
qrk_status qrk_bb_blocks_from_pattern(int32_t rows, int32_t cols, int32_t block_rows, int32_t block_cols, int32_t block_overlap,
                                      int32_t suggested_block_cols, int32_t cap, int32_t* num_blocks, int32_t* blocks);

/* The same structure analysis without a device (pure host integer logic): writes up to `cap` blocks as
 * (idxRow, idxCol, numRows, numCols) and, when row_perm != NULL, the row permutation indices;
 * *num_blocks receives the block count.  Lets the reference's known answers
 * (test/test-utils.cpp:199-205,228-241,264-271) be checked anywhere. */
qrk_status qrk_bb_analyze_host(int32_t rows, int32_t cols, const int32_t* csr_rowptr, const int32_t* csr_colidx,
                               int32_t suggested_block_cols, int32_t cap, int32_t* num_blocks, int32_t* blocks,
                               int32_t* row_perm, int32_t* has_row_perm);

/* num_blocks merged blocks; nnz_r entries of m_R (explicit zeros of the emitted rows included, :487-491);
 * y_len / t_len doubles of the implicit Q: per block the panel factorised in place (activeRows x numCols,
 * ROW-major; Y of the reference's BlockYTY, :471-475, is its unit-lower view - the diagonal and what lies
 * above it are to be ignored) and T (numCols x numCols, upper, column-major, NEGATED as the reference stores
 * it, :477); has_row_perm as
 * AsBandedAsPossible::hasPermutation. */
qrk_status qrk_bb_plan_info(qrk_bb_plan plan, int32_t* num_blocks, int64_t* nnz_r, int64_t* y_len,
                            int64_t* t_len, int32_t* has_row_perm);

/* Which code qrk_bb_factorize runs on panel `panel` (0 .. num_blocks - 1) of this plan, host only: "bb_chain_kernel", or
 * "bb_chain2_kernel ob<16|32> nr<3|4|8|16> t_<lds|global>" (block width and 64-row registers of the panel's blocked QR; T of
 * the panels built in LDS or in place).  The environment switches QRK_BB_CHAIN_V1 and QRK_BB_T_GLOBAL are read as
 * qrk_bb_factorize reads them.  "" for a bad argument.  The pointer is static, like qrk_bd_kernel_name. */
const char* qrk_bb_kernel_name(qrk_bb_plan plan, int32_t panel);

/* Host outputs: blocks[4*num_blocks] = (idxRow, idxCol, numRows, numCols) of m_blockInfo in order;
 * row_perm[rows] = rowsPermutation().indices(): (P*M).row(row_perm[i]) = M.row(i);
 * yty[6*num_blocks] = per block (rowIndex, numZeros, rows(Y), cols(Y), ... ) see INTEGRATION.md. */
qrk_status qrk_bb_plan_blocks(qrk_bb_plan plan, int32_t* blocks, int32_t* row_perm, int64_t* yty);

/* CSC pattern of m_R (cols+1 pointers, nnz_r row indices). */
qrk_status qrk_bb_pattern(qrk_bb_plan plan, int32_t* r_colptr, int32_t* r_rowidx, qrk_memspace space);

/* factorize() (:443-519): csr_vals are the values of the UNPERMUTED matrix in the CSR order given to
 * qrk_bb_plan_create; r_vals [nnz_r] in CSC order; y_vals [y_len]; t_vals [t_len]. */
qrk_status qrk_bb_factorize(qrk_bb_plan plan, const double* csr_vals, int64_t nnz, double* r_vals,
                            double* y_vals, double* t_vals, qrk_memspace space);

/* v (rows x nrhs, ld = rows) <- Q^T v (transpose != 0; blocks ascending with T^T) or Q v (descending
 * with T): SparseBlockYTY_VecProduct (src/QRKit/SparseBlockYTY.h:100-139). */
qrk_status qrk_bb_apply_q(qrk_bb_plan plan, const double* y_vals, const double* t_vals, int transpose,
                          double* v, int64_t nrhs, qrk_memspace space);

/* v(0:cols, :) <- R(0:cols, 0:cols).triangularView<Upper>().solve(v(0:cols, :)) in place for nrhs columns (leading
 * dimension ldv >= cols): the back substitution that ends BandedBlockedSparseQR::_solve_impl
 * (src/QRKit/BandedBlockedSparseQR.h:290-311, after y = Q^T b).  R is the one of the last qrk_bb_factorize of this
 * plan (the plan keeps its rows on the device). */
qrk_status qrk_bb_solve_r(qrk_bb_plan plan, double* v, int64_t ldv, int64_t nrhs, qrk_memspace space);

/* ------------------------------------------------------------- multi-GPU: shards of the diagonal blocks */

/* One process per GPU.  The hot loop of BlockDiagonalSparseQR::factorize (src/QRKit/BlockDiagonalSparseQR.h:432-526) carries nothing
 * from block to block but the running offsets base_row / base_col (:428-431, :524-525), so the blocks shard as CONTIGUOUS ranges
 * with no data-path collective: rank g factorises blocks [first_block, first_block + num_blocks) with a plan of its own and its
 * Q / R / permutation shards are already in the global order.  No reference site (the reference is single-threaded): SURVEY.md 8(e).
 *
 * qrk_shard_ranges: ranges balanced by the Householder cost r c^2 per block (equal counts for uniform blocks), and the global
 * offsets of each range.  Host-only integer logic: no handle, no GPU.  Uniform layouts pass rows = cols = NULL and block_rows /
 * block_cols.  shards: world + 1 entries; entry world is the end sentinel (first_block = num_blocks, num_blocks = 0, the offsets
 * = the totals), so that the element counts of rank g are differences of consecutive entries. */
typedef struct qrk_shard {
    int64_t first_block, num_blocks;
    int64_t base_row, base_col;      /* rows / columns of the matrix before the range (BlockDiagonalSparseQR.h:428-431) */
    int64_t tiles_off, q_off, r_off; /* offsets of the range in the global tiles / q_vals (tile part) / r_vals arrays */
} qrk_shard;
qrk_status qrk_shard_ranges(int64_t num_blocks, int32_t block_rows, int32_t block_cols, const int32_t* rows, const int32_t* cols,
                            int32_t world, qrk_shard* shards);

/* The only exchange of the path: the composed R (packed CSC values) and the column permutation gathered on `root` with their TRUE
 * counts -- ncclGroupStart / one ncclRecv per peer on the root, one ncclSend on every other rank / ncclGroupEnd, on the handle's
 * stream (RCCL over xGMI; no padding to the largest shard).  nccl_comm: the caller's ncclComm_t of `world` ranks (passed as void*:
 * this header needs no RCCL header; the library resolves ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd from the RCCL that
 * is already loaded in the process, else from librccl.so); may be NULL when world = 1.  r_local / perm_local: this rank's shards
 * as qrk_bd_factorize of its own plan wrote them (device; permutation indices local to the shard).  r_all [r_off of the sentinel],
 * perm_all [base_col of the sentinel]: device, root only (ignored elsewhere); perm_all holds GLOBAL column indices
 * (m_outputPerm_c.indices(), :519-521: the shard's base_col added). */
qrk_status qrk_gather_r(qrk_handle h, void* nccl_comm, int32_t rank, int32_t world, int32_t root, const qrk_shard* shards,
                        const double* r_local, const int32_t* perm_local, double* r_all, int32_t* perm_all);

/* The sharded SOLVE: _solve_impl (BlockDiagonalSparseQR.h:257-280) is block-local -- x_g = P_g R_g^-1 (Q_g^T b_g)(0:cols_g) needs
 * only the rank's own Q, R and permutation (qrk_bd_solve on the rank's plan) -- so a least-squares consumer never needs the composed
 * R: only x travels, 8 bytes per column and right-hand side (256 B per 32 x 32 tile against 4 352 B of R and permutation).
 * x_local: this rank's solution as qrk_bd_solve wrote it (device; nrhs vectors of cols_g entries, vector k at k * cols_g).  x_all: device,
 * root only: nrhs vectors of the whole matrix's columns, vector k at k * total_cols, rank g's piece at base_col of its shard.  One
 * grouped ncclSend / ncclRecv per peer and right-hand side, true counts, on the handle's stream. */
qrk_status qrk_gather_x(qrk_handle h, void* nccl_comm, int32_t rank, int32_t world, int32_t root, const qrk_shard* shards,
                        const double* x_local, int64_t nrhs, double* x_all);

/* The two exchanges of the ANGULAR solver sharded by rows (the TSQR route of qrk_tsqr_* above; BlockAngularSparseQR.h:361-369, 459-514;
 * host side: qrkit::ShardedBlockAngularSparseQR, qrkit_amd/sharding.py): every rank's `count` doubles to `root` (recv: world * count
 * doubles on the root, piece g at g * count; one n x n triangle, or one n-vector, per rank), and `bytes` bytes at `buf` from `root` to
 * every rank (the permutation of the right block, z2).  Device memory, the handle's stream, grouped ncclSend / ncclRecv on the caller's
 * communicator exactly as qrk_gather_r.  Collective: every rank calls them with the same world / root / count / bytes. */
qrk_status qrk_gather_equal(qrk_handle h, void* nccl_comm, int32_t rank, int32_t world, int32_t root, const double* send, int64_t count,
                            double* recv);
qrk_status qrk_bcast(qrk_handle h, void* nccl_comm, int32_t rank, int32_t world, int32_t root, void* buf, int64_t bytes);

/* ------------------------------------------------------------- measurement */

/* Launch the factorisation kernel(s) of `plan` `iters` times back to back on the
 * handle's stream, rotating over `nsets` consecutive copies of the input/output
 * arrays (set s uses tiles + s*tiles_len, q_vals + s*nnz_q, ...), bracketed by
 * HIP events on that same stream.  *avg_ms = elapsed / iters.  Device memory only. */
qrk_status qrk_bd_time_factorize(qrk_bd_plan plan, const double* tiles, double* q_vals,
                                 double* r_vals, int32_t* perm, int nsets, int iters,
                                 float* avg_ms);

/* Name of the factorisation kernel `plan` launches for its tiles (which = 0: the kernel of the largest size class present),
 * taken from the same dispatch qrk_bd_factorize uses; for reports (bench.py's roofline.kernel).  The pointer is static. */
const char* qrk_bd_kernel_name(qrk_bd_plan plan, int which);


#ifdef __cplusplus
}
#endif
#endif /* QRKIT_AMD_H */
