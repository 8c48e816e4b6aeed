// bdqr_qless.hip -- the two small kernels behind the Q-less fast paths of qrk_bd_factorize_rhs (bdqr_thin_rhs.hip, the right-hand-side
// form of bdqr_pair4.hip), for gfx950.
//
//  * bdqr_qless_redo_kernel: the tiles a fast kernel flagged (a decision inside its rounding margin, see bdqr_exact.hip) again, in
//    Eigen's own operation order -- blockSolver.compute(block), src/QRKit/BlockDiagonalSparseQR.h:437-447,519-521 -- and then, from the
//    Q_i that exact::tile_qr leaves in LDS, this tile's part of _solve_impl (:257-280): y = Q_i^T b_i, the back substitution with R_i,
//    the permutation.  One workgroup of 64 threads per listed tile; working copy and Q_i in LDS (tiles of at most 32 x 32), Q_i never
//    leaves the chip.  Generic data never gets here: the list is empty and the workgroups return at once.
//  * qless_backsolve32_kernel: x = P R^-1 y for uniform 32 x 32 batches, IN PLACE in x (the 32 x 32 kernel leaves the top of Q^T b at
//    the tile's own columns of x; the permutation of a tile stays inside those columns).  bd_aux.hip's grouped back substitution with
//    y taken from x: 32 lanes per tile, the lane's row of R in registers, same sums in the same order.
#include "qrk_device.h"
#include "bdqr_exact_tile.h"

namespace qrk {

namespace qless {
constexpr int MAXD = 32;        // largest tile dimension of the redo kernel
}

template <bool PIVOT>
__global__ void __launch_bounds__(64)
bdqr_qless_redo_kernel(int64_t num_tiles, int r, int c, const int32_t* __restrict__ ids, const int32_t* __restrict__ count,
                       int32_t* next_count, const double* __restrict__ tiles, const double* __restrict__ b, int64_t nrhs, int64_t mat_rows,
                       int64_t mat_cols, int q_format, double* __restrict__ r_vals, int32_t* __restrict__ perm,
                       double* __restrict__ hcoeffs, double* __restrict__ qtb, double* __restrict__ x)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qless_smem[];
    exact::Shared sh;
    double* W = exact::carve_shared<64>(qless_smem, r, c, sh);      // [r][c] working copy, row-major
    double* q = W + r * c;                                          // [r][r] Q_i, row-major
    const int lane = threadIdx.x;
    // (the list counter of the NEXT factorisation is reset here, as bdqr_exact_kernel does: no memset sits on the stream)
    if (next_count && blockIdx.x == 0 && lane == 0) *next_count = 0;
    int64_t n = (int64_t)*count;
    if (n > num_tiles) n = num_tiles;
    for (int64_t li = blockIdx.x; li < n; li += gridDim.x) {
        const int64_t t = (int64_t)ids[li];
        if (t < 0 || t >= num_tiles) continue;
        const int cbase = (int)(t * c);
        __syncthreads();
        exact::tile_qr<PIVOT, 64>(r, c, tiles + t * (int64_t)r * c, W, q, sh);
        exact::tile_store<64>(r, c, cbase, W, nullptr, sh, perm, hcoeffs, r_vals + t * (int64_t)(c * (c + 1) / 2), nullptr);
        __syncthreads();
        const int64_t base_row = t * (int64_t)r;
        for (int64_t rhs = 0; rhs < nrhs; ++rhs) {
            // y_k = sum_j Q(j, k) b_j, j ascending: lane k (r <= 32: one entry per lane), the sum of bd_apply_qt_kernel
            const double* bb = b + rhs * mat_rows + base_row;
            double yk = 0.0;
            if (lane < r)
                for (int j = 0; j < r; ++j) yk = fma(q[j * r + lane], bb[j], yk);
            if (qtb && lane < r) {
                int64_t idx;
                if (q_format == 0) idx = lane < c ? (int64_t)cbase + lane : mat_cols + (base_row - cbase) + (lane - c);
                else idx = base_row + lane;
                qtb[rhs * mat_rows + idx] = yk;
            }
            if (x) {
                // column-oriented back substitution (bd_solve_kernel): R(i, kk) is entry (i, col_at[kk]) of the working copy
                for (int kk = c - 1; kk >= 0; --kk) {
                    const int col = sh.col_at[kk];
                    const double piv = readlane_f64(yk, kk) / W[kk * c + col];
                    if (lane == kk) yk = piv;
                    else if (lane < kk) yk = fma(-W[lane * c + col], piv, yk);
                }
                if (lane < c) x[rhs * mat_cols + cbase + sh.col_at[lane]] = yk;
            }
        }
    }
}

hipError_t launch_bdqr_qless_redo(int64_t num_tiles, int r, int c, int pivoting, const int32_t* ids, const int32_t* count, int32_t* next_count,
                                  const double* tiles, const double* b, int64_t nrhs, int64_t mat_rows, int64_t mat_cols, int q_format,
                                  double* r_vals, int32_t* perm, double* hcoeffs, double* qtb, double* x, int num_wg, hipStream_t stream)
{
    if (num_tiles <= 0 || num_wg <= 0) return hipSuccess;
    if (r > qless::MAXD || c > r || c < 1) return hipErrorInvalidValue;
    // exact::carve_shared<64>: [r + 3 c + 64] doubles, [2 c + 64] ints, rounded up to 16 bytes; then W and Q
    const size_t smem = (((size_t)(r + 3 * c + 64) * sizeof(double) + (size_t)(2 * c + 64) * sizeof(int) + 15) & ~(size_t)15) + 16 +
                        (size_t)(r * c + r * r) * sizeof(double);
    const dim3 grid((unsigned)((int64_t)num_wg < num_tiles ? num_wg : num_tiles)), block(64);
    if (pivoting)
        hipLaunchKernelGGL(bdqr_qless_redo_kernel<true>, grid, block, smem, stream, num_tiles, r, c, ids, count, next_count, tiles, b, nrhs,
                           mat_rows, mat_cols, q_format, r_vals, perm, hcoeffs, qtb, x);
    else
        hipLaunchKernelGGL(bdqr_qless_redo_kernel<false>, grid, block, smem, stream, num_tiles, r, c, ids, count, next_count, tiles, b, nrhs,
                           mat_rows, mat_cols, q_format, r_vals, perm, hcoeffs, qtb, x);
    return hipGetLastError();
}

// The panel sibling of bdqr_qless_redo_kernel, behind qrk_bd_factorize_apply_qt (bdqr_thin_panel.hip): the listed tiles again, then
// Q_i^T on the tile's rows of EVERY column of a strided panel (column j at pc + j * ldc, out at qtc + j * ldq), no x.  Tiles of at most
// 32 rows: lane k of each half of the wavefront owns output entry k, the two halves take alternate columns.
template <bool PIVOT>
__global__ void __launch_bounds__(64)
bdqr_qless_redo_panel_kernel(int64_t num_tiles, int r, int c, const int32_t* __restrict__ ids, const int32_t* __restrict__ count,
                             int32_t* next_count, const double* __restrict__ tiles, const double* __restrict__ pc, int64_t ldc,
                             int64_t ncols, int64_t mat_cols, int q_format, double* __restrict__ r_vals, int32_t* __restrict__ perm,
                             double* __restrict__ hcoeffs, double* __restrict__ qtc, int64_t ldq)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char qless_smem[];
    exact::Shared sh;
    double* W = exact::carve_shared<64>(qless_smem, r, c, sh);      // [r][c] working copy, row-major
    double* q = W + r * c;                                          // [r][r] Q_i, row-major
    const int lane = threadIdx.x, k = lane & 31, half = lane >> 5;
    if (next_count && blockIdx.x == 0 && lane == 0) *next_count = 0;
    int64_t n = (int64_t)*count;
    if (n > num_tiles) n = num_tiles;
    for (int64_t li = blockIdx.x; li < n; li += gridDim.x) {
        const int64_t t = (int64_t)ids[li];
        if (t < 0 || t >= num_tiles) continue;
        const int cbase = (int)(t * c);
        __syncthreads();
        exact::tile_qr<PIVOT, 64>(r, c, tiles + t * (int64_t)r * c, W, q, sh);
        exact::tile_store<64>(r, c, cbase, W, nullptr, sh, perm, hcoeffs, r_vals + t * (int64_t)(c * (c + 1) / 2), nullptr);
        __syncthreads();
        const int64_t base_row = t * (int64_t)r;
        if (k < r) {
            int64_t idx;
            if (q_format == 0) idx = k < c ? (int64_t)cbase + k : mat_cols + (base_row - cbase) + (k - c);
            else idx = base_row + k;
            for (int64_t j = half; j < ncols; j += 2) {
                // y_k = sum_i Q(i, k) c_i, i ascending: the sum of bd_apply_qt_kernel
                const double* bb = pc + j * ldc + base_row;
                double yk = 0.0;
                for (int i = 0; i < r; ++i) yk = fma(q[i * r + k], bb[i], yk);
                qtc[j * ldq + idx] = yk;
            }
        }
    }
}

hipError_t launch_bdqr_qless_redo_panel(int64_t num_tiles, int r, int c, int pivoting, const int32_t* ids, const int32_t* count,
                                        int32_t* next_count, const double* tiles, const double* pc, int64_t ldc, int64_t ncols,
                                        int64_t mat_cols, int q_format, double* r_vals, int32_t* perm, double* hcoeffs, double* qtc,
                                        int64_t ldq, int num_wg, hipStream_t stream)
{
    if (num_tiles <= 0 || num_wg <= 0) return hipSuccess;
    if (r > qless::MAXD || c > r || c < 1) return hipErrorInvalidValue;
    // (the carve of launch_bdqr_qless_redo)
    const size_t smem = (((size_t)(r + 3 * c + 64) * sizeof(double) + (size_t)(2 * c + 64) * sizeof(int) + 15) & ~(size_t)15) + 16 +
                        (size_t)(r * c + r * r) * sizeof(double);
    const dim3 grid((unsigned)((int64_t)num_wg < num_tiles ? num_wg : num_tiles)), block(64);
    if (pivoting)
        hipLaunchKernelGGL(bdqr_qless_redo_panel_kernel<true>, grid, block, smem, stream, num_tiles, r, c, ids, count, next_count, tiles, pc,
                           ldc, ncols, mat_cols, q_format, r_vals, perm, hcoeffs, qtc, ldq);
    else
        hipLaunchKernelGGL(bdqr_qless_redo_panel_kernel<false>, grid, block, smem, stream, num_tiles, r, c, ids, count, next_count, tiles, pc,
                           ldc, ncols, mat_cols, q_format, r_vals, perm, hcoeffs, qtc, ldq);
    return hipGetLastError();
}

__global__ void __launch_bounds__(64)
qless_backsolve32_kernel(int64_t num_tiles, const double* __restrict__ r_vals, const int32_t* __restrict__ perm, int64_t nrhs,
                         int64_t mat_cols, double* x)
{
    constexpr int G = 32;
    const int lane = threadIdx.x, grp = lane >> 5, k = lane & 31;
    const int64_t ntg = (num_tiles + 1) / 2;
    const int64_t total = ntg * nrhs;
    for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const int64_t t = (w % ntg) * 2 + grp, rhs = w / ntg;
        const bool valid = t < num_tiles;
        const int64_t roff = (valid ? t : 0) * 528, base_col = (valid ? t : 0) * 32;
        // the lane's row of R: entry (k, kk) of the packed upper triangle is at kk (kk + 1) / 2 + k
        double rrow[G];
#pragma unroll
        for (int kk = 0; kk < G; ++kk) {
            const double v = r_vals[roff + ((valid && kk >= k) ? kk * (kk + 1) / 2 + k : 0)];
            rrow[kk] = (valid && kk >= k) ? v : 1.0;
        }
        double* xx = x + rhs * mat_cols + base_col;
        double yk = valid ? xx[k] : 0.0;
        const int dst = perm[base_col + k] - (int)base_col;
#pragma unroll
        for (int kk = G - 1; kk >= 0; --kk) {
            const double pv = yk / rrow[kk];                   // (meaningful in lane kk of the group)
            const double piv = __shfl(pv, grp * G + kk, 64);
            if (k == kk) yk = piv;
            else if (k < kk) yk = fma(-rrow[kk], piv, yk);
        }
        // (every lane of the wave has read its entry of y by now: the tile's columns of x are rewritten in place)
        if (valid && dst >= 0 && dst < G) xx[dst] = yk;
    }
}

void launch_qless_backsolve32(int64_t num_tiles, const double* r_vals, const int32_t* perm, int64_t nrhs, int64_t mat_cols, double* x,
                              hipStream_t stream)
{
    const int64_t total = ((num_tiles + 1) / 2) * nrhs;
    if (total <= 0) return;
    const unsigned grid = (unsigned)(total < 262144 ? total : 262144);
    hipLaunchKernelGGL(qless_backsolve32_kernel, dim3(grid), dim3(64), 0, stream, num_tiles, r_vals, perm, nrhs, mat_cols, x);
}

}  // namespace qrk
