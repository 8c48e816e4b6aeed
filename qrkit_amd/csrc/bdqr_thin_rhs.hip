// bdqr_thin_rhs.hip -- factorise-and-solve WITHOUT Q for uniform batches of tall-thin small tiles (1 or 2 columns, at most 16 rows):
// one tile per LANE, for gfx950.  The Q-less sibling of bdqr_thin.hip, behind qrk_bd_factorize_rhs.
//
// Seam in the reference: the hot loop of QRKit::BlockDiagonalSparseQR::factorize (src/QRKit/BlockDiagonalSparseQR.h:432-526) followed by
// _solve_impl (:257-280) -- y = Q^T b, the triangular solve with R, the column permutation -- as a Levenberg-Marquardt caller runs them
// every iteration (examples/ellipse_fitting.cpp:126-142).  That caller never reads Q: with two columns Q^T b = H1 H0 b is two reflector
// applications on the lane's own r entries of b, so the r^2 entries of Q_i (648 bytes per 9 x 2 tile, written by one launch and read
// back by the next: 1 296 of the 1 592 bytes the two-call route moves) are neither formed nor stored.  Per 9 x 2 tile and right-hand side: 144 B of tile and 72 B of b in; 24 B of R,
// 8 B of permutation, 72 B of Q^T b and 16 B of x out (+ 16 B of tau when asked for).
//
// Arithmetic and decisions are bdqr_thin.hip's, statement for statement: squared norms, un-normalised reflector, the pivot (one
// comparison), a degenerate reflector on a non-empty tail, a first entry too small to fix the sign of beta and a pivot at the noise
// level are only taken when clear of rounding, else the tile goes to the redo list (bdqr_qless.hip redoes it in Eigen's operation order).
#include "qrk_device.h"

#include <float.h>

namespace qrk {
namespace thin_rhs {

using namespace decide;
constexpr int RM = 16;      // rows of a tile at most

__device__ __forceinline__ double sqrt_pos(double x)      // <= 1 ulp for positive normal x (bdqr_thin.hip)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double e = fma(-h, g, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
    const double d = fma(-g, g, x);
    return fma(d, h, g);
}
__device__ __forceinline__ double recip(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    return y;
}

// One workgroup = 256 lanes = 256 consecutive tiles, and their 256 segments of b: one contiguous run of r * 256 doubles per right-hand
// side.  Every global access is a coalesced sweep through LDS, as in bdqr_thin.hip:
//   in    the tiles (tile t at an odd stride) and, in flight with them, the segments of right-hand side 0 (segment t at the odd stride sb);
//   out   every lane leaves its r entries of Q^T b over its segment and its one or two unknowns, already permuted, in the (dead) tile
//         area; the workgroup then writes Q^T b and x in OUTPUT order.
// Further right-hand sides take one more trip through the segment area each (the reflectors stay in registers).  The trailing identity
// rows of Q (mat_rows > the rows the tiles cover) pass b through: a grid-stride copy at the start of the launch.
template <bool PIVOT, bool HC>
__global__ void __launch_bounds__(256)
bdqr_thin_rhs_kernel(int64_t num_tiles, int r, int c, const double* __restrict__ tiles, const double* __restrict__ b, int nrhs,
                     int64_t mat_rows, int64_t mat_cols, int q_format, double* __restrict__ r_vals, int32_t* __restrict__ perm,
                     double* __restrict__ hcoeffs, double* __restrict__ qtb, double* __restrict__ x, int32_t* __restrict__ redo_count,
                     int32_t* __restrict__ redo_ids)
{
    extern __shared__ double thin_rhs_lds[];
    const int tid = threadIdx.x;
    const int rc = r * c;
    const int sin = rc | 1;              // LDS stride of a tile's input (odd)
    const int sb = r | 1;                // LDS stride of a tile's segment of b / of Q^T b (odd)
    double* const lds_a = thin_rhs_lds;              // [256][sin] tiles in, then [256][c] the unknowns out
    double* const lds_b = thin_rhs_lds + 256 * sin;  // [256][sb]
    const float inv_r = 1.0f / (float)r;
    if (qtb) {
        const int64_t sum_rows = num_tiles * r, ntail = mat_rows - sum_rows;
        for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < ntail * nrhs; i += (int64_t)gridDim.x * 256) {
            const int64_t rhs = i / ntail, k = i - rhs * ntail;
            qtb[rhs * mat_rows + sum_rows + k] = b[rhs * mat_rows + sum_rows + k];
        }
    }
    for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < num_tiles; t0 += (int64_t)gridDim.x * 256) {
        const int nt = (int)(num_tiles - t0 < 256 ? num_tiles - t0 : 256);
        const int nb = nt * r;           // entries of b of this workgroup: at most 16 per thread
        // ---- in: the segments of right-hand side 0 are requested first and stored last, so that they travel with the tiles
        double bv[RM];
        {
            const double* src = b + t0 * (int64_t)r;
#pragma unroll
            for (int u = 0; u < RM; ++u) { const int e = tid + 256 * u; bv[u] = QRK_TILE_LOAD(src + (e < nb ? e : nb - 1)); }
        }
        {
            // (bdqr_thin.hip's copy: all the loads of a thread issued before the first one is waited for, clamped addresses)
            const double* src = tiles + t0 * (int64_t)rc;
            const int n = nt * rc;
            if ((rc & 1) == 0) {
                typedef double d2 __attribute__((ext_vector_type(2)));
                const d2* src2 = reinterpret_cast<const d2*>(src);             // (t0 is a multiple of 256: 16-byte aligned)
                const int n2 = n >> 1, h2 = rc >> 1;
                const float inv_h2 = 1.0f / (float)h2;
                for (int base = tid; base < n2; base += 256 * 8) {
                    d2 v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { const int e = base + 256 * u; v[u] = QRK_TILE_LOAD(src2 + (e < n2 ? e : n2 - 1)); }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int e = base + 256 * u;
                        if (e < n2) {
                            const int tl = (int)(((float)e + 0.5f) * inv_h2);
                            double* o = lds_a + tl * sin + 2 * (e - tl * h2);
                            o[0] = v[u].x; o[1] = v[u].y;
                        }
                    }
                }
            } else {
                const float inv_rc = 1.0f / (float)rc;
                for (int base = tid; base < n; base += 256 * 8) {
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { const int e = base + 256 * u; v[u] = QRK_TILE_LOAD(src + (e < n ? e : n - 1)); }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int e = base + 256 * u;
                        if (e < n) {
                            const int tl = (int)(((float)e + 0.5f) * inv_rc);
                            lds_a[tl * sin + (e - tl * rc)] = v[u];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < RM; ++u) {
            const int e = tid + 256 * u;
            if (e < nb) {
                const int tl = (int)(((float)e + 0.5f) * inv_r);
                lds_b[tl * sb + (e - tl * r)] = bv[u];
            }
        }
        __syncthreads();
        const int64_t t = t0 + tid;
        const bool have = tid < nt;
        double a0[RM], a1[RM], y[RM];
#pragma unroll
        for (int i = 0; i < RM; ++i) {
            a0[i] = (have && i < r) ? lds_a[tid * sin + i] : 0.0;
            a1[i] = (have && c > 1 && i < r) ? lds_a[tid * sin + r + i] : 0.0;
            y[i] = (have && i < r) ? lds_b[tid * sb + i] : 0.0;
        }
        __syncthreads();                 // (the input areas are dead: the results go over them)
        bool unclear = false;
        int P = 0;
        double a2 = 0.0;
        if (c > 1 && PIVOT) {
            // first maximum of the two squared column norms; a tie or a near tie is Eigen's to decide (exact path)
            double n0 = 0.0, n1 = 0.0;
#pragma unroll
            for (int i = 0; i < RM; ++i) { n0 = fma(a0[i], a0[i], n0); n1 = fma(a1[i], a1[i], n1); }
            P = n1 > n0 ? 1 : 0;
            const double best = P ? n1 : n0, other = P ? n0 : n1;
            a2 = best;
            if (near_best(other, other * THR_HI, best, a2)) unclear = true;
            if (P) {
#pragma unroll
                for (int i = 0; i < RM; ++i) { const double tmp = a0[i]; a0[i] = a1[i]; a1[i] = tmp; }
            }
        }
        // ---- reflector 0 on a0 (makeHouseholder, Eigen/src/Householder/Householder.h)
        double tsq = 0.0;
#pragma unroll
        for (int i = 1; i < RM; ++i) tsq = fma(a0[i], a0[i], tsq);
        const double x0 = a0[0];
        if (!(c > 1 && PIVOT)) a2 = fma(x0, x0, tsq);
        if (have && unclear_reflector(x0, tsq, r > 1, PIVOT, a2)) unclear = true;
        double tau0, beta0, inv0;
        if (!(tsq > DBL_MIN)) { tau0 = 0.0; beta0 = x0; inv0 = 0.0; }
        else {
            beta0 = sqrt_pos(fma(x0, x0, tsq));
            if (x0 >= 0.0) beta0 = -beta0;
            inv0 = recip(x0 - beta0);
            tau0 = (beta0 - x0) * recip(beta0);
        }
        a0[0] = 1.0;                                      // v0 = [1; essential] in place
#pragma unroll
        for (int i = 1; i < RM; ++i) a0[i] *= inv0;
        double tau1 = 0.0, beta1 = 0.0, r01 = 0.0;
        if (c > 1) {
            // applyHouseholderOnTheLeft to the other column: tmp = y0 + ess^T y_tail; y0 -= tau tmp; y_tail -= tau tmp ess
            double tmp = a1[0];
#pragma unroll
            for (int i = 1; i < RM; ++i) tmp = fma(a0[i], a1[i], tmp);
            const double g = tau0 * tmp;
            r01 = a1[0] - g;
#pragma unroll
            for (int i = 1; i < RM; ++i) a1[i] = fma(-g, a0[i], a1[i]);
            // ---- reflector 1 on a1(1:)
            double tsq1 = 0.0;
#pragma unroll
            for (int i = 2; i < RM; ++i) tsq1 = fma(a1[i], a1[i], tsq1);
            const double y0 = a1[1];
            if (have && unclear_reflector(y0, tsq1, r > 2, PIVOT, a2)) unclear = true;
            double inv1;
            if (!(tsq1 > DBL_MIN)) { tau1 = 0.0; beta1 = y0; inv1 = 0.0; }
            else {
                beta1 = sqrt_pos(fma(y0, y0, tsq1));
                if (y0 >= 0.0) beta1 = -beta1;
                inv1 = recip(y0 - beta1);
                tau1 = (beta1 - y0) * recip(beta1);
            }
            a1[0] = 0.0; a1[1] = 1.0;                     // v1 = [0; 1; essential]
#pragma unroll
            for (int i = 2; i < RM; ++i) a1[i] *= inv1;
        }
        if (have) {
            // ---- a decision inside its error margin: the exact path redoes the tile (its outputs below are overwritten)
            if (unclear) redo_ids[atomicAdd(redo_count, 1)] = (int32_t)t;
            // ---- R (packed upper triangle by columns), permutation, tau
            double* rv = r_vals + t * (int64_t)(c * (c + 1) / 2);
            rv[0] = beta0;
            if (c > 1) { rv[1] = r01; rv[2] = beta1; }
            const int cbase = (int)(t * c);
            perm[cbase] = cbase + P;
            if (c > 1) perm[cbase + 1] = cbase + 1 - P;
            if (HC && hcoeffs) { hcoeffs[cbase] = tau0; if (c > 1) hcoeffs[cbase + 1] = tau1; }
        }
        for (int rhs = 0; rhs < nrhs; ++rhs) {
            if (rhs > 0) {
                // the segments of the next right-hand side (the sweeps of the previous one ended with a barrier)
                const double* src = b + rhs * mat_rows + t0 * (int64_t)r;
#pragma unroll
                for (int u = 0; u < RM; ++u) { const int e = tid + 256 * u; bv[u] = QRK_TILE_LOAD(src + (e < nb ? e : nb - 1)); }
#pragma unroll
                for (int u = 0; u < RM; ++u) {
                    const int e = tid + 256 * u;
                    if (e < nb) {
                        const int tl = (int)(((float)e + 0.5f) * inv_r);
                        lds_b[tl * sb + (e - tl * r)] = bv[u];
                    }
                }
                __syncthreads();
#pragma unroll
                for (int i = 0; i < RM; ++i) y[i] = (have && i < r) ? lds_b[tid * sb + i] : 0.0;
                __syncthreads();
            }
            // ---- y = Q^T b = H1 H0 b (applyHouseholderOnTheLeft, twice; the entries past row r are zero in v0, v1 and b)
            {
                double tmp = y[0];
#pragma unroll
                for (int i = 1; i < RM; ++i) tmp = fma(a0[i], y[i], tmp);
                const double g = tau0 * tmp;
                y[0] -= g;
#pragma unroll
                for (int i = 1; i < RM; ++i) y[i] = fma(-g, a0[i], y[i]);
            }
            if (c > 1) {
                double tmp = y[1];
#pragma unroll
                for (int i = 2; i < RM; ++i) tmp = fma(a1[i], y[i], tmp);
                const double g = tau1 * tmp;
                y[1] -= g;
#pragma unroll
                for (int i = 2; i < RM; ++i) y[i] = fma(-g, a1[i], y[i]);
            }
            if (have) {
                double* o = lds_b + tid * sb;
#pragma unroll
                for (int i = 0; i < RM; ++i)
                    if (i < r) o[i] = y[i];
                // ---- column-oriented back substitution with R (the triangularView<Upper>().solve of _solve_impl, :271) and the
                // permutation: x(perm(k)) = z(k)
                if (c > 1) {
                    const double z1 = y[1] / beta1;
                    const double z0 = fma(-r01, z1, y[0]) / beta0;
                    lds_a[tid * 2 + P] = z0;
                    lds_a[tid * 2 + 1 - P] = z1;
                } else
                    lds_a[tid] = y[0] / beta0;
            }
            __syncthreads();
            // ---- out, in output order.  FullQ: the first c entries of every tile at its columns, the others behind mat_cols (the [U | N]
            // split, :455-471); BlockDiagonalQ: entry k of tile t at its row
            if (qtb) {
                double* dst = qtb + rhs * mat_rows;
                if (q_format == 0) {
                    const int nc = nt * c, m = r - c;
                    for (int e = tid; e < nc; e += 256) {
                        const int tl = c > 1 ? e >> 1 : e;
                        QRK_OUT_STORE(dst + t0 * c + e, lds_b[tl * sb + (e - tl * c)]);
                    }
                    if (m > 0) {
                        const float inv_m = 1.0f / (float)m;
                        double* dn = dst + mat_cols + t0 * (int64_t)m;
                        const int nm = nt * m;
                        for (int e = tid; e < nm; e += 256) {
                            const int tl = (int)(((float)e + 0.5f) * inv_m);
                            QRK_OUT_STORE(dn + e, lds_b[tl * sb + c + (e - tl * m)]);
                        }
                    }
                } else {
                    for (int e = tid; e < nb; e += 256) {
                        const int tl = (int)(((float)e + 0.5f) * inv_r);
                        QRK_OUT_STORE(dst + t0 * (int64_t)r + e, lds_b[tl * sb + (e - tl * r)]);
                    }
                }
            }
            if (x) {
                double* dst = x + rhs * mat_cols + t0 * c;
                const int nc = nt * c;
                for (int e = tid; e < nc; e += 256) QRK_OUT_STORE(dst + e, lds_a[e]);
            }
            __syncthreads();
        }
    }
}

}  // namespace thin_rhs

bool bdqr_thin_rhs_supported(int r, int c, int64_t nrhs) { return r >= c && r <= thin_rhs::RM && c >= 1 && c <= 2 && nrhs >= 1 && nrhs <= BDQR_THIN_RHS_MAX; }

hipError_t launch_bdqr_thin_rhs(int64_t num_tiles, int r, int c, int pivoting, const double* tiles, const double* b, int nrhs, int64_t mat_rows,
                                int64_t mat_cols, int q_format, double* r_vals, int32_t* perm, double* hcoeffs, double* qtb, double* x,
                                int max_blocks, int32_t* redo_count, int32_t* redo_ids, hipStream_t stream)
{
    if (num_tiles <= 0) return hipSuccess;
    int64_t nwg = (num_tiles + 255) / 256;
    if (max_blocks > 0 && nwg > max_blocks) nwg = max_blocks;
    const dim3 grid((unsigned)nwg), block(256);
    const int sin = (r * c) | 1, sb = r | 1;
    const size_t smem = (size_t)256 * (sin + sb) * sizeof(double);      // 57 KB at 9 x 2; 256 x 50 x 8 = 100 KB at 16 x 2
    if (smem > 64 * 1024) {
        static hipError_t attr = [] {
            hipError_t e = hipSuccess;
            const void* fns[4] = {reinterpret_cast<const void*>(thin_rhs::bdqr_thin_rhs_kernel<true, true>), reinterpret_cast<const void*>(thin_rhs::bdqr_thin_rhs_kernel<true, false>),
                                  reinterpret_cast<const void*>(thin_rhs::bdqr_thin_rhs_kernel<false, true>), reinterpret_cast<const void*>(thin_rhs::bdqr_thin_rhs_kernel<false, false>)};
            for (const void* f : fns) if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 4096);
            return e;
        }();
        if (attr != hipSuccess) return attr;
    }
#define QRK_THIN_RHS(P, H)                                                                                                             \
    hipLaunchKernelGGL((thin_rhs::bdqr_thin_rhs_kernel<P, H>), grid, block, smem, stream, num_tiles, r, c, tiles, b, nrhs, mat_rows, \
                       mat_cols, q_format, r_vals, perm, hcoeffs, qtb, x, redo_count, redo_ids)
    if (pivoting) { if (hcoeffs) QRK_THIN_RHS(true, true); else QRK_THIN_RHS(true, false); }
    else { if (hcoeffs) QRK_THIN_RHS(false, true); else QRK_THIN_RHS(false, false); }
#undef QRK_THIN_RHS
    return hipGetLastError();
}

}  // namespace qrk
