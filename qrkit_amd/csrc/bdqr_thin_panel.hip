// bdqr_thin_panel.hip -- factorise uniform batches of tall-thin small tiles (1 or 2 columns, at most 16 rows) and apply Q^T to a WIDE,
// STRIDED panel of columns in the same launch, Q never in memory: one tile per LANE, for gfx950.  Behind qrk_bd_factorize_apply_qt.
//
// Seam in the reference: the left half of QRKit::BlockAngularSparseQR::factorize (src/QRKit/BlockAngularSparseQR.h:459-514) --
// m_leftSolver.compute(J1), then J2.topRows(n1) = Q1^T * J2.topRows(n1) -- with the right-hand side of the Levenberg-Marquardt step
// (examples/ellipse_fitting.cpp:117-142) riding as one more column of the panel.  The explicit route writes sum r^2 doubles of Q1 and
// reads them back for the panel; here a lane keeps its tile's one or two reflectors in registers and walks the panel's columns.
// Per 7 x 2 tile and column: 56 B of the panel in, 56 B out; per tile and launch 112 B of tile in, 24 B of R, 8 B of permutation (+ 16 B of
// tau) out -- times the number of column slices for the tile input (every slice re-derives the reflectors), once for the outputs.
//
// Arithmetic and decisions are bdqr_thin_rhs.hip's, statement for statement (squared norms, the pivot, unclear_reflector, near_best); a
// flagged tile goes to the plan's redo list (bdqr_qless.hip redoes it for the whole panel in Eigen's operation order).
//
// Columns move in GROUPS of G columns (4, 2, 2, 1 for tiles of up to 2, 4, 8, 16 rows) through two LDS areas: the global loads of group g + 1 are issued before
// group g is computed and swept out, and land in the other area after the sweep's stores have been issued, so that a trip never ends
// with the memory pipe empty.  The tile area is dead once the reflectors are in registers: the two areas lie over it.
#include "qrk_device.h"

#include <float.h>

namespace qrk {
namespace thin_panel {

using namespace decide;

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

// the segments of gcur <= G columns of the panel (column g at src + g * ldc, nb entries each): requested into registers ...
template <int RM, int G>
__device__ __forceinline__ void group_request(const double* __restrict__ src, int64_t ldc, int gcur, int r, int nb, int tid, double (&pv)[G][RM])
{
    const int last = nb - 1;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const double* const col = src + g * ldc;
#pragma unroll
        for (int u = 0; u < RM; ++u) {
            const int e = tid + 256 * u;
            pv[g][u] = 0.0;
            if (g < gcur && u < r) pv[g][u] = QRK_TILE_LOAD(col + (e < nb ? e : last));
        }
    }
}
// ... and stored to the LDS area (segment of tile tl of column g at area + g * seg + tl * sb)
template <int RM, int G>
__device__ __forceinline__ void group_land(double* __restrict__ area, int seg, int sb, int gcur, int r, float inv_r, int nb, int tid,
                                           const double (&pv)[G][RM])
{
#pragma unroll
    for (int u = 0; u < RM; ++u) {
        const int e = tid + 256 * u;
        if (u < r && e < nb) {
            const int tl = (int)(((float)e + 0.5f) * inv_r);
            double* const o = area + tl * sb + (e - tl * r);
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < gcur) o[g * seg] = pv[g][u];
        }
    }
}

// One workgroup = 256 lanes = 256 consecutive tiles (blockIdx.x, grid-stride) x one slice of the panel's columns (blockIdx.y: columns
// [y * cps, (y + 1) * cps)).  Every workgroup derives the reflectors of its tiles; slice 0 alone writes R, the permutation and tau and
// appends to the redo list.  The trailing identity rows of Q (mat_rows > the rows the tiles cover) copy the panel through.
template <bool PIVOT, int RM, int G>
__global__ void __launch_bounds__(256, 2)
bdqr_thin_panel_kernel(int64_t num_tiles, int r, int c, const double* __restrict__ tiles, const double* __restrict__ pc, int64_t ldc,
                       int64_t ncols, int cps, int64_t mat_rows, int64_t mat_cols, int q_format, double* __restrict__ r_vals,
                       int32_t* __restrict__ perm, double* __restrict__ hcoeffs, double* __restrict__ qtc, int64_t ldq,
                       int32_t* __restrict__ redo_count, int32_t* __restrict__ redo_ids)
{
    extern __shared__ double thin_panel_lds[];
    const int tid = threadIdx.x;
    const int rc = r * c;
    const int sin = rc | 1;              // LDS stride of a tile's input (odd)
    const int sb = r | 1;                // LDS stride of a tile's segment of a column (odd)
    const int seg = 256 * sb;            // one column of the workgroup in an area
    double* const lds_a = thin_panel_lds;                      // [256][sin] tiles in; dead after the reflectors are in registers
    double* const area0 = thin_panel_lds;                      // [G][256][sb], over the tile area
    double* const area1 = thin_panel_lds + G * seg;
    const float inv_r = 1.0f / (float)r;
    const bool slice0 = blockIdx.y == 0;
    const int64_t j0 = (int64_t)blockIdx.y * cps;
    const int64_t j1 = j0 + cps < ncols ? j0 + cps : ncols;
    if (!slice0 && j0 >= j1) return;
    {
        const int64_t sum_rows = num_tiles * r, ntail = mat_rows - sum_rows;
        const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x, nwg = (int64_t)gridDim.x * gridDim.y;
        for (int64_t i = wg * 256 + tid; i < ntail * ncols; i += nwg * 256) {
            const int64_t j = i / ntail, k = i - j * ntail;
            qtc[j * ldq + sum_rows + k] = pc[j * ldc + sum_rows + k];
        }
    }
    const int ngroups = (int)((j1 - j0 + G - 1) / G);
    for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < num_tiles; t0 += (int64_t)gridDim.x * 256) {
        const int nt = (int)(num_tiles - t0 < 256 ? num_tiles - t0 : 256);
        const int nb = nt * r;           // entries of a column of this workgroup: at most 16 per thread
        const double* const csrc = pc + t0 * (int64_t)r;
        // ---- in: the first group of columns is requested first and stored last, so that it travels with the tiles
        double pv[G][RM];
        if (ngroups > 0) {
            const int g0 = (int)(j1 - j0 < G ? j1 - j0 : G);
            group_request<RM, G>(csrc + j0 * ldc, ldc, g0, r, nb, tid, pv);
        }
        {
            // (bdqr_thin.hip's copy: all the loads of a thread issued before the first one is waited for, clamped addresses)
            const double* src = tiles + t0 * (int64_t)rc;
            const int n = nt * rc;
            if ((rc & 1) == 0 && (reinterpret_cast<uintptr_t>(tiles) & 15u) == 0) {
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
        __syncthreads();
        const int64_t t = t0 + tid;
        const bool have = tid < nt;
        double a0[RM], a1[RM];
#pragma unroll
        for (int i = 0; i < RM; ++i) {
            a0[i] = (have && i < r) ? lds_a[tid * sin + i] : 0.0;
            a1[i] = (have && c > 1 && i < r) ? lds_a[tid * sin + r + i] : 0.0;
        }
        __syncthreads();                 // (the tile area is dead: the column areas go over it)
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
        if (have && slice0) {
            // ---- a decision inside its error margin: the exact path redoes the tile (its outputs, of every slice, are overwritten)
            if (unclear) redo_ids[atomicAdd(redo_count, 1)] = (int32_t)t;
            // ---- R (packed upper triangle by columns), permutation, tau
            double* rv = r_vals + t * (int64_t)(c * (c + 1) / 2);
            rv[0] = beta0;
            if (c > 1) { rv[1] = r01; rv[2] = beta1; }
            const int cbase = (int)(t * c);
            perm[cbase] = cbase + P;
            if (c > 1) perm[cbase + 1] = cbase + 1 - P;
            if (hcoeffs) { hcoeffs[cbase] = tau0; if (c > 1) hcoeffs[cbase + 1] = tau1; }
        }
        if (ngroups > 0) {
            const int g0 = (int)(j1 - j0 < G ? j1 - j0 : G);
            group_land<RM, G>(area0, seg, sb, g0, r, inv_r, nb, tid, pv);
        }
        __syncthreads();
        for (int gi = 0; gi < ngroups; ++gi) {
            double* const cur = (gi & 1) ? area1 : area0;
            double* const nxt = (gi & 1) ? area0 : area1;
            const int64_t jg = j0 + (int64_t)gi * G;
            const int gcur = (int)(j1 - jg < G ? j1 - jg : G);
            const int64_t jn = jg + G;
            const int gnext = gi + 1 < ngroups ? (int)(j1 - jn < G ? j1 - jn : G) : 0;
            // the next group's loads go out before this group is touched
            if (gnext > 0) group_request<RM, G>(csrc + jn * ldc, ldc, gnext, r, nb, tid, pv);
            for (int g = 0; g < gcur; ++g) {
                double* const o = cur + g * seg + tid * sb;
                double y[RM];
#pragma unroll
                for (int i = 0; i < RM; ++i) y[i] = (have && i < r) ? o[i] : 0.0;
                // ---- y = Q^T c_j = H1 H0 c_j (applyHouseholderOnTheLeft, twice; the entries past row r are zero in v0, v1 and c_j)
                {
                    double tmp = y[0];
#pragma unroll
                    for (int i = 1; i < RM; ++i) tmp = fma(a0[i], y[i], tmp);
                    const double gg = tau0 * tmp;
                    y[0] -= gg;
#pragma unroll
                    for (int i = 1; i < RM; ++i) y[i] = fma(-gg, a0[i], y[i]);
                }
                if (c > 1) {
                    double tmp = y[1];
#pragma unroll
                    for (int i = 2; i < RM; ++i) tmp = fma(a1[i], y[i], tmp);
                    const double gg = tau1 * tmp;
                    y[1] -= gg;
#pragma unroll
                    for (int i = 2; i < RM; ++i) y[i] = fma(-gg, a1[i], y[i]);
                }
                if (have) {
#pragma unroll
                    for (int i = 0; i < RM; ++i)
                        if (i < r) o[i] = y[i];
                }
            }
            __syncthreads();
            // ---- out, in output order.  FullQ: the first c entries of every tile at its columns, the others behind mat_cols (the [U | N]
            // split, BlockDiagonalSparseQR.h:455-471); BlockDiagonalQ: entry k of tile t at its row
            for (int g = 0; g < gcur; ++g) {
                const double* const lb = cur + g * seg;
                double* const dst = qtc + (jg + g) * ldq;
                if (q_format == 0) {
                    const int nc = nt * c, m = r - c;
                    for (int e = tid; e < nc; e += 256) {
                        const int tl = c > 1 ? e >> 1 : e;
                        QRK_OUT_STORE(dst + t0 * c + e, lb[tl * sb + (e - tl * c)]);
                    }
                    if (m > 0) {
                        const float inv_m = 1.0f / (float)m;
                        double* dn = dst + mat_cols + t0 * (int64_t)m;
                        const int nm = nt * m;
                        for (int e = tid; e < nm; e += 256) {
                            const int tl = (int)(((float)e + 0.5f) * inv_m);
                            QRK_OUT_STORE(dn + e, lb[tl * sb + c + (e - tl * m)]);
                        }
                    }
                } else {
                    for (int e = tid; e < nb; e += 256) {
                        const int tl = (int)(((float)e + 0.5f) * inv_r);
                        QRK_OUT_STORE(dst + t0 * (int64_t)r + e, lb[tl * sb + (e - tl * r)]);
                    }
                }
            }
            // (the other area was swept out one trip ago, before that trip's closing barrier)
            if (gnext > 0) group_land<RM, G>(nxt, seg, sb, gnext, r, inv_r, nb, tid, pv);
            __syncthreads();
        }
    }
}

}  // namespace thin_panel

bool bdqr_thin_panel_supported(int r, int c) { return r >= c && r <= 16 && c >= 1 && c <= 2; }

ThinPanelGrid bdqr_thin_panel_grid(int64_t num_tiles, int r, int c, int64_t ncols, int num_cus)
{
    ThinPanelGrid pg{};
    const int sin = (r * c) | 1, sb = r | 1;
    pg.group = r <= 2 ? 4 : (r <= 8 ? 2 : 1);             // (the instantiations of launch_bdqr_thin_panel)
    int64_t chunks = (num_tiles + 255) / 256;
    if (chunks > (int64_t)num_cus * 32) chunks = (int64_t)num_cus * 32;      // (bdqr_thin_rhs's cap; the kernel strides over the rest)
    if (chunks < 1) chunks = 1;
    pg.chunks = (int)chunks;
    // When the tile chunks alone leave CUs idle the panel's columns are cut into slices of whole groups, up to the workgroups that are
    // resident at once: two per CU (a workgroup holds up to 70 KB of the CU's 160 KB of LDS; bdqr_thin_rhs's 57 KB at 9 x 2 gives the same)
    const int64_t target = 2 * (int64_t)num_cus;
    int64_t slices = (target + chunks - 1) / chunks;
    const int64_t groups = (ncols + pg.group - 1) / pg.group;
    if (slices > groups) slices = groups;
    if (slices < 1) slices = 1;
    int64_t cps = ((groups + slices - 1) / slices) * pg.group;           // columns per slice: whole groups
    if (cps < pg.group) cps = pg.group;
    if (cps > 0x7fffffff) cps = 0x7fffffff / pg.group * pg.group;
    slices = ncols > 0 ? (ncols + cps - 1) / cps : 1;
    if (slices > 65535) { slices = 65535; cps = (((ncols + slices - 1) / slices + pg.group - 1) / pg.group) * pg.group; slices = (ncols + cps - 1) / cps; }
    pg.slices = (int)slices;
    pg.cols_per_slice = (int)cps;
    const size_t tile_area = (size_t)256 * sin, col_areas = (size_t)2 * pg.group * 256 * sb;
    pg.smem = (tile_area > col_areas ? tile_area : col_areas) * sizeof(double);     // 57 KB at 7 x 2, 73.7 KB at 8 x 2 (G = 2), 69.6 KB at 16 x 2 (G = 1)
    return pg;
}

hipError_t launch_bdqr_thin_panel(int64_t num_tiles, int r, int c, int pivoting, const double* tiles, const double* pc, int64_t ldc,
                                  int64_t ncols, int64_t mat_rows, int64_t mat_cols, int q_format, double* r_vals, int32_t* perm,
                                  double* hcoeffs, double* qtc, int64_t ldq, int num_cus, int32_t* redo_count, int32_t* redo_ids,
                                  hipStream_t stream)
{
    if (num_tiles <= 0) return hipSuccess;
    if (!bdqr_thin_panel_supported(r, c)) return hipErrorInvalidValue;
    const ThinPanelGrid pg = bdqr_thin_panel_grid(num_tiles, r, c, ncols, num_cus);
    const dim3 grid((unsigned)pg.chunks, (unsigned)pg.slices), block(256);
    if (pg.smem > 64 * 1024) {
        static hipError_t attr = [] {
            hipError_t e = hipSuccess;
            const void* fns[4] = {reinterpret_cast<const void*>(thin_panel::bdqr_thin_panel_kernel<true, 8, 2>), reinterpret_cast<const void*>(thin_panel::bdqr_thin_panel_kernel<true, 16, 1>),
                                  reinterpret_cast<const void*>(thin_panel::bdqr_thin_panel_kernel<false, 8, 2>), reinterpret_cast<const void*>(thin_panel::bdqr_thin_panel_kernel<false, 16, 1>)};
            for (const void* f : fns) if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
            return e;
        }();
        if (attr != hipSuccess) return attr;
    }
#define QRK_THIN_PANEL(P, R, GG)                                                                                                            \
    hipLaunchKernelGGL((thin_panel::bdqr_thin_panel_kernel<P, R, GG>), grid, block, pg.smem, stream, num_tiles, r, c, tiles, pc, ldc, ncols, \
                       pg.cols_per_slice, mat_rows, mat_cols, q_format, r_vals, perm, hcoeffs, qtc, ldq, redo_count, redo_ids)
#define QRK_THIN_PANEL_R(P)                                                    \
    do {                                                                       \
        if (r <= 2) QRK_THIN_PANEL(P, 2, 4);                                   \
        else if (r <= 4) QRK_THIN_PANEL(P, 4, 2);                              \
        else if (r <= 8) QRK_THIN_PANEL(P, 8, 2);                              \
        else QRK_THIN_PANEL(P, 16, 1);                                         \
    } while (0)
    if (pivoting) QRK_THIN_PANEL_R(true); else QRK_THIN_PANEL_R(false);
#undef QRK_THIN_PANEL_R
#undef QRK_THIN_PANEL
    return hipGetLastError();
}

}  // namespace qrk
