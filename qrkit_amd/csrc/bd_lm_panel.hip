// bd_lm_panel.hip -- the damped elimination of the block-diagonal factors applied to a PANEL of columns: the left
// half of the Levenberg-Marquardt damped solve on the factors the block-angular solver keeps (BlockAngularSparseQR.h:459-514 with
// the lmpar / qrsolv of examples/ellipse_fitting.cpp:257-280 on top).  Behind qrk_bd_lm_panel; qrk_dense_lm_stack's kernel is at
// the end of the file.
//
// Per tile t (c columns, first column base_col, Dt = diag permuted by the tile's pivoting) the stack [R_t; sqrt(par) Dt] is
// triangularised by bd_lm.hip's reflectors (K9: reflector k lives on R(k, k) and on k + 1 rows of the lower part, kept
// un-normalised as (v0, gm, l)), and the same reflectors go over the tile's c rows of a panel C stacked on c zero rows:
//     H_{c-1} ... H_0 [R_t  C_t]   [S_t  top_t ]
//                     [sDt  0  ] = [0    fill_t]
// s_vals receives S_t in r_vals' layout, top and fill the two c x ncols results at the tile's rows.  Nothing is summed: no atomics,
// no partials; the grid is a function of the plan and ncols.
//
// par = 0: sigma = 0 for every reflector, so v0 = gm = 0, every w below is an exact zero, s_vals and top are copies and fill is
// +0.0 (a fill leaves as f + 0.0, which is f for every f but -0.0).
#include "qrk_device.h"
#include "bd_lm_geom.h"

namespace qrk {
namespace lm {

// ---- tiles with 1 or 2 columns: one lane per tile, the reflectors in closed form in registers (lm_thin_tiles' statements) -------
// grid.x = chunks of 256 tiles, grid.y = slices of `cps` panel columns; slice 0 alone writes s_vals.  Per tile and column the lane
// loads c doubles and stores 2 c; consecutive lanes read consecutive addresses of a column.  The columns move in batches of U: the
// loads of batch b + 1 are issued before batch b is computed and stored, so the memory pipe is never drained inside the loop.
constexpr int PANEL_U = 4;

__device__ __forceinline__ void thin_panel_request(const double* __restrict__ c, int64_t ldc, const int32_t* __restrict__ colidx,
                                                   int64_t j, int64_t j1, int bc, bool two, bool have, double (&v)[PANEL_U][2])
{
#pragma unroll
    for (int u = 0; u < PANEL_U; ++u) {
        v[u][0] = 0.0; v[u][1] = 0.0;
        if (have && j + u < j1) {
            const int64_t col = colidx ? (int64_t)colidx[j + u] : j + u;
            const double* const src = c + col * ldc + bc;
            v[u][0] = src[0];
            if (two) v[u][1] = src[1];
        }
    }
}

__global__ void __launch_bounds__(THREADS)
bd_lm_panel_thin_kernel(LmGeom g, const double* __restrict__ r_vals, const int32_t* __restrict__ perm,
                        const double* __restrict__ diag, double par, const double* __restrict__ c, int64_t ldc, int64_t ncols, int cps,
                        const int32_t* __restrict__ colidx, double* __restrict__ s_vals, double* __restrict__ top, int64_t ldt,
                        double* __restrict__ fill, int64_t ldf)
{
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool have = t < g.num_tiles;
    const int64_t j0 = (int64_t)blockIdx.y * cps;
    const int64_t j1 = j0 + cps < ncols ? j0 + cps : ncols;
    int cc = 1, bc = 0;
    int64_t roff = 0;
    if (have) lm_geom(g, t, cc, roff, bc);
    const bool two = cc == 2;
    // the first batch of the panel travels with the factors
    double cur[PANEL_U][2];
    thin_panel_request(c, ldc, colidx, j0, j1, bc, two, have, cur);
    const double sp = sqrt(par);
    double r00 = 1.0, r01 = 0.0, r11 = 1.0, d0 = 1.0, d1 = 1.0;
    if (have) {
        r00 = r_vals[roff];
        if (two) { r01 = r_vals[roff + 1]; r11 = r_vals[roff + 2]; }
        if (diag) { d0 = diag[perm[bc]]; if (two) d1 = diag[perm[bc + 1]]; }
    }
    // reflector 0 on [r00; sp d0]: column 1 gets a fill in row 0 of the lower part
    const double l0 = sp * d0;
    double s00, va, ga;
    lm_reflector(r00, l0 * l0, s00, va, ga);
    const double w01 = va * r01 * ga;
    const double s01 = fma(-w01, va, r01), l01 = -w01 * l0;
    // reflector 1 on [r11; l01; sp d1]
    const double l1 = sp * d1;
    double s11, vb, gb;
    lm_reflector(r11, fma(l01, l01, l1 * l1), s11, vb, gb);
    if (have && blockIdx.y == 0) {
        s_vals[roff] = s00;
        if (two) { s_vals[roff + 1] = s01; s_vals[roff + 2] = s11; }
    }
    for (int64_t j = j0; j < j1; j += PANEL_U) {
        double nxt[PANEL_U][2];
        thin_panel_request(c, ldc, colidx, j + PANEL_U, j1, bc, two, have, nxt);
#pragma unroll
        for (int u = 0; u < PANEL_U; ++u) {
            if (have && j + u < j1) {
                const double y0 = cur[u][0], y1 = cur[u][1];
                double w = va * y0 * ga;
                const double t0 = fma(-w, va, y0), f0 = -w * l0;
                double* const to = top + (j + u) * ldt + bc;
                double* const fo = fill + (j + u) * ldf + bc;
                to[0] = t0;
                if (two) {
                    w = fma(l01, f0, vb * y1) * gb;
                    to[1] = fma(-w, vb, y1);
                    fo[0] = fma(-w, l01, f0) + 0.0;
                    fo[1] = -w * l1 + 0.0;
                } else {
                    fo[0] = f0 + 0.0;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PANEL_U; ++u) { cur[u][0] = nxt[u][0]; cur[u][1] = nxt[u][1]; }
    }
}

// ---- tiles with up to 32 columns: CAP lanes per tile, THREADS / CAP tiles per workgroup ---------------------------------------------
// Phase A, lane = column j of R: K9's elimination.  Lane j holds column j of R in registers (row k of R is untouched until reflector
// k, so the unrolled step k indexes it statically) and column j of the lower part, packed, in LDS; R's diagonal is in LDS from the
// start.  At step k every lane j >= k derives reflector k from column k of the lower part (final since step k - 1) -- the same
// statements on the same values in every lane -- lane k parks (v0, gm) for phase B, the lanes j > k update their column; one barrier
// per step.  Then s_vals leaves, a contiguous run of the packed triangle per lane.
// Phase B, lane = (tile, panel column): the tile's c entries of the column and the c fills in registers, the reflectors read from
// LDS (column k of the lower part IS reflector k's tail).  A workgroup serves CAP panel columns of its tiles per trip.
// LDS: TPB (CAP (CAP + 1) / 2 + 3 CAP) doubles = 15.4 / 23.6 / 39.9 KB for CAP = 8 / 16 / 32.  No scratch.
template <int CAP>
__global__ void __launch_bounds__(THREADS)
bd_lm_panel_group_kernel(LmGeom g, const double* __restrict__ r_vals, const int32_t* __restrict__ perm,
                         const double* __restrict__ diag, double par, const double* __restrict__ c, int64_t ldc, int64_t ncols, int cps,
                         const int32_t* __restrict__ colidx, double* __restrict__ s_vals, double* __restrict__ top, int64_t ldt,
                         double* __restrict__ fill, int64_t ldf)
{
    constexpr int TPB = THREADS / CAP;
    constexpr int TRI = CAP * (CAP + 1) / 2;
    __shared__ double Ls[TPB][TRI];                   // column k of the lower part at k (k + 1) / 2, k + 1 entries
    __shared__ double Rd[TPB][CAP], V0[TPB][CAP], GM[TPB][CAP];
    const int kmax = g.t_cols ? CAP : (g.cols < CAP ? g.cols : CAP);     // steps of the unrolled loops (workgroup-uniform)
    {
        const int jl = threadIdx.x & (CAP - 1), slot = threadIdx.x / CAP;
        const int64_t t = (int64_t)blockIdx.x * TPB + slot;
        const bool valid = t < g.num_tiles;
        int cc = 0, bc = 0;
        int64_t roff = 0;
        if (valid) lm_geom(g, t, cc, roff, bc);
        const bool col = jl < cc;
        const int64_t coff = roff + (int64_t)(jl * (jl + 1) / 2);
        double Rc[CAP];
#pragma unroll
        for (int i = 0; i < CAP; ++i) {
            double v = 0.0;
            if (col && i <= jl) v = r_vals[coff + i];
            Rc[i] = v;
        }
        double* const Lt = Ls[slot];
        double* const own = Lt + jl * (jl + 1) / 2;
        if (col) {
            const double dj = diag ? diag[perm[bc + jl]] : 1.0;
            own[jl] = sqrt(par) * dj;                 // entry (j, j) of the lower part; the entries above it are fill, first assigned below
            Rd[slot][jl] = r_vals[coff + jl];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CAP; ++k) {
            if (k < kmax) {
                if (col && jl >= k) {
                    const double* const lk = Lt + k * (k + 1) / 2;
                    const double lkk = lk[k];
                    double sigma = lkk * lkk;
                    for (int i = 0; i < k; ++i) sigma = fma(lk[i], lk[i], sigma);
                    double beta, v0, gm;
                    lm_reflector(Rd[slot][k], sigma, beta, v0, gm);
                    if (jl == k) {
                        Rc[k] = beta;
                        V0[slot][k] = v0; GM[slot][k] = gm;
                    } else {
                        double dot = v0 * Rc[k];
                        for (int i = 0; i < k; ++i) dot = fma(lk[i], own[i], dot);
                        const double wv = dot * gm;
                        Rc[k] = fma(-wv, v0, Rc[k]);
                        for (int i = 0; i < k; ++i) own[i] = fma(-wv, lk[i], own[i]);
                        own[k] = -wv * lkk;
                    }
                }
                __syncthreads();
            }
        }
        if (col && blockIdx.y == 0) {
#pragma unroll
            for (int i = 0; i < CAP; ++i)
                if (i <= jl) s_vals[coff + i] = Rc[i];
        }
    }
    // ---- phase B
    const int slot = threadIdx.x % TPB, pc = threadIdx.x / TPB;
    const int64_t t = (int64_t)blockIdx.x * TPB + slot;
    if (t >= g.num_tiles) return;
    int cc, bc;
    int64_t roff;
    lm_geom(g, t, cc, roff, bc);
    const double* const Lt = Ls[slot];
    const int64_t j0 = (int64_t)blockIdx.y * cps;
    const int64_t j1 = j0 + cps < ncols ? j0 + cps : ncols;
    for (int64_t j = j0 + pc; j < j1; j += CAP) {
        const int64_t cj = colidx ? (int64_t)colidx[j] : j;
        const double* const src = c + cj * ldc + bc;
        // cc again behind an empty asm (bd_lm.hip's device): the lane predicates i < cc of the unrolled loops do not depend on the
        // column, and hoisted out of the column loop they would occupy two scalar registers each
        int cv = cc;
        asm volatile("" : "+v"(cv));
        double y[CAP], f[CAP];
#pragma unroll
        for (int i = 0; i < CAP; ++i) {
            double v = 0.0;
            if (i < cv) v = src[i];
            y[i] = v; f[i] = 0.0;
        }
        asm volatile("" : "+v"(cv));
#pragma unroll
        for (int k = 0; k < CAP; ++k) {
            if (k < kmax && k < cv) {
                const double* const lk = Lt + k * (k + 1) / 2;
                const double v0 = V0[slot][k], gm = GM[slot][k];
                double dot = v0 * y[k];
#pragma unroll
                for (int i = 0; i < k; ++i) dot = fma(lk[i], f[i], dot);
                const double wv = dot * gm;
                y[k] = fma(-wv, v0, y[k]);
#pragma unroll
                for (int i = 0; i < k; ++i) f[i] = fma(-wv, lk[i], f[i]);
                f[k] = -wv * lk[k];
            }
        }
        double* const to = top + j * ldt + bc;
        double* const fo = fill + j * ldf + bc;
        asm volatile("" : "+v"(cv));
#pragma unroll
        for (int i = 0; i < CAP; ++i) {
            if (i < cv) { to[i] = y[i]; fo[i] = f[i] + 0.0; }
        }
    }
}

// ---- qrk_dense_lm_stack: the 2 m2 rows of the right stack G ((m2 + m1 + m2) x (m2 + 1)) that are not the panel kernel's ---------------
// rows 0 .. m2: [triu(R2) | y2] (the reflectors below R2's diagonal in the packed QR stay out); rows m2 + m1 ..: [sqrt(par) D2(P2) | 0]
__global__ void __launch_bounds__(THREADS)
dense_lm_stack_kernel(const double* __restrict__ qr, int64_t lda, int m2, const double* __restrict__ y2, const double* __restrict__ diag2,
                      const int32_t* __restrict__ perm2, double par, int64_t m1, double* __restrict__ gs, int64_t ldg)
{
    const int64_t n = 2 * (int64_t)m2 * ((int64_t)m2 + 1);
    const double sp = sqrt(par);
    for (int64_t e = (int64_t)blockIdx.x * THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * THREADS) {
        const int64_t j = e / (2 * (int64_t)m2);
        const int i = (int)(e - j * 2 * (int64_t)m2);
        double v = 0.0;
        if (i < m2) {
            if (j == m2) v = y2[i];
            else if (i <= j) v = qr[j * lda + i];
            gs[j * ldg + i] = v;
        } else {
            const int k = i - m2;
            if (k == j) v = sp * (diag2 ? diag2[perm2 ? perm2[k] : k] : 1.0);
            gs[j * ldg + m2 + m1 + k] = v;
        }
    }
}

}  // namespace lm

// The kernel of qrk_bd_lm_panel for a plan whose widest tile has max_cols columns: 0 = bd_lm_panel_thin_kernel, 8 / 16 / 32 =
// bd_lm_panel_group_kernel<CAP>, -1 = not supported (more than 32 columns)
int bd_lm_panel_cap(int max_cols)
{
    if (max_cols <= 2) return 0;
    if (max_cols <= 8) return 8;
    if (max_cols <= 16) return 16;
    return max_cols <= 32 ? 32 : -1;
}

// grid.x = workgroups over the tiles; grid.y = slices of whole batches of panel columns, cut (as bdqr_thin_panel_grid cuts them) when
// the tile workgroups alone leave the chip idle: up to four resident workgroups per CU.  A function of the plan and ncols.
LmPanelGrid bd_lm_panel_grid(int64_t num_tiles, int max_cols, int64_t ncols, int num_cus)
{
    LmPanelGrid pg{};
    const int cap = bd_lm_panel_cap(max_cols);
    const int tpb = cap <= 0 ? lm::THREADS : lm::THREADS / cap, group = cap <= 0 ? lm::PANEL_U : cap;
    int64_t chunks = (num_tiles + tpb - 1) / tpb;      // (mat_cols is an int32: at most 2^31 / tpb workgroups)
    if (chunks < 1) chunks = 1;
    const int64_t target = 4 * (int64_t)num_cus;
    int64_t slices = (target + chunks - 1) / chunks;
    const int64_t groups = (ncols + group - 1) / group;
    if (slices > groups) slices = groups;
    if (slices < 1) slices = 1;
    int64_t cps = ((groups + slices - 1) / slices) * group;
    if (cps < group) cps = group;
    if (cps > 0x7fffffff) cps = 0x7fffffff / group * group;
    slices = ncols > 0 ? (ncols + cps - 1) / cps : 1;
    if (slices > 65535) { slices = 65535; cps = (((ncols + slices - 1) / slices + group - 1) / group) * group; slices = (ncols + cps - 1) / cps; }
    pg.chunks = (int)chunks; pg.slices = (int)slices; pg.cols_per_slice = (int)cps;
    return pg;
}

hipError_t launch_bd_lm_panel(const TileGeom& g, int max_cols, const double* r_vals, const int32_t* perm, const double* diag, double par,
                              const double* c, int64_t ldc, int64_t ncols, const int32_t* colidx, double* s_vals, double* top, int64_t ldt,
                              double* fill, int64_t ldf, int num_cus, hipStream_t stream)
{
    const int cap = bd_lm_panel_cap(max_cols);
    if (cap < 0) return hipErrorInvalidValue;
    if (g.num_tiles <= 0) return hipSuccess;
    const LmPanelGrid pg = bd_lm_panel_grid(g.num_tiles, max_cols, ncols, num_cus);
    const dim3 grid((unsigned)pg.chunks, (unsigned)pg.slices), block(lm::THREADS);
    const lm::LmGeom lg = lm::lm_geom_of(g);
#define QRK_LM_PANEL(CAP) case CAP: hipLaunchKernelGGL((lm::bd_lm_panel_group_kernel<CAP>), grid, block, 0, stream, lg, r_vals, perm, diag, par, c, ldc, ncols, pg.cols_per_slice, colidx, s_vals, top, ldt, fill, ldf); break;
    switch (cap) {
    case 0: hipLaunchKernelGGL(lm::bd_lm_panel_thin_kernel, grid, block, 0, stream, lg, r_vals, perm, diag, par, c, ldc, ncols, pg.cols_per_slice, colidx, s_vals, top, ldt, fill, ldf); break;
    QRK_LM_PANEL(8) QRK_LM_PANEL(16) QRK_LM_PANEL(32)
    default: break;
    }
#undef QRK_LM_PANEL
    return hipGetLastError();
}

hipError_t launch_dense_lm_stack(const double* qr, int64_t lda, int m2, const double* y2, const double* diag2, const int32_t* perm2,
                                 double par, int64_t m1, double* gs, int64_t ldg, hipStream_t stream)
{
    if (m2 <= 0) return hipSuccess;
    const int64_t n = 2 * (int64_t)m2 * ((int64_t)m2 + 1);
    int64_t blocks = (n + lm::THREADS - 1) / lm::THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(lm::dense_lm_stack_kernel, dim3((unsigned)blocks), dim3(lm::THREADS), 0, stream, qr, lda, m2, y2, diag2, perm2, par, m1, gs, ldg);
    return hipGetLastError();
}

}  // namespace qrk
