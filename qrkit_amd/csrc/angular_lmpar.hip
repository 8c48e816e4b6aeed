// angular_lmpar.hip -- the transposed pass of MINPACK's lmpar on the factors the block-angular solver keeps.
//
// In the pivoted order the damped triangular factor of the block-angular matrix is S^ = [S1 Top; 0 Rg]: S1 block diagonal (the tiles
// qrk_bd_lm_panel writes), Top = top(:, 0:m2), Rg = the upper triangle of the factorised right stack.  lmpar's Newton step needs
// || S^-T u ||^2 with u = D~^2 z, by forward substitution:
//     w1 = S1^-T u1               qrk_bd_solve_rt       bd_solve_rt_thin_kernel / bd_solve_rt_group_kernel + bd_solve_rt_finish_kernel
//     t  = u2 - Top^T w1          qrk_dense_gemv_t      dense_gemv_t_partial_kernel + dense_gemv_t_finish_kernel
//     w2 = Rg^-T t                qrk_dense_solve_rt    dense_solve_rt_kernel
// and its upper bound needs the gradient g2 = Strip(:, P2)^T y1 + R2^T y2: qrk_dense_gemv_t again and qrk_dense_trmv_t
// (dense_trmv_t_kernel).
//
// Every sum is formed in a fixed order: lanes by an xor butterfly, the wavefronts of a workgroup in order, one partial per workgroup,
// the partials in a fixed order by a second kernel.  No floating-point atomics; every grid is a function of the shapes alone.
#include "qrk_device.h"
#include "bd_lm_geom.h"

namespace qrk {
namespace lm {

// Sum of v[n] over the 256 threads of the workgroup (bd_lm.hip's block_sum restated: butterfly inside every wavefront, then the
// four wavefronts in order).  red: 4 N doubles of LDS.
template <int N>
__device__ __forceinline__ void rt_block_sum(double (&v)[N], double* red)
{
#pragma unroll
    for (int n = 0; n < N; ++n) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[n] += __shfl_xor(v[n], o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) red[wave * N + n] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = ((red[n] + red[N + n]) + red[2 * N + n]) + red[3 * N + n];
    __syncthreads();
}

// ---- w_t = R_t^-T u_t, tiles with 1 or 2 columns: one lane per tile, closed form -------------------------------------------------
__global__ void __launch_bounds__(THREADS)
bd_solve_rt_thin_kernel(LmGeom g, const double* __restrict__ r_vals, const double* __restrict__ u, double* __restrict__ w,
                        double* __restrict__ partials)
{
    __shared__ double red[8];
    double acc[2] = {0.0, 0.0};
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < g.num_tiles; t += (int64_t)gridDim.x * THREADS) {
        int c, bc;
        int64_t roff;
        lm_geom(g, t, c, roff, bc);
        const bool two = c == 2;
        const double r00 = r_vals[roff], r01 = two ? r_vals[roff + 1] : 0.0, r11 = two ? r_vals[roff + 2] : 1.0;
        const double u0 = u[bc], u1 = two ? u[bc + 1] : 0.0;
        const bool zero = r00 == 0.0 || r11 == 0.0;
        double w0 = u0 / r00;
        double w1 = two ? fma(-r01, w0, u1) / r11 : 0.0;
        if (zero) { w0 = 0.0; w1 = 0.0; }
        w[bc] = w0;
        if (two) w[bc + 1] = w1;
        acc[0] += fma(w0, w0, w1 * w1);
        acc[1] += zero ? 1.0 : 0.0;
    }
    if (partials) {
        rt_block_sum<2>(acc, red);
        if (threadIdx.x == 0) { partials[2 * blockIdx.x] = acc[0]; partials[2 * blockIdx.x + 1] = acc[1]; }
    }
}

// ---- tiles with up to 32 columns: G lanes per tile (a power of two >= the widest tile, 4 .. 32), lane k = column k -------------------
// The forward substitution of bd_lm_group_kernel's sums[1], restated on the packed triangle as it lies in memory: by columns, one
// broadcast per step.  Column k of R_t is a contiguous run, so lane k reads R(i, k) at step i < k; nothing is kept in register arrays.
__global__ void __launch_bounds__(THREADS)
bd_solve_rt_group_kernel(LmGeom g, int G, const double* __restrict__ r_vals, const double* __restrict__ u, double* __restrict__ w,
                         double* __restrict__ partials)
{
    __shared__ double red[8];
    const int lane = threadIdx.x & 63, jl = lane & (G - 1), gbase = lane & ~(G - 1), slot = threadIdx.x / G, tpb = THREADS / G;
    const int64_t ntg = (g.num_tiles + tpb - 1) / tpb;
    double acc[2] = {0.0, 0.0};
    for (int64_t wi = blockIdx.x; wi < ntg; wi += gridDim.x) {
        const int64_t t = wi * tpb + slot;
        const bool valid = t < g.num_tiles;
        int c, bc;
        int64_t roff;
        lm_geom(g, valid ? t : 0, c, roff, bc);
        if (!valid) c = 0;
        const bool col = jl < c;
        int cw = c;                                   // the widest tile of the wavefront bounds the loop (uniform: the shuffles need it)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const int other = __shfl_xor(cw, o, 64); cw = other > cw ? other : cw; }
        const double* rc = r_vals + roff + (int64_t)(jl * (jl + 1) / 2);
        const double rd = col ? rc[jl] : 1.0;         // R(jl, jl)
        double a = col ? u[bc + jl] : 0.0;
        int rz = (col && rd == 0.0) ? 1 : 0;
        for (int o = G >> 1; o >= 1; o >>= 1) rz |= __shfl_xor(rz, o, 64);
        for (int i = 0; i < cw; ++i) {
            const double wb = __shfl(a / rd, gbase + i, 64);       // w_i, final in lane i since step i - 1
            if (col && jl > i) a = fma(-rc[i], wb, a);
        }
        double wk = a / rd;
        if (rz) wk = 0.0;
        if (col) {
            w[bc + jl] = wk;
            acc[0] = fma(wk, wk, acc[0]);
        }
        if (valid && jl == 0 && rz) acc[1] += 1.0;
    }
    if (partials) {
        rt_block_sum<2>(acc, red);
        if (threadIdx.x == 0) { partials[2 * blockIdx.x] = acc[0]; partials[2 * blockIdx.x + 1] = acc[1]; }
    }
}

// the two partials of `nblocks` workgroups added in a fixed order: one workgroup
__global__ void __launch_bounds__(THREADS)
bd_solve_rt_finish_kernel(const double* __restrict__ partials, int nblocks, double* __restrict__ out)
{
    __shared__ double red[8];
    double v[2] = {0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += THREADS) { v[0] += partials[2 * (int64_t)b]; v[1] += partials[2 * (int64_t)b + 1]; }
    rt_block_sum<2>(v, red);
    if (threadIdx.x == 0) { out[0] = v[0]; out[1] = v[1]; }
}

}  // namespace lm

// Lanes per tile of qrk_bd_solve_rt: 0 = one lane per tile, 4 .. 32 = the group kernel, -1 = not supported
int bd_solve_rt_group_width(int max_cols)
{
    if (max_cols > 32) return -1;
    if (max_cols <= 2) return 0;
    int G = 4;
    while (G < max_cols) G *= 2;
    return G;
}

hipError_t launch_bd_solve_rt(const TileGeom& g, int max_cols, const double* r_vals, const double* u, double* w, double* partials,
                              double* sums2, hipStream_t stream)
{
    const int G = bd_solve_rt_group_width(max_cols);
    if (G < 0) return hipErrorInvalidValue;
    if (g.num_tiles <= 0) return sums2 ? hipMemsetAsync(sums2, 0, 2 * sizeof(double), stream) : hipSuccess;
    const int64_t tpb = G == 0 ? lm::THREADS : lm::THREADS / G;
    const int64_t ntg = (g.num_tiles + tpb - 1) / tpb;
    const int blocks = (int)(ntg < BD_LM_MAX_BLOCKS ? ntg : BD_LM_MAX_BLOCKS);
    double* const part = sums2 ? partials : nullptr;
    const lm::LmGeom lg = lm::lm_geom_of(g);
    if (G == 0)
        hipLaunchKernelGGL(lm::bd_solve_rt_thin_kernel, dim3(blocks), dim3(lm::THREADS), 0, stream, lg, r_vals, u, w, part);
    else
        hipLaunchKernelGGL(lm::bd_solve_rt_group_kernel, dim3(blocks), dim3(lm::THREADS), 0, stream, lg, G, r_vals, u, w, part);
    if (sums2) hipLaunchKernelGGL(lm::bd_solve_rt_finish_kernel, dim3(1), dim3(lm::THREADS), 0, stream, partials, blocks, sums2);
    return hipGetLastError();
}

// ---- out[j] = alpha sum_i A(i, colidx[j]) w[i] + add[j]: a tall-skinny A^T w read once ----------------------------------------------
// Lanes run along the rows (a wavefront loads 512 contiguous bytes of a column), every lane keeps GEMVT_CB column accumulators so that
// w[i] is loaded once per row; a workgroup owns a chunk of rows and a slice of GEMVT_CB columns and leaves one partial per column in
// `work` (work[chunk cols + j]); dense_gemv_t_finish_kernel adds the chunks of a column in a fixed order, one wavefront per column.
namespace gemvt {

constexpr int THREADS = 256;
constexpr int CB = 8;                 // columns per workgroup = accumulators per lane
constexpr int64_t MIN_CHUNK = 256;    // rows per workgroup: a multiple of the workgroup, between these two
constexpr int64_t MAX_CHUNK = 4096;
constexpr int64_t TARGET_WGS = 1024;  // four workgroups per CU when the matrix has the rows for it

__global__ void __launch_bounds__(THREADS)
dense_gemv_t_partial_kernel(const double* __restrict__ A, int64_t lda, int64_t rows, int cols, const int32_t* __restrict__ colidx,
                            const double* __restrict__ w, int64_t chunk, int nslices, double* __restrict__ work)
{
    __shared__ double red[4 * CB];
    const int64_t ci = blockIdx.x / nslices;
    const int j0 = (int)(blockIdx.x - ci * nslices) * CB;
    const int nb = cols - j0 < CB ? cols - j0 : CB;
    const int64_t r0 = ci * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    const double* colp[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) {
        const int j = j0 + (b < nb ? b : 0);
        colp[b] = A + (int64_t)(colidx ? colidx[j] : j) * lda;
    }
    double acc[CB];
#pragma unroll
    for (int b = 0; b < CB; ++b) acc[b] = 0.0;
    if (nb == CB) {
#pragma unroll 4
        for (int64_t i = r0 + threadIdx.x; i < r1; i += THREADS) {
            const double wi = w[i];
#pragma unroll
            for (int b = 0; b < CB; ++b) acc[b] = fma(colp[b][i], wi, acc[b]);
        }
    } else {
#pragma unroll 4
        for (int64_t i = r0 + threadIdx.x; i < r1; i += THREADS) {
            const double wi = w[i];
#pragma unroll
            for (int b = 0; b < CB; ++b)
                if (b < nb) acc[b] = fma(colp[b][i], wi, acc[b]);
        }
    }
#pragma unroll
    for (int b = 0; b < CB; ++b) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[b] += __shfl_xor(acc[b], o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int b = 0; b < CB; ++b) red[wave * CB + b] = acc[b];
    }
    __syncthreads();
    if ((int)threadIdx.x < nb) {
        const int b = threadIdx.x;
        work[ci * cols + j0 + b] = ((red[b] + red[CB + b]) + red[2 * CB + b]) + red[3 * CB + b];
    }
}

__global__ void __launch_bounds__(THREADS)
dense_gemv_t_finish_kernel(const double* __restrict__ work, int64_t nchunks, int cols, double alpha, const double* __restrict__ add,
                           double* __restrict__ out)
{
    const int j = blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= cols) return;                            // (a whole wavefront)
    double s = 0.0;
#pragma unroll 8
    for (int64_t c = lane; c < nchunks; c += 64) s += work[c * cols + j];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[j] = add ? alpha * s + add[j] : alpha * s;
}

static int64_t chunk_rows(int64_t rows, int64_t cols)
{
    const int64_t nslices = (cols + CB - 1) / CB;
    int64_t per = (rows * nslices + TARGET_WGS - 1) / TARGET_WGS;
    per = (per + THREADS - 1) / THREADS * THREADS;
    return per < MIN_CHUNK ? MIN_CHUNK : (per > MAX_CHUNK ? MAX_CHUNK : per);
}

}  // namespace gemvt

// doubles of workspace: one partial per column and per chunk of the smallest chunk size (the grid's own chunk is never smaller)
int64_t dense_gemv_t_work(int64_t rows, int64_t cols)
{
    const int64_t nch = (rows + gemvt::MIN_CHUNK - 1) / gemvt::MIN_CHUNK;
    return (nch < 1 ? 1 : nch) * (cols < 1 ? 1 : cols);
}

hipError_t launch_dense_gemv_t(const double* A, int64_t lda, int64_t rows, int64_t cols, const int32_t* colidx, const double* w,
                               double alpha, const double* add, double* out, double* work, hipStream_t stream)
{
    if (cols <= 0) return hipSuccess;
    const int64_t chunk = gemvt::chunk_rows(rows, cols);
    const int64_t nchunks = (rows + chunk - 1) / chunk, nslices = (cols + gemvt::CB - 1) / gemvt::CB;
    if (cols > 0x7fffffff || nchunks * nslices > 0x7fffffff) return hipErrorInvalidValue;
    if (nchunks > 0)
        hipLaunchKernelGGL(gemvt::dense_gemv_t_partial_kernel, dim3((unsigned)(nchunks * nslices)), dim3(gemvt::THREADS), 0, stream, A, lda, rows,
                           (int)cols, colidx, w, chunk, (int)nslices, work);
    hipLaunchKernelGGL(gemvt::dense_gemv_t_finish_kernel, dim3((unsigned)((cols + 3) / 4)), dim3(gemvt::THREADS), 0, stream, work, nchunks, (int)cols,
                       alpha, add, out);
    return hipGetLastError();
}

// ---- the right triangle, transposed: one workgroup ----------------------------------------------------------------------------------
namespace rt {

constexpr int THREADS = 256;
constexpr int PANEL = 64;

// b <- R^-T b, R = the upper triangle of qr (column j of R is contiguous: b_j = (b_j - sum_{i < j} R(i, j) b_i) / R(j, j)).  Panels of 64
// columns: the four wavefronts subtract what the solved entries contribute to the panel's columns (one column per wavefront at a
// time, butterfly sum), then the first wavefront solves the 64 x 64 triangle by columns with one broadcast per step.  The solved
// entries are read back from b (workgroup-scope visibility behind __syncthreads).  Nothing below the diagonal is read.
__global__ void __launch_bounds__(THREADS)
dense_solve_rt_kernel(const double* __restrict__ qr, int64_t lda, int n, double* b)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j0 = 0; j0 < n; j0 += PANEL) {
        const int pw = n - j0 < PANEL ? n - j0 : PANEL;
        if (j0 > 0) {
            for (int k = wave; k < pw; k += THREADS / 64) {
                const double* rc = qr + (int64_t)(j0 + k) * lda;
                double s = 0.0;
                for (int i = lane; i < j0; i += 64) s = fma(rc[i], b[i], s);
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
                if (lane == 0) b[j0 + k] -= s;
            }
            __syncthreads();
        }
        if (wave == 0) {
            const bool col = lane < pw;
            const double* rc = qr + (int64_t)(j0 + (col ? lane : 0)) * lda + j0;
            const double rd = col ? rc[lane] : 1.0;
            double a = col ? b[j0 + lane] : 0.0;
            for (int i = 0; i < pw; ++i) {
                const double wb = __shfl(a / rd, i, 64);
                if (col && lane > i) a = fma(-rc[i], wb, a);
            }
            if (col) b[j0 + lane] = a / rd;
        }
        __syncthreads();
    }
}

// out[j] += sum_{i <= j} R(i, j) y[i]: one wavefront per column, lanes along the column, butterfly sum
__global__ void __launch_bounds__(THREADS)
dense_trmv_t_kernel(const double* __restrict__ qr, int64_t lda, int n, const double* __restrict__ y, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int j = wave; j < n; j += THREADS / 64) {
        const double* rc = qr + (int64_t)j * lda;
        double s = 0.0;
        for (int i = lane; i <= j; i += 64) s = fma(rc[i], y[i], s);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) out[j] += s;
    }
}

}  // namespace rt

hipError_t launch_dense_solve_rt(const double* qr, int64_t lda, int n, double* b, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rt::dense_solve_rt_kernel, dim3(1), dim3(rt::THREADS), 0, stream, qr, lda, n, b);
    return hipGetLastError();
}

hipError_t launch_dense_trmv_t(const double* qr, int64_t lda, int n, const double* y, double* out, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rt::dense_trmv_t_kernel, dim3(1), dim3(rt::THREADS), 0, stream, qr, lda, n, y, out);
    return hipGetLastError();
}

}  // namespace qrk
