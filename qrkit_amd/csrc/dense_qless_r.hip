// dense_qless_r.hip -- the R factor of a tall-skinny device matrix without Q: qrk_dense_qless_r.
//
// R^T R = A^T A for A (rows x cols, cols <= 32), by Householder reflectors that are never stored: a tree of QR factorisations
// (TSQR), so the condition number is A's and not its square.  The block-angular LM step reduces the fill [F | f] of
// qrk_bd_lm_panel to one (m2 + 1) x (m2 + 1) triangle with it, after which the right stack no longer depends on m1.
//
// One kernel, applied level by level.  A level cuts its input rows into chunks (a multiple of 256 rows); one workgroup of four
// wavefronts reduces a chunk to one cols x cols triangle; the triangles of a level, stacked, are the next level's input matrix
// (in `work`, two buffers used alternately); the last level is one chunk and writes r.  The schedule is host code
// (qless_r_schedule) and a function of (rows, cols) alone: no atomics, no dependence on the device, identical bits for
// identical calls.
//
// Inside a workgroup a wavefront walks its quarter of the chunk in slabs of 64 rows, lane = row, a row's columns in NC
// registers (static indices, loops unrolled); the next slab's loads are issued before the current one is worked on.  The
// wavefront's running triangle T lives next to the slab, row k in lane k.  A slab S is absorbed as the QR of [T; S] with T upper
// triangular: reflector j has v = [v0 at T's row j; S(:, j)], so it costs one wave sum for sigma = |S(:, j)|^2 and one per
// remaining column for v^T x, and T's other rows are not touched.  lm_reflector's rule (bd_lm_geom.h) makes a column whose
// remaining part is zero (a squared norm below DBL_MIN) the identity: zero rows past the end of the matrix, zero columns and an all-zero A cost nothing and give
// no NaN.  The four triangles then meet in LDS and the first wavefront absorbs the other three as slabs.
#include "bd_lm_geom.h"

#include <float.h>

namespace qrk {

// ---- the schedule: plain host code -------------------------------------------------------------------------------------------
constexpr int64_t QLESS_R_SLAB = 256;           // rows a workgroup takes per step (4 wavefronts x 64 lanes): the unit of a chunk
constexpr int64_t QLESS_R_TARGET_WGS = 1024;    // level 1: about four workgroups per CU of a 256-CU part (fixed: not the device's)
constexpr int64_t QLESS_R_INNER_CHUNK = 1024;   // levels >= 2: rows per workgroup ...
constexpr int64_t QLESS_R_INNER_LAST = 2048;    // ... unless one workgroup can take them all
constexpr int QLESS_R_MAX_LEVELS = 4;           // (three occur: level 1 leaves <= 1 025 triangles = 32 800 rows at most, level 2 <= 33, level 3 is one chunk)

// Level l reads level_rows[l] rows in chunks of level_chunk[l] rows; its ceil(rows / chunk) triangles (cols rows each) are the next
// level's rows.  Returns the number of levels (0 for cols <= 0) and writes the first min(levels, cap) entries.
int qless_r_schedule(int64_t rows, int cols, int64_t* level_rows, int64_t* level_chunk, int cap)
{
    if (cols <= 0 || rows < 0) return 0;
    int64_t n = rows;
    int levels = 0;
    for (;;) {
        int64_t chunk;
        if (levels == 0) chunk = (n + QLESS_R_TARGET_WGS - 1) / QLESS_R_TARGET_WGS;
        else chunk = n <= QLESS_R_INNER_LAST ? n : QLESS_R_INNER_CHUNK;
        chunk = (chunk + QLESS_R_SLAB - 1) / QLESS_R_SLAB * QLESS_R_SLAB;
        if (chunk < QLESS_R_SLAB) chunk = QLESS_R_SLAB;
        if (levels < cap) {
            if (level_rows) level_rows[levels] = n;
            if (level_chunk) level_chunk[levels] = chunk;
        }
        ++levels;
        const int64_t nch = (n + chunk - 1) / chunk;
        if (nch <= 1) return levels;
        n = nch * cols;
    }
}

// doubles of workspace: the outputs of levels 1 and 2 next to each other
int64_t dense_qless_r_work(int64_t rows, int cols)
{
    int64_t lr[QLESS_R_MAX_LEVELS], lc[QLESS_R_MAX_LEVELS];
    const int levels = qless_r_schedule(rows, cols, lr, lc, QLESS_R_MAX_LEVELS);
    int64_t need = 0;
    if (levels >= 2) need += lr[1] * cols;
    if (levels >= 3) need += lr[2] * cols;
    return need < 1 ? 1 : need;
}

int dense_qless_r_cap(int cols) { return cols <= 0 || cols > 32 ? -1 : (cols <= 8 ? 8 : (cols <= 16 ? 16 : 32)); }

namespace qless {

constexpr int THREADS = 256;

// Sum over the 64 lanes, the same value in every lane: four DPP steps inside the rows of 16, then the four row sums through
// SGPRs.  A fixed order.
__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);   // row_half_mirror
    v += dpp_f64<0x140>(v);   // row_mirror
    return (readlane_f64(v, 0) + readlane_f64(v, 16)) + (readlane_f64(v, 32) + readlane_f64(v, 48));
}

// k < cols as a scalar compare and branch at the place of use: the unrolled loops test cols some NC^2 / 2 times, and the compiler
// would otherwise compute the NC conditions once, as 64-bit lane masks, and hold them (with the NC masks lane == j: spilled scalars)
__device__ __forceinline__ bool below(int k, int cols)
{
    asm volatile("" : "+s"(cols));
    return k < cols;
}

// [T; S] <- its R factor: T (row k in lane k, t[c] = T(k, c), zero left of the diagonal and in lanes >= cols) stays upper
// triangular, the slab S (a[c] = S(lane, c)) is consumed.
template <int NC>
__device__ __forceinline__ void absorb(double (&t)[NC], double (&a)[NC], int cols, int lane)
{
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (!below(j, cols)) continue;
        const double sigma = wave_sum(a[j] * a[j]);
        // (the same in every lane.  Below the smallest normal number -- zero, or what rounding left of a column that the rows above
        // already span, squared -- 1 / (beta v0) would overflow: the identity, as for an exact zero)
        if (sigma >= DBL_MIN) {
            double beta, v0, gm;
            lm::lm_reflector(readlane_f64(t[j], j), sigma, beta, v0, gm);
            int l = lane;
            asm volatile("" : "+v"(l));                         // (keeps the NC masks lane == j from being computed ahead and held)
            const double vt = l == j ? v0 : 0.0;                // v's entry in T's rows: v0 in row j, zero elsewhere (no branch below)
#pragma unroll
            for (int k = j + 1; k < NC; ++k) {
                if (!below(k, cols)) continue;
                const double w = gm * wave_sum(fma(vt, t[k], a[j] * a[k]));
                a[k] = fma(-w, a[j], a[k]);
                t[k] = fma(-w, vt, t[k]);
            }
            t[j] = l == j ? beta : t[j];
        }
    }
}

// Rows [row, row + 64) of the level's input, zero past `end`
template <int NC>
__device__ __forceinline__ void load_slab(double (&a)[NC], const double* __restrict__ A, int64_t lda, int cols, int64_t row, int64_t end)
{
#pragma unroll
    for (int c = 0; c < NC; ++c) a[c] = 0.0;
    if (row < end) {
        const double* p = A + row;                    // (a per-lane address stepped by lda: NC uniform column bases would fill the scalar file)
#pragma unroll
        for (int c = 0; c < NC; ++c, p += lda) {
            if (below(c, cols)) a[c] = *p;
        }
    }
}

template <int NC>
__global__ void __launch_bounds__(THREADS)
dense_qless_r_kernel(const double* __restrict__ A, int64_t lda, int64_t rows, int cols, int64_t chunk, double* __restrict__ out, int64_t ldo)
{
    __shared__ double tri[3 * NC * NC];               // column c of the three stacked triangles at tri[c * 3 NC ...]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * chunk;
    const int64_t end = r0 + chunk < rows ? r0 + chunk : rows;
    const int64_t per_wave = chunk / 4;               // a multiple of 64
    const int64_t w0 = r0 + wave * per_wave;
    const int64_t w1 = w0 + per_wave < end ? w0 + per_wave : end;

    double t[NC], a[NC], nx[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) t[c] = 0.0;
    if (w0 < w1) {
        load_slab<NC>(nx, A, lda, cols, w0 + lane, w1);
        for (int64_t s = w0; s < w1; s += 64) {
#pragma unroll
            for (int c = 0; c < NC; ++c) a[c] = nx[c];
            if (s + 64 < w1) load_slab<NC>(nx, A, lda, cols, s + 64 + lane, w1);
            absorb<NC>(t, a, cols, lane);
        }
    }
    if (wave > 0 && lane < cols) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (below(c, cols)) tri[c * (3 * NC) + (wave - 1) * cols + lane] = t[c];
        }
    }
    __syncthreads();
    if (wave != 0) return;
    const int stacked = 3 * cols;
    for (int s = 0; s < stacked; s += 64) {
#pragma unroll
        for (int c = 0; c < NC; ++c) a[c] = 0.0;
        if (s + lane < stacked) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                if (below(c, cols)) a[c] = tri[c * (3 * NC) + s + lane];
            }
        }
        absorb<NC>(t, a, cols, lane);
    }
    if (lane < cols) {
        double* o = out + (int64_t)blockIdx.x * cols + lane;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (below(c, cols)) o[(int64_t)c * ldo] = c >= lane ? t[c] : 0.0;
        }
    }
}

}  // namespace qless

hipError_t launch_dense_qless_r(const double* A, int64_t lda, int64_t rows, int cols, double* r, int64_t ldr, double* work, hipStream_t stream)
{
    const int cap = dense_qless_r_cap(cols);
    if (cap < 0) return hipErrorInvalidValue;
    int64_t lr[QLESS_R_MAX_LEVELS], lc[QLESS_R_MAX_LEVELS];
    const int levels = qless_r_schedule(rows, cols, lr, lc, QLESS_R_MAX_LEVELS);
    if (levels < 1 || levels > QLESS_R_MAX_LEVELS) return hipErrorInvalidValue;
    double* const buf[2] = {work, work + (levels >= 2 ? lr[1] * cols : 0)};
    const double* in = A;
    int64_t ldin = lda;
    for (int l = 0; l < levels; ++l) {
        const bool last = l + 1 == levels;
        const int64_t nch = last ? 1 : (lr[l] + lc[l] - 1) / lc[l];
        double* const o = last ? r : buf[l & 1];
        const int64_t ldo = last ? ldr : lr[l + 1];
        const dim3 grid((unsigned)nch), block(qless::THREADS);
        switch (cap) {
        case 8: hipLaunchKernelGGL(qless::dense_qless_r_kernel<8>, grid, block, 0, stream, in, ldin, lr[l], cols, lc[l], o, ldo); break;
        case 16: hipLaunchKernelGGL(qless::dense_qless_r_kernel<16>, grid, block, 0, stream, in, ldin, lr[l], cols, lc[l], o, ldo); break;
        default: hipLaunchKernelGGL(qless::dense_qless_r_kernel<32>, grid, block, 0, stream, in, ldin, lr[l], cols, lc[l], o, ldo); break;
        }
        in = o; ldin = ldo;
    }
    return hipGetLastError();
}

}  // namespace qrk
