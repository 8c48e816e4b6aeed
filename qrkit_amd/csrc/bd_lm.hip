// bd_lm.hip -- the Levenberg-Marquardt trust-region step on the factors of the block-diagonal solver (DESIGN.md K9;
// MINPACK's lmpar over them as one enqueue, its scalar steps on the device: K10).
//
// Between two factorisations Eigen::LevenbergMarquardt (examples/ellipse_fitting.cpp:257-280, bench/bench_sparse_qr_extra.cpp:303-346)
// runs MINPACK's lmpar on matrixR(), colsPermutation() and Q^T f: up to ten times a damped solve
//     min || R P^T x - Q^T f ||^2 + par || D x ||^2                                                  (MINPACK qrsolv)
// the norm || D x || and one triangular solve with the damped factor.  For a block-diagonal R all of it is block-local apart from
// two global sums, and it reads c (c + 1) / 2 + 3 c doubles per tile (R, y, the permutation, diag) -- no tile, no Q, no reflector.
//
// Per tile (c columns, first column base_col, z in the pivoted order, dt_k = diag[perm[base_col + k]]):
//   * the stack [R; sqrt(par) Dt] is triangularised by c Householder reflectors.  Row k of R is untouched until reflector k, and
//     the lower part stays upper triangular (reflector k fills row k of it), so reflector k lives on R(k, k) and k + 1 rows of the
//     lower part.  The reflector is kept un-normalised: H = I - g v v^T, v = [R(k,k) - beta; l], g = -1 / (beta v_0).
//   * z = S^-1 (top of the transformed right-hand side), zero from the first exact zero on S's diagonal on (MINPACK's nsing rule;
//     with par > 0 and a positive diag there is none, with par = 0 S = R);
//   * sums[0] += sum (dt_k z_k)^2, sums[1] += || S^-T (Dt^2 z) ||^2 (tiles without a zero on S's diagonal), sums[2] += 1 for a tile
//     with an exact zero on R's diagonal.
// Squares are formed directly (no scaling against overflow), as everywhere in the fast kernels of this library.
//
// The sums are deterministic: every workgroup adds its lanes in a fixed order into one partial per sum (a scratch the plan owns),
// a one-workgroup pass adds the partials in a fixed order; no floating-point atomics; the grid is a function of the plan.
#include "qrk_device.h"
#include "bd_lm_geom.h"     // LmGeom, lm_geom, lm_reflector, THREADS: shared with bd_lm_panel.hip

namespace qrk {
namespace lm {

// Sum of v[n] over the 256 threads of the workgroup in a fixed order: xor butterfly inside every wavefront (the same bits in all of
// its lanes), then the four wavefronts in order.  red: 4 N doubles of LDS.
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* red)
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

// ---- tiles with 1 or 2 columns: one lane per tile (the 10^6-tile LM shape; R is 1 or 3 doubles) ---------------------------------
// The body of bd_lm_thin_kernel (par a kernel argument) and of bd_lm_thin_ctl_kernel / bd_lm_thin_last_kernel (par from the control
// block of the device-side lmpar, below)
__device__ __forceinline__ void
lm_thin_tiles(LmGeom g, const double* r_vals, const int32_t* perm, const double* y,
              const double* diag, double par, double* x, double* partials)
{
    __shared__ double red[12];
    const double sp = sqrt(par);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < g.num_tiles; t += (int64_t)gridDim.x * THREADS) {
        int c, bc;
        int64_t roff;
        lm_geom(g, t, c, roff, bc);
        const bool two = c == 2;
        const double r00 = r_vals[roff], r01 = two ? r_vals[roff + 1] : 0.0, r11 = two ? r_vals[roff + 2] : 1.0;
        const int p0 = perm[bc], p1 = two ? perm[bc + 1] : p0;
        const double d0 = diag ? diag[p0] : 1.0, d1 = (two && diag) ? diag[p1] : 1.0;
        const double y0 = y[bc], y1 = two ? y[bc + 1] : 0.0;
        // reflector 0 on [r00; sp d0]: column 1 and the right-hand side get a fill in row 0 of the lower part
        const double l0 = sp * d0;
        double s00, v0, gm;
        lm_reflector(r00, l0 * l0, s00, v0, gm);
        double w = v0 * r01 * gm;
        const double s01 = fma(-w, v0, r01), l01 = -w * l0;
        w = v0 * y0 * gm;
        const double t0 = fma(-w, v0, y0), f0 = -w * l0;
        // reflector 1 on [r11; l01; sp d1]
        const double l1 = sp * d1;
        double s11;
        lm_reflector(r11, fma(l01, l01, l1 * l1), s11, v0, gm);
        w = fma(l01, f0, v0 * y1) * gm;
        const double t1 = fma(-w, v0, y1);
        // z = S^-1 t up to the first zero on the diagonal
        const int k0 = s00 == 0.0 ? 0 : ((two && s11 == 0.0) ? 1 : c);
        const double z1 = (two && k0 > 1) ? t1 / s11 : 0.0;
        const double z0 = k0 > 0 ? fma(-s01, z1, t0) / s00 : 0.0;
        x[p0] = z0;
        if (two) x[p1] = z1;
        if (partials) {
            const double a0 = d0 * z0, a1 = d1 * z1;
            acc[0] += fma(a0, a0, a1 * a1);
            if (k0 == c) {                                   // S^T w = Dt^2 z
                const double w0 = d0 * a0 / s00;
                const double w1 = two ? fma(-s01, w0, d1 * a1) / s11 : 0.0;
                acc[1] += fma(w0, w0, w1 * w1);
            }
            if (r00 == 0.0 || (two && r11 == 0.0)) acc[2] += 1.0;
        }
    }
    if (partials) {
        block_sum<3>(acc, red);
        if (threadIdx.x == 0) {
            partials[3 * blockIdx.x] = acc[0]; partials[3 * blockIdx.x + 1] = acc[1]; partials[3 * blockIdx.x + 2] = acc[2];
        }
    }
}

__global__ void __launch_bounds__(THREADS)
bd_lm_thin_kernel(LmGeom g, const double* __restrict__ r_vals, const int32_t* __restrict__ perm, const double* __restrict__ y,
                  const double* __restrict__ diag, double par, double* __restrict__ x, double* __restrict__ partials)
{
    lm_thin_tiles(g, r_vals, perm, y, diag, par, x, partials);
}

// One damped evaluation of the device-side lmpar: nothing (x included) is touched once the search has stopped
__global__ void __launch_bounds__(THREADS)
bd_lm_thin_ctl_kernel(LmGeom g, const double* __restrict__ r_vals, const int32_t* __restrict__ perm, const double* __restrict__ y,
                      const double* __restrict__ diag, const LmControl* __restrict__ ctl, double* __restrict__ x,
                      double* __restrict__ partials)
{
    if (ctl->done) return;                            // (uniform loads: the control block is read through the scalar cache)
    lm_thin_tiles(g, r_vals, perm, y, diag, ctl->par, x, partials);
}

// ---- tiles with up to 32 columns: a group of G lanes per tile ----------------------------------------------------------------------
// Lane k of a group holds column k of R and of the lower part in registers (static indices: every loop is unrolled), the lane after
// the last column holds the right-hand side as one more column -- so G > c: 8 / 16 / 32 lanes for up to 7 / 15 / 31 columns, the
// whole wavefront for 32.  Reflector k is computed in lane k and read by the others (v_readlane when the group is the wavefront,
// ds_bpermute otherwise).  Back substitution by rows: the products S(k, j) z_j sit in the lanes j > k, one butterfly sum per row,
// lane k keeps z_k.  The forward substitution of sums[1] is by columns and broadcasts one entry per step.

// v again, wave-uniform, as a value the compiler cannot relate to v: the comparisons k < v of one unrolled phase are then not kept
// in scalar registers for the next phase
__device__ __forceinline__ int opaque_uniform(int v)
{
    asm volatile("" : "+s"(v));
    return __builtin_amdgcn_readfirstlane(v);
}

template <int G>
__device__ __forceinline__ double group_bcast(double v, int src_lane, int k)
{
    if (G == 64) return readlane_f64(v, k);
    return __shfl(v, src_lane, 64);
}

// The body of bd_lm_group_kernel<G>, bd_lm_group_ctl_kernel<G> and bd_lm_group_last_kernel<G>
template <int G>
__device__ __forceinline__ void
lm_group_tiles(LmGeom g, const double* r_vals, const int32_t* perm, const double* y,
               const double* diag, double par, double* x, double* partials)
{
    constexpr int CM = G == 64 ? 32 : G - 1;          // widest tile of this instantiation
    constexpr int TPB = THREADS / G;                  // tiles per workgroup
    __shared__ double red[12];
    const int lane = threadIdx.x & 63, jl = lane & (G - 1), gbase = lane & ~(G - 1), slot = threadIdx.x / G;
    const int64_t ntg = (g.num_tiles + TPB - 1) / TPB;
    const double sp = sqrt(par);
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t wi = blockIdx.x; wi < ntg; wi += gridDim.x) {
        const int64_t t = wi * TPB + slot;
        const bool valid = t < g.num_tiles;
        // jv = jl behind an empty asm: the lane predicates of the unrolled steps (jl == k, jl > k, ...) do not depend on the tile, and
        // hoisted out of the tile loop they would occupy two scalar registers each for the whole kernel
        int jv = jl;
        asm volatile("" : "+v"(jv));
        int c, bc;
        int64_t roff;
        lm_geom(g, valid ? t : 0, c, roff, bc);
        if (!valid) c = 0;
        const bool col = jl < c, rhs = valid && jl == c;
        int cw = c;                                   // widest tile of the wavefront bounds the unrolled loops
        if (G < 64) {                                 // (also the empty slots behind the last tile: c = 0 there)
#pragma unroll
            for (int o = 32; o >= G; o >>= 1) { const int other = __shfl_xor(cw, o, 64); cw = other > cw ? other : cw; }
        }
        cw = __builtin_amdgcn_readfirstlane(cw);
        // column jl of R (a contiguous run of the packed triangle), or y in the lane of the right-hand side
        int pj = 0;
        double dj = 1.0;
        if (col) { pj = perm[bc + jl]; if (diag) dj = diag[pj]; }
        const double* src = col ? r_vals + roff + (int64_t)(jl * (jl + 1) / 2) : y + bc;
        const int n = col ? jl + 1 : (rhs ? c : 0);
        // entry (jl, jl) of the lower part; its other entries are fill: reflector k writes row k of it, so Lc[k] is first assigned there
        const double lj = col ? sp * dj : 0.0;
        double Rc[CM], Lc[CM];
#pragma unroll
        for (int i = 0; i < CM; ++i) {
            double v = 0.0;
            if (i < n) v = src[i];                    // (predicated, not clamped: one address register pair for the whole run)
            Rc[i] = v;
        }
        const double rdiag = col ? src[jl] : 1.0;     // R(jl, jl)
        // triangularise [R; sp Dt]
        double sd = 1.0;                              // S(jl, jl)
#pragma unroll
        for (int k = 0; k < CM; ++k) {
            if (k < cw) {
                double sigma = lj * lj;
#pragma unroll
                for (int i = 0; i < k; ++i) sigma = fma(Lc[i], Lc[i], sigma);
                double beta, v0, gm;
                lm_reflector(Rc[k], sigma, beta, v0, gm);          // (meaningful in lane k of the group)
                if (col && jv == k) sd = beta;
                const double bv0 = group_bcast<G>(v0, gbase + k, k), bgm = group_bcast<G>(gm, gbase + k, k);
                const double blj = group_bcast<G>(lj, gbase + k, k);
                const bool right = jv > k && jv <= c;              // the columns right of the pivot, the right-hand side included
                double dot = bv0 * Rc[k];
                if (G == 64) {
                    // the reflector is read twice (v_readlane is cheap) instead of being kept in 2 k scalar registers
#pragma unroll
                    for (int i = 0; i < k; ++i) {
                        dot = fma(readlane_f64(Lc[i], k), Lc[i], dot);
                        if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);   // (at most 16 scalar registers of reflector in flight)
                    }
                    const double wv = right ? dot * bgm : 0.0;
                    Rc[k] = fma(-wv, bv0, Rc[k]);
                    // (an empty asm per register: otherwise the compiler sees that the second read returns what the first did and keeps
                    //  all of the first pass alive in scalar registers)
#pragma unroll
                    for (int i = 0; i < k; ++i) asm volatile("" : "+v"(Lc[i]));
#pragma unroll
                    for (int i = 0; i < k; ++i) {
                        Lc[i] = fma(-wv, readlane_f64(Lc[i], k), Lc[i]);
                        if ((i & 7) == 7) __builtin_amdgcn_sched_barrier(0);
                    }
                    Lc[k] = -wv * blj;
                } else {
                    double lv[CM];
#pragma unroll
                    for (int i = 0; i < k; ++i) { lv[i] = __shfl(Lc[i], gbase + k, 64); dot = fma(lv[i], Lc[i], dot); }
                    const double wv = right ? dot * bgm : 0.0;
                    Rc[k] = fma(-wv, bv0, Rc[k]);
#pragma unroll
                    for (int i = 0; i < k; ++i) Lc[i] = fma(-wv, lv[i], Lc[i]);
                    Lc[k] = -wv * blj;
                }
                __builtin_amdgcn_sched_barrier(0);    // (keeps the broadcasts of step k + 1 from being hoisted over step k)
            }
        }
        // first zero on S's diagonal, a zero on R's
        int k0 = (col && sd == 0.0) ? jl : c;
        int rz = (col && rdiag == 0.0) ? 1 : 0;
#pragma unroll
        for (int o = G / 2; o >= 1; o >>= 1) {
            const int a = __shfl_xor(k0, o, 64), b = __shfl_xor(rz, o, 64);
            k0 = a < k0 ? a : k0;
            rz |= b;
        }
        // z = S^-1 t by rows, last row first
        asm volatile("" : "+v"(jv));                  // (the predicates again: not shared with the steps above)
        const int cw2 = opaque_uniform(cw);
        double z = 0.0;
#pragma unroll
        for (int k = CM - 1; k >= 0; --k) {
            if (k < cw2) {
                double term = (col && jv > k) ? -Rc[k] * z : (rhs ? Rc[k] : 0.0);
#pragma unroll
                for (int o = G / 2; o >= 1; o >>= 1) term += __shfl_xor(term, o, 64);
                if (jv == k && k < k0) z = term / sd;
            }
        }
        if (col) x[pj] = z;
        if (partials) {
            const double dz = dj * z;
            // S^T w = Dt^2 z by columns
            asm volatile("" : "+v"(jv));
            const int cw3 = opaque_uniform(cw);
            double a = dj * dz, wk = 0.0;
#pragma unroll
            for (int i = 0; i < CM; ++i) {
                if (i < cw3) {
                    const double wloc = a / sd;                    // (meaningful in lane i)
                    const double wb = group_bcast<G>(wloc, gbase + i, i);
                    if (jv == i) wk = wloc;
                    a = (col && jv > i) ? fma(-Rc[i], wb, a) : a;
                }
            }
            acc[0] += col ? dz * dz : 0.0;
            acc[1] += (col && k0 == c) ? wk * wk : 0.0;
            acc[2] += (valid && jl == 0 && rz) ? 1.0 : 0.0;
        }
    }
    if (partials) {
        block_sum<3>(acc, red);
        if (threadIdx.x == 0) {
            partials[3 * blockIdx.x] = acc[0]; partials[3 * blockIdx.x + 1] = acc[1]; partials[3 * blockIdx.x + 2] = acc[2];
        }
    }
}

template <int G>
__global__ void __launch_bounds__(THREADS)
bd_lm_group_kernel(LmGeom g, const double* __restrict__ r_vals, const int32_t* __restrict__ perm, const double* __restrict__ y,
                   const double* __restrict__ diag, double par, double* __restrict__ x, double* __restrict__ partials)
{
    lm_group_tiles<G>(g, r_vals, perm, y, diag, par, x, partials);
}

template <int G>
__global__ void __launch_bounds__(THREADS)
bd_lm_group_ctl_kernel(LmGeom g, const double* __restrict__ r_vals, const int32_t* __restrict__ perm, const double* __restrict__ y,
                       const double* __restrict__ diag, const LmControl* __restrict__ ctl, double* __restrict__ x,
                       double* __restrict__ partials)
{
    if (ctl->done) return;
    lm_group_tiles<G>(g, r_vals, perm, y, diag, ctl->par, x, partials);
}

// ---- the partials of `nblocks` workgroups (n sums each) added in a fixed order: one workgroup -------------------------------------
// sum s of the n: every thread its partials b = threadIdx.x, threadIdx.x + 256, ... in that order, then block_sum (the same value in
// every thread)
__device__ __forceinline__ double lm_sum_partials(const double* __restrict__ partials, int nblocks, int n, int s, double* red)
{
    double v[1] = {0.0};
    for (int b = threadIdx.x; b < nblocks; b += THREADS) v[0] += partials[(int64_t)b * n + s];
    block_sum<1>(v, red);
    return v[0];
}

__global__ void __launch_bounds__(THREADS)
bd_lm_finish_kernel(const double* __restrict__ partials, int nblocks, int n, double* __restrict__ out)
{
    __shared__ double red[4];
    for (int s = 0; s < n; ++s) {
        const double v = lm_sum_partials(partials, nblocks, n, s, red);
        if (threadIdx.x == 0) out[s] = v;
    }
}

// ---- the device-side lmpar (qrk_bd_lmpar_device): MINPACK's update of par as one lane's work behind the sums of an evaluation -------
// The scalar arithmetic of qrk_bd_lmpar's host loop (capi.hip; include/qrkit_amd.h spells out steps 1-5) operation for operation:
// correctly rounded sqrt and division, no contraction (there is no a * b + c in it, and the pragma keeps it so), std::min / std::max
// as comparisons.
__device__ __forceinline__ double lm_max(double a, double b) { return a < b ? b : a; }     // std::max(a, b)
__device__ __forceinline__ double lm_min(double a, double b) { return b < a ? b : a; }     // std::min(a, b)
constexpr double LM_DBL_MIN = 2.2250738585072014e-308;

// Steps 1-4 behind the evaluation at par = 0: s = (s0, s1, s2) of that solve, gnorm2 = | D^-1 g |^2.  Leaves the control block ready
// for the first damped evaluation, or done.
__device__ void lm_control_first(LmControl* ctl, double s0, double s1, double s2, double gnorm2, const double* delta_p, double* par_p,
                                 int32_t* iters, double* trace)
{
#pragma clang fp contract(off)
    const double delta = *delta_p, par0 = *par_p;
    if (trace) { trace[0] = 0.0; trace[1] = s0; trace[2] = s1; }
    ctl->evals = 1;
    ctl->done = 1;
    if (!(delta > 0.0) || !(par0 >= 0.0)) {           // what qrk_bd_lmpar refuses on the host: *par stays, no damped evaluation
        if (iters) *iters = -1;
        return;
    }
    if (iters) *iters = 0;
    const double dxnorm = sqrt(s0);
    const double fp = dxnorm - delta;
    if (fp <= 0.1 * delta) { *par_p = 0.0; return; }
    const double parl = (s2 > 0.0 || !(s1 > 0.0)) ? 0.0 : fp / (delta * s1 / s0);
    const double gnorm = sqrt(gnorm2);
    double paru = gnorm / delta;
    if (paru == 0.0) paru = LM_DBL_MIN / lm_min(delta, 0.1);
    double pv = lm_min(lm_max(par0, parl), paru);
    if (pv == 0.0) pv = gnorm / dxnorm;
    if (pv == 0.0) pv = lm_max(LM_DBL_MIN, 0.001 * paru);         // (the head of pass 1)
    ctl->par = pv; ctl->parl = parl; ctl->paru = paru; ctl->fp = fp; ctl->delta = delta; ctl->gnorm = gnorm;
    ctl->done = 0;
}

// Step 5 behind damped evaluation number ctl->evals (= the pass of the loop): stop, or the next par
__device__ void lm_control_pass(LmControl* ctl, double s0, double s1, double* par_p, int32_t* iters, double* trace)
{
#pragma clang fp contract(off)
    const int iter = ctl->evals;
    double pv = ctl->par, parl = ctl->parl, paru = ctl->paru;
    const double delta = ctl->delta, temp = ctl->fp;
    if (trace) { trace[3 * iter] = pv; trace[3 * iter + 1] = s0; trace[3 * iter + 2] = s1; }
    const double dxnorm = sqrt(s0);
    const double fp = dxnorm - delta;
    if (iters) *iters = iter;
    ctl->evals = iter + 1;
    ctl->fp = fp;
    if (fabs(fp) <= 0.1 * delta || (parl == 0.0 && fp <= temp && temp < 0.0) || iter == 10) {
        *par_p = pv;
        ctl->done = 1;
        return;
    }
    const double parc = fp / (delta * s1 / s0);
    if (fp > 0.0) parl = lm_max(parl, pv);
    if (fp < 0.0) paru = lm_min(paru, pv);
    pv = lm_max(parl, pv + parc);
    if (pv == 0.0) pv = lm_max(LM_DBL_MIN, 0.001 * paru);         // (the head of the next pass)
    ctl->par = pv; ctl->parl = parl; ctl->paru = paru;
}

// One workgroup behind the gradient's column kernel of evaluation 0 (FIRST: sums = s0, s1, s2 of the solve at par = 0, already
// finished by bd_lm_finish_kernel; partials = the `nblocks` partials of | D^-1 g |^2; the unused rows of trace are cleared here) or
// behind a damped solve (partials = its 3 `nblocks` partials).  The sums are bd_lm_finish_kernel's, bit for bit; lane 0 does the
// control step.
template <bool FIRST>
__global__ void __launch_bounds__(THREADS)
bd_lm_control_kernel(const double* __restrict__ partials, int nblocks, double* __restrict__ sums, LmControl* __restrict__ ctl,
                     const double* __restrict__ delta, double* __restrict__ par, int32_t* __restrict__ iters,
                     double* __restrict__ trace)
{
    __shared__ double red[4];
    if (FIRST) {
        const double gnorm2 = lm_sum_partials(partials, nblocks, 1, 0, red);
        if (trace && threadIdx.x >= 3 && threadIdx.x < 33) trace[threadIdx.x] = 0.0;
        if (threadIdx.x == 0) {
            sums[3] = gnorm2;
            lm_control_first(ctl, sums[0], sums[1], sums[2], gnorm2, delta, par, iters, trace);
        }
    } else {
        if (ctl->done) return;
        double s[3];
        for (int i = 0; i < 3; ++i) s[i] = lm_sum_partials(partials, nblocks, 3, i, red);
        if (threadIdx.x == 0) {
            sums[0] = s[0]; sums[1] = s[1]; sums[2] = s[2];
            lm_control_pass(ctl, s[0], s[1], par, iters, trace);
        }
    }
}

// ---- the same control step without a kernel of its own: the workgroup that arrives last does it ---------------------------------
// Behind the partial of a damped solve (the hand-off of an in-launch reduction; nobody waits, a workgroup that is not last exits):
// every wave drains its stores, the workgroup meets, lane 0 releases at agent scope and draws a ticket from the counter of this pass
// (cleared with the control block at the start of the call); the workgroup that draws the last ticket acquires at agent scope and
// then reads all partials -- added in bd_lm_finish_kernel's order, so the sums keep their bits -- and lane 0 does the control step.
// Returns at once for every workgroup but that one.  fin: 4 doubles of LDS.
struct LmResult {
    double* sums;
    double* par;
    int32_t* iters;
    double* trace;
};

__device__ __forceinline__ void lm_last_arriver(LmControl* ctl, int pass, const double* partials, const LmResult& out, double* fin)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t ticket = __hip_atomic_fetch_add(&ctl->arrived[pass], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fin[0] = ticket == gridDim.x - 1 ? 1.0 : 0.0;
    }
    __syncthreads();
    const bool last = fin[0] != 0.0;
    if (!last) return;
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    double s[3];
    for (int i = 0; i < 3; ++i) s[i] = lm_sum_partials(partials, (int)gridDim.x, 3, i, fin);
    if (threadIdx.x == 0) {
        out.sums[0] = s[0]; out.sums[1] = s[1]; out.sums[2] = s[2];
        lm_control_pass(ctl, s[0], s[1], out.par, out.iters, out.trace);
    }
}

__global__ void __launch_bounds__(THREADS)
bd_lm_thin_last_kernel(LmGeom g, const double* __restrict__ r_vals, const int32_t* __restrict__ perm, const double* __restrict__ y,
                       const double* __restrict__ diag, LmControl* ctl, double* __restrict__ x, double* partials, LmResult out)
{
    __shared__ double fin[4];
    if (ctl->done) return;
    const int pass = ctl->evals;                      // (read before any workgroup can have written the next one: that takes all tickets)
    lm_thin_tiles(g, r_vals, perm, y, diag, ctl->par, x, partials);
    lm_last_arriver(ctl, pass, partials, out, fin);
}

template <int G>
__global__ void __launch_bounds__(THREADS)
bd_lm_group_last_kernel(LmGeom g, const double* __restrict__ r_vals, const int32_t* __restrict__ perm, const double* __restrict__ y,
                        const double* __restrict__ diag, LmControl* ctl, double* __restrict__ x, double* partials, LmResult out)
{
    __shared__ double fin[4];
    if (ctl->done) return;
    const int pass = ctl->evals;
    lm_group_tiles<G>(g, r_vals, perm, y, diag, ctl->par, x, partials);
    lm_last_arriver(ctl, pass, partials, out, fin);
}

// ---- g = P R^T y and the column norms of R: G lanes per tile (a power of two >= the widest tile), lane k = column k ----------------
// MODE 0: out[perm[base_col + k]] = sum_{i <= k} R(i, k) y_i (out may be null) and the partial of sum (g_j / diag_j)^2 (partials may
// be null); MODE 1: out[perm[base_col + k]] = || R(0:k, k) ||.
template <int MODE>
__global__ void __launch_bounds__(THREADS)
bd_lm_columns_kernel(LmGeom g, int G, const double* __restrict__ r_vals, const int32_t* __restrict__ perm,
                     const double* __restrict__ y, const double* __restrict__ diag, double* __restrict__ out,
                     double* __restrict__ partials)
{
    __shared__ double red[4];
    const int jl = threadIdx.x & (G - 1), slot = threadIdx.x / G, tpb = THREADS / G;
    const int64_t ntg = (g.num_tiles + tpb - 1) / tpb;
    double acc[1] = {0.0};
    for (int64_t wi = blockIdx.x; wi < ntg; wi += gridDim.x) {
        const int64_t t = wi * tpb + slot;
        if (t >= g.num_tiles) continue;
        int c, bc;
        int64_t roff;
        lm_geom(g, t, c, roff, bc);
        if (jl >= c) continue;
        const double* rc = r_vals + roff + (int64_t)(jl * (jl + 1) / 2);
        const int pj = perm[bc + jl];
        double s = 0.0;
        if (MODE == 0) {
            for (int i = 0; i <= jl; ++i) s = fma(rc[i], y[bc + i], s);
            if (out) out[pj] = s;
            const double q = s / (diag ? diag[pj] : 1.0);
            acc[0] = fma(q, q, acc[0]);
        } else {
            for (int i = 0; i <= jl; ++i) s = fma(rc[i], rc[i], s);
            out[pj] = sqrt(s);
        }
    }
    if (MODE == 0 && partials) {
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
    }
}

}  // namespace lm

// Lanes per tile of the damped solve for a plan whose widest tile has max_cols columns: 0 = one lane per tile (bd_lm_thin_kernel),
// 8 / 16 / 32 / 64 = bd_lm_group_kernel<G>, -1 = not supported (more than 32 columns).
int bd_lm_group_width(int max_cols)
{
    if (max_cols <= 2) return 0;
    if (max_cols <= 7) return 8;
    if (max_cols <= 15) return 16;
    if (max_cols <= 31) return 32;
    return max_cols <= 32 ? 64 : -1;
}

// Workgroups of the damped solve: a function of the plan (tile count and widest tile) alone, at most BD_LM_MAX_BLOCKS
static int lm_solve_blocks(int64_t num_tiles, int G)
{
    const int64_t tpb = G == 0 ? lm::THREADS : lm::THREADS / G;
    const int64_t ntg = (num_tiles + tpb - 1) / tpb;
    return (int)(ntg < BD_LM_MAX_BLOCKS ? ntg : BD_LM_MAX_BLOCKS);
}

hipError_t launch_bd_lm_solve(const TileGeom& g, int max_cols, const double* r_vals, const int32_t* perm, const double* y,
                              const double* diag, double par, double* x, double* partials, double* sums, hipStream_t stream)
{
    const int G = bd_lm_group_width(max_cols);
    if (G < 0) return hipErrorInvalidValue;
    if (g.num_tiles <= 0) return sums ? hipMemsetAsync(sums, 0, 3 * sizeof(double), stream) : hipSuccess;
    const int blocks = lm_solve_blocks(g.num_tiles, G);
    double* const part = sums ? partials : nullptr;
    const lm::LmGeom lg = lm::lm_geom_of(g);
#define QRK_LM_G(GG) case GG: hipLaunchKernelGGL((lm::bd_lm_group_kernel<GG>), dim3(blocks), dim3(lm::THREADS), 0, stream, lg, r_vals, perm, y, diag, par, x, part); break;
    switch (G) {
    case 0: hipLaunchKernelGGL(lm::bd_lm_thin_kernel, dim3(blocks), dim3(lm::THREADS), 0, stream, lg, r_vals, perm, y, diag, par, x, part); break;
    QRK_LM_G(8) QRK_LM_G(16) QRK_LM_G(32) QRK_LM_G(64)
    default: break;
    }
#undef QRK_LM_G
    if (sums) hipLaunchKernelGGL(lm::bd_lm_finish_kernel, dim3(1), dim3(lm::THREADS), 0, stream, partials, blocks, 3, sums);
    return hipGetLastError();
}

static void lm_columns_grid(int64_t num_tiles, int max_cols, int& G, int& blocks);

// MINPACK's lmpar as a fixed chain on the stream (qrk_bd_lmpar_device): no launch depends on a host decision.
//   memset of the control block; evaluation 0 = the solve at par = 0 with its finish (the kernels and sums of launch_bd_lm_solve),
//   the gradient's column kernel, bd_lm_control_kernel<true>; then ten damped evaluations, which return at once when the control
//   block says done: bd_lm_*_last_kernel (last_arriver: the sums and the control step in the workgroup that arrives last), or
//   bd_lm_*_ctl_kernel + bd_lm_control_kernel<false> (a kernel boundary in place of the hand-off).
// scratch: the plan's (BD_LM_SCRATCH_DOUBLES); delta, par, iters, trace: device.
hipError_t launch_bd_lmpar_device(const TileGeom& g, int max_cols, const double* r_vals, const int32_t* perm, const double* y,
                                  const double* diag, const double* delta, double* par, double* x, int32_t* iters, double* trace,
                                  double* scratch, bool last_arriver, hipStream_t stream)
{
    const int G = bd_lm_group_width(max_cols);
    if (G < 0) return hipErrorInvalidValue;
    double* const partials = scratch;
    double* const sums = scratch + 3 * BD_LM_MAX_BLOCKS;
    LmControl* const ctl = (LmControl*)(scratch + 3 * BD_LM_MAX_BLOCKS + 4);
    hipError_t e = hipMemsetAsync(ctl, 0, sizeof(LmControl), stream);
    if (e != hipSuccess) return e;
    if ((e = launch_bd_lm_solve(g, max_cols, r_vals, perm, y, diag, 0.0, x, partials, sums, stream)) != hipSuccess) return e;
    const lm::LmGeom lg = lm::lm_geom_of(g);
    const bool any = g.num_tiles > 0;
    int gblocks = 0;
    if (any) {
        int GC;
        lm_columns_grid(g.num_tiles, max_cols, GC, gblocks);
        hipLaunchKernelGGL(lm::bd_lm_columns_kernel<0>, dim3(gblocks), dim3(lm::THREADS), 0, stream, lg, GC, r_vals, perm, y, diag, (double*)nullptr,
                           partials);
    }
    hipLaunchKernelGGL(lm::bd_lm_control_kernel<true>, dim3(1), dim3(lm::THREADS), 0, stream, partials, gblocks, sums, ctl, delta, par, iters, trace);
    const int blocks = any ? lm_solve_blocks(g.num_tiles, G) : 0;
    const lm::LmResult res{sums, par, iters, trace};
    for (int pass = 1; pass <= 10 && any && last_arriver; ++pass) {
#define QRK_LM_G(GG) case GG: hipLaunchKernelGGL((lm::bd_lm_group_last_kernel<GG>), dim3(blocks), dim3(lm::THREADS), 0, stream, lg, r_vals, perm, y, diag, ctl, x, partials, res); break;
        switch (G) {
        case 0: hipLaunchKernelGGL(lm::bd_lm_thin_last_kernel, dim3(blocks), dim3(lm::THREADS), 0, stream, lg, r_vals, perm, y, diag, ctl, x, partials, res); break;
        QRK_LM_G(8) QRK_LM_G(16) QRK_LM_G(32) QRK_LM_G(64)
        default: break;
        }
#undef QRK_LM_G
    }
    for (int pass = 1; pass <= 10 && any && !last_arriver; ++pass) {
#define QRK_LM_G(GG) case GG: hipLaunchKernelGGL((lm::bd_lm_group_ctl_kernel<GG>), dim3(blocks), dim3(lm::THREADS), 0, stream, lg, r_vals, perm, y, diag, ctl, x, partials); break;
        switch (G) {
        case 0: hipLaunchKernelGGL(lm::bd_lm_thin_ctl_kernel, dim3(blocks), dim3(lm::THREADS), 0, stream, lg, r_vals, perm, y, diag, ctl, x, partials); break;
        QRK_LM_G(8) QRK_LM_G(16) QRK_LM_G(32) QRK_LM_G(64)
        default: break;
        }
#undef QRK_LM_G
        hipLaunchKernelGGL(lm::bd_lm_control_kernel<false>, dim3(1), dim3(lm::THREADS), 0, stream, partials, blocks, sums, ctl, delta, par, iters, trace);
    }
    return hipGetLastError();
}

// lanes per tile and workgroups of the column kernels
static void lm_columns_grid(int64_t num_tiles, int max_cols, int& G, int& blocks)
{
    G = 1;
    while (G < max_cols) G *= 2;
    const int64_t tpb = lm::THREADS / G, ntg = (num_tiles + tpb - 1) / tpb;
    blocks = (int)(ntg < BD_LM_MAX_BLOCKS ? ntg : BD_LM_MAX_BLOCKS);
}

hipError_t launch_bd_lm_gradient(const TileGeom& g, int max_cols, const double* r_vals, const int32_t* perm, const double* y,
                                 const double* diag, double* gout, double* partials, double* gnorm2, hipStream_t stream)
{
    if (max_cols > 32) return hipErrorInvalidValue;
    if (g.num_tiles <= 0) return gnorm2 ? hipMemsetAsync(gnorm2, 0, sizeof(double), stream) : hipSuccess;
    int G, blocks;
    lm_columns_grid(g.num_tiles, max_cols, G, blocks);
    hipLaunchKernelGGL(lm::bd_lm_columns_kernel<0>, dim3(blocks), dim3(lm::THREADS), 0, stream, lm::lm_geom_of(g), G, r_vals, perm, y, diag, gout,
                       gnorm2 ? partials : nullptr);
    if (gnorm2) hipLaunchKernelGGL(lm::bd_lm_finish_kernel, dim3(1), dim3(lm::THREADS), 0, stream, partials, blocks, 1, gnorm2);
    return hipGetLastError();
}

hipError_t launch_bd_r_col_norms(const TileGeom& g, int max_cols, const double* r_vals, const int32_t* perm, double* norms,
                                 hipStream_t stream)
{
    if (max_cols > 32) return hipErrorInvalidValue;
    if (g.num_tiles <= 0) return hipSuccess;
    int G, blocks;
    lm_columns_grid(g.num_tiles, max_cols, G, blocks);
    hipLaunchKernelGGL(lm::bd_lm_columns_kernel<1>, dim3(blocks), dim3(lm::THREADS), 0, stream, lm::lm_geom_of(g), G, r_vals, perm, nullptr, nullptr, norms,
                       nullptr);
    return hipGetLastError();
}

}  // namespace qrk
