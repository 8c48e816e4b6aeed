// bd_lm_geom.h -- what the Levenberg-Marquardt kernels on the block-diagonal factors share: the tile geometry they read and the
// reflector of the damped elimination (bd_lm.hip: DESIGN.md K9 / K10; bd_lm_panel.hip: K11).
#pragma once
#include "qrk_device.h"

namespace qrk {
namespace lm {

constexpr int THREADS = 256;

// What these kernels need of a TileGeom (kernel arguments live in scalar registers for the whole kernel: 9 instead of 26)
struct LmGeom {
    int64_t num_tiles;
    const int32_t* t_cols;       // null: uniform tiles of `cols` columns
    const int64_t* r_off;
    const int32_t* c_off;
    int32_t cols;
};

static inline LmGeom lm_geom_of(const TileGeom& g)
{
    LmGeom l{};
    l.num_tiles = g.num_tiles; l.cols = g.cols;
    l.t_cols = g.t_rows ? g.t_cols : nullptr; l.r_off = g.r_off; l.c_off = g.c_off;
    return l;
}

__device__ __forceinline__ void lm_geom(const LmGeom& g, int64_t t, int& c, int64_t& roff, int& base_col)
{
    if (g.t_cols) {
        c = g.t_cols[t]; roff = g.r_off[t]; base_col = g.c_off[t];
    } else {
        c = g.cols; roff = t * (int64_t)(c * (c + 1) / 2); base_col = (int)(t * c);
    }
}

// Reflector of the column [a; l], sigma = |l|^2: beta = the new diagonal entry, v0 = a - beta (no cancellation: beta has the sign
// of -a), gm = 1 / (v^T v / 2).  sigma = 0 (par = 0, or nothing below): the identity, written as gm = v0 = 0.
__device__ __forceinline__ void lm_reflector(double a, double sigma, double& beta, double& v0, double& gm)
{
    if (sigma > 0.0) {
        beta = -copysign(sqrt(fma(a, a, sigma)), a);
        v0 = a - beta;
        gm = -1.0 / (beta * v0);
    } else {
        beta = a; v0 = 0.0; gm = 0.0;
    }
}

}  // namespace lm
}  // namespace qrk
