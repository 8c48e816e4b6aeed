// C++ test of the Levenberg-Marquardt step through the facade: BlockDiagonalSparseQR::colNorms / lmGradient / lmSolve / lmpar
// (qrk_bd_r_col_norms, qrk_bd_lm_gradient, qrk_bd_lm_solve, qrk_bd_lmpar) after the Q-less factorizeAndSolve().
//  * the primitives on the reference's 7x2 input (generate_block_diagonal_matrix, test/test-qrkit.cpp:101-117) against plain loops over
//    matrixR() and colsPermutation() on the host;
//  * a trust-region fit of y = exp(a t) + b (7 samples and 2 parameters per block, the block shape of the reference's tests) on
//    UNDAMPED tiles: one factorizeAndSolve() per Jacobian, lmpar() for every trial step, the pattern analysed once -- the loop of
//    Eigen::LevenbergMarquardt (examples/ellipse_fitting.cpp:257-280) with this solver behind it.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>

#include "qrkit/QRKit.hpp"

using namespace qrkit;

static double relDiff(const Vector& a, const Vector& b) {
    if (a.size() != b.size()) return 1e300;
    double num = 0, na = 0, nb = 0;
    for (size_t i = 0; i < a.size(); ++i) { const double d = a[i] - b[i]; num += d * d; na += a[i] * a[i]; nb += b[i] * b[i]; }
    const double den = std::sqrt(std::min(na, nb));
    return den > 0 ? std::sqrt(num) / den : std::sqrt(num);
}

static int test_primitives(int numBlocks) {
    const int br = 7, bc = 2;
    std::default_random_engine gen;
    std::uniform_real_distribution<double> dist(0.5, 5.0);
    SparseBlockDiagonal m;
    Matrix a(br, bc);
    for (int i = 0; i < numBlocks; ++i) { for (int e = 0; e < br * bc; ++e) a.data()[e] = dist(gen); m.insertBack(a); }
    m.setDims(numBlocks * br, numBlocks * bc);
    Vector b((size_t)(numBlocks * br));
    for (double& v : b) v = dist(gen) - 2.5;
    const size_t n = (size_t)(numBlocks * bc);

    int fails = 0;
    BlockDiagonalSparseQR<> qr;
    Vector qtb;
    const Vector x0 = qr.computeAndSolve(m, b, &qtb);
    if (qr.hasQ() || qr.lmKernelName().find("bd_lm_thin_kernel") == std::string::npos) { std::printf("  state / kernel name wrong\n"); ++fails; }
    // R of block i (packed upper triangle: r00, r01, r11) and the permutation, on the host
    const Vector& rv = qr.matrixR().values();
    const std::vector<int>& perm = qr.colsPermutation().indices();
    Vector norms(n), g(n), xd(n);
    const double par = 0.3;
    double s0 = 0, gn2 = 0;
    for (int i = 0; i < numBlocks; ++i) {
        const double r00 = rv[3 * i], r01 = rv[3 * i + 1], r11 = rv[3 * i + 2], y0 = qtb[2 * i], y1 = qtb[2 * i + 1];
        const int p0 = perm[2 * i], p1 = perm[2 * i + 1];
        norms[p0] = std::fabs(r00); norms[p1] = std::sqrt(r01 * r01 + r11 * r11);
        g[p0] = r00 * y0; g[p1] = r01 * y0 + r11 * y1;
    }
    for (int i = 0; i < numBlocks; ++i) {
        // (R^T R + par Dt^2) z = R^T y with Dt = the column norms, by Cramer's rule
        const double r00 = rv[3 * i], r01 = rv[3 * i + 1], r11 = rv[3 * i + 2];
        const int p0 = perm[2 * i], p1 = perm[2 * i + 1];
        const double d0 = norms[p0], d1 = norms[p1];
        const double a00 = r00 * r00 + par * d0 * d0, a01 = r00 * r01, a11 = r01 * r01 + r11 * r11 + par * d1 * d1;
        const double det = a00 * a11 - a01 * a01;
        xd[p0] = (g[p0] * a11 - a01 * g[p1]) / det;
        xd[p1] = (a00 * g[p1] - a01 * g[p0]) / det;
        s0 += d0 * d0 * xd[p0] * xd[p0] + d1 * d1 * xd[p1] * xd[p1];
        gn2 += g[p0] * g[p0] / (d0 * d0) + g[p1] * g[p1] / (d1 * d1);
    }
    const Vector diag = qr.colNorms();
    if (relDiff(diag, norms) > 1e-13) { std::printf("  colNorms() differs: %g\n", relDiff(diag, norms)); ++fails; }
    double gnorm = 0;
    if (relDiff(qr.lmGradient(qtb, &diag, &gnorm), g) > 1e-13) { std::printf("  lmGradient() differs\n"); ++fails; }
    if (std::fabs(gnorm * gnorm - gn2) > 1e-12 * gn2) { std::printf("  gnorm differs\n"); ++fails; }
    if (relDiff(qr.lmSolve(qtb, 0, 0.0), x0) > 2e-11) { std::printf("  lmSolve(par = 0) differs from factorizeAndSolve()'s x\n"); ++fails; }
    double sums[3];
    const Vector x = qr.lmSolve(qtb, &diag, par, sums);
    if (relDiff(x, xd) > 1e-11) { std::printf("  lmSolve(par) differs from the normal equations: %g\n", relDiff(x, xd)); ++fails; }
    if (std::fabs(sums[0] - s0) > 1e-11 * s0 || sums[2] != 0.0) { std::printf("  sums differ\n"); ++fails; }
    // lmpar: half the Gauss-Newton step
    double dx0 = 0;
    for (size_t j = 0; j < n; ++j) dx0 += diag[j] * diag[j] * x0[j] * x0[j];
    dx0 = std::sqrt(dx0);
    double pv = 0.0;
    int iters = -1;
    Vector trace;
    const Vector xs = qr.lmpar(qtb, &diag, 0.5 * dx0, pv, &iters, &trace);
    double dxn = 0;
    for (size_t j = 0; j < n; ++j) dxn += diag[j] * diag[j] * xs[j] * xs[j];
    dxn = std::sqrt(dxn);
    if (!(pv > 0.0) || iters < 1 || iters > 5 || trace.size() != (size_t)(3 * (iters + 1)) || std::fabs(dxn - 0.5 * dx0) > 0.05 * dx0) {
        std::printf("  lmpar(0.5 |D x0|): par %g, %d passes, |D x| %g of %g\n", pv, iters, dxn, 0.5 * dx0); ++fails;
    }
    pv = 0.0;
    const Vector xf = qr.lmpar(qtb, &diag, 2.0 * dx0, pv, &iters);
    if (pv != 0.0 || iters != 0 || relDiff(xf, x0) > 2e-11) { std::printf("  lmpar(2 |D x0|) is not the Gauss-Newton step\n"); ++fails; }
    std::printf("LM primitives, %d blocks of 7x2: %s\n", numBlocks, fails ? "Failed." : "Passed.");
    return fails;
}

static int test_fit(int numBlocks) {
    const int br = 7, bc = 2;
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> ud(-1.0, 1.0);
    Vector aTrue((size_t)numBlocks), bTrue((size_t)numBlocks), a((size_t)numBlocks, 0.0), b((size_t)numBlocks, 0.0);
    for (int i = 0; i < numBlocks; ++i) { aTrue[(size_t)i] = ud(rng); bTrue[(size_t)i] = ud(rng); }
    double t[br];
    for (int j = 0; j < br; ++j) t[j] = j / 6.0;
    auto residual = [&](const Vector& aa, const Vector& bb, Vector& r) {
        r.resize((size_t)(numBlocks * br));
        double cost = 0;
        for (int i = 0; i < numBlocks; ++i)
            for (int j = 0; j < br; ++j) {
                const double v = std::exp(aa[(size_t)i] * t[j]) + bb[(size_t)i] - (std::exp(aTrue[(size_t)i] * t[j]) + bTrue[(size_t)i]);
                r[(size_t)(i * br + j)] = v; cost += 0.5 * v * v;
            }
        return cost;
    };
    BlockDiagonalSparseQR<> qr;
    Vector r, rNew, diag;
    double cost = residual(a, b, r), delta = 1.0, par = 0.0;
    int fails = 0, factorizations = 0, damped = 0;
    for (int it = 0; it < 40 && cost >= 1e-24; ++it) {
        SparseBlockDiagonal m;
        Matrix J(br, bc);
        for (int i = 0; i < numBlocks; ++i) {
            for (int j = 0; j < br; ++j) { J.data()[j] = t[j] * std::exp(a[(size_t)i] * t[j]); J.data()[br + j] = 1.0; }
            m.insertBack(J);
        }
        m.setDims(numBlocks * br, numBlocks * bc);
        if (it == 0) qr.analyzePattern(m);
        Vector f(r.size()), qtb;
        for (size_t e = 0; e < r.size(); ++e) f[e] = -r[e];
        (void)qr.factorizeAndSolve(m, f, &qtb);
        ++factorizations;
        const Vector norms = qr.colNorms();
        if (diag.empty()) diag = norms;
        for (size_t j = 0; j < diag.size(); ++j) diag[j] = std::max(diag[j], norms[j]);
        for (int inner = 0; inner < 20; ++inner) {          // trial steps on the SAME factors
            const Vector dx = qr.lmpar(qtb, &diag, delta, par);
            damped += par > 0.0;
            Vector an(a), bn(b);
            double pnorm = 0, lin = 0;
            for (int i = 0; i < numBlocks; ++i) {
                const double da = dx[(size_t)(2 * i)], db = dx[(size_t)(2 * i + 1)];
                an[(size_t)i] += da; bn[(size_t)i] += db;
                pnorm += std::pow(diag[(size_t)(2 * i)] * da, 2) + std::pow(diag[(size_t)(2 * i + 1)] * db, 2);
                for (int j = 0; j < br; ++j) lin += 0.5 * std::pow(r[(size_t)(i * br + j)] + t[j] * std::exp(a[(size_t)i] * t[j]) * da + db, 2);
            }
            pnorm = std::sqrt(pnorm);
            const double newCost = residual(an, bn, rNew), predicted = cost - lin;
            const double ratio = predicted > 0 ? (cost - newCost) / predicted : 0.0;
            if (ratio <= 0.25) delta = 0.5 * std::min(delta, pnorm);
            else if (par == 0.0 || ratio >= 0.75) delta = 2.0 * pnorm;
            if (ratio >= 1e-4) { a = an; b = bn; r = rNew; cost = newCost; break; }
        }
    }
    double worst = 0;
    for (int i = 0; i < numBlocks; ++i) worst = std::max(worst, std::max(std::fabs(a[(size_t)i] - aTrue[(size_t)i]), std::fabs(b[(size_t)i] - bTrue[(size_t)i])));
    if (!(worst < 1e-8) || damped < 3) { std::printf("  fit: worst parameter error %g, %d damped steps\n", worst, damped); ++fails; }
    std::printf("LM fit, %d blocks of 7x2, %d factorisations, %d damped steps: %s\n", numBlocks, factorizations, damped, fails ? "Failed." : "Passed.");
    return fails;
}

int main() {
    int fails = 0;
    fails += test_primitives(256);      // the reference's main(): numVars = 256 (test-qrkit.cpp:369-377)
    fails += test_fit(500);
    return fails ? 1 : 0;
}
