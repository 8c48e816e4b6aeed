// C++ test of the device-side lmpar through the facade: BlockDiagonalSparseQR::lmparDevice (qrk_bd_lmpar_device, one enqueue and one
// download per search) against BlockDiagonalSparseQR::lmpar (qrk_bd_lmpar, one synchronisation per evaluation) on the same factors.
// Both run the same kernels' sums and the same scalar steps: the pass counts are equal, par agrees to 1e-12 and x to the tolerances
// of the plain solve (1e-11 on (0.5, 5.0) data, 1e-9 on (-1, 1) data).
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

static int test_case(int numBlocks, int br, int bc, double lo, double hi, double xtol, const char* kernel) {
    std::default_random_engine gen(17u + (unsigned)(br * 100 + bc));
    std::uniform_real_distribution<double> dist(lo, hi), rhs(-1.0, 1.0);
    SparseBlockDiagonal m;
    Matrix a(br, bc);
    for (int i = 0; i < numBlocks; ++i) { for (int e = 0; e < br * bc; ++e) a.data()[e] = dist(gen); m.insertBack(a); }
    m.setDims(numBlocks * br, numBlocks * bc);
    Vector b((size_t)(numBlocks * br));
    for (double& v : b) v = rhs(gen);
    const size_t n = (size_t)(numBlocks * bc);

    int fails = 0;
    BlockDiagonalSparseQR<> qr;
    Vector qtb;
    const Vector x0 = qr.computeAndSolve(m, b, &qtb);
    if (qr.lmKernelName().find(kernel) == std::string::npos) { std::printf("  kernel %s, expected %s\n", qr.lmKernelName().c_str(), kernel); ++fails; }
    Vector diag = qr.colNorms();
    for (double& v : diag) if (v == 0.0) v = 1.0;
    double dx0 = 0;
    for (size_t j = 0; j < n; ++j) dx0 += diag[j] * diag[j] * x0[j] * x0[j];
    dx0 = std::sqrt(dx0);
    const double factors[4] = {2.0, 0.5, 0.1, 0.01};
    for (double f : factors) {
        const double delta = f * dx0;
        double parH = 0.0, parD = 0.0;
        int itH = -1, itD = -2;
        Vector trH, trD;
        const Vector xH = qr.lmpar(qtb, &diag, delta, parH, &itH, &trH);
        const Vector xD = qr.lmparDevice(qtb, &diag, delta, parD, &itD, &trD);
        const double dpar = parH != 0.0 ? std::fabs(parD - parH) / parH : std::fabs(parD);
        const double dx = relDiff(xD, xH);
        bool ok = itD == itH && dpar <= 1e-12 && dx <= xtol && trD.size() == trH.size();
        for (size_t e = 0; ok && e < trH.size(); ++e) ok = std::fabs(trD[e] - trH[e]) <= 1e-12 * std::fabs(trH[e]);
        if (f == 2.0) ok = ok && parD == 0.0 && itD == 0 && relDiff(xD, x0) <= 2 * xtol;
        else {
            double dxn = 0;
            for (size_t j = 0; j < n; ++j) dxn += diag[j] * diag[j] * xD[j] * xD[j];
            ok = ok && parD > 0.0 && itD >= 1 && std::fabs(std::sqrt(dxn) - delta) <= 0.1 * delta;
        }
        if (!ok) {
            std::printf("  delta = %g |D x0|: device par %.17g in %d passes, host par %.17g in %d passes, x differs by %g\n", f, parD, itD, parH, itH, dx);
            ++fails;
        }
    }
    // a refused value never reaches the device
    bool threw = false;
    double pv = 0.0;
    try { (void)qr.lmparDevice(qtb, &diag, 0.0, pv); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) { std::printf("  delta = 0 was not refused\n"); ++fails; }
    std::printf("lmparDevice against lmpar, %d blocks of %dx%d: %s\n", numBlocks, br, bc, fails ? "Failed." : "Passed.");
    return fails;
}

int main() {
    int fails = 0;
    fails += test_case(300, 7, 2, 0.5, 5.0, 1e-11, "bd_lm_thin_kernel");
    fails += test_case(300, 8, 6, -1.0, 1.0, 1e-9, "bd_lm_group_kernel<8>");
    return fails ? 1 : 0;
}
