// C++ test of the reduced LM route through the facade: BlockAngularSparseQR::setLmRoute / lmRoute, lmSolve and lmpar
// with the fill reduced to one triangle by qrk_dense_qless_r, and qrkit::DenseQlessR (g++ -> include/qrkit/QRKit.hpp).  64 blocks of
// 7 x 2 next to 24 dense columns, as tests/cpp/test_angular_lm.cpp generates them.  The reduced route against the stacked route on a
// second object at 2e-9 (two device results), par = 0 against factorizeAndSolve()'s x at 1e-9, lmpar on the two routes with the same
// passes and par within 1e-9 relative, x = lmSolve(diag, par) of the same route bit for bit, and each route's own bits again after
// switching back and forth.
#include <cmath>
#include <cstdio>
#include <random>
#include <stdexcept>

#include "qrkit/QRKit.hpp"

using namespace qrkit;

static double relDiff(const Vector& a, const Vector& b) {
    if (a.size() != b.size()) return 1e300;
    double num = 0, na = 0, nb = 0;
    for (size_t i = 0; i < a.size(); ++i) { const double d = a[i] - b[i]; num += d * d; na += a[i] * a[i]; nb += b[i] * b[i]; }
    const double den = std::sqrt(std::min(na, nb));
    return den > 0 ? std::sqrt(num) / den : std::sqrt(num);
}

typedef BlockAngularSparseQR<BlockDiagonalSparseQR<ColPivHouseholderQR>, ColPivHouseholderQR> Solver;

static int test_routes(int nb, int br, int bc, Index m2) {
    int fails = 0;
    std::default_random_engine gen;
    std::uniform_real_distribution<double> dist(0.5, 5.0), ud(-1.0, 1.0);
    const Index rows = (Index)nb * br, m1 = (Index)nb * bc, cols = m1 + m2;
    std::vector<Triplet> t;
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < bc; ++j)
            for (int r = 0; r < br; ++r) t.emplace_back(i * br + r, i * bc + j, dist(gen));
    SparseMatrixColMajor left(rows, m1);
    left.setFromTriplets(t);
    SparseBlockDiagonal blk;
    blk.fromBlockDiagonalPattern(left, br, bc);
    Matrix right(rows, m2);
    for (Index i = 0; i < rows; i++) for (Index j = 0; j < m2; j++) right(i, j) = dist(gen);
    Vector b((size_t)rows), diag((size_t)cols);
    for (double& v : b) v = ud(gen);
    for (size_t j = 0; j < diag.size(); ++j) diag[j] = 1.0 + 0.5 * (double)(j % 3);
    BlockMatrix1x2<SparseBlockDiagonal, Matrix> mat(blk, right);

    Solver red, stk;
    bool threw = false;
    try { (void)red.lmRoute(); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { std::printf("  lmRoute() under auto before a factorisation did not throw\n"); ++fails; }
    threw = false;
    try { red.setLmRoute("fastest"); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) { std::printf("  setLmRoute(\"fastest\") did not throw\n"); ++fails; }
    const Vector x0 = red.computeAndSolve(mat, b);
    (void)stk.computeAndSolve(mat, b);
    stk.setLmRoute("stacked");
    if (red.lmRoute() != "reduced" || stk.lmRoute() != "stacked") { std::printf("  routes: %s / %s\n", red.lmRoute().c_str(), stk.lmRoute().c_str()); ++fails; }

    const double e0 = relDiff(red.lmSolve(0, 0.0), x0);
    std::printf("  reduced, par 0 against factorizeAndSolve(): %.2e\n", e0);
    if (e0 > 1e-9) ++fails;
    const struct { double par; const Vector* diag; } cases[3] = {{0.0, &diag}, {1e-2, 0}, {10.0, &diag}};
    for (const auto& c : cases) {
        double dr = 0.0, ds = 0.0;
        const Vector xr = red.lmSolve(c.diag, c.par, &dr), xs = stk.lmSolve(c.diag, c.par, &ds);
        const double ex = relDiff(xr, xs), en = std::fabs(dr - ds) / ds;
        std::printf("  par %g diag %s: reduced against stacked %.2e, |D x|^2 %.2e\n", c.par, c.diag ? "given" : "null", ex, en);
        if (ex > 2e-9 || en > 1e-8) ++fails;
        if (relDiff(red.lmSolve(c.diag, c.par), xr) > 0.0) { std::printf("  a second reduced lmSolve() differs\n"); ++fails; }
    }
    // lmpar on the two routes at delta = 0.1 || D x0 ||
    double n0 = 0.0;
    for (size_t j = 0; j < x0.size(); ++j) n0 += diag[j] * x0[j] * diag[j] * x0[j];
    const double delta = 0.1 * std::sqrt(n0);
    double pr = 0.0, ps = 0.0;
    int ir = -1, is = -1;
    const Vector lr = red.lmpar(&diag, delta, pr, &ir), ls = stk.lmpar(&diag, delta, ps, &is);
    std::printf("  lmpar: reduced par %.6e after %d passes, stacked %.6e after %d\n", pr, ir, ps, is);
    if (ir != is || !(pr > 0.0) || std::fabs(pr - ps) > 1e-9 * ps || relDiff(lr, ls) > 2e-9) ++fails;
    if (relDiff(lr, red.lmSolve(&diag, pr)) > 0.0) { std::printf("  lmpar's x is not lmSolve's on the reduced route\n"); ++fails; }
    // switching: each route repeats its own bits on one object
    const Vector a1 = red.lmSolve(&diag, 0.25);
    red.setLmRoute("stacked");
    const Vector s1 = red.lmSolve(&diag, 0.25);
    red.setLmRoute("auto");
    const Vector a2 = red.lmSolve(&diag, 0.25);
    red.setLmRoute("stacked");
    const Vector s2 = red.lmSolve(&diag, 0.25);
    if (relDiff(a1, a2) > 0.0 || relDiff(s1, s2) > 0.0 || relDiff(s1, stk.lmSolve(&diag, 0.25)) > 0.0 || relDiff(a1, s1) > 2e-9) {
        std::printf("  switching routes changed a route's bits\n"); ++fails;
    }
    red.setLmRoute("auto");
    if (relDiff(red.factorizeAndSolve(mat, b), x0) > 0.0) { std::printf("  factorizeAndSolve() after the damped solves differs\n"); ++fails; }
    std::printf("test_angular_lm_reduced %d blocks of %dx%d + %lld columns: %s\n", nb, br, bc, (long long)m2, fails ? "Failed." : "Passed.");
    return fails;
}

// more than 31 right columns: "auto" is the stacked route, "reduced" throws at the evaluation
static int test_edge() {
    int fails = 0;
    std::default_random_engine gen(7);
    std::uniform_real_distribution<double> dist(0.5, 5.0);
    const int nb = 40, br = 3, bc = 2;
    const Index m2 = 32, rows = (Index)nb * br + m2 + 4, m1 = (Index)nb * bc;
    std::vector<Triplet> t;
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < bc; ++j)
            for (int r = 0; r < br; ++r) t.emplace_back(i * br + r, i * bc + j, dist(gen));
    SparseMatrixColMajor left((Index)nb * br, m1);
    left.setFromTriplets(t);
    SparseBlockDiagonal blk;
    blk.fromBlockDiagonalPattern(left, br, bc);
    Matrix right(rows, m2);
    for (Index i = 0; i < rows; i++) for (Index j = 0; j < m2; j++) right(i, j) = dist(gen);
    Vector b((size_t)rows);
    for (double& v : b) v = dist(gen);
    BlockMatrix1x2<SparseBlockDiagonal, Matrix> mat(blk, right);
    Solver s;
    (void)s.computeAndSolve(mat, b);
    if (s.lmRoute() != "stacked") { std::printf("  m2 = 32 under auto: %s\n", s.lmRoute().c_str()); ++fails; }
    const Vector x = s.lmSolve(0, 0.5);
    s.setLmRoute("reduced");
    bool threw = false;
    try { (void)s.lmSolve(0, 0.5); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { std::printf("  the reduced route with m2 = 32 did not throw\n"); ++fails; }
    s.setLmRoute("stacked");
    if (relDiff(s.lmSolve(0, 0.5), x) > 0.0) { std::printf("  stacked differs from auto at m2 = 32\n"); ++fails; }
    std::printf("test_angular_lm_reduced edge (m2 = 32): %s\n", fails ? "Failed." : "Passed.");
    return fails;
}

static int test_dense_qless_r(Index rows, Index cols) {
    int fails = 0;
    std::default_random_engine gen(3);
    std::normal_distribution<double> nd(0.0, 1.0);
    Matrix A(rows, cols);
    for (Index j = 0; j < cols; ++j) for (Index i = 0; i < rows; ++i) A(i, j) = nd(gen);
    DenseQlessR q;
    const Matrix R = q.compute(A).matrixR();
    double worst = 0.0, scale = 1.0;
    bool lower = false;
    for (Index i = 0; i < cols; ++i)
        for (Index j = 0; j < cols; ++j) {
            double g = 0.0, rr = 0.0;
            for (Index k = 0; k < rows; ++k) g += A(k, i) * A(k, j);
            for (Index k = 0; k < cols; ++k) rr += R(k, i) * R(k, j);
            worst = std::max(worst, std::fabs(rr - g));
            scale = std::max(scale, std::fabs(g));
            if (i > j && R(i, j) != 0.0) lower = true;
        }
    std::printf("  DenseQlessR %lld x %lld: | R^T R - A^T A | = %.2e of the scale\n", (long long)rows, (long long)cols, worst / scale);
    if (worst > 1e-11 * scale || lower || R.rows() != cols || R.cols() != cols || q.rows() != rows) ++fails;
    Matrix again = q.compute(A).matrixR();
    for (Index i = 0; i < cols; ++i) for (Index j = 0; j < cols; ++j) if (again(i, j) != R(i, j)) { ++fails; i = cols; break; }
    std::printf("test_dense_qless_r: %s\n", fails ? "Failed." : "Passed.");
    return fails;
}

int main() {
    int fails = test_routes(64, 7, 2, 24);
    fails += test_edge();
    fails += test_dense_qless_r(4097, 17);
    return fails ? 1 : 0;
}
