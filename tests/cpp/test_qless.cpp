// C++ test of the Q-less route through the facade: BlockDiagonalSparseQR::factorizeAndSolve / computeAndSolve
// (qrk_bd_factorize_rhs) on the reference's own input (generate_block_diagonal_matrix, test/test-qrkit.cpp:101-117: 7x2 blocks,
// default_random_engine + uniform_real_distribution(0.5, 5.0)): the least-squares recovery of test_block_diagonal (:203) at the
// reference's 1e-6 (test/test.h:31), agreement with compute() + solve() and with applyQt() at 1e-11, and the Q-less state
// (matrixQ() / solve() throw until the next compute()).  Also a 32x32 batch and an LM-style loop with the pattern analysed once.
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

static void generate_block_diagonal_matrix(Index numParams, Index numResiduals, int blockRows, int blockCols, SparseMatrixColMajor& spJ) {
    std::default_random_engine gen;
    std::uniform_real_distribution<double> dist(0.5, 5.0);
    std::vector<Triplet> jvals;
    for (int i = 0; i < numParams; i++)
        for (int j = i * blockCols; j < (i * blockCols) + blockCols && j < numParams; j++)
            for (int r = 0; r < blockRows; ++r) jvals.emplace_back(i * blockRows + r, j, dist(gen));
    spJ.resize(numResiduals, numParams);
    spJ.setFromTriplets(jvals);
}

template <typename F>
static bool throwsRuntimeError(F f) {
    try { f(); } catch (const std::runtime_error&) { return true; }
    return false;
}

// xtol: agreement of x with compute() + solve() (1e-11 on the 7x2 input; random 32x32 tiles amplify the rounding of Q^T b by their
// condition number, as in the reference-shaped tests of the explicit route: 1e-9)
static int test_qless(int numVars, int br, int bc, double xtol) {
    const Index numParams = (Index)numVars * bc, numResiduals = (Index)numVars * br;
    SparseMatrixColMajor spJ;
    generate_block_diagonal_matrix(numParams, numResiduals, br, bc, spJ);
    SparseBlockDiagonal blkDiag;
    blkDiag.fromBlockDiagonalPattern(spJ, br, bc);
    std::mt19937_64 rng(1);
    std::uniform_real_distribution<double> ud(-1.0, 1.0);
    Vector x((size_t)numParams);
    for (double& v : x) v = ud(rng);
    const Vector b = spJ * x;

    // the explicit-Q route: compute() + solve() + applyQt()
    BlockDiagonalSparseQR<ColPivHouseholderQR> ref;
    ref.compute(blkDiag);
    const Vector xRef = ref.solve(b), yRef = ref.applyQt(b);

    int fails = 0;
    BlockDiagonalSparseQR<ColPivHouseholderQR> qr;
    Vector y;
    const Vector xq = qr.computeAndSolve(blkDiag, b, &y);
    if (qr.info() != Success || qr.rank() != numParams || qr.hasQ()) { std::printf("  info / rank / state wrong\n"); ++fails; }
    if (relDiff(xq, x) > 1e-6) { std::printf("  LS recovery failed: %g\n", relDiff(xq, x)); ++fails; }                  // (:203)
    if (relDiff(xq, xRef) > xtol) { std::printf("  x differs from compute() + solve(): %g\n", relDiff(xq, xRef)); ++fails; }
    if (relDiff(y, yRef) > 1e-11) { std::printf("  Q^T b differs from applyQt(): %g\n", relDiff(y, yRef)); ++fails; }
    if (qr.colsPermutation().indices() != ref.colsPermutation().indices()) { std::printf("  column permutation differs\n"); ++fails; }
    if (relDiff(qr.matrixR().values(), ref.matrixR().values()) > 1e-12) { std::printf("  R differs\n"); ++fails; }
    // R and the permutation are usable without Q: x = P R^-1 (Q^T b)(0:cols)
    Vector top(y.begin(), y.begin() + numParams);
    const Vector z = qr.solveR(top);
    Vector back((size_t)numParams, 0.0);
    for (Index i = 0; i < numParams; ++i) back[(size_t)qr.colsPermutation().indices()[(size_t)i]] = z[(size_t)i];
    if (relDiff(back, xq) > xtol) { std::printf("  solveR() on the returned Q^T b differs from x\n"); ++fails; }
    // no Q: the accessors that need it throw, and the next compute() brings them back
    if (!throwsRuntimeError([&] { (void)qr.matrixQ(); }) || !throwsRuntimeError([&] { (void)qr.solve(b); }) ||
        !throwsRuntimeError([&] { (void)qr.applyQt(b); }) || !throwsRuntimeError([&] { (void)qr.applyQ(b); })) {
        std::printf("  a Q accessor did not throw after factorizeAndSolve()\n"); ++fails;
    }
    qr.compute(blkDiag);
    if (!qr.hasQ() || relDiff(qr.solve(b), xRef) > 0.0) { std::printf("  compute() did not restore the explicit-Q behaviour\n"); ++fails; }
    std::printf("test_qless %dx%d x %d blocks: %s\n", br, bc, numVars, fails ? "Failed." : "Passed.");
    return fails;
}

// An LM-style loop: analyzePattern() once, factorizeAndSolve() per iteration with new tiles and a new right-hand side
static int test_qless_loop(int numBlocks, int br, int bc) {
    std::default_random_engine gen;
    std::uniform_real_distribution<double> dist(0.5, 5.0);
    BlockDiagonalSparseQR<> qr, ref;
    int fails = 0;
    for (int it = 0; it < 3; ++it) {
        SparseBlockDiagonal m;
        Matrix a(br, bc);
        for (int i = 0; i < numBlocks; ++i) { for (int e = 0; e < br * bc; ++e) a.data()[e] = dist(gen); m.insertBack(a); }
        m.setDims(numBlocks * br, numBlocks * bc);
        Vector b((size_t)(numBlocks * br));
        for (double& v : b) v = dist(gen) - 2.5;
        if (it == 0) qr.analyzePattern(m);
        const Vector xq = qr.factorizeAndSolve(m, b);
        ref.compute(m);
        if (relDiff(xq, ref.solve(b)) > 1e-11) { std::printf("  iteration %d: x differs from compute() + solve()\n", it); ++fails; }
    }
    std::printf("Q-less loop, %d blocks of %dx%d: %s\n", numBlocks, br, bc, fails ? "Failed." : "Passed.");
    return fails;
}

int main() {
    int fails = 0;
    fails += test_qless(256, 7, 2, 1e-11);     // the reference's main(): numVars = 256 (test-qrkit.cpp:369-377)
    fails += test_qless(40, 32, 32, 1e-9);
    fails += test_qless_loop(500, 9, 2);  // the LM-damped block shape (test/test-utils.cpp:254-274)
    return fails ? 1 : 0;
}
