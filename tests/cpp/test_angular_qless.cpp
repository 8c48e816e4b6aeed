// C++ test of the fused Levenberg-Marquardt step through the facade: BlockAngularSparseQR::computeAndSolve / factorizeAndSolve
// (g++ -> include/qrkit/QRKit.hpp -> qrk_bd_factorize_apply_qt and the dense right solver on one device matrix W).  Inputs from the
// reference's generator (generate_block_angular_matrix, test/test-qrkit.cpp:132-165: default_random_engine +
// uniform_real_distribution(0.5, 5.0)): 100 blocks of 7 x 2 next to 30 dense columns with 17 rows below J1, dense and sparse right
// blocks, and the ellipse shape of examples/ellipse_fitting.cpp:117-142 (300 blocks of 2 x 1 next to 5 columns).  Checked by the
// reference's own invariant -- the recovery of x from b = J x at 1e-6 (test/test.h:31) -- and against compute() + solve() at 2e-9
// (both routes answer to the oracle within 1e-9, tests/test_angular.py), plus the state afterwards.
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

// numBlocks blocks of br x bc on the diagonal of `left` ((numBlocks br + extraRows) x numBlocks bc), a dense `right` with m2 columns
static void generate_block_angular(int numBlocks, int br, int bc, Index m2, Index extraRows, SparseMatrixColMajor& left, Matrix& right) {
    std::default_random_engine gen;
    std::uniform_real_distribution<double> dist(0.5, 5.0);
    const Index rows = (Index)numBlocks * br + extraRows, m1 = (Index)numBlocks * bc;
    std::vector<Triplet> jvals;
    for (int i = 0; i < numBlocks; i++)
        for (int j = 0; j < bc; ++j)
            for (int r = 0; r < br; ++r) jvals.emplace_back(i * br + r, i * bc + j, dist(gen));
    right = Matrix(rows, m2);
    for (Index i = 0; i < rows; i++) for (Index j = 0; j < m2; j++) right(i, j) = dist(gen);
    left.resize(rows, m1);
    left.setFromTriplets(jvals);
}

template <typename F>
static bool throwsRuntimeError(F f) {
    try { f(); } catch (const std::runtime_error&) { return true; }
    return false;
}

typedef BlockAngularSparseQR<BlockDiagonalSparseQR<ColPivHouseholderQR>, ColPivHouseholderQR> Solver;

template <typename RightMat>
static int check_step(const SparseBlockDiagonal& blk, const RightMat& rightForSolver, const Vector& x, const Vector& b, const Vector& xRef,
                      const Vector& yRef, const Solver& ref, const char* what) {
    int fails = 0;
    Solver fused;
    BlockMatrix1x2<SparseBlockDiagonal, RightMat> mat(blk, rightForSolver);
    Vector y;
    const Vector xf = fused.computeAndSolve(mat, b, &y);
    if (fused.info() != Success || fused.rank() != (Index)x.size() || fused.hasQ()) { std::printf("  %s: info / rank / state wrong\n", what); ++fails; }
    if (fused.leftSolver().panelKernelName(2).find("bdqr_thin_panel_kernel") == std::string::npos) { std::printf("  %s: not the panel kernel\n", what); ++fails; }
    if (relDiff(xf, x) > 1e-6) { std::printf("  %s: LS recovery failed: %g\n", what, relDiff(xf, x)); ++fails; }                 // (test.h:31)
    if (relDiff(xf, xRef) > 2e-9) { std::printf("  %s: x differs from compute() + solve(): %g\n", what, relDiff(xf, xRef)); ++fails; }
    if (relDiff(y, yRef) > 2e-12) { std::printf("  %s: Q^T b differs from applyQt(): %g\n", what, relDiff(y, yRef)); ++fails; }
    if (fused.colsPermutation().indices() != ref.colsPermutation().indices()) { std::printf("  %s: column permutation differs\n", what); ++fails; }
    if (fused.rowsPermutation().indices() != ref.rowsPermutation().indices()) { std::printf("  %s: row permutation differs\n", what); ++fails; }
    if (relDiff(fused.matrixR().values(), ref.matrixR().values()) > 2e-12) { std::printf("  %s: R differs\n", what); ++fails; }
    // no Q1: the accessors that need it throw, the next compute() brings them back
    if (!throwsRuntimeError([&] { (void)fused.matrixQ(); }) || !throwsRuntimeError([&] { (void)fused.solve(b); }) ||
        !throwsRuntimeError([&] { (void)fused.applyQt(b); }) || !throwsRuntimeError([&] { (void)fused.applyQ(b); })) {
        std::printf("  %s: a Q accessor did not throw after computeAndSolve()\n", what); ++fails;
    }
    // a second step on the same object (the plan and W are reused): the same bits
    if (relDiff(fused.factorizeAndSolve(mat, b), xf) > 0.0) { std::printf("  %s: a second factorizeAndSolve() differs\n", what); ++fails; }
    fused.compute(mat);
    if (!fused.hasQ() || relDiff(fused.solve(b), xRef) > 0.0) { std::printf("  %s: compute() did not restore the explicit route\n", what); ++fails; }
    // ... and the fused step again after an explicit factorisation
    if (relDiff(fused.computeAndSolve(mat, b), xf) > 0.0) { std::printf("  %s: computeAndSolve() after compute() differs\n", what); ++fails; }
    return fails;
}

static int test_angular_qless(int numBlocks, int br, int bc, Index m2, Index extraRows, bool sparseToo) {
    SparseMatrixColMajor left;
    Matrix right;
    generate_block_angular(numBlocks, br, bc, m2, extraRows, left, right);
    SparseBlockDiagonal blk;
    blk.fromBlockDiagonalPattern(left, br, bc);
    const Index rows = right.rows(), m1 = left.cols(), cols = m1 + m2;
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> ud(-1.0, 1.0);
    Vector x((size_t)cols);
    for (double& v : x) v = ud(rng);
    Vector xl(x.begin(), x.begin() + m1);
    Vector b = left * xl;
    for (Index j = 0; j < m2; ++j) for (Index i = 0; i < rows; ++i) b[(size_t)i] += right(i, j) * x[(size_t)(m1 + j)];

    Solver ref;
    BlockMatrix1x2<SparseBlockDiagonal, Matrix> mat(blk, right);
    ref.compute(mat);
    const Vector xRef = ref.solve(b), yRef = ref.applyQt(b);
    int fails = check_step(blk, right, x, b, xRef, yRef, ref, "dense right block");
    if (sparseToo) {
        std::vector<Triplet> t;
        for (Index j = 0; j < m2; ++j) for (Index i = 0; i < rows; ++i) t.emplace_back((int)i, (int)j, right(i, j));
        SparseMatrixColMajor rc(rows, m2);
        rc.setFromTriplets(t);
        SparseMatrixRowMajor rr(rows, m2);
        rr.setFromTriplets(t);
        fails += check_step(blk, rc, x, b, xRef, yRef, ref, "sparse right block (column-major)");
        fails += check_step(blk, rr, x, b, xRef, yRef, ref, "sparse right block (row-major)");
    }
    std::printf("test_angular_qless %d blocks of %dx%d + %lld columns, %lld rows below: %s\n", numBlocks, br, bc, (long long)m2,
                (long long)extraRows, fails ? "Failed." : "Passed.");
    return fails;
}

int main() {
    int fails = 0;
    fails += test_angular_qless(100, 7, 2, 30, 17, true);
    fails += test_angular_qless(300, 2, 1, 5, 0, false);       // the ellipse shape
    return fails ? 1 : 0;
}
