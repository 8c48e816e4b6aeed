// C++ test of the damped solve on kept factors through the facade: BlockAngularSparseQR::lmSolve (g++ -> include/qrkit/QRKit.hpp ->
// qrk_bd_lm_panel, qrk_dense_lm_stack and the dense calls).  64 blocks of 7 x 2 next to 24 dense columns from the reference's generator
// (generate_block_angular_matrix, test/test-qrkit.cpp:132-165).  lmSolve at two values of par (diag null and a positive diag) against
// the route it replaces -- computeAndSolve() on the damped matrix [J; sqrt(par) D] in block-angular form, the damping rows of a
// block's own columns right below the block -- at 2e-9 (two device results; each answers to lstsq within 1e-9,
// tests/test_angular_lm_gpu.py); par = 0 against factorizeAndSolve()'s own x; the state before and after.
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

// the blocks (column-major br x bc each), the dense right block and the right-hand side
struct Problem {
    int nb, br, bc;
    Index m2;
    std::vector<double> blocks;
    Matrix right;
    Vector b;
};

static Problem generate(int nb, int br, int bc, Index m2) {
    std::default_random_engine gen;
    std::uniform_real_distribution<double> dist(0.5, 5.0);
    Problem p;
    p.nb = nb; p.br = br; p.bc = bc; p.m2 = m2;
    p.blocks.resize((size_t)nb * br * bc);
    for (double& v : p.blocks) v = dist(gen);
    const Index rows = (Index)nb * br;
    p.right = Matrix(rows, m2);
    for (Index i = 0; i < rows; i++) for (Index j = 0; j < m2; j++) p.right(i, j) = dist(gen);
    std::uniform_real_distribution<double> ud(-1.0, 1.0);
    p.b.resize((size_t)rows);
    for (double& v : p.b) v = ud(gen);
    return p;
}

// [J; sqrt(par) D] in block-angular form: bc damping rows below every block and m2 below J2 (damped = false: the matrix itself)
static void assemble(const Problem& p, const Vector* diag, double par, bool damped, SparseBlockDiagonal& blk, Matrix& right, Vector& b) {
    const int ex = damped ? p.bc : 0, tr = p.br + ex;
    const Index m1 = (Index)p.nb * p.bc, rows = (Index)p.nb * tr + (damped ? p.m2 : 0);
    const double sq = std::sqrt(par);
    std::vector<Triplet> t;
    for (int i = 0; i < p.nb; ++i)
        for (int j = 0; j < p.bc; ++j)
            for (int r = 0; r < tr; ++r) {
                double v = 0.0;
                if (r < p.br) v = p.blocks[(size_t)((i * p.bc + j) * p.br + r)];
                else if (r - p.br == j) v = sq * (diag ? (*diag)[(size_t)(i * p.bc + j)] : 1.0);
                t.emplace_back(i * tr + r, i * p.bc + j, v);
            }
    SparseMatrixColMajor left(rows, m1);
    left.setFromTriplets(t);
    blk.fromBlockDiagonalPattern(left, tr, p.bc);
    right = Matrix(rows, p.m2);
    b.assign((size_t)rows, 0.0);
    for (Index j = 0; j < p.m2; ++j) for (Index i = 0; i < rows; ++i) right(i, j) = 0.0;
    for (int i = 0; i < p.nb; ++i)
        for (int r = 0; r < p.br; ++r) {
            for (Index j = 0; j < p.m2; ++j) right((Index)i * tr + r, j) = p.right((Index)i * p.br + r, j);
            b[(size_t)(i * tr + r)] = p.b[(size_t)(i * p.br + r)];
        }
    if (damped)
        for (Index j = 0; j < p.m2; ++j) right((Index)p.nb * tr + j, j) = sq * (diag ? (*diag)[(size_t)(m1 + j)] : 1.0);
}

static int test_angular_lm(int nb, int br, int bc, Index m2) {
    int fails = 0;
    const Problem p = generate(nb, br, bc, m2);
    const Index cols = (Index)nb * bc + m2;
    Vector diag((size_t)cols);
    for (size_t j = 0; j < diag.size(); ++j) diag[j] = 1.0 + 0.5 * (double)(j % 3);

    Solver kept, other;
    bool threw = false;
    try { (void)kept.lmSolve(0, 1.0); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { std::printf("  lmSolve() before a factorisation did not throw\n"); ++fails; }

    SparseBlockDiagonal blk;
    Matrix right;
    Vector b;
    assemble(p, 0, 0.0, false, blk, right, b);
    BlockMatrix1x2<SparseBlockDiagonal, Matrix> mat(blk, right);
    const Vector x0 = kept.computeAndSolve(mat, b);
    if (kept.info() != Success) { std::printf("  computeAndSolve() failed\n"); return 1; }
    if (kept.leftSolver().lmPanelKernelName(m2 + 1).find("bd_lm_panel_thin_kernel") == std::string::npos) { std::printf("  not the thin panel kernel\n"); ++fails; }
    const Vector Rbefore = kept.matrixR().values();

    const Vector xz = kept.lmSolve(0, 0.0);
    const double e0 = relDiff(xz, x0);
    std::printf("  par 0 against factorizeAndSolve(): %.2e\n", e0);
    if (e0 > 1e-9) ++fails;
    const struct { double par; const Vector* diag; } cases[2] = {{1e-2, 0}, {10.0, &diag}};
    for (const auto& c : cases) {
        double dx2 = 0.0;
        const Vector x = kept.lmSolve(c.diag, c.par, &dx2);
        SparseBlockDiagonal dblk;
        Matrix dright;
        Vector db;
        assemble(p, c.diag, c.par, true, dblk, dright, db);
        BlockMatrix1x2<SparseBlockDiagonal, Matrix> dmat(dblk, dright);
        const Vector xd = other.computeAndSolve(dmat, db);
        double want = 0.0;
        for (size_t j = 0; j < xd.size(); ++j) { const double v = (c.diag ? (*c.diag)[j] : 1.0) * xd[j]; want += v * v; }
        const double ex = relDiff(x, xd), en = std::fabs(dx2 - want) / want;
        std::printf("  par %g diag %s: x against the damped computeAndSolve() %.2e, |D x|^2 %.2e\n", c.par, c.diag ? "given" : "null", ex, en);
        // (|D x|^2 of two device results that may differ by 2e-9 in x: twice that, with room)
        if (ex > 2e-9 || en > 1e-8) ++fails;
        if (relDiff(kept.lmSolve(c.diag, c.par), x) > 0.0) { std::printf("  a second lmSolve() differs\n"); ++fails; }
    }
    // W is intact: the undamped solve on the kept factors gives the same bits as before the damped ones, R reads the same, and the
    // next factorisation gives the same x
    if (relDiff(kept.lmSolve(0, 0.0), xz) > 0.0) { std::printf("  lmSolve(par = 0) changed after damped solves\n"); ++fails; }
    if (relDiff(kept.matrixR().values(), Rbefore) > 0.0) { std::printf("  R changed under lmSolve()\n"); ++fails; }
    if (relDiff(kept.factorizeAndSolve(mat, b), x0) > 0.0) { std::printf("  factorizeAndSolve() after lmSolve() differs\n"); ++fails; }
    // the explicit route keeps nothing to damp
    kept.compute(mat);
    threw = false;
    try { (void)kept.lmSolve(0, 1.0); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { std::printf("  lmSolve() after compute() did not throw\n"); ++fails; }
    std::printf("test_angular_lm %d blocks of %dx%d + %lld columns: %s\n", nb, br, bc, (long long)m2, fails ? "Failed." : "Passed.");
    return fails;
}

int main() {
    return test_angular_lm(64, 7, 2, 24) ? 1 : 0;
}
