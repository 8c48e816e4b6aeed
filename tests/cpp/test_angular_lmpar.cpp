// C++ test of lmpar on kept factors through the facade: BlockAngularSparseQR::lmpar / lmGradient (g++ -> include/qrkit/QRKit.hpp ->
// qrk_bd_solve_rt, qrk_dense_gemv_t, qrk_dense_solve_rt, qrk_dense_trmv_t, qrk_lmpar_begin / qrk_lmpar_next).  One thin problem (64
// blocks of 7 x 2 next to 24 dense columns) and one general (20 blocks of 8 x 6 next to 9), from the reference's generator
// (generate_block_angular_matrix, test/test-qrkit.cpp:132-165), each with diag null and a positive diag.  Everything is recomputed here:
//   lmGradient against J^T b formed on the host from the blocks (1e-11);
//   lmpar at delta = f || D x0 ||, f = 0.1 and 0.5: | || D x || - delta | <= 0.1 delta after 1 .. 9 passes, x = lmSolve(diag, par) bit
//   for bit, x against computeAndSolve() on the damped matrix [J; sqrt(par) D] (2e-9, tests/cpp/test_angular_lm.cpp's bound), and the
//   last trace row: s0 = || D x ||^2 of that route, s1 = u^T v with (J^T J + par D^2) v = u = D^2 x, v again from computeAndSolve() on
//   the damped matrix with the right-hand side [0; u / (sqrt(par) D)] (1e-8: two device results of 2e-9 each);
//   f = 2: par = 0, no pass, x = lmSolve(diag, 0); a start value above the root; the refusals; the state before and after.
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

struct Problem {
    int nb, br, bc;
    Index m2;
    std::vector<double> blocks;      // column-major br x bc each
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

// [J; sqrt(par) D] in block-angular form: bc damping rows below every block and m2 below J2 (damped = false: the matrix itself);
// b = the right-hand side next to J's rows, and `below` (cols entries, J's column order, may be null) next to the damping rows
static void assemble(const Problem& p, const Vector* diag, double par, bool damped, const Vector* below, SparseBlockDiagonal& blk,
                     Matrix& right, Vector& b, bool with_b = true) {
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
    for (int i = 0; i < p.nb; ++i) {
        for (int r = 0; r < p.br; ++r) {
            for (Index j = 0; j < p.m2; ++j) right((Index)i * tr + r, j) = p.right((Index)i * p.br + r, j);
            if (with_b) b[(size_t)(i * tr + r)] = p.b[(size_t)(i * p.br + r)];
        }
        if (damped && below)
            for (int j = 0; j < p.bc; ++j) b[(size_t)(i * tr + p.br + j)] = (*below)[(size_t)(i * p.bc + j)];
    }
    if (damped)
        for (Index j = 0; j < p.m2; ++j) {
            right((Index)p.nb * tr + j, j) = sq * (diag ? (*diag)[(size_t)(m1 + j)] : 1.0);
            if (below) b[(size_t)((Index)p.nb * tr + j)] = (*below)[(size_t)(m1 + j)];
        }
}

static double dnorm(const Vector* diag, const Vector& x) {
    double s = 0.0;
    for (size_t j = 0; j < x.size(); ++j) { const double v = (diag ? (*diag)[j] : 1.0) * x[j]; s += v * v; }
    return std::sqrt(s);
}

static int test_angular_lmpar(int nb, int br, int bc, Index m2, bool thin) {
    int fails = 0;
    const Problem p = generate(nb, br, bc, m2);
    const Index m1 = (Index)nb * bc, cols = m1 + m2;
    Vector dgiven((size_t)cols);
    for (size_t j = 0; j < dgiven.size(); ++j) dgiven[j] = 1.0 + 0.5 * (double)(j % 3);

    Solver kept, other;
    double par = 0.0;
    bool threw = false;
    try { (void)kept.lmpar(0, 1.0, par); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { std::printf("  lmpar() before a factorisation did not throw\n"); ++fails; }
    threw = false;
    try { (void)kept.lmGradient(); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { std::printf("  lmGradient() before a factorisation did not throw\n"); ++fails; }

    SparseBlockDiagonal blk;
    Matrix right;
    Vector b;
    assemble(p, 0, 0.0, false, 0, blk, right, b);
    BlockMatrix1x2<SparseBlockDiagonal, Matrix> mat(blk, right);
    const Vector x0 = kept.computeAndSolve(mat, b);
    if (kept.info() != Success) { std::printf("  computeAndSolve() failed\n"); return 1; }
    const std::string name = kept.leftSolver().solveRtKernelName();
    if ((name.find("bd_solve_rt_thin_kernel") != std::string::npos) != thin || name.find("unsupported") != std::string::npos) {
        std::printf("  unexpected kernel %s\n", name.c_str()); ++fails;
    }
    const Vector Rbefore = kept.matrixR().values();

    // J^T b on the host
    Vector jtb((size_t)cols, 0.0);
    for (int i = 0; i < nb; ++i)
        for (int j = 0; j < bc; ++j)
            for (int r = 0; r < br; ++r) jtb[(size_t)(i * bc + j)] += p.blocks[(size_t)((i * bc + j) * br + r)] * p.b[(size_t)(i * br + r)];
    for (Index j = 0; j < m2; ++j)
        for (Index i = 0; i < (Index)nb * br; ++i) jtb[(size_t)(m1 + j)] += p.right(i, j) * p.b[(size_t)i];

    const Vector* diags[2] = {0, &dgiven};
    for (const Vector* diag : diags) {
        const char* dn = diag ? "given" : "null";
        double gnorm = 0.0, want = 0.0;
        const Vector g = kept.lmGradient(diag, &gnorm);
        for (size_t j = 0; j < jtb.size(); ++j) { const double q = jtb[j] / (diag ? (*diag)[j] : 1.0); want += q * q; }
        want = std::sqrt(want);
        const double eg = relDiff(g, jtb), en = std::fabs(gnorm - want) / want;
        std::printf("  diag %s: g against J^T b %.2e, gnorm %.2e\n", dn, eg, en);
        if (eg > 1e-11 || en > 1e-11) ++fails;

        const Vector xz = kept.lmSolve(diag, 0.0);
        const double dx0 = dnorm(diag, xz);
        const double fs[2] = {0.1, 0.5};
        for (double f : fs) {
            const double delta = f * dx0;
            int iters = -1;
            Vector trace;
            par = 0.0;
            const Vector x = kept.lmpar(diag, delta, par, &iters, &trace);
            const double dxn = dnorm(diag, x);
            std::printf("  diag %s f %g: par %.6e after %d passes, | |D x| - delta | / delta %.3f\n", dn, f, par, iters, std::fabs(dxn - delta) / delta);
            if (!(par > 0.0) || iters < 1 || iters > 9 || std::fabs(dxn - delta) > 0.1 * delta) { std::printf("  lmpar did not meet the radius\n"); ++fails; continue; }
            if ((int)trace.size() != 3 * (iters + 1) || trace[0] != 0.0 || trace[(size_t)(3 * iters)] != par) { std::printf("  the trace is not lmpar's\n"); ++fails; continue; }
            if (relDiff(kept.lmSolve(diag, par), x) > 0.0) { std::printf("  x is not lmSolve(diag, par), bit for bit\n"); ++fails; }
            // the damped matrix's own solution, and (J^T J + par D^2) v = u through the same route
            SparseBlockDiagonal dblk;
            Matrix dright;
            Vector db;
            assemble(p, diag, par, true, 0, dblk, dright, db);
            BlockMatrix1x2<SparseBlockDiagonal, Matrix> dmat(dblk, dright);
            const Vector xd = other.computeAndSolve(dmat, db);
            Vector u(xd.size()), below(xd.size());
            for (size_t j = 0; j < xd.size(); ++j) {
                const double d = diag ? (*diag)[j] : 1.0;
                u[j] = d * d * xd[j];
                below[j] = u[j] / (std::sqrt(par) * d);
            }
            assemble(p, diag, par, true, &below, dblk, dright, db, false);
            BlockMatrix1x2<SparseBlockDiagonal, Matrix> vmat(dblk, dright);
            const Vector v = other.computeAndSolve(vmat, db);
            double s1 = 0.0;
            for (size_t j = 0; j < v.size(); ++j) s1 += u[j] * v[j];
            const double s0 = dnorm(diag, xd) * dnorm(diag, xd);
            const double ex = relDiff(x, xd), e0 = std::fabs(trace[(size_t)(3 * iters + 1)] - s0) / s0, e1 = std::fabs(trace[(size_t)(3 * iters + 2)] - s1) / s1;
            std::printf("  diag %s f %g: x against the damped computeAndSolve() %.2e, s0 %.2e, s1 %.2e\n", dn, f, ex, e0, e1);
            if (ex > 2e-9 || e0 > 1e-8 || e1 > 1e-8) ++fails;
            // a second call repeats it to the bit; a start value far above the root still meets the radius
            double par2 = 0.0, par3 = 1e9;
            int it2 = -1;
            if (relDiff(kept.lmpar(diag, delta, par2, &it2), x) > 0.0 || par2 != par || it2 != iters) { std::printf("  a second lmpar() differs\n"); ++fails; }
            const Vector x3 = kept.lmpar(diag, delta, par3);
            if (!(par3 > 0.0) || std::fabs(dnorm(diag, x3) - delta) > 0.1 * delta) { std::printf("  lmpar from par = 1e9 did not meet the radius\n"); ++fails; }
        }
        // the Gauss-Newton step lies inside a region of twice its length
        int iters = -1;
        par = 3.0;
        const Vector xg = kept.lmpar(diag, 2.0 * dx0, par, &iters);
        if (par != 0.0 || iters != 0 || relDiff(xg, xz) > 0.0) { std::printf("  f = 2 did not return the Gauss-Newton step\n"); ++fails; }
    }
    // refusals
    const double bad[3] = {0.0, -1.0, std::nan("")};
    for (double delta : bad) {
        threw = false; par = 0.0;
        try { (void)kept.lmpar(0, delta, par); } catch (const std::invalid_argument&) { threw = true; }
        if (!threw) { std::printf("  lmpar(delta = %g) did not throw\n", delta); ++fails; }
    }
    threw = false; par = -1.0;
    try { (void)kept.lmpar(0, 1.0, par); } catch (const std::invalid_argument&) { threw = true; }
    if (!threw) { std::printf("  lmpar(par < 0) did not throw\n"); ++fails; }
    // W is intact
    if (relDiff(kept.matrixR().values(), Rbefore) > 0.0) { std::printf("  R changed under lmpar()\n"); ++fails; }
    if (relDiff(kept.factorizeAndSolve(mat, b), x0) > 0.0) { std::printf("  factorizeAndSolve() after lmpar() differs\n"); ++fails; }
    kept.compute(mat);
    threw = false; par = 0.0;
    try { (void)kept.lmpar(0, 1.0, par); } catch (const std::runtime_error&) { threw = true; }
    if (!threw) { std::printf("  lmpar() after compute() did not throw\n"); ++fails; }
    std::printf("test_angular_lmpar %d blocks of %dx%d + %lld columns: %s\n", nb, br, bc, (long long)m2, fails ? "Failed." : "Passed.");
    return fails;
}

int main() {
    int fails = test_angular_lmpar(64, 7, 2, 24, true);
    fails += test_angular_lmpar(20, 8, 6, 9, false);
    return fails ? 1 : 0;
}
