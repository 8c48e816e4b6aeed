"""The numpy side of the block-angular lmpar tests.  Nothing here is shared with the product.

  * the problems: the Gaussian block-angular matrices and the ellipse of tests/test_angular_lm_gpu.py, restated;
  * the factor-free judge: x by lstsq on [J; sqrt(par) D], s0 = || D x ||^2, s1 = u^T (J^T J + par D^2)^-1 u with u = D^2 x,
    g = J^T b, and MINPACK's lmpar loop (include/qrkit_amd.h, qrk_bd_lmpar, steps 1-5) over that evaluation;
  * the prototype of the transposed chain on numpy-made kept factors: per-tile solve(S^T, .), Top^T w1, solve(Rg^T, .), and the
    gradient g1 = R1^T y1, g2 = Strip^T y1 + R2^T y2.  tests/test_angular_lmpar_cpu.py checks it against the judge.
"""
import functools

import numpy as np
import scipy.sparse as sp


class Problem:
    """[J1 | J2] x = b with J1 = num_vars blocks of r x c (column-major tiles) and n2 rows below them"""

    def __init__(self, num_vars, r, c, m2, n2, tiles, J2, b):
        self.num_vars, self.r, self.c, self.m2, self.n2 = num_vars, r, c, m2, n2
        self.tiles, self.J2, self.b = tiles, J2, b
        self.blocks = [tiles[i * r * c:(i + 1) * r * c].reshape(c, r).T for i in range(num_vars)]
        J1 = sp.block_diag(self.blocks, format="csc").toarray()
        if n2:
            J1 = np.vstack([J1, np.zeros((n2, c * num_vars))])
        self.J = np.hstack([J1, J2])
        self.m1 = c * num_vars
        self.norms = np.linalg.norm(self.J, axis=0)

    def mat(self, qa):
        left = qa.SparseBlockDiagonal.fromTiles(np.full(self.num_vars, self.r, np.int32), np.full(self.num_vars, self.c, np.int32),
                                                self.tiles, rows=self.r * self.num_vars)
        return qa.BlockMatrix1x2(left, self.J2)


@functools.lru_cache(maxsize=None)
def gaussian_problem(num_vars, r, c, m2, n2, seed):
    rng = np.random.default_rng(seed)
    tiles = rng.standard_normal(num_vars * r * c)
    J2 = rng.standard_normal((num_vars * r + n2, m2))
    return Problem(num_vars, r, c, m2, n2, tiles, J2, rng.standard_normal(num_vars * r + n2))


GAUSSIAN = {"8x(2x1)": (8, 2, 1, 5, 0, 1), "64x(7x2)": (64, 7, 2, 24, 3, 2), "20x(8x6)": (20, 8, 6, 9, 2, 3),
            "300x(7x2)": (300, 7, 2, 70, 5, 4)}

# ---- the ellipse of examples/ellipse_fitting.cpp, restated ------------------------------------------------------------------------

NPTS = 300


def ellipse_model(uv):
    t, (a, b, x0, y0, r) = uv[:NPTS], uv[NPTS:]
    return np.stack([a * np.cos(t) * np.cos(r) - b * np.sin(t) * np.sin(r) + x0,
                     a * np.cos(t) * np.sin(r) + b * np.sin(t) * np.cos(r) + y0])


def ellipse_jacobian(uv, pts):
    """The undamped Jacobian of EllipseFitting (examples/ellipse_fitting.cpp:46-96) in block-angular form: one 2 x 1 block per point
    next to the 5 ellipse parameters; returns (tiles, J2, -f)."""
    t, (a, b, x0, y0, r) = uv[:NPTS], uv[NPTS:]
    f = (pts - ellipse_model(uv)).T
    ct, st, cr, sr = np.cos(t), np.sin(t), np.cos(r), np.sin(r)
    tiles = np.zeros((NPTS, 1, 2))
    tiles[:, 0, 0] = a * cr * st + b * sr * ct
    tiles[:, 0, 1] = a * sr * st - b * cr * ct
    J2 = np.zeros((NPTS, 2, 5))
    J2[:, 0, :] = np.stack([-ct * cr, st * sr, -np.ones(NPTS), np.zeros(NPTS), a * ct * sr + b * st * cr], axis=1)
    J2[:, 1, :] = np.stack([-ct * sr, -st * cr, np.zeros(NPTS), -np.ones(NPTS), -a * ct * cr + b * st * sr], axis=1)
    return tiles.ravel(), J2.reshape(2 * NPTS, 5), -f.ravel()


def ellipse_data():
    rng = np.random.default_rng(11)
    truth = np.concatenate([np.sort(rng.uniform(0.0, 2.0 * np.pi, NPTS)), [3.0, 2.0, 0.5, -0.3, 0.4]])
    pts = ellipse_model(truth)                                     # noise-free
    start = truth + np.concatenate([0.05 * rng.standard_normal(NPTS), [0.3, -0.2, 0.1, 0.1, -0.1]])
    return truth, pts, start


@functools.lru_cache(maxsize=None)
def ellipse_problem():
    _, pts, start = ellipse_data()
    tiles, J2, rhs = ellipse_jacobian(start, pts)
    return Problem(NPTS, 2, 1, 5, 0, tiles, J2, rhs)


def problem(name):
    return ellipse_problem() if name == "ellipse" else gaussian_problem(*GAUSSIAN[name])


# ---- the factor-free judge ------------------------------------------------------------------------------------------------------------

def free_evaluate(J, b, diag, par):
    """(x, s0, s1) at one par from the original matrix alone."""
    n = J.shape[1]
    D = np.ones(n) if diag is None else np.asarray(diag, dtype=np.float64)
    A = np.vstack([J, np.sqrt(par) * np.diag(D)])
    x = np.linalg.lstsq(A, np.concatenate([b, np.zeros(n)]), rcond=None)[0]
    u = D * D * x
    s1 = float(u @ np.linalg.solve(J.T @ J + par * np.diag(D * D), u))
    return x, float(np.sum((D * x) ** 2)), s1


def free_gradient(J, b, diag):
    """(g, gnorm) = (J^T b, || D^-1 J^T b ||)."""
    g = J.T @ b
    D = np.ones(J.shape[1]) if diag is None else np.asarray(diag, dtype=np.float64)
    return g, float(np.linalg.norm(g / D))


def lmpar_loop(evaluate, gnorm, delta, par=0.0):
    """MINPACK's lmpar over evaluate(par) -> (x, s0, s1): steps 1-5 of qrk_bd_lmpar (include/qrkit_amd.h) without the rank-deficient
    branch.  Returns (par, x, iters, trace, margin): margin = the smallest distance of a stop decision from its threshold 0.1 delta
    (| fp - 0.1 delta | at par = 0, | |fp| - 0.1 delta | in the loop), so that a caller can tell a decision that hangs on rounding."""
    dbl_min = np.finfo(np.float64).tiny
    trace = []

    def ev(pv):
        x, s0, s1 = evaluate(pv)
        trace.append((pv, s0, s1))
        return x, s0, s1

    x, s0, s1 = ev(0.0)
    dxnorm = np.sqrt(s0)
    fp = dxnorm - delta
    margin = abs(fp - 0.1 * delta)
    if fp <= 0.1 * delta:
        return 0.0, x, 0, np.array(trace), margin
    parl = fp / (delta * s1 / s0) if s1 > 0.0 else 0.0
    paru = gnorm / delta
    if paru == 0.0:
        paru = dbl_min / min(delta, 0.1)
    par = min(max(par, parl), paru)
    if par == 0.0:
        par = gnorm / dxnorm
    it = 0
    while True:
        it += 1
        if par == 0.0:
            par = max(dbl_min, 0.001 * paru)
        x, s0, s1 = ev(par)
        dxnorm = np.sqrt(s0)
        temp = fp
        fp = dxnorm - delta
        margin = min(margin, abs(abs(fp) - 0.1 * delta))
        if abs(fp) <= 0.1 * delta or (parl == 0.0 and fp <= temp and temp < 0.0) or it == 10:
            break
        parc = fp / (delta * s1 / s0)
        if fp > 0.0:
            parl = max(parl, par)
        if fp < 0.0:
            paru = min(paru, par)
        par = max(parl, par + parc)
    return par, x, it, np.array(trace), margin


def free_lmpar(J, b, diag, delta, par=0.0):
    return lmpar_loop(lambda pv: free_evaluate(J, b, diag, pv), free_gradient(J, b, diag)[1], delta, par)


class JudgeStepper:
    """The solver's two calls of trust_region_fit with the factor-free judge in their place"""

    def factorize(self, tiles, J2, rhs):
        self.p = Problem(NPTS, 2, 1, 5, 0, tiles, J2, rhs)

    def lmpar(self, diag, delta, par):
        par, x, _, _, _ = free_lmpar(self.p.J, self.p.b, diag, delta, par)
        return x, par


def trust_region_fit(start, pts, stepper, budget):
    """The loop of tests/test_lmpar_gpu.py's fit on the ellipse: one stepper.factorize(tiles, J2, -f) of the undamped Jacobian per
    accepted iterate, one stepper.lmpar(diag, delta, par) -> (dx, par) per trial step on the same factors, MINPACK's ratio test and
    radius update (lmder: ratio <= 1/4 halves the region, par = 0 or ratio >= 3/4 sets it to 2 |D dx|; a step is accepted from
    ratio >= 1e-4), diag = the running maximum of J's column norms, delta_0 = 1.  Stops below a cost of 1e-24 or after `budget`
    trial steps.  Returns (uv, cost, factorisations, trials)."""
    uv, delta, par, diag = start.copy(), 1.0, 0.0, None
    cost = 0.5 * np.sum((pts - ellipse_model(uv)) ** 2)
    factorisations = trials = 0
    while trials < budget and cost >= 1e-24:
        tiles, J2, rhs = ellipse_jacobian(uv, pts)
        stepper.factorize(tiles, J2, rhs)
        factorisations += 1
        norms = np.concatenate([np.linalg.norm(tiles.reshape(NPTS, 2), axis=1), np.linalg.norm(J2, axis=0)])
        diag = np.where(norms == 0.0, 1.0, norms) if diag is None else np.maximum(diag, norms)
        while trials < budget:
            dx, par = stepper.lmpar(diag, delta, par)
            trials += 1
            pnorm = np.linalg.norm(diag * dx)
            new_cost = 0.5 * np.sum((pts - ellipse_model(uv + dx)) ** 2)
            lin = rhs - (np.repeat(dx[:NPTS], 2) * tiles + J2 @ dx[NPTS:])          # -f - J dx
            predicted = cost - 0.5 * np.sum(lin ** 2)
            ratio = (cost - new_cost) / predicted if predicted > 0 else 0.0
            if ratio <= 0.25:
                delta = 0.5 * min(delta, pnorm)
            elif par == 0.0 or ratio >= 0.75:
                delta = 2.0 * pnorm
            if ratio >= 1e-4:
                uv, cost = uv + dx, new_cost
                break
    return uv, cost, factorisations, trials


# ---- the prototype of the chain on kept factors ---------------------------------------------------------------------------------------

class KeptFactors:
    """What factorizeAndSolve() keeps, made with numpy.linalg.qr (no pivoting: both permutations are the identity): the left tiles'
    triangles R_t, Strip = (Q1^T J2)(0:m1, :), R2 and y = Q^T b cut into y1, y2."""

    def __init__(self, p):
        r, c, nv, m2 = p.r, p.c, p.num_vars, p.m2
        panel = np.hstack([p.J2, p.b[:, None]])
        self.Rs, top, rest = [], [], []
        for t, T in enumerate(p.blocks):
            Q, R = np.linalg.qr(T, mode="complete")
            self.Rs.append(R[:c])
            w = Q.T @ panel[t * r:(t + 1) * r]
            top.append(w[:c]); rest.append(w[c:])
        top, rest = np.vstack(top), np.vstack(rest + [panel[nv * r:]])
        Q2, R2 = np.linalg.qr(rest[:, :m2], mode="complete")
        self.strip, self.R2 = top[:, :m2], R2[:m2]
        self.y1, self.y2 = top[:, m2], (Q2.T @ rest[:, m2])[:m2]
        self.c, self.m1, self.m2 = c, p.m1, m2


def chain_evaluate(f, diag, par):
    """(x, s0, s1) on the kept factors f: the damped elimination of lm_panel_reference.damped_solve, then the transposed pass
    w1 = S1^-T u1 tile by tile, w2 = Rg^-T (u2 - Top^T w1), s1 = |w1|^2 + |w2|^2 (the permutations are the identity)."""
    m1, m2, c = f.m1, f.m2, f.c
    D = np.ones(m1 + m2) if diag is None else np.asarray(diag, dtype=np.float64)
    panel = np.hstack([f.strip, f.y1[:, None]])
    top, fill, Ss = np.zeros_like(panel), np.zeros_like(panel), []
    for t, R in enumerate(f.Rs):
        sl = slice(t * c, (t + 1) * c)
        Q, S = np.linalg.qr(np.vstack([R, np.sqrt(par) * np.diag(D[sl])]), mode="complete")
        out = Q.T @ np.vstack([panel[sl], np.zeros((c, m2 + 1))])
        Ss.append(S[:c]); top[sl] = out[:c]; fill[sl] = out[c:]
    G = np.vstack([np.hstack([np.triu(f.R2), f.y2[:, None]]), fill, np.hstack([np.sqrt(par) * np.diag(D[m1:]), np.zeros((m2, 1))])])
    Qg, Rg = np.linalg.qr(G[:, :m2])
    z2 = np.linalg.solve(Rg, Qg.T @ G[:, m2])
    rhs1 = top[:, m2] - top[:, :m2] @ z2
    z1 = np.concatenate([np.linalg.solve(S, rhs1[t * c:(t + 1) * c]) for t, S in enumerate(Ss)])
    z = np.concatenate([z1, z2])
    u = D * D * z
    w1 = np.concatenate([np.linalg.solve(S.T, u[t * c:(t + 1) * c]) for t, S in enumerate(Ss)])
    w2 = np.linalg.solve(Rg.T, u[m1:] - top[:, :m2].T @ w1)
    return z, float(np.sum((D * z) ** 2)), float(w1 @ w1 + w2 @ w2)


def chain_gradient(f, diag):
    """(g, gnorm) on the undamped kept factors: g1 = R1^T y1 per tile, g2 = Strip^T y1 + R2^T y2."""
    c = f.c
    g1 = np.concatenate([R.T @ f.y1[t * c:(t + 1) * c] for t, R in enumerate(f.Rs)])
    g = np.concatenate([g1, f.strip.T @ f.y1 + np.triu(f.R2).T @ f.y2])
    D = np.ones(g.size) if diag is None else np.asarray(diag, dtype=np.float64)
    return g, float(np.linalg.norm(g / D))
