"""The judge of the Levenberg-Marquardt tests: a dense numpy restatement of what qrk_bd_lm_solve / qrk_bd_lm_gradient /
qrk_bd_r_col_norms / qrk_bd_lmpar compute, tile by tile, from the SAME packed R, permutation and y the device call reads.

z per tile by numpy.linalg.lstsq on the stack [R; sqrt(par) Dt], S by numpy.linalg.qr(stack, mode="r"), the sums from those, and
lmpar as the loop spelled out in include/qrkit_amd.h.  Nothing here is shared with the product.
"""
import numpy as np


def unpack_r(r_vals, cols):
    """The dense upper triangles of the packed m_R values (column p of a tile is the run at p (p + 1) / 2)."""
    out, off = [], 0
    for c in np.asarray(cols).tolist():
        R = np.zeros((c, c))
        for p in range(c):
            R[:p + 1, p] = r_vals[off + p * (p + 1) // 2: off + p * (p + 1) // 2 + p + 1]
        out.append(R)
        off += c * (c + 1) // 2
    return out


class Tiles:
    """R, the permutation and y of one batch, cut into tiles once."""

    def __init__(self, cols, r_vals, perm, y):
        self.cols = np.asarray(cols, np.int64)
        self.n = int(self.cols.sum())
        self.base = np.concatenate([[0], np.cumsum(self.cols)[:-1]]).astype(np.int64)
        self.R = unpack_r(np.asarray(r_vals, np.float64), self.cols)
        self.perm = np.asarray(perm, np.int64)[:self.n]
        self.y = np.asarray(y, np.float64).ravel()[:self.n]

    def tile(self, t, diag):
        b, c = int(self.base[t]), int(self.cols[t])
        p = self.perm[b:b + c]
        return self.R[t], p, self.y[b:b + c], (np.ones(c) if diag is None else np.asarray(diag, np.float64)[p])


def solve(tiles, diag, par):
    """(x, sums[3], z per tile): the damped solve with MINPACK's nsing rule per tile."""
    x = np.zeros(tiles.n)
    sums = np.zeros(3)
    zs = []
    for t in range(len(tiles.cols)):
        R, p, y, d = tiles.tile(t, diag)
        c = len(p)
        stack = np.vstack([R, np.sqrt(par) * np.diag(d)])
        S = np.atleast_2d(np.linalg.qr(stack, mode="r"))
        if np.any(np.diag(R) == 0.0):
            sums[2] += 1.0
        zero = np.flatnonzero(np.diag(S) == 0.0) if par > 0.0 else np.flatnonzero(np.diag(R) == 0.0)
        k0 = int(zero[0]) if zero.size else c
        z = np.zeros(c)
        if k0 > 0:
            z[:k0] = np.linalg.lstsq(stack[:, :k0], np.concatenate([y, np.zeros(c)]), rcond=None)[0] if k0 == c else \
                np.linalg.lstsq(R[:k0, :k0], y[:k0], rcond=None)[0]
        x[p] = z
        zs.append(z)
        sums[0] += float(np.sum((d * z) ** 2))
        if k0 == c:
            w = np.linalg.solve(S.T, d * d * z)
            sums[1] += float(np.sum(w ** 2))
    return x, sums, zs


def gradient(tiles, diag):
    """(g, gnorm2): g = P R^T y in the matrix's column order, gnorm2 = sum (g_j / diag_j)^2."""
    g = np.zeros(tiles.n)
    for t in range(len(tiles.cols)):
        R, p, y, _ = tiles.tile(t, None)
        g[p] = R.T @ y
    d = np.ones(tiles.n) if diag is None else np.asarray(diag, np.float64)
    return g, float(np.sum((g / d) ** 2))


def col_norms(tiles):
    out = np.zeros(tiles.n)
    for t in range(len(tiles.cols)):
        R, p, _, _ = tiles.tile(t, None)
        out[p] = np.linalg.norm(R, axis=0)
    return out


def lmpar(tiles, diag, delta, par=0.0):
    """(par, x, iters, trace): the loop of include/qrkit_amd.h, qrk_bd_lmpar, steps 1-6."""
    dbl_min = np.finfo(np.float64).tiny
    trace = []

    def evaluate(pv):
        x, s, _ = solve(tiles, diag, pv)
        trace.append((pv, s[0], s[1]))
        return x, s

    x, s = evaluate(0.0)
    dxnorm = np.sqrt(s[0])
    fp = dxnorm - delta
    if fp <= 0.1 * delta:
        return 0.0, x, 0, np.array(trace)
    parl = 0.0 if s[2] > 0 else fp / (delta * s[1] / s[0])
    gnorm = np.sqrt(gradient(tiles, diag)[1])
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
        x, s = evaluate(par)
        dxnorm = np.sqrt(s[0])
        temp = fp
        fp = dxnorm - delta
        if abs(fp) <= 0.1 * delta or (parl == 0.0 and fp <= temp and temp < 0.0) or it == 10:
            break
        parc = fp / (delta * s[1] / s[0])
        if fp > 0.0:
            parl = max(parl, par)
        if fp < 0.0:
            paru = min(paru, par)
        par = max(parl, par + parc)
    return par, x, it, np.array(trace)


def per_tile_rel(got, want, tiles):
    """Largest relative error of x over the tiles (x in the matrix's column order: tile t owns perm[base : base + c])."""
    worst = 0.0
    for t in range(len(tiles.cols)):
        b, c = int(tiles.base[t]), int(tiles.cols[t])
        p = tiles.perm[b:b + c]
        den = np.linalg.norm(want[p])
        num = np.linalg.norm(np.asarray(got)[p] - want[p])
        worst = max(worst, num / den if den > 0 else num)
    return worst
