"""The numpy judge of the block-angular damped solve on kept factors: dense numpy QR tile by tile, no code shared
with the product.

Per left tile the stack [R_t; sqrt(par) Dt] is factorised by numpy.linalg.qr (complete), Q^T goes over [C_t; 0]; the fills join the
right stack G = [triu(R2) y2; fills; sqrt(par) D2(P2) 0], whose QR gives z2; back substitution gives z1.  tests/test_lm_panel_cpu.py
checks this prototype against numpy.linalg.lstsq on the original damped matrix.
"""
import numpy as np


def unpack_tiles(cols, r_vals):
    """The c x c upper triangles of a packed r_vals (tile after tile, each by columns: column k has k + 1 entries)."""
    out, off = [], 0
    for c in (int(v) for v in cols):
        R = np.zeros((c, c))
        for k in range(c):
            R[:k + 1, k] = r_vals[off:off + k + 1]
            off += k + 1
        out.append(R)
    return out


def tile_step(R, dt, par, C):
    """(S, top, fill) of one tile: Q, S = qr([R; sqrt(par) diag(dt)]), [top; fill] = Q^T [C; 0].  S's diagonal signs are numpy's."""
    c = R.shape[0]
    Q, S = np.linalg.qr(np.vstack([R, np.sqrt(par) * np.diag(dt)]), mode="complete")
    out = Q.T @ np.vstack([C, np.zeros_like(C)])
    return S[:c], out[:c], out[c:]


def match_signs(S, top, device_diag):
    """Rows of (S, top) flipped so that S's diagonal has the signs of device_diag (a QR is unique up to these signs)."""
    flip = np.where(np.sign(device_diag) * np.sign(np.diag(S)) < 0, -1.0, 1.0)
    return S * flip[:, None], top * flip[:, None]


def damped_solve(Rs, perm1, strip_p, R2, p2, y1, y2, diag, par):
    """x = argmin || J x - b ||^2 + par || D x ||^2 from the kept factors: Rs the left tiles' triangles, perm1 their global column
    indices, strip_p = S(:, P2) (m1 x m2), R2 (m2 x m2, upper), p2, y = Q^T b cut into y1 (m1) and y2 (m2), diag in J's column order
    (None = ones)."""
    m1, m2 = len(perm1), len(p2)
    D = np.ones(m1 + m2) if diag is None else np.asarray(diag, dtype=np.float64)
    panel = np.hstack([strip_p, y1[:, None]])
    top, fill, Ss, base = np.zeros_like(panel), np.zeros_like(panel), [], 0
    for R in Rs:
        c = R.shape[0]
        S, top[base:base + c], fill[base:base + c] = tile_step(R, D[perm1[base:base + c]], par, panel[base:base + c])
        Ss.append(S)
        base += c
    G = np.vstack([np.hstack([np.triu(R2), y2[:, None]]), fill,
                   np.hstack([np.sqrt(par) * np.diag(D[m1 + np.asarray(p2)]), np.zeros((m2, 1))])])
    Qg, Rg = np.linalg.qr(G[:, :m2])
    z2 = np.linalg.solve(Rg, Qg.T @ G[:, m2])
    rhs1 = top[:, m2] - top[:, :m2] @ z2
    z1, base = np.zeros(m1), 0
    for S in Ss:
        c = S.shape[0]
        z1[base:base + c] = np.linalg.solve(S, rhs1[base:base + c])
        base += c
    x = np.zeros(m1 + m2)
    x[np.concatenate([np.asarray(perm1), m1 + np.asarray(p2)])] = np.concatenate([z1, z2])
    return x


def damped_lstsq(J, b, diag, par):
    """The independent answer: lstsq on [J; sqrt(par) D] built from the original matrix."""
    n = J.shape[1]
    D = np.ones(n) if diag is None else np.asarray(diag, dtype=np.float64)
    A = np.vstack([J, np.sqrt(par) * np.diag(D)])
    return np.linalg.lstsq(A, np.concatenate([b, np.zeros(n)]), rcond=None)[0]
