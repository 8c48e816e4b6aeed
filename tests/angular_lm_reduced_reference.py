"""The numpy prototype of the reduced block-angular LM evaluation.  Nothing here is shared with the product.

angular_lmpar_reference.chain_evaluate with one change: the fill [F | f] (m1 x (m2 + 1), the right-hand side riding as the last
column) is reduced to one (m2 + 1) x (m2 + 1) triangle T = [T11 t; 0 rho] by a chunked Householder TSQR (numpy.linalg.qr chunk by
chunk, then of the stacked triangles), and the right stack is [R2 y2; T; sqrt(par) D2 0], (3 m2 + 1) x (m2 + 1), instead of
[R2 y2; F f; sqrt(par) D2 0].  min || [R2; F; sqrt(par) D2] z - [y2; f; 0] || and min || [R2; T11; sqrt(par) D2] z - [y2; t; 0] ||
have the same minimiser: the residuals differ by the constant rho^2.
"""
import numpy as np


def tsqr_r(A, chunk):
    """The R factor (cols x cols, zero rows appended when A has fewer rows) of A by QR of chunks of `chunk` rows and QR of the stacked
    triangles, repeated until one chunk is left.  chunk = None: one QR of the whole matrix."""
    rows, cols = A.shape
    if chunk is None:
        chunk = max(rows, 1)
    chunk = max(chunk, cols + 1)                    # (a level must shrink)
    while True:
        parts = [np.linalg.qr(A[i:i + chunk], mode="r") for i in range(0, A.shape[0], chunk)]
        A = np.vstack(parts) if parts else np.zeros((0, cols))
        if len(parts) <= 1:
            break
    R = np.zeros((cols, cols))
    R[:A.shape[0]] = np.triu(A)[:cols]
    return R


def chain_evaluate_reduced(f, diag, par, chunk):
    """(x, s0, s1) on the kept factors f (angular_lmpar_reference.KeptFactors) by the reduced route."""
    m1, m2, c = f.m1, f.m2, f.c
    D = np.ones(m1 + m2) if diag is None else np.asarray(diag, dtype=np.float64)
    panel = np.hstack([f.strip, f.y1[:, None]])
    top, fill, Ss = np.zeros_like(panel), np.zeros_like(panel), []
    for t, R in enumerate(f.Rs):
        sl = slice(t * c, (t + 1) * c)
        Q, S = np.linalg.qr(np.vstack([R, np.sqrt(par) * np.diag(D[sl])]), mode="complete")
        out = Q.T @ np.vstack([panel[sl], np.zeros((c, m2 + 1))])
        Ss.append(S[:c]); top[sl] = out[:c]; fill[sl] = out[c:]
    T = tsqr_r(fill, chunk)                                                               # (m2 + 1) x (m2 + 1)
    G = np.vstack([np.hstack([np.triu(f.R2), f.y2[:, None]]), T, np.hstack([np.sqrt(par) * np.diag(D[m1:]), np.zeros((m2, 1))])])
    assert G.shape == (3 * m2 + 1, m2 + 1)
    Qg, Rg = np.linalg.qr(G[:, :m2])
    z2 = np.linalg.solve(Rg, Qg.T @ G[:, m2])
    rhs1 = top[:, m2] - top[:, :m2] @ z2
    z1 = np.concatenate([np.linalg.solve(S, rhs1[t * c:(t + 1) * c]) for t, S in enumerate(Ss)])
    z = np.concatenate([z1, z2])
    u = D * D * z
    w1 = np.concatenate([np.linalg.solve(S.T, u[t * c:(t + 1) * c]) for t, S in enumerate(Ss)])
    w2 = np.linalg.solve(Rg.T, u[m1:] - top[:, :m2].T @ w1)
    return z, float(np.sum((D * z) ** 2)), float(w1 @ w1 + w2 @ w2)
