"""The definition of qpgpu_vjp in numpy (TEST INFRASTRUCTURE ONLY).

include/qpgpu.h fixes every operation: no FMA, every product rounded before it is added or
subtracted, IEEE division and sqrt, no branch on any pivot.  The loops below run over the index a
sum is serial in (k in the factorisation and the substitutions, i in S and r, t in y) and are
vectorised over the index it is independent in (the rows below a pivot, the columns of a right-hand
side, the entries of S): each element still sees exactly the definition's operations in the
definition's order, on np.float64, and nothing here uses `@` or a BLAS call.

vjp_box() restates the box entry's own form (generated columns of CI = [-I, +I], dhi / dlo instead of
dCI / dci0); dense_kkt() is the independent check: the (n + q) x (n + q) KKT system by
np.linalg.solve.
"""
from __future__ import annotations

import numpy as np

import qpgpu

DENSE_OUTPUTS = ("dG", "dg0", "dCE", "dce0", "dCI", "dci0")
BOX_OUTPUTS = ("dG", "dg0", "dCE", "dce0", "dhi", "dlo")


def chol(A):
    """Lower factor by the definition's order; reads the lower triangle only."""
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        s = A[j:, j].copy()  # rows i >= j, each its own serial sum over k
        for k in range(j):
            s = s - L[j:, k] * L[j, k]
        d = np.sqrt(s[0])
        L[j, j] = d
        L[j + 1:, j] = s[1:] / d
    return L


def fsub(L, r):
    """L y = r for a vector or, column by column, a matrix r."""
    y = np.zeros_like(r)
    for i in range(L.shape[0]):
        s = r[i].copy()
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s / L[i, i]
    return y


def bsub(L, r):
    """L^T z = r."""
    N = L.shape[0]
    z = np.zeros_like(r)
    for i in range(N - 1, -1, -1):
        s = r[i].copy()
        for k in range(i + 1, N):
            s = s - L[k, i] * z[k]
        z[i] = s / L[i, i]
    return z


def working_list(u, p):
    """Positions of W: (equality k) for k < p, then the inequalities i ascending with u[p+i] != 0."""
    return list(range(p)), [int(i) for i in np.nonzero(u[p:] != 0)[0]]


def _solve(G, A, gx):
    """(a, c) of the definition for the n x q working columns A."""
    n, q = A.shape
    L = chol(G)
    w = fsub(L, gx)
    M = fsub(L, A)
    S = np.zeros((q, q))
    r = np.zeros(q)
    for i in range(n):
        S = S + M[i][:, None] * M[i][None, :]
        r = r + M[i] * w[i]
    R = chol(S)
    c = bsub(R, fsub(R, r))
    y = w.copy()
    for t in range(q):
        y = y - M[:, t] * c[t]
    return bsub(L, y), c


def _one(G, CE, CIcol, m, x, u, gx):
    """One QP: (mode, a, c, ineq) — mode "nan" when q > n; ineq the inequalities of W in order.
    CIcol(j) is column j of CI."""
    n, p = G.shape[0], CE.shape[1]
    eqs, ineq = working_list(u, p)
    if p + len(ineq) > n:
        return "nan", None, None, ineq
    A = np.zeros((n, p + len(ineq)))
    for k in eqs:
        A[:, k] = CE[:, k]
    for t, j in enumerate(ineq):
        A[:, p + t] = CIcol(j)
    a, c = _solve(G, A, gx)
    return "ok", a, c, ineq


def _arrays(pr, x, u, gx):
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    x = np.asarray(x, dtype=np.float64).reshape(B, n)
    gx = np.asarray(gx, dtype=np.float64).reshape(B, n)
    u = np.zeros((B, 0)) if p + m == 0 else np.asarray(u, dtype=np.float64).reshape(B, p + m)
    G = np.asarray(pr.G, dtype=np.float64).reshape(B, n, n)
    CE = np.asarray(pr.CE, dtype=np.float64).reshape(B, n, p)
    return x, u, gx, G, CE


def _common(out, b, a, c, x, u, p):
    out["dg0"][b] = -a
    out["dG"][b] = -0.5 * (a[:, None] * x[None, :] + x[:, None] * a[None, :])
    out["dCE"][b] = a[:, None] * u[None, :p] - x[:, None] * c[None, :p]
    out["dce0"][b] = -c[:p]


def vjp(pr, x, u, gx, status=None) -> dict:
    """The six gradients of the dense entry for `pr` (qpgpu.Problems) at (x, u) and gx: a dict of
    (B, ...) arrays shaped like the inputs.  With `status`, a QP that is not QP_OK is all +0.0."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    x, u, gx, G, CE = _arrays(pr, x, u, gx)
    CI = np.asarray(pr.CI, dtype=np.float64).reshape(B, n, m)
    out = {"dG": np.zeros((B, n, n)), "dg0": np.zeros((B, n)), "dCE": np.zeros((B, n, p)),
           "dce0": np.zeros((B, p)), "dCI": np.zeros((B, n, m)), "dci0": np.zeros((B, m))}
    with np.errstate(all="ignore"):
        for b in range(B):
            if status is not None and status[b] != qpgpu.QP_OK:
                continue
            mode, a, c, ineq = _one(G[b], CE[b], lambda j: CI[b][:, j], m, x[b], u[b], gx[b])
            if mode == "nan":
                for v in out.values():
                    v[b] = np.nan
                continue
            _common(out, b, a, c, x[b], u[b], p)
            for t, j in enumerate(ineq):
                out["dCI"][b][:, j] = a * u[b, p + j] - x[b] * c[p + t]
                out["dci0"][b][j] = -c[p + t]
    return out


def box_column(n, j):
    """Column j of CI = [-I, +I] as BoxProblems.to_dense() materialises it."""
    col = np.full(n, -0.0) if j < n else np.zeros(n)
    col[j if j < n else j - n] = -1.0 if j < n else 1.0
    return col


def vjp_box(bp, x, u, gx, status=None) -> dict:
    """The box entry's six gradients for `bp` (qpgpu.BoxProblems), u = [equalities, upper, lower]."""
    B, n, p = bp.batch, bp.n, bp.p
    x, u, gx, G, CE = _arrays(bp, x, u, gx)
    out = {"dG": np.zeros((B, n, n)), "dg0": np.zeros((B, n)), "dCE": np.zeros((B, n, p)),
           "dce0": np.zeros((B, p)), "dhi": np.zeros((B, n)), "dlo": np.zeros((B, n))}
    with np.errstate(all="ignore"):
        for b in range(B):
            if status is not None and status[b] != qpgpu.QP_OK:
                continue
            mode, a, c, ineq = _one(G[b], CE[b], lambda j: box_column(n, j), 2 * n, x[b], u[b], gx[b])
            if mode == "nan":
                for v in out.values():
                    v[b] = np.nan
                continue
            _common(out, b, a, c, x[b], u[b], p)
            for t, j in enumerate(ineq):
                if j < n:
                    out["dhi"][b][j] = -c[p + t]
                else:
                    out["dlo"][b][j - n] = c[p + t]
    return out


def dense_kkt(pr, x, u, gx) -> dict:
    """The same gradients from one np.linalg.solve of [[G, A], [A^T, 0]] [a; c] = [gx; 0] per QP
    (every QP is evaluated; q > n raises)."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    x, u, gx, G, CE = _arrays(pr, x, u, gx)
    CI = np.asarray(pr.CI, dtype=np.float64).reshape(B, n, m)
    out = {"dG": np.zeros((B, n, n)), "dg0": np.zeros((B, n)), "dCE": np.zeros((B, n, p)),
           "dce0": np.zeros((B, p)), "dCI": np.zeros((B, n, m)), "dci0": np.zeros((B, m))}
    for b in range(B):
        _, ineq = working_list(u[b], p)
        A = np.concatenate([CE[b], CI[b][:, ineq]], axis=1)
        q = A.shape[1]
        assert q <= n
        Gs = np.tril(G[b]) + np.tril(G[b], -1).T  # the symmetric G the definition reads
        K = np.block([[Gs, A], [A.T, np.zeros((q, q))]])
        sol = np.linalg.solve(K, np.concatenate([gx[b], np.zeros(q)]))
        a, c = sol[:n], sol[n:]
        lam = np.concatenate([u[b, :p], u[b, p:][ineq]])
        dA = np.outer(a, lam) - np.outer(x[b], c)
        out["dg0"][b] = -a
        out["dG"][b] = -0.5 * (np.outer(a, x[b]) + np.outer(x[b], a))
        out["dCE"][b] = dA[:, :p]
        out["dce0"][b] = -c[:p]
        out["dCI"][b][:, ineq] = dA[:, p:]
        out["dci0"][b][ineq] = -c[p:]
    return out


def make_gx(pr, seed=0):
    """dl/dx of the GPU tests: standard normals from a fixed seed, (B, n)."""
    return np.random.default_rng([pr.n, pr.p, pr.m, pr.batch, seed]).standard_normal((pr.batch, pr.n))


def same_bits(a, b) -> bool:
    """Equal bit for bit (so -0.0 differs from +0.0), NaN equal to NaN whatever its payload."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def mismatches(got: dict, want: dict, show=4) -> list:
    """(output, index, got, want) hex of the first elements that are not the same bits."""
    bad = []
    for k, w in want.items():
        g = np.ascontiguousarray(got[k], dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if g.shape != w.shape:
            bad.append((k, "shape", g.shape, w.shape))
            continue
        diff = (g.view(np.uint64) != w.view(np.uint64)) & ~(np.isnan(g) & np.isnan(w))
        for idx in list(zip(*np.nonzero(diff)))[:show]:
            bad.append((k, tuple(int(i) for i in idx), float(g[idx]).hex(), float(w[idx]).hex()))
    return bad
