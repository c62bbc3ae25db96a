"""The definition of qpgpu_vjp_full / qpgpu_vjp_box_full in numpy (TEST INFRASTRUCTURE ONLY).

tests/vjp_ref.py restated for the three cotangents gx, gu, gf of a loss l(x, u, f), with
include/qpgpu.h's two additions and nothing else: gl(t) joins r once, after its sum, and gf turns a
into ah (in dG), adds g * x to dg0 and turns c into ct (in every constraint gradient) while
y = w - M c keeps c.  A cotangent that is None adds no operation, so gu = gf = None is vjp_ref
bit for bit.  chol / fsub / bsub / working_list are vjp_ref's: every sum runs in the definition's
order on np.float64, products rounded before they are added, no `@`, no BLAS.

dense_kkt() is the independent check: np.linalg.solve on [[G, A], [A^T, 0]] [a; c] = [gx; -gl],
then the envelope terms of f added in plain float64.
"""
from __future__ import annotations

import numpy as np

import qpgpu
from vjp_ref import box_column, bsub, chol, fsub, working_list, _arrays

DENSE_OUTPUTS = ("dG", "dg0", "dCE", "dce0", "dCI", "dci0")
BOX_OUTPUTS = ("dG", "dg0", "dCE", "dce0", "dhi", "dlo")


def _solve(G, A, gx, gl):
    """(a, c) of the definition for the n x q working columns A; gl (q,) or None."""
    n, q = A.shape
    L = chol(G)
    w = fsub(L, gx)
    M = fsub(L, A)
    S = np.zeros((q, q))
    r = np.zeros(q)
    for i in range(n):
        S = S + M[i][:, None] * M[i][None, :]
        r = r + M[i] * w[i]
    if gl is not None:
        r = r + gl
    R = chol(S)
    c = bsub(R, fsub(R, r))
    y = w.copy()
    for t in range(q):
        y = y - M[:, t] * c[t]
    return bsub(L, y), c


def _one(G, CE, CIcol, x, u, gx, gu, gf):
    """One QP: None when q > n, else (a, ah, d0, ct, lam, ineq): a, the a that dG reads, dg0, the c
    the constraint gradients read, the multipliers of W and its inequalities in order."""
    n, p = G.shape[0], CE.shape[1]
    eqs, ineq = working_list(u, p)
    q = p + len(ineq)
    if q > n:
        return None
    A = np.zeros((n, q))
    for k in eqs:
        A[:, k] = CE[:, k]
    for t, j in enumerate(ineq):
        A[:, p + t] = CIcol(j)
    pos = eqs + [p + j for j in ineq]  # the u (and gu) entry of position t
    lam = u[pos] if q else np.zeros(0)
    gl = None if gu is None else (gu[pos] if q else np.zeros(0))
    a, c = _solve(G, A, gx, gl)
    if gf is None:
        return a, a, -a, c, lam, ineq
    g = np.float64(gf)
    hh = 0.5 * g
    ah = a - hh * x
    d0 = -(a - g * x)
    ct = c + g * lam
    return a, ah, d0, ct, lam, ineq


def _cot(B, E, gu, gf):
    gu = None if gu is None else np.asarray(gu, dtype=np.float64).reshape(B, E)
    gf = None if gf is None else np.asarray(gf, dtype=np.float64).reshape(B)
    return gu, gf


def _common(out, b, a, ah, d0, ct, x, u, p):
    out["dg0"][b] = d0
    out["dG"][b] = -0.5 * (ah[:, None] * x[None, :] + x[:, None] * ah[None, :])
    out["dCE"][b] = a[:, None] * u[None, :p] - x[:, None] * ct[None, :p]
    out["dce0"][b] = -ct[:p]


def vjp_full(pr, x, u, gx, gu=None, gf=None, status=None) -> dict:
    """The six gradients of the dense entry for `pr` (qpgpu.Problems) at (x, u) and the cotangents
    gx (B, n), gu (B, p + m) or None, gf (B,) or None.  With `status`, a QP that is not QP_OK is all
    +0.0; q > n is all NaN."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    x, u, gx, G, CE = _arrays(pr, x, u, gx)
    gu, gf = _cot(B, p + m, gu, gf)
    CI = np.asarray(pr.CI, dtype=np.float64).reshape(B, n, m)
    out = {"dG": np.zeros((B, n, n)), "dg0": np.zeros((B, n)), "dCE": np.zeros((B, n, p)),
           "dce0": np.zeros((B, p)), "dCI": np.zeros((B, n, m)), "dci0": np.zeros((B, m))}
    with np.errstate(all="ignore"):
        for b in range(B):
            if status is not None and status[b] != qpgpu.QP_OK:
                continue
            one = _one(G[b], CE[b], lambda j: CI[b][:, j], x[b], u[b], gx[b],
                       None if gu is None else gu[b], None if gf is None else gf[b])
            if one is None:
                for v in out.values():
                    v[b] = np.nan
                continue
            a, ah, d0, ct, lam, ineq = one
            _common(out, b, a, ah, d0, ct, x[b], u[b], p)
            for t, j in enumerate(ineq):
                out["dCI"][b][:, j] = a * u[b, p + j] - x[b] * ct[p + t]
                out["dci0"][b][j] = -ct[p + t]
    return out


def vjp_box_full(bp, x, u, gx, gu=None, gf=None, status=None) -> dict:
    """The box entry's six gradients for `bp` (qpgpu.BoxProblems); u and gu = [equalities, upper,
    lower]."""
    B, n, p = bp.batch, bp.n, bp.p
    x, u, gx, G, CE = _arrays(bp, x, u, gx)
    gu, gf = _cot(B, p + 2 * n, gu, gf)
    out = {"dG": np.zeros((B, n, n)), "dg0": np.zeros((B, n)), "dCE": np.zeros((B, n, p)),
           "dce0": np.zeros((B, p)), "dhi": np.zeros((B, n)), "dlo": np.zeros((B, n))}
    with np.errstate(all="ignore"):
        for b in range(B):
            if status is not None and status[b] != qpgpu.QP_OK:
                continue
            one = _one(G[b], CE[b], lambda j: box_column(n, j), x[b], u[b], gx[b],
                       None if gu is None else gu[b], None if gf is None else gf[b])
            if one is None:
                for v in out.values():
                    v[b] = np.nan
                continue
            a, ah, d0, ct, lam, ineq = one
            _common(out, b, a, ah, d0, ct, x[b], u[b], p)
            for t, j in enumerate(ineq):
                if j < n:
                    out["dhi"][b][j] = -ct[p + t]
                else:
                    out["dlo"][b][j - n] = ct[p + t]
    return out


def dense_kkt(pr, x, u, gx, gu=None, gf=None) -> dict:
    """The same gradients from one np.linalg.solve of [[G, A], [A^T, 0]] [a; c] = [gx; -gl] per QP,
    plus gf times the envelope derivatives of f (every QP is evaluated; q > n raises)."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    x, u, gx, G, CE = _arrays(pr, x, u, gx)
    gu, gf = _cot(B, p + m, gu, gf)
    CI = np.asarray(pr.CI, dtype=np.float64).reshape(B, n, m)
    out = {"dG": np.zeros((B, n, n)), "dg0": np.zeros((B, n)), "dCE": np.zeros((B, n, p)),
           "dce0": np.zeros((B, p)), "dCI": np.zeros((B, n, m)), "dci0": np.zeros((B, m))}
    for b in range(B):
        _, ineq = working_list(u[b], p)
        A = np.concatenate([CE[b], CI[b][:, ineq]], axis=1)
        q = A.shape[1]
        assert q <= n
        pos = list(range(p)) + [p + j for j in ineq]
        gl = np.zeros(q) if gu is None else gu[b][pos]
        Gs = np.tril(G[b]) + np.tril(G[b], -1).T  # the symmetric G the definition reads
        K = np.block([[Gs, A], [A.T, np.zeros((q, q))]])
        sol = np.linalg.solve(K, np.concatenate([gx[b], -gl]))
        a, c = sol[:n], sol[n:]
        lam = u[b][pos]
        g = 0.0 if gf is None else gf[b]
        # l = ... + g f:  df/dg0 = x, df/dG = x x^T / 2, df/dA = -x lam^T, df/db = -lam
        dA = np.outer(a, lam) - np.outer(x[b], c) - g * np.outer(x[b], lam)
        db = -c - g * lam
        out["dg0"][b] = -a + g * x[b]
        out["dG"][b] = -0.5 * (np.outer(a, x[b]) + np.outer(x[b], a)) + 0.5 * g * np.outer(x[b], x[b])
        out["dCE"][b] = dA[:, :p]
        out["dce0"][b] = db[:p]
        out["dCI"][b][:, ineq] = dA[:, p:]
        out["dci0"][b][ineq] = db[p:]
    return out


def make_cotangents(pr, seed=0):
    """(gu, gf) of the GPU tests: standard normals from a fixed seed, (B, p + m) and (B,)."""
    rng = np.random.default_rng([pr.n, pr.p, pr.m, pr.batch, seed, 77])
    return rng.standard_normal((pr.batch, pr.p + pr.m)), rng.standard_normal(pr.batch)
