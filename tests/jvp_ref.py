"""The definition of qpgpu_jvp / qpgpu_jvp_box in numpy (TEST INFRASTRUCTURE ONLY).

include/qpgpu.h fixes every operation: no FMA, every product rounded before it is added or
subtracted, IEEE division and sqrt, no branch on any pivot, every sum from +0.0 and ascending.  chol,
fsub, bsub and working_list are tests/vjp_ref.py's; the loops here run over the index a sum is serial
in and are vectorised over the index it is independent in, so each element sees exactly the
definition's operations in the definition's order on np.float64; nothing uses `@` or a BLAS call.

A tangent that is None is the entry's NULL: a zero tangent whose steps are not executed.
jvp_box() restates the box entry's own form (generated columns, no tangent of a bound's column,
tb = thi[k] / -tlo[k]); dense_kkt() is the independent check: one np.linalg.solve of
[[G, -A], [A^T, 0]] [tx; tl] = [h; k] per QP.
"""
from __future__ import annotations

import numpy as np

import qpgpu
from vjp_ref import box_column, bsub, chol, fsub, working_list

DENSE_TANGENTS = ("G", "g0", "CE", "ce0", "CI", "ci0")
BOX_TANGENTS = ("G", "g0", "CE", "ce0", "hi", "lo")
OUTPUTS = ("tx", "tu", "tf")


def _arrays(pr, x, u):
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    x = np.asarray(x, dtype=np.float64).reshape(B, n)
    u = np.zeros((B, 0)) if p + m == 0 else np.asarray(u, dtype=np.float64).reshape(B, p + m)
    G = np.asarray(pr.G, dtype=np.float64).reshape(B, n, n)
    CE = np.asarray(pr.CE, dtype=np.float64).reshape(B, n, p)
    return x, u, G, CE


def _tangent(tangents, name, shape):
    t = tangents.get(name)
    return None if t is None else np.asarray(t, dtype=np.float64).reshape(shape)


def _one(G, A, x, lam, tG, tg0, tcols, tbs):
    """One QP with q <= n: (tx, dl, tf).  A (n, q): the working columns; tcols[t]: the tangent of
    column t or None; tbs[t]: the tangent of its offset or None."""
    n, q = A.shape
    sG = np.zeros(n)
    if tG is not None:
        for j in range(n):
            sG = sG + tG[:, j] * x[j]
    h = np.zeros(n)
    for t in range(q):
        if tcols[t] is not None:
            h = h + tcols[t] * lam[t]
    if tG is not None:
        h = h - sG
    if tg0 is not None:
        h = h - tg0
    k = np.zeros(q)
    for t in range(q):
        s = np.float64(0.0)
        if tcols[t] is not None:
            for i in range(n):
                s = s + tcols[t][i] * x[i]
        if tbs[t] is not None:
            s = s + tbs[t]
        k[t] = -s
    L = chol(G)
    w = fsub(L, h)
    M = fsub(L, A)
    S = np.zeros((q, q))
    rs = np.zeros(q)
    for i in range(n):
        S = S + M[i][:, None] * M[i][None, :]
        rs = rs + M[i] * w[i]
    r = k - rs
    R = chol(S)
    dl = bsub(R, fsub(R, r))
    y = w.copy()
    for t in range(q):
        y = y + M[:, t] * dl[t]
    tx = bsub(L, y)
    qq = np.float64(0.0)
    ll = np.float64(0.0)
    kk = np.float64(0.0)
    for i in range(n):
        qq = qq + x[i] * sG[i]
    if tg0 is not None:
        for i in range(n):
            ll = ll + tg0[i] * x[i]
    for t in range(q):
        kk = kk + lam[t] * k[t]
    return tx, dl, ((0.5 * qq) + ll) + kk


def _run(pr, x, u, status, tG, tg0, columns):
    """columns(b, ineq) -> (A, tcols, tbs) of QP b for the inequalities `ineq` of W."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    out = {"tx": np.zeros((B, n)), "tu": np.zeros((B, p + m)), "tf": np.zeros(B)}
    xs, us, G, CE = _arrays(pr, x, u)
    with np.errstate(all="ignore"):
        for b in range(B):
            if status is not None and status[b] != qpgpu.QP_OK:
                continue
            eqs, ineq = working_list(us[b], p)
            if p + len(ineq) > n:
                for v in out.values():
                    v[b] = np.nan
                continue
            A, tcols, tbs = columns(b, ineq)
            pos = eqs + [p + j for j in ineq]
            lam = us[b][pos] if pos else np.zeros(0)
            tx, dl, tf = _one(G[b], A, xs[b], lam, None if tG is None else tG[b], None if tg0 is None else tg0[b],
                              tcols, tbs)
            out["tx"][b] = tx
            out["tf"][b] = tf
            for t, e in enumerate(pos):
                out["tu"][b, e] = dl[t]
    return out


def jvp(pr, x, u, tangents, status=None) -> dict:
    """tx (B, n), tu (B, p + m), tf (B,) of the dense entry for `pr` (qpgpu.Problems) at (x, u);
    tangents: a dict from G, g0, CE, ce0, CI, ci0 to an array shaped like that input (missing or None:
    NULL).  With `status`, a QP that is not QP_OK is all +0.0; q > n is all NaN."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    assert set(tangents) <= set(DENSE_TANGENTS), tangents.keys()
    _, _, _, CE = _arrays(pr, x, u)
    CI = np.asarray(pr.CI, dtype=np.float64).reshape(B, n, m)
    tG, tg0 = _tangent(tangents, "G", (B, n, n)), _tangent(tangents, "g0", (B, n))
    tCE, tce0 = _tangent(tangents, "CE", (B, n, p)), _tangent(tangents, "ce0", (B, p))
    tCI, tci0 = _tangent(tangents, "CI", (B, n, m)), _tangent(tangents, "ci0", (B, m))

    def columns(b, ineq):
        A = np.zeros((n, p + len(ineq)))
        tcols, tbs = [], []
        for k in range(p):
            A[:, k] = CE[b][:, k]
            tcols.append(None if tCE is None else tCE[b][:, k])
            tbs.append(None if tce0 is None else tce0[b, k])
        for t, j in enumerate(ineq):
            A[:, p + t] = CI[b][:, j]
            tcols.append(None if tCI is None else tCI[b][:, j])
            tbs.append(None if tci0 is None else tci0[b, j])
        return A, tcols, tbs

    return _run(pr, x, u, status, tG, tg0, columns)


def jvp_box(bp, x, u, tangents, status=None) -> dict:
    """The box entry for `bp` (qpgpu.BoxProblems), u = [equalities, upper, lower]; tangents: a dict
    from G, g0, CE, ce0, hi, lo.  tu is (B, p + 2n)."""
    B, n, p = bp.batch, bp.n, bp.p
    assert set(tangents) <= set(BOX_TANGENTS), tangents.keys()
    _, _, _, CE = _arrays(bp, x, u)
    tG, tg0 = _tangent(tangents, "G", (B, n, n)), _tangent(tangents, "g0", (B, n))
    tCE, tce0 = _tangent(tangents, "CE", (B, n, p)), _tangent(tangents, "ce0", (B, p))
    thi, tlo = _tangent(tangents, "hi", (B, n)), _tangent(tangents, "lo", (B, n))

    def columns(b, ineq):
        A = np.zeros((n, p + len(ineq)))
        tcols, tbs = [], []
        for k in range(p):
            A[:, k] = CE[b][:, k]
            tcols.append(None if tCE is None else tCE[b][:, k])
            tbs.append(None if tce0 is None else tce0[b, k])
        for t, j in enumerate(ineq):
            A[:, p + t] = box_column(n, j)
            tcols.append(None)
            if j < n:
                tbs.append(None if thi is None else thi[b, j])
            else:
                tbs.append(None if tlo is None else -tlo[b, j - n])
        return A, tcols, tbs

    return _run(bp, x, u, status, tG, tg0, columns)


def box_tangents_as_dense(bp, tangents) -> dict:
    """The dense entry's tangents the box entry is defined by: tCI = NULL, tci0 = [thi; -tlo]."""
    B, n = bp.batch, bp.n
    out = {k: tangents[k] for k in ("G", "g0", "CE", "ce0") if tangents.get(k) is not None}
    thi, tlo = tangents.get("hi"), tangents.get("lo")
    if thi is not None or tlo is not None:
        thi = np.zeros((B, n)) if thi is None else np.asarray(thi, dtype=np.float64).reshape(B, n)
        tlo = np.zeros((B, n)) if tlo is None else np.asarray(tlo, dtype=np.float64).reshape(B, n)
        out["ci0"] = np.concatenate([thi, -tlo], axis=1)
    return out


def dense_kkt(pr, x, u, tangents) -> dict:
    """The same three outputs from one np.linalg.solve of [[G, -A], [A^T, 0]] [tx; tl] = [h; k] per QP,
    h, k and tf in plain float64 (every QP is evaluated; q > n raises)."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    x, u, G, CE = _arrays(pr, x, u)
    CI = np.asarray(pr.CI, dtype=np.float64).reshape(B, n, m)
    zero = lambda name, shape: np.zeros(shape) if tangents.get(name) is None else _tangent(tangents, name, shape)
    tG, tg0 = zero("G", (B, n, n)), zero("g0", (B, n))
    tCE, tce0 = zero("CE", (B, n, p)), zero("ce0", (B, p))
    tCI, tci0 = zero("CI", (B, n, m)), zero("ci0", (B, m))
    out = {"tx": np.zeros((B, n)), "tu": np.zeros((B, p + m)), "tf": np.zeros(B)}
    for b in range(B):
        _, ineq = working_list(u[b], p)
        A = np.concatenate([CE[b], CI[b][:, ineq]], axis=1)
        tA = np.concatenate([tCE[b], tCI[b][:, ineq]], axis=1)
        tb = np.concatenate([tce0[b], tci0[b][ineq]])
        q = A.shape[1]
        assert q <= n
        pos = list(range(p)) + [p + j for j in ineq]
        lam = u[b][pos]
        h = tA @ lam - tG[b] @ x[b] - tg0[b]
        k = -(tA.T @ x[b] + tb)
        Gs = np.tril(G[b]) + np.tril(G[b], -1).T  # the symmetric G the definition reads
        K = np.block([[Gs, -A], [A.T, np.zeros((q, q))]])
        sol = np.linalg.solve(K, np.concatenate([h, k]))
        out["tx"][b] = sol[:n]
        out["tu"][b, pos] = sol[n:]
        out["tf"][b] = 0.5 * x[b] @ tG[b] @ x[b] + tg0[b] @ x[b] + lam @ k
    return out


def make_tangents(pr, seed=0) -> dict:
    """The tangents of the tests: standard normals from a fixed seed, one per input of `pr`
    (qpgpu.Problems: G, g0, CE, ce0, CI, ci0; qpgpu.BoxProblems: G, g0, CE, ce0, hi, lo), tG
    symmetrised."""
    names = BOX_TANGENTS if isinstance(pr, qpgpu.BoxProblems) else DENSE_TANGENTS
    rng = np.random.default_rng([pr.n, pr.p, pr.m, pr.batch, seed, 1311])
    out = {k: rng.standard_normal(np.asarray(a).shape) for k, a in zip(names, pr.arrays())}
    out["G"] = 0.5 * (out["G"] + np.swapaxes(out["G"], 1, 2))
    return out
