"""The definition of qpgpu_jvp_many / qpgpu_jvp_box_many in numpy (TEST INFRASTRUCTURE ONLY).

Direction k of the entry is qpgpu_jvp's definition (tests/jvp_ref.py) on the k-th slice of every given
tangent.  This restatement factors once per QP, as the kernels do: L = chol(G), M = fsub(L, A), S, R =
chol(S) with chol, fsub, bsub and working_list of tests/vjp_ref.py, then runs the K right-hand sides
against the shared L, M and R.  The K directions are the trailing axis of every array here: a loop runs
over the index a sum is serial in and is vectorised over the directions, so each direction's elements
see exactly the definition's operations in the definition's order on np.float64 (nothing uses `@`).
tests/test_jvp_many_cpu.py checks that sharing the factorisation changes no bit against jvp_ref.

Tangents are shaped (B, K, ...): a (B, K, n, n) array is the QP-major tG.  A tangent that is None is the
entry's NULL: a zero tangent in all K directions whose steps are not executed.
"""
from __future__ import annotations

import numpy as np

import jvp_ref
import qpgpu
from vjp_ref import box_column, bsub, chol, fsub, working_list


def _tangent(tangents, name, shape):
    t = tangents.get(name)
    return None if t is None else np.asarray(t, dtype=np.float64).reshape(shape)


def _factor(G, A):
    """What the K directions share: L, M and R of one QP with working columns A (n, q)."""
    n, q = A.shape
    L = chol(G)
    M = fsub(L, A)
    S = np.zeros((q, q))
    for i in range(n):
        S = S + M[i][:, None] * M[i][None, :]
    return L, M, chol(S)


def _directions(L, M, R, x, lam, tG, tg0, tcols, tbs, K):
    """(tx (K, n), dl (K, q), tf (K,)) of one QP.  tG (K, n, n) or None, tg0 (K, n) or None; tcols[t]:
    (K, n), the K tangents of working column t, or None; tbs[t]: (K,) or None."""
    n, q = M.shape
    sG = np.zeros((n, K))
    if tG is not None:
        for j in range(n):
            sG = sG + tG[:, :, j].T * x[j]
    h = np.zeros((n, K))
    for t in range(q):
        if tcols[t] is not None:
            h = h + tcols[t].T * lam[t]
    if tG is not None:
        h = h - sG
    if tg0 is not None:
        h = h - tg0.T
    k = np.zeros((q, K))
    for t in range(q):
        s = np.zeros(K)
        if tcols[t] is not None:
            for i in range(n):
                s = s + tcols[t][:, i] * x[i]
        if tbs[t] is not None:
            s = s + tbs[t]
        k[t] = -s
    w = fsub(L, h)
    rs = np.zeros((q, K))
    for i in range(n):
        rs = rs + M[i][:, None] * w[i][None, :]
    r = k - rs
    dl = bsub(R, fsub(R, r))
    y = w.copy()
    for t in range(q):
        y = y + M[:, t][:, None] * dl[t][None, :]
    tx = bsub(L, y)
    qq = np.zeros(K)
    ll = np.zeros(K)
    kk = np.zeros(K)
    for i in range(n):
        qq = qq + x[i] * sG[i]
    if tg0 is not None:
        for i in range(n):
            ll = ll + tg0[:, i] * x[i]
    for t in range(q):
        kk = kk + lam[t] * k[t]
    return tx.T, dl.T, ((0.5 * qq) + ll) + kk


def _run(pr, x, u, status, K, tG, tg0, columns):
    """columns(b, ineq) -> (A, tcols, tbs) of QP b for the inequalities `ineq` of W."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    out = {"tx": np.zeros((B, K, n)), "tu": np.zeros((B, K, p + m)), "tf": np.zeros((B, K))}
    xs, us, G, _ = jvp_ref._arrays(pr, x, u)
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
            L, M, R = _factor(G[b], A)
            tx, dl, tf = _directions(L, M, R, xs[b], lam, None if tG is None else tG[b],
                                     None if tg0 is None else tg0[b], tcols, tbs, K)
            out["tx"][b] = tx
            out["tf"][b] = tf
            for t, e in enumerate(pos):
                out["tu"][b, :, e] = dl[:, t]
    return out


def jvp_many(pr, x, u, tangents, K, status=None) -> dict:
    """tx (B, K, n), tu (B, K, p + m), tf (B, K) of the dense entry for `pr` (qpgpu.Problems) at (x, u);
    tangents: a dict from G, g0, CE, ce0, CI, ci0 to an array (B, K, ...) (missing or None: NULL).  With
    `status`, a QP that is not QP_OK is all +0.0; q > n is all NaN."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    assert set(tangents) <= set(jvp_ref.DENSE_TANGENTS), tangents.keys()
    _, _, _, CE = jvp_ref._arrays(pr, x, u)
    CI = np.asarray(pr.CI, dtype=np.float64).reshape(B, n, m)
    tG, tg0 = _tangent(tangents, "G", (B, K, n, n)), _tangent(tangents, "g0", (B, K, n))
    tCE, tce0 = _tangent(tangents, "CE", (B, K, n, p)), _tangent(tangents, "ce0", (B, K, p))
    tCI, tci0 = _tangent(tangents, "CI", (B, K, n, m)), _tangent(tangents, "ci0", (B, K, m))

    def columns(b, ineq):
        A = np.zeros((n, p + len(ineq)))
        tcols, tbs = [], []
        for k in range(p):
            A[:, k] = CE[b][:, k]
            tcols.append(None if tCE is None else tCE[b][:, :, k])
            tbs.append(None if tce0 is None else tce0[b, :, k])
        for t, j in enumerate(ineq):
            A[:, p + t] = CI[b][:, j]
            tcols.append(None if tCI is None else tCI[b][:, :, j])
            tbs.append(None if tci0 is None else tci0[b, :, j])
        return A, tcols, tbs

    return _run(pr, x, u, status, K, tG, tg0, columns)


def jvp_box_many(bp, x, u, tangents, K, status=None) -> dict:
    """The box entry for `bp` (qpgpu.BoxProblems), u = [equalities, upper, lower]; tangents: a dict
    from G, g0, CE, ce0, hi, lo to an array (B, K, ...).  tu is (B, K, p + 2n)."""
    B, n, p = bp.batch, bp.n, bp.p
    assert set(tangents) <= set(jvp_ref.BOX_TANGENTS), tangents.keys()
    _, _, _, CE = jvp_ref._arrays(bp, x, u)
    tG, tg0 = _tangent(tangents, "G", (B, K, n, n)), _tangent(tangents, "g0", (B, K, n))
    tCE, tce0 = _tangent(tangents, "CE", (B, K, n, p)), _tangent(tangents, "ce0", (B, K, p))
    thi, tlo = _tangent(tangents, "hi", (B, K, n)), _tangent(tangents, "lo", (B, K, n))

    def columns(b, ineq):
        A = np.zeros((n, p + len(ineq)))
        tcols, tbs = [], []
        for k in range(p):
            A[:, k] = CE[b][:, k]
            tcols.append(None if tCE is None else tCE[b][:, :, k])
            tbs.append(None if tce0 is None else tce0[b, :, k])
        for t, j in enumerate(ineq):
            A[:, p + t] = box_column(n, j)
            tcols.append(None)
            if j < n:
                tbs.append(None if thi is None else thi[b, :, j])
            else:
                tbs.append(None if tlo is None else -tlo[b, :, j - n])
        return A, tcols, tbs

    return _run(bp, x, u, status, K, tG, tg0, columns)


def make_many_tangents(pr, K) -> dict:
    """K directions per input of `pr`, each (B, K, ...): direction k is jvp_ref.make_tangents(pr, seed=k)."""
    per = [jvp_ref.make_tangents(pr, seed=k) for k in range(K)]
    return {name: np.stack([t[name] for t in per], axis=1) for name in per[0]}


def slice_tangents(tangents, k) -> dict:
    """Direction k of (B, K, ...) tangents, as jvp_ref takes them (None stays None)."""
    return {name: None if t is None else np.ascontiguousarray(np.asarray(t)[:, k]) for name, t in tangents.items()}
