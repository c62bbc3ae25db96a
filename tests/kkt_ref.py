"""The definition of qpgpu_kkt_residuals in numpy (TEST INFRASTRUCTURE ONLY).

include/qpgpu.h fixes every operation: each sum starts from +0.0 and adds in ascending index,
every product is rounded before it is added, ratio(a, b) = b > 0 ? a / b : a, and every running
maximum is smax from +0.0, which keeps a NaN.  The loops below run over the summation index and
are vectorised over the batch and over the index the sum does not run over (each (QP, row) or
(QP, column) is an independent sum, so that changes no operation): `a = a + G[:, :, j] * x[:, j]`
adds the rounded product of column j to every row's running sum.

residuals_box() restates the box entry's own forms (the one or two non-zero terms of each sum over
a row or column of CI = [-I, +I]); tests/test_kkt_cpu.py holds it to residuals() on to_dense().
"""
from __future__ import annotations

import numpy as np

import qpgpu

NRES = 8
STAT, STAT_SCALE, EQ, INEQ, COMP, UMIN, OBJ, NNZ = range(NRES)


def ratio(a, b):
    with np.errstate(all="ignore"):
        return np.where(b > 0, a / np.where(b > 0, b, 1.0), a)


def smax(acc, v):
    return np.where(np.isnan(acc), acc, np.where((v > acc) | np.isnan(v), v, acc))


def _row_sums(M, v):
    """For M (B, n, c) and v (B, c): s[b, i] = sum_k M[b, i, k] v[b, k] and the same of magnitudes."""
    B, n, c = M.shape
    s, sa = np.zeros((B, n)), np.zeros((B, n))
    Ma, va = np.abs(M), np.abs(v)
    for k in range(c):
        s = s + M[:, :, k] * v[:, k, None]
        sa = sa + Ma[:, :, k] * va[:, k, None]
    return s, sa


def _col_sums(M, x):
    """For M (B, n, c) and x (B, n): s[b, k] = sum_i M[b, i, k] x[b, i] and the same of magnitudes."""
    B, n, c = M.shape
    s, sa = np.zeros((B, c)), np.zeros((B, c))
    Ma, xa = np.abs(M), np.abs(x)
    for i in range(n):
        s = s + M[:, i, :] * x[:, i, None]
        sa = sa + Ma[:, i, :] * xa[:, i, None]
    return s, sa


def _smax_over(v):
    acc = np.zeros(v.shape[0])
    for k in range(v.shape[1]):
        acc = smax(acc, v[:, k])
    return acc


def _finish(pr, x, ue, ui, d, da, s, sa, status):
    """The slots from the inequality sums (d, da per row; s, sa per inequality) and everything
    the dense and the box form share."""
    B, n, p = pr.batch, pr.n, pr.p
    g0 = np.asarray(pr.g0, dtype=np.float64).reshape(B, n)
    with np.errstate(all="ignore"):
        a, aa = _row_sums(np.asarray(pr.G, dtype=np.float64).reshape(B, n, n), x)
        CE = np.asarray(pr.CE, dtype=np.float64).reshape(B, n, p)
        ce0 = np.asarray(pr.ce0, dtype=np.float64).reshape(B, p)
        c, ca = _row_sums(CE, ue)
        t = ((a + g0) - c) - d
        ts = ((aa + np.abs(g0)) + ca) + da
        stat, scale = _smax_over(np.abs(t)), _smax_over(ts)
        q, l = np.zeros(B), np.zeros(B)
        for i in range(n):
            q = q + x[:, i] * a[:, i]
            l = l + g0[:, i] * x[:, i]
        e, ea = _col_sums(CE, x)
        e, ea = e + ce0, ea + np.abs(ce0)
        r = np.zeros((B, NRES))
        r[:, STAT] = ratio(stat, scale)
        r[:, STAT_SCALE] = scale
        r[:, EQ] = _smax_over(ratio(np.abs(e), ea))
        viol = np.where(s < 0, ratio(-s, sa), np.where(np.isnan(s), np.nan, 0.0))
        r[:, INEQ] = _smax_over(viol)
        comp, umin, nnz = np.zeros(B), np.zeros(B), np.zeros(B)
        cterm = ratio(np.abs(s), sa)
        for k in range(ui.shape[1]):
            on = ui[:, k] != 0
            comp = np.where(on, smax(comp, cterm[:, k]), comp)
            umin = np.where(ui[:, k] < umin, ui[:, k], umin)
            nnz = nnz + on
        r[:, COMP], r[:, UMIN], r[:, NNZ] = comp, umin, nnz
        r[:, OBJ] = 0.5 * q + l
    if status is not None:
        r[np.asarray(status) != qpgpu.QP_OK] = np.nan
    return r


def _pair(pr, x, u):
    B, E = pr.batch, pr.p + pr.m
    x = np.asarray(x, dtype=np.float64).reshape(B, pr.n)
    u = np.zeros((B, 0)) if E == 0 else np.asarray(u, dtype=np.float64).reshape(B, E)
    return x, u[:, :pr.p], u[:, pr.p:]


def residuals(pr, x, u, status=None) -> np.ndarray:
    """(B, 8): the slots of include/qpgpu.h for the dense problem `pr` (qpgpu.Problems) at (x, u);
    with `status`, an all-NaN row for every QP that is not QP_OK."""
    x, ue, ui = _pair(pr, x, u)
    B, n, m = pr.batch, pr.n, pr.m
    CI = np.asarray(pr.CI, dtype=np.float64).reshape(B, n, m)
    ci0 = np.asarray(pr.ci0, dtype=np.float64).reshape(B, m)
    with np.errstate(all="ignore"):
        d, da = _row_sums(CI, ui)
        s, sa = _col_sums(CI, x)
        s, sa = s + ci0, sa + np.abs(ci0)
    return _finish(pr, x, ue, ui, d, da, s, sa, status)


def residuals_box(bp, x, u, status=None) -> np.ndarray:
    """The box entry's forms for `bp` (qpgpu.BoxProblems), u = [equalities, upper, lower]."""
    x, ue, ui = _pair(bp, x, u)
    n = bp.n
    hi = np.asarray(bp.hi, dtype=np.float64).reshape(-1, n)
    nlo = -np.asarray(bp.lo, dtype=np.float64).reshape(-1, n)
    uu, ul = ui[:, :n], ui[:, n:]
    with np.errstate(all="ignore"):
        d = (0.0 - uu) + ul
        da = (0.0 + np.abs(uu)) + np.abs(ul)
        s = np.concatenate([(0.0 - x) + hi, (0.0 + x) + nlo], axis=1)
        sa = np.concatenate([(0.0 + np.abs(x)) + np.abs(hi), (0.0 + np.abs(x)) + np.abs(nlo)], axis=1)
    return _finish(bp, x, ue, ui, d, da, s, sa, status)


def same_bits(a, b) -> bool:
    """Equal bit for bit, NaN equal to NaN whatever its payload (test_dual_cpu._same_bits)."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def mismatches(a, b, show=6) -> list:
    """(index, got, want) hex of the first elements that are not the same bits."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel()
    assert a.shape == b.shape, (a.shape, b.shape)
    diff = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))
    return [(int(i) // NRES, int(i) % NRES, float(a[i]).hex(), float(b[i]).hex()) for i in np.where(diff)[0][:show]]
