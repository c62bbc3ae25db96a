"""CPU reference for qpgpu_solve_batched_box_dual (TEST INFRASTRUCTURE ONLY).

The entry is defined as qpgpu_solve_batched_dual on the materialised problem, so the reference of
every case of tests/box_ref.py is tests/dual_ref.py's restatement (the oracle with an export hook
at `done:`) on BoxProblems.to_dense(), under the C-ABI's default step cap.  Nothing new is built.
"""
from __future__ import annotations

import functools

import box_ref
import dual_ref

# ids whose data is adversarial on purpose (infeasible, tied, dependent, indefinite or scaled so
# that the rollback quirk of DESIGN §3.5 is taken): the KKT identities are asserted on the rest
ILL_POSED_PREFIXES = ("crossed", "ints", "dupce", "indef", "scaled_ce")


def well_posed_cases() -> list:
    return [cid for cid in box_ref.cases() if not cid.startswith(ILL_POSED_PREFIXES)]


@functools.lru_cache(maxsize=None)
def reference(cid: str, max_steps: int = 0):
    """(x, f, status, iters, u, nact) of a box_ref case, u of shape (B, p + 2n): equalities, upper
    bounds, lower bounds.  Computed once; the arrays are shared between tests and read-only."""
    bp = box_ref.case(cid)
    res = dual_ref.solve(box_ref.dense(cid), max_steps or box_ref.default_cap(bp.n, bp.p))
    for a in res:
        a.setflags(write=False)
    return res
