"""The device-resident control cycle with MGQP_SOLVER_UNIT_HESSIAN (update_device(..., unit=True)):
every level solved by qpgpu_solve_batched_unit instead of qpgpu_solve_batched_eq on the workspace's
identity matrices.  The bar: codes, torques and tracking equal the cycle without the bit, bit for
bit — on the lane family (DOF 3), the wave family (DOF 5, 7, 16), a stack with three non-empty
levels, robots that take the reference's retry, and across the cached workspace's reuse, where the
dense cycles must still find their identity G where they expect it."""
import numpy as np
import pytest

import mgqp
import mgqp_cases as mc
import mgqp_oracle as mo
import test_gpu_mgqp as G
import test_gpu_mgqp_shapes as S

pytestmark = pytest.mark.gpu


def _both(ctl, sc, stream=None):
    """(codes, torques, tracking) of the cycle without and with the bit, as numpy."""
    import torch

    dsc = mgqp.DeviceScenario(sc, "cuda")
    out = []
    for unit in (False, True):
        rc, codes, tq, tr = ctl().update_device(dsc, unit=unit, stream=stream)
        torch.cuda.synchronize()
        assert rc == 0
        out.append((codes.cpu().numpy(), tq.cpu().numpy(), tr.cpu().numpy()))
    return out


def _assert_same(dense, unit, what=""):
    """Codes of every robot; torques and tracking of the robots with code 0 (the cycle writes no
    outputs for the others: their rows are whatever the fresh tensors held), compared as bytes."""
    assert dense[0].tobytes() == unit[0].tobytes(), f"{what}: codes differ at {np.argwhere(dense[0] != unit[0])[:4].tolist()}"
    ok = dense[0] == 0
    for a, b, name in zip(dense[1:], unit[1:], ("torques", "tracking")):
        assert a[ok].tobytes() == b[ok].tobytes(), f"{what}: {name} differ at {np.argwhere(a[ok] != b[ok])[:4].tolist()}"


def _default(K=130, seed=70):
    return mgqp.make_scenario(K, seed=seed), mgqp.ops_controller


@pytest.mark.parametrize("name", ["dof3", "dof5", "default", "dof16", "r7"])
def test_unit_cycle_equals_dense_cycle(gpu, name):
    sc, ctl = _default() if name == "default" else mc.controllers(name)[:2]
    dense, unit = _both(ctl, sc)
    _assert_same(dense, unit, name)
    ok = int((dense[0] == 0).sum())
    print(f"{name}: {ok} of {sc.count} robots with code 0")
    assert ok >= 1
    if name not in S.DEGENERATE:
        assert ok == sc.count


def _retries(sc, configure, robots, monkeypatch):
    """Per robot of `robots`, how many level solves of the CPU oracle controller take the
    reference's retry (src/mgqp.cpp:717-736): its second solve_quadprog call, with no inequality."""
    counts = []
    real = mo.qpo.solve_one

    def counting(G, g0, CE, ce0, CI, ci0, *a, **k):
        if np.asarray(CI).shape[-1] == 0:
            counts[-1] += 1
        return real(G, g0, CE, ce0, CI, ci0, *a, **k)

    monkeypatch.setattr(mo.qpo, "solve_one", counting)
    o = mo.ops_oracle()
    configure(None, o)
    for r in robots:
        counts.append(0)
        o.update(sc, r)
    monkeypatch.undo()
    return np.array(counts)


def test_unit_cycle_with_retries(gpu, monkeypatch):
    """Wide angle limits (test_gpu_mgqp.py test_batched_wide_mixed_feasibility): some robots' level
    QPs are infeasible and take the retry without inequalities, which the unit entry returns as its
    eq triple; a few do not.  Both kinds are counted with the CPU oracle controller before anything
    is compared (measured: 249 robots with one retry, 7 with none; the float glue may move a robot
    or two between the kinds, so the bars are half of each count).  Equal to the dense cycle and to
    the host-orchestrated batch."""
    sc = mgqp.make_scenario(256, seed=9)
    retries = _retries(sc, G._wide, range(sc.count), monkeypatch)
    print(f"robots with a retry: {int((retries > 0).sum())} of {len(retries)}")
    assert (retries > 0).sum() >= 124 and (retries == 0).sum() >= 3

    def ctl():
        c = mgqp.ops_controller()
        G._wide(c)
        return c

    dense, unit = _both(ctl, sc)
    _assert_same(dense, unit, "wide")
    codes_h, tq_h, tr_h = ctl().update_batched(sc)
    assert (codes_h == 0).all()
    _assert_same((codes_h, tq_h, tr_h), unit, "wide vs host")


def _run_steps(steps, units):
    """The steps on one fresh stream (a workspace of its own), step i with unit=units[i]; every
    step against the host-orchestrated batch, all robots with code 0."""
    import torch

    s = torch.cuda.Stream()
    for i, ((what, (sc, ctl)), unit) in enumerate(zip(steps, units)):
        codes_h, tq_h, tr_h = ctl().update_batched(sc)
        assert (codes_h == 0).all()
        rc, codes, tq, tr = ctl().update_device(mgqp.DeviceScenario(sc, "cuda"), unit=unit, stream=s.cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        _assert_same((codes_h, tq_h, tr_h), (codes.cpu().numpy(), tq.cpu().numpy(), tr.cpu().numpy()),
                     f"step {i + 1} ({what}), unit={unit}")


def test_unit_cycle_workspace_reuse(gpu):
    """test_device_workspace_reuse's six steps on one stream with unit=True on alternate steps, in
    both parities: the dense cycles between the unit ones must find (or write) their identity
    matrices where their layout puts them."""
    steps = [("default, 11 rows", _default(130)), ("one more joint row, 12", S._more_joint_rows()),
             ("default again", _default(130)), ("K = 260", _default(260)),
             ("DOF 5", mc.controllers("dof5", K=130)[:2]), ("default", _default(130))]
    _run_steps(steps, [True, False, True, False, True, False])
    _run_steps(steps, [False, True, False, True, False, True])


def test_unit_cycle_moves_the_arrays_in_a_buffer_that_does_not_grow(gpu):
    """Same K and dim, task stacks of 11 and 12 rows, after a K = 260 cycle has made the buffer
    large enough for both: nothing is reallocated, so only the record of where G = I and g0 = 0 lie
    protects the dense cycles.  A unit cycle of the other stack puts its g0, CE, ce0 and V over the
    recorded layout's G and g0; the dense cycle that follows on the recorded stack must write them
    again.  Both directions (12 dense, 11 unit, 12 dense; 11 dense, 12 unit, 11 dense), then a unit
    cycle of the recorded stack itself, after which the dense cycle may keep what it finds."""
    grow = ("K = 260", _default(260))
    s11, s12 = ("11 rows", _default(130)), ("12 rows", S._more_joint_rows())
    _run_steps([grow, s12, s11, s12, s12, s12], [False, False, True, False, True, False])
    _run_steps([grow, s11, s12, s11, s11, s11], [False, False, True, False, True, False])
    _run_steps([grow, s12, s11, s11, s12], [True, False, True, False, False])


def test_unit_with_fast_raises(gpu):
    sc, ctl = _default(8)
    dsc = mgqp.DeviceScenario(sc, "cuda")
    with pytest.raises(RuntimeError, match="UNIT_HESSIAN"):
        ctl().update_device(dsc, unit=True, fast=True)
    rc, codes, _, _ = ctl().update_device(dsc, unit=True)  # the batch object is still usable
    assert rc == 0 and (codes.cpu().numpy() == 0).all()
