"""The device-resident control cycle beyond the 7-DOF reference robot (tests/mgqp_cases.py): every
builder kernel (register-resident dims 6..14, the generic one at DOF 1, 2, 8, 16), every stacked
row count the register projector is instantiated for, the LDS projector in both shapes (fewer
stacked rows than columns, and at least as many), a Jacobian narrower than the problem, and the
cached per-(device, stream) workspace across successive configurations.

The bar is the one of test_gpu_mgqp.py: the device cycle equals the host-orchestrated batch bit
for bit (same operations in the same order, bitwise solver), the host controller matches the
numpy/C oracle within 1e-4 x max(1, |output|) where the case is well posed, and the batched host
path equals the single-cycle path bit for bit.  The checks that need no device cycle take the
controller library as a parameter and run in the CPU suite as well (test_mgqp_host.py).
"""
import numpy as np
import pytest

import mgqp
import mgqp_cases as mc
import test_gpu_mgqp as G

pytestmark = pytest.mark.gpu

LIB = None  # None = the shipped libmgqp_amd.so (GPU)

# Z after these cases' stacked levels is round-off (as many rows as columns, or more), so the
# next level is chaotic against the oracle; device and host still share every operation
DEGENERATE = ("dof3", "dof4", "r14", "r15")
DEVICE_CASES = ("dof3", "dof4", "dof5", "dof6", "dof8", "dof16", "r7", "r8", "r9_12", "r13",
                "r14", "r15", "narrow_jac_l1", "narrow_jac_l0")
# (case, K, seed): the oracle comparison's well-posed cases.  Measured (CPU harness and GPU
# library alike): robots the oracle marks ill-conditioned 0, 0, 0, 0, 0, 0, 2 (robots 70 and 101);
# worst error over max(1, |output|) 2.0e-7, 2.3e-7, 2.5e-7, 4.4e-7, 4.9e-7, 5.0e-7, 1.2e-6
ORACLE_CASES = (("dof5", 100, 55), ("dof6", 100, 56), ("dof8_default", 100, 58),
                ("dof16", 100, 66), ("r7", 200, 61), ("r8", 200, 62), ("r9_12", 200, 63))
# the oracle marks 9-60 % of these cases' robots ill-conditioned, or differs from the host on
# exception codes through float noise: batched == single cycle instead
BITWISE_CASES = ("r13", "r14", "r15", "narrow_jac_l1", "narrow_jac_l0", "dof3", "dof4")


# --- host controller against the oracle, and against itself -------------------------------------
def _check_ill(ill, checked):
    """At most 1 robot in 50 may be excluded as ill-conditioned; the failure lists them."""
    assert len(ill) <= checked // 50, f"{len(ill)} of {checked} robots excluded as ill-conditioned: {ill}"


@pytest.mark.parametrize("name,K,seed", ORACLE_CASES)
def test_host_matches_oracle(gpu, name, K, seed, lib=LIB):
    sc, ctl, oracle = mc.controllers(name, lib, K, seed)
    codes, tq, tr = ctl().update_batched(sc)
    o = oracle()
    ill, worst = [], 0.0
    for r in range(sc.count):
        ocode, otq, otr = o.update(sc, r)
        assert codes[r] == ocode == 0
        if o.ill_conditioned:
            ill.append(r)
            continue
        for a, b in ((tr[r], otr), (tq[r], otq)):
            worst = max(worst, float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max())))
    print(f"{name}: K={K} seed={seed} ill-conditioned {ill} worst error {worst:.2e}")
    _check_ill(ill, sc.count)
    assert worst <= 1e-4


@pytest.mark.parametrize("name", BITWISE_CASES)
def test_batched_equals_single_bitwise(gpu, name, lib=LIB):
    sc, ctl, _ = mc.controllers(name, lib, K=48)
    codes, tq, tr = ctl().update_batched(sc)
    c1 = ctl()
    for r in range(0, sc.count, 5):
        code, t1, r1, _ = c1.updateHook(sc.robot(r))
        assert code == codes[r]
        if code == 0:
            np.testing.assert_array_equal(tr[r], r1)
            np.testing.assert_array_equal(tq[r], t1)
    assert (codes[::5] == 0).any()


def test_narrow_jacobian_zero_fill(gpu, lib=LIB):
    """Builder against hand values: joint 4's task has J = [e1; e2; e3] (3 x 4), Jdot = 0 and
    position error (0.01, -0.02, 0.005) at level 0, all other task ports equal.  With kTP = 100
    its rows read acc[0:3] = (1, -2, 0.5) exactly when columns 4..13 of the rows are zero."""
    sc, ctl, _ = mc.controllers("narrow_jac_l0", lib, K=4)
    J = np.zeros((3, 4), np.float32)
    J[0, 0] = J[1, 1] = J[2, 2] = 1
    sc.ports[(3, "jacobian")][0] = J
    sc.ports[(3, "jacobian_dot")][0] = 0
    for nm in mgqp.TS_PORTS:
        sc.ports[(3, nm)][0] = 0
    sc.ports[(3, "desired_ts_position")][0] = (0.01, -0.02, 0.005)
    want = np.array([1, -2, 0.5], np.float32)
    code, _, tr, _ = ctl().updateHook(sc.robot(0))
    assert code == 0
    np.testing.assert_allclose(tr[:3], want, rtol=0, atol=1e-4)
    codes, _, trb = ctl().update_batched(sc)
    assert codes[0] == 0
    np.testing.assert_array_equal(trb[0], tr)


@pytest.mark.parametrize("name", ["dof1", "dof2"])
def test_more_rows_than_columns_raise(gpu, name, lib=LIB):
    """DOF 1 and 2: level 0 stacks 3 task rows and DOF dynamics rows on 2 x DOF columns (4 on 2,
    5 on 4), so the equality phase finds a dependent row for every robot: CYCLE_EXCEPTION, as
    the reference's solve_quadprog throws."""
    sc, ctl, oracle = mc.controllers(name, lib, K=6)
    c = ctl()
    codes, _, _ = c.update_batched(sc)
    assert (codes == mgqp.CYCLE_EXCEPTION).all()
    assert c.updateHook(sc.robot(2))[0] == mgqp.CYCLE_EXCEPTION
    assert "linearly dependent" in c.last_error()
    with pytest.raises(RuntimeError, match="linearly dependent"):
        oracle().update(sc, 2)


# --- device-resident cycle against the host-orchestrated batch ----------------------------------
@pytest.mark.parametrize("name", DEVICE_CASES)
def test_device_cycle_equals_batched(gpu, name):
    sc, ctl, _ = mc.controllers(name)
    codes = G._device_vs_batched(ctl(), ctl(), sc)
    ok = int((codes == 0).sum())
    print(f"{name}: {ok} of {sc.count} robots with code 0")
    if name in DEGENERATE:
        assert ok >= 1  # otherwise the projector's output is never observed
    else:
        assert ok == sc.count


@pytest.mark.parametrize("name", ["dof1", "dof2"])
def test_device_cycle_more_rows_than_columns(gpu, name):
    sc, ctl, _ = mc.controllers(name)
    codes = G._device_vs_batched(ctl(), ctl(), sc)
    assert (codes == mgqp.CYCLE_EXCEPTION).all()


@pytest.mark.parametrize("name", ["dof5", "dof8", "dof16"])
def test_device_cycle_fast_solves(gpu, name):
    import torch

    sc, ctl, _ = mc.controllers(name)
    dsc = mgqp.DeviceScenario(sc, "cuda")
    rc, codes, tq, tr = ctl().update_device(dsc)
    torch.cuda.synchronize()
    codes, tq, tr = codes.cpu().numpy(), tq.cpu().numpy(), tr.cpu().numpy()
    rcf, codesf, tqf, trf = ctl().update_device(dsc, fast=True)
    torch.cuda.synchronize()
    assert rc == rcf == 0
    np.testing.assert_array_equal(codesf.cpu().numpy(), codes)
    ok = codes == 0
    assert ok.any()
    G._close(tqf.cpu().numpy()[ok], tq[ok])
    G._close(trf.cpu().numpy()[ok], tr[ok])


def _more_joint_rows(K=130, seed=71):
    """The default stack with a second joint row at level 2: 12 rows in all instead of 11."""
    sc = mgqp.make_scenario(K, seed=seed)
    sc.ports[(1, "desired_js_position")] = np.linspace(-0.3, 0.3, K).astype(np.float32)

    def ctl():
        c = mgqp.ops_controller()
        assert c.setPriorityLevel("in_desiredJointSpacePosition_2", 2)
        return c
    return sc, ctl


def test_device_workspace_reuse(gpu):
    """One stream, successive configurations: the cached workspace's identity Hessian and zero
    linear term must be where each cycle's layout puts them.  Steps 1-3 keep K and DOF and move
    the QP arrays by one task row; 4 grows the buffer; 5 changes the dimension; 6 comes back."""
    default = lambda K: (mgqp.make_scenario(K, seed=70), mgqp.ops_controller)
    steps = [("default, 11 rows", default(130)), ("one more joint row, 12", _more_joint_rows()),
             ("default again", default(130)), ("K = 260", default(260)),
             ("DOF 5", mc.controllers("dof5", K=130)[:2]), ("default", default(130))]
    for i, (what, (sc, ctl)) in enumerate(steps):
        try:
            codes = G._device_vs_batched(ctl(), ctl(), sc)
        except AssertionError as e:
            raise AssertionError(f"step {i + 1} ({what}): {e}") from None
        assert (codes == 0).all(), f"step {i + 1} ({what})"


def test_device_two_streams(gpu):
    """Two streams, a different case on each, three cycles each, interleaved from one thread:
    each (device, stream) has its own workspace."""
    import torch

    runs = []
    for name in ("r7", "dof8"):
        sc, ctl, _ = mc.controllers(name, K=130)
        runs.append((sc, mgqp.DeviceScenario(sc, "cuda"), ctl(), ctl().update_batched(sc),
                     torch.cuda.Stream(), []))
    torch.cuda.synchronize()
    for _ in range(3):
        for sc, dsc, c, _, stream, outs in runs:
            rc, codes, tq, tr = c.update_device(dsc, stream=stream.cuda_stream)
            assert rc == 0
            outs.append((codes, tq, tr))
    torch.cuda.synchronize()
    for sc, dsc, c, (codes_h, tq_h, tr_h), stream, outs in runs:
        assert (codes_h == 0).all()
        for codes, tq, tr in outs:
            np.testing.assert_array_equal(codes.cpu().numpy(), codes_h)
            np.testing.assert_array_equal(tq.cpu().numpy(), tq_h)
            np.testing.assert_array_equal(tr.cpu().numpy(), tr_h)
