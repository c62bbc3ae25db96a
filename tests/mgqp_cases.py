"""Controller cases beyond the 7-DOF reference robot with its default stack: every DOF class of
the device-resident cycle (csrc/mgqp_device.hip), every stacked-row count its projector kernels
are instantiated for, and a Jacobian narrower than the problem.

A case is a function `case(K=..., seed=...)` returning `(scenario, configure)`;
`configure(ctl_or_oracle)` applies the case's priority levels to a `mgqp.Controller` (through
setPriorityLevel) or to an `OracleController` (through its `levels` dict).  `controllers(name)`
builds fresh, configured ones.

`device_plan()` restates in Python how `update_device` (csrc/mgqp_device_host.cpp) groups the
rows by level, and `EXPECTED[name]` is the (dim, stacked rows per non-last level) that makes the
case reach the device code named next to it.  The tests assert that the two agree, so a later
edit of a case cannot silently stop reaching its kernel.

Joints are numbered from 1 in port names ("joint 2" is `in_desiredJointSpacePosition_2`,
scenario port index 1), as in the reference deployment.
"""
import numpy as np

import mgqp
import mgqp_oracle as mo

WS = 3
STACK = 3  # stack_of_tasks.init(3)
_TS = ("Position", "Velocity", "Acceleration")


def _ramp(K):
    return np.linspace(-0.3, 0.3, K).astype(np.float32)


def _set_levels(pairs):
    def configure(c):
        for name, lvl in pairs:
            if isinstance(c, mgqp.Controller):
                assert c.setPriorityLevel(name, lvl)
            else:
                c.levels[name] = lvl
    return configure


def _js(sc, joint, kind="position"):
    """Connects joint-space port `kind` of joint `joint` (numbered from 1); returns its task name."""
    sc.ports[(joint - 1, "desired_js_" + kind)] = _ramp(sc.count)
    return f"in_desiredJointSpace{kind.capitalize()}_{joint}"


def _task_levels(joint, lvl):
    return [(f"in_desiredTaskSpace{nm}_{joint}", lvl) for nm in _TS]


def _copy_task(sc, joint, seed, cols=None):
    """Gives joint `joint` (numbered from 1) the six task-space ports and both Jacobians of
    another seed's end effector; `cols` keeps only the Jacobians' first columns."""
    other = mgqp.make_scenario(sc.count, seed=seed, dof=sc.dof)
    e = sc.dof - 1
    for nm in mgqp.TS_PORTS:
        sc.ports[(joint - 1, nm)] = other.ports[(e, nm)].copy()
    for nm in ("jacobian", "jacobian_dot"):
        J = other.ports[(e, nm)]
        sc.ports[(joint - 1, nm)] = np.ascontiguousarray(J if cols is None else J[:, :, :cols])


def _default(dof, K0, seed0):
    def case(K=K0, seed=seed0):
        return mgqp.make_scenario(K, seed=seed, dof=dof), _set_levels([])
    return case


def _js_positions(dof, joints, lvl, K0, seed0):
    def case(K=K0, seed=seed0):
        sc = mgqp.make_scenario(K, seed=seed, dof=dof)
        return sc, _set_levels([(_js(sc, j), lvl) for j in joints])
    return case


def _r7(K=200, seed=61):
    sc = mgqp.make_scenario(K, seed=seed)
    return sc, _set_levels(_task_levels(7, 1))


def _r8(K=200, seed=62):
    sc = mgqp.make_scenario(K, seed=seed)
    return sc, _set_levels(_task_levels(7, 1) + [("in_desiredJointSpacePosition_1", 0),
                                                 (_js(sc, 3, "velocity"), 2)])


def _r9_12(K=200, seed=63):
    sc = mgqp.make_scenario(K, seed=seed)
    return sc, _set_levels(_task_levels(7, 1) + [("in_desiredJointSpacePosition_1", 0),
                                                 (_js(sc, 3, "velocity"), 2), (_js(sc, 2), 0)])


def _narrow(lvl, seed0):
    def case(K=200, seed=seed0):
        sc = mgqp.make_scenario(K, seed=seed)
        _copy_task(sc, 4, seed + 1000, cols=4)  # second task joint: index 3, (K, 3, 4) Jacobians
        return sc, _set_levels(_task_levels(4, lvl))
    return case


CASES = {
    "dof1": _default(1, 130, 51),
    "dof2": _default(2, 130, 52),
    "dof3": _default(3, 200, 53),
    "dof4": _js_positions(4, [2], 1, 200, 54),
    "dof5": _default(5, 200, 55),
    "dof6": _default(6, 200, 56),
    "dof8": _js_positions(8, [2, 3], 1, 200, 58),
    "dof8_default": _default(8, 100, 58),
    "dof16": _default(16, 130, 66),
    "r7": _r7,
    "r8": _r8,
    "r9_12": _r9_12,
    "r13": _js_positions(7, [2, 3, 4], 1, 200, 64),
    "r14": _js_positions(7, [2, 3, 4, 5], 1, 200, 65),
    "r15": _js_positions(7, [2, 3, 4, 5, 6], 1, 200, 67),
    "narrow_jac_l1": _narrow(1, 68),
    "narrow_jac_l0": _narrow(0, 69),
}

# name -> (dim, stacked rows Acumul holds after each level but the last): what the device's
# projector is launched with, hence which kernel serves the case
EXPECTED = {
    "dof1": (2, [4]),              # generic builder; level 0 has 4 rows > dim: "dependent"
    "dof2": (4, [5]),              # the same with 5 rows > 4
    "dof3": (6, [6]),              # build_level_reg<6>; generic projector, rr == c after level 0
    "dof4": (8, [7, 8]),           # build_level_reg<8>; rr < c, then rr == c
    "dof5": (10, [8]),             # build_level_reg<10>; generic projector, rr < c
    "dof6": (12, [9]),             # build_level_reg<12>
    "dof8": (16, [11, 13]),        # generic builder; projector blocks of 32 lanes
    "dof8_default": (16, [11]),
    "dof16": (32, [19]),           # generic builder; blocks of 8 lanes; QP (32, 19, 64)
    "r7": (14, [7, 10]),           # finish_level_reg<14,7> + zform
    "r8": (14, [8, 11]),           # <14,8>
    "r9_12": (14, [9, 12]),        # <14,9>, <14,12>
    "r13": (14, [10, 13]),         # generic projector at dim 14, rr < c
    "r14": (14, [10, 14]),         # rr >= c with the rotation accumulator; blocks of 16 lanes
    "r15": (14, [10, 15]),
    "narrow_jac_l1": (14, [10, 13]),  # c < jc zero fill in a level-1 row block
    "narrow_jac_l0": (14, [13]),      # ... and in level 0
}

# the device builders: register-resident for these dims, the generic kernel for every other
REG_BUILDER_DIMS = (6, 8, 10, 12, 14)
# stacked-row counts of finish_level_reg<14, R>; every other (dim, rows) takes the LDS projector
REG_PROJECTOR_ROWS = (7, 8, 9, 10, 11, 12)


def controllers(name, library=None, K=None, seed=None):
    """(scenario, configured mgqp.Controller factory, configured oracle factory) of a case."""
    kw = {k: v for k, v in (("K", K), ("seed", seed)) if v is not None}
    sc, configure = CASES[name](**kw)

    def ctl():
        c = mgqp.ops_controller(dof=sc.dof, library=library)
        configure(c)
        return c

    def oracle():
        o = mo.ops_oracle(dof=sc.dof)
        configure(o)
        return o

    return sc, ctl, oracle


def device_plan(sc, levels):
    """update_device's row plan for scenario `sc` under the task -> level map `levels`: returns
    (dim, rows per level, stacked rows passed to the projector after each level but the last).
    Joints outer, levels inner; a joint's task rows (WS of them) when any of its three
    desired/current task-space port pairs is connected at that level, one joint row when any of
    its joint-space ports is; the DOF dynamics rows close level 0."""
    D = sc.dof
    rows = [0] * STACK
    for j in range(D):
        for lvl in range(STACK):
            if any((j, "desired_ts_" + nm.lower()) in sc.ports and
                   (j, "current_ts_" + nm.lower()) in sc.ports and
                   levels.get(f"in_desiredTaskSpace{nm}_{j + 1}", -1) == lvl for nm in _TS):
                rows[lvl] += WS
            if any((j, "desired_js_" + nm.lower()) in sc.ports and
                   levels.get(f"in_desiredJointSpace{nm}_{j + 1}", -1) == lvl for nm in _TS):
                rows[lvl] += 1
    rows[0] += D
    last = max(l for l in range(STACK) if rows[l] > 0)
    stacked, acc = [], 0
    for l in range(last):
        acc += rows[l]
        if rows[l] > 0:
            stacked.append(acc)
    return 2 * D, rows, stacked


def plan_of(name):
    sc, _, oracle = controllers(name, K=2)
    return device_plan(sc, oracle().levels)
