"""qpgpu — Python host mirror of the batched solve_quadprog() C-ABI (include/qpgpu.h).

The reference interface this mirrors is the solver call at reference src/mgqp.cpp:708
(``solve_quadprog(G, g0, t(CE), ce0, t(CI), ci0, x)``, declared at
include/QuadProgpp/QuadProg++.hh:69-72), batched: the same argument meanings, the same sign
convention (``CE^T x + ce0 = 0``, ``CI^T x + ci0 >= 0``), the same "G is overwritten" option,
and the same error outcomes, reported per QP as status codes instead of exceptions
(``solve_quadprog`` in this module re-raises them exactly like the reference for one QP).

Every solve runs on the gfx950 HIP kernels in ``lib/libqpgpu.so``.  If that library is missing
this module raises at import time; there is no CPU fallback.

Also hosts the synthetic problem generator of SURVEY.md §8(d): a counter-based SplitMix64
stream keyed by (seed, qp_index, stream, element), so any shard of a batch can be generated
independently and identically on every rank.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.environ.get("QPGPU_LIB_PATH") or os.path.join(LIB_DIR, "libqpgpu.so")  # env: A/B builds only
DROPIN_PATH = os.path.join(LIB_DIR, "libquadprog_amd.so")

# per-QP status codes (include/qpgpu.h)
QP_OK = 0
QP_INFEASIBLE = 1
QP_NOT_POSITIVE_DEFINITE = 2
QP_DEPENDENT = 3
QP_MAX_ITER = 4
STATUS_NAMES = {0: "ok", 1: "infeasible", 2: "not_positive_definite", 3: "dependent", 4: "max_iter"}

# API return codes
SUCCESS = 0
ERR_INVALID_ARGUMENT = 1
ERR_UNSUPPORTED_SHAPE = 2
ERR_HIP = 3
ERR_NO_DEVICE = 4

FLAG_WRITE_FACTOR = 0x1
FLAG_EXACT = 0x2  # reference operation order for n > 64 too (no MFMA panel setup)
FLAG_FAST = 0x4  # lane-kernel shapes: fused multiply-adds, shared reciprocals (1e-10, not bitwise)
FLAG_FORCE_LANE = 0x100
FLAG_FORCE_SUBGROUP = 0x200
FLAG_FORCE_WAVE = 0x400
FLAG_FORCE_GENERIC = 0x800  # any shape: the generic workspace kernel (qp_generic.hip)
FAMILY_FLAGS = {None: 0, "auto": 0, "lane": FLAG_FORCE_LANE, "subgroup": FLAG_FORCE_SUBGROUP,
                "wave": FLAG_FORCE_WAVE, "generic": FLAG_FORCE_GENERIC}
LAYOUT_QP_MAJOR = 0
LAYOUT_TILED64 = 1
LAYOUTS = {None: 0, "qp_major": LAYOUT_QP_MAJOR, "tiled64": LAYOUT_TILED64}

# slots of a QP's block of qpgpu_kkt_residuals (include/qpgpu.h)
KKT_STAT, KKT_STAT_SCALE, KKT_EQ, KKT_INEQ, KKT_COMP, KKT_UMIN, KKT_OBJ, KKT_NNZ = range(8)
KKT_NRES = 8

EXPORTED_SYMBOLS = (
    "qpgpu_solve_batched",
    "qpgpu_solve_batched_eq",
    "qpgpu_solve_batched_dual",
    "qpgpu_solve_batched_box",
    "qpgpu_kernel_name_box",
    "qpgpu_solve_batched_box_dual",
    "qpgpu_kernel_name_box_dual",
    "qpgpu_solve_batched_unit",
    "qpgpu_kernel_name_unit",
    "qpgpu_kkt_residuals",
    "qpgpu_kkt_residuals_box",
    "qpgpu_vjp",
    "qpgpu_vjp_box",
    "qpgpu_kernel_name_vjp",
    "qpgpu_vjp_workspace_bytes",
    "qpgpu_vjp_ws",
    "qpgpu_vjp_box_ws",
    "qpgpu_kernel_name_vjp_ws",
    "qpgpu_vjp_full",
    "qpgpu_vjp_box_full",
    "qpgpu_kernel_name_vjp_full",
    "qpgpu_jvp",
    "qpgpu_jvp_box",
    "qpgpu_kernel_name_jvp",
    "qpgpu_jvp_many",
    "qpgpu_jvp_box_many",
    "qpgpu_kernel_name_jvp_many",
    "qpgpu_solve_batched_host",
    "qpgpu_max_n",
    "qpgpu_max_m",
    "qpgpu_kernel_name",
    "qpgpu_kernel_name_flags",
    "qpgpu_last_error",
    "qpgpu_device_count",
    "qpgpu_abi_version",
    "qpgpu_relayout",
    "qpgpu_solve_batched_multi",
)


class QpgpuError(RuntimeError):
    pass


class ProblemDesc(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int32),
        ("p", ctypes.c_int32),
        ("m", ctypes.c_int32),
        ("max_iter", ctypes.c_int32),
        ("batch", ctypes.c_int64),
        ("flags", ctypes.c_uint32),
        ("layout", ctypes.c_uint32),
    ]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"qpgpu: {LIB_PATH} is missing; build it with `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    vp = ctypes.c_void_p
    lib.qpgpu_solve_batched.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 11
    lib.qpgpu_solve_batched.restype = ctypes.c_int
    lib.qpgpu_solve_batched_eq.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 14
    lib.qpgpu_solve_batched_eq.restype = ctypes.c_int
    lib.qpgpu_solve_batched_dual.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 13
    lib.qpgpu_solve_batched_dual.restype = ctypes.c_int
    lib.qpgpu_solve_batched_box.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 11
    lib.qpgpu_solve_batched_box.restype = ctypes.c_int
    lib.qpgpu_kernel_name_box.argtypes = [ctypes.c_int32] * 2 + [ctypes.c_uint32]
    lib.qpgpu_kernel_name_box.restype = ctypes.c_char_p
    lib.qpgpu_solve_batched_box_dual.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 13
    lib.qpgpu_solve_batched_box_dual.restype = ctypes.c_int
    lib.qpgpu_kernel_name_box_dual.argtypes = [ctypes.c_int32] * 2 + [ctypes.c_uint32]
    lib.qpgpu_kernel_name_box_dual.restype = ctypes.c_char_p
    lib.qpgpu_solve_batched_unit.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 13
    lib.qpgpu_solve_batched_unit.restype = ctypes.c_int
    lib.qpgpu_kernel_name_unit.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_uint32]
    lib.qpgpu_kernel_name_unit.restype = ctypes.c_char_p
    lib.qpgpu_kkt_residuals.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 11
    lib.qpgpu_kkt_residuals.restype = ctypes.c_int
    lib.qpgpu_kkt_residuals_box.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 11
    lib.qpgpu_kkt_residuals_box.restype = ctypes.c_int
    lib.qpgpu_vjp.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 14
    lib.qpgpu_vjp.restype = ctypes.c_int
    lib.qpgpu_vjp_box.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 13
    lib.qpgpu_vjp_box.restype = ctypes.c_int
    lib.qpgpu_kernel_name_vjp.argtypes = [ctypes.c_int32] * 3
    lib.qpgpu_kernel_name_vjp.restype = ctypes.c_char_p
    lib.qpgpu_vjp_workspace_bytes.argtypes = [ctypes.POINTER(ProblemDesc), ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.qpgpu_vjp_workspace_bytes.restype = ctypes.c_int
    lib.qpgpu_vjp_ws.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 13 + [vp, ctypes.c_int64, vp]
    lib.qpgpu_vjp_ws.restype = ctypes.c_int
    lib.qpgpu_vjp_box_ws.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 12 + [vp, ctypes.c_int64, vp]
    lib.qpgpu_vjp_box_ws.restype = ctypes.c_int
    lib.qpgpu_kernel_name_vjp_ws.argtypes = [ctypes.c_int32] * 3
    lib.qpgpu_kernel_name_vjp_ws.restype = ctypes.c_char_p
    lib.qpgpu_vjp_full.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 15 + [vp, ctypes.c_int64, vp]
    lib.qpgpu_vjp_full.restype = ctypes.c_int
    lib.qpgpu_vjp_box_full.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 14 + [vp, ctypes.c_int64, vp]
    lib.qpgpu_vjp_box_full.restype = ctypes.c_int
    lib.qpgpu_kernel_name_vjp_full.argtypes = [ctypes.c_int32] * 3
    lib.qpgpu_kernel_name_vjp_full.restype = ctypes.c_char_p
    lib.qpgpu_jvp.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 16
    lib.qpgpu_jvp.restype = ctypes.c_int
    lib.qpgpu_jvp_box.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 15
    lib.qpgpu_jvp_box.restype = ctypes.c_int
    lib.qpgpu_kernel_name_jvp.argtypes = [ctypes.c_int32] * 3
    lib.qpgpu_kernel_name_jvp.restype = ctypes.c_char_p
    lib.qpgpu_jvp_many.argtypes = [ctypes.POINTER(ProblemDesc), ctypes.c_int32] + [vp] * 16
    lib.qpgpu_jvp_many.restype = ctypes.c_int
    lib.qpgpu_jvp_box_many.argtypes = [ctypes.POINTER(ProblemDesc), ctypes.c_int32] + [vp] * 15
    lib.qpgpu_jvp_box_many.restype = ctypes.c_int
    lib.qpgpu_kernel_name_jvp_many.argtypes = [ctypes.c_int32] * 3
    lib.qpgpu_kernel_name_jvp_many.restype = ctypes.c_char_p
    lib.qpgpu_solve_batched_host.argtypes = [ctypes.POINTER(ProblemDesc)] + [vp] * 10
    lib.qpgpu_solve_batched_host.restype = ctypes.c_int
    lib.qpgpu_solve_batched_multi.argtypes = [ctypes.POINTER(ProblemDesc), ctypes.c_int32, vp] + [vp] * 10
    lib.qpgpu_solve_batched_multi.restype = ctypes.c_int
    lib.qpgpu_kernel_name.argtypes = [ctypes.c_int32] * 3
    lib.qpgpu_kernel_name.restype = ctypes.c_char_p
    lib.qpgpu_kernel_name_flags.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_uint32]
    lib.qpgpu_kernel_name_flags.restype = ctypes.c_char_p
    lib.qpgpu_last_error.restype = ctypes.c_char_p
    lib.qpgpu_max_n.restype = ctypes.c_int
    lib.qpgpu_max_m.restype = ctypes.c_int
    lib.qpgpu_device_count.restype = ctypes.c_int
    lib.qpgpu_abi_version.restype = ctypes.c_int
    lib.qpgpu_relayout.argtypes = [ctypes.c_int64, ctypes.c_int32, vp, vp, ctypes.c_int32, vp]
    lib.qpgpu_relayout.restype = ctypes.c_int
    return lib


LIB = _load()


def build_provenance() -> dict:
    """Which sources the loaded libqpgpu.so was built from: the md5 of the library, the sha256 the
    Makefile recorded over its sources at link time (lib/libqpgpu.sources), the sha256 of those
    files now, and whether they match (False: the library is older than its sources — rebuild;
    None: the record or the sources are absent, e.g. an A/B library)."""
    import hashlib

    rec = os.path.join(os.path.dirname(LIB_PATH), "libqpgpu.sources")
    out = {"lib": os.path.relpath(LIB_PATH, os.path.dirname(LIB_DIR)),
           "lib_md5": hashlib.md5(open(LIB_PATH, "rb").read()).hexdigest(),
           "sources_sha256_at_build": None, "sources_sha256_now": None, "matches_sources": None}
    try:
        files, sha = open(rec).read().split("\n")[:2]
    except (OSError, ValueError):
        return out
    out["sources_sha256_at_build"] = sha.strip()
    pkg = os.path.dirname(LIB_DIR)
    try:
        h = hashlib.sha256()
        for f in files.split():
            h.update(open(os.path.join(pkg, f), "rb").read())
        out["sources_sha256_now"] = h.hexdigest()
        out["matches_sources"] = out["sources_sha256_now"] == out["sources_sha256_at_build"]
    except OSError:
        pass
    return out


def kernel_name(n: int, p: int, m: int, fast: bool = False) -> str:
    if fast:
        return LIB.qpgpu_kernel_name_flags(n, p, m, FLAG_FAST).decode()
    return LIB.qpgpu_kernel_name(n, p, m).decode()


def kernel_name_box(n: int, p: int, flags: int = 0) -> str:
    """The kernel a qpgpu_solve_batched_box launch of shape (n, p) with `flags` runs ("" for a
    rejected flag combination or n <= 0); every box kernel's name contains "box"."""
    return LIB.qpgpu_kernel_name_box(n, p, flags).decode()


def kernel_name_box_dual(n: int, p: int, flags: int = 0) -> str:
    """The kernel a qpgpu_solve_batched_box_dual launch of shape (n, p) with `flags` runs ("" where
    kernel_name_box is ""); every such name contains "box" and "dual"."""
    return LIB.qpgpu_kernel_name_box_dual(n, p, flags).decode()


def kernel_name_unit(n: int, p: int, m: int, flags: int = 0) -> str:
    """The kernel a qpgpu_solve_batched_unit launch of shape (n, p, m) with `flags` runs; every
    such name contains "unit".  "" where the entry refuses: n > 64, m > 256, FLAG_FORCE_GENERIC,
    FLAG_FAST, FLAG_WRITE_FACTOR, a forced family that lacks the shape."""
    return LIB.qpgpu_kernel_name_unit(n, p, m, flags).decode()


def kernel_name_vjp(n: int, p: int = 0, m: int = 0) -> str:
    """The kernel a qpgpu_vjp / qpgpu_vjp_box launch of this shape runs: a "lane" name for n <= 8, a
    "group" name for 8 < n <= 64, "" beyond (QPGPU_ERR_UNSUPPORTED_SHAPE)."""
    return LIB.qpgpu_kernel_name_vjp(n, p, m).decode()


VJP_ON_CHIP_N = 64  # qpgpu_vjp / qpgpu_vjp_box stop here; beyond, the _ws entries take a workspace
VJP_SLOTS = 512     # QPs in flight of a backward step with a workspace, unless the caller says


def kernel_name_vjp_ws(n: int, p: int = 0, m: int = 0) -> str:
    """The kernel a qpgpu_vjp_ws / qpgpu_vjp_box_ws launch of this shape runs: kernel_name_vjp's for
    n <= 64, a "ws" name for 64 < n <= 256, "" beyond (QPGPU_ERR_UNSUPPORTED_SHAPE)."""
    return LIB.qpgpu_kernel_name_vjp_ws(n, p, m).decode()


def kernel_name_vjp_full(n: int, p: int = 0, m: int = 0) -> str:
    """The kernel a qpgpu_vjp_full / qpgpu_vjp_box_full launch of this shape runs: a name with "full"
    in it, and "lane" for n <= 8, "group" for 8 < n <= 64, "ws" for 64 < n <= 256; "" beyond."""
    return LIB.qpgpu_kernel_name_vjp_full(n, p, m).decode()


def kernel_name_jvp(n: int, p: int = 0, m: int = 0) -> str:
    """The kernel a qpgpu_jvp / qpgpu_jvp_box launch of this shape runs: a name with "jvp", and "lane"
    for n <= 8, "group" for 8 < n <= 64; "" for n > 64 or n <= 0."""
    return LIB.qpgpu_kernel_name_jvp(n, p, m).decode()


def kernel_name_jvp_many(n: int, p: int = 0, m: int = 0) -> str:
    """The kernel a qpgpu_jvp_many / qpgpu_jvp_box_many launch of this shape runs: a name with "jvp" and
    "many", and "lane" or "group"; "" for n > 64 or n <= 0."""
    return LIB.qpgpu_kernel_name_jvp_many(n, p, m).decode()


JVP_OUTPUTS = ("tx", "tu", "tf")


def vjp_workspace_bytes(n: int, p: int, m: int, slots: int) -> int:
    """qpgpu_vjp_workspace_bytes: the workspace of `slots` QPs in flight (0 for n <= 64)."""
    d = ProblemDesc(n, p, m, 0, 0, 0, 0)
    out = ctypes.c_int64(0)
    _check(LIB.qpgpu_vjp_workspace_bytes(ctypes.byref(d), slots, ctypes.byref(out)), "qpgpu_vjp_workspace_bytes")
    return out.value


def _vjp_workspace(n, p, m, batch, slots, device):
    """The uint8 workspace tensor of min(batch, slots) slots, from torch's caching allocator (so it
    is ordered on the current stream like every other tensor)."""
    import torch

    return torch.empty(vjp_workspace_bytes(n, p, m, max(1, min(batch, slots))), dtype=torch.uint8, device=device)


# the n > 64 default path's certification: a QP whose decisions the tolerance mode
# cannot certify carries STATUS_RESOLVE | reasons << 9 until the EXACT re-solve rewrites it
STATUS_RESOLVE = 0x100
UNC_REASONS = ("dependent", "setup", "max_iter", "step_tie", "zz", "t_t2", "select_tie", "psi",
               "f_cancel", "x_cancel", "non_finite", "t1_tie", "givens")


def set_resolve(on: bool) -> None:
    """Test / diagnostic hook: False skips the EXACT re-solve of uncertified n > 64 QPs and leaves
    their marks in the status words (see unc_reasons)."""
    fn = LIB.qpgpu_debug_set_resolve
    fn.argtypes = [ctypes.c_int]
    fn(1 if on else 0)


def set_shadow(on: bool) -> None:
    """Test / diagnostic hook: False makes the n > 64 default path's l1 scans fp64-only instead of
    reading the fp32 copy of CI first; results are the same bit for bit."""
    fn = LIB.qpgpu_debug_set_shadow
    fn.argtypes = [ctypes.c_int]
    fn(1 if on else 0)


def shadow_stats(reset: bool = True) -> tuple:
    """(l1 scans of the n > 64 default path that tried the fp32 copy of CI, scans it settled, fp64
    re-evaluations of candidates in those) since the last reset; synchronises the device."""
    fn = LIB.qpgpu_debug_shadow_stats
    fn.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    fn.restype = ctypes.c_int
    out = (ctypes.c_uint64 * 3)()
    rc = fn(out, 1 if reset else 0)
    if rc:
        raise QpgpuError(f"qpgpu_debug_shadow_stats: {rc} {LIB.qpgpu_last_error().decode()}")
    return int(out[0]), int(out[1]), int(out[2])


def unc_reasons(status: np.ndarray) -> dict:
    """Counts of each certification reason in status words returned with set_resolve(False)."""
    st = np.asarray(status, dtype=np.int64)
    marked = (st & STATUS_RESOLVE) != 0
    out = {"marked": int(marked.sum())}
    for k, name in enumerate(UNC_REASONS):
        c = int((marked & (((st >> 9) >> k) & 1).astype(bool)).sum())
        if c:
            out[name] = c
    return out


def device_count() -> int:
    return int(LIB.qpgpu_device_count())


def _check(rc: int, what: str):
    if rc != SUCCESS:
        detail = LIB.qpgpu_last_error().decode() if rc in (ERR_HIP, ERR_NO_DEVICE) else ""
        raise QpgpuError(f"{what} failed with code {rc} {detail}".strip())


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


# ----------------------------------------------------------------------------------------------
# problem container
# ----------------------------------------------------------------------------------------------
@dataclass
class Problems:
    """A batch of QPs in the include/qpgpu.h layout (numpy float64, QP-major, row-major)."""

    n: int
    p: int
    m: int
    G: np.ndarray  # (B, n, n)
    g0: np.ndarray  # (B, n)
    CE: np.ndarray  # (B, n, p)
    ce0: np.ndarray  # (B, p)
    CI: np.ndarray  # (B, n, m)
    ci0: np.ndarray  # (B, m)

    @property
    def batch(self) -> int:
        return int(self.G.shape[0])

    def slice(self, b0: int, b1: int) -> "Problems":
        return Problems(self.n, self.p, self.m, self.G[b0:b1].copy(), self.g0[b0:b1].copy(),
                        self.CE[b0:b1].copy(), self.ce0[b0:b1].copy(), self.CI[b0:b1].copy(),
                        self.ci0[b0:b1].copy())

    def arrays(self):
        return (self.G, self.g0, self.CE, self.ce0, self.CI, self.ci0)


@dataclass
class BoxProblems:
    """A batch of bound-constrained QPs, lo <= x <= hi instead of a dense CI
    (qpgpu_solve_batched_box): numpy float64, QP-major."""

    n: int
    p: int
    G: np.ndarray  # (B, n, n)
    g0: np.ndarray  # (B, n)
    CE: np.ndarray  # (B, n, p)
    ce0: np.ndarray  # (B, p)
    hi: np.ndarray  # (B, n)
    lo: np.ndarray  # (B, n)

    @property
    def batch(self) -> int:
        return int(self.G.shape[0])

    @property
    def m(self) -> int:
        return 2 * self.n

    def slice(self, b0: int, b1: int) -> "BoxProblems":
        return BoxProblems(self.n, self.p, self.G[b0:b1].copy(), self.g0[b0:b1].copy(),
                           self.CE[b0:b1].copy(), self.ce0[b0:b1].copy(), self.hi[b0:b1].copy(),
                           self.lo[b0:b1].copy())

    def arrays(self):
        return (self.G, self.g0, self.CE, self.ce0, self.hi, self.lo)

    def to_dense(self) -> Problems:
        """The dense problem the box entry is defined as: CI = [-I, +I], ci0 = [hi; -lo]
        (inequality k < n the upper bound of variable k, n + k its lower bound)."""
        B, n = self.batch, self.n
        eye = np.eye(n)
        CI = np.broadcast_to(np.concatenate([-eye, eye], axis=1), (B, n, 2 * n)).copy()
        ci0 = np.concatenate([np.asarray(self.hi, dtype=np.float64).reshape(B, n),
                              -np.asarray(self.lo, dtype=np.float64).reshape(B, n)], axis=1)
        return Problems(n, self.p, 2 * n, self.G.copy(), self.g0.copy(), self.CE.copy(),
                        self.ce0.copy(), np.ascontiguousarray(CI), np.ascontiguousarray(ci0))


@dataclass
class UnitProblems:
    """A batch of QPs whose Hessian is the identity, min 1/2 x^T x + g0^T x under the constraints
    (qpgpu_solve_batched_unit): no G array.  numpy float64, QP-major."""

    n: int
    p: int
    m: int
    g0: np.ndarray  # (B, n)
    CE: np.ndarray  # (B, n, p)
    ce0: np.ndarray  # (B, p)
    CI: np.ndarray  # (B, n, m)
    ci0: np.ndarray  # (B, m)

    @property
    def batch(self) -> int:
        return int(self.g0.shape[0])

    def slice(self, b0: int, b1: int) -> "UnitProblems":
        return UnitProblems(self.n, self.p, self.m, self.g0[b0:b1].copy(), self.CE[b0:b1].copy(),
                            self.ce0[b0:b1].copy(), self.CI[b0:b1].copy(), self.ci0[b0:b1].copy())

    def arrays(self):
        return (self.g0, self.CE, self.ce0, self.CI, self.ci0)

    def to_dense(self) -> Problems:
        """The dense problem the unit entry is defined as: the same arrays and G = I."""
        G = np.broadcast_to(np.eye(self.n), (self.batch, self.n, self.n)).copy()
        return Problems(self.n, self.p, self.m, np.ascontiguousarray(G), self.g0.copy(), self.CE.copy(),
                        self.ce0.copy(), self.CI.copy(), self.ci0.copy())


def to_tiled64(a: np.ndarray) -> np.ndarray:
    """(B, ...) per-QP blocks -> TILED64 flat array of ceil(B/64) tiles (include/qpgpu.h)."""
    B = a.shape[0]
    E = int(np.prod(a.shape[1:])) if a.ndim > 1 else 1
    BB = (B + 63) // 64 * 64
    pad = np.zeros((BB, E), dtype=np.float64)
    pad[:B] = a.reshape(B, E)
    return np.ascontiguousarray(pad.reshape(BB // 64, 64, E).transpose(0, 2, 1)).reshape(-1)


def from_tiled64(flat: np.ndarray, B: int, shape) -> np.ndarray:
    """Inverse of to_tiled64: returns (B, *shape)."""
    E = int(np.prod(shape)) if len(shape) else 1
    BB = (B + 63) // 64 * 64
    t = np.asarray(flat).reshape(BB // 64, E, 64).transpose(0, 2, 1).reshape(BB, E)
    return np.ascontiguousarray(t[:B]).reshape((B,) + tuple(shape))


def rel_error_per_qp(x, x_ref, f, f_ref, tiny: float = np.finfo(np.float64).tiny, f_scale=None):
    """north_star's parity measure ("primal/objective within 1e-10 relative"), per QP:
    ex_i = ||x_i - xref_i||_inf / max(||xref_i||_inf, tiny), ef_i = |f_i - fref_i| / max(|fref_i|, tiny).
    With f_scale (per QP, objective_term_scale()), ef_i is relative to max(|fref_i|, f_scale_i): the
    magnitude of the objective's terms, which is the scale f is determined to when its two terms
    cancel.  Entries that are equal (inf == inf included) or NaN in both count as 0.  Returns the
    arrays (ex, ef) so callers can report max, percentiles and the worst QP."""
    if len(f) == 0:
        return np.zeros(0), np.zeros(0)
    x = np.asarray(x, dtype=np.float64).reshape(len(f), -1)
    xr = np.asarray(x_ref, dtype=np.float64).reshape(len(f_ref), -1)
    f = np.asarray(f, dtype=np.float64)
    fr = np.asarray(f_ref, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = np.abs(x - xr)
        dx[(x == xr) | (np.isnan(x) & np.isnan(xr))] = 0.0
        nx = np.max(np.abs(np.where(np.isnan(xr), 0.0, xr)), axis=1) if xr.shape[1] else np.zeros(len(xr))
        ex = (np.max(dx, axis=1) if xr.shape[1] else np.zeros(len(xr))) / np.maximum(nx, tiny)
        df = np.abs(f - fr)
        df[(f == fr) | (np.isnan(f) & np.isnan(fr))] = 0.0
        den = np.maximum(np.abs(np.where(np.isnan(fr), 0.0, fr)), tiny)
        if f_scale is not None:
            den = np.maximum(den, np.where(np.isfinite(f_scale), f_scale, 0.0))
        ef = df / den
    ex[np.isnan(ex)] = np.inf  # one side NaN only
    ef[np.isnan(ef)] = np.inf
    return ex, ef


def objective_term_scale(G, g0, x):
    """Per QP, 0.5 |x^T G x| + |g0^T x|: the magnitudes of the two terms whose sum is the objective
    f = 0.5 x^T G x + g0^T x (G the original matrix, x the reference solution).  When they cancel,
    f itself is only determined to ~eps times this scale (the reference's own rounding), so the
    objective's relative error is measured against max(|f|, this)."""
    G = np.asarray(G, dtype=np.float64)
    if G.shape[0] == 0:
        return np.zeros(0)
    x = np.asarray(x, dtype=np.float64).reshape(G.shape[0], -1)
    g0 = np.asarray(g0, dtype=np.float64).reshape(G.shape[0], -1)
    with np.errstate(invalid="ignore", over="ignore"):
        return 0.5 * np.abs(np.einsum("bi,bij,bj->b", x, G, x)) + np.abs(np.einsum("bi,bi->b", g0, x))


def algorithmic_bytes_per_qp(n: int, p: int, m: int) -> int:
    """read G, g0, CE, ce0, CI, ci0; write x and f (status excluded)."""
    return 8 * (n * n + n + n * p + p + n * m + m) + 8 * (n + 1)


def algorithmic_bytes_per_qp_box(n: int, p: int) -> int:
    """The same count for the box entry: read G, g0, CE, ce0, hi, lo; write x and f."""
    return 8 * (n * n + n + n * p + p + 2 * n + n + 1)


def algorithmic_bytes_per_qp_unit(n: int, p: int, m: int) -> int:
    """The same count for the unit entry: read g0, CE, ce0, CI, ci0 (no G); write x and f."""
    return 8 * (n + n * p + p + n * m + m) + 8 * (n + 1)


# ----------------------------------------------------------------------------------------------
# host-pointer solve (numpy in, numpy out) — copies through the C-ABI's host entry point
# ----------------------------------------------------------------------------------------------
def _host_call(d, arrs, outs, devices):
    """qpgpu_solve_batched_host, or qpgpu_solve_batched_multi over `devices` (device ids)."""
    if devices is None:
        return LIB.qpgpu_solve_batched_host(ctypes.byref(d), *[_ptr(a) for a in arrs], *[_ptr(o) for o in outs])
    dv = np.ascontiguousarray(devices, dtype=np.int32)
    return LIB.qpgpu_solve_batched_multi(ctypes.byref(d), len(dv), _ptr(dv), *[_ptr(a) for a in arrs],
                                         *[_ptr(o) for o in outs])


def solve_batched_host(pr: Problems, write_factor: bool = False, max_iter: int = 0, family=None,
                       layout=None, exact: bool = False, fast: bool = False, devices=None):
    """Solve every QP of `pr` on the GPU.  Returns (x, f, status, iters).

    With write_factor=True, pr.G is overwritten with each QP's Cholesky factor, as the
    reference overwrites G (QuadProg++.hh:42-45).  layout="tiled64" sends the batch in the
    TILED64 layout (converted here on the host) and converts x / G back.  exact=True keeps the
    reference's operation order for n > 64 as well (QPGPU_FLAG_EXACT); fast=True runs the lane
    kernel's fast build (QPGPU_FLAG_FAST: within 1e-10, not bitwise).  devices=[d0, d1, ...]
    splits the batch into contiguous shards over those GPUs (qpgpu_solve_batched_multi)."""
    B, n, p, m = pr.batch, pr.n, pr.p, pr.m
    xflags = FAMILY_FLAGS[family] | (FLAG_EXACT if exact else 0) | (FLAG_FAST if fast else 0)
    if LAYOUTS[layout] == LAYOUT_TILED64:
        arrs = [to_tiled64(np.asarray(a, dtype=np.float64)) for a in pr.arrays()]
        xt = np.zeros((B + 63) // 64 * 64 * n, dtype=np.float64)
        f = np.zeros(B, dtype=np.float64)
        st = np.zeros(B, dtype=np.int32)
        it = np.zeros(B, dtype=np.int32)
        d = ProblemDesc(n, p, m, max_iter, B,
                        (FLAG_WRITE_FACTOR if write_factor else 0) | xflags, LAYOUT_TILED64)
        rc = _host_call(d, arrs, (xt, f, st, it), devices)
        _check(rc, "qpgpu_solve_batched_host")
        if write_factor:
            pr.G[...] = from_tiled64(arrs[0], B, (n, n))
        return from_tiled64(xt, B, (n,)), f, st, it
    arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in pr.arrays()]
    if write_factor:
        if not (pr.G.flags.c_contiguous and pr.G.dtype == np.float64):
            raise ValueError("write_factor needs a C-contiguous float64 G")
        arrs[0] = pr.G
    x = np.zeros((B, n), dtype=np.float64)
    f = np.zeros(B, dtype=np.float64)
    st = np.zeros(B, dtype=np.int32)
    it = np.zeros(B, dtype=np.int32)
    d = ProblemDesc(n, p, m, max_iter, B, (FLAG_WRITE_FACTOR if write_factor else 0) | xflags, 0)
    rc = _host_call(d, arrs, (x, f, st, it), devices)
    _check(rc, "qpgpu_solve_batched_host")
    return x, f, st, it


# ----------------------------------------------------------------------------------------------
# device-pointer solve (torch tensors already resident in HBM)
# ----------------------------------------------------------------------------------------------
class _DeviceBatchBase:
    """What DeviceBatch and DeviceBoxBatch share: the device tensors, the prebuilt ctypes arguments
    and the results.  A subclass names its six input attributes (_INPUTS: the order of its
    problem container's arrays() and of the C entries' arguments) and its C entries (solve, solve
    with multipliers, KKT check)."""

    _INPUTS = ()
    _ENTRY = _ENTRY_DUAL = _ENTRY_KKT = _ENTRY_VJP = _ENTRY_JVP = None
    _JVP_TANGENTS = ()  # the inputs the forward-mode entry takes a tangent of, in its C entry's order
    _VJP_INPUTS = ()   # the inputs the backward step reads, in its C entry's order
    _VJP_OUTPUTS = ()  # its six gradients, in its C entry's order

    def __init__(self, pr, device, with_iters: bool = True, layout=None):
        import torch

        self.n, self.p, self.m, self.batch = pr.n, pr.p, pr.m, pr.batch
        self.layout = LAYOUTS[layout]
        conv = to_tiled64 if self.layout == LAYOUT_TILED64 else (lambda a: a)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(conv(np.asarray(a, dtype=np.float64)))).to(device)
        for name, a in zip(self._INPUTS, pr.arrays()):
            setattr(self, name, t(a))
        rows = (self.batch + 63) // 64 * 64 if self.layout == LAYOUT_TILED64 else self.batch
        self.x = torch.zeros((rows, self.n), dtype=torch.float64, device=device)
        self.f = torch.zeros(self.batch, dtype=torch.float64, device=device)
        self.status = torch.zeros(self.batch, dtype=torch.int32, device=device)
        self.iters = torch.zeros(self.batch, dtype=torch.int32, device=device) if with_iters else None

    def _args(self, stream, max_iter, flags, extra=()):
        """(descriptor, ctypes arguments) of a C entry: the inputs, the four outputs, the entry's
        `extra` output tensors, the stream."""
        d = ProblemDesc(self.n, self.p, self.m, max_iter, self.batch, flags, self.layout)
        vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        tensors = [getattr(self, k) for k in self._INPUTS] + [self.x, self.f, self.status, self.iters]
        return d, (ctypes.byref(d), *[vp(t) for t in tensors], *[vp(t) for t in extra],
                   ctypes.c_void_p(stream.cuda_stream))

    def _solve(self, stream, max_iter, flags, dual_out=None):
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.x.device)
        entry = self._ENTRY if dual_out is None else self._ENTRY_DUAL
        _, args = self._args(stream, max_iter, flags, dual_out or ())
        _check(getattr(LIB, entry)(*args), entry)

    def _launcher(self, stream, max_iter, flags):
        d, args = self._args(stream, max_iter, flags)
        fn, entry = getattr(LIB, self._ENTRY), self._ENTRY

        def launch():
            rc = fn(*args)
            if rc != SUCCESS:
                _check(rc, entry)

        launch._keep = (d, self)
        return launch

    def kkt_residuals(self, u, r=None, status=True, stream=None, x=None):
        """Enqueue the KKT check (qpgpu_kkt_residuals / _box, include/qpgpu.h) of this batch's
        resident inputs at (x, u) on `stream` (default current): no host round trip, so it can
        follow a dual solve on the same stream.  u: p + m float64 per QP in this batch's layout (a
        dual solve's dual_out[0]; may be None when p + m == 0); x: default this batch's own.
        status=True masks by this batch's status (a non-OK QP's block is all NaN), None or False
        evaluates every QP, a tensor is used as given.  Returns r, the (rows, 8) float64 device
        tensor written (TILED64: tiles of [8][64] as x's; kkt_rows() decodes a host copy)."""
        import torch

        x = self.x if x is None else x
        if stream is None:
            stream = torch.cuda.current_stream(x.device)
        if r is None:
            r = torch.empty((x.numel() // self.n, KKT_NRES), dtype=torch.float64, device=x.device)
        st = self.status if status is True else (None if status is None or status is False else status)
        d = ProblemDesc(self.n, self.p, self.m, 0, self.batch, 0, self.layout)
        vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        tensors = [getattr(self, k) for k in self._INPUTS] + [x, u, st, r]
        _check(getattr(LIB, self._ENTRY_KKT)(ctypes.byref(d), *[vp(t) for t in tensors],
                                             ctypes.c_void_p(stream.cuda_stream)), self._ENTRY_KKT)
        return r

    def _vjp_shape(self, name):
        n, p, m = self.n, self.p, self.m
        return {"dG": (n, n), "dg0": (n,), "dCE": (n, p), "dce0": (p,), "dCI": (n, m), "dci0": (m,),
                "dhi": (n,), "dlo": (n,)}[name]

    def _vjp_elems(self, name):
        return math.prod(self._vjp_shape(name))

    def _sens_call(self, entry, names, shape, outs, status, stream, x):
        """What vjp() and jvp() share: x and stream by default, the outputs `names` of `entry` as
        `outs` selects them (a tensor, or True for a new one of shape(name, rows)), the status
        selection, the descriptor.  Returns (x, stream, outs, st, d, vp), vp turning a tensor or
        None into a ctypes argument."""
        import torch

        x = self.x if x is None else x
        if stream is None:
            stream = torch.cuda.current_stream(x.device)
        rows = x.numel() // self.n
        outs = dict.fromkeys(names, True) if outs is None else dict(outs)
        for k in outs:
            if k not in names:
                raise ValueError(f"{k!r} is no output of {entry}: {names}")
            if outs[k] is True:
                outs[k] = torch.empty(shape(k, rows), dtype=torch.float64, device=x.device)
        st = self.status if status is True else (None if status is None or status is False else status)
        d = ProblemDesc(self.n, self.p, self.m, 0, self.batch, 0, self.layout)
        vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        return x, stream, outs, st, d, vp

    def _rows(self, t, shape):
        """A host copy of a device array of one `shape` block per QP as numpy (batch, *shape),
        whatever the layout."""
        h = t.cpu().numpy().reshape(-1)
        if self.layout == LAYOUT_TILED64:
            return from_tiled64(h, self.batch, shape)
        return h[:self.batch * math.prod(shape)].reshape((self.batch,) + shape)

    def vjp(self, u, gx, outs=None, status=True, stream=None, x=None, slots=VJP_SLOTS, workspace=None,
            gu=None, gf=None):
        """Enqueue the backward step (qpgpu_vjp / qpgpu_vjp_box, include/qpgpu.h) of this batch's
        resident inputs at (x, u) for gx = dl/dx on `stream` (default current): no host round
        trip, so it can follow a dual solve on the same stream.  u as kkt_residuals() takes it; gx:
        n float64 per QP in the layout of x; x: default this batch's own.  status=True masks by
        this batch's status (a non-OK QP's gradients are +0.0), None or False evaluates every QP, a
        tensor is used as given.  outs: None computes all six gradients into new tensors; otherwise
        a dict from output name (dG, dg0, dCE, dce0 and dCI, dci0 or dhi, dlo) to the tensor to
        write, or True to allocate it: an output that is not named is passed as NULL and not
        computed.  Returns the dict of the tensors written, each (rows, E) in this batch's layout
        (vjp_rows() decodes host copies).  For n > 64 the call goes to qpgpu_vjp_ws /
        qpgpu_vjp_box_ws with `workspace` (a uint8 tensor; default: a new one of min(batch, slots)
        slots, which the results do not depend on); for n <= 64 both are ignored.  gu (dl/du, laid out
        like u) and gf (dl/df, one float64 per QP in either layout): with either given the call
        goes to qpgpu_vjp_full / qpgpu_vjp_box_full, the backward step of a loss l(x, u, f)."""
        import torch

        x, stream, outs, st, d, vp = self._sens_call(
            self._ENTRY_VJP, self._VJP_OUTPUTS, lambda k, rows: (rows, self._vjp_elems(k)), outs, status, stream, x)
        tensors = [getattr(self, k) for k in self._VJP_INPUTS] + [x, u, st, gx] + [outs.get(k) for k in self._VJP_OUTPUTS]
        full = gu is not None or gf is not None
        if full:
            k = len(self._VJP_INPUTS) + 4
            tensors[k:k] = [gu, gf]
        if self.n <= VJP_ON_CHIP_N:
            if full:
                entry = self._ENTRY_VJP + "_full"
                _check(getattr(LIB, entry)(ctypes.byref(d), *[vp(t) for t in tensors], None, 0,
                                           ctypes.c_void_p(stream.cuda_stream)), entry)
                return outs
            _check(getattr(LIB, self._ENTRY_VJP)(ctypes.byref(d), *[vp(t) for t in tensors],
                                                 ctypes.c_void_p(stream.cuda_stream)), self._ENTRY_VJP)
            return outs
        entry = self._ENTRY_VJP + ("_full" if full else "_ws")
        if workspace is None:
            with torch.cuda.stream(stream):
                workspace = _vjp_workspace(self.n, self.p, self.m, self.batch, slots, x.device)
        _check(getattr(LIB, entry)(ctypes.byref(d), *[vp(t) for t in tensors], vp(workspace), workspace.numel(),
                                   ctypes.c_void_p(stream.cuda_stream)), entry)
        return outs

    def vjp_rows(self, outs):
        """A vjp() result as numpy arrays shaped like the inputs ((batch, n, n) for dG, ...),
        whatever the layout."""
        return {k: self._rows(t, self._vjp_shape(k)) for k, t in outs.items()}

    def jvp(self, u, tangents, outs=None, status=True, stream=None, x=None):
        """Enqueue the forward-mode sensitivities (qpgpu_jvp / qpgpu_jvp_box, include/qpgpu.h) of this
        batch's resident inputs at (x, u) on `stream` (default current): no host round trip, so it
        can follow a dual solve on the same stream.  u, status and x as vjp() takes them.  tangents: a
        dict from input name (G, g0, CE, ce0 and CI, ci0 or hi, lo) to a float64 device tensor in this
        batch's layout, shaped like that input; a missing name (or None) is passed as NULL, a zero
        tangent.  outs: None computes tx, tu and tf into new tensors; otherwise a dict from output
        name to the tensor to write, or True to allocate it: an output that is not named is passed
        as NULL and not computed.  Returns the dict of the tensors written: tx (rows, n) and tu
        (rows, p + m) in this batch's layout, tf (batch,) (jvp_rows() decodes host copies)."""
        for k in tangents:
            if k not in self._JVP_TANGENTS:
                raise ValueError(f"{k!r} is no tangent of {self._ENTRY_JVP}: {self._JVP_TANGENTS}")
        shape = lambda k, rows: {"tx": (rows, self.n), "tu": (rows, self.p + self.m), "tf": (self.batch,)}[k]
        x, stream, outs, st, d, vp = self._sens_call(self._ENTRY_JVP, JVP_OUTPUTS, shape, outs, status, stream, x)
        tensors = ([getattr(self, k) for k in self._VJP_INPUTS] + [x, u, st] + [tangents.get(k) for k in self._JVP_TANGENTS]
                   + [outs.get(k) for k in JVP_OUTPUTS])
        _check(getattr(LIB, self._ENTRY_JVP)(ctypes.byref(d), *[vp(t) for t in tensors],
                                             ctypes.c_void_p(stream.cuda_stream)), self._ENTRY_JVP)
        return outs

    def jvp_rows(self, outs):
        """A jvp() result as numpy arrays: tx (batch, n), tu (batch, p + m), tf (batch,), whatever the
        layout."""
        shapes = {"tx": (self.n,), "tu": (self.p + self.m,)}
        return {k: t.cpu().numpy().reshape(-1)[:self.batch].copy() if k == "tf" else self._rows(t, shapes[k])
                for k, t in outs.items()}

    def jvp_many(self, u, tangents, ntan, outs=None, status=True, stream=None, x=None):
        """jvp() along ntan directions per QP in one launch (qpgpu_jvp_many / qpgpu_jvp_box_many,
        include/qpgpu.h): the factorisations are shared by the directions, and direction k has the bits
        of jvp() on slice k.  A tangent of an input with E elements per QP has ntan * E, direction-major
        (QP-major: (batch, ntan, ...)), in this batch's layout; so have the outputs: tx (rows, ntan * n),
        tu (rows, ntan * (p + m)), tf (rows, ntan) (jvp_many_rows() decodes host copies).  Everything else
        as jvp() takes it."""
        for k in tangents:
            if k not in self._JVP_TANGENTS:
                raise ValueError(f"{k!r} is no tangent of {self._ENTRY_JVP}_many: {self._JVP_TANGENTS}")
        K = int(ntan)
        shape = lambda k, rows: (rows, K * {"tx": self.n, "tu": self.p + self.m, "tf": 1}[k])
        entry = self._ENTRY_JVP + "_many"
        x, stream, outs, st, d, vp = self._sens_call(entry, JVP_OUTPUTS, shape, outs, status, stream, x)
        tensors = ([getattr(self, k) for k in self._VJP_INPUTS] + [x, u, st] + [tangents.get(k) for k in self._JVP_TANGENTS]
                   + [outs.get(k) for k in JVP_OUTPUTS])
        _check(getattr(LIB, entry)(ctypes.byref(d), K, *[vp(t) for t in tensors],
                                   ctypes.c_void_p(stream.cuda_stream)), entry)
        return outs

    def jvp_many_rows(self, outs, ntan=None):
        """A jvp_many() result as numpy arrays: tx (batch, ntan, n), tu (batch, ntan, p + m), tf
        (batch, ntan), whatever the layout.  ntan: by default what the tensors' second dimension
        says (jvp_many() shapes them (rows, ntan * E))."""
        per = {"tx": self.n, "tu": self.p + self.m, "tf": 1}
        rows = {}
        for k, t in outs.items():
            K = int(ntan) if ntan is not None else t.shape[1] // max(per[k], 1)
            rows[k] = self._rows(t, (K,) if k == "tf" else (K, per[k]))
        return rows

    def kkt_rows(self, r):
        """A kkt_residuals() result as numpy (batch, 8), whatever the layout."""
        return self._rows(r, (KKT_NRES,))

    def results(self):
        it = None if self.iters is None else self.iters.cpu().numpy()
        x = self.x.cpu().numpy()
        if self.layout == LAYOUT_TILED64:
            x = from_tiled64(x.reshape(-1), self.batch, (self.n,))
        return x, self.f.cpu().numpy(), self.status.cpu().numpy(), it


class DeviceBatch(_DeviceBatchBase):
    """Device-resident inputs/outputs for repeated solves (torch tensors on one GPU)."""

    _INPUTS = ("G", "g0", "CE", "ce0", "CI", "ci0")
    _ENTRY, _ENTRY_DUAL = "qpgpu_solve_batched", "qpgpu_solve_batched_dual"
    _ENTRY_KKT = "qpgpu_kkt_residuals"
    _ENTRY_VJP = "qpgpu_vjp"
    _VJP_INPUTS = ("G", "CE", "CI")
    _VJP_OUTPUTS = ("dG", "dg0", "dCE", "dce0", "dCI", "dci0")
    _ENTRY_JVP = "qpgpu_jvp"
    _JVP_TANGENTS = ("G", "g0", "CE", "ce0", "CI", "ci0")

    def __init__(self, pr: Problems, device, with_iters: bool = True, layout=None):
        super().__init__(pr, device, with_iters, layout)

    def solve(self, stream=None, max_iter: int = 0, write_factor: bool = False, family=None,
              eq_out=None, exact: bool = False, fast: bool = False, dual_out=None):
        """Enqueue one batched solve on `stream` (a torch.cuda.Stream, default current).
        eq_out=(x_eq, f_eq, status_eq) tensors also receive the m = 0 answer
        (qpgpu_solve_batched_eq).  dual_out=(u, nact) tensors receive the multipliers, p + m
        float64 per QP in this batch's layout, and the int32 active-inequality counts
        (qpgpu_solve_batched_dual: reference operation order always; either may be None where
        the C entry takes NULL).  eq_out and dual_out are separate entries: not both."""
        flags = ((FLAG_WRITE_FACTOR if write_factor else 0) | FAMILY_FLAGS[family]
                 | (FLAG_EXACT if exact else 0) | (FLAG_FAST if fast else 0))
        if eq_out is None:
            return self._solve(stream, max_iter, flags, dual_out)
        if dual_out is not None:
            raise ValueError("eq_out and dual_out are separate entry points: pass one")
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.x.device)
        _, args = self._args(stream, max_iter, flags, eq_out)
        _check(LIB.qpgpu_solve_batched_eq(*args), "qpgpu_solve_batched")

    def launcher(self, stream, max_iter: int = 0, family=None, exact: bool = False, fast: bool = False):
        """A zero-argument callable that enqueues this batch's solve on `stream` with every ctypes
        argument prebuilt (for tight launch loops: ~2 us of host time per launch)."""
        return self._launcher(stream, max_iter,
                              FAMILY_FLAGS[family] | (FLAG_EXACT if exact else 0) | (FLAG_FAST if fast else 0))


class DeviceBoxBatch(_DeviceBatchBase):
    """DeviceBatch for bound-constrained QPs (qpgpu_solve_batched_box): hi and lo, n float64 per
    QP in the layout of x, instead of CI and ci0."""

    _INPUTS = ("G", "g0", "CE", "ce0", "hi", "lo")
    _ENTRY, _ENTRY_DUAL = "qpgpu_solve_batched_box", "qpgpu_solve_batched_box_dual"
    _ENTRY_KKT = "qpgpu_kkt_residuals_box"
    _ENTRY_VJP = "qpgpu_vjp_box"
    _VJP_INPUTS = ("G", "CE")
    _VJP_OUTPUTS = ("dG", "dg0", "dCE", "dce0", "dhi", "dlo")
    _ENTRY_JVP = "qpgpu_jvp_box"
    _JVP_TANGENTS = ("G", "g0", "CE", "ce0", "hi", "lo")

    def __init__(self, bp: BoxProblems, device, with_iters: bool = True, layout=None):
        super().__init__(bp, device, with_iters, layout)

    def solve(self, stream=None, max_iter: int = 0, write_factor: bool = False, family=None,
              flags: int = 0, dual_out=None):
        """Enqueue one batched box solve on `stream` (a torch.cuda.Stream, default current);
        `flags` are OR-ed in as given (tests pass QPGPU_FLAG_FAST to see it refused).
        dual_out=(u, nact) tensors receive the multipliers, p + 2n float64 per QP in the layout of
        x, and the active-set sizes, int32 (qpgpu_solve_batched_box_dual; either may be None where
        the C entry takes NULL)."""
        self._solve(stream, max_iter, (FLAG_WRITE_FACTOR if write_factor else 0) | FAMILY_FLAGS[family] | flags,
                    dual_out)

    def launcher(self, stream, max_iter: int = 0, family=None):
        """A zero-argument callable that enqueues this batch's solve on `stream` with every ctypes
        argument prebuilt (see DeviceBatch.launcher)."""
        return self._launcher(stream, max_iter, FAMILY_FLAGS[family])


class DeviceUnitBatch(_DeviceBatchBase):
    """DeviceBatch for QPs with the identity as Hessian (qpgpu_solve_batched_unit): no G tensor."""

    _INPUTS = ("g0", "CE", "ce0", "CI", "ci0")
    _ENTRY = "qpgpu_solve_batched_unit"

    def __init__(self, up: UnitProblems, device, with_iters: bool = True, layout=None):
        super().__init__(up, device, with_iters, layout)
        self.x_eq = self.f_eq = self.status_eq = None

    def _eq_tensors(self):
        import torch

        if self.x_eq is None:
            self.x_eq = torch.zeros_like(self.x)
            self.f_eq = torch.zeros_like(self.f)
            self.status_eq = torch.zeros_like(self.status)
        return (self.x_eq, self.f_eq, self.status_eq)

    def solve(self, stream=None, max_iter: int = 0, family=None, eq: bool = False, flags: int = 0):
        """Enqueue one batched unit solve on `stream` (a torch.cuda.Stream, default current).
        eq=True also writes the m = 0 answers into self.x_eq, self.f_eq, self.status_eq (allocated
        at first use; eq_results() reads them).  `flags` are OR-ed in as given (tests pass
        QPGPU_FLAG_FAST to see it refused)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.x.device)
        extra = self._eq_tensors() if eq else (None, None, None)
        _, args = self._args(stream, max_iter, FAMILY_FLAGS[family] | flags, extra)
        _check(LIB.qpgpu_solve_batched_unit(*args), self._ENTRY)

    def launcher(self, stream, max_iter: int = 0, family=None, eq: bool = False):
        """A zero-argument callable that enqueues this batch's solve on `stream` with every ctypes
        argument prebuilt (see DeviceBatch.launcher)."""
        extra = self._eq_tensors() if eq else (None, None, None)
        d, args = self._args(stream, max_iter, FAMILY_FLAGS[family], extra)
        fn, entry = LIB.qpgpu_solve_batched_unit, self._ENTRY

        def launch():
            rc = fn(*args)
            if rc != SUCCESS:
                _check(rc, entry)

        launch._keep = (d, self)
        return launch

    def eq_results(self):
        """(x_eq, f_eq, status_eq) of the last solve(eq=True) as numpy, x_eq (B, n) whatever the layout."""
        x = self.x_eq.cpu().numpy()
        if self.layout == LAYOUT_TILED64:
            x = from_tiled64(x.reshape(-1), self.batch, (self.n,))
        return x, self.f_eq.cpu().numpy(), self.status_eq.cpu().numpy()


def solve_batched_unit(up: UnitProblems, family=None, layout=None, max_iter: int = 0, eq: bool = False,
                       device="cuda:0"):
    """Solve every QP of `up` on the GPU through qpgpu_solve_batched_unit: (x, f, status, iters) as
    numpy, x of shape (B, n) whatever the device layout; with eq=True followed by (x_eq, f_eq,
    status_eq), the answers of the same QPs without their inequalities."""
    import torch

    db = DeviceUnitBatch(up, device, layout=layout)
    db.solve(max_iter=max_iter, family=family, eq=eq)
    torch.cuda.synchronize(db.x.device)
    return db.results() + (db.eq_results() if eq else ())


def _solve_with_multipliers(db, pr, family, max_iter, write_factor):
    """The staging and unpacking solve_batched_dual and solve_batched_box_dual share: u and nact
    tensors for `db` (the device batch of `pr`), the solve, and every result as numpy in QP-major
    order; with write_factor, pr.G receives the factors."""
    import torch

    device = db.x.device
    B, E = pr.batch, pr.p + pr.m
    rows = (B + 63) // 64 * 64 if db.layout == LAYOUT_TILED64 else B
    u = torch.zeros((rows, E), dtype=torch.float64, device=device)
    nact = torch.zeros(B, dtype=torch.int32, device=device)
    db.solve(max_iter=max_iter, write_factor=write_factor, family=family, dual_out=(u, nact))
    torch.cuda.synchronize(device)
    x, f, st, it = db.results()
    uh = u.cpu().numpy()
    if db.layout == LAYOUT_TILED64:
        uh = from_tiled64(uh.reshape(-1), B, (E,))
    if write_factor:
        Gh = db.G.cpu().numpy()
        pr.G[...] = from_tiled64(Gh.reshape(-1), B, (pr.n, pr.n)) if db.layout == LAYOUT_TILED64 else Gh
    return x, f, st, it, uh.reshape(B, E), nact.cpu().numpy()


def solve_batched_dual(pr: Problems, family=None, layout=None, max_iter: int = 0,
                       write_factor: bool = False, device="cuda:0"):
    """Solve every QP of `pr` on the GPU and return the multipliers too:
    (x, f, status, iters, u, nact) as numpy, u of shape (B, p + m) in QP-major order whatever
    the device layout — u[:, :p] the equalities', u[:, p:] the inequalities' (include/qpgpu.h,
    qpgpu_solve_batched_dual).  Stages `pr` through device tensors; with write_factor=True,
    pr.G receives each QP's Cholesky factor."""
    return _solve_with_multipliers(DeviceBatch(pr, device, layout=layout), pr, family, max_iter, write_factor)


def solve_batched_box(bp: BoxProblems, family=None, layout=None, max_iter: int = 0, device="cuda:0"):
    """Solve every QP of `bp` on the GPU through qpgpu_solve_batched_box: (x, f, status, iters)
    as numpy, x of shape (B, n) whatever the device layout."""
    import torch

    db = DeviceBoxBatch(bp, device, layout=layout)
    db.solve(max_iter=max_iter, family=family)
    torch.cuda.synchronize(db.x.device)
    return db.results()


def solve_batched_box_dual(bp: BoxProblems, family=None, layout=None, max_iter: int = 0,
                           write_factor: bool = False, device="cuda:0"):
    """Solve every QP of `bp` on the GPU through qpgpu_solve_batched_box_dual:
    (x, f, status, iters, u, nact) as numpy, u of shape (B, p + 2n) in QP-major order whatever the
    device layout — u[:, :p] the equalities', u[:, p:p+n] the upper bounds', u[:, p+n:] the lower
    bounds' (include/qpgpu.h).  With write_factor=True, bp.G receives each QP's Cholesky factor."""
    return _solve_with_multipliers(DeviceBoxBatch(bp, device, layout=layout), bp, family, max_iter, write_factor)


def kkt_residuals(pr, x, u, status=None, layout=None, device="cuda:0"):
    """The KKT residuals of (x, u) for every QP of `pr` (Problems: qpgpu_kkt_residuals; BoxProblems:
    qpgpu_kkt_residuals_box), computed on the GPU: a (B, 8) float64 array indexed by KKT_STAT ...
    KKT_NNZ (include/qpgpu.h).  x is (B, n), u is (B, p + m) in QP-major order (as
    solve_batched_dual / solve_batched_box_dual return them; may be None when p + m == 0); with
    `status` (B int32) a QP that is not QP_OK gets an all-NaN row.  layout="tiled64" runs the
    TILED64 form of the kernel (the arrays are converted here on the host)."""
    import torch

    db = (DeviceBoxBatch if isinstance(pr, BoxProblems) else DeviceBatch)(pr, device, with_iters=False, layout=layout)
    B, E = pr.batch, pr.p + pr.m
    conv = to_tiled64 if db.layout == LAYOUT_TILED64 else (lambda a: a)
    up = lambda a, cols: torch.from_numpy(np.array(
        conv(np.asarray(a, dtype=np.float64).reshape(B, cols)), dtype=np.float64, order="C")).to(device)
    xd = up(x, pr.n)
    ud = up(u, E) if E > 0 else None
    sd = None if status is None else torch.from_numpy(np.array(status, dtype=np.int32, order="C")).to(device)
    r = db.kkt_residuals(ud, status=sd, x=xd)
    torch.cuda.synchronize(r.device)
    return db.kkt_rows(r)


def vjp(pr, x, u, gx, status=None, layout=None, device="cuda:0", outs=None, slots=VJP_SLOTS, gu=None, gf=None):
    """The gradients of l with respect to the data of every QP of `pr` (Problems: qpgpu_vjp;
    BoxProblems: qpgpu_vjp_box) at the primal-dual pair (x, u) for gx = dl/dx, computed on the GPU:
    a dict of float64 arrays shaped like the inputs — dG (B, n, n), dg0 (B, n), dCE (B, n, p),
    dce0 (B, p) and dCI (B, n, m), dci0 (B, m), or dhi, dlo (B, n) for bounds (include/qpgpu.h).
    x and gx are (B, n), u is (B, p + m) in QP-major order (may be None when p + m == 0); with
    `status` (B int32) a QP that is not QP_OK gets +0.0 everywhere.  outs: the names to compute
    (default all six).  layout="tiled64" runs the TILED64 form (converted here on the host).  For
    n > 64 the entries are qpgpu_vjp_ws / qpgpu_vjp_box_ws with a workspace of min(B, slots) slots.
    gu (B, p + m) = dl/du and gf (B,) = dl/df: with either given the entries are qpgpu_vjp_full /
    qpgpu_vjp_box_full, the backward step of a loss l(x, u, f)."""
    import torch

    db = (DeviceBoxBatch if isinstance(pr, BoxProblems) else DeviceBatch)(pr, device, with_iters=False, layout=layout)
    B, E = pr.batch, pr.p + pr.m
    conv = to_tiled64 if db.layout == LAYOUT_TILED64 else (lambda a: a)
    up = lambda a, cols: torch.from_numpy(np.array(
        conv(np.asarray(a, dtype=np.float64).reshape(B, cols)), dtype=np.float64, order="C")).to(device)
    xd, gd = up(x, pr.n), up(gx, pr.n)
    ud = up(u, E) if E > 0 else None
    sd = None if status is None else torch.from_numpy(np.array(status, dtype=np.int32, order="C")).to(device)
    gud = None if gu is None else up(gu, E)
    gfd = None if gf is None else torch.from_numpy(np.array(gf, dtype=np.float64, order="C").reshape(B)).to(device)
    res = db.vjp(ud, gd, outs=None if outs is None else dict.fromkeys(outs, True), status=sd, x=xd, slots=slots,
                 gu=gud, gf=gfd)
    torch.cuda.synchronize(xd.device)
    return db.vjp_rows(res)


def jvp(pr, x, u, tangents, status=None, layout=None, device="cuda:0", outs=None):
    """The forward-mode sensitivities of every QP of `pr` (Problems: qpgpu_jvp; BoxProblems:
    qpgpu_jvp_box) at the primal-dual pair (x, u), computed on the GPU: a dict of float64 arrays tx
    (B, n), tu (B, p + m) and tf (B,) (include/qpgpu.h).  tangents: a dict from input name (G, g0, CE,
    ce0 and CI, ci0, or hi, lo for bounds) to an array shaped like that input; a missing name (or None)
    is a NULL tangent.  x is (B, n), u is (B, p + m) in QP-major order (may be None when
    p + m == 0); with `status` (B int32) a QP that is not QP_OK gets +0.0 everywhere.  outs: the names
    to compute (default all three).  layout="tiled64" runs the TILED64 form (converted here on the
    host)."""
    import torch

    db = (DeviceBoxBatch if isinstance(pr, BoxProblems) else DeviceBatch)(pr, device, with_iters=False, layout=layout)
    B, E = pr.batch, pr.p + pr.m
    conv = to_tiled64 if db.layout == LAYOUT_TILED64 else (lambda a: a)
    up = lambda a, cols: torch.from_numpy(np.array(
        conv(np.asarray(a, dtype=np.float64).reshape(B, cols)), dtype=np.float64, order="C")).to(device)
    xd = up(x, pr.n)
    ud = up(u, E) if E > 0 else None
    sd = None if status is None else torch.from_numpy(np.array(status, dtype=np.int32, order="C")).to(device)
    td = {k: up(t, np.asarray(t).size // B) for k, t in tangents.items() if t is not None and np.asarray(t).size}
    res = db.jvp(ud, td, outs=None if outs is None else dict.fromkeys(outs, True), status=sd, x=xd)
    torch.cuda.synchronize(xd.device)
    return db.jvp_rows(res)


def jvp_many(pr, x, u, tangents, status=None, layout=None, device="cuda:0", outs=None, ntan=None):
    """jvp() along K directions per QP in one launch (qpgpu_jvp_many / qpgpu_jvp_box_many): every
    tangent is shaped (B, K, ...), the result is tx (B, K, n), tu (B, K, p + m) and tf (B, K), and
    direction k has the bits of jvp() on slice k.  ntan: K, by default the tangents' second dimension
    (required when no tangent is given)."""
    import torch

    given = {k: np.asarray(t, dtype=np.float64) for k, t in tangents.items() if t is not None}
    if ntan is None:
        if not given:
            raise ValueError("jvp_many without a tangent needs ntan")
        ntan = next(iter(given.values())).shape[1]
    K = int(ntan)
    for k, t in given.items():
        if t.ndim < 2 or t.shape[1] != K:
            raise ValueError(f"the tangent of {k} is not (B, {K}, ...)")
    db = (DeviceBoxBatch if isinstance(pr, BoxProblems) else DeviceBatch)(pr, device, with_iters=False, layout=layout)
    B, E = pr.batch, pr.p + pr.m
    conv = to_tiled64 if db.layout == LAYOUT_TILED64 else (lambda a: a)
    up = lambda a, cols: torch.from_numpy(np.array(
        conv(np.asarray(a, dtype=np.float64).reshape(B, cols)), dtype=np.float64, order="C")).to(device)
    xd = up(x, pr.n)
    ud = up(u, E) if E > 0 else None
    sd = None if status is None else torch.from_numpy(np.array(status, dtype=np.int32, order="C")).to(device)
    td = {k: up(t, t.size // B) for k, t in given.items() if t.size}
    res = db.jvp_many(ud, td, K, outs=None if outs is None else dict.fromkeys(outs, True), status=sd, x=xd)
    torch.cuda.synchronize(xd.device)
    return db.jvp_many_rows(res, K)


def _qp_jvp(box, G, g0, CE, ce0, c5, c6, tangents, many=False):
    import torch

    B, n, p = G.shape[0], G.shape[-1], CE.shape[-1]
    m = 2 * n if box else c5.shape[-1]
    names = ("G", "g0", "CE", "ce0") + (("hi", "lo") if box else ("CI", "ci0"))
    for t in (G, g0, CE, ce0, c5, c6) + tuple(t for t in tangents.values() if t is not None):
        if t.dtype != torch.float64 or not t.is_cuda:
            raise ValueError("qp_jvp takes float64 tensors on the GPU")
    for k in tangents:
        if k not in names:
            raise ValueError(f"{k!r} is no input of the QP: {names}")
    ins = [t.detach().contiguous() for t in (G, g0, CE, ce0, c5, c6)]
    tan = [None if tangents.get(k) is None else tangents[k].detach().contiguous() for k in names]
    K = None
    if many:
        given = [t for t in tan if t is not None]
        if not given or given[0].dim() < 2:
            raise ValueError("qp_jvp_many takes at least one tangent, shaped (B, K, ...)")
        K = int(given[0].shape[1])
    for k, a, t in zip(names, ins, tan):
        want = a.shape if K is None else a.shape[:1] + (K,) + a.shape[1:]
        if t is not None and t.shape != want:
            raise ValueError(f"the tangent of {k} has shape {tuple(t.shape)}, not {tuple(want)}")
    dev = G.device
    x = torch.zeros((B, n), dtype=torch.float64, device=dev)
    f = torch.empty(B, dtype=torch.float64, device=dev)
    st = torch.empty(B, dtype=torch.int32, device=dev)
    u = torch.zeros((B, p + m), dtype=torch.float64, device=dev)
    kdim = () if K is None else (K,)
    tx = torch.empty((B,) + kdim + (n,), dtype=torch.float64, device=dev)
    tu = torch.empty((B,) + kdim + (p + m,), dtype=torch.float64, device=dev)
    tf = torch.empty((B,) + kdim, dtype=torch.float64, device=dev)
    d = ProblemDesc(n, p, m, 0, B, 0, LAYOUT_QP_MAJOR)
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    entry = "qpgpu_solve_batched_box_dual" if box else "qpgpu_solve_batched_dual"
    _check(getattr(LIB, entry)(ctypes.byref(d), *[vp(t) for t in ins], vp(x), vp(f), vp(st), None, vp(u), None,
                               stream), entry)
    entry = ("qpgpu_jvp_box" if box else "qpgpu_jvp") + ("" if K is None else "_many")
    data = (() if K is None else (K,)) + (vp(ins[0]), vp(ins[2])) + (() if box else (vp(ins[4]),))
    _check(getattr(LIB, entry)(ctypes.byref(d), *data, vp(x), vp(u), vp(st), *[vp(t) for t in tan], vp(tx), vp(tu),
                               vp(tf), stream), entry)
    return x, u, f, st, tx, tu, tf


def qp_jvp(G, g0, CE, ce0, CI, ci0, tangents):
    """The batched QP and its forward-mode sensitivities in one call: (x, u, f, status, tx, tu, tf) for
    float64 device tensors shaped as qp_layer takes them and `tangents`, a dict from input name (G, g0,
    CE, ce0, CI, ci0) to a tensor shaped like that input (a missing name: a zero tangent).  A dual
    solve (qpgpu_solve_batched_dual), then qpgpu_jvp, on the current stream with no host round trip.
    tx (B, n), tu (B, p + m) and tf (B,) are +0.0 for a QP whose status is not QP_OK.  Not hooked into
    torch.autograd.forward_ad."""
    return _qp_jvp(False, G, g0, CE, ce0, CI, ci0, tangents)


def qp_jvp_box(G, g0, CE, ce0, hi, lo, tangents):
    """qp_jvp for bounds lo <= x <= hi (tangent names G, g0, CE, ce0, hi, lo): u and tu are
    (B, p + 2n), equalities, upper bounds, lower bounds (qpgpu_solve_batched_box_dual, then qpgpu_jvp_box)."""
    return _qp_jvp(True, G, g0, CE, ce0, hi, lo, tangents)


def qp_jvp_many(G, g0, CE, ce0, CI, ci0, tangents):
    """qp_jvp along K directions per QP: every tangent is shaped (B, K, ...) (at least one is given; a
    missing name: a zero tangent in all K directions).  A dual solve, then qpgpu_jvp_many, on the
    current stream: (x, u, f, status, tx, tu, tf) with tx (B, K, n), tu (B, K, p + m) and tf (B, K);
    direction k has the bits of qp_jvp on slice k."""
    return _qp_jvp(False, G, g0, CE, ce0, CI, ci0, tangents, many=True)


def qp_jvp_box_many(G, g0, CE, ce0, hi, lo, tangents):
    """qp_jvp_many for bounds lo <= x <= hi (tangent names G, g0, CE, ce0, hi, lo), as qp_jvp_box is
    to qp_jvp (qpgpu_solve_batched_box_dual, then qpgpu_jvp_box_many)."""
    return _qp_jvp(True, G, g0, CE, ce0, hi, lo, tangents, many=True)


@functools.lru_cache(maxsize=None)
def _layer_functions():
    """The torch.autograd.Functions behind qp_layer / qp_layer_box and their _full forms, which also
    return u, f and status and take their cotangents (built at first use: torch is
    imported lazily everywhere in this module)."""
    import torch

    def run(box, ctx, G, g0, CE, ce0, c5, c6, full=False):
        B, n, p = G.shape[0], G.shape[-1], CE.shape[-1]
        m = 2 * n if box else c5.shape[-1]
        for t in (G, g0, CE, ce0, c5, c6):
            if t.dtype != torch.float64 or not t.is_cuda:
                raise ValueError("qp_layer takes float64 tensors on the GPU")
        ins = [t.detach().contiguous() for t in (G, g0, CE, ce0, c5, c6)]
        dev = G.device
        x = torch.zeros((B, n), dtype=torch.float64, device=dev)
        f = torch.empty(B, dtype=torch.float64, device=dev)
        st = torch.empty(B, dtype=torch.int32, device=dev)
        u = torch.zeros((B, p + m), dtype=torch.float64, device=dev)
        d = ProblemDesc(n, p, m, 0, B, 0, LAYOUT_QP_MAJOR)
        vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        entry = "qpgpu_solve_batched_box_dual" if box else "qpgpu_solve_batched_dual"
        _check(getattr(LIB, entry)(ctypes.byref(d), *[vp(t) for t in ins], vp(x), vp(f), vp(st), None, vp(u),
                                   None, stream), entry)
        ctx.save_for_backward(ins[0], ins[2], ins[4], x, u, st)
        ctx.shape = (B, n, p, m)
        if full:
            ctx.mark_non_differentiable(st)
            ctx.set_materialize_grads(False)
            return x, u, f, st
        return x

    def back(box, ctx, gx, gu=None, gf=None, full=False):
        G, CE, c5, x, u, st = ctx.saved_tensors
        B, n, p, m = ctx.shape
        need = ctx.needs_input_grad
        sizes = ((B, n, n), (B, n), (B, n, p), (B, p)) + (((B, n), (B, n)) if box else ((B, n, m), (B, m)))
        outs = [torch.empty(sz, dtype=torch.float64, device=G.device) if nd else None for sz, nd in zip(sizes, need)]
        d = ProblemDesc(n, p, m, 0, B, 0, LAYOUT_QP_MAJOR)
        vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
        stream = ctypes.c_void_p(torch.cuda.current_stream(G.device).cuda_stream)
        if full:  # one call to the full entry; an output the loss does not use arrives as None: NULL
            gx = torch.zeros((B, n), dtype=torch.float64, device=G.device) if gx is None else gx.contiguous()
            gu = None if gu is None else gu.contiguous()
            gf = None if gf is None else gf.contiguous()
            ins = (vp(G), vp(CE)) + (() if box else (vp(c5),)) + (vp(x), vp(u), vp(st), vp(gx), vp(gu), vp(gf))
            entry = "qpgpu_vjp_box_full" if box else "qpgpu_vjp_full"
            ws = _vjp_workspace(n, p, m, B, VJP_SLOTS, G.device) if n > VJP_ON_CHIP_N else None
            _check(getattr(LIB, entry)(ctypes.byref(d), *ins, *[vp(t) for t in outs], vp(ws),
                                       0 if ws is None else ws.numel(), stream), entry)
            return tuple(outs)
        gx = gx.contiguous()
        ins = (vp(G), vp(CE)) + (() if box else (vp(c5),)) + (vp(x), vp(u), vp(st), vp(gx))
        entry = "qpgpu_vjp_box" if box else "qpgpu_vjp"
        if n <= VJP_ON_CHIP_N:
            rc = getattr(LIB, entry)(ctypes.byref(d), *ins, *[vp(t) for t in outs], stream)
        else:  # the workspace: torch's caching allocator, on the current stream
            entry += "_ws"
            ws = _vjp_workspace(n, p, m, B, VJP_SLOTS, G.device)
            rc = getattr(LIB, entry)(ctypes.byref(d), *ins, *[vp(t) for t in outs], vp(ws), ws.numel(), stream)
        _check(rc, entry)
        return tuple(outs)

    class QpLayer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, G, g0, CE, ce0, CI, ci0):
            return run(False, ctx, G, g0, CE, ce0, CI, ci0)

        @staticmethod
        def backward(ctx, gx):
            return back(False, ctx, gx)

    class QpLayerBox(torch.autograd.Function):
        @staticmethod
        def forward(ctx, G, g0, CE, ce0, hi, lo):
            return run(True, ctx, G, g0, CE, ce0, hi, lo)

        @staticmethod
        def backward(ctx, gx):
            return back(True, ctx, gx)

    class QpLayerFull(torch.autograd.Function):
        @staticmethod
        def forward(ctx, G, g0, CE, ce0, CI, ci0):
            return run(False, ctx, G, g0, CE, ce0, CI, ci0, full=True)

        @staticmethod
        def backward(ctx, gx, gu, gf, gst):
            return back(False, ctx, gx, gu, gf, full=True)

    class QpLayerBoxFull(torch.autograd.Function):
        @staticmethod
        def forward(ctx, G, g0, CE, ce0, hi, lo):
            return run(True, ctx, G, g0, CE, ce0, hi, lo, full=True)

        @staticmethod
        def backward(ctx, gx, gu, gf, gst):
            return back(True, ctx, gx, gu, gf, full=True)

    return QpLayer, QpLayerBox, QpLayerFull, QpLayerBoxFull


def qp_layer(G, g0, CE, ce0, CI, ci0):
    """The batched QP as a differentiable layer: x* (B, n) of
        min 0.5 x^T G x + g0^T x   s.t.  CE^T x + ce0 = 0,  CI^T x + ci0 >= 0
    for float64 device tensors G (B, n, n), g0 (B, n), CE (B, n, p), ce0 (B, p), CI (B, n, m),
    ci0 (B, m), QP-major.  Forward is qpgpu_solve_batched_dual, backward qpgpu_vjp (n > 64:
    qpgpu_vjp_ws, its workspace from torch's caching allocator) on the current
    stream with no host round trip; an input that does not require grad gets none (its gradient
    is not computed), and no gradient flows through a QP whose status is not QP_OK (+0.0; its x is
    whatever the solve left: zeros for a G that is not positive definite)."""
    return _layer_functions()[0].apply(G, g0, CE, ce0, CI, ci0)


def qp_layer_box(G, g0, CE, ce0, hi, lo):
    """qp_layer for bounds lo <= x <= hi (hi, lo: (B, n)): qpgpu_solve_batched_box_dual forward,
    qpgpu_vjp_box backward."""
    return _layer_functions()[1].apply(G, g0, CE, ce0, hi, lo)


def qp_layer_full(G, g0, CE, ce0, CI, ci0):
    """qp_layer returning everything the dual solve does, (x, u, f, status): x (B, n), the
    multipliers u (B, p + m), the optimal values f (B,) and the int32 status (B,), which carries no
    gradient.  A loss may use any of x, u and f: backward is one call to qpgpu_vjp_full on the
    current stream (n > 64: with a workspace from torch's caching allocator), an output the loss
    does not use passed as NULL, so a graph that uses only x gets the bits of qp_layer's gradients.
    No gradient flows through a QP whose status is not QP_OK, nor through the multiplier of an
    inequality that is exactly 0 (include/qpgpu.h)."""
    return _layer_functions()[2].apply(G, g0, CE, ce0, CI, ci0)


def qp_layer_box_full(G, g0, CE, ce0, hi, lo):
    """qp_layer_full for bounds lo <= x <= hi: u is (B, p + 2n), equalities, upper bounds, lower
    bounds (qpgpu_solve_batched_box_dual forward, qpgpu_vjp_box_full backward)."""
    return _layer_functions()[3].apply(G, g0, CE, ce0, hi, lo)


def relayout(src, dst, batch: int, elems: int, to_tiled: bool, stream=None):
    """Device conversion of one per-QP array between layouts (torch tensors)."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream(src.device)
    rc = LIB.qpgpu_relayout(batch, elems, ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                            1 if to_tiled else 0, ctypes.c_void_p(stream.cuda_stream))
    _check(rc, "qpgpu_relayout")


# ----------------------------------------------------------------------------------------------
# synthetic problems, counter-based so shards regenerate identically
# ----------------------------------------------------------------------------------------------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _uniform01(seed: int, idx: np.ndarray, stream: int, count: int) -> np.ndarray:
    """(len(idx), count) uniforms in (0, 1], keyed by (seed, qp index, stream, element)."""
    idx = idx.astype(np.uint64)[:, None]
    k = np.arange(count, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        key = _splitmix64(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ np.uint64(0x5851F42D4C957F2D * (stream + 1) & 0xFFFFFFFFFFFFFFFF))
        c = (idx << np.uint64(24)) + k
        bits = _splitmix64(_splitmix64(c) ^ key)
    return ((bits >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)


def _normal(seed: int, idx: np.ndarray, stream: int, count: int) -> np.ndarray:
    u1 = _uniform01(seed, idx, 2 * stream, count)
    u2 = _uniform01(seed, idx, 2 * stream + 1, count)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)


def make_problems(kind: str, n: int, p: int, m: int, b0: int, b1: int, seed: int = 2026,
                  threads: int = 0) -> Problems:
    """Generate QPs [b0, b1) of a synthetic batch.

    kind="general" (C1, C3, C4, C5): G = M^T M + n I, g0 ~ 10 N(0,1), feasible point
        x_f ~ 0.1 N(0,1), CE ~ N(0,1), ce0 = -CE^T x_f, CI ~ N(0,1), ci0 = -CI^T x_f + |N(0,1)|.
    kind="box" (C2, mgqp joint-limit ordering, reference src/mgqp.cpp:1111-1112): same G, g0, CE;
        CI = [-I, +I] (m = 2n), ci0 = [hi; -lo] with hi = -lo = 1.

    Every QP depends only on (seed, its global index), so large ranges are generated in chunks
    on `threads` host threads (0 = up to 8; numpy releases the GIL) with identical results.
    """
    B = b1 - b0
    chunk = 8192
    if threads == 0:
        threads = min(8, os.cpu_count() or 1)
    if threads > 1 and B > 2 * chunk:
        from concurrent.futures import ThreadPoolExecutor

        cuts = list(range(b0, b1, chunk)) + [b1]
        with ThreadPoolExecutor(threads) as ex:
            parts = list(ex.map(lambda c: _make_range(kind, n, p, m, c[0], c[1], seed),
                                zip(cuts[:-1], cuts[1:])))
        cat = lambda k: np.concatenate([getattr(q, k) for q in parts])
        return Problems(n, p, m, cat("G"), cat("g0"), cat("CE"), cat("ce0"), cat("CI"), cat("ci0"))
    return _make_range(kind, n, p, m, b0, b1, seed)


def make_box_problems(n: int, p: int, b0: int, b1: int, seed: int = 2026) -> BoxProblems:
    """QPs [b0, b1) of make_problems("box", n, p, 2n, ...) with the bounds as vectors: the same
    G, g0, CE, ce0, and hi = 1, lo = -1, so to_dense() equals that call bit for bit."""
    pr = make_problems("box", n, p, 2 * n, b0, b1, seed)
    B = b1 - b0
    return BoxProblems(n, p, pr.G, pr.g0, pr.CE, pr.ce0, np.ones((B, n)), -np.ones((B, n)))


def make_unit_problems(n: int, p: int, m: int, b0: int, b1: int, seed: int = 2026,
                       g0_scale: float = 10.0) -> UnitProblems:
    """QPs [b0, b1) of make_problems("general", n, p, m, ...) with G dropped (the identity stands
    for it) and g0 ~ g0_scale N(0,1) (0.0 gives the controller's g0 = +0.0): the same CE, ce0, CI,
    ci0, so the feasible point is the generator's."""
    pr = make_problems("general", n, p, m, b0, b1, seed)
    g0 = pr.g0 * (g0_scale / 10.0) if g0_scale != 0.0 else np.zeros_like(pr.g0)
    return UnitProblems(n, p, m, np.ascontiguousarray(g0), pr.CE, pr.ce0, pr.CI, pr.ci0)


def _make_range(kind: str, n: int, p: int, m: int, b0: int, b1: int, seed: int) -> Problems:
    idx = np.arange(b0, b1, dtype=np.uint64)
    B = b1 - b0
    M = _normal(seed, idx, 0, n * n).reshape(B, n, n)
    G = np.einsum("bki,bkj->bij", M, M) + n * np.eye(n)[None]
    g0 = 10.0 * _normal(seed, idx, 1, n)
    xf = 0.1 * _normal(seed, idx, 2, n)
    CE = _normal(seed, idx, 3, n * p).reshape(B, n, p)
    ce0 = -np.einsum("bnp,bn->bp", CE, xf)
    if kind == "general":
        CI = _normal(seed, idx, 4, n * m).reshape(B, n, m)
        ci0 = -np.einsum("bnm,bn->bm", CI, xf) + np.abs(_normal(seed, idx, 5, m))
    elif kind == "box":
        if m != 2 * n:
            raise ValueError("box problems need m = 2n")
        eye = np.eye(n)
        CI = np.broadcast_to(np.concatenate([-eye, eye], axis=1), (B, n, m)).copy()
        ci0 = np.ones((B, m))
    else:
        raise ValueError(kind)
    return Problems(n, p, m, np.ascontiguousarray(G), np.ascontiguousarray(g0),
                    np.ascontiguousarray(CE), np.ascontiguousarray(ce0), np.ascontiguousarray(CI),
                    np.ascontiguousarray(ci0))


# ----------------------------------------------------------------------------------------------
# one QP, reference semantics (exceptions instead of status codes)
# ----------------------------------------------------------------------------------------------
def solve_quadprog(G: np.ndarray, g0, CE, ce0, CI, ci0):
    """Single-QP mirror of the reference call: returns (f, x); overwrites G with its Cholesky
    factor; raises ValueError/RuntimeError where the reference raises logic_error/runtime_error.
    CE is n x p and CI is n x m (the t(CE) / t(CI) mgqp passes)."""
    G = np.asarray(G)
    n = G.shape[1]
    CE = np.asarray(CE, dtype=np.float64).reshape(n, -1) if np.size(CE) else np.zeros((n, 0))
    CI = np.asarray(CI, dtype=np.float64).reshape(n, -1) if np.size(CI) else np.zeros((n, 0))
    p, m = CE.shape[1], CI.shape[1]
    if G.shape[0] != n:
        raise ValueError(f"The matrix G is not a squared matrix ({G.shape[0]} x {G.shape[1]})")
    ce0 = np.asarray(ce0, dtype=np.float64).reshape(-1)
    ci0 = np.asarray(ci0, dtype=np.float64).reshape(-1)
    if ce0.size != p:
        raise ValueError(f"The vector ce0 is incompatible (incorrect dimension {ce0.size}, expecting {p})")
    if ci0.size != m:
        raise ValueError(f"The vector ci0 is incompatible (incorrect dimension {ci0.size}, expecting {m})")
    Gc = np.ascontiguousarray(G, dtype=np.float64).reshape(1, n, n).copy()
    pr = Problems(n, p, m, Gc, np.asarray(g0, dtype=np.float64).reshape(1, n), CE.reshape(1, n, p),
                  ce0.reshape(1, p), CI.reshape(1, n, m), ci0.reshape(1, m))
    x, f, st, _ = solve_batched_host(pr, write_factor=True)
    if G.dtype == np.float64 and G.flags.c_contiguous:
        G[...] = Gc[0]
    s = int(st[0])
    if s == QP_NOT_POSITIVE_DEFINITE:
        raise ValueError(f"Error in cholesky decomposition, sum: {f[0]:g}")
    if s == QP_DEPENDENT:
        raise RuntimeError("Constraints are linearly dependent")
    if s == QP_MAX_ITER:
        raise RuntimeError("qpgpu: active-set step cap reached")
    return float(f[0]), x[0]
