// qpgpu_api.cpp — host side of the C-ABI declared in include/qpgpu.h.
//
// Validates the descriptor, picks the gfx950 kernel variant for (n, p, m) and enqueues it on the
// caller's stream.  There is deliberately no CPU path: a shape no kernel covers is an error
// (QPGPU_ERR_UNSUPPORTED_SHAPE), and a missing device is an error (QPGPU_ERR_NO_DEVICE).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/qpgpu.h"
#include "qp_common.h"
#include "qp_kkt.h"
#include "qp_jvp.h"
#include "qp_jvp_many.h"
#include "qp_vjp.h"

extern "C" hipError_t qpk_relayout(int64_t batch, int E, const double* src, double* dst,
                                   int to_tiled, hipStream_t stream);

namespace {

thread_local std::string g_last_error;
uint64_t* g_stamps = nullptr;  // diagnostic stamp buffer (qpgpu_debug_set_stamps)

int hip_fail(hipError_t e, const char* what) {
  g_last_error = std::string(what) + ": " + hipGetErrorString(e);
  return QPGPU_ERR_HIP;
}

// Default safety cap on active-set steps (l2a entries).  Goldfarb–Idnani terminates in a
// finite number of steps; the cap only guarantees that every wave drains on pathological
// input and is far above any count seen on terminating problems.
int default_max_steps(int n, int p, int m) { return 1000 + 100 * (n + p + m); }

// The flag rules of include/qpgpu.h: known bits only, FAST excludes EXACT and WRITE_FACTOR, at
// most one forced family.  Shared by validate() and qpgpu_kernel_name_flags().
bool flags_valid(uint32_t flags) {
  const uint32_t fam = QPGPU_FLAG_FORCE_LANE | QPGPU_FLAG_FORCE_SUBGROUP | QPGPU_FLAG_FORCE_WAVE |
                       QPGPU_FLAG_FORCE_GENERIC;
  const uint32_t known = QPGPU_FLAG_WRITE_FACTOR | QPGPU_FLAG_EXACT | QPGPU_FLAG_FAST | fam;
  if (flags & ~known) return false;
  if ((flags & QPGPU_FLAG_FAST) && (flags & (QPGPU_FLAG_EXACT | QPGPU_FLAG_WRITE_FACTOR))) return false;
  const uint32_t f = flags & fam;
  return (f & (f - 1)) == 0;
}

int validate(const qpgpu_problem_desc* d) {
  if (!d) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->n <= 0 || d->p < 0 || d->m < 0 || d->batch < 0) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->layout != QPGPU_LAYOUT_QP_MAJOR && d->layout != QPGPU_LAYOUT_TILED64)
    return QPGPU_ERR_INVALID_ARGUMENT;
  if (!flags_valid(d->flags)) return QPGPU_ERR_INVALID_ARGUMENT;
  return QPGPU_SUCCESS;
}

struct HostWorkspace {
  void* buf = nullptr;
  size_t bytes = 0;
  int device = -1;
  hipStream_t stream = nullptr;
  ~HostWorkspace() {
    if (buf) (void)hipFree(buf);
    if (stream) (void)hipStreamDestroy(stream);
  }
};
thread_local HostWorkspace g_ws;

// Device workspace for the kernels that keep J and R in global memory (n > 64).  Grow-only and
// cached per (device, stream), so launches on different streams never share one; growing syncs
// only the stream that used the old buffer.  The caller keeps `hold` (the cache's lock) until its
// launches are enqueued: a host thread that grows the buffer of a stream another thread has just
// been handed — the default stream, say — would otherwise free it before that thread's kernel is
// in the stream (the stream sync before the free only covers work already enqueued).
struct DevWorkspace {
  void* buf = nullptr;
  size_t bytes = 0;
};
std::mutex g_dev_ws_mu;
std::map<std::pair<int, hipStream_t>, DevWorkspace> g_dev_ws;

int device_workspace(int64_t bytes, hipStream_t stream, double** out, std::unique_lock<std::mutex>& hold) {
  *out = nullptr;
  if (bytes <= 0) return QPGPU_SUCCESS;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
  if (!hold.owns_lock()) hold = std::unique_lock<std::mutex>(g_dev_ws_mu);
  DevWorkspace& w = g_dev_ws[{dev, stream}];
  if (w.bytes < (size_t)bytes) {
    if (w.buf) {
      if ((e = hipStreamSynchronize(stream)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
      (void)hipFree(w.buf);
      w.buf = nullptr;
      w.bytes = 0;
    }
    if ((e = hipMalloc(&w.buf, (size_t)bytes)) != hipSuccess) return hip_fail(e, "hipMalloc workspace");
    w.bytes = (size_t)bytes;
  }
  *out = static_cast<double*>(w.buf);
  return QPGPU_SUCCESS;
}

}  // namespace

extern "C" {

int qpgpu_abi_version(void) { return QPGPU_ABI_VERSION; }

const char* qpgpu_last_error(void) { return g_last_error.c_str(); }

int qpgpu_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

// the wave family's workspace class, the largest a table kernel holds (the generic kernel beyond it)
#define QPK_CLASS_N(S, N, M) N
#define QPK_CLASS_M(S, N, M) M
int qpgpu_max_n(void) { return QPK_WAVE_WS_SIZE(QPK_CLASS_N); }
int qpgpu_max_m(void) { return QPK_WAVE_WS_SIZE(QPK_CLASS_M); }
#undef QPK_CLASS_N
#undef QPK_CLASS_M

// Default family order: lane (n <= 8, m <= 16), then the subgroup kernel only where it is the
// faster one — n <= 8, m <= 32 (its S = 8 variants) — then the wave kernels.  Measured on MI355X
// with 65 536 QPs per launch (profiles/r01_s2/family_crossover.log): the wave family's
// runtime-sized LDS layout beats the S = 16 subgroup kernel from n = 9 up (n = 14, m = 28:
// 2.2 vs 3.5 ms) and at m = 64; the S = 8 subgroup kernel still wins at n <= 8, m <= 32.
static bool default_small(int n, int m) { return n <= 8 && m <= 32; }

// Largest device workspace one generic-kernel launch uses (bytes); larger batches run as
// sub-batches (launch_generic).  4 GiB; qpgpu_debug_set_generic_ws_cap lowers it in tests.
static int64_t g_generic_ws_cap = (int64_t)4 << 30;

// ---- the selection: which kernel runs for (n, p, m, flags, mode, build) -----------
// The one statement of the policy: the name functions, the host entries' coverage check and the
// launch (run) all ask it.  family == kNone: no kernel — a rejected flag combination or a shape
// (or mode) the family asked for lacks.
enum Family { kNone, kLane, kSmall, kWave, kGeneric };
// A family's builds: the exact kernels, the QPGPU_FLAG_FAST restatement, the unit-Hessian kernels of
// qpgpu_solve_batched_unit.  (An unaligned lane build runs what its aligned twin names.)
enum Build { kExact, kFast, kUnit };
struct Pick {
  Family family = kNone;
  Build build = kExact;
  const char* name = "";
};

// Largest shape the generic kernel accepts: n*n and the workspace offsets stay within int64 and a
// QP's workspace within 2^34 doubles (128 GiB); int32 element indices of the inputs (n*n, n*m).
// CE offsets (n*p, j*p + i) are computed in int64, so p is not bounded here.
static bool generic_covers(int n, int m) {
  return n >= 1 && m >= 0 && (int64_t)n * n < ((int64_t)1 << 31) && (int64_t)n * m < ((int64_t)1 << 31);
}

// Every kernel's name: one row per size class (n <= nmax, m <= mmax) of the families' lists in
// qp_common.h, smallest first within a family, and in a row one name per build and mode — NULL
// where the build has no kernel: the fast and the unit builds restate the plain kernels only, the
// subgroup and generic families have no fast build, the generic family no unit build, and the wave
// family's workspace class is the exact build's alone.  A shape runs in its family's first row that
// holds it; the generic family's one row holds what generic_covers.
static const char* kernel_name(Family family, Build build, int n, int m, qpk::Mode mode) {
  static const struct {
    Family family;
    int nmax, mmax;
    const char* name[3][4];  // [Build][qpk::Mode]
  } rows[] = {
// the exact build's four names (the plain one after `pre`), then the fast and the unit build's
#define QPK_NAMES(pre, k, s, fast, unit) \
  {{pre k "<" s ">", k "_dual<" s ">", k "_box<" s ">", k "_box_dual<" s ">"}, {fast}, {unit}}
#define QPK_NM(N, M) "N=" #N ",M=" #M
#define QPK_SNM(S, N, M) "S=" #S ",N=" #N ",M=" #M
#define QPK_LANE_ROW(N, M)                                                                   \
  {kLane, N, M, QPK_NAMES("", "qp_lane", QPK_NM(N, M), "qp_lane_fast<" QPK_NM(N, M) ">", \
                          "qp_lane_unit<" QPK_NM(N, M) ">")},
#define QPK_SMALL_ROW(S, N, M) \
  {kSmall, N, M, QPK_NAMES("", "qp_small", QPK_SNM(S, N, M), nullptr, "qp_small_unit<" QPK_SNM(S, N, M) ">")},
#define QPK_WAVE_ROW(S, N, M)                                                                         \
  {kWave, N, M, QPK_NAMES("", "qp_wave", QPK_SNM(S, N, M), "qp_wave_fast<" QPK_SNM(S, N, M) ">", \
                          "qp_wave_unit<" QPK_SNM(S, N, M) ">")},
// (the plain mode's default is the panel path; the other modes always run EXACT, without it)
#define QPK_WAVE_WS_ROW(S, N, M)                                                                       \
  {kWave, N, M, QPK_NAMES("qp_panel<MFMA f64 16x16x4> + ", "qp_wave", QPK_SNM(S, N, M) ",global J/R", \
                          nullptr, nullptr)},
      QPK_LANE_SIZES(QPK_LANE_ROW) QPK_SMALL_SIZES(QPK_SMALL_ROW) QPK_WAVE_LDS_SIZES(QPK_WAVE_ROW)
          QPK_WAVE_WS_SIZE(QPK_WAVE_WS_ROW)
      {kGeneric, INT32_MAX, INT32_MAX, QPK_NAMES("", "qp_generic", "BS=256,global workspace", nullptr, nullptr)},
#undef QPK_WAVE_WS_ROW
#undef QPK_WAVE_ROW
#undef QPK_SMALL_ROW
#undef QPK_LANE_ROW
#undef QPK_SNM
#undef QPK_NM
#undef QPK_NAMES
  };
  if (family == kGeneric && !generic_covers(n, m)) return nullptr;
  for (const auto& r : rows)
    if (r.family == family && n <= r.nmax && m <= r.mmax) return r.name[build][mode];
  return nullptr;
}

// build: kExact (QPGPU_FLAG_FAST makes it kFast) or kUnit, the selection of qpgpu_solve_batched_unit
// (DESIGN §3.10): plain mode only, and nothing for QPGPU_FLAG_FAST (there is no fast unit form),
// QPGPU_FLAG_WRITE_FACTOR (there is no G) and QPGPU_FLAG_FORCE_GENERIC (no unit kernel beyond the
// wave family's LDS classes: n > 64 and m > 256 have none either).
static Pick select_kernel(int n, int p, int m, uint32_t flags, qpk::Mode mode, Build build = kExact) {
  if (!flags_valid(flags)) return {};
  // the fast builds restate the plain kernels only: the other modes refuse QPGPU_FLAG_FAST
  if ((flags & QPGPU_FLAG_FAST) && mode != qpk::kPlain) return {};
  if (build == kUnit && (flags & (QPGPU_FLAG_FAST | QPGPU_FLAG_WRITE_FACTOR | QPGPU_FLAG_FORCE_GENERIC))) return {};
  const uint32_t force = flags & (QPGPU_FLAG_FORCE_LANE | QPGPU_FLAG_FORCE_SUBGROUP |
                                  QPGPU_FLAG_FORCE_WAVE | QPGPU_FLAG_FORCE_GENERIC);
  // Sizes no launch has (validate): no kernel — except that qpgpu_kernel_name_flags has always
  // answered with a forced family's exact kernel where that family's table admits them.
  const bool sized = n > 0 && p >= 0 && m >= 0;
  if (!sized && (!force || mode != qpk::kPlain || build == kUnit)) return {};
  if ((flags & QPGPU_FLAG_FAST) && sized) build = kFast;
  // A forced family keeps to that family; otherwise lane, subgroup (only where default_small),
  // wave, generic.  With FAST a family's fast build comes first where it covers the shape and its
  // exact kernels otherwise; the subgroup and generic families have none, so FAST | FORCE_GENERIC
  // is the generic kernel and a default_small shape takes the subgroup kernel ahead of the fast
  // wave build.
  for (const Family family : {kLane, kSmall, kWave, kGeneric}) {
    static const uint32_t kForce[] = {0, QPGPU_FLAG_FORCE_LANE, QPGPU_FLAG_FORCE_SUBGROUP, QPGPU_FLAG_FORCE_WAVE,
                                      QPGPU_FLAG_FORCE_GENERIC};
    if (force ? force != kForce[family] : (family == kSmall && !default_small(n, m))) continue;
    if (const char* s = kernel_name(family, build, n, m, mode)) return {family, build, s};
    if (build != kFast) continue;
    if (const char* s = kernel_name(family, kExact, n, m, mode)) return {family, kExact, s};
  }
  return {};
}

const char* qpgpu_kernel_name_unit(int32_t n, int32_t p, int32_t m, uint32_t flags) {
  return select_kernel(n, p, m, flags, qpk::kPlain, kUnit).name;
}

const char* qpgpu_kernel_name_flags(int32_t n, int32_t p, int32_t m, uint32_t flags) {
  return select_kernel(n, p, m, flags, qpk::kPlain).name;
}

const char* qpgpu_kernel_name(int32_t n, int32_t p, int32_t m) { return select_kernel(n, p, m, 0, qpk::kPlain).name; }

// the box entries' kernels: the selection for (n, p, 2n) in their mode
static const char* box_kernel_name(int32_t n, int32_t p, uint32_t flags, qpk::Mode mode) {
  return n > INT32_MAX / 2 ? "" : select_kernel(n, p, 2 * n, flags, mode).name;
}
const char* qpgpu_kernel_name_box(int32_t n, int32_t p, uint32_t flags) {
  return box_kernel_name(n, p, flags, qpk::kBox);
}
const char* qpgpu_kernel_name_box_dual(int32_t n, int32_t p, uint32_t flags) {
  return box_kernel_name(n, p, flags, qpk::kBoxDual);
}

// Does a kernel cover the shape (the forced family's, if one is forced)?  The host entries check
// it before any copy is queued.
static bool family_covers(uint32_t flags, int n, int p, int m) {
  return select_kernel(n, p, m, flags, qpk::kPlain).family != kNone;
}

// The internal QpArgs.flags bits that license the lane kernel's explicit 16-byte accesses through
// the caller's pointers (include/qpgpu.h asks for natural alignment only).  One bit per group of
// arrays, so that an odd g0 does not switch off CI's on-chip copy and an odd ci0 not the staging:
//   kArgAligned16  CI and ci0: the per-lane LDS-DMA of CI rows, the LDS-resident CI rows and the
//                  double2 row loads of the l1 scan
//   kArgStage16    G, g0 and (p > 0) CE, ce0: the per-wave LDS-DMA staging (stage_all / round B)
// A NULL pointer (an empty array, or CI / ci0 of the box entries) counts as aligned: it is never
// read through.  Whole tiles and QP blocks of 64 keep every wave's base at the array's residue.
static uint32_t alignment_flags(const double* G, const double* g0, const double* CE,
                                const double* ce0, const double* CI, const double* ci0, int32_t p) {
  auto bits = [](const void* q) { return reinterpret_cast<uintptr_t>(q); };
  uint32_t f = 0;
  if (((bits(CI) | bits(ci0)) & 15u) == 0) f |= qpk::kArgAligned16;
  uintptr_t st = bits(G) | bits(g0);
  if (p > 0) st |= bits(CE) | bits(ce0);
  if ((st & 15u) == 0) f |= qpk::kArgStage16;
  return f;
}

// The kernels' argument from a validated descriptor and the arrays every entry has, as the caller
// passed them (the alignment bits are theirs).  An entry then sets its own optional members by
// name — x_eq / f_eq / st_eq, u / nact, hi / lo (CI and ci0 NULL) — and calls run().
static qpk::QpArgs make_args(const qpgpu_problem_desc* d, double* G, const double* g0, const double* CE,
                             const double* ce0, const double* CI, const double* ci0, double* x, double* f,
                             int32_t* status, int32_t* iters) {
  qpk::QpArgs a = {};
  a.n = d->n;
  a.p = d->p;
  a.m = d->m;
  a.max_steps = d->max_iter > 0 ? d->max_iter : default_max_steps(d->n, d->p, d->m);
  a.batch = d->batch;
  a.tile = d->layout == QPGPU_LAYOUT_TILED64 ? 64 : 1;
  a.flags = (d->flags & (QPGPU_FLAG_WRITE_FACTOR | QPGPU_FLAG_EXACT)) | alignment_flags(G, g0, CE, ce0, CI, ci0, d->p);
  a.G = G;
  a.g0 = g0;
  a.CE = CE;
  a.ce0 = ce0;
  a.CI = CI;
  a.ci0 = ci0;
  a.x = x;
  a.f = f;
  a.status = status;
  a.iters = iters;
  a.stamps = g_stamps;
  return a;
}

// The generic kernel's workspace is per QP (2n^2 + 12n + 2m doubles): a large shape launches
// over sub-batches whose workspace stays within g_generic_ws_cap (one allocation reused by every
// sub-batch in stream order), instead of one allocation for the whole batch — n = 2000 over
// 1000 QPs would otherwise ask for ~64 GB and keep it cached.  TILED64 sub-batches are whole
// 64-QP tiles, so each one's arrays start at a tile boundary.
static int launch_generic(const qpk::QpArgs& a, hipStream_t s, std::unique_lock<std::mutex>& ws_hold) {
  const int64_t per = qpk_generic_workspace_bytes(a.n, a.m, 1);
  int64_t chunk = a.batch;
  if (a.batch > g_generic_ws_cap / per) {  // per * batch > cap, without the int64 overflow
    chunk = g_generic_ws_cap / per;
    if (a.tile == 64) chunk = chunk / 64 * 64;
    if (chunk < (a.tile == 64 ? 64 : 1)) chunk = a.tile == 64 ? 64 : 1;
  }
  double* ws = nullptr;
  const int rc = device_workspace(per * (chunk < a.batch ? chunk : a.batch), s, &ws, ws_hold);
  if (rc) return rc;
  for (int64_t b0 = 0; b0 < a.batch; b0 += chunk) {
    qpk::QpArgs c = qpk::sub_range(a, b0, a.batch - b0 < chunk ? a.batch - b0 : chunk);
    if (c.hi) c.CI = c.ci0 = c.g0;  // (never read; kept inside an array of this sub-batch)
    c.stamps = nullptr;
    const hipError_t e = qpk_launch_generic(&c, s, ws);
    if (e != hipSuccess) return hip_fail(e, "kernel launch");
  }
  return QPGPU_SUCCESS;
}

// What every device-pointer entry ends in, after validate(d) and its own rules: the empty batch,
// the NULL checks of the common arrays, the selection, the launch.  unit: the entry without a G
// array (qpgpu_solve_batched_unit) — a.G is NULL and the families' unit builds run.
static int run(const qpgpu_problem_desc* d, qpk::QpArgs a, void* stream, bool unit = false) {
  if (d->batch == 0) return QPGPU_SUCCESS;
  if ((!unit && !a.G) || !a.g0 || !a.x || !a.f || !a.status) return QPGPU_ERR_INVALID_ARGUMENT;
  if ((a.p > 0 && (!a.CE || !a.ce0)) || (!a.hi && a.m > 0 && (!a.CI || !a.ci0)))
    return QPGPU_ERR_INVALID_ARGUMENT;
  const Pick k = select_kernel(a.n, a.p, a.m, d->flags, qpk::mode_of(a), unit ? kUnit : kExact);
  if (k.family == kNone) return QPGPU_ERR_UNSUPPORTED_SHAPE;
  // An empty array (p == 0: CE, ce0; m == 0: CI, ci0) may be passed as NULL, and a torch tensor of
  // no elements has a NULL data_ptr; the box kernels never read CI / ci0.  The wave kernels' l1
  // scan loads element 0 of a clamped constraint index without a predicate and discards the value
  // (qp_wave.hip, "a lane's two constraints"), which faulted on NULL: give the kernels readable
  // memory instead — g0, whose first element of every QP block (or tile) exists in both layouts.
  if (!a.CE) a.CE = a.g0;
  if (!a.ce0) a.ce0 = a.g0;
  if (!a.CI) a.CI = a.g0;
  if (!a.ci0) a.ci0 = a.g0;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  std::unique_lock<std::mutex> ws_hold;  // the workspace cache's lock, until the launches are enqueued
  using Launch = hipError_t (*)(const qpk::QpArgs*, hipStream_t);
  hipError_t e = hipSuccess;
  switch (k.family) {
    case kLane: {
      // The lane kernels stage G, g0, CE and ce0 by 16-byte LDS-DMA: launched only when those arrays
      // are 16-byte aligned, their QPGPU_LANE_UNALIGNED builds (per-lane 8-byte copies) otherwise.
      // (The unit builds' staged group is g0, CE and ce0: alignment_flags saw a NULL G.)
      static const Launch kLaneLaunch[3][2] = {{qpk_launch_lane_u, qpk_launch_lane},  // [Build][kArgStage16 set]
                                               {qpk_launch_lane_fast_u, qpk_launch_lane_fast},
                                               {qpk_launch_lane_unit_u, qpk_launch_lane_unit}};
      e = kLaneLaunch[k.build][(a.flags & qpk::kArgStage16) != 0](&a, s);
      break;
    }
    case kSmall:
      e = k.build == kUnit ? qpk_launch_small_unit(&a, s) : qpk_launch_small(&a, s);
      break;
    case kWave:
      if (k.build == kExact) {
        double* ws = nullptr;
        const int rc = device_workspace(qpk_medium_workspace_bytes(&a), s, &ws, ws_hold);
        if (rc) return rc;
        e = qpk_launch_medium(&a, s, ws);
      } else {
        e = k.build == kUnit ? qpk_launch_medium_unit(&a, s) : qpk_launch_medium_fast(&a, s);
      }
      break;
    case kGeneric:
      return launch_generic(a, s, ws_hold);
    case kNone:
      break;
  }
  if (e != hipSuccess) return hip_fail(e, "kernel launch");
  return QPGPU_SUCCESS;
}

int qpgpu_solve_batched(const qpgpu_problem_desc* d, double* G, const double* g0,
                        const double* CE, const double* ce0, const double* CI,
                        const double* ci0, double* x, double* f, int32_t* status,
                        int32_t* iters, void* stream) {
  const int rc = validate(d);
  if (rc) return rc;
  return run(d, make_args(d, G, g0, CE, ce0, CI, ci0, x, f, status, iters), stream);
}

int qpgpu_solve_batched_eq(const qpgpu_problem_desc* d, double* G, const double* g0,
                           const double* CE, const double* ce0, const double* CI,
                           const double* ci0, double* x, double* f, int32_t* status,
                           int32_t* iters, double* x_eq, double* f_eq, int32_t* status_eq,
                           void* stream) {
  const int rc = validate(d);
  if (rc) return rc;
  if (!x_eq || !f_eq || !status_eq) return QPGPU_ERR_INVALID_ARGUMENT;
  qpk::QpArgs a = make_args(d, G, g0, CE, ce0, CI, ci0, x, f, status, iters);
  a.x_eq = x_eq;
  a.f_eq = f_eq;
  a.st_eq = status_eq;
  return run(d, a, stream);
}

// The identity Hessian without a G array (include/qpgpu.h).  The unit kernels restate
// the reference's operation order only, so the call runs as if QPGPU_FLAG_EXACT were set;
// QPGPU_FLAG_FAST and QPGPU_FLAG_WRITE_FACTOR are refused.  The m = 0 snapshot is all three arrays
// or none.  Every rule is decided from the descriptor and the pointers' values before anything is
// launched; no workspace, one kernel, so the first call for a shape can be captured.
int qpgpu_solve_batched_unit(const qpgpu_problem_desc* d, const double* g0, const double* CE,
                             const double* ce0, const double* CI, const double* ci0, double* x,
                             double* f, int32_t* status, int32_t* iters, double* x_eq, double* f_eq,
                             int32_t* status_eq, void* stream) {
  const int rc = validate(d);
  if (rc) return rc;
  if (d->flags & (QPGPU_FLAG_FAST | QPGPU_FLAG_WRITE_FACTOR)) return QPGPU_ERR_INVALID_ARGUMENT;
  const int eq = (x_eq ? 1 : 0) + (f_eq ? 1 : 0) + (status_eq ? 1 : 0);
  if (eq != 0 && eq != 3) return QPGPU_ERR_INVALID_ARGUMENT;
  qpk::QpArgs a = make_args(d, nullptr, g0, CE, ce0, CI, ci0, x, f, status, iters);
  a.flags |= QPGPU_FLAG_EXACT;
  a.x_eq = x_eq;
  a.f_eq = f_eq;
  a.st_eq = status_eq;
  return run(d, a, stream, true);
}

// The multipliers too (include/qpgpu.h).  The dual kernels restate the reference's operation
// order only, so the call runs as if QPGPU_FLAG_EXACT were set — for n > 64 that keeps it off the
// tolerance mode (panel setup, tree sums, certification, re-solve), which has no dual form — and
// QPGPU_FLAG_FAST is refused.  With p + m == 0 there is nothing to return: the plain kernels run.
int qpgpu_solve_batched_dual(const qpgpu_problem_desc* d, double* G, const double* g0,
                             const double* CE, const double* ce0, const double* CI,
                             const double* ci0, double* x, double* f, int32_t* status,
                             int32_t* iters, double* u, int32_t* nact, void* stream) {
  const int rc = validate(d);
  if (rc) return rc;
  if (d->flags & QPGPU_FLAG_FAST) return QPGPU_ERR_INVALID_ARGUMENT;
  const bool any = (int64_t)d->p + d->m > 0;
  if (any && !u) return QPGPU_ERR_INVALID_ARGUMENT;
  qpk::QpArgs a = make_args(d, G, g0, CE, ce0, CI, ci0, x, f, status, iters);
  a.flags |= QPGPU_FLAG_EXACT;
  if (any) {
    a.u = u;
    a.nact = nact;
  } else if (nact && d->batch > 0) {
    hipError_t e = hipMemsetAsync(nact, 0, (size_t)d->batch * sizeof(int32_t),
                                  reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
  }
  return run(d, a, stream);
}

// Bounds instead of a dense CI (include/qpgpu.h), and with the multipliers (box_dual): the rules
// the two entries share.  The box kernels restate the reference's operation order only, so the
// call runs as if QPGPU_FLAG_EXACT were set — for n > 64 that keeps it off the tolerance mode,
// which has no box form — and QPGPU_FLAG_FAST is refused.
static int box_rules(const qpgpu_problem_desc* d, const double* hi, const double* lo) {
  const int rc = validate(d);
  if (rc) return rc;
  if (d->flags & QPGPU_FLAG_FAST) return QPGPU_ERR_INVALID_ARGUMENT;
  if ((int64_t)d->m != 2 * (int64_t)d->n) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->batch > 0 && (!hi || !lo)) return QPGPU_ERR_INVALID_ARGUMENT;
  return QPGPU_SUCCESS;
}

int qpgpu_solve_batched_box(const qpgpu_problem_desc* d, double* G, const double* g0,
                            const double* CE, const double* ce0, const double* hi,
                            const double* lo, double* x, double* f, int32_t* status,
                            int32_t* iters, void* stream) {
  const int rc = box_rules(d, hi, lo);
  if (rc) return rc;
  qpk::QpArgs a = make_args(d, G, g0, CE, ce0, nullptr, nullptr, x, f, status, iters);
  a.flags |= QPGPU_FLAG_EXACT;
  a.hi = hi;
  a.lo = lo;
  return run(d, a, stream);
}

// With hi and u both set every family launches its box-dual kernel; no CI is written anywhere.
int qpgpu_solve_batched_box_dual(const qpgpu_problem_desc* d, double* G, const double* g0,
                                 const double* CE, const double* ce0, const double* hi,
                                 const double* lo, double* x, double* f, int32_t* status,
                                 int32_t* iters, double* u, int32_t* nact, void* stream) {
  const int rc = box_rules(d, hi, lo);
  if (rc) return rc;
  if (!u) return QPGPU_ERR_INVALID_ARGUMENT;  // p + 2n > 0 always
  qpk::QpArgs a = make_args(d, G, g0, CE, ce0, nullptr, nullptr, x, f, status, iters);
  a.flags |= QPGPU_FLAG_EXACT;
  a.hi = hi;
  a.lo = lo;
  a.u = u;
  a.nact = nact;
  return run(d, a, stream);
}


// ---- the KKT check (include/qpgpu.h; kernel: qp_kkt.hip) -------------------------------
// Both entries: every rule is decided from the descriptor and the pointers' values, before any
// array is read; no workspace, one kernel, so the first call for a shape can be captured.
static int kkt_run(const qpgpu_problem_desc* d, bool box, const double* G, const double* g0,
                   const double* CE, const double* ce0, const double* CI, const double* ci0,
                   const double* hi, const double* lo, const double* x, const double* u,
                   const int32_t* status, double* r, void* stream) {
  if (!d) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->n <= 0 || d->p < 0 || d->m < 0 || d->batch < 0) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->layout != QPGPU_LAYOUT_QP_MAJOR && d->layout != QPGPU_LAYOUT_TILED64)
    return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->flags != 0) return QPGPU_ERR_INVALID_ARGUMENT;
  if (box && (int64_t)d->m != 2 * (int64_t)d->n) return QPGPU_ERR_INVALID_ARGUMENT;
  if ((int64_t)d->p + d->m > 0 && !u) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->batch > 0) {
    if (!G || !g0 || !x || !r) return QPGPU_ERR_INVALID_ARGUMENT;
    if (d->p > 0 && (!CE || !ce0)) return QPGPU_ERR_INVALID_ARGUMENT;
    if (box ? (!hi || !lo) : (d->m > 0 && (!CI || !ci0))) return QPGPU_ERR_INVALID_ARGUMENT;
  }
  // the solve entries' size limit (qp_generic.hip): a per-QP block is indexed with 32 bits
  const int64_t lim = (int64_t)1 << 31;
  if ((int64_t)d->n * d->n >= lim || (int64_t)d->n * d->m >= lim || (int64_t)d->n * d->p >= lim ||
      (int64_t)d->p + d->m >= lim)
    return QPGPU_ERR_UNSUPPORTED_SHAPE;
  if (d->batch == 0) return QPGPU_SUCCESS;
  qpk::KktArgs a = {d->n, d->p, d->m, 0, d->batch, 0, G, g0, CE, ce0, box ? nullptr : CI, box ? nullptr : ci0,
                    box ? hi : nullptr, box ? lo : nullptr, x, u, status, r};
  const hipError_t e = qpk_launch_kkt(&a, d->layout == QPGPU_LAYOUT_TILED64, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "kernel launch");
  return QPGPU_SUCCESS;
}

int qpgpu_kkt_residuals(const qpgpu_problem_desc* d, const double* G, const double* g0,
                        const double* CE, const double* ce0, const double* CI, const double* ci0,
                        const double* x, const double* u, const int32_t* status, double* r,
                        void* stream) {
  return kkt_run(d, false, G, g0, CE, ce0, CI, ci0, nullptr, nullptr, x, u, status, r, stream);
}

int qpgpu_kkt_residuals_box(const qpgpu_problem_desc* d, const double* G, const double* g0,
                            const double* CE, const double* ce0, const double* hi, const double* lo,
                            const double* x, const double* u, const int32_t* status, double* r,
                            void* stream) {
  return kkt_run(d, true, G, g0, CE, ce0, nullptr, nullptr, hi, lo, x, u, status, r, stream);
}

// ---- the backward step (include/qpgpu.h; kernels: qp_vjp.hip) -------------------------
// Both entries: every rule is decided from the descriptor and the pointers' values, before any
// array is read; no workspace, one kernel, so the first call for a shape can be captured.
// The argument rules that the backward and the forward entries share, in the header's order.
static int sens_rules(const qpgpu_problem_desc* d, bool box, const double* G, const double* CE,
                      const double* CI, const double* x, const double* u) {
  if (!d) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->n <= 0 || d->p < 0 || d->m < 0 || d->batch < 0) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->layout != QPGPU_LAYOUT_QP_MAJOR && d->layout != QPGPU_LAYOUT_TILED64)
    return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->flags != 0) return QPGPU_ERR_INVALID_ARGUMENT;
  if (box && (int64_t)d->m != 2 * (int64_t)d->n) return QPGPU_ERR_INVALID_ARGUMENT;
  if ((int64_t)d->p + d->m > 0 && !u) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->batch > 0) {
    if (!G || !x) return QPGPU_ERR_INVALID_ARGUMENT;
    if (d->p > 0 && !CE) return QPGPU_ERR_INVALID_ARGUMENT;
    if (!box && d->m > 0 && !CI) return QPGPU_ERR_INVALID_ARGUMENT;
  }
  return QPGPU_SUCCESS;
}

// The argument rules of the backward entries: the shared ones, and gx.
static int vjp_rules(const qpgpu_problem_desc* d, bool box, const double* G, const double* CE,
                     const double* CI, const double* x, const double* u, const double* gx) {
  const int rc = sens_rules(d, box, G, CE, CI, x, u);
  if (rc) return rc;
  return (d->batch > 0 && !gx) ? QPGPU_ERR_INVALID_ARGUMENT : QPGPU_SUCCESS;
}

// The kernels' argument block: the arrays of the other kind of CI are dropped.
static qpk::VjpArgs vjp_args(const qpgpu_problem_desc* d, bool box, const double* G, const double* CE,
                             const double* CI, const double* x, const double* u, const int32_t* status,
                             const double* gx, double* dG, double* dg0, double* dCE, double* dce0, double* dCI,
                             double* dci0, double* dhi, double* dlo) {
  return {d->n, d->p, d->m, box ? 1 : 0, d->batch, 0, G, CE, box ? nullptr : CI, x, u, status, gx,
          dG, dg0, dCE, dce0, box ? nullptr : dCI, box ? nullptr : dci0, box ? dhi : nullptr,
          box ? dlo : nullptr};
}

// a kernel's name for the qpgpu_kernel_name_* entries: the first that exists, else ""
static const char* name_or_empty(const char* k, const char* k2 = nullptr) { return k ? k : k2 ? k2 : ""; }

// a per-QP block is indexed with 32 bits
static bool vjp_sizes_fit(const qpgpu_problem_desc* d) {
  const int64_t lim = (int64_t)1 << 31;
  return (int64_t)d->n * d->m < lim && (int64_t)d->n * d->p < lim && (int64_t)d->p + d->m < lim;
}

static int vjp_run(const qpgpu_problem_desc* d, bool box, const double* G, const double* CE,
                   const double* CI, const double* x, const double* u, const int32_t* status,
                   const double* gx, double* dG, double* dg0, double* dCE, double* dce0, double* dCI,
                   double* dci0, double* dhi, double* dlo, void* stream, bool full = false,
                   const double* gu = nullptr, const double* gf = nullptr) {
  const int rc = vjp_rules(d, box, G, CE, CI, x, u, gx);
  if (rc) return rc;
  // n <= 64: L, M and S of a QP fit on chip
  if (!qpk_vjp_name(d->n) || !vjp_sizes_fit(d)) return QPGPU_ERR_UNSUPPORTED_SHAPE;
  if (d->batch == 0) return QPGPU_SUCCESS;
  const qpk::VjpArgs a = vjp_args(d, box, G, CE, CI, x, u, status, gx, dG, dg0, dCE, dce0, dCI, dci0, dhi, dlo);
  const int tiled = d->layout == QPGPU_LAYOUT_TILED64;
  hipError_t e;
  if (full) {
    const qpk::VjpFullArgs fa = {a, gu, gf};
    e = qpk_launch_vjp_full(&fa, tiled, reinterpret_cast<hipStream_t>(stream));
  } else {
    e = qpk_launch_vjp(&a, tiled, reinterpret_cast<hipStream_t>(stream));
  }
  if (e != hipSuccess) return hip_fail(e, "kernel launch");
  return QPGPU_SUCCESS;
}

int qpgpu_vjp(const qpgpu_problem_desc* d, const double* G, const double* CE, const double* CI,
              const double* x, const double* u, const int32_t* status, const double* gx, double* dG,
              double* dg0, double* dCE, double* dce0, double* dCI, double* dci0, void* stream) {
  return vjp_run(d, false, G, CE, CI, x, u, status, gx, dG, dg0, dCE, dce0, dCI, dci0, nullptr, nullptr, stream);
}

int qpgpu_vjp_box(const qpgpu_problem_desc* d, const double* G, const double* CE, const double* x,
                  const double* u, const int32_t* status, const double* gx, double* dG, double* dg0,
                  double* dCE, double* dce0, double* dhi, double* dlo, void* stream) {
  return vjp_run(d, true, G, CE, nullptr, x, u, status, gx, dG, dg0, dCE, dce0, nullptr, nullptr, dhi, dlo, stream);
}

const char* qpgpu_kernel_name_vjp(int32_t n, int32_t, int32_t) { return name_or_empty(qpk_vjp_name(n)); }

// ---- the backward step with a caller's workspace (kernel for 64 < n <= 256: qp_vjp_ws.hip) --------
// n <= 64 is vjp_run itself.  Beyond, the workspace rules follow the shape rule, all before the
// device is touched; the launch allocates nothing, so the first call for a shape can be captured.
static int vjp_ws_run(const qpgpu_problem_desc* d, bool box, const double* G, const double* CE,
                      const double* CI, const double* x, const double* u, const int32_t* status,
                      const double* gx, double* dG, double* dg0, double* dCE, double* dce0, double* dCI,
                      double* dci0, double* dhi, double* dlo, void* workspace, int64_t workspace_bytes,
                      void* stream, bool full = false, const double* gu = nullptr, const double* gf = nullptr) {
  const int rc = vjp_rules(d, box, G, CE, CI, x, u, gx);
  if (rc) return rc;
  if (qpk_vjp_name(d->n))
    return vjp_run(d, box, G, CE, CI, x, u, status, gx, dG, dg0, dCE, dce0, dCI, dci0, dhi, dlo, stream, full, gu, gf);
  if (!qpk_vjp_ws_name(d->n) || !vjp_sizes_fit(d)) return QPGPU_ERR_UNSUPPORTED_SHAPE;
  if (d->batch == 0) return QPGPU_SUCCESS;
  const int64_t per = qpk_vjp_ws_doubles(d->n) * (int64_t)sizeof(double);
  if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 8 != 0 || workspace_bytes < per)
    return QPGPU_ERR_INVALID_ARGUMENT;
  const qpk::VjpArgs a = vjp_args(d, box, G, CE, CI, x, u, status, gx, dG, dg0, dCE, dce0, dCI, dci0, dhi, dlo);
  const int tiled = d->layout == QPGPU_LAYOUT_TILED64;
  hipError_t e;
  if (full) {
    const qpk::VjpFullArgs fa = {a, gu, gf};
    e = qpk_launch_vjp_ws_full(&fa, tiled, workspace, workspace_bytes / per, reinterpret_cast<hipStream_t>(stream));
  } else {
    e = qpk_launch_vjp_ws(&a, tiled, workspace, workspace_bytes / per, reinterpret_cast<hipStream_t>(stream));
  }
  if (e != hipSuccess) return hip_fail(e, "kernel launch");
  return QPGPU_SUCCESS;
}

int qpgpu_vjp_workspace_bytes(const qpgpu_problem_desc* d, int64_t slots, int64_t* bytes) {
  if (!d || !bytes || slots < 1) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->n <= 0 || d->p < 0 || d->m < 0 || d->batch < 0) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->n > 64 && !qpk_vjp_ws_name(d->n)) return QPGPU_ERR_UNSUPPORTED_SHAPE;
  const int64_t per = qpk_vjp_ws_doubles(d->n) * (int64_t)sizeof(double);
  if (per > 0 && slots > INT64_MAX / per) return QPGPU_ERR_INVALID_ARGUMENT;
  *bytes = slots * per;
  return QPGPU_SUCCESS;
}

int qpgpu_vjp_ws(const qpgpu_problem_desc* d, const double* G, const double* CE, const double* CI,
                 const double* x, const double* u, const int32_t* status, const double* gx, double* dG,
                 double* dg0, double* dCE, double* dce0, double* dCI, double* dci0, void* workspace,
                 int64_t workspace_bytes, void* stream) {
  return vjp_ws_run(d, false, G, CE, CI, x, u, status, gx, dG, dg0, dCE, dce0, dCI, dci0, nullptr, nullptr,
                    workspace, workspace_bytes, stream);
}

int qpgpu_vjp_box_ws(const qpgpu_problem_desc* d, const double* G, const double* CE, const double* x,
                     const double* u, const int32_t* status, const double* gx, double* dG, double* dg0,
                     double* dCE, double* dce0, double* dhi, double* dlo, void* workspace,
                     int64_t workspace_bytes, void* stream) {
  return vjp_ws_run(d, true, G, CE, nullptr, x, u, status, gx, dG, dg0, dCE, dce0, nullptr, nullptr, dhi, dlo,
                    workspace, workspace_bytes, stream);
}

const char* qpgpu_kernel_name_vjp_ws(int32_t n, int32_t, int32_t) {
  return name_or_empty(qpk_vjp_name(n), qpk_vjp_ws_name(n));
}

// ---- the full backward step: cotangents on u and f too ----------------------------
// The rules and the workspace semantics are vjp_ws_run's; gu and gf may each be NULL.  The kernels
// are the FULL builds of the same sources.
int qpgpu_vjp_full(const qpgpu_problem_desc* d, const double* G, const double* CE, const double* CI,
                   const double* x, const double* u, const int32_t* status, const double* gx,
                   const double* gu, const double* gf, double* dG, double* dg0, double* dCE, double* dce0,
                   double* dCI, double* dci0, void* workspace, int64_t workspace_bytes, void* stream) {
  return vjp_ws_run(d, false, G, CE, CI, x, u, status, gx, dG, dg0, dCE, dce0, dCI, dci0, nullptr, nullptr,
                    workspace, workspace_bytes, stream, true, gu, gf);
}

int qpgpu_vjp_box_full(const qpgpu_problem_desc* d, const double* G, const double* CE, const double* x,
                       const double* u, const int32_t* status, const double* gx, const double* gu,
                       const double* gf, double* dG, double* dg0, double* dCE, double* dce0, double* dhi,
                       double* dlo, void* workspace, int64_t workspace_bytes, void* stream) {
  return vjp_ws_run(d, true, G, CE, nullptr, x, u, status, gx, dG, dg0, dCE, dce0, nullptr, nullptr, dhi, dlo,
                    workspace, workspace_bytes, stream, true, gu, gf);
}

const char* qpgpu_kernel_name_vjp_full(int32_t n, int32_t, int32_t) {
  return name_or_empty(qpk_vjp_full_name(n), qpk_vjp_ws_full_name(n));
}

// ---- forward-mode sensitivities (include/qpgpu.h; kernels: qp_jvp.hip) ---------------
// The rules are sens_rules, decided before any array is read; no workspace, one kernel, so the
// first call for a shape can be captured.
static int jvp_run(const qpgpu_problem_desc* d, bool box, const double* G, const double* CE,
                   const double* CI, const double* x, const double* u, const int32_t* status,
                   const double* tG, const double* tg0, const double* tCE, const double* tce0,
                   const double* tCI, const double* tci0, const double* thi, const double* tlo, double* tx,
                   double* tu, double* tf, void* stream) {
  const int rc = sens_rules(d, box, G, CE, CI, x, u);
  if (rc) return rc;
  // n <= 64: L, M and S of a QP fit on chip
  if (!qpk_jvp_name(d->n) || !vjp_sizes_fit(d)) return QPGPU_ERR_UNSUPPORTED_SHAPE;
  if (d->batch == 0 || (!tx && !tu && !tf)) return QPGPU_SUCCESS;
  const qpk::JvpArgs a = {d->n, d->p, d->m, box ? 1 : 0, d->batch, 0, G, CE, box ? nullptr : CI, x, u, status,
                          tG, tg0, tCE, tce0, box ? nullptr : tCI, box ? nullptr : tci0, box ? thi : nullptr,
                          box ? tlo : nullptr, tx, tu, tf};
  const hipError_t e = qpk_launch_jvp(&a, d->layout == QPGPU_LAYOUT_TILED64, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "kernel launch");
  return QPGPU_SUCCESS;
}

int qpgpu_jvp(const qpgpu_problem_desc* d, const double* G, const double* CE, const double* CI,
              const double* x, const double* u, const int32_t* status, const double* tG, const double* tg0,
              const double* tCE, const double* tce0, const double* tCI, const double* tci0, double* tx,
              double* tu, double* tf, void* stream) {
  return jvp_run(d, false, G, CE, CI, x, u, status, tG, tg0, tCE, tce0, tCI, tci0, nullptr, nullptr, tx, tu, tf,
                 stream);
}

int qpgpu_jvp_box(const qpgpu_problem_desc* d, const double* G, const double* CE, const double* x,
                  const double* u, const int32_t* status, const double* tG, const double* tg0,
                  const double* tCE, const double* tce0, const double* thi, const double* tlo, double* tx,
                  double* tu, double* tf, void* stream) {
  return jvp_run(d, true, G, CE, nullptr, x, u, status, tG, tg0, tCE, tce0, nullptr, nullptr, thi, tlo, tx, tu, tf,
                 stream);
}

const char* qpgpu_kernel_name_jvp(int32_t n, int32_t, int32_t) { return name_or_empty(qpk_jvp_name(n)); }

// ---- K directions on one factorisation (include/qpgpu.h; kernels: qp_jvp_many.hip) ---
// sens_rules, then ntan, then the shape rule: a per-QP block of K directions is indexed with 32 bits.
static int jvp_many_run(const qpgpu_problem_desc* d, int32_t ntan, bool box, const double* G, const double* CE,
                        const double* CI, const double* x, const double* u, const int32_t* status,
                        const double* tG, const double* tg0, const double* tCE, const double* tce0,
                        const double* tCI, const double* tci0, const double* thi, const double* tlo, double* tx,
                        double* tu, double* tf, void* stream) {
  const int rc = sens_rules(d, box, G, CE, CI, x, u);
  if (rc) return rc;
  if (ntan < 1) return QPGPU_ERR_INVALID_ARGUMENT;
  if (!qpk_jvp_many_name(d->n) || !vjp_sizes_fit(d)) return QPGPU_ERR_UNSUPPORTED_SHAPE;
  const int64_t lim = (int64_t)1 << 31, K = ntan, n = d->n;
  if (K * n * n >= lim || K * n * d->p >= lim || K * n * d->m >= lim || K * ((int64_t)d->p + d->m) >= lim)
    return QPGPU_ERR_UNSUPPORTED_SHAPE;
  if (d->batch == 0 || (!tx && !tu && !tf)) return QPGPU_SUCCESS;
  const qpk::JvpManyArgs a = {{d->n, d->p, d->m, box ? 1 : 0, d->batch, 0, G, CE, box ? nullptr : CI, x, u, status,
                               tG, tg0, tCE, tce0, box ? nullptr : tCI, box ? nullptr : tci0, box ? thi : nullptr,
                               box ? tlo : nullptr, tx, tu, tf},
                              ntan};
  const hipError_t e =
      qpk_launch_jvp_many(&a, d->layout == QPGPU_LAYOUT_TILED64, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "kernel launch");
  return QPGPU_SUCCESS;
}

int qpgpu_jvp_many(const qpgpu_problem_desc* d, int32_t ntan, const double* G, const double* CE, const double* CI,
                   const double* x, const double* u, const int32_t* status, const double* tG, const double* tg0,
                   const double* tCE, const double* tce0, const double* tCI, const double* tci0, double* tx,
                   double* tu, double* tf, void* stream) {
  return jvp_many_run(d, ntan, false, G, CE, CI, x, u, status, tG, tg0, tCE, tce0, tCI, tci0, nullptr, nullptr, tx,
                      tu, tf, stream);
}

int qpgpu_jvp_box_many(const qpgpu_problem_desc* d, int32_t ntan, const double* G, const double* CE, const double* x,
                       const double* u, const int32_t* status, const double* tG, const double* tg0,
                       const double* tCE, const double* tce0, const double* thi, const double* tlo, double* tx,
                       double* tu, double* tf, void* stream) {
  return jvp_many_run(d, ntan, true, G, CE, nullptr, x, u, status, tG, tg0, tCE, tce0, nullptr, nullptr, thi, tlo,
                      tx, tu, tf, stream);
}

const char* qpgpu_kernel_name_jvp_many(int32_t n, int32_t, int32_t) { return name_or_empty(qpk_jvp_many_name(n)); }

// Host-pointer entry (the drop-in's path, one QP per solve_quadprog() call, and the batched
// controller's).  Device buffers are one allocation per thread, laid out
//   [G | g0 | CE | ce0 | CI | ci0 | x || f | status | iters]
// (256-B aligned pieces).  Batches up to kStagedBytes go through a pinned host staging buffer of
// the same layout: the inputs are packed on the host, then ONE H2D copy, the launch and ONE D2H
// copy of [x | f | status | iters] (+ G with WRITE_FACTOR) — instead of 7 + 4 pageable copies —
// which is what a 50 ms control cycle's single solves need (latency, tools/dropin_latency.cpp).
// Larger batches copy each array directly (a host-side pack would only add a pass over them).
// Measured for one C1 QP (profiles/r02_s3/latency.log): 41 us p50 staged, 114 us with per-array
// copies.
static constexpr size_t kStagedBytes = 4u << 20;
// Batches up to g_zero_copy_bytes (a few dozen C1 QPs; one drop-in solve_quadprog() call is 2 KB)
// skip both copies: the kernel reads its inputs from, and writes its outputs to, the pinned
// staging buffer itself (mapped host memory), and the call waits for the stream's completion
// once (a hipStreamQuery spin).  Measured per shape, host to host with the factor written
// back as the drop-in asks (profiles/r06_s6/latency_parts.log, copies -> zero-copy): (7, 6, 14)
// 42.6 -> 38.6 us, (14, 10, 28) 85.3 -> 82.0, (30, 6, 60) 214.1 -> 208.2, but (8, 0, 16)
// 61.2 -> 65.1: without an equality phase the first l1 scan waits on the host-memory reads of CI
// at once, so p = 0 calls keep the copies.
static size_t g_zero_copy_bytes = 64u << 10;  // kZeroCopyBytes; qpgpu_debug_set_zero_copy

struct PinnedStage {
  void* buf = nullptr;
  size_t bytes = 0;
  ~PinnedStage() {
    if (buf) (void)hipHostFree(buf);
  }
};
thread_local PinnedStage g_pin;

int qpgpu_solve_batched_host(const qpgpu_problem_desc* d, double* G, const double* g0,
                             const double* CE, const double* ce0, const double* CI,
                             const double* ci0, double* x, double* f, int32_t* status,
                             int32_t* iters) {
  int rc = validate(d);
  if (rc) return rc;
  if (d->batch == 0) return QPGPU_SUCCESS;
  if (!G || !g0 || !x || !f || !status) return QPGPU_ERR_INVALID_ARGUMENT;
  if ((d->p > 0 && (!CE || !ce0)) || (d->m > 0 && (!CI || !ci0)))
    return QPGPU_ERR_INVALID_ARGUMENT;
  if (!family_covers(d->flags, d->n, d->p, d->m)) return QPGPU_ERR_UNSUPPORTED_SHAPE;
  if (qpgpu_device_count() <= 0) {
    g_last_error = "no HIP device visible";
    return QPGPU_ERR_NO_DEVICE;
  }
  const size_t B = (size_t)d->batch, n = d->n, p = d->p, m = d->m;
  // per-QP-block arrays hold whole tiles in the TILED64 layout
  const size_t BB = d->layout == QPGPU_LAYOUT_TILED64 ? (B + 63) / 64 * 64 : B;
  auto al = [](size_t bytes) { return (bytes + 255) & ~(size_t)255; };
  const size_t nG = BB * n * n * 8, ng0 = BB * n * 8, nCE = BB * n * p * 8, nce0 = BB * p * 8,
               nCI = BB * n * m * 8, nci0 = BB * m * 8, nx = BB * n * 8, nf = B * 8, ns = B * 4,
               ni = B * 4;
  // byte offsets of the pieces
  const size_t oG = 0, og0 = oG + al(nG), oCE = og0 + al(ng0), oce0 = oCE + al(nCE),
               oCI = oce0 + al(nce0), oci0 = oCI + al(nCI), ox = oci0 + al(nci0), of = ox + al(nx),
               os = of + al(nf), oi = os + al(ns), total = oi + al(ni);
  hipError_t e;
  int dev = 0;
  if ((e = hipGetDevice(&dev)) != hipSuccess) return hip_fail(e, "hipGetDevice");
  if (g_ws.device != dev || g_ws.bytes < total) {
    if (g_ws.buf) (void)hipFree(g_ws.buf);
    if (g_ws.stream && g_ws.device != dev) {
      (void)hipStreamDestroy(g_ws.stream);
      g_ws.stream = nullptr;
    }
    g_ws.buf = nullptr;
    g_ws.bytes = 0;
    if ((e = hipMalloc(&g_ws.buf, total)) != hipSuccess) return hip_fail(e, "hipMalloc");
    g_ws.bytes = total;
    g_ws.device = dev;
  }
  if (!g_ws.stream) {
    if ((e = hipStreamCreateWithFlags(&g_ws.stream, hipStreamNonBlocking)) != hipSuccess)
      return hip_fail(e, "hipStreamCreate");
  }
  char* base = static_cast<char*>(g_ws.buf);
  auto D = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
  double* dG = D(oG);
  hipStream_t s = g_ws.stream;
  const bool wf = (d->flags & QPGPU_FLAG_WRITE_FACTOR) != 0;
  const bool staged = total <= kStagedBytes;
  // after a failure past the first queued copy, drain the stream before returning so no copy
  // still reads or writes the caller's buffers
  auto fail_drain = [&](hipError_t err, const char* what) {
    (void)hipStreamSynchronize(s);
    return hip_fail(err, what);
  };
  if (staged) {
    if (g_pin.bytes < total) {
      if (g_pin.buf) (void)hipHostFree(g_pin.buf);
      g_pin.buf = nullptr;
      g_pin.bytes = 0;
      if ((e = hipHostMalloc(&g_pin.buf, total, hipHostMallocDefault)) != hipSuccess)
        return hip_fail(e, "hipHostMalloc");
      g_pin.bytes = total;
    }
    char* h = static_cast<char*>(g_pin.buf);
    auto put = [&](size_t off, const void* src, size_t bytes) {
      if (bytes) std::memcpy(h + off, src, bytes);
    };
    put(oG, G, nG);
    put(og0, g0, ng0);
    put(oCE, CE, nCE);
    put(oce0, ce0, nce0);
    put(oCI, CI, nCI);
    put(oci0, ci0, nci0);
    put(ox, x, nx);  // x passes through unchanged on NONPD
    // f | status | iters poisoned (NaN, -1, -1) and sent with the inputs: outputs a kernel did
    // not write never come back as the previous call's values from the reused device buffer
    std::memset(h + of, 0xFF, total - of);
    // the outputs from the staging buffer to the caller's arrays, once the stream has completed
    auto copy_back = [&] {
      std::memcpy(x, h + ox, nx);
      std::memcpy(f, h + of, nf);
      std::memcpy(status, h + os, ns);
      if (iters) std::memcpy(iters, h + oi, ni);
      if (wf) std::memcpy(G, h + oG, nG);
    };
    if (total <= g_zero_copy_bytes && d->p > 0) {
      // zero-copy: the kernel works on the mapped staging buffer directly
      auto Hp = [&](size_t off) { return reinterpret_cast<double*>(h + off); };
      rc = qpgpu_solve_batched(d, Hp(oG), Hp(og0), Hp(oCE), Hp(oce0), Hp(oCI), Hp(oci0), Hp(ox), Hp(of),
                               reinterpret_cast<int32_t*>(h + os), reinterpret_cast<int32_t*>(h + oi), s);
      if (rc) {
        (void)hipStreamSynchronize(s);
        return rc;
      }
      // The outputs are read once the stream has completed (the end-of-kernel release makes every
      // store visible).  Polling the status words instead (the kernel storing x, f, iters, a
      // system-scope fence, then the status; round 6's first form) raced: a status word was seen
      // with x, or the factor's last rows, still the values the host had staged — in the
      // coarse-grained pinned buffer and in a fine-grained one alike (tests/test_gpu_dropin.py::
      // test_eigen_api_matches_oracle, test_single_calls_outputs_fresh; profiles/r06_f6, r06_s26).
      // A hipStreamQuery spin measured slower than the blocking sync (39.2 vs 36.8 us per C1 call,
      // profiles/r06_s27/latency_parts.log).
      if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
      copy_back();
      return QPGPU_SUCCESS;
    }
    if ((e = hipMemcpyAsync(base, h, total, hipMemcpyHostToDevice, s)) != hipSuccess)
      return fail_drain(e, "hipMemcpyAsync H2D");
    rc = qpgpu_solve_batched(d, dG, D(og0), D(oCE), D(oce0), D(oCI), D(oci0), D(ox), D(of),
                             reinterpret_cast<int32_t*>(base + os),
                             reinterpret_cast<int32_t*>(base + oi), s);
    if (rc) {
      (void)hipStreamSynchronize(s);
      return rc;
    }
    if ((e = hipMemcpyAsync(h + ox, base + ox, total - ox, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return fail_drain(e, "hipMemcpyAsync D2H");
    if (wf && (e = hipMemcpyAsync(h + oG, base + oG, nG, hipMemcpyDeviceToHost, s)) != hipSuccess)
      return fail_drain(e, "hipMemcpyAsync D2H");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    copy_back();
    return QPGPU_SUCCESS;
  }
  auto h2d = [&](size_t off, const void* src, size_t bytes) -> hipError_t {
    if (!bytes) return hipSuccess;
    return hipMemcpyAsync(base + off, src, bytes, hipMemcpyHostToDevice, s);
  };
  if ((e = h2d(oG, G, nG)) != hipSuccess || (e = h2d(og0, g0, ng0)) != hipSuccess ||
      (e = h2d(oCE, CE, nCE)) != hipSuccess || (e = h2d(oce0, ce0, nce0)) != hipSuccess ||
      (e = h2d(oCI, CI, nCI)) != hipSuccess || (e = h2d(oci0, ci0, nci0)) != hipSuccess ||
      (e = h2d(ox, x, nx)) != hipSuccess)  // x passes through unchanged on NONPD
    return fail_drain(e, "hipMemcpyAsync H2D");
  // f | status | iters poisoned (NaN, -1, -1), as in the staged path
  if ((e = hipMemsetAsync(base + of, 0xFF, total - of, s)) != hipSuccess) return fail_drain(e, "hipMemsetAsync");
  rc = qpgpu_solve_batched(d, dG, D(og0), D(oCE), D(oce0), D(oCI), D(oci0), D(ox), D(of),
                           reinterpret_cast<int32_t*>(base + os),
                           reinterpret_cast<int32_t*>(base + oi), s);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  auto d2h = [&](void* dst_, size_t off, size_t bytes) -> hipError_t {
    return hipMemcpyAsync(dst_, base + off, bytes, hipMemcpyDeviceToHost, s);
  };
  if (wf && (e = d2h(G, oG, nG)) != hipSuccess) return fail_drain(e, "hipMemcpyAsync D2H");
  if ((e = d2h(x, ox, nx)) != hipSuccess || (e = d2h(f, of, nf)) != hipSuccess ||
      (e = d2h(status, os, ns)) != hipSuccess || (iters && (e = d2h(iters, oi, ni)) != hipSuccess))
    return fail_drain(e, "hipMemcpyAsync D2H");
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
  return QPGPU_SUCCESS;
}

// ---- several GPUs from one process (qpgpu_solve_batched_multi) ---------------------------------
// One persistent worker thread per shard slot: slot k runs shard k's qpgpu_solve_batched_host on
// the device the call names, with that thread's own device buffers, pinned staging and stream
// (the host entry's thread_local state), so a slot's buffers are reused across calls and two
// slots on the same device never share a stream.  Workers are detached and live for the process.
namespace {
struct ShardWorker {
  std::mutex mu;
  std::condition_variable cv;
  std::function<int()> job;
  bool busy = false;
  int rc = 0;
  std::string err;
  ShardWorker() {
    std::thread([this] {
      for (;;) {
        std::function<int()> j;
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [this] { return job != nullptr; });
          j = std::move(job);
          job = nullptr;
        }
        const int r = j();
        const std::string e = r == QPGPU_ERR_HIP ? g_last_error : std::string();
        {
          std::lock_guard<std::mutex> lk(mu);
          rc = r;
          err = e;
          busy = false;
        }
        cv.notify_all();
      }
    }).detach();
  }
  void submit(std::function<int()> j) {
    std::lock_guard<std::mutex> lk(mu);
    busy = true;
    job = std::move(j);
    cv.notify_all();
  }
  int wait(std::string* e) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return !busy; });
    *e = err;
    return rc;
  }
};
std::mutex g_pool_mu;  // one multi-device call at a time owns the pool
// never destroyed: a worker blocks on its condition variable until the process ends
std::vector<ShardWorker*>& g_pool = *new std::vector<ShardWorker*>();
}  // namespace

int qpgpu_solve_batched_multi(const qpgpu_problem_desc* d, int32_t ndev, const int32_t* devices,
                              double* G, const double* g0, const double* CE, const double* ce0,
                              const double* CI, const double* ci0, double* x, double* f,
                              int32_t* status, int32_t* iters) {
  int rc = validate(d);
  if (rc) return rc;
  if (ndev <= 0 || ndev > 64 || !devices) return QPGPU_ERR_INVALID_ARGUMENT;
  const int have = qpgpu_device_count();
  if (have <= 0) {
    g_last_error = "no HIP device visible";
    return QPGPU_ERR_NO_DEVICE;
  }
  for (int k = 0; k < ndev; k++)
    if (devices[k] < 0 || devices[k] >= have) return QPGPU_ERR_INVALID_ARGUMENT;
  if (d->batch == 0) return QPGPU_SUCCESS;
  if (!G || !g0 || !x || !f || !status) return QPGPU_ERR_INVALID_ARGUMENT;
  if ((d->p > 0 && (!CE || !ce0)) || (d->m > 0 && (!CI || !ci0))) return QPGPU_ERR_INVALID_ARGUMENT;
  if (!family_covers(d->flags, d->n, d->p, d->m)) return QPGPU_ERR_UNSUPPORTED_SHAPE;
  const bool tiled = d->layout == QPGPU_LAYOUT_TILED64;
  const int64_t B = d->batch;
  // shard bounds: contiguous, whole tiles in TILED64 (a shard may come out empty)
  std::vector<int64_t> lo(ndev + 1);
  for (int k = 0; k <= ndev; k++) {
    int64_t b = B * k / ndev;
    if (tiled) b = (b + 63) / 64 * 64;
    lo[k] = b < B ? b : B;
  }
  const qpk::QpArgs all = make_args(d, G, g0, CE, ce0, CI, ci0, x, f, status, iters);
  std::lock_guard<std::mutex> pool_hold(g_pool_mu);
  while ((int)g_pool.size() < ndev) g_pool.emplace_back(new ShardWorker());
  std::vector<int> used;
  for (int k = 0; k < ndev; k++) {
    const int64_t cnt = lo[k + 1] - lo[k];
    if (cnt <= 0) continue;
    qpgpu_problem_desc dk = *d;
    dk.batch = cnt;
    const qpk::QpArgs c = qpk::sub_range(all, lo[k], cnt);
    const int dev = devices[k];
    g_pool[k]->submit([=]() -> int {
      hipError_t e = hipSetDevice(dev);
      if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
      return qpgpu_solve_batched_host(&dk, c.G, c.g0, c.CE, c.ce0, c.CI, c.ci0, c.x, c.f, c.status, c.iters);
    });
    used.push_back(k);
  }
  int first = QPGPU_SUCCESS;
  for (int k : used) {
    std::string e;
    const int r = g_pool[k]->wait(&e);
    if (r && !first) {
      first = r;
      if (r == QPGPU_ERR_HIP) g_last_error = "device " + std::to_string(devices[k]) + ": " + e;
    }
  }
  return first;
}

// Diagnostic hook (not in include/qpgpu.h): device buffer of kStampSlots uint64 per wave that
// the next launches fill with s_memtime phase stamps; NULL turns it off.
void qpgpu_debug_set_stamps(void* dev_buf) { g_stamps = static_cast<uint64_t*>(dev_buf); }

// Test / measurement hook (not in include/qpgpu.h): largest host-entry call (bytes of inputs and
// outputs) that runs zero-copy on the mapped staging buffer; 0 = always copy.
void qpgpu_debug_set_zero_copy(int64_t bytes) { g_zero_copy_bytes = bytes > 0 ? (size_t)bytes : 0; }

// Test hook (not in include/qpgpu.h): 0 skips the n > 64 default path's EXACT re-solve of the
// QPs its tolerance mode did not certify, leaving their marks (0x100 | reasons << 9) in status.
extern "C" void qpk_set_resolve(int on);
void qpgpu_debug_set_resolve(int on) { qpk_set_resolve(on); }

// Test hook (not in include/qpgpu.h): 0 makes the n > 64 default path's l1 scans fp64-only
// (no fp32 copy of CI), the A/B side of the shadow scan's bitwise test.
extern "C" void qpk_set_shadow(int on);
void qpgpu_debug_set_shadow(int on) { qpk_set_shadow(on); }
// Diagnostic (not in include/qpgpu.h): out[0] = l1 scans of the n > 64 default path that tried
// the fp32 copy of CI, out[1] = those its bounds settled, out[2] = the fp64 re-evaluations of
// candidates those made, since the last reset (reset != 0 zeroes them after reading).
// Synchronises the current device.
extern "C" hipError_t qpk_shadow_stats(unsigned long long* out, int reset);
int qpgpu_debug_shadow_stats(uint64_t* out, int reset) {
  unsigned long long v[3] = {0, 0, 0};
  const hipError_t e = qpk_shadow_stats(v, reset);
  if (e != hipSuccess) return hip_fail(e, "shadow stats");
  for (int k = 0; k < 3; k++) out[k] = v[k];
  return QPGPU_SUCCESS;
}

// Test hook (not in include/qpgpu.h): the generic kernel's per-launch workspace cap in bytes
// (<= 0 restores the 4 GiB default), so the sub-batch path runs on small shapes.
void qpgpu_debug_set_generic_ws_cap(int64_t bytes) { g_generic_ws_cap = bytes > 0 ? bytes : ((int64_t)4 << 30); }

// Test hook (not in include/qpgpu.h): what the solve entries derive from the addresses of their
// input arrays (alignment_flags; the pointers are only looked at, never read through).  Bit 0: CI
// and ci0 are 16-byte aligned (kArgAligned16); bit 1: G, g0 and, with p > 0, CE and ce0 are
// (kArgStage16).
int qpgpu_debug_alignment_bits(const void* G, const void* g0, const void* CE, const void* ce0,
                               const void* CI, const void* ci0, int32_t p) {
  auto D = [](const void* q) { return static_cast<const double*>(q); };
  const uint32_t f = alignment_flags(D(G), D(g0), D(CE), D(ce0), D(CI), D(ci0), p);
  return ((f & qpk::kArgAligned16) ? 1 : 0) | ((f & qpk::kArgStage16) ? 2 : 0);
}

// Test hook (not in include/qpgpu.h): how many full-wave lane kernels (out[0]) and how many general
// lane kernels for the QPs past the last whole 64-QP block (out[1]) this thread's solves have
// enqueued since the last reset.  A launch that the full-wave kernels do not take — arrays off
// the 16-byte checks, QPGPU_FLAG_WRITE_FACTOR, a pass count asked for — counts in neither.
static thread_local int64_t g_lane_launches[2] = {0, 0};
void qpk_lane_count_launch(int full) { g_lane_launches[full ? 0 : 1]++; }
void qpgpu_debug_lane_launches(int64_t* out, int reset) {
  out[0] = g_lane_launches[0];
  out[1] = g_lane_launches[1];
  if (reset) g_lane_launches[0] = g_lane_launches[1] = 0;
}

int qpgpu_relayout(int64_t batch, int32_t elems, const double* src, double* dst, int32_t to_tiled,
                   void* stream) {
  if (batch < 0 || elems < 0 || (batch > 0 && elems > 0 && (!src || !dst)))
    return QPGPU_ERR_INVALID_ARGUMENT;
  if (batch == 0 || elems == 0) return QPGPU_SUCCESS;
  hipError_t e = qpk_relayout(batch, elems, src, dst, to_tiled ? 1 : 0,
                              reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess) return hip_fail(e, "relayout launch");
  return QPGPU_SUCCESS;
}

}  // extern "C"
