// qp_lane.hip — gfx950 batched Goldfarb–Idnani solver, ONE QP PER LANE (n <= 8, m <= 16).
//
// Restates solve_quadprog() (reference include/QuadProgpp/QuadProg++.hh:69-72; operation order
// of the prebuilt libquadprog.a fixed in SURVEY.md §3.2) for the 64 QPs of one wavefront.
//
// Why one QP per lane: at these sizes the cost is the serial chain of every QP (Givens
// coefficients = 4 IEEE divisions + 1 sqrt each, back-substitutions, step lengths); running it
// once per QP instead of once per lane of a subgroup cuts issued instructions ~4x versus
// qp_small.hip.  65 536 QPs are exactly one wave per SIMD (1 024 SIMDs), so a launch is as long
// as its slowest wave and every wave's latency is exposed.  State placement (gfx950: 512
// VGPR+AGPR per lane at 1 wave/SIMD, 160 KiB LDS per CU = 40 KiB per wave at 4 waves/CU):
//   * J (= L^{-T}), R (upper triangle + first subdiagonal, the only entries the algorithm makes
//     non-zero), x, z, d, np, u, r, A, s and the loop's rollback copies live in registers for
//     the whole solve, indexed only with compile-time indices (fully unrolled loops with
//     run-time predicates);
//   * G, g0, CE, ce0 are brought in by LDS-DMA (global_load_lds_dwordx4) of the wave's 64
//     contiguous QP blocks into a 40 KiB staging buffer and read per lane from it;
//   * CI / ci0 (QP-major EXACT shapes): the first l1 scan reads them from global memory (their
//     cache lines were touched during the equality phase) and leaves them on chip — rows
//     0..kCiRows-1 in the LDS staging buffer, and (C1-sized shapes with an equality phase) the
//     remaining rows and ci0 in AGPRs — so later scans and the selected-column gathers issue no
//     global loads at all.
// IEEE binary64 throughout, no contraction: results are bitwise identical to the CPU
// restatement (oracle/qp_oracle.c), which tests/ check.
//
// The same source built a second time with QPGPU_LANE_FAST=1 and -ffp-contract=fast
// (qp_lane_fast.hip) is the QPGPU_FLAG_FAST kernel: same algorithm and decisions, but multiply-
// adds fused, every division by a shared divisor a multiplication by one refined reciprocal
// (Cholesky columns, J = L^-T, the solve, the Givens coefficients), and the rotation length as
// sqrt(a^2 + b^2) for operands well inside the exponent range — within north_star's 1e-10
// relative of the reference instead of bit-identical.
//
// Seven objects are built from this source: qp_lane.o and qp_lane_p0.o (the exact aligned build in
// two parts), qp_lane_fast.o, the unaligned twins qp_lane_u.o and qp_lane_fast_u.o, and the unit-
// Hessian qp_lane_unit.o and qp_lane_unit_u.o.  Their wrapper sources set the macros below, which
// choose the namespace, the kernel's name, the entry's suffix and the branches inside lane_body.
// What an object holds beyond that is a few constexpr facts beside kFast; the one launcher at the
// end of the file selects on them, over the size classes of QPK_LANE_SIZES (qp_common.h), and the
// kernel names are a host table over the same list (qpgpu_api.cpp kernel_name).  DESIGN §5.14.
#include <type_traits>
#include <utility>

#include "qp_common.h"

#ifndef QPGPU_LANE_FAST
#define QPGPU_LANE_FAST 0
#endif
// The same source built again with QPGPU_LANE_UNALIGNED=1 (qp_lane_u.hip, qp_lane_fast_u.hip) is
// what the host launches when G, g0, CE or ce0 is not 16-byte aligned (include/qpgpu.h asks for
// natural alignment only): G, g0, CE and ce0 then reach the LDS staging buffer by per-lane 8-byte
// copies instead of 16-byte LDS-DMA, everything else is the same code and the same arithmetic.
// A build of its own, not a branch in these kernels: with the branch in place several N = 8
// instantiations, which sit at the 512-register limit, gained scratch
// (profiles/placement/kernel_regs_branch_in_kernel.txt), while this way the aligned kernels are
// the code they were.  All of its instantiations share one translation unit.
#ifndef QPGPU_LANE_UNALIGNED
#define QPGPU_LANE_UNALIGNED 0
#endif
// The same source built with QPGPU_LANE_UNIT=1 (qp_lane_unit.hip, qp_lane_unit_u.hip) is the
// kernel of qpgpu_solve_batched_unit: the Hessian is the identity, so the setup is stated instead
// of computed — J = I, c1 = c2 = the sum of n ones, x0 = -g0, f0 = 0.5 sum g0[i] x0[i] — and a.G is
// never read.  Only the run-time-shape instantiations, which carry the m = 0
// snapshot, are built, in namespaces of their own: the kernels of the other builds are the code
// they were.
#ifndef QPGPU_LANE_UNIT
#define QPGPU_LANE_UNIT 0
#endif
#if QPGPU_LANE_UNIT && QPGPU_LANE_FAST
#error "the unit-Hessian lane kernels restate the reference's operation order only"
#endif
// The exact aligned build is two objects: its p = 0 instantiations (C2, the joint-limit QPs) are
// compiled in qp_lane_p0.hip (QPGPU_LANE_PART = 2) under LLVM's iterative-minreg scheduler, the
// rest in qp_lane.o (QPGPU_LANE_PART = 1, Makefile DEFS_qp_lane) under iterative-ilp: measured C2
// 71.2-71.9 -> 68.6-69.1 us with minreg, while C1 is slower with it (43.7-44.7 -> 46.1-47.9 us;
// profiles/r05_s11).  Part 1's launcher forwards p = 0 to part 2's entry, qpk_launch_lane_p0.
// Part 0 (every other build, A/B builds) keeps all of its instantiations in one object.
#ifndef QPGPU_LANE_PART
#define QPGPU_LANE_PART 0
#endif
#if QPGPU_LANE_PART && (QPGPU_LANE_FAST || QPGPU_LANE_UNALIGNED || QPGPU_LANE_UNIT)
#error "only the exact aligned build is split into parts"
#endif
// The preprocessor's share of a build: the namespace, the kernel's name and the suffix of the
// exported entry.  Everything else a build is or lacks is a constexpr fact below (kPart ...).
#if QPGPU_LANE_PART == 2
#define QPK_LANE_NS qpk
#define QP_LANE_KERNEL qp_lane_kernel
#define QPK_LANE_C(name) name##_p0
#elif QPGPU_LANE_UNIT && QPGPU_LANE_UNALIGNED
#define QPK_LANE_NS qpk_unit_u
#define QP_LANE_KERNEL qp_lane_unit_kernel
#define QPK_LANE_C(name) name##_unit_u
#elif QPGPU_LANE_UNIT
#define QPK_LANE_NS qpk_unit
#define QP_LANE_KERNEL qp_lane_unit_kernel
#define QPK_LANE_C(name) name##_unit
#elif QPGPU_LANE_FAST && QPGPU_LANE_UNALIGNED
#define QPK_LANE_NS qpk_fast_u
#define QP_LANE_KERNEL qp_lane_fast_kernel
#define QPK_LANE_C(name) name##_fast_u
#elif QPGPU_LANE_FAST
#define QPK_LANE_NS qpk_fast
#define QP_LANE_KERNEL qp_lane_fast_kernel
#define QPK_LANE_C(name) name##_fast
#elif QPGPU_LANE_UNALIGNED
#define QPK_LANE_NS qpk_u
#define QP_LANE_KERNEL qp_lane_kernel
#define QPK_LANE_C(name) name##_u
#else
#define QPK_LANE_NS qpk
#define QP_LANE_KERNEL qp_lane_kernel
#define QPK_LANE_C(name) name
#endif

// Diagnostic s_memtime stamps (tools/stamps.py): compiled in (QPGPU_LANE_STAMPS = 1), each one a
// wave-uniform null test of a.stamps unless a stamp buffer is passed; 0 removes them (measured
// the same C1 time either way, profiles/r05_s8), 2 adds the loop's l2a split.
#ifndef QPGPU_LANE_STAMPS
#define QPGPU_LANE_STAMPS 1
#endif
#if defined(QPGPU_LANE_OCC2) || defined(QPGPU_LANE_DMA_P0) || defined(QPGPU_LANE_CE_LATE) ||       \
    defined(QPGPU_LANE_WARMUP) || defined(QPGPU_LANE_LOOPTOP_EXIT) || defined(QPGPU_LANE_FULL) || \
    defined(QPGPU_LANE_AB_C1ONLY) || defined(QPGPU_LANE_AB_N8P0ONLY)
#error "retired build switch: its default is folded into qp_lane.hip; the other side is an earlier revision (DESIGN 5.15, tools/ab_build.sh SRCFILE=)"
#endif

// part 2's entry, which part 1's launcher calls (between the two objects only, so declared here)
extern "C" hipError_t qpk_launch_lane_p0(const qpk::QpArgs* a, hipStream_t stream);

namespace QPK_LANE_NS {
using namespace qpk;
constexpr bool kFast = QPGPU_LANE_FAST != 0;
// What this object holds, for the launcher at the end of the file (lane_body reads the macros):
constexpr bool kUnit = QPGPU_LANE_UNIT != 0;
constexpr int kPart = QPGPU_LANE_PART;
// the compile-time-shape instantiations <EXACT = true>; the unit builds have the run-time shape only
constexpr bool kFixedShapes = !kUnit;
// the dual, box and box-dual kernels: the exact builds', with part 1 where the build is split
constexpr bool kHasModes = !kFast && !kUnit && kPart != 2;
// the full-wave kernels of (7, p, 14), p = 6 and p = 0: the exact aligned build's
constexpr bool kHasFull = !kFast && !kUnit && QPGPU_LANE_UNALIGNED == 0;
// the plain kernel <EXACT, PX>: part 2 holds <true, 0> and nothing else, part 1 all but that one
constexpr bool has_plain(bool exact, int px) {
  const bool p0 = exact && px == 0;
  return (!exact || kFixedShapes) && (kPart == 0 || (kPart == 2) == p0);
}
constexpr bool kStamps = QPGPU_LANE_STAMPS != 0;
__device__ __forceinline__ void lstamp(const QpArgs& a, int slot) {
  if constexpr (kStamps) qp_stamp(a, slot);
}

// opq_l, lsel_lo, lsel, lput_lo, RIdx, wave_any: qp_common.h (shared with qp_pair.hip)

// A double parked in two AGPRs.  VALU cannot operate on AGPRs, but v_accvgpr_read/write move a
// dword in one issue slot, far cheaper than the L2 / Infinity-Cache round trip the scan would
// otherwise pay; the "a" constraints make the register allocator keep these values in the
// accumulator half of the unified file, which the C1 kernel leaves mostly unused.  The reads
// are volatile so that they stay where the values are consumed (a hoisted read would move the
// value back into a VGPR for the whole loop).
struct AgprD {
  uint32_t lo, hi;
};
__device__ __forceinline__ AgprD to_agpr(double v) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  AgprD a;
  asm("v_accvgpr_write_b32 %0, %1" : "=a"(a.lo) : "v"((uint32_t)u));
  asm("v_accvgpr_write_b32 %0, %1" : "=a"(a.hi) : "v"((uint32_t)(u >> 32)));
  return a;
}
__device__ __forceinline__ double from_agpr(const AgprD& a) {
  uint32_t lo, hi;
  asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(lo) : "a"(a.lo));
  asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(hi) : "a"(a.hi));
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

constexpr int kQpw = 64;      // QPs per wave: one per lane
// One wave per SIMD: 512 registers per lane and a 40 KiB stage, four waves per CU.  Two waves per
// SIMD (256 registers, a 20 KiB stage, G and CE loaded per lane from global memory) measured
// 85.5 us against 40.4 on C1 and was not kept.
constexpr int kLaneOcc = 1;
constexpr int kStage = 5120;  // staging buffer, doubles (40 KiB: 4 waves per CU)
// The first l1 scan (which fills the on-chip CI copy) is software-pipelined two rows deep: row
// j+1's loads are issued (and fenced from the scheduler) before row j is consumed, so one memory
// latency covers two rows instead of the scheduler's one-load-at-a-time minimum-pressure order.
constexpr int kScanDepth = 2;
// The staging buffer as the LDS-DMA sees it.  The kernels cast their __shared__ array to LdsD
// where it is declared (a constant the compiler folds) and lane_body keeps that pointer for the
// copies' destinations: a generic pointer cast to address space 3 at each copy is a run-time
// generic -> local conversion, which the compiler guards with a null test ahead of every M0 write.
using LdsD = __attribute__((address_space(3))) double;
using LdsC = __attribute__((address_space(3))) char;
using LdsV = __attribute__((address_space(3))) void;
using GlobalV = __attribute__((address_space(1))) void;
// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in that order: the LDS-DMA
// builtin's offset is an immediate of the instruction, so a chunk or piece index that reaches it
// has to be a constant expression (a fully unrolled loop's counter is not one).
template <int... K, class F>
__device__ __forceinline__ void for_seq_impl(std::integer_sequence<int, K...>, F&& f) {
  (f(std::integral_constant<int, K>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void for_seq(F&& f) {
  for_seq_impl(std::make_integer_sequence<int, N>{}, f);
}
// Choices of the staging that measurements settled (the other sides: DESIGN §5.15):
//   * p = 0 (no equality phase): the first scan loads the CI rows, no DMA copies them into LDS.
//     Measured on C2 (profiles/r03_s6): 83.6 us with the DMA at the end of the setup, 72.9
//     without — the DMA's per-lane 16-B pieces take ~23k cycles per wave to issue, the first
//     scan's direct loads 18.5k, and nothing hides either; a part per Cholesky row measured 75.2 us
//     per launch against 67.6-68.0 (profiles/r06_s15).  With p > 0 the equality phase hides the DMA.
//   * The DMA path does not touch the CI rows past the LDS copy and ci0 ahead of the first scan,
//     which loads them (the product since round 5).  Measured on C1 (profiles/r05_s3): FETCH
//     146.4 / 125.0 / 130.1 MB for a touch after the CE -> AGPR move (rounds 3-4) / none / one at
//     the last equality step — the touched lines leave L2 before the first scan reads them, so the
//     touch only adds a second fetch — at 44.6 / 44.8 / 45.7 us (two runs each; the first two
//     within the run-to-run spread).
//   * The setup waits for round B (CE / ce0 into LDS) after J = L^-T and the solve, which need
//     only the factor, not right after the Cholesky (rounds 1-4).
//   * The fast build checks for an invalid fast form at the top of every loop pass as well (the
//     product since round 5), not only after the equality phase and after the loop.  Round 4
//     dropped the check after a wrong-result run that no committed source reproduces (DESIGN §5.6,
//     profiles/r05_s2, r05_s3).

// ---- arithmetic of the fast build (frcp, rcp_ok, ldiv_r, ldiv, ldistance): qp_common.h,
// shared with the lane-pair kernel (qp_pair.hip).

// What lane_body's kResident kernel keeps on the lane through its loop: the CI rows past the LDS copy
// (VGPRs), ci0 and the rollback copy of x (AGPRs).  Three unused bytes in every other instantiation.
template <bool ON, int ROWS, int NM, int MM>
struct LaneResident {
  double kept[ROWS][MM];
  AgprD ci0_ag[MM], xold_ag[NM];
};
template <int ROWS, int NM, int MM>
struct LaneResident<false, ROWS, NM, MM> {
  char kept, ci0_ag, xold_ag;
};

// One l1 pass of the kernel that keeps the late CI rows on the lane (lane_body's kResident, the
// QP-major one-free full-wave kernel): s = CI^T x + ci0 with rows 0..ROWS-1 of CI from the LDS
// copy, rows ROWS..NM-1 from the VGPRs kept[0..NM-ROWS) and ci0 from the AGPRs ci0_ag (the select
// never reads ci0, so it is read back once per scan, into the registers the LDS rows have left).
// LOAD (the first pass, peeled out of the loop) fills both from global memory first, as dwordx4
// under the scan's own predicate; later passes issue no global load.  The same sums in the same
// order as lane_body's scan_pass: every s[i] sums j ascending from 0.0, then + ci0[i]; psi and
// the optimality test are scan_pass's.
// The LDS rows are read one row ahead of their sums and fenced from the scheduler.  Left alone
// it issues all ROWS rows' reads at once, and with the kept rows live across the whole loop the
// allocator then moves column NM - 1 of J through AGPRs, in the loop and in every step of the
// equality phase.  The first pass reads no row ahead: it waits for its global loads anyway, and
// ci0 is still in VGPRs there.
template <int NM, int MM, int ROWS, bool LOAD>
__device__ __forceinline__ void lane_scan_kept(const double* sbuf, int lane, const double* CIg, const double* ci0g,
                                               const double (&xv)[NM], double (&kept)[NM - ROWS][MM],
                                               AgprD (&ci0_ag)[MM], double (&sv)[MM], double c1, double c2,
                                               bool need_scan, bool& active, int& iter, uint64_t& excl, double& ss,
                                               int& ip) {
  const bool do_scan = active && need_scan;
  if (!wave_any(do_scan)) return;
  if (do_scan) {
    iter++;
    double c0[MM];
    if constexpr (LOAD) {
#pragma unroll
      for (int r = ROWS; r <= NM; r++) {
        const double* src = r < NM ? CIg + r * MM : ci0g;
#pragma unroll
        for (int i = 0; i < MM; i += 2) {
          const double2 v = *reinterpret_cast<const double2*>(src + i);
          (r < NM ? kept[r < NM ? r - ROWS : 0][i] : c0[i]) = v.x;
          (r < NM ? kept[r < NM ? r - ROWS : 0][i + 1] : c0[i + 1]) = v.y;
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int i = 0; i < MM; i++) sv[i] = 0.0;
    constexpr int AHEAD = LOAD ? 0 : 1;
    double2 row[2][MM / 2];
    auto ldrow = [&](int j, double2(&dst)[MM / 2]) {
#pragma unroll
      for (int i = 0; i < MM; i += 2)
        dst[i / 2] = *reinterpret_cast<const double2*>(sbuf + (((j * MM + i) >> 1) * kQpw + lane) * 2);
    };
#pragma unroll
    for (int j = 0; j < AHEAD; j++) ldrow(j, row[j % 2]);
#pragma unroll
    for (int j = 0; j < NM; j++) {
      const double xj = xv[j];
      if (j + AHEAD < ROWS) ldrow(j + AHEAD, row[(j + AHEAD) % 2]);
      if constexpr (!LOAD) {
        if (j == ROWS) {
#pragma unroll
          for (int i = 0; i < MM; i++) c0[i] = from_agpr(ci0_ag[i]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (j < ROWS) {
#pragma unroll
        for (int i = 0; i < MM; i += 2) {
          sv[i] += row[j % 2][i / 2].x * xj;
          sv[i + 1] += row[j % 2][i / 2].y * xj;
        }
      } else {
#pragma unroll
        for (int i = 0; i < MM; i++) sv[i] += kept[j >= ROWS ? j - ROWS : 0][i] * xj;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    double psi = 0.0;
#pragma unroll
    for (int i = 0; i < MM; i++) {
      sv[i] += c0[i];
      psi += (sv[i] < 0.0) ? sv[i] : 0.0;
    }
    if constexpr (LOAD) {
#pragma unroll
      for (int i = 0; i < MM; i++) ci0_ag[i] = to_agpr(c0[i]);
    }
    excl = 0;
    ss = 0.0;
    ip = 0;
    if (fabs(psi) <= (double)MM * kEps * c1 * c2 * 100.0) active = false;  // optimal
  }
}

// PX >= 0: p is the compile-time constant PX as well (C1/C4: 6, C2: 0), which folds every
// [p, iq) loop of the active-set phase (for n = 7, p = 6 that range holds at most one entry).
// The solve of one wave's 64 QPs.  SAFE: the IEEE forms of division and distance (the exact
// build always; the fast build's fallback).  Returns false as soon as a fast form was not
// valid for some lane (checked after the equality phase and after the loop): x, f, status
// and iters are not written then, and the caller re-solves the wave with SAFE, which rewrites
// everything — including the m = 0 snapshot (x_eq, f_eq, st_eq) the fast attempt may already
// have written.  In the fast build (-ffp-contract=fast) the SAFE body's multiply-adds are
// contracted too: a fallback wave keeps the reference's divisions and distance(), not its
// bitwise results (still within 1e-10).
// DUAL (qpgpu_solve_batched_dual; the exact build's general instantiation only): r and u are
// carried over the whole active set — the equality phase runs the reference's update_r and its
// u[:iq] update, the loop's update_r and u update start at row 0 — and the multipliers leave
// through a.u / a.nact.  t1, the drop choice and the rollback still look at the inequalities
// only, so x, f, status and the l1 passes are the same bits.  With BOX (qpgpu_solve_batched_box_dual)
// both box forms carry it; with p = 0 the loop is the box kernel's and only the epilogue is added.
// BOX (qpgpu_solve_batched_box; the exact build only): the inequalities are lo <= x <= hi, i.e.
// CI = [-I, +I] and ci0 = [hi; -lo] never materialised (m = 2n).  The bounds b = [hi; -lo] live in
// 2 NM registers and so does s, both at compile-time positions: the upper bound of variable v at v,
// the lower at NM + v (constraint index v and n + v).  The reference's sums over a column of CI
// reduce to their one non-zero term added to the +0.0 the sum starts from: the l1
// scan is (0.0 -+ x[v]) + b, d = J^T np is 0.0 -+ J[v][:], z.np is 0.0 -+ z[v].  No CI copy in LDS,
// no DMA staging, no cache warm-up, no CI / ci0 load of any kind.
// FULL (the exact aligned build's EXACT shapes with PX known; qp_lane_full_kernel): the host has
// established that every wave of the launch is full, that G, g0, CE and ce0 pass the 16-byte
// staging check (kArgStage16) and CI and ci0 theirs (kArgAligned16), that the factor is not
// written back and that no pass count is asked for.  live, full, dma, ce_staged, ce_agpr, ci_lds
// and vec are then constants: the `live ?:` selects, the partial wave's per-lane staging, the
// LDS and global sources of CE and the scalar CI row loads leave the code, and with them their
// branches.  The arithmetic is the same operations in the same order.
template <int NM, int MM, int T, bool EXACT, int PX, bool SAFE, bool DUAL = false, bool BOX = false,
          bool FULL = false>
__device__ __forceinline__ bool lane_body(const QpArgs& a, LdsD* lds) {
  double* const sbuf = (double*)lds;  // the LDS reads and the per-lane copies (LDS-DMA: lds)
  static_assert(MM <= 64, "bitmask bookkeeping holds m <= 64");
  static_assert(!BOX || (!kFast && MM == 2 * NM), "the box mode is the exact build's, m = 2n");
  static_assert(!FULL || (!kFast && !QPGPU_LANE_UNALIGNED && EXACT && PX >= 0 && !DUAL && !BOX),
                "the full-wave form is the exact aligned build's, for a compile-time shape");
  static_assert(!DUAL || (!kFast && (BOX || (!EXACT && PX < 0))),
                "the dual mode is the exact build's general instantiation, or a box form");
  using RI = RIdx<NM>;
  constexpr int STAGE = kStage;
  constexpr bool F = kFast && !SAFE;
  bool fok = true;  // F: every fast form so far was valid on this lane
  // CI / ci0 cache warm-up before the equality phase: only with an equality phase long enough
  // for the loads to land (p > 0 or p unknown).  Measured for p = 0 (no equality phase): the
  // first scan then waits on the same burst either way (profiles/r02_s2, r02_s46).
  constexpr bool kLanePrefetch = PX != 0 && !BOX;

  const int lane = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * kQpw;
  const int64_t b = b0 + lane;
  const int valid = (int)min<int64_t>(kQpw, a.batch - b0);
  const bool live = FULL || lane < valid;

  // EXACT: the shape is (NM, *, MM), so every element offset is a compile-time constant
  const int n = EXACT ? NM : a.n;
  const int m = EXACT ? MM : a.m;
  const int p = PX >= 0 ? PX : a.p;
  const double inf = dinf();

  // The wave's 64 QPs occupy [X + b0*E, X + (b0+64)*E) in both layouts (TILED64 arrays hold
  // whole tiles, so its waves are always full).  Staging copies a contiguous span of that
  // range into sbuf with LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave-instruction, no
  // VGPRs, everything in flight at once); a partial last QP-major wave copies per lane.  Each
  // DMA piece is a 16-byte load from X + b0*E + 2*lane + k: 16-byte aligned exactly when X is
  // (b0*E*8 is a multiple of 512).  The host checks that for G, g0, CE and ce0 (kArgStage16) and
  // launches these kernels only then; otherwise it launches the QPGPU_LANE_UNALIGNED build, where
  // every wave copies per lane, 8 bytes at a time, in both layouts.  (Preprocessor, not
  // `if constexpr`: the unaligned build stages G, g0, CE and ce0 by stage_all's per-lane copy
  // alone and never reaches copy_span; its CI copy, dma_ci_part, is the aligned build's.)
#if QPGPU_LANE_UNALIGNED
  const bool full = false;
#else
  const bool full = FULL || (T == 64) || (valid == kQpw);
#endif
  // Chunk J (0..3) of the run of chunks that starts at double k0 of a span: doubles
  // [k0 + 128 J, k0 + 128 J + 128).  J goes in the instruction's immediate offset, which the
  // hardware adds to the global address and to the LDS address (M0 + offset + 16 * lane) alike:
  // both strides are 1 KiB here, so the chunks of a run share one per-lane source address and one
  // M0, and four chunks fit the 13-bit signed immediate.  The lanes past the span's end load from
  // src instead: with the immediate that is the first piece of the span's own chunk J, which lies
  // inside the span whenever chunk J of any run is issued.
  auto copy_chunk = [&](auto J, const double* src, int nd, int off, int k0) {
    constexpr int j = decltype(J)::value;
    static_assert(j >= 0 && j * 1024 < 4096, "the chunk's offset is the instruction's immediate");
    const int e = k0 + 2 * lane;
    __builtin_amdgcn_global_load_lds((const GlobalV*)(e + j * 128 < nd ? src + e : src),
                                     (LdsV*)(lds + off + k0), 16, j * 1024, 0);
  };
  auto copy_run = [&](const double* src, int nd, int off, int k0) {  // the chunks of [k0, k0 + 512)
    copy_chunk(std::integral_constant<int, 0>{}, src, nd, off, k0);
    if (k0 + 128 < nd) copy_chunk(std::integral_constant<int, 1>{}, src, nd, off, k0);
    if (k0 + 256 < nd) copy_chunk(std::integral_constant<int, 2>{}, src, nd, off, k0);
    if (k0 + 384 < nd) copy_chunk(std::integral_constant<int, 3>{}, src, nd, off, k0);
  };
  // The full-wave kernels unroll the span into its runs (straight-line code, every test folded).
  // The others keep the loop over single chunks: unrolled or run-wise spans grew their static size
  // and the scratch of some N = 8 instantiations (profiles/lane_dma/isa_census.txt).
  auto copy_span = [&](const double* src, int nd, int off) {  // nd even, full waves only
    if constexpr (FULL) {
#pragma unroll
      for (int k0 = 0; k0 < nd; k0 += 512) copy_run(src, nd, off, k0);
    } else {
#pragma unroll 4
      for (int k = 0; k < nd; k += 128) copy_chunk(std::integral_constant<int, 0>{}, src, nd, off, k);
    }
  };
  // whole tile of X (E doubles per QP) -> sbuf[off...]
#if QPGPU_LANE_UNALIGNED
  auto stage_all = [&](const double* X, int E, int off) {
    if constexpr (T == 64) {
      // (the tile is whole: the padding slots of a last tile are copied as the DMA copies them)
      const double* src = X + b0 * (int64_t)E + lane;
      for (int e = 0; e < E; e++) sbuf[off + e * kQpw + lane] = src[e * kQpw];
    } else if (live) {
      const double* src = X + b * (int64_t)E;
      for (int e = 0; e < E; e++) sbuf[off + lane * E + e] = src[e];
    }
  };
  (void)copy_span;  // (no DMA in this build)
#else
  auto stage_all = [&](const double* X, int E, int off) {
    if (full) {
      copy_span(X + b0 * (int64_t)E, kQpw * E, off);
    } else if (live) {
      const double* src = X + b * (int64_t)E;
      for (int e = 0; e < E; e++) sbuf[off + lane * E + e] = src[e];
    }
  };
#endif
  auto rd_all = [&](int off, int E, int k) -> double {
    if constexpr (T == 64)
      return sbuf[off + k * 64 + lane];
    else
      return sbuf[off + lane * E + k];
  };
  auto view = [&](double* X, int E) -> double* {
    if constexpr (T == 64)
      return X + b0 * (int64_t)E + lane;
    else
      return X + b * (int64_t)E;
  };

  int status = QPGPU_QP_OK;
  double fval = 0.0;
  int iter = 0;
  double xv[NM];
#pragma unroll
  for (int i = 0; i < NM; i++) xv[i] = 0.0;
  double c1 = 0.0, c2 = 0.0;
  // LDS regions: the bottom of the buffer stages G (setup), then CE / ce0 (equality phase),
  // then rows 0..kCiRows-1 of every lane's CI for the active-set loop (16-B pieces, piece k of
  // lane l at doubles (k*64 + l)*2).  RB, at the top, stages g0.
  constexpr int RB = (STAGE - kQpw * NM) / 2 * 2;
  // G and g0 stage through LDS
  static_assert(RB >= kQpw * NM * NM, "G and g0 staging exceed the stage buffer");
  // CI rows held in LDS through the loop (EXACT QP-major shapes)
  constexpr int kCiRowsFit = (RB / kQpw) / MM;
  constexpr int kCiRows = (!BOX && EXACT && T == 1 && MM % 2 == 0) ? (kCiRowsFit < NM ? kCiRowsFit : NM) : 0;
  // Rows 0..kCiRows-1 of every lane's CI go straight from HBM into that LDS copy by per-lane
  // LDS-DMA while the setup / equality phase computes (kCiDma: p compile-time, CI 16-B aligned),
  // so the first l1 scan finds them on chip instead of re-reading all of CI from the Infinity
  // Cache after a cache warm-up (that re-read was 11k of a wave's ~88k cycles, profiles/r03_s3).
  // With p > 0 the CE / ce0 staging occupies the LDS then, so once it has landed it moves to
  // AGPRs (ceag, read back once per equality step) and the DMA takes its place.
  // With p = 0 there is no equality phase to hide the copy behind: the first scan loads the rows.
  constexpr bool kCiDma = kCiRows > 0 && PX > 0;
  constexpr int kCeN = PX > 0 ? NM * PX + PX : 1;  // CE (n x p) then ce0 (p)
  [[maybe_unused]] AgprD ceag[kCiDma ? kCeN : 1];
  const bool dma = kCiDma && (FULL || (a.flags & kArgAligned16));
  double Jreg[NM][NM];  // J lives in registers for the whole solve
  bool ce_staged = false;
  bool ce_agpr = false;
  // cache warm-up: one dword per 128-B line of this lane's CI / ci0 blocks — with kCiDma only
  // the rows past the LDS copy (which the scans keep reading from L2)
  constexpr int kPfCI = (NM * MM * 8 + 127) / 128 + 1, kPfC0 = (MM * 8 + 127) / 128 + 1;
  [[maybe_unused]] uint32_t pf[kPfCI + kPfC0];
  bool warmed = false;  // the warm-up loads were issued (they retire after the equality phase)
  auto warmup = [&]() {
    warmed = true;
    if (live) {
      const int off = dma ? kCiRows * MM * 8 : 0;  // (repeats the last line when shorter)
      const char* c = reinterpret_cast<const char*>(a.CI + b * (int64_t)(n * m)) + off;
      const char* c0 = reinterpret_cast<const char*>(a.ci0 + b * (int64_t)m);
      const int bc = n * m * 8 - off, b0c = m * 8;
#pragma unroll
      for (int k = 0; k < kPfCI; k++)
        pf[k] = (bc >= 4) ? *reinterpret_cast<const uint32_t*>(c + min(k * 128, bc - 4)) : 0u;
#pragma unroll
      for (int k = 0; k < kPfC0; k++)
        pf[kPfCI + k] = (b0c >= 4) ? *reinterpret_cast<const uint32_t*>(c0 + min(k * 128, b0c - 4)) : 0u;
    }
  };
  // rows 0..kCiRows-1 of this lane's CI block -> LDS piece k at doubles (k*64 + lane)*2 (the
  // scans' layout): one global_load_lds_dwordx4 per 16-B piece, a per-lane source address and
  // the wave-uniform LDS base.  Lanes past the batch copy lane 0's block (never read).  Issued
  // part by part between compute steps (part `part` of `parts`): all 35 pieces at once stall
  // the wave's issue until HBM has delivered most of them (the CU's memory queues fill), which
  // serialised the whole CI transfer with the setup (+25k cycles per wave, profiles/r03_s4).
  // The piece index goes in the instruction's immediate offset (16 k bytes: the global stride),
  // which the hardware adds to the LDS address as well, where the stride is 1 KiB: piece k's LDS
  // base is k * (1024 - 16).  One per-lane source address serves every piece of every part.
  constexpr int kCiPieces = kCiRows * MM / 2;
  static_assert(kCiPieces * 16 <= 4096, "the piece's offset is the instruction's immediate");
  auto dma_ci_part = [&](int part, int parts) {
    const int per = (kCiPieces + parts - 1) / parts;
    const double* src = a.CI + (live ? b : b0) * (int64_t)(NM * MM);
    for_seq<kCiPieces>([&](auto K) {
      constexpr int k = decltype(K)::value;
      if (k >= part * per && k < (part + 1) * per)
        __builtin_amdgcn_global_load_lds((const GlobalV*)src, (LdsV*)((LdsC*)lds + k * (kQpw * 16 - 16)), 16,
                                         16 * k, 0);
    });
  };
  lstamp(a, 0);
  // BOX: b = [hi; -lo] at the positions above, loaded first so that the setup hides the latency
  [[maybe_unused]] double bv[BOX ? MM : 1];
  if constexpr (BOX) {
    const double* hib = view(const_cast<double*>(a.hi), n);
    const double* lob = view(const_cast<double*>(a.lo), n);
#pragma unroll
    for (int v = 0; v < NM; v++) {
      const double h = (live && v < n) ? hib[v * T] : 0.0;
      const double l = (live && v < n) ? lob[v * T] : 0.0;
      bv[v] = h;
      bv[NM + v] = -l;
    }
  }

  // ---------------------------------------------------------------- setup
  bool chol_ok = live;  // idle lanes (past the batch) never touch LDS slots
  double bad_sum = 0.0;
  {
#if !QPGPU_LANE_UNIT
    double Gr[NM][NM];
#endif
    // round A: G and g0 (the unit build: g0 only)
    const int offg0 = RB;
#if !QPGPU_LANE_UNIT
    stage_all(a.G, n * n, 0);
#endif
    stage_all(a.g0, n, offg0);
    __syncthreads();
    // The LDS reads are unconditional (in range for every lane; an idle lane's slot holds stale
    // data that the select drops): a read under `live` becomes one exec-masked block per element,
    // which the scheduler can neither pair nor overlap.
    double g0v[NM];
#pragma unroll
    for (int i = 0; i < NM; i++) {
#if !QPGPU_LANE_UNIT
#pragma unroll
      for (int j = 0; j < NM; j++) {
        const double v = (i < n && j < n) ? rd_all(0, n * n, i * n + j) : 0.0;
        Gr[i][j] = live ? v : 0.0;
      }
#endif
      const double v0 = i < n ? rd_all(offg0, n, i) : 0.0;
      g0v[i] = live ? v0 : 0.0;
    }
    __syncthreads();
    lstamp(a, 9);  // diagnostic: G / g0 in registers
    // round B: CE and ce0 (equality phase), landing during the Cholesky, the J build and the
    // solve.  A full wave issues its span a part per Cholesky row: issued at once, its LDS-DMA
    // instructions held the wave's issue until most of the data had arrived (the CU's memory
    // queues fill), which serialised the transfer with the Cholesky.
    const int npB = n * p;
    const int offcB = (kQpw * npB + 127) / 128 * 128;
    const bool stageB = p > 0 && offcB + kQpw * p <= STAGE;
    auto round_b = [&](int part) {  // part `part` of NM
      constexpr int parts = NM;
      if (!stageB) return;
      if (!full) {
        if (part == 0) {
          stage_all(a.CE, npB, 0);
          stage_all(a.ce0, p, offcB);
        }
        return;
      }
      const double* ce = a.CE + b0 * (int64_t)npB;
      const double* c0 = a.ce0 + b0 * (int64_t)p;
      if constexpr (EXACT && PX > 0) {
        // the shape is compile-time: the chunks of a part that lie in one array are runs of up to
        // four on one source address and one M0 (copy_chunk), in the same ascending order
        constexpr int nce = (kQpw * NM * PX + 127) / 128, tot = nce + (kQpw * PX + 127) / 128;
        constexpr int per = (tot + parts - 1) / parts;
        for_seq<tot>([&](auto C) {
          constexpr int c = decltype(C)::value;
          constexpr int arr = c < nce ? 0 : nce;                         // the array's first chunk
          constexpr int run = c - c % per > arr ? c - c % per : arr;     // the part's, within the array
          constexpr int j = (c - run) % 4, k0 = (c - j - arr) * 128;     // chunk j of the run at k0
          if (c >= part * per && c < (part + 1) * per) {
            if constexpr (c < nce)
              copy_chunk(std::integral_constant<int, j>{}, ce, kQpw * NM * PX, 0, k0);
            else
              copy_chunk(std::integral_constant<int, j>{}, c0, kQpw * PX, nce * 128, k0);
          }
        });
      } else {
        const int nce = (kQpw * npB + 127) / 128, tot = nce + (kQpw * p + 127) / 128;
        const int per = (tot + parts - 1) / parts;
        for (int c = part * per; c < min(tot, (part + 1) * per); c++) {
          if (c < nce)
            copy_chunk(std::integral_constant<int, 0>{}, ce, kQpw * npB, 0, c * 128);
          else
            copy_chunk(std::integral_constant<int, 0>{}, c0, kQpw * p, offcB, (c - nce) * 128);
        }
      }
    };
#if QPGPU_LANE_UNIT
    // G = I stated: c1 = c2 = the ascending sum of n ones, J = I, x0 = -g0 and f0 from it.  Nothing
    // is factored, so round B has no Cholesky rows to go between.  Its NM parts still go one per
    // trip of this loop, back to back: measured against one round_b(0, 1) ahead of the loop, which
    // is the same copies in another instruction order, that form was 2 % slower on (7, 6, 14) and
    // within the spread on (7, 0, 14).
#pragma unroll
    for (int i = 0; i < NM; i++) {
      round_b(i);
      if (i < n) c1 += 1.0;
    }
#else
#pragma unroll
    for (int i = 0; i < NM; i++)
      if (i < n) c1 += Gr[i][i];
    // cholesky_decomposition (@.text+0x2df0): row-wise, descending-k sums, upper mirrored
#pragma unroll
    for (int i = 0; i < NM; i++) {
      round_b(i);  // every lane (the copy is per wave)
      if (i < n && chol_ok) {
        double sum = Gr[i][i];
#pragma unroll
        for (int k = i - 1; k >= 0; k--) sum -= Gr[i][k] * Gr[i][k];
        if (sum <= 0.0) {
          chol_ok = false;
          bad_sum = sum;
        } else {
          const double dg = sqrt(sum);
          Gr[i][i] = dg;
          const double rdg = F ? frcp(dg) : 0.0;
#pragma unroll
          for (int j = i + 1; j < NM; j++)
            if (j < n) {
              double s2 = Gr[i][j];
#pragma unroll
              for (int k = i - 1; k >= 0; k--) s2 -= Gr[i][k] * Gr[j][k];
              Gr[j][i] = ldiv_r<F>(s2, dg, rdg, fok);
            }
#pragma unroll
          for (int k = i + 1; k < NM; k++) Gr[i][k] = Gr[k][i];
        }
      }
    }
    if (!FULL && (a.flags & QPGPU_FLAG_WRITE_FACTOR) && live) {
      double* Gw = view(a.G, n * n);
#pragma unroll
      for (int i = 0; i < NM; i++)
#pragma unroll
        for (int j = 0; j < NM; j++)
          if (i < n && j < n) Gw[(i * n + j) * T] = Gr[i][j];
    }
#endif  // !QPGPU_LANE_UNIT
    // round B lands: the staged CE / ce0 are read in the equality phase.  Called once, after
    // J = L^-T and the solve (which need only the factor), so the CE transfer lands under them
    // instead of stalling the wave after the Cholesky.  (A lambda still: with the body written
    // out at the call the kernels' instruction order changes, profiles/ab_retire/README.md.)
    auto land_round_b = [&]() {
    if (p > 0) {
      const int np_ = n * p;
      const int offc = (kQpw * np_ + 127) / 128 * 128;
      ce_staged = offc + kQpw * p <= STAGE;
      __syncthreads();
      lstamp(a, 10);  // diagnostic: round B (CE) landed
      if constexpr (kCiDma) {
        if (dma && ce_staged) {
          // CE / ce0 -> AGPRs, then the LDS is the CI copy's (round C)
#pragma unroll
          for (int e = 0; e < NM * PX; e++) {
            const double v = rd_all(0, np_, e);
            ceag[e] = to_agpr(live ? v : 0.0);
          }
#pragma unroll
          for (int e = 0; e < PX; e++) {
            const double v = rd_all(offc, p, e);
            ceag[NM * PX + e] = to_agpr(live ? v : 0.0);
          }
          ce_agpr = true;
          __syncthreads();
          lstamp(a, 11);  // diagnostic: CE in AGPRs
          // (the copy itself goes a part per equality step; the rows past it and ci0 are not
          // warmed here.  Round 3 measured the C1 kernel at 47.4 us with a warm-up here, 48.6
          // without it, 49.9 with it at the first equality step, profiles/r03_s10; round 5's
          // fetch counts, at kScanDepth above, settled it the other way)
        }
      }
    }
    };
#if QPGPU_LANE_UNIT
    if (chol_ok) {
#pragma unroll
      for (int r = 0; r < NM; r++) {
#pragma unroll
        for (int j = 0; j < NM; j++) Jreg[r][j] = (r < n && j == r) ? 1.0 : 0.0;
        if (r < n) c2 += 1.0;
      }
      // (entries past n are -0.0, as the dense setup's negation of the +0.0 it starts from)
#pragma unroll
      for (int i = 0; i < NM; i++) xv[i] = -g0v[i];
#pragma unroll
      for (int i = 0; i < NM; i++)
        if (i < n) fval += g0v[i] * xv[i];
      fval = 0.5 * fval;
    }
#else
    if (chol_ok) {
      // J = L^{-T}: row r of J = L^{-1} e_r (forward_elimination); c2 = trace(J).
      // With a finite L the first r entries of L^{-1} e_r are exactly +0.0 (0.0 - L*(+0) and
      // 0.0 / L stay +0.0) and contribute exact zeros to later sums, so they are skipped: same
      // bits, ~40% fewer divisions.  A non-finite L (NaN inputs) takes the literal path.
      bool lfin = true;
#pragma unroll
      for (int i = 0; i < NM; i++)
#pragma unroll
        for (int j = 0; j <= i; j++)
          if (i < n) lfin = lfin && (fabs(Gr[i][j]) < inf);
      // fast build: one reciprocal per pivot serves the J build and the solve
      double rdiag[NM];
#pragma unroll
      for (int i = 0; i < NM; i++) rdiag[i] = (F && i < n) ? frcp(Gr[i][i]) : 0.0;
      auto build_j = [&](const bool skip) {
#pragma unroll
        for (int r = 0; r < NM; r++) {
          double y[NM];
#pragma unroll
          for (int i = 0; i < NM; i++) {
            double v = 0.0;
            if (r < n && i < n && !(skip && i < r)) {
              v = (i == r) ? 1.0 : 0.0;
#pragma unroll
              for (int j = 0; j < i; j++)
                if (!(skip && j < r)) v -= Gr[i][j] * y[j];
              v = ldiv_r<F>(v, Gr[i][i], rdiag[i], fok);
            }
            y[i] = v;
          }
#pragma unroll
          for (int j = 0; j < NM; j++) Jreg[r][j] = y[j];
          if (r < n) c2 += y[r];
        }
      };
      // (fast build: the skipping form unless some lane's factor is non-finite, decided per
      // wave so that the two forms stay separate code)
      if (F ? !wave_any(!lfin) : lfin)
        build_j(true);
      else
        build_j(false);
      // cholesky_solve (@.text+0x31a2): x = -G^{-1} g0
      double y[NM];
#pragma unroll
      for (int i = 0; i < NM; i++) {
        double v = 0.0;
        if (i < n) {
          v = g0v[i];
#pragma unroll
          for (int j = 0; j < i; j++) v -= Gr[i][j] * y[j];
          v = ldiv_r<F>(v, Gr[i][i], rdiag[i], fok);
        }
        y[i] = v;
      }
#pragma unroll
      for (int i = NM - 1; i >= 0; i--) {
        if (i < n) {
          double v = y[i];
#pragma unroll
          for (int j = i + 1; j < NM; j++)
            if (j < n) v -= Gr[i][j] * xv[j];
          xv[i] = ldiv_r<F>(v, Gr[i][i], rdiag[i], fok);
        }
      }
#pragma unroll
      for (int i = 0; i < NM; i++) xv[i] = -xv[i];
#pragma unroll
      for (int i = 0; i < NM; i++)
        if (i < n) fval += g0v[i] * xv[i];
      fval = 0.5 * fval;
    }
#endif  // QPGPU_LANE_UNIT
    land_round_b();
  }
  lstamp(a, 1);
  // Without the DMA: touch every cache line of this lane's CI and ci0 blocks before the
  // equality phase: the loads complete during it (nothing waits on them until its end), so the
  // first l1 scan reads L2 / MALL instead of queueing on one chip-wide HBM burst.  Issued after
  // the setup: vmcnt waits are in issue order, so earlier they would also delay the G / CE
  // waits (measured slower, profiles/r02_s4).
  if constexpr (T == 1 && kLanePrefetch) {
    if (!ce_agpr) warmup();
  }
  if (!chol_ok) {
    status = QPGPU_QP_NOT_POSITIVE_DEFINITE;
    fval = bad_sum;
  }
  const bool ok_lane = live && chol_ok;

  // ---------------------------------------------------------------- state
  double Rv[RI::SIZE];
#pragma unroll
  for (int i = 0; i < RI::SIZE; i++) Rv[i] = 0.0;
  double dv[NM], zv[NM], npv[NM], uv[NM + 1], rv[NM];
  int Av[NM + 1];
#pragma unroll
  for (int i = 0; i < NM; i++) dv[i] = zv[i] = npv[i] = rv[i] = 0.0;
#pragma unroll
  for (int i = 0; i <= NM; i++) {
    uv[i] = 0.0;
    Av[i] = 0;
  }
  double R_norm = 1.0;
  int iq = 0;

  auto compute_d = [&]() {
#pragma unroll
    for (int c = 0; c < NM; c++) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NM; j++)
        if (j < n) s += Jreg[j][c] * npv[j];
      dv[c] = s;
    }
  };
  // LoC: compile-time lower bound on iq (see add_constraint below)
  auto update_z = [&](auto LoC) {
    constexpr int LO = decltype(LoC)::value;
#pragma unroll
    for (int r = 0; r < NM; r++) {
      double z = 0.0;
#pragma unroll
      for (int j = LO; j < NM; j++)
        if (j >= iq && j < n) z += Jreg[r][j] * dv[j];
      zv[r] = z;
    }
  };
  // r = R^{-1} d for the active set's inequality rows only (i >= p; LoC: a compile-time bound on
  // iq, here p).  In the active-set loop only those rows' r feed anything — t1 and the
  // inequalities' multipliers; the equality constraints' multipliers u[0..p) are never read there,
  // nor output — and r[i] for i >= p does not depend on the rows below, so the reference's
  // back-substitution stops at row p (x, f, status and the l1 passes are unchanged).
  auto update_r = [&](auto LoC) {
    constexpr int LO = decltype(LoC)::value;
#pragma unroll
    for (int i = NM - 1; i >= 0; i--) {
      if (i >= LO && (DUAL || i >= p) && i < iq) {
        double s = 0.0;
#pragma unroll
        for (int j = i + 1; j < NM; j++)
          if (j < iq) s += Rv[RI::at(i, j)] * rv[j];
        rv[i] = ldiv<F>(dv[i] - s, Rv[RI::at(i, i)], fok);
      }
    }
  };
  // Fast build: the Givens step of add_constraint / delete_constraint without a branch.  The
  // pair (a, b) -> (+-h, 0) with h = |(a, b)| and the sign of a (the reference's cc < 0 test,
  // h > 0); the rows (t1, t2) -> (cc t1 + ss t2, ss t1 - cc t2), which is the reference's
  // xny (t1 + n1) - t2 with xny = ss / (1 + cc) and ss^2 + cc^2 = 1, without that division.  When
  // |h| < eps the reference skips the rotation: the coefficients become (1, 0 | 0, -1), the
  // identity, and (a, b) stay — so the step is straight-line code the scheduler can overlap with
  // the next rotation's h chain (which needs only +-h, not the coefficients).
  auto rot_fast = [&](double& a_, double& b_, auto&& apply) {
    const double a0 = a_, b0 = b_;
    const double h = ldistance<true>(a0, b0, fok);
    const bool skip = fabs(h) < kEps;
    const double rh = frcp(h);
    fok = fok && (skip || rcp_ok(rh));
    const bool neg = a0 < 0.0;
    const double cc = fabs(a0) * rh;
    const double ss = (neg ? -b0 : b0) * rh;
    a_ = skip ? a0 : (neg ? -h : h);
    b_ = skip ? b0 : 0.0;
    const double c1_ = skip ? 1.0 : cc, s1_ = skip ? 0.0 : ss;
    const double c2_ = skip ? -1.0 : cc, s2_ = skip ? 0.0 : ss;
    apply([&](double& t1r, double& t2r) {
      const double t1 = t1r, t2 = t2r;
      t1r = c1_ * t1 + s1_ * t2;
      t2r = s2_ * t1 - c2_ * t2;
    });
  };
  // LoC: a compile-time lower bound on iq (std::integral_constant).  In the active-set loop
  // iq >= p always (equality constraints are never dropped), so entries below p of R, A, u and
  // d are never the ones written or selected there: with p a compile-time constant (PX) the
  // predicated updates of those entries disappear.
  auto add_constraint = [&](auto LoC) -> bool {
    constexpr int LO = decltype(LoC)::value;
    if (iq >= n) return false;  // reference UB (p > n); reported as dependent
#pragma unroll
    for (int j = NM - 1; j >= LO + 1; j--) {
      if (j <= n - 1 && j >= iq + 1) {
        if constexpr (F) {
          rot_fast(dv[j - 1], dv[j], [&](auto&& rot) {
#pragma unroll
            for (int k = 0; k < NM; k++)
              if (k < n) rot(Jreg[k][j - 1], Jreg[k][j]);
          });
          continue;
        }
        double cc = dv[j - 1], ss = dv[j];
        const double h = ldistance<F>(cc, ss, fok);
        if (!(fabs(h) < kEps)) {
          dv[j] = 0.0;
          const double rh = F ? frcp(h) : 0.0;
          ss = ldiv_r<F>(ss, h, rh, fok);
          cc = ldiv_r<F>(cc, h, rh, fok);
          if (cc < 0.0) {
            cc = -cc;
            ss = -ss;
            dv[j - 1] = -h;
          } else {
            dv[j - 1] = h;
          }
          const double xny = ldiv<F>(ss, 1.0 + cc, fok);
#pragma unroll
          for (int k = 0; k < NM; k++)
            if (k < n) {
              const double t1 = Jreg[k][j - 1], t2 = Jreg[k][j];
              const double n1 = t1 * cc + t2 * ss;
              Jreg[k][j - 1] = n1;
              Jreg[k][j] = xny * (t1 + n1) - t2;
            }
        }
      }
    }
    iq++;
    // R[:iq, iq-1] = d[:iq]
#pragma unroll
    for (int c = LO; c < NM; c++)
#pragma unroll
      for (int i = 0; i <= c; i++) {
        const bool w = (c == iq - 1);
        Rv[RI::at(i, c)] = w ? dv[i] : Rv[RI::at(i, c)];
      }
    const double dd = fabs(lsel_lo<LO < NM ? LO : NM - 1>(dv, iq - 1));
    if (dd <= kEps * R_norm) return false;
    R_norm = (R_norm < dd) ? dd : R_norm;
    return true;
  };
  auto delete_constraint = [&](int l, auto LoC) {
    constexpr int LO = decltype(LoC)::value;  // qq >= LO (the deleted constraint is an inequality)
    int qq = 0;
    bool found = false;
#pragma unroll
    for (int k = 0; k <= NM; k++)
      if (!found && k >= p && k < iq && Av[k] == l) {
        qq = k;
        found = true;
      }
#pragma unroll
    for (int i = LO; i < NM; i++)
      if (i >= qq && i < iq - 1) {
        Av[i] = Av[i + 1];
        uv[i] = uv[i + 1];
      }
    // shift R columns left from qq (only upper + subdiagonal entries exist)
#pragma unroll
    for (int c = LO; c < NM - 1; c++) {
      const bool sh = (c >= qq && c < iq - 1);
#pragma unroll
      for (int r = 0; r <= c + 1 && r < NM; r++) {
        // destination R[r][c] (upper or subdiagonal), source R[r][c+1] (upper)
        Rv[RI::at(r, c)] = sh ? Rv[RI::at(r, c + 1)] : Rv[RI::at(r, c)];
      }
    }
    {
      const int aiq = lsel_lo<LO>(Av, iq);
      const double uiq = lsel_lo<LO>(uv, iq);
      lput_lo<LO>(Av, iq - 1, aiq);
      lput_lo<LO>(uv, iq - 1, uiq);
      lput_lo<LO>(Av, iq, 0);
      lput_lo<LO>(uv, iq, 0.0);
    }
    // R[j][iq-1] = 0 for j < iq
#pragma unroll
    for (int c = LO; c < NM; c++)
#pragma unroll
      for (int r = 0; r <= c + 1 && r < NM; r++) {
        const bool z = (c == iq - 1) && (r < iq);
        Rv[RI::at(r, c)] = z ? 0.0 : Rv[RI::at(r, c)];
      }
    iq--;
    if (iq == 0) return;
#pragma unroll
    for (int j = LO; j < NM - 1; j++) {
      if (j >= qq && j < iq) {
        if constexpr (F) {
          rot_fast(Rv[RI::at(j, j)], Rv[RI::at(j + 1, j)], [&](auto&& rot) {
#pragma unroll
            for (int k = j + 1; k < NM; k++)
              if (k < iq) rot(Rv[RI::at(j, k)], Rv[RI::at(j + 1, k)]);
#pragma unroll
            for (int k = 0; k < NM; k++)
              if (k < n) rot(Jreg[k][j], Jreg[k][j + 1]);
          });
          continue;
        }
        double cc = Rv[RI::at(j, j)], ss = Rv[RI::at(j + 1, j)];
        const double h = ldistance<F>(cc, ss, fok);
        if (!(fabs(h) < kEps)) {
          const double rh = F ? frcp(h) : 0.0;
          cc = ldiv_r<F>(cc, h, rh, fok);
          ss = ldiv_r<F>(ss, h, rh, fok);
          Rv[RI::at(j + 1, j)] = 0.0;
          if (cc < 0.0) {
            Rv[RI::at(j, j)] = -h;
            cc = -cc;
            ss = -ss;
          } else {
            Rv[RI::at(j, j)] = h;
          }
          const double xny = ldiv<F>(ss, 1.0 + cc, fok);
#pragma unroll
          for (int k = j + 1; k < NM; k++)
            if (k < iq) {
              const double t1 = Rv[RI::at(j, k)], t2 = Rv[RI::at(j + 1, k)];
              const double r1 = t1 * cc + t2 * ss;
              Rv[RI::at(j, k)] = r1;
              Rv[RI::at(j + 1, k)] = xny * (t1 + r1) - t2;
            }
#pragma unroll
          for (int k = 0; k < NM; k++)
            if (k < n) {
              const double t1 = Jreg[k][j], t2 = Jreg[k][j + 1];
              const double n1 = t1 * cc + t2 * ss;
              Jreg[k][j] = n1;
              Jreg[k][j + 1] = xny * (n1 + t1) - t2;
            }
        }
      }
    }
  };
  auto dot = [&](const double(&u_)[NM], const double(&v_)[NM]) -> double {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NM; i++)
      if (i < n) s += u_[i] * v_[i];
    return s;
  };
  const auto kZero = std::integral_constant<int, 0>{};
  // BOX: position (see above) of constraint i, and d = 0.0 -+ J[v][:] for the constraint at pos
  [[maybe_unused]] auto box_pos = [&](int i) -> int { return i < n ? i : NM + (i - n); };
  [[maybe_unused]] auto compute_d_box = [&](int pos) {
    const bool up = pos < NM;
    const int v = up ? pos : pos - NM;
#pragma unroll
    for (int c = 0; c < NM; c++) {
      double jv = opq_l(Jreg[0][c]);
#pragma unroll
      for (int k = 1; k < NM; k++) jv = (k == v) ? opq_l(Jreg[k][c]) : jv;
      dv[c] = 0.0 + (up ? -jv : jv);
    }
  };

  // ---------------------------------------------------------------- equality phase
  // Fully unrolled: in step i the active-set size iq equals i (every earlier step added a
  // constraint, or the phase stopped), so pinning iq to the compile-time i folds every
  // iq-predicate of compute_d / update_z / update_r / add_constraint.
  bool done = !ok_lane;
#pragma unroll
  for (int i = 0; i <= NM; i++) {
    if constexpr (kCiDma) {
      if (ce_agpr && i < PX) dma_ci_part(i, PX);  // every lane (the copy is per wave)
    }
    if (i < p && !done) {
      iq = i;
      double c0;
      if (i < NM) {
        const int np_ = n * p;
        const int offc = (kQpw * np_ + 127) / 128 * 128;
#pragma unroll
        for (int j = 0; j < NM; j++) {
          if constexpr (kCiDma) {
            if (ce_agpr) {
              // (idle lanes' ceag already holds zeros)
              npv[j] = j < n ? from_agpr(ceag[(j * PX + i) < kCeN ? j * PX + i : 0]) : 0.0;
              continue;
            }
          }
          if (ce_staged) {  // unconditional LDS read, then the select (see the G reads)
            const double v = j < n ? rd_all(0, np_, j * p + i) : 0.0;
            npv[j] = live ? v : 0.0;
          } else {
            npv[j] = (live && j < n) ? view(const_cast<double*>(a.CE), np_)[(j * p + i) * T] : 0.0;
          }
        }
        bool c0_done = false;
        if constexpr (kCiDma) {
          if (ce_agpr) {
            c0 = from_agpr(ceag[NM * PX + i < kCeN ? NM * PX + i : 0]);
            c0_done = true;
          }
        }
        if (!c0_done) {
          if (ce_staged) {
            const double v = rd_all(offc, p, i);
            c0 = live ? v : 0.0;
          } else {
            c0 = live ? view(const_cast<double*>(a.ce0), p)[i * T] : 0.0;
          }
        }
      } else {  // p > n: the step that reports "dependent" (reference UB, see oracle)
        const double* CEb = view(const_cast<double*>(a.CE), n * p);
#pragma unroll
        for (int j = 0; j < NM; j++) npv[j] = (j < n) ? CEb[(j * p + i) * T] : 0.0;
        c0 = view(const_cast<double*>(a.ce0), p)[i * T];
      }
      compute_d();
      update_z(kZero);
      if constexpr (DUAL) update_r(kZero);  // the reference's: r for the u[:i] update below
      // (no update_r and no u[:i] update here: r and the equality constraints' multipliers u[0..p)
      // feed nothing — the active-set loop reads u only for the inequalities (t1, the dual step's
      // drop, the rollback) and x, f never use u — so the reference's back-substitution of every
      // equality step is skipped; x, f, status and the l1 passes are unchanged)
      double t2 = 0.0;
      const double zz = dot(zv, zv);
      const double znp = dot(zv, npv);
      if (fabs(zz) > kEps) t2 = ldiv<F>(-dot(npv, xv) - c0, znp, fok);
#pragma unroll
      for (int k = 0; k < NM; k++) xv[k] += t2 * zv[k];
      uv[i < NM + 1 ? i : NM] = t2;
      if constexpr (DUAL) {
#pragma unroll
        for (int k = 0; k < NM; k++)
          if (k < i) uv[k] -= t2 * rv[k];
      }
      fval += 0.5 * (t2 * t2) * znp;
      Av[i < NM + 1 ? i : NM] = -i - 1;
      if (!add_constraint(kZero)) {
        status = QPGPU_QP_DEPENDENT;
        done = true;
      }
    }
  }
  // the m = 0 answer (qpgpu_solve_batched_eq): an empty l1 scan returns right here.  Only the
  // generic instantiations carry it; the launcher routes snapshot calls there so the EXACT
  // fast paths keep their register budget.
  if (!EXACT && a.x_eq && live) {
    if (chol_ok) {
      double* xb = view(a.x_eq, n);
#pragma unroll
      for (int i = 0; i < NM; i++)
        if (i < n) xb[i * T] = xv[i];
    }
    a.f_eq[b] = fval;
    a.st_eq[b] = status;
  }
  if constexpr (T == 1 && kLanePrefetch) {
    if (live && warmed)  // the warm-up loads retire here, long after they landed
#pragma unroll
      for (int k = 0; k < kPfCI + kPfC0; k++) asm volatile("" ::"v"(pf[k]));
  }
  // CI rows 0..kCiRows-1 are kept in LDS for the loop: brought in by the DMA above, or written
  // by the first l1 scan (which every active lane runs, loading those rows into registers
  // anyway).  Later scans then issue only the remaining rows' global loads, and the
  // selected-column gather takes those rows from LDS — no extra global traffic.
  const bool ci_lds = kCiRows > 0 && (FULL || (a.flags & kArgAligned16));
  bool ci_ready = false;  // wave-uniform: the on-chip copy has been written (or has landed)
  if constexpr (kCiDma) {
    if (dma && ce_agpr) {
      __syncthreads();  // the DMA has landed
      ci_ready = true;
    }
  }
  // element e (= row * MM + column) of this lane's CI from the LDS copy (e < kCiRows * MM)
  auto ci_lds_at = [&](int e) -> double { return sbuf[((e >> 1) * kQpw + lane) * 2 + (e & 1)]; };
  lstamp(a, 2);
  // Fast build: a fast form that went out of range in the setup or the equality phase (or
  // non-finite data) sends the wave to the IEEE re-solve now, instead of after a loop that
  // would run on garbage up to the step cap.  (The CE / CI copies into LDS have landed: the
  // re-solve may restage.)  The loop checks again at the top of every pass and after the last one.
  if constexpr (F) {
    if (wave_any(!fok)) return false;
  }

  // ---------------------------------------------------------------- active-set loop
  // Wave-uniform loop: every lane stays until all 64 are done; per-lane work is predicated on
  // `active`.  Every active lane has iq >= p here (the equality phase completed, only
  // inequalities are ever dropped), so with p known at compile time the loop's iq-indexed
  // updates start at p.
  constexpr int IQLO = PX >= 0 ? (PX <= NM ? PX : NM) : 0;
  const auto kLo = std::integral_constant<int, IQLO>{};
  // One free dimension (the full-wave kernel of a shape with p = n - 1: C1 / C4's (7, 6, 14)): the
  // active set holds at most one inequality, and the loop pass below the scan is a
  // two-state machine over a handful of scalars, instead of the general select and step.
  constexpr bool kOneFree = FULL && PX >= 0 && PX == NM - 1;
  {
    double sv[MM];
#pragma unroll
    for (int i = 0; i < MM; i++) sv[i] = 0.0;
    // rollback copies (compile-time indices only)
    double xold[NM], uold[NM];
    int aold[NM];
#pragma unroll
    for (int i = 0; i < NM; i++) {
      xold[i] = uold[i] = 0.0;
      aold[i] = 0;
    }
    uint64_t act = 0;   // bit c set <=> iai[c] == -1
    uint64_t excl = 0;  // bit c set <=> iaexcl[c] == false
    int ip = 0, steps = 0;
    double ss = 0.0, ci0ip = 0.0;
    bool need_scan = true, need_select = true;
    bool active = !done;
    const int max_steps = a.max_steps;
    // (BOX: none of the CI / ci0 loaders below is ever called; g0 keeps the pointers valid)
    const double* CIg = view(const_cast<double*>(BOX ? a.g0 : a.CI), n * m);
    const double* ci0g = view(const_cast<double*>(BOX ? a.g0 : a.ci0), m);
    // element loaders for this lane's CI / ci0 block.  TILED64: raw buffer loads off a
    // wave-uniform descriptor (tile base) + one lane-offset VGPR + element offset in SGPR/imm,
    // so no 64-bit address per element is kept live.
    // descriptor inputs through readfirstlane so the compiler can PROVE them uniform (else
    // it wraps every buffer op in a waterfall loop: guide T20)
    auto uniform_ptr = [](const double* ptr) -> double* {
      const uint64_t v = reinterpret_cast<uint64_t>(ptr);
      const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
      const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
      return reinterpret_cast<double*>(((uint64_t)hi << 32) | lo);
    };
    [[maybe_unused]] const auto rsCI = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(BOX ? a.g0 : a.CI + b0 * (int64_t)(n * m)), 0,
        __builtin_amdgcn_readfirstlane(64 * n * m * 8), 0x00020000);
    [[maybe_unused]] const auto rsci0 = __builtin_amdgcn_make_buffer_rsrc(
        uniform_ptr(BOX ? a.g0 : a.ci0 + b0 * (int64_t)m), 0, __builtin_amdgcn_readfirstlane(64 * m * 8),
        0x00020000);
    auto ldCI = [&](int e) -> double {
      if constexpr (T == 64)
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsCI, lane * 8, e * 512, 0));
      else
        return CIg[e];
    };
    auto ldci0 = [&](int e) -> double {
      if constexpr (T == 64)
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rsci0, lane * 8, e * 512, 0));
      else
        return ci0g[e];
    };
    // elements i, i+1 of row r (< kCiRows) of the LDS copy
    auto lds_pair = [&](int r, int i) -> double2 {
      return *reinterpret_cast<const double2*>(sbuf + (((r * MM + i) >> 1) * kQpw + lane) * 2);
    };
    // one l1 pass (the first fills the LDS copy when the DMA did not)
    auto scan_pass = [&]() {
        // ---- l1: s = CI^T x + ci0 (each s[i] sums j ascending, then + ci0[i])
        const bool do_scan = active && need_scan;
        if (wave_any(do_scan)) {
          double psi = 0.0;
          if (do_scan) {
            iter++;
            if constexpr (!kOneFree) {  // (the one-free pass forms the mask from its one slot)
#pragma unroll
            for (int k = 0; k < NM; k++)
              if (k >= p && k < iq) act |= 1ull << Av[k];
            }
#pragma unroll
            for (int i = 0; i < MM; i++) sv[i] = 0.0;
          }
          if constexpr (BOX) {
            if (do_scan) {
              // uppers then lowers: the reference's constraint order for psi
#pragma unroll
              for (int v = 0; v < NM; v++)
                if (v < n) {
                  sv[v] = (0.0 + -xv[v]) + bv[v];
                  sv[NM + v] = (0.0 + xv[v]) + bv[NM + v];
                }
#pragma unroll
              for (int q = 0; q < MM; q++)
                if ((q < NM ? q : q - NM) < n) psi += (sv[q] < 0.0) ? sv[q] : 0.0;
            }
          } else if (do_scan) {
            // QP-major rows of an EXACT even-m shape are 16-B aligned when the arrays are
            // (checked on the host: kArgAligned16): load them as dwordx4, half the instructions
            // and half the cache-line lookups per row
            constexpr bool VEC = (T == 1) && EXACT && (MM % 2 == 0);
            const bool vec = VEC && (FULL || (a.flags & kArgAligned16));
            auto ldrow = [&](double* dst, const double* src) {
              if (VEC && vec) {
#pragma unroll
                for (int i = 0; i < MM; i += 2) {
                  const double2 v = *reinterpret_cast<const double2*>(src + i);
                  dst[i] = v.x;
                  dst[i + 1] = v.y;
                }
              } else {
#pragma unroll
                for (int i = 0; i < MM; i++) dst[i] = (i < m) ? src[i] : 0.0;
              }
            };
            const bool from_chip = ci_lds && ci_ready;
            // "rows" 0..NM-1 are CI's rows (those >= n are never read), row NM is ci0
            auto load_row = [&](int r, double* dst) {
              if (r < NM) {
                if (r < n) {
                  if constexpr (T == 1)
                    ldrow(dst, CIg + r * m);
                  else
#pragma unroll
                    for (int i = 0; i < MM; i++) dst[i] = (i < m) ? ldCI(r * m + i) : 0.0;
                }
              } else if (r == NM) {
                if constexpr (T == 1)
                  ldrow(dst, ci0g);
                else
#pragma unroll
                  for (int i = 0; i < MM; i++) dst[i] = (i < m) ? ldci0(i) : 0.0;
              }
            };
            if (kCiRows > 0 && from_chip) {
              // the LDS rows summed while every global row (the rest of CI, ci0) is in
              // flight (same j order)
              constexpr int NG = NM + 1 - kCiRows;
              double gbuf[NG][MM];
#pragma unroll
              for (int r = kCiRows; r <= NM; r++) load_row(r, gbuf[r - kCiRows]);
              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
              for (int j = 0; j < NM; j++) {
                if (j < n) {
                  const double xj = xv[j];
                  if (j < kCiRows) {
#pragma unroll
                    for (int i = 0; i < MM; i += 2) {
                      const double2 v = lds_pair(j, i);
                      if (i < m) sv[i] += v.x * xj;
                      if (i + 1 < m) sv[i + 1] += v.y * xj;
                    }
                  } else {
                    const int g = j - kCiRows < NG ? j - kCiRows : 0;
#pragma unroll
                    for (int i = 0; i < MM; i++)
                      if (i < m) sv[i] += gbuf[g][i] * xj;
                  }
                }
              }
#pragma unroll
              for (int i = 0; i < MM; i++)
                if (i < m) {
                  sv[i] += gbuf[NG - 1][i];
                  psi += (sv[i] < 0.0) ? sv[i] : 0.0;
                }
            } else {
              // the first scan without the DMA (and every scan of the shapes without an
              // on-chip copy): software-pipelined two rows deep; row r lands in rowbuf[r % D]
              const bool fill = ci_lds && !ci_ready;
              constexpr int D = kScanDepth;
              double rowbuf[D][MM];
#pragma unroll
              for (int r = 0; r < D - 1; r++) load_row(r, rowbuf[r % D]);
#pragma unroll
              for (int j = 0; j < NM; j++) {
                load_row(j + D - 1, rowbuf[(j + D - 1) % D]);
                __builtin_amdgcn_sched_barrier(0);
                if (j < n) {
                  const double xj = xv[j];
#pragma unroll
                  for (int i = 0; i < MM; i++)
                    if (i < m) sv[i] += rowbuf[j % D][i] * xj;
                  if (j < kCiRows && fill) {
#pragma unroll
                    for (int i = 0; i < MM; i += 2)
                      *reinterpret_cast<double2*>(sbuf + (((j * MM + i) >> 1) * kQpw + lane) * 2) =
                          double2{rowbuf[j % D][i], rowbuf[j % D][i + 1]};
                  }
                }
                __builtin_amdgcn_sched_barrier(0);
              }
#pragma unroll
              for (int i = 0; i < MM; i++)
                if (i < m) {
                  sv[i] += rowbuf[NM % D][i];
                  psi += (sv[i] < 0.0) ? sv[i] : 0.0;
                }
            }
          }
          ci_ready = ci_ready || ci_lds;
          if (do_scan) {
            excl = 0;
            ss = 0.0;
            ip = 0;
            if (fabs(psi) <= (double)m * kEps * c1 * c2 * 100.0) {
              active = false;  // optimal
            } else if constexpr (!kOneFree) {  // (the one-free pass copies x under its select's loads)
#pragma unroll
              for (int i = 0; i < NM; i++) {
                if (i < IQLO || i < iq) {
                  uold[i] = uv[i];
                  aold[i] = Av[i];
                }
                xold[i] = xv[i];
              }
            }
          }
        }
    };
    uint64_t tscan = 0, tsel = 0, nloop = 0, tfirst = 0;  // diagnostic stamps only
    [[maybe_unused]] uint64_t tdzr = 0, tstep = 0;        // (QPGPU_LANE_STAMPS == 2: l2a split)
    // kResident (the QP-major one-free kernel, qp_lane_full_kernel<7, 14, 1, 6>): the CI rows past
    // the LDS copy stay in VGPRs (kept) and ci0 in AGPRs (ci0_ag) from the first scan to the end of
    // the loop, so no pass after the first issues a global load: the later scans sum from the
    // registers, and the select picks np's late rows out of kept under its own `take` (below).
    // The rollback copy of x, which only a rollback reads, is parked in AGPRs too (xold_ag; set
    // once ahead of the loop so that it is defined on entry).  Without the two parkings and the
    // scan's row-ahead fence the allocator moves column NM - 1 of J through AGPRs in every step of
    // the equality phase.  The first scan is peeled out of the loop, which then runs select,
    // step, next scan: the kept rows are defined in straight-line code ahead of the loop instead
    // of being a loop-carried value with an undefined entry.  Every lane that is ever active scans
    // in that first pass (need_scan starts true), so nothing else needs a load path.  The scan is
    // lane_scan_kept, a function of its own and not a lambda here, so that the other instantiations
    // of lane_body are the code they were.
    constexpr bool kResident = kOneFree && kCiDma;
    constexpr int kKept = kResident ? NM - kCiRows : 1;
    // (the full-wave DMA path always completes for such a shape, so ci_ready is true at the loop)
    static_assert(!kResident || (kQpw * NM * PX + 127) / 128 * 128 + kQpw * PX <= STAGE,
                  "the kept-row scan reads the LDS copy the DMA path fills");
    [[maybe_unused]] LaneResident<kResident, kKept, NM, MM> res;
    [[maybe_unused]] auto& kept = res.kept;
    [[maybe_unused]] auto& ci0_ag = res.ci0_ag;
    [[maybe_unused]] auto& xold_ag = res.xold_ag;
    // (stamps: nloop counts the passes as the unpeeled loop does, one per scan position reached
    // with a lane still active)
    if constexpr (kResident) {
      const uint64_t ts0 = (kStamps && a.stamps) ? __builtin_amdgcn_s_memtime() : 0;
      if (kStamps && a.stamps && wave_any(active)) nloop = 1;
      lane_scan_kept<NM, MM, kCiRows, true>(sbuf, lane, CIg, ci0g, xv, kept, ci0_ag, sv, c1, c2, need_scan, active,
                                            iter, excl, ss, ip);
      if (kStamps && a.stamps) tfirst = tscan = __builtin_amdgcn_s_memtime() - ts0;
#pragma unroll
      for (int i = 0; i < NM; i++) xold_ag[i] = to_agpr(xv[i]);
    }
    while (wave_any(active)) {
      if constexpr (F) {
        if (wave_any(!fok)) return false;
      }
      const uint64_t tl0 = (kStamps && a.stamps) ? __builtin_amdgcn_s_memtime() : 0;
      if constexpr (!kResident) scan_pass();
      const uint64_t tl1 = kResident ? tl0 : (kStamps && a.stamps) ? __builtin_amdgcn_s_memtime() : 0;
      if constexpr (!kResident) {
        if (kStamps && a.stamps) {
          tscan += tl1 - tl0;
          if (nloop == 0) tfirst = tl1 - tl0;
        }
        nloop++;
      }
      // kOneFree: select and step of one pass, the general ones below restated for n - p = 1.  Then
      // iq is S = n - 1 or S + 1, and of the general machinery only this is ever reached:
      //   * add_constraint and delete_constraint rotate nothing (their Givens loops run over j >= S + 1
      //     and over an empty range), so J is the equality phase's for the whole loop, and only its
      //     column S is read: d[S] = J[:,S] . np, and z = J[:,S] d[S] while slot S is empty;
      //   * the only entry of R that is read is R[S][S] (r[S] = d[S] / R[S][S]), written by the add;
      //   * with slot S empty (iq = S) no inequality can be dropped, t1 = inf: the step is the full
      //     step to constraint ip or, without a finite t2, infeasible; t = t2 exactly, so the partial
      //     step and its refresh of s[ip] never occur, s is the scan's, and s[ip] is the select's ss
      //     (ss < 0 whenever a step runs, and no pass moves ip without moving ss to s[ip]);
      //   * with slot S taken (iq = S + 1) z sums over an empty range: z = 0, zz = 0, t2 = inf, and the
      //     step is infeasible or the dual step that drops slot S, after which the pending constraint
      //     ip and its multiplier 0.0 + t (u[S + 1] is the select's 0.0 there) move into the slot and
      //     the same ip is stepped to without a scan or a select;
      //   * a failed add leaves iq = S, so the rollback restores x alone; the slot's A and u are
      //     rewritten by the select that follows.  ss and ip keep their values through it (no
      //     eligible s[i] is below the old minimum), as in the general loop.
      // State: iq, A[S] (the constraint in the slot; read only while iq = S + 1), u[S], R[S][S],
      // R_norm, x, f, ip, ss, np, excl and xold.  Every floating-point value comes from the general
      // loop's operations in their order (sums ascending from 0.0, the 0.0 + starts kept).
      if constexpr (kOneFree) {
        constexpr int S = NM - 1;
        constexpr int RSS = RI::at(S, S);
        // ---- l2: the most violated constraint not in the slot and not excluded
        if (active && need_select) {
          const uint32_t blocked = (uint32_t)excl | (iq > S ? 1u << Av[S] : 0u);
#pragma unroll
          for (int i = 0; i < MM; i++) {
            const bool take = sv[i] < ss && !((blocked >> i) & 1u);
            ss = take ? sv[i] : ss;
            ip = take ? i : ip;
            // kResident: np's rows past the LDS copy ride the same chain, out of the kept rows,
            // so that np = CI[:, ip] without a load.  Exact because (1) np persists across the
            // passes that do not select (the dual step's re-add of the pending ip), (2) a
            // re-select after a rollback in which no candidate is taken keeps ip, and with it
            // these rows of np, and (3) a scan resets ss and ip, so the first take after it (one
            // fires whenever the select goes on to a step: ss < 0) rewrites both rows.
            if constexpr (kResident) {
#pragma unroll
              for (int j = kCiRows; j < NM; j++) npv[j] = take ? kept[j - kCiRows < kKept ? j - kCiRows : 0][i] : npv[j];
            }
          }
          if (ss >= 0.0) {
            active = false;  // optimal
          } else {
#pragma unroll
            for (int j = 0; j < (kResident ? kCiRows : NM); j++)
              npv[j] = (j < kCiRows && ci_ready) ? ci_lds_at(j * MM + ip) : ldCI(j * m + ip);
            // (ci0[ip] is not loaded: only the partial step's refresh reads it)
            // the rollback copy, under the loads: x is the scan's here, or the x a rollback restored
#pragma unroll
            for (int i = 0; i < NM; i++) {
              if constexpr (kResident)
                xold_ag[i] = to_agpr(xv[i]);
              else
                xold[i] = xv[i];
            }
            if (iq == S) uv[S] = 0.0;  // (u[S + 1] = 0.0 is implied, A[iq] = ip is the slot's at the add)
          }
        }
        if (kStamps && a.stamps) {
          const double sink = npv[0] + npv[NM - 1];  // the select's loads are part of its span
          asm volatile("" ::"v"(sink));
          tsel += __builtin_amdgcn_s_memtime() - tl1;
        }
        // ---- l2a
        if (active) {
          if (max_steps > 0 && ++steps > max_steps) {
            status = QPGPU_QP_MAX_ITER;
            active = false;
          } else {
            [[maybe_unused]] uint64_t ts0 = 0;
            if constexpr (QPGPU_LANE_STAMPS == 2) ts0 = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
            const bool has = iq > S;  // slot S holds an inequality
            double dS = 0.0;
#pragma unroll
            for (int j = 0; j < NM; j++) dS += Jreg[j][S] * npv[j];
            double rS = 0.0;
            if (has) {
              rS = ldiv<F>(dS - 0.0, Rv[RSS], fok);
            } else {
#pragma unroll
              for (int r = 0; r < NM; r++) zv[r] = 0.0 + Jreg[r][S] * dS;
            }
            if constexpr (QPGPU_LANE_STAMPS == 2) {
              if (a.stamps) {
                const double sink = rS + zv[0] + dS;
                asm volatile("" ::"v"(sink));
                tdzr += __builtin_amdgcn_s_memtime() - ts0;
              }
            }
            if (has) {
              // t2 = inf, t = t1 = u[S] / r[S] where r[S] > 0 and the quotient is below inf
              double t1 = inf;
              if (rS > 0.0) {
                const double q_ = ldiv<F>(uv[S], rS, fok);
                t1 = (q_ < t1) ? q_ : t1;
              }
              if (t1 >= inf) {
                status = QPGPU_QP_INFEASIBLE;
                fval = inf;
                active = false;
              } else {  // dual step: slot S is dropped, the pending constraint takes it
                uv[S] = 0.0 + t1;
                iq = S;
                need_scan = need_select = false;
              }
            } else {
              const double zz = dot(zv, zv);
              const double znp = dot(zv, npv);
              double t2 = inf;
              if (fabs(zz) > kEps) {
                t2 = ldiv<F>(-ss, znp, fok);
                if (t2 < 0) t2 = inf;  // Takano Akio patch
              }
              if (!(t2 < inf)) {  // t = t1 = inf
                status = QPGPU_QP_INFEASIBLE;
                fval = inf;
                active = false;
              } else {  // full step (t = t2), then the add
                const double t = t2;
#pragma unroll
                for (int k = 0; k < NM; k++) xv[k] += t * zv[k];
                fval += t * znp * (0.5 * t + uv[S]);
                uv[S] = uv[S] + t;
                const double dd = fabs(dS);
                if (dd <= kEps * R_norm) {  // degenerate: roll back to the l1 state, select again
                  excl = (uint32_t)excl | (1u << ip);
#pragma unroll
                  for (int i = 0; i < NM; i++) {
                    if constexpr (kResident)
                      xv[i] = from_agpr(xold_ag[i]);
                    else
                      xv[i] = xold[i];
                  }
                  need_scan = false;
                  need_select = true;
                } else {
                  R_norm = (R_norm < dd) ? dd : R_norm;
                  Rv[RSS] = dS;
                  Av[S] = ip;
                  iq = S + 1;
                  need_scan = need_select = true;
                }
              }
            }
          }
        }
        if constexpr (kResident) {  // the next pass's scan, from the kept rows
          const uint64_t ts0 = (kStamps && a.stamps) ? __builtin_amdgcn_s_memtime() : 0;
          if (kStamps && a.stamps && wave_any(active)) nloop++;
          lane_scan_kept<NM, MM, kCiRows, false>(sbuf, lane, CIg, ci0g, xv, kept, ci0_ag, sv, c1, c2, need_scan,
                                                 active, iter, excl, ss, ip);
          if (kStamps && a.stamps) tscan += __builtin_amdgcn_s_memtime() - ts0;
        }
        continue;
      }
      // ---- l2: pick the most violated constraint (ss deliberately not reset: reference quirk)
      if (active && need_select) {
        if constexpr (BOX) {
#pragma unroll
          for (int q = 0; q < MM; q++)
            if ((q < NM ? q : q - NM) < n) {
              const int i = q < NM ? q : n + (q - NM);
              const bool elig = !((act >> i) & 1ull) && !((excl >> i) & 1ull);
              const bool take = sv[q] < ss && elig;
              ss = take ? sv[q] : ss;
              ip = take ? i : ip;
            }
        } else {  // (body left at its indentation)
#pragma unroll
        for (int i = 0; i < MM; i++)
          if (i < m) {
            const bool elig = !((act >> i) & 1ull) && !((excl >> i) & 1ull);
            const bool take = sv[i] < ss && elig;
            ss = take ? sv[i] : ss;
            ip = take ? i : ip;
          }
        }
        if (ss >= 0.0) {
          active = false;  // optimal
        } else {
          if constexpr (!BOX) {  // np gather (BOX forms no np in the loop); body left at its indentation
#pragma unroll
          for (int j = 0; j < NM; j++)
            npv[j] = (j < n) ? ((j < kCiRows && ci_ready) ? ci_lds_at(j * MM + ip) : ldCI(j * m + ip)) : 0.0;
          ci0ip = ldci0(ip);
          }
          lput_lo<IQLO>(uv, iq, 0.0);
          lput_lo<IQLO>(Av, iq, ip);
        }
      }
      if (kStamps && a.stamps) {
        // make the select's loads part of the select span
        const double sink = npv[0] + ci0ip;
        asm volatile("" ::"v"(sink));
        const uint64_t tl2 = __builtin_amdgcn_s_memtime();
        tsel += tl2 - tl1;
      }
      // ---- l2a
      if (active) {
        if (max_steps > 0 && ++steps > max_steps) {
          status = QPGPU_QP_MAX_ITER;
          active = false;
        } else {
          [[maybe_unused]] uint64_t ts0 = 0;
          if constexpr (QPGPU_LANE_STAMPS == 2) ts0 = a.stamps ? __builtin_amdgcn_s_memtime() : 0;
          [[maybe_unused]] const int ipos = BOX ? box_pos(ip) : ip;  // where s[ip] and b[ip] live
          if constexpr (BOX)
            compute_d_box(ipos);
          else
            compute_d();
          update_z(kLo);
          update_r(kLo);
          if constexpr (QPGPU_LANE_STAMPS == 2) {
            if (a.stamps) {
              const double sink = rv[0] + zv[0] + dv[NM - 1];
              asm volatile("" ::"v"(sink));
              tdzr += __builtin_amdgcn_s_memtime() - ts0;
            }
          }
          int l = 0;
          double t1 = inf;
#pragma unroll
          for (int k = 0; k < NM; k++)
            if (k >= p && k < iq && rv[k] > 0.0) {
              const double q_ = ldiv<F>(uv[k], rv[k], fok);
              const bool take = q_ < t1;
              t1 = take ? q_ : t1;
              l = take ? opq_l(Av[k]) : l;
            }
          const double zz = dot(zv, zv);
          double znp;
          if constexpr (BOX) {
            const double zs = lsel(zv, ipos < NM ? ipos : ipos - NM);
            znp = 0.0 + (ipos < NM ? -zs : zs);
          } else {
            znp = dot(zv, npv);
          }
          double t2;
          if (fabs(zz) > kEps) {
            t2 = ldiv<F>(-lsel<MM>(sv, ipos), znp, fok);
            if (t2 < 0) t2 = inf;  // Takano Akio patch
          } else {
            t2 = inf;
          }
          const double t = (t2 < t1) ? t2 : t1;
          // The step's four outcomes (infeasible, dual step, full step, partial step) as per-lane
          // predicates over ONE copy of each piece: a wave whose lanes take different outcomes
          // executes the union of the pieces, and delete_constraint — which the dual step
          // (drops l), the degenerate full step (drops ip) and the partial step (drops l) all
          // need — is the largest of them.  Each lane runs exactly its outcome's operations in
          // the reference's order (x, f, then u; add_constraint; then the delete; then the
          // rollback or the s[ip] refresh).
          const bool infs = t >= inf;
          const bool dual = !infs && t2 >= inf;
          const bool prim = !infs && !dual;
          const bool full = prim && fabs(t - t2) < kEps;
          const bool part = prim && !full;
          if (infs) {
            status = QPGPU_QP_INFEASIBLE;
            fval = inf;
            active = false;
          }
          if (prim) {
#pragma unroll
            for (int k = 0; k < NM; k++) xv[k] += t * zv[k];
            fval += t * znp * (0.5 * t + lsel_lo<IQLO>(uv, iq));
          }
          if (dual || prim) {
#pragma unroll
            for (int k = 0; k < NM; k++)
              if ((DUAL || k >= p) && k < iq) uv[k] -= t * rv[k];  // (u[0..p) are never read)
            lput_lo<IQLO>(uv, iq, lsel_lo<IQLO>(uv, iq) + t);
          }
          bool add_fail = false;
          if (full) {
            if (!add_constraint(kLo)) {
              add_fail = true;
              excl |= 1ull << ip;
            } else {
              act |= 1ull << ip;
              need_scan = need_select = true;
            }
          }
          if (dual || part) act &= ~(1ull << l);
          if (dual || part || add_fail) delete_constraint((dual || part) ? l : ip, kLo);
          if (add_fail) {  // degenerate: roll back to the l1 state, select again
            act = 0;
#pragma unroll
            for (int i = 0; i < NM; i++)
              if (i >= p && i < iq) {
                Av[i] = aold[i];
                uv[i] = uold[i];
                act |= 1ull << Av[i];
              }
#pragma unroll
            for (int i = 0; i < NM; i++) xv[i] = xold[i];
            need_scan = false;
            need_select = true;
          }
          if (part) {  // refresh s[ip] = CI[:,ip]^T x + ci0[ip]
            if constexpr (BOX) {
              const double xs = lsel(xv, ipos < NM ? ipos : ipos - NM);
              lput_lo<0>(sv, ipos, (0.0 + (ipos < NM ? -xs : xs)) + lsel<MM>(bv, ipos));
            } else {  // (body left at its indentation)
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < NM; j++)
              if (j < n) s += npv[j] * xv[j];
            lput_lo<0>(sv, ip, s + ci0ip);
            }
          }
          if (dual || part) need_scan = need_select = false;
        }
      }
    }
    if (kStamps && a.stamps && lane == 0) {
      a.stamps[(uint64_t)blockIdx.x * kStampSlots + 5] = tscan;
      a.stamps[(uint64_t)blockIdx.x * kStampSlots + 6] = tsel;
      a.stamps[(uint64_t)blockIdx.x * kStampSlots + 7] = nloop;
      a.stamps[(uint64_t)blockIdx.x * kStampSlots + 8] = tfirst;
      if constexpr (QPGPU_LANE_STAMPS == 2) a.stamps[(uint64_t)blockIdx.x * kStampSlots + 12] = tdzr;
    }
  }
  lstamp(a, 3);
  if constexpr (F) {
    if (wave_any(!fok)) return false;
  }

  if (live) {
    if (chol_ok) {
      double* xb = view(a.x, n);
#pragma unroll
      for (int i = 0; i < NM; i++)
        if (i < n) xb[i * T] = xv[i];
    }
    a.f[b] = fval;
    if (!FULL && a.iters) a.iters[b] = iter;
    a.status[b] = status;
  }
  if constexpr (DUAL) {
    // u dense, like x: equality j's multiplier is u[j] (A[j] = -j-1: equalities never move),
    // inequality A[k]'s is u[k] (k in [p, iq)), every other slot and every non-OK QP +0.0.  The
    // slot of u[k] differs per lane: MM predicated selects per entry, no private-array index.
    if (live) {
      const bool okq = status == QPGPU_QP_OK;
      double* ub = view(a.u, p + m);
      for (int j = 0; j < p; j++) ub[j * T] = (okq && j <= NM) ? lsel(uv, j) : 0.0;
      double ud[MM];
#pragma unroll
      for (int i = 0; i < MM; i++) ud[i] = 0.0;
      // (BOX: ud at the positions of s and b, the upper bound of v at v, the lower at NM + v)
#pragma unroll
      for (int k = 0; k < NM; k++) {
        const bool in = okq && k >= p && k < iq;
        const int pos = BOX ? box_pos(Av[k]) : Av[k];
        lput_lo<0>(ud, in ? pos : -1, uv[k]);
      }
      if constexpr (BOX) {
#pragma unroll
        for (int v = 0; v < NM; v++)
          if (v < n) {
            ub[(p + v) * T] = ud[v];
            ub[(p + n + v) * T] = ud[NM + v];
          }
      } else {  // (body left at its indentation)
#pragma unroll
      for (int i = 0; i < MM; i++)
        if (i < m) ub[(p + i) * T] = ud[i];
      }
      if (a.nact) a.nact[b] = okq ? iq - p : 0;
    }
  }
  lstamp(a, 4);
  return true;
}

template <int NM, int MM, int T, bool EXACT, int PX>
__global__ void __launch_bounds__(64, kLaneOcc) QP_LANE_KERNEL(const QpArgs a) {
  __shared__ double sbuf[kStage];
  if constexpr (kFast) {
    if (!lane_body<NM, MM, T, EXACT, PX, false>(a, (LdsD*)sbuf)) {
      __syncthreads();  // the fast attempt's LDS traffic is over
      lane_body<NM, MM, T, EXACT, PX, true>(a, (LdsD*)sbuf);
    }
  } else {
    lane_body<NM, MM, T, EXACT, PX, true>(a, (LdsD*)sbuf);
  }
}

// The kernels of the other modes and the full-wave kernels.  Templates, so an object that never
// launches one (the facts at the top of the file) has no code for it.  Kernels of their own, not
// branches in the kernel above, which stays the same code as without them: a branch in the kernel
// once pushed the N = 8 instantiations into scratch
// (profiles/placement/kernel_regs_branch_in_kernel.txt).
// qpgpu_solve_batched_dual: the general instantiation (run-time n, p, m) carrying r and u over the
// whole active set.
template <int NM, int MM, int T>
__global__ void __launch_bounds__(64, kLaneOcc) qp_lane_dual_kernel(const QpArgs a) {
  __shared__ double sbuf[kStage];
  lane_body<NM, MM, T, false, -1, true, true>(a, (LdsD*)sbuf);
}
// qpgpu_solve_batched_box: bounds instead of CI.  The compile-time p = 0 form of the exact shape
// (EXACT, PX = 0) and the run-time-shape form (any p, n <= NM).
template <int NM, int MM, int T, bool EXACT, int PX>
__global__ void __launch_bounds__(64, kLaneOcc) qp_lane_box_kernel(const QpArgs a) {
  __shared__ double sbuf[kStage];
  lane_body<NM, MM, T, EXACT, PX, true, false, true>(a, (LdsD*)sbuf);
}
// qpgpu_solve_batched_box_dual: the two box forms with the multipliers carried and returned.
template <int NM, int MM, int T, bool EXACT, int PX>
__global__ void __launch_bounds__(64, kLaneOcc) qp_lane_box_dual_kernel(const QpArgs a) {
  __shared__ double sbuf[kStage];
  lane_body<NM, MM, T, EXACT, PX, true, true, true>(a, (LdsD*)sbuf);
}
// The full-wave aligned kernels (lane_body's FULL): the shapes behind C1 / C4 (7, 6, 14) and C2
// (7, 0, 14), in both layouts.
template <int NM, int MM, int T, int PX>
__global__ void __launch_bounds__(64, kLaneOcc) qp_lane_full_kernel(const QpArgs a) {
  __shared__ double sbuf[kStage];
  lane_body<NM, MM, T, true, PX, true, false, false, true>(a, (LdsD*)sbuf);
}

// ---- the launcher: one policy for every build, read top to bottom ---------------------------------
// qpk_launch_lane* (at the end) picks the size class, launch_lane_t the mode and the instantiation,
// launch_plain enqueues a plain-mode kernel.  A kernel the object lacks is hipErrorInvalidValue.

// The plain kernel <EXACT, PX> over the whole batch.
template <int NM, int MM, int T, bool EXACT, int PX>
static hipError_t launch_plain(const QpArgs& a, hipStream_t stream) {
  if constexpr (kPart == 1 && EXACT && PX == 0) {
    return qpk_launch_lane_p0(&a, stream);  // part 2 has these kernels (and their full-wave forms)
  } else if constexpr (!has_plain(EXACT, PX)) {
    return hipErrorInvalidValue;
  } else {
    const dim3 blk(64);
    if constexpr (kHasFull && NM == 7 && MM == 14 && EXACT && PX >= 0) {
      // What the full-wave kernel assumes of a launch, apart from whole waves: the LDS-DMA and
      // double2 alignment bits, no factor written back, no iteration counts.
      constexpr uint32_t kAligned = kArgStage16 | kArgAligned16;
      if ((a.flags & kAligned) == kAligned && !(a.flags & QPGPU_FLAG_WRITE_FACTOR) && !a.iters) {
        // The whole 64-QP blocks of the batch through it, the remaining QPs (batch % 64) through
        // the general kernel as a second launch on the same stream over the sub-range past those
        // blocks.  A whole number of 64-QP blocks is a whole number of tiles and of 512-byte
        // steps, so the remainder's arrays keep the layout and the 16-byte residues the host
        // checked.
        const int64_t nb = a.batch / kQpw, done = nb * kQpw;
        if (nb > 0) {
          QpArgs c = a;
          c.batch = done;
          hipLaunchKernelGGL((qp_lane_full_kernel<NM, MM, T, PX>), dim3((unsigned)nb), blk, 0, stream, c);
          qpk_lane_count_launch(1);
        }
        if (a.batch > done) {
          QpArgs c = sub_range(a, done, a.batch - done);
          c.stamps = a.stamps ? a.stamps + nb * kStampSlots : nullptr;  // (per wave, not per QP)
          hipLaunchKernelGGL((QP_LANE_KERNEL<NM, MM, T, true, PX>), dim3(1), blk, 0, stream, c);
          qpk_lane_count_launch(0);
        }
        return hipSuccess;
      }
    }
    const dim3 g((unsigned)((a.batch + kQpw - 1) / kQpw));
    hipLaunchKernelGGL((QP_LANE_KERNEL<NM, MM, T, EXACT, PX>), g, blk, 0, stream, a);
    return hipSuccess;
  }
}

template <int NM, int MM, int T>
static hipError_t launch_lane_t(const QpArgs& a, hipStream_t stream) {
  const Mode mode = mode_of(a);
  if (mode != kPlain) {
    if constexpr (!kHasModes) {
      return hipErrorInvalidValue;
    } else {
      const dim3 g((unsigned)((a.batch + kQpw - 1) / kQpw)), blk(64);
      if (mode != kDual) {
        if (a.m != 2 * a.n || a.x_eq) return hipErrorInvalidValue;
        if (a.u) {
          if (a.n == NM && a.p == 0)
            hipLaunchKernelGGL((qp_lane_box_dual_kernel<NM, MM, T, true, 0>), g, blk, 0, stream, a);
          else
            hipLaunchKernelGGL((qp_lane_box_dual_kernel<NM, MM, T, false, -1>), g, blk, 0, stream, a);
        } else if (a.n == NM && a.p == 0) {
          hipLaunchKernelGGL((qp_lane_box_kernel<NM, MM, T, true, 0>), g, blk, 0, stream, a);
        } else {
          hipLaunchKernelGGL((qp_lane_box_kernel<NM, MM, T, false, -1>), g, blk, 0, stream, a);
        }
      } else {
        hipLaunchKernelGGL((qp_lane_dual_kernel<NM, MM, T>), g, blk, 0, stream, a);
      }
      return hipSuccess;
    }
  }
  // plain mode: the class's own shape (and no x_eq snapshot) runs a compile-time-shape kernel
  if (kFixedShapes && a.n == NM && a.m == MM && !a.x_eq) {
    if (a.p == 6) return launch_plain<NM, MM, T, true, 6>(a, stream);
    if (a.p == 0) return launch_plain<NM, MM, T, true, 0>(a, stream);
    return launch_plain<NM, MM, T, true, -1>(a, stream);
  }
  return launch_plain<NM, MM, T, false, -1>(a, stream);
}

template <int NM, int MM>
static hipError_t launch_lane(const QpArgs& a, hipStream_t stream) {
  const hipError_t e = a.tile == 64 ? launch_lane_t<NM, MM, 64>(a, stream) : launch_lane_t<NM, MM, 1>(a, stream);
  return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace QPK_LANE_NS

// qpk_launch_lane, _fast, _u, _fast_u, _unit, _unit_u, and part 2's qpk_launch_lane_p0: the first
// size class of QPK_LANE_SIZES (qp_common.h) that holds the shape.
extern "C" hipError_t QPK_LANE_C(qpk_launch_lane)(const qpk::QpArgs* a, hipStream_t stream) {
#define QPK_LANE_TRY(N, M) \
  if (a->n <= N && a->m <= M) return QPK_LANE_NS::launch_lane<N, M>(*a, stream);
  QPK_LANE_SIZES(QPK_LANE_TRY)
#undef QPK_LANE_TRY
  return hipErrorInvalidValue;
}
