// qp_small.hip — gfx950 batched Goldfarb–Idnani solver for small dense QPs (n <= 16).
//
// Restates solve_quadprog() (reference include/QuadProgpp/QuadProg++.hh:69-72; body in the
// prebuilt libquadprog.a, operation order fixed in SURVEY.md §3.2) for a batch of independent
// QPs, one QP per SUBGROUP of S lanes of a 64-lane wavefront (64/S QPs per wave).
//
// Work split inside a subgroup (lane ls = 0..S-1):
//   * rows k = ls + q*S of J (= L^{-T}) live in registers (Jr[q][:]); every Givens rotation of
//     add_constraint / delete_constraint is row-parallel, and update_z is a row-local dot;
//   * inequality columns c = ls + q*S of CI (and ci0) live in registers (CIr[q][:]); the
//     l1 scan s = CI^T x + ci0 is column-local;
//   * compute_d's column sums go through an LDS transpose (P) so each sum keeps the reference
//     order (j ascending); G/L and R live in LDS (R is touched column-wise by add_constraint
//     and row-pair-wise by delete_constraint);
//   * the O(n) serial state (x, z, d, np, u, r, A and every step length) is replicated in all
//     S lanes and computed redundantly — identical values, so every control decision is
//     subgroup-uniform and the subgroup never diverges internally.
// All replicated arrays are indexed with compile-time indices only (fully unrolled loops with
// run-time predicates), so nothing spills to scratch.  Arithmetic is IEEE binary64 with the
// reference's evaluation order and no contraction: results are bitwise identical to the CPU
// restatement (oracle/qp_oracle.c), which tests/ check.
#include "qp_common.h"

namespace qpk {

// Opaque copy of a register value.  Selecting among array elements that are still loads at
// InstCombine time gets rewritten into ONE load through a selected address, which pins the
// array in scratch memory; routing each element through an empty asm keeps it a register.
template <typename T>
__device__ __forceinline__ T opq(T v) {
  asm("" : "+v"(v));
  return v;
}

template <int N, typename T>
__device__ __forceinline__ T sel(const T (&v)[N], int i) {
  // unconditional selects: a conditional form lets the optimiser merge the chain back into
  // a run-time-indexed load, which sends the whole array to scratch.
  T r = opq(v[0]);
#pragma unroll
  for (int k = 1; k < N; k++) r = (k == i) ? opq(v[k]) : r;
  return r;
}

template <int N, typename T>
__device__ __forceinline__ void put(T (&v)[N], int i, T x) {
#pragma unroll
  for (int k = 0; k < N; k++) v[k] = (k == i) ? x : v[k];
}

template <int S, int NM, int MM>
struct SmallCfg {
  static_assert(64 % S == 0, "S must divide 64");
  static_assert(MM <= 64, "bitmask bookkeeping holds m <= 64");
  static constexpr int QPW = 64 / S;            // QPs per wavefront
  static constexpr int RPL = (NM + S - 1) / S;  // J rows per lane
  static constexpr int CPL = (MM + S - 1) / S;  // CI columns per lane
  static constexpr int RS = NM + 1;             // LDS row stride (odd: conflict-free rows)
  static constexpr int OFF_R = 0;
  static constexpr int OFF_P = OFF_R + NM * RS;  // G / L during setup, then compute_d transpose
  static constexpr int OFF_S = OFF_P + NM * RS;  // s[m]
  static constexpr int OFF_D = OFF_S + MM;       // d exchange
  static constexpr int OFF_Z = OFF_D + NM;       // z exchange
  static constexpr int OFF_NP = OFF_Z + NM;      // np exchange
  static constexpr int OFF_XOLD = OFF_NP + NM;
  static constexpr int OFF_UOLD = OFF_XOLD + NM;
  static constexpr int OFF_AOLD = OFF_UOLD + NM + 1;
  static constexpr int RAW = OFF_AOLD + NM + 1;
  static constexpr int REGION = ((RAW + 31) / 32) * 32 + 1;  // odd stride between QPs
  static constexpr int LDS_DOUBLES = QPW * REGION;
};

// the kernel, and a second time with the multipliers carried and returned (a kernel of its own,
// so the first is the same code as without it)
#define QP_SMALL_UNIT 0
#define QP_SMALL_BOX false
#define QP_SMALL_KERNEL qp_small_kernel
#define QP_SMALL_DUAL false
#include "qp_small_kernel.inc"
#undef QP_SMALL_KERNEL
#undef QP_SMALL_DUAL
#define QP_SMALL_KERNEL qp_small_dual_kernel
#define QP_SMALL_DUAL true
#include "qp_small_kernel.inc"
#undef QP_SMALL_KERNEL
#undef QP_SMALL_DUAL
#undef QP_SMALL_BOX
// a third time for bound constraints (qpgpu_solve_batched_box)
#define QP_SMALL_KERNEL qp_small_box_kernel
#define QP_SMALL_DUAL false
#define QP_SMALL_BOX true
#include "qp_small_kernel.inc"
#undef QP_SMALL_KERNEL
#undef QP_SMALL_DUAL
// a fourth time for bound constraints with the multipliers (qpgpu_solve_batched_box_dual)
#define QP_SMALL_KERNEL qp_small_box_dual_kernel
#define QP_SMALL_DUAL true
#include "qp_small_kernel.inc"
#undef QP_SMALL_KERNEL
#undef QP_SMALL_DUAL
#undef QP_SMALL_BOX
#undef QP_SMALL_UNIT
// a fifth time for the identity Hessian without a G array (qpgpu_solve_batched_unit)
#define QP_SMALL_UNIT 1
#define QP_SMALL_KERNEL qp_small_unit_kernel
#define QP_SMALL_DUAL false
#define QP_SMALL_BOX false
#include "qp_small_kernel.inc"
#undef QP_SMALL_KERNEL
#undef QP_SMALL_DUAL
#undef QP_SMALL_BOX
#undef QP_SMALL_UNIT

// ------------------------------------------------------------------------------------------
// launch table
// ------------------------------------------------------------------------------------------
// One launcher per size class: its kernel for mode_of(a), or (UNIT) its unit-Hessian kernel, which
// has no dual or box form.
template <int S, int NM, int MM, bool UNIT>
static hipError_t launch_small(const QpArgs& a, hipStream_t stream) {
  using C = SmallCfg<S, NM, MM>;
  const dim3 g((unsigned)((a.batch + C::QPW - 1) / C::QPW)), blk(64);
  const Mode mode = mode_of(a);
  if constexpr (UNIT) {
    if (mode != kPlain) return hipErrorInvalidValue;
    hipLaunchKernelGGL((qp_small_unit_kernel<S, NM, MM>), g, blk, 0, stream, a);
  } else {
    switch (mode) {
      case kBoxDual:
        hipLaunchKernelGGL((qp_small_box_dual_kernel<S, NM, MM>), g, blk, 0, stream, a);
        break;
      case kBox:
        hipLaunchKernelGGL((qp_small_box_kernel<S, NM, MM>), g, blk, 0, stream, a);
        break;
      case kDual:
        hipLaunchKernelGGL((qp_small_dual_kernel<S, NM, MM>), g, blk, 0, stream, a);
        break;
      case kPlain:
        hipLaunchKernelGGL((qp_small_kernel<S, NM, MM>), g, blk, 0, stream, a);
        break;
    }
  }
  return hipGetLastError();
}

// The size classes of QPK_SMALL_SIZES (qp_common.h), once for the four kernels by mode and once
// for the unit kernel; the names are the host's table over the same list (qpgpu_api.cpp kernel_name).
struct SmallVariant {
  int nmax, mmax;
  hipError_t (*launch)(const QpArgs&, hipStream_t);
};
#define QPK_SMALL_COUNT(S, N, M) +1
static const SmallVariant kSmallVariants[2][QPK_SMALL_SIZES(QPK_SMALL_COUNT)] = {  // [unit][class]
#define QPK_SMALL_ROW(S, N, M) {N, M, launch_small<S, N, M, false>},
#define QPK_SMALL_UNIT_ROW(S, N, M) {N, M, launch_small<S, N, M, true>},
    {QPK_SMALL_SIZES(QPK_SMALL_ROW)}, {QPK_SMALL_SIZES(QPK_SMALL_UNIT_ROW)}
#undef QPK_SMALL_ROW
#undef QPK_SMALL_UNIT_ROW
};
#undef QPK_SMALL_COUNT

// the first size class that holds the shape
static hipError_t launch_small_class(const QpArgs& a, hipStream_t stream, bool unit) {
  for (const auto& v : kSmallVariants[unit])
    if (a.n <= v.nmax && a.m <= v.mmax) return v.launch(a, stream);  // any p: iq never exceeds n
  return hipErrorInvalidValue;
}

}  // namespace qpk

extern "C" hipError_t qpk_launch_small(const qpk::QpArgs* a, hipStream_t stream) {
  return qpk::launch_small_class(*a, stream, false);
}
extern "C" hipError_t qpk_launch_small_unit(const qpk::QpArgs* a, hipStream_t stream) {
  return qpk::launch_small_class(*a, stream, true);
}
