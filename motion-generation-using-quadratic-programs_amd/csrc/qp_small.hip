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
template <int S, int NM, int MM>
static hipError_t launch_small(const QpArgs& a, hipStream_t stream) {
  using C = SmallCfg<S, NM, MM>;
  const dim3 g((unsigned)((a.batch + C::QPW - 1) / C::QPW)), blk(64);
  switch (mode_of(a)) {
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
  return hipGetLastError();
}

struct SmallVariant {
  int nmax, mmax;
  const char* name[4];  // by Mode
  hipError_t (*launch)(const QpArgs&, hipStream_t);
};

#define QPK_SMALL_NAMES(s) {"qp_small<" s ">", "qp_small_dual<" s ">", "qp_small_box<" s ">", "qp_small_box_dual<" s ">"}
static const SmallVariant kSmallVariants[] = {
    {8, 16, QPK_SMALL_NAMES("S=8,N=8,M=16"), launch_small<8, 8, 16>},
    {8, 32, QPK_SMALL_NAMES("S=8,N=8,M=32"), launch_small<8, 8, 32>},
    {16, 32, QPK_SMALL_NAMES("S=16,N=16,M=32"), launch_small<16, 16, 32>},
    {16, 64, QPK_SMALL_NAMES("S=16,N=16,M=64"), launch_small<16, 16, 64>},
};

// the unit-Hessian kernel of each variant (no dual or box form)
template <int S, int NM, int MM>
static hipError_t launch_small_unit(const QpArgs& a, hipStream_t stream) {
  using C = SmallCfg<S, NM, MM>;
  const dim3 g((unsigned)((a.batch + C::QPW - 1) / C::QPW)), blk(64);
  hipLaunchKernelGGL((qp_small_unit_kernel<S, NM, MM>), g, blk, 0, stream, a);
  return hipGetLastError();
}
struct SmallUnitVariant {
  int nmax, mmax;
  const char* name;
  hipError_t (*launch)(const QpArgs&, hipStream_t);
};
static const SmallUnitVariant kSmallUnitVariants[] = {
    {8, 16, "qp_small_unit<S=8,N=8,M=16>", launch_small_unit<8, 8, 16>},
    {8, 32, "qp_small_unit<S=8,N=8,M=32>", launch_small_unit<8, 8, 32>},
    {16, 32, "qp_small_unit<S=16,N=16,M=32>", launch_small_unit<16, 16, 32>},
    {16, 64, "qp_small_unit<S=16,N=16,M=64>", launch_small_unit<16, 16, 64>},
};
const SmallUnitVariant* pick_small_unit(int n, int m) {
  for (const auto& v : kSmallUnitVariants)
    if (n <= v.nmax && m <= v.mmax) return &v;
  return nullptr;
}

const SmallVariant* pick_small(int n, int m) {
  for (const auto& v : kSmallVariants)
    if (n <= v.nmax && m <= v.mmax) return &v;  // any p: iq never exceeds n
  return nullptr;
}

}  // namespace qpk

extern "C" hipError_t qpk_launch_small(const qpk::QpArgs* a, hipStream_t stream) {
  const qpk::SmallVariant* v = qpk::pick_small(a->n, a->m);
  return v ? v->launch(*a, stream) : hipErrorInvalidValue;
}

extern "C" const char* qpk_small_name(int n, int m, int mode) {
  const qpk::SmallVariant* v = qpk::pick_small(n, m);
  return v ? v->name[mode] : nullptr;
}

extern "C" hipError_t qpk_launch_small_unit(const qpk::QpArgs* a, hipStream_t stream) {
  const qpk::SmallUnitVariant* v = qpk::pick_small_unit(a->n, a->m);
  return (v && !a->u && !a->hi) ? v->launch(*a, stream) : hipErrorInvalidValue;
}

extern "C" const char* qpk_small_name_unit(int n, int m) {
  const qpk::SmallUnitVariant* v = qpk::pick_small_unit(n, m);
  return v ? v->name : nullptr;
}
