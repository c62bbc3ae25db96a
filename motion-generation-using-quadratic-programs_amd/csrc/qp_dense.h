// qp_dense.h — the dense linear algebra that the on-chip sensitivity kernels share: qp_vjp.hip
//  and qp_jvp.hip (§3.11) run the same factorisations and substitutions on the same
// working set with other right-hand sides, in the same two mappings (one QP per lane, one QP per
// group of S lanes).  include/qpgpu.h fixes every sum's order and the tests check it bit for bit,
// so each piece here exists once: a change of order reaches every entry or none.  qp_vjp_ws.hip
// takes box_entry alone; its panel routines are another algorithm.
//
// What is here compiles to the instructions it compiled to as text of the two files.  The steps
// that both kernels still write out (the register Cholesky and back substitution, the working-list
// scans, the M-column sweep, the Gram rows, R = chol(S) in the lane's slice) did not: as calls they
// moved branches, registers or unrolling in at least one kernel (profiles/dense_helpers).
#pragma once

#include <mutex>
#include <set>
#include <utility>

#include "qp_common.h"

namespace qpk {

// element i of column j of CI = [-I, +I] (n x 2n)
__device__ __forceinline__ double box_entry(int i, int j, int n) {
  return j < n ? (i == j ? -1.0 : -0.0) : (i == j - n ? 1.0 : 0.0);
}

constexpr int tri(int i, int k) { return i * (i + 1) / 2 + k; }

// ---- one QP per lane: L (packed lower triangle) and the vectors in registers ----------------------
template <int N>
__device__ __forceinline__ void lane_fsub(const double (&L)[N * (N + 1) / 2], double (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) {
    double s = v[i];
#pragma unroll
    for (int k = 0; k < i; k++) s = s - L[tri(i, k)] * v[k];
    v[i] = s / L[tri(i, i)];
  }
}

// ---- one QP per lane: the lane-private LDS slice ---------------------------------------------------
// Element e of lane l at e * 64 + l.  Ms: M (N x q), Ss: S / R (packed), Cs: the q-vector, Ws: the
// working list; N and lane are the names in scope.
#define MS(i, t) Ms[((i) * N + (t)) * 64 + lane]
#define SS(s, t) Ss[tri((s), (t)) * 64 + lane]
#define CS(t) Cs[(t) * 64 + lane]
#define WS(t) Ws[(t) * 64 + lane]

// Cs = bsub(R, fsub(R, Cs)), in place
__device__ __forceinline__ void lane_lds_solve(const double* Ss, double* Cs, int nq, int lane) {
  for (int i = 0; i < nq; i++) {
    double s = CS(i);
    for (int k = 0; k < i; k++) s = s - SS(i, k) * CS(k);
    CS(i) = s / SS(i, i);
  }
  for (int i = nq - 1; i >= 0; i--) {
    double s = CS(i);
    for (int k = i + 1; k < nq; k++) s = s - SS(k, i) * CS(k);
    CS(i) = s / SS(i, i);
  }
}

// ---- one QP per group of S lanes -----------------------------------------------------------------
constexpr int group_lanes(int n) { return n <= 16 ? 16 : n <= 32 ? 32 : 64; }  // the smallest S that holds n

// doubles of LDS per group: three S x (S + 1) tiles, four vectors, the working list (S ints).  Both
// directions keep to this footprint, so the same number of workgroups fits a CU (with three more
// vectors the forward mode's S = 32 kernel kept two workgroups per CU instead of three and took
// 2.24 ms instead of 1.57 ms on C3): what a kernel needs beyond it lives in the spare
// columns of the tiles.
template <int S>
constexpr int group_doubles() {
  return 3 * S * (S + 1) + 4 * S + S / 2;
}

// A = chol(A) in place on rows and columns [0, size) of a tile; lane sl owns row sl.  `bound` (>= size)
// is the trip count, the same in every lane of the wave.
template <int S>
__device__ __forceinline__ void group_chol(double* A, int size, int bound, int sl, int base) {
  constexpr int LD = S + 1;
  for (int j = 0; j < bound; j++) {
    double s = A[sl * LD + j];
    for (int k = 0; k < j; k++) s = s - A[sl * LD + k] * A[j * LD + k];
    const double sq = sqrt(s);
    const double d = __shfl(sq, base + j, 64);  // lane j's: the pivot
    const double val = sl == j ? sq : s / d;
    if (j < size && sl >= j && sl < size) A[sl * LD + j] = val;
    sg_sync();
  }
}

// lane i's element of fsub(A, rhs) (rhs: lane i's element); z is the group's scratch vector
template <int S>
__device__ __forceinline__ double group_fsub(const double* A, int size, int bound, int sl, double rhs, double* z) {
  constexpr int LD = S + 1;
  double out = 0.0;
  for (int i = 0; i < bound; i++) {
    if (sl == i && i < size) {
      double s = rhs;
      for (int k = 0; k < i; k++) s = s - A[i * LD + k] * z[k];
      out = s / A[i * LD + i];
      z[i] = out;
    }
    sg_sync();
  }
  return out;
}

// the same for bsub(A, rhs): A^T z = rhs
template <int S>
__device__ __forceinline__ double group_bsub(const double* A, int size, int bound, int sl, double rhs, double* z) {
  constexpr int LD = S + 1;
  double out = 0.0;
  for (int i = bound - 1; i >= 0; i--) {
    if (sl == i && i < size) {
      double s = rhs;
      for (int k = i + 1; k < size; k++) s = s - A[k * LD + i] * z[k];
      out = s / A[i * LD + i];
      z[i] = out;
    }
    sg_sync();
  }
  return out;
}

// ---- host side -----------------------------------------------------------------------------------
// Dynamic LDS beyond 64 KiB is granted once per kernel and device; host threads may launch
// concurrently (include/qpgpu.h), so the record is locked.
inline hipError_t grant_lds(const void* k, size_t bytes) {
  static std::mutex mu;
  static std::set<std::pair<const void*, int>> granted;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const std::pair<const void*, int> key(k, dev);
  std::lock_guard<std::mutex> lk(mu);
  if (granted.count(key)) return hipSuccess;
  e = hipFuncSetAttribute(key.first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) granted.insert(key);
  return e;
}

// Kernel k (the lane kernel of a->n <= 8, else the group kernel of S = group_lanes(a->n)) over QPs
// [0, a->batch), one wavefront per workgroup, in launches of at most 2^30 workgroups.  The caller
// has checked 1 <= a->n <= 64.
template <class Args>
hipError_t launch_dense(void (*k)(Args), const Args* a, hipStream_t stream) {
  const bool lane = a->n <= 8;
  const int S = group_lanes(a->n);
  const int64_t per_wg = lane ? 64 : 64 / S;  // QPs per workgroup
  size_t lds = 0;
  if (!lane) {
    const int per = S == 16 ? group_doubles<16>() : S == 32 ? group_doubles<32>() : group_doubles<64>();
    lds = (size_t)per * (64 / S) * sizeof(double);
    if (lds > 65536) {  // S = 64: beyond the default limit, inside the CU's 160 KiB
      const hipError_t e = grant_lds(reinterpret_cast<const void*>(k), lds);
      if (e != hipSuccess) return e;
    }
  }
  Args c = *a;
  const int64_t per = (int64_t)1 << 30;  // workgroups per launch: the grid stays inside 32 bits
  for (int64_t w0 = 0; w0 * per_wg < a->batch; w0 += per) {
    c.qp0 = w0 * per_wg;
    const int64_t left = (a->batch - c.qp0 + per_wg - 1) / per_wg;
    hipLaunchKernelGGL(k, dim3((unsigned)(left < per ? left : per)), dim3(64), lds, stream, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// names[0, 8): the lane kernels of n = 1..8, then the group kernels of S = 16, 32, 64; NULL for n
// outside [1, 64]
inline const char* dense_kernel_name(const char* const (&names)[11], int n) {
  if (n < 1 || n > 64) return nullptr;
  return names[n <= 8 ? n - 1 : n <= 16 ? 8 : n <= 32 ? 9 : 10];
}

}  // namespace qpk
