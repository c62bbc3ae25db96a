// qp_vjp.h — what qp_vjp.hip exports to qpgpu_api.cpp: the argument block of the backward step
// (include/qpgpu.h qpgpu_vjp / qpgpu_vjp_box), its launch and the name of the kernel it runs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpk {

struct VjpArgs {
  int n, p, m;
  int box;             // non-zero: CI = [-I, +I] is generated, never read; dhi / dlo instead of dCI / dci0
  int64_t batch, qp0;  // a launch covers QPs [qp0, batch); callers pass qp0 = 0
  const double* G;
  const double* CE;
  const double* CI;  // NULL with box
  const double* x;
  const double* u;
  const int32_t* status;  // may be NULL: every QP is evaluated
  const double* gx;
  // the gradients; each may be NULL (not computed, not written)
  double* dG;
  double* dg0;
  double* dCE;
  double* dce0;
  double* dCI;   // dense only
  double* dci0;  // dense only
  double* dhi;   // box only
  double* dlo;   // box only
};

// The argument block of the full form (qpgpu_vjp_full / qpgpu_vjp_box_full).  The two cotangents sit
// in a block of its own: the x-only kernels keep the kernel argument they had, byte for byte (the
// register allocation of qp_vjp_ws.hip's kernel moved with the argument's size alone).
struct VjpFullArgs : VjpArgs {
  const double* gu;  // dl/du in the layout of u; may be NULL
  const double* gf;  // dl/df, one double per QP in either layout; may be NULL
};

}  // namespace qpk

// The kernel a launch of this n runs: NULL for n outside [1, 64].
extern "C" const char* qpk_vjp_name(int n);
// Enqueue the backward step of QPs [0, a->batch) on `stream`; tiled != 0: QPGPU_LAYOUT_TILED64.
// n outside [1, 64] is hipErrorInvalidValue.
extern "C" hipError_t qpk_launch_vjp(const qpk::VjpArgs* a, int tiled, hipStream_t stream);
// The same two for the full form.
extern "C" const char* qpk_vjp_full_name(int n);
extern "C" hipError_t qpk_launch_vjp_full(const qpk::VjpFullArgs* a, int tiled, hipStream_t stream);

// qp_vjp_ws.hip, 64 < n <= 256 (include/qpgpu.h qpgpu_vjp_ws / qpgpu_vjp_box_ws).
// The kernel a launch of this n runs: NULL for n outside [65, 256].
extern "C" const char* qpk_vjp_ws_name(int n);
// Doubles of workspace per QP in flight (a slot): 3 n^2 + n; 0 for n outside [65, 256].
extern "C" int64_t qpk_vjp_ws_doubles(int n);
// Enqueue the backward step of QPs [0, a->batch) on `stream`: min(slots, a->batch) workgroups, workgroup
// s working in ws[s * doubles, (s + 1) * doubles) on the QPs s, s + slots, ...  n outside [65, 256], a
// NULL ws or slots < 1 is hipErrorInvalidValue.
extern "C" hipError_t qpk_launch_vjp_ws(const qpk::VjpArgs* a, int tiled, void* ws, int64_t slots, hipStream_t stream);
// The same two for the full form (qp_vjp_ws_full.hip: qp_vjp_ws.hip built a second time).
extern "C" const char* qpk_vjp_ws_full_name(int n);
extern "C" hipError_t qpk_launch_vjp_ws_full(const qpk::VjpFullArgs* a, int tiled, void* ws, int64_t slots,
                                             hipStream_t stream);
