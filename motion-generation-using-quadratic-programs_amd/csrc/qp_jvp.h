// qp_jvp.h — what qp_jvp.hip exports to qpgpu_api.cpp: the argument block of the forward-mode
// sensitivities (include/qpgpu.h qpgpu_jvp / qpgpu_jvp_box), its launch and the name of the kernel it runs.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpk {

struct JvpArgs {
  int n, p, m;
  int box;             // non-zero: CI = [-I, +I] is generated, never read; thi / tlo instead of tCI / tci0
  int64_t batch, qp0;  // a launch covers QPs [qp0, batch); callers pass qp0 = 0
  const double* G;
  const double* CE;
  const double* CI;  // NULL with box
  const double* x;
  const double* u;
  const int32_t* status;  // may be NULL: every QP is evaluated
  // the tangents; each may be NULL (a zero tangent whose steps are not executed)
  const double* tG;
  const double* tg0;
  const double* tCE;
  const double* tce0;
  const double* tCI;   // dense only
  const double* tci0;  // dense only
  const double* thi;   // box only
  const double* tlo;   // box only
  // the outputs; each may be NULL (not computed, not written)
  double* tx;
  double* tu;
  double* tf;
};

}  // namespace qpk

// The kernel a launch of this n runs: NULL for n outside [1, 64].
extern "C" const char* qpk_jvp_name(int n);
// Enqueue the sensitivities of QPs [0, a->batch) on `stream`; tiled != 0: QPGPU_LAYOUT_TILED64.
// n outside [1, 64] is hipErrorInvalidValue.
extern "C" hipError_t qpk_launch_jvp(const qpk::JvpArgs* a, int tiled, hipStream_t stream);
