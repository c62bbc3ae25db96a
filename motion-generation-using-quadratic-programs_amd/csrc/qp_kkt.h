// qp_kkt.h — what qp_kkt.hip exports to qpgpu_api.cpp: the argument block of the KKT check
// (include/qpgpu.h qpgpu_kkt_residuals / qpgpu_kkt_residuals_box) and its launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpk {

struct KktArgs {
  int n, p, m;
  int group;  // lanes per QP (8, 16, 32 or 64): set by qpk_launch_kkt from n
  int64_t batch, qp0;  // a launch covers QPs [qp0, batch); callers pass qp0 = 0
  const double* G;
  const double* g0;
  const double* CE;
  const double* ce0;
  const double* CI;  // NULL with hi set: the box kernel reads no CI / ci0
  const double* ci0;
  const double* hi;  // non-NULL selects the box kernel (m = 2n)
  const double* lo;
  const double* x;
  const double* u;
  const int32_t* status;  // may be NULL: every QP is evaluated
  double* r;
};

}  // namespace qpk

// Enqueue the check of QPs [0, a->batch) on `stream`; tiled != 0: QPGPU_LAYOUT_TILED64.
extern "C" hipError_t qpk_launch_kkt(const qpk::KktArgs* a, int tiled, hipStream_t stream);
