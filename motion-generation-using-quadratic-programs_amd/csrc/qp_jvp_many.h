// qp_jvp_many.h — what qp_jvp_many.hip exports to qpgpu_api.cpp: the argument block of the forward-mode
// sensitivities along several directions (include/qpgpu.h qpgpu_jvp_many / qpgpu_jvp_box_many), its
// launch and the name of the kernel it runs.
#pragma once

#include "qp_jvp.h"

namespace qpk {

// JvpArgs with every tangent and output holding ntan blocks per QP, direction-major: direction k's
// element e of an array of E elements per QP and direction is element k * E + e of the QP's block.
struct JvpManyArgs {
  JvpArgs a;
  int ntan;  // >= 1
};

}  // namespace qpk

// The kernel a launch of this n runs: NULL for n outside [1, 64].
extern "C" const char* qpk_jvp_many_name(int n);
// Enqueue the sensitivities of QPs [0, a->a.batch) on `stream`; tiled != 0: QPGPU_LAYOUT_TILED64.
// n outside [1, 64] is hipErrorInvalidValue.
extern "C" hipError_t qpk_launch_jvp_many(const qpk::JvpManyArgs* a, int tiled, hipStream_t stream);
