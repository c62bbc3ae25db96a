// qp_lane_u.hip — the exact lane kernels for G, g0, CE or ce0 that are not 16-byte aligned:
// qp_lane.hip compiled with QPGPU_LANE_UNALIGNED=1 into its own namespace and entry point
// (qpk_launch_lane_u), every instantiation in this one translation unit.  The staging of G, g0, CE
// and ce0 into LDS is a per-lane 8-byte copy here instead of 16-byte LDS-DMA; the arithmetic is
// the same source under the same flags, so the results are the same bits
// (tests/test_gpu_placement.py).  qpgpu_api.cpp launches it when kArgStage16 is not set.
#define QPGPU_LANE_UNALIGNED 1
#include "qp_lane.hip"
