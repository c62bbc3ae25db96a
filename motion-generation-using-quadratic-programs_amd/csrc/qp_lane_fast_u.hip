// qp_lane_fast_u.hip — the QPGPU_FLAG_FAST lane kernels for G, g0, CE or ce0 that are not 16-byte
// aligned: qp_lane.hip with QPGPU_LANE_FAST=1 and QPGPU_LANE_UNALIGNED=1, built with qp_lane_fast's
// flags (Makefile SCHED_ / CONTRACT_qp_lane_fast_u), entry point qpk_launch_lane_fast_u.  See
// qp_lane_u.hip.
#define QPGPU_LANE_FAST 1
#define QPGPU_LANE_UNALIGNED 1
#include "qp_lane.hip"
