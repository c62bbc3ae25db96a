// qp_lane_unit_u.hip — the unit-Hessian lane kernels for g0, CE or ce0 that are not 16-byte
// aligned: qp_lane.hip with QPGPU_LANE_UNIT=1 and QPGPU_LANE_UNALIGNED=1, entry point
// qpk_launch_lane_unit_u.  See qp_lane_unit.hip and qp_lane_u.hip.
#define QPGPU_LANE_UNIT 1
#define QPGPU_LANE_UNALIGNED 1
#include "qp_lane.hip"
