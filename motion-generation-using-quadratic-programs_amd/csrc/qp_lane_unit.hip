// qp_lane_unit.hip — the lane kernels of qpgpu_solve_batched_unit (identity Hessian, no G array):
// qp_lane.hip compiled with QPGPU_LANE_UNIT=1 into its own namespace and entry point
// (qpk_launch_lane_unit), under qp_lane's flags (Makefile).  The common launcher with the plain
// mode's run-time-shape instantiations only (kFixedShapes, kHasModes).  The setup is
// stated instead of computed; from there the same source, so the same bits as the exact kernels
// on a materialised identity (tests/test_gpu_unit.py).
#define QPGPU_LANE_UNIT 1
#include "qp_lane.hip"
