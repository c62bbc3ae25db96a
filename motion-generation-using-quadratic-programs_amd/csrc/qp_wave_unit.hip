// qp_wave_unit.hip — the wave kernels of qpgpu_solve_batched_unit (identity Hessian, no G array)
// for the LDS variants of qp_wave.hip (n <= 64, m <= 256): the same source with
// QPGPU_WAVE_UNIT=1, under qp_wave's flags, into its own namespace and entry points
// (qpk_launch_medium_unit).  See qp_wave.hip's header and DESIGN §3.10.
#define QPGPU_WAVE_UNIT 1
#include "qp_wave.hip"
