// qp_vjp_ws_full.hip — qpgpu_vjp_full / qpgpu_vjp_box_full for 64 < n <= 256: qp_vjp_ws.hip built a
// second time with the cotangents on u and f.
#define QPGPU_VJP_FULL 1
#include "qp_vjp_ws.hip"
