/*
 * qpgpu.h — C-ABI of the MI355X-native batched Goldfarb–Idnani QP solver.
 *
 * This is the drop-in boundary for the reference's one hot path,
 *   double solve_quadprog(Matrix<double>& G, Vector<double>& g0,
 *                         const Matrix<double>& CE, const Vector<double>& ce0,
 *                         const Matrix<double>& CI, const Vector<double>& ci0,
 *                         Vector<double>& x);
 * declared at reference include/QuadProgpp/QuadProg++.hh:69-72 (body only in the prebuilt
 * lib/QuadProgpp/libquadprog.a, linked at CMakeLists.txt:95) and called from
 * src/mgqp.cpp:708 and src/mgqp.cpp:725.
 *
 * Problem (QuadProg++.hh:8-13, sign convention :35-37):
 *     min 0.5 x^T G x + g0^T x   s.t.  CE^T x + ce0 = 0,  CI^T x + ci0 >= 0
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * The C++ ArrayHH signature above is re-exported by libquadprog_amd.so (see
 * include/quadprog_amd/QuadProg++.hh), which calls qpgpu_solve_batched_host() for one QP.
 *
 * Two batch layouts (qpgpu_problem_desc.layout).  In both, a QP's matrix is row-major exactly
 * as ArrayHH::Matrix stores it (reference Array.hh:910-919: v[0] = new T[n*m],
 * v[i] = v[i-1] + m); e below is that row-major element index.
 *
 * QPGPU_LAYOUT_QP_MAJOR (0, default): QP b occupies a contiguous block in each array:
 *     G  [b][i][j]  at  G  + b*n*n + i*n + j          (n x n)
 *     g0 [b][i]     at  g0 + b*n + i                   (n)
 *     CE [b][i][k]  at  CE + b*n*p + i*p + k           (n x p, i.e. the t(CE) mgqp passes)
 *     ce0[b][k]     at  ce0 + b*p + k                  (p)
 *     CI [b][i][k]  at  CI + b*n*m + i*m + k           (n x m, i.e. the t(CI) mgqp passes)
 *     ci0[b][k]     at  ci0 + b*m + k                  (m)
 *     x  [b][i]     at  x  + b*n + i                   (n, output)
 *     f[b], status[b], iters[b]                        (outputs; iters may be NULL)
 *
 * QPGPU_LAYOUT_TILED64 (1): QPs are grouped in tiles of 64; inside a tile the element index
 * is the slow axis and the QP index the fast one, so lane t of a wavefront reading element e of
 * QP 64k+t touches consecutive addresses (fully coalesced 512-B rows):
 *     element e of a per-QP block of E elements (E = n*n for G, n for g0/x, n*p for CE, ...)
 *     of QP b lives at  X + (b / 64) * 64 * E + e * 64 + (b % 64).
 *     Arrays hold ceil(batch/64) whole tiles; f, status, iters stay one value per QP.
 * qpgpu_relayout() converts one array between the two layouts on the device.
 *
 * Where the arrays may lie (every device-pointer entry below):
 *   - Natural alignment is sufficient: 8 bytes for the float64 arrays, 4 for the int32 ones.  No
 *     entry needs more, and results do not depend on the alignment: every output is the same bits
 *     wherever the arrays lie.
 *   - 16-byte alignment of the float64 INPUT arrays enables the staged paths of the lane kernels
 *     (n <= 8, m <= 16), in two independent groups: G, g0 and, with p > 0, CE and ce0 (their copy
 *     into on-chip memory by 16-byte transfers); CI and ci0 (the on-chip copy of CI and 16-byte row
 *     loads).  A group with a member that is only 8-byte aligned runs 8-byte paths instead: slower,
 *     same bits.  hipMalloc and torch allocations are aligned far beyond this.
 *   - A pointer into a larger batch is legal: to solve QPs [b0, b0 + B) of arrays that hold more,
 *     pass every per-QP array advanced by b0 blocks (X + b0*E for a block of E elements, f + b0,
 *     status + b0, ...) and batch = B.  In QPGPU_LAYOUT_QP_MAJOR any b0 will do (an odd b0 moves an
 *     array with odd E to 8 mod 16: see above); in QPGPU_LAYOUT_TILED64 b0 must be a multiple of
 *     64, a whole-tile boundary, and the last tile touched must exist whole.
 *   - A call writes x, f, status, iters (and x_eq, f_eq, status_eq, u, nact where the entry has
 *     them) of its own QPs and nothing else: no element before, between or after them, no TILED64
 *     padding slot, and no input (G only with QPGPU_FLAG_WRITE_FACTOR).  x (and x_eq) of a QP whose
 *     status is QPGPU_QP_NOT_POSITIVE_DEFINITE is left as it was.
 */
#ifndef QPGPU_H
#define QPGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QPGPU_ABI_VERSION 1

/* ---- per-QP status (what the reference does for that QP) -------------------------------- */
enum qpgpu_qp_status {
  /* solve_quadprog returned normally; f[b] is its return value (may be NaN, as mgqp.cpp:717 expects). */
  QPGPU_QP_OK = 0,
  /* returned std::numeric_limits<double>::infinity() through the "t >= inf" exit
     (QuadProg++.hh:27-29: problem infeasible, x not meaningful); f[b] = +inf. */
  QPGPU_QP_INFEASIBLE = 1,
  /* cholesky_decomposition hit sum <= 0: the reference prints G and throws
     std::logic_error("Error in cholesky decomposition, sum: <sum>").  f[b] holds that sum. */
  QPGPU_QP_NOT_POSITIVE_DEFINITE = 2,
  /* add_constraint failed in the equality phase: std::runtime_error("Constraints are linearly
     dependent").  f[b] holds the objective accumulated so far. */
  QPGPU_QP_DEPENDENT = 3,
  /* The safety cap on active-set steps was reached.  The reference has no cap (it would loop);
     the cap only exists so every GPU wave terminates and never fires on terminating problems. */
  QPGPU_QP_MAX_ITER = 4
};

/* ---- API return codes ------------------------------------------------------------------- */
enum qpgpu_error {
  QPGPU_SUCCESS = 0,
  QPGPU_ERR_INVALID_ARGUMENT = 1,  /* NULL pointer, negative size, n == 0, ...              */
  QPGPU_ERR_UNSUPPORTED_SHAPE = 2, /* (n, p, m) outside what the compiled kernels cover      */
  QPGPU_ERR_HIP = 3,               /* a HIP runtime call failed (message: qpgpu_last_error) */
  QPGPU_ERR_NO_DEVICE = 4          /* no gfx950 device visible                              */
};

/* batch layouts (see the top of this file) */
#define QPGPU_LAYOUT_QP_MAJOR 0u
#define QPGPU_LAYOUT_TILED64 1u

/* flags */
#define QPGPU_FLAG_WRITE_FACTOR 0x1u  /* write the Cholesky factor back into G, as the
                                          reference does (QuadProg++.hh:42-45).  Off by default
                                          in batched use: it is extra HBM traffic. */

#define QPGPU_FLAG_EXACT 0x2u         /* keep the reference's floating-point operation order
                                          everywhere, so x and f are bit-identical to the CPU
                                          restatement of QuadProg++'s order (SURVEY §3.2;
                                          reference-pinned on the demo KAT only).
                                          Shapes with n <= 64 and m <= 256 always do.  The
                                          others (n > 64, or m > 256, which the workspace
                                          variant serves) by default run the O(n^3) setup
                                          (Cholesky, J = L^-T, x0) as blocked f64 MFMA
                                          (qp_panel.hip) and the loop's d, z, r sums as tree
                                          sums, which match within 1e-10 relative (same status
                                          and iteration counts) instead.  Implied by
                                          QPGPU_FLAG_WRITE_FACTOR. */

#define QPGPU_FLAG_FAST 0x4u          /* n <= 64, m <= 256 (the lane kernel's shapes and the wave
                                          kernel's LDS variants: C1, C2, the mgqp levels, C3):
                                          run the fast builds — multiply-adds fused, one refined
                                          reciprocal per divisor, rotation lengths as
                                          sqrt(a^2 + b^2) inside the exponent range — whose x and
                                          f match the reference within 1e-10 relative per QP
                                          (||x - x_ref||_inf / ||x_ref||_inf, |f - f_ref| /
                                          |f_ref|) with the same decisions on well-conditioned
                                          problems, instead of bit for bit.  Other shapes run as
                                          without it (n > 64 already defaults to the 1e-10 MFMA
                                          panel path).  Not combinable with QPGPU_FLAG_EXACT or
                                          QPGPU_FLAG_WRITE_FACTOR (QPGPU_ERR_INVALID_ARGUMENT). */

/* Kernel-family selection (benchmarking / testing knobs; default = fastest for the shape):
 *   LANE      one QP per lane (qp_lane.hip, n <= 8, m <= 16)
 *   SUBGROUP  one QP per S-lane subgroup, register state (qp_small.hip, n <= 16, m <= 64)
 *   WAVE      one QP per 32/64/256 lanes, LDS / workspace state (qp_wave.hip, n <= 256,
 *             m <= 1024; n > 64 uses a cached device workspace of ~1 MiB per QP, allocated by
 *             the first call for that size — call once before capturing into a hipGraph)
 *   GENERIC   one QP per 256-thread workgroup, every array in a device workspace sized from
 *             (n, m) at run time (qp_generic.hip): ANY shape with n*n and n*m below 2^31, as the
 *             reference's solve_quadprog takes any n, p, m (QuadProg++.hh:69-72).  The default
 *             for the shapes no other family covers (n > 256 or m > 1024); bitwise with the
 *             reference's operation order; ~2 n^2 + 12 n + 2 m doubles of workspace per QP.
 * Forcing a family that does not cover the shape returns QPGPU_ERR_UNSUPPORTED_SHAPE.
 * (Bit 0x1000 selected a lane-pair kernel in ABI 4's round-4 builds; it measured slower than
 * LANE and was removed from the library — the bit is now unknown: QPGPU_ERR_INVALID_ARGUMENT.) */
#define QPGPU_FLAG_FORCE_LANE 0x100u
#define QPGPU_FLAG_FORCE_SUBGROUP 0x200u
#define QPGPU_FLAG_FORCE_WAVE 0x400u
#define QPGPU_FLAG_FORCE_GENERIC 0x800u

typedef struct qpgpu_problem_desc {
  int32_t n;         /* variables                      (G.ncols() in the reference)  */
  int32_t p;         /* equality constraints           (CE.ncols())                  */
  int32_t m;         /* inequality constraints         (CI.ncols())                  */
  int32_t max_iter;  /* safety cap on active-set steps per QP; <= 0 selects the default */
  int64_t batch;     /* number of independent QPs                                    */
  uint32_t flags;    /* QPGPU_FLAG_*                                                  */
  uint32_t layout;   /* QPGPU_LAYOUT_* (0 = QP-major)                                  */
} qpgpu_problem_desc;

/* Solve `d->batch` independent QPs.  Every pointer is DEVICE memory (hipMalloc'd or a torch
 * tensor's data_ptr on the current device); `stream` is a hipStream_t (NULL = default stream).
 * The call only enqueues work and does not synchronise, so it can be captured into a hipGraph.
 * Shapes with n > 64 (J and R in global memory) use a device workspace cached per
 * (device, stream): the first call on a stream allocates it (do that before capturing), and
 * launches on different streams never share one.  Host threads may call concurrently, on one
 * stream or several: the workspace cache's lock is held until a call's launches are enqueued, so
 * launches on one stream share its workspace in stream order.  G is read-only unless
 * QPGPU_FLAG_WRITE_FACTOR is set.
 * `iters` (l1 passes per QP, the reference's `iter`) may be NULL.
 * Replaces: the per-QP call at reference src/mgqp.cpp:708, batched. */
int qpgpu_solve_batched(const qpgpu_problem_desc* d,
                        double* G, const double* g0,
                        const double* CE, const double* ce0,
                        const double* CI, const double* ci0,
                        double* x, double* f, int32_t* status, int32_t* iters,
                        void* stream);

/* Same as qpgpu_solve_batched, plus, per QP, the answer of the same problem with the
 * inequality constraints dropped (m = 0): x_eq (n doubles, same layout as x), f_eq, status_eq.
 * That is the state the full solve passes through after its equality phase, so it costs a
 * few stores, and it is bit-identical to a separate qpgpu_solve_batched with m = 0.  This is
 * the retry of reference src/mgqp.cpp:717-736 (solve_quadprog again with CI of 0 columns)
 * folded into the first solve. */
int qpgpu_solve_batched_eq(const qpgpu_problem_desc* d,
                           double* G, const double* g0,
                           const double* CE, const double* ce0,
                           const double* CI, const double* ci0,
                           double* x, double* f, int32_t* status, int32_t* iters,
                           double* x_eq, double* f_eq, int32_t* status_eq,
                           void* stream);

/* Same as qpgpu_solve_batched, plus the dual side of each QP: the Lagrange multipliers and the
 * size of the final active set.  Device pointers, enqueue only, graph-capturable like it.
 *
 * u is the multiplier vector the reference's Goldfarb-Idnani iteration holds when it returns
 * (its local u[0..iq) with the index array A[0..iq)), written dense, p + m doubles per QP in the
 * layout of x (QP-major: u + b*(p+m) + j; TILED64: a per-QP block of E = p + m elements):
 *     u[b][j]      j < p   multiplier of equality j
 *     u[b][p + i]  i < m   multiplier of inequality i
 * Every constraint that is not in the final active set is exactly +0.0.  nact[b] (may be NULL) is
 * the number of active inequalities.  For any status other than QPGPU_QP_OK the whole block is
 * +0.0 and nact[b] = 0 (that includes QPGPU_QP_NOT_POSITIVE_DEFINITE, where the reference
 * throws before u exists).  With p + m == 0, u is not touched and may be NULL; otherwise a NULL u
 * is QPGPU_ERR_INVALID_ARGUMENT.
 *
 * Sign convention (the problem statement at the top of this file): at a solution
 *     G x + g0 = CE u[0:p] + CI u[p:],   u[p:] >= 0,   u[p+i] != 0 only where CI[:,i]^T x + ci0[i] = 0.
 *
 * u is whatever the reference's arithmetic holds, like every other output, including one quirk:
 * when a full step's add_constraint finds the new column dependent, the reference rolls back x
 * and the INEQUALITIES' multipliers u[p..iq) to their values at the last l1 pass but leaves the
 * equalities' u[0..p) as the abandoned step updated them.  On well-posed data this path is not
 * taken (or changes u below its rounding); on adversarially scaled or tied inputs u can then
 * miss the identities above while x is still the reference's, bit for bit.
 *
 * x, f, status and iters are bit-identical to qpgpu_solve_batched with QPGPU_FLAG_EXACT on the
 * same inputs: the entry always runs the reference's operation order, as if QPGPU_FLAG_EXACT
 * were set.  This matters for n > 64 or m > 256, whose default tolerance mode (MFMA panel setup,
 * tree sums, certification and re-solve launch) has no dual form.  QPGPU_FLAG_FAST is
 * QPGPU_ERR_INVALID_ARGUMENT here (the fast builds have no dual form either);
 * QPGPU_FLAG_WRITE_FACTOR, both layouts and the QPGPU_FLAG_FORCE_* flags work as in
 * qpgpu_solve_batched. */
int qpgpu_solve_batched_dual(const qpgpu_problem_desc* d,
                             double* G, const double* g0,
                             const double* CE, const double* ce0,
                             const double* CI, const double* ci0,
                             double* x, double* f, int32_t* status, int32_t* iters,
                             double* u, int32_t* nact, void* stream);

/* Bound constraints without a dense CI:
 *     min 1/2 x^T G x + g0^T x   s.t.   CE^T x + ce0 = 0,   lo <= x <= hi.
 * Device pointers, enqueue only, graph-capturable like qpgpu_solve_batched.  hi and lo are n
 * doubles per QP in the layout of x (QP-major: hi + b*n + k; TILED64: a per-QP block of E = n).
 *
 * The call is DEFINED as the dense problem (n, p, m = 2n) with CI = [-I, +I] and
 * ci0 = [hi; -lo] — the limits matrix of reference src/mgqp.cpp:1080-1136: inequality k < n is
 * the upper bound of variable k, inequality n + k its lower bound.  iters, status, f and max_iter
 * mean what they mean for that dense problem, and d->m must be 2 * d->n (anything else is
 * QPGPU_ERR_INVALID_ARGUMENT).  hi[k] = +inf or lo[k] = -inf means "no bound on that side"; this
 * needs no special handling, the dense form with ci0 = +inf behaves the same way.
 *
 * x, f, status and iters are bit-identical to qpgpu_solve_batched with QPGPU_FLAG_EXACT on the
 * materialised problem (and so to the reference) on every QP for which that solve never forms a
 * non-finite entry of J, z or x: the box kernels keep the one non-zero term of each sum over a
 * column of CI and skip the products with its zeros, which are +-0 exactly when the other factor
 * is finite.  On data that overflows, the dense form turns 0 * inf into NaN and the box form does
 * not; hi = -inf, lo = +inf and NaN bounds are outside the contract for the same reason.
 *
 * The entry always runs the reference's operation order, as if QPGPU_FLAG_EXACT were set (the
 * n > 64 tolerance mode has no box form), and QPGPU_FLAG_FAST is QPGPU_ERR_INVALID_ARGUMENT.
 * QPGPU_FLAG_WRITE_FACTOR, both layouts and the QPGPU_FLAG_FORCE_* flags work as in
 * qpgpu_solve_batched (a forced family that does not cover (n, p, 2n) is
 * QPGPU_ERR_UNSUPPORTED_SHAPE); the default dispatch follows its order for (n, p, 2n).  NULL hi or
 * lo with batch > 0 is QPGPU_ERR_INVALID_ARGUMENT; CE and ce0 may be NULL when p = 0. */
int qpgpu_solve_batched_box(const qpgpu_problem_desc* d,
                            double* G, const double* g0,
                            const double* CE, const double* ce0,
                            const double* hi, const double* lo,
                            double* x, double* f, int32_t* status, int32_t* iters,
                            void* stream);

/* Name of the kernel a qpgpu_solve_batched_box launch of shape (n, p) with these flags runs
 * (every box kernel's name contains "box"); "" for a rejected flag combination or n <= 0. */
const char* qpgpu_kernel_name_box(int32_t n, int32_t p, uint32_t flags);

/* qpgpu_solve_batched_box plus the dual side: the multipliers of the equalities and of the bounds,
 * and the size of the final active set.  Device pointers, enqueue only, graph-capturable.
 *
 * The call is DEFINED as qpgpu_solve_batched_dual on the materialised problem (n, p, m = 2n) with
 * CI = [-I, +I], ci0 = [hi; -lo], on every QP that meets the finite-data condition of
 * qpgpu_solve_batched_box (its comment above): x, f, status and iters are the bits of
 * qpgpu_solve_batched_box, u and nact the bits of qpgpu_solve_batched_dual on that dense problem.
 * u is dense, p + 2n doubles per QP in the layout of x (QP-major: u + b*(p+2n) + j; TILED64: a
 * per-QP block of E = p + 2n elements):
 *     u[b][j]          j < p   multiplier of equality j
 *     u[b][p + k]      k < n   multiplier of the upper bound of variable k (x[k] <= hi[k])
 *     u[b][p + n + k]  k < n   multiplier of the lower bound of variable k (x[k] >= lo[k])
 * Every slot outside the final active set is exactly +0.0; any status other than QPGPU_QP_OK gives
 * an all-+0.0 block and nact[b] = 0.  nact may be NULL; a NULL u is QPGPU_ERR_INVALID_ARGUMENT
 * (p + 2n > 0 always).
 *
 * Sign convention: that of qpgpu_solve_batched_dual with CI = [-I, +I], i.e. at a solution
 *     G x + g0 = CE u[0:p] - u[p:p+n] + u[p+n:],   u[p:] >= 0,
 * and u[p + k] != 0 only where x[k] sits on that bound.  The rollback quirk described at
 * qpgpu_solve_batched_dual is kept.
 *
 * Arguments: the union of the two entries' rules.  d->m must be 2 * d->n, NULL hi or lo with
 * batch > 0 and QPGPU_FLAG_FAST are QPGPU_ERR_INVALID_ARGUMENT, QPGPU_FLAG_EXACT is implied, CE
 * and ce0 may be NULL when p = 0.  QPGPU_FLAG_WRITE_FACTOR, both layouts, max_iter, the
 * QPGPU_FLAG_FORCE_* flags and the default dispatch work as in qpgpu_solve_batched_box.  No kernel
 * behind this entry reads a CI or ci0, and none is written anywhere. */
int qpgpu_solve_batched_box_dual(const qpgpu_problem_desc* d,
                                 double* G, const double* g0,
                                 const double* CE, const double* ce0,
                                 const double* hi, const double* lo,
                                 double* x, double* f, int32_t* status, int32_t* iters,
                                 double* u, int32_t* nact, void* stream);

/* Name of the kernel a qpgpu_solve_batched_box_dual launch of shape (n, p) with these flags runs
 * (every such name contains "box" and "dual"); "" where qpgpu_kernel_name_box returns "". */
const char* qpgpu_kernel_name_box_dual(int32_t n, int32_t p, uint32_t flags);

/* The identity Hessian without a G array:
 *     min 1/2 x^T x + g0^T x   s.t.   CE^T x + ce0 = 0,   CI^T x + ci0 >= 0,
 * the Euclidean projection of -g0 onto a polytope, and the form of every QP the reference's
 * controller solves (src/mgqp.cpp:672-708: JG = Identity, g0 = 0).  Device pointers, enqueue only,
 * graph-capturable like qpgpu_solve_batched (no workspace: a first call can be captured); both
 * layouts, natural alignment, sub-ranges of a larger batch; only the outputs of its own QPs are
 * written.  x_eq, f_eq and status_eq are the m = 0 answers of qpgpu_solve_batched_eq: pass all
 * three or none (a mixed triple is QPGPU_ERR_INVALID_ARGUMENT).
 *
 * The call is DEFINED as qpgpu_solve_batched with QPGPU_FLAG_EXACT (qpgpu_solve_batched_eq with
 * the triple) on the same arrays and a materialised G = I.  The setup is stated, not computed:
 *     J = I (1.0 on the diagonal, +0.0 elsewhere),   c1 = c2 = the ascending sum of n ones,
 *     x0[i] = -g0[i] (IEEE negation),   f0 = 0.5 * sum_i g0[i] * x0[i] (ascending from +0.0, each
 *     product rounded),   R_norm = 1,   iq = 0,
 * and from there the reference's algorithm runs unchanged.  x, f, status and iters (and x_eq,
 * f_eq, status_eq) are bit-identical to that dense solve, and so to the reference, on every QP
 * whose g0 entries are all finite and none of which is -0.0: the dense setup forms
 * g0[i] - (+0.0 * y[k]), which is g0[i] exactly unless y[k] is non-finite, and whose sign for
 * g0[i] = -0.0 depends on the signs of the other entries.  The reference's own g0 = +0.0 is
 * inside the contract; NaN, +-inf and -0.0 entries of g0 are outside it.
 *
 * QPGPU_FLAG_EXACT is accepted and implied.  QPGPU_FLAG_FAST (there is no fast unit form) and
 * QPGPU_FLAG_WRITE_FACTOR (there is no G to write a factor into) are QPGPU_ERR_INVALID_ARGUMENT.
 * With batch > 0 a NULL g0, x, f or status, a NULL CE or ce0 with p > 0 and a NULL CI or ci0 with
 * m > 0 are QPGPU_ERR_INVALID_ARGUMENT; iters may be NULL; batch = 0 is QPGPU_SUCCESS.
 * Shapes: n <= 64 and m <= 256 (the lane, subgroup and wave-LDS families); the default dispatch
 * follows qpgpu_solve_batched's order for (n, p, m), and QPGPU_FLAG_FORCE_LANE / _SUBGROUP / _WAVE
 * work as there.  n > 64, m > 256, QPGPU_FLAG_FORCE_GENERIC and a forced family that does not
 * cover the shape are QPGPU_ERR_UNSUPPORTED_SHAPE. */
int qpgpu_solve_batched_unit(const qpgpu_problem_desc* d,
                             const double* g0,
                             const double* CE, const double* ce0,
                             const double* CI, const double* ci0,
                             double* x, double* f, int32_t* status, int32_t* iters,
                             double* x_eq, double* f_eq, int32_t* status_eq,
                             void* stream);

/* Name of the kernel a qpgpu_solve_batched_unit launch of shape (n, p, m) with these flags runs
 * (every unit kernel's name contains "unit"); "" where the entry would refuse the flags or the
 * shape. */
const char* qpgpu_kernel_name_unit(int32_t n, int32_t p, int32_t m, uint32_t flags);

/* ---- the KKT check: is (x, u) a solution of its QP? ---------------------------------------------
 * qpgpu_kkt_residuals evaluates, on the device, the optimality conditions of every QP of a batch
 * at a given primal-dual pair: QPGPU_KKT_NRES doubles per QP, independent of any reference solver.
 * It is the caller's means to detect multipliers that miss the identities at
 * qpgpu_solve_batched_dual (the rollback quirk) and to certify an x of the 1e-10 modes.
 *
 * Device pointers, enqueue only.  No workspace for any shape: the first call for a shape can be
 * captured into a hipGraph.  Inputs are laid out exactly as qpgpu_solve_batched_dual takes and
 * produces them (u: p + m doubles per QP), in either layout; r is QPGPU_KKT_NRES doubles per QP in
 * the layout of x (QP-major: r + b*8 + k; TILED64: a per-QP block of E = 8).  Natural alignment and
 * sub-ranges as at the top of this file; the call writes the r blocks of its own QPs and nothing
 * else (no TILED64 padding slot, no input).  Every shape the solve entries accept (n >= 1, n*n and
 * n*m below 2^31; beyond: QPGPU_ERR_UNSUPPORTED_SHAPE).  d->max_iter is ignored; d->flags must be 0.
 * Decided before any array is read, QPGPU_ERR_INVALID_ARGUMENT: non-zero flags; a NULL u with
 * p + m > 0; with batch > 0 a NULL G, g0, x or r, a NULL CE / ce0 with p > 0, a NULL CI / ci0 with
 * m > 0.  batch = 0 is QPGPU_SUCCESS.  status may be NULL: every QP is evaluated.  With status
 * given, a QP whose status is not QPGPU_QP_OK gets all eight slots NaN (its x is not meaningful,
 * and was never written for QPGPU_QP_NOT_POSITIVE_DEFINITE).
 *
 * The definition, which the kernel reproduces bit for bit (tests/kkt_ref.py restates it).
 * ue = u[0:p], ui = u[p:]; |.| is fabs; every sum starts from +0.0 and adds in ascending index;
 * every product is rounded before it is added (no FMA); every division is IEEE;
 *     ratio(a, b) = b > 0 ? a / b : a
 *     smax(acc, v) = acc is NaN ? acc : ((v > acc || v != v) ? v : acc)
 * and every running maximum uses smax from +0.0, so a NaN anywhere is kept.  G is read as stored,
 * row by row: the check assumes the symmetric G the solver assumes.
 *   for each row i < n:
 *     a_i  = sum_j G[i][j] x[j]             aa_i = sum_j |G[i][j]| |x[j]|
 *     c_i  = sum_k<p CE[i][k] ue[k]         ca_i = sum_k |CE[i][k]| |ue[k]|
 *     d_i  = sum_k<m CI[i][k] ui[k]         da_i = sum_k |CI[i][k]| |ui[k]|
 *     t_i  = ((a_i + g0[i]) - c_i) - d_i    ts_i = ((aa_i + |g0[i]|) + ca_i) + da_i
 *     stat = smax_i |t_i|     scale = smax_i ts_i     q = sum_i x[i] a_i     l = sum_i g0[i] x[i]
 *   for each equality k < p:    e_k = (sum_i CE[i][k] x[i]) + ce0[k]   ea_k = (sum_i |CE[i][k]| |x[i]|) + |ce0[k]|
 *   for each inequality k < m:  s_k = (sum_i CI[i][k] x[i]) + ci0[k]   sa_k = (sum_i |CI[i][k]| |x[i]|) + |ci0[k]|
 *   r[QPGPU_KKT_STAT]       = ratio(stat, scale)    scaled stationarity residual of G x + g0 = CE ue + CI ui
 *   r[QPGPU_KKT_STAT_SCALE] = scale
 *   r[QPGPU_KKT_EQ]         = smax_k ratio(|e_k|, ea_k)
 *   r[QPGPU_KKT_INEQ]       = smax_k ( s_k < 0 ? ratio(-s_k, sa_k) : (s_k != s_k ? NaN : 0.0) )
 *   r[QPGPU_KKT_COMP]       = smax over k with ui[k] != 0 of ratio(|s_k|, sa_k)
 *   r[QPGPU_KKT_UMIN]       = the smallest ui[k] that is < 0, else +0.0  (running v < acc ? v : acc from +0.0)
 *   r[QPGPU_KKT_OBJ]        = 0.5 q + l
 *   r[QPGPU_KKT_NNZ]        = the number of k with ui[k] != 0, as a double
 * Slots STAT, EQ, INEQ and COMP are residuals over the magnitude of their own terms: a solution in
 * binary64 leaves them at a small multiple of 2^-53 at every scaling of the problem.  A bound
 * ci0[k] = +inf gives s_k = +inf: no violation and, with ui[k] == 0, no complementarity term. */
#define QPGPU_KKT_NRES 8
enum { QPGPU_KKT_STAT, QPGPU_KKT_STAT_SCALE, QPGPU_KKT_EQ, QPGPU_KKT_INEQ,
       QPGPU_KKT_COMP, QPGPU_KKT_UMIN, QPGPU_KKT_OBJ, QPGPU_KKT_NNZ };

int qpgpu_kkt_residuals(const qpgpu_problem_desc* d,
                        const double* G, const double* g0, const double* CE, const double* ce0,
                        const double* CI, const double* ci0,
                        const double* x, const double* u, const int32_t* status,
                        double* r, void* stream);

/* The same for bounds lo <= x <= hi, with u in the layout of qpgpu_solve_batched_box_dual.  DEFINED
 * as qpgpu_kkt_residuals on CI = [-I, +I], ci0 = [hi; -lo] (d->m must be 2 * d->n; NULL hi or lo
 * with batch > 0 is QPGPU_ERR_INVALID_ARGUMENT) and equal to it bit for bit under the finite-data
 * condition stated at qpgpu_solve_batched_box: each sum over a row or column of that CI is its one
 * or two non-zero terms added to the +0.0 it starts from,
 *     d_i = (0.0 - u[p+i]) + u[p+n+i]            da_i = (0.0 + |u[p+i]|) + |u[p+n+i]|
 *     s_k = (0.0 - x[k]) + hi[k]                 sa_k = (0.0 + |x[k]|) + |hi[k]|        (k < n)
 *     s_(n+k) = (0.0 + x[k]) + (-lo[k])          sa_(n+k) = (0.0 + |x[k]|) + |-lo[k]|
 * The kernel reads no CI. */
int qpgpu_kkt_residuals_box(const qpgpu_problem_desc* d,
                            const double* G, const double* g0, const double* CE, const double* ce0,
                            const double* hi, const double* lo,
                            const double* x, const double* u, const int32_t* status,
                            double* r, void* stream);

/* ---- the backward step: gradients of the solution with respect to the data ------------------------
 * qpgpu_vjp evaluates, on the device, the vector-Jacobian product of every QP of a batch: given
 * gx = dl/dx at the solution x* of
 *     min 0.5 x^T G x + g0^T x   s.t.  CE^T x + ce0 = 0,  CI^T x + ci0 >= 0,
 * the gradients of l with respect to G, g0, CE, ce0, CI and ci0.  With A = [CE, CI_act] the n x q
 * matrix of working columns, lam their multipliers and b their offsets, the solution satisfies
 * G x + g0 = A lam and A^T x + b = 0; solving  G a + A c = gx,  A^T a = 0  gives
 *     dg0 = -a,   dG = -1/2 (a x^T + x a^T),   dA = a lam^T - x c^T,   db = -c.
 * dG is the gradient with respect to a SYMMETRIC G, the G the solver assumes (only its lower
 * triangle is read).  A constraint whose multiplier is exactly 0 is treated as inactive: x* is not
 * differentiable where a constraint is weakly active, and this is the one-sided choice made there.
 * Cotangents on f or on the multipliers are not taken here: qpgpu_vjp_full below takes them.
 *
 * Device pointers, enqueue only.  No workspace for any supported shape: the first call for a shape
 * can be captured into a hipGraph.  G, CE, CI, x, u and status are laid out exactly as
 * qpgpu_solve_batched_dual takes and produces them (u: p + m doubles per QP), in either layout; gx
 * is n doubles per QP in the layout of x; every output has the layout and the per-QP size of the
 * input it is the gradient of.  Any output pointer may be NULL: that gradient is then neither
 * computed nor written.  Natural alignment and sub-ranges as at the top of this file; the call
 * writes the requested gradient blocks of its own QPs and nothing else (no TILED64 padding slot, no
 * input).
 *
 * Shapes: n <= 64 with any p and any m (n*n, n*p and n*m below 2^31).  n > 64 is
 * QPGPU_ERR_UNSUPPORTED_SHAPE here: L, M and S of one QP no longer fit on chip, and qpgpu_vjp_ws
 * below serves 64 < n <= 256 from a workspace the caller provides.  d->max_iter is
 * ignored; d->flags must be 0.  Decided before any array is read, QPGPU_ERR_INVALID_ARGUMENT:
 * non-zero flags; a NULL u with p + m > 0; with batch > 0 a NULL G, x or gx, a NULL CE with p > 0, a
 * NULL CI with m > 0.  batch = 0 is QPGPU_SUCCESS.  status may be NULL: every QP is evaluated.  With
 * status given, a QP whose status is not QPGPU_QP_OK gets +0.0 in every requested output: no
 * gradient flows through a failed QP.
 *
 * The definition, which the kernels reproduce bit for bit (tests/vjp_ref.py restates it).  No FMA:
 * every product is rounded before it is added or subtracted; division and sqrt are IEEE; there is
 * no branch on any pivot: a non-positive pivot yields NaN or inf by IEEE rules and propagates.
 *   Working list W: the equalities k = 0..p-1 in order, then the inequalities i in ascending order
 *   with u[p+i] != 0.  q = |W|; col(t) is the CE or CI column at position t, lam(t) its u entry.
 *   If q > n, every requested output element of the QP is NaN.
 *   chol(A), reads the lower triangle only; for j ascending:
 *       s = A[j][j]; for k < j ascending s = s - L[j][k]*L[j][k];  L[j][j] = sqrt(s)
 *       for i > j:  s = A[i][j]; for k < j ascending s = s - L[i][k]*L[j][k];  L[i][j] = s / L[j][j]
 *   fsub(L, r), for i ascending:   s = r[i]; for k < i ascending s = s - L[i][k]*y[k];  y[i] = s / L[i][i]
 *   bsub(L, r) solves L^T z = r, for i descending (N the order of L):
 *       s = r[i]; for k = i+1..N-1 ascending s = s - L[k][i]*z[k];  z[i] = s / L[i][i]
 *   L = chol(G);  w = fsub(L, gx);  M[:,t] = fsub(L, col(t)) for t < q
 *   S[s][t] = sum_i M[i][s]*M[i][t] for s >= t,  r[t] = sum_i M[i][t]*w[i]   (from +0.0, i ascending)
 *   R = chol(S);  c = bsub(R, fsub(R, r))
 *   y[i] = w[i], then for t ascending y[i] = y[i] - M[i][t]*c[t];  a = bsub(L, y)
 *   dg0[i]    = -a[i]
 *   dG[i][j]  = -0.5 * (a[i]*x[j] + x[i]*a[j])                  (bit-symmetric)
 *   dCE[i][k] = a[i]*u[k] - x[i]*c[k]        dce0[k] = -c[k]
 *   inequality j at position t of W:  dCI[i][j] = a[i]*u[p+j] - x[i]*c[t],  dci0[j] = -c[t]
 *   inequality j not in W:            dCI[i][j] = +0.0,                      dci0[j] = +0.0
 * The Goldfarb-Idnani working set has independent columns, so q <= n and S is positive definite
 * on every pair (x, u) the dual solve entries produce with QPGPU_QP_OK. */
int qpgpu_vjp(const qpgpu_problem_desc* d,
              const double* G, const double* CE, const double* CI,
              const double* x, const double* u, const int32_t* status,
              const double* gx,
              double* dG, double* dg0, double* dCE, double* dce0, double* dCI, double* dci0,
              void* stream);

/* The same for bounds lo <= x <= hi, with u in the layout of qpgpu_solve_batched_box_dual (d->m must
 * be 2 * d->n: anything else is QPGPU_ERR_INVALID_ARGUMENT).  DEFINED as qpgpu_vjp on CI = [-I, +I]
 * (column k < n: -1.0 at row k among -0.0; column n + k: +1.0 at row k among +0.0, the matrix
 * BoxProblems.to_dense() of the Python mirror materialises) and equal to it bit for bit; the kernel
 * generates those columns, reads no CI and writes no dCI.  dhi and dlo are n doubles per QP in the
 * layout of x:
 *     dhi[k] = -c[t] if the upper bound of k is at position t of W (u[p+k] != 0),    else +0.0
 *     dlo[k] = +c[t] if the lower bound of k is at position t of W (u[p+n+k] != 0),  else +0.0
 * (ci0 = [hi; -lo], so dhi = dci0[0:n] and dlo = -dci0[n:2n] on the active bounds). */
int qpgpu_vjp_box(const qpgpu_problem_desc* d,
                  const double* G, const double* CE,
                  const double* x, const double* u, const int32_t* status,
                  const double* gx,
                  double* dG, double* dg0, double* dCE, double* dce0, double* dhi, double* dlo,
                  void* stream);

/* Name of the kernel a qpgpu_vjp / qpgpu_vjp_box launch of this shape runs: a name containing
 * "lane" (one QP per lane) for n <= 8, "group" (one QP per 16, 32 or 64 lanes) for 8 < n <= 64,
 * "" for n > 64 or n <= 0. */
const char* qpgpu_kernel_name_vjp(int32_t n, int32_t p, int32_t m);

/* ---- the backward step with a caller's workspace: n <= 256 ------------------------------------------
 * qpgpu_vjp_ws and qpgpu_vjp_box_ws are qpgpu_vjp and qpgpu_vjp_box with two more arguments, a
 * workspace in device memory and its size.  Everything said at qpgpu_vjp and qpgpu_vjp_box holds
 * unless stated here: the mathematics and the definition, bit for bit; both layouts, natural
 * alignment and sub-ranges; NULL outputs; status masking to +0.0 and q > n giving NaN; d->flags
 * must be 0 and d->max_iter is ignored; the argument rules and their order, all decided before any
 * array is read or anything is launched.
 *
 * Shapes.  n <= 64 runs exactly the launch qpgpu_vjp makes: the same kernel, the same bits; the
 * workspace is not touched and may be NULL with workspace_bytes 0.  64 < n <= 256 with any p and
 * any m (n*p and n*m below 2^31) runs the workspace kernel, one workgroup of 256 lanes per QP in
 * flight.  Not built: n > 256 is QPGPU_ERR_UNSUPPORTED_SHAPE (the kernel gives a row of L, and of
 * S, to a lane of one workgroup).
 *
 * Workspace.  One QP in flight occupies a slot of
 *     per_qp(n, p, m) = 8 * (3*n*n + n) bytes for 64 < n <= 256,   0 for n <= 64
 * (a multiple of 8; p and m do not enter): L (n x n), M with gx as an extra column (n x (n+1)) and
 * S, then R, (n x n); the short vectors and the working list stay on chip.
 * qpgpu_vjp_workspace_bytes writes slots * per_qp to *bytes: QPGPU_ERR_INVALID_ARGUMENT for
 * slots < 1, a NULL bytes, a NULL d or d->n <= 0 (or a negative p, m or batch);
 * QPGPU_ERR_UNSUPPORTED_SHAPE for n > 256.  The entry uses
 *     slots = min(batch, workspace_bytes / per_qp)
 * of them: one resident workgroup per slot, workgroup s walking the QPs s, s + slots, ...  For
 * n > 64 and batch > 0, decided after the rules above and before the device is touched, each of a
 * NULL workspace, a workspace that is not 8-byte aligned and a workspace with room for less than
 * one slot is QPGPU_ERR_INVALID_ARGUMENT.  The workspace's contents on entry do not matter and its
 * contents afterwards are unspecified; the call writes nothing outside
 * [workspace, workspace + slots * per_qp) and its own QPs' requested gradients.  THE RESULTS DO NOT
 * DEPEND ON THE NUMBER OF SLOTS, only the time does.  Calls on one stream may share a workspace
 * (they run in stream order); concurrent streams need one each.
 *
 * The call only enqueues: it allocates nothing and synchronises nothing, so the first call for a
 * shape can be captured into a hipGraph, with the workspace the caller's like every other array. */
int qpgpu_vjp_workspace_bytes(const qpgpu_problem_desc* d, int64_t slots, int64_t* bytes);

int qpgpu_vjp_ws(const qpgpu_problem_desc* d,
                 const double* G, const double* CE, const double* CI,
                 const double* x, const double* u, const int32_t* status,
                 const double* gx,
                 double* dG, double* dg0, double* dCE, double* dce0, double* dCI, double* dci0,
                 void* workspace, int64_t workspace_bytes, void* stream);

int qpgpu_vjp_box_ws(const qpgpu_problem_desc* d,
                     const double* G, const double* CE,
                     const double* x, const double* u, const int32_t* status,
                     const double* gx,
                     double* dG, double* dg0, double* dCE, double* dce0, double* dhi, double* dlo,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* Name of the kernel a qpgpu_vjp_ws / qpgpu_vjp_box_ws launch of this shape runs:
 * qpgpu_kernel_name_vjp's for n <= 64, a name containing "ws" for 64 < n <= 256, "" for n > 256 or
 * n <= 0. */
const char* qpgpu_kernel_name_vjp_ws(int32_t n, int32_t p, int32_t m);

/* ---- the full backward step: cotangents on the multipliers and the optimal value too ---------------
 * qpgpu_vjp_full and qpgpu_vjp_box_full are qpgpu_vjp_ws and qpgpu_vjp_box_ws with two more inputs.
 * For a loss l(x, u, f) of everything a dual solve returns there are three cotangents per QP:
 *     gx = dl/dx   n doubles in the layout of x          (required, as before: zeros if l ignores x)
 *     gu = dl/du   p + m doubles in the layout of u      (box: p + 2n, the layout of
 *                                                         qpgpu_solve_batched_box_dual); may be NULL
 *     gf = dl/df   one double per QP, QP b's at gf[b] in EITHER layout, like f; may be NULL
 * Everything said at qpgpu_vjp_ws holds unless stated here: shapes (n <= 256; n <= 64 does not
 * touch the workspace, which may be NULL with workspace_bytes 0; 64 < n <= 256 takes
 * qpgpu_vjp_workspace_bytes as it is, same slot size, same slot rule, results independent of the
 * number of slots; n > 256 is QPGPU_ERR_UNSUPPORTED_SHAPE), the argument rules and their order, all
 * decided before the device is touched, both layouts, natural alignment, sub-ranges, NULL outputs,
 * status masking to +0.0, q > n giving NaN, enqueue only, no allocation, capturable first call.
 *
 * The mathematics.  With gl(t) the gu entry of the constraint at position t of W, the adjoint
 * system is  G a + A c = gx,  A^T a = -gl:  a cotangent on the multipliers changes only the
 * right-hand side of the q x q solve.  u of an inequality outside W is locally the constant 0 (the
 * one-sided choice of qpgpu_vjp), so its gu entry never enters the arithmetic: it may hold
 * anything, NaN included, without changing a bit of any output.  A cotangent on f needs no solve:
 * by the envelope theorem df/dg0 = x, df/dG = 1/2 x x^T, df/dA = -x lam^T, df/db = -lam.
 *
 * The definition is qpgpu_vjp's with exactly two additions (tests/vjp_full_ref.py restates it).
 *   With gu given:   r[t] = (sum_i M[i][t]*w[i]) + gl(t): the sum as before, gl(t) added once, after
 *     it;  gl(t) = gu[t] for t < p,  gl(t) = gu[p+j] for inequality (or bound) j at position t.
 *   With gf given, g = gf[b]:
 *     hh = 0.5*g;  ah[i] = a[i] - hh*x[i];  dG[i][j] = -0.5 * (ah[i]*x[j] + x[i]*ah[j])  (bit-symmetric)
 *     dg0[i] = -(a[i] - g*x[i])
 *     ct[t] = c[t] + g*lam(t), and ct replaces c in dCE, dce0, dCI, dci0, dhi and dlo:
 *     dCE[i][k] = a[i]*u[k] - x[i]*ct[k],  dce0[k] = -ct[k],  dhi[k] = -ct[t],  dlo[k] = +ct[t], ...
 *     (a, not ah, stays in dCE and dCI;  y = w - M c still uses c).
 * With gu == NULL and gf == NULL every output is bit-identical to qpgpu_vjp_ws / qpgpu_vjp_box_ws
 * (and so to qpgpu_vjp for n <= 64): a NULL cotangent adds no operation, not even a + 0.0. */
int qpgpu_vjp_full(const qpgpu_problem_desc* d,
                   const double* G, const double* CE, const double* CI,
                   const double* x, const double* u, const int32_t* status,
                   const double* gx, const double* gu, const double* gf,
                   double* dG, double* dg0, double* dCE, double* dce0, double* dCI, double* dci0,
                   void* workspace, int64_t workspace_bytes, void* stream);

int qpgpu_vjp_box_full(const qpgpu_problem_desc* d,
                       const double* G, const double* CE,
                       const double* x, const double* u, const int32_t* status,
                       const double* gx, const double* gu, const double* gf,
                       double* dG, double* dg0, double* dCE, double* dce0, double* dhi, double* dlo,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* Name of the kernel a qpgpu_vjp_full / qpgpu_vjp_box_full launch of this shape runs: a name
 * containing "full", and "lane" for n <= 8, "group" for 8 < n <= 64, "ws" for 64 < n <= 256; "" for
 * n > 256 or n <= 0. */
const char* qpgpu_kernel_name_vjp_full(int32_t n, int32_t p, int32_t m);

/* ---- forward-mode sensitivities: how x*, the multipliers and the optimal value move ----------------
 * qpgpu_jvp evaluates, on the device, the Jacobian-vector product of every QP of a batch: given a
 * tangent (tG, tg0, tCE, tce0, tCI, tci0) of the data, the tangents tx of x*, tu of the multipliers
 * and tf of the optimal value.  With A, lam and b as at qpgpu_vjp, G x + g0 = A lam and A^T x + b = 0;
 * differentiating,
 *     G tx - A tlam = h,   A^T tx = k,      h = tA lam - tG x - tg0,   k = -(tA^T x + tb),
 * and with w = L^-1 h:  (M^T M) tlam = k - M^T w,  tx = L^-T (w + M tlam).  By the envelope theorem
 *     tf = 1/2 x^T tG x + tg0^T x + lam^T k.
 * A multiplier outside W is locally the constant 0 (the one-sided choice of qpgpu_vjp): its tu is
 * +0.0, and the column of tCI and the entry of tci0 of an inequality outside W never enter the
 * arithmetic: they may hold anything, NaN included, without changing a bit of any output.  tG is
 * read as stored, row by row: a symmetric tangent is assumed.
 *
 * Device pointers, enqueue only, no allocation, no workspace: a first call can be captured into a
 * hipGraph.  G, CE, CI, x, u and status are laid out as qpgpu_vjp takes them, in either layout; every
 * tangent has the layout and the per-QP size of the array it is the tangent of.  Each tangent may be
 * NULL: a NULL tangent is a zero tangent, and the steps marked [given] below are then not executed.
 * tx is n doubles per QP in the layout of x, tu p + m doubles per QP in the layout of u, tf one
 * double per QP at tf[b] in either layout, like f.  Each output may be NULL: it is then neither
 * computed nor written; all three NULL is QPGPU_SUCCESS and writes nothing.  Natural alignment and
 * sub-ranges as at the top of this file; the call writes the requested outputs of its own QPs and
 * nothing else (no TILED64 padding slot, no input).
 *
 * Shapes: n <= 64 with any p and any m (n*n, n*p and n*m below 2^31); n > 64 is
 * QPGPU_ERR_UNSUPPORTED_SHAPE (a workspace form is not built).  d->max_iter is ignored; d->flags
 * must be 0.  The argument rules and their order are qpgpu_vjp's, decided before any array is read,
 * QPGPU_ERR_INVALID_ARGUMENT: non-zero flags; a NULL u with p + m > 0; with batch > 0 a NULL G or x, a
 * NULL CE with p > 0, a NULL CI with m > 0.  The shape rule comes after these.  batch = 0 is
 * QPGPU_SUCCESS.  status may be NULL: every QP is evaluated.  With status given, a QP whose status is
 * not QPGPU_QP_OK gets +0.0 in every requested output.
 *
 * The definition, which the kernels reproduce bit for bit (tests/jvp_ref.py restates it).  No FMA,
 * every product rounded before it is added or subtracted, IEEE division and sqrt, no branch on a
 * pivot, every sum from +0.0 and ascending.  W, q, col(t), lam(t), chol, fsub and bsub are exactly
 * as at qpgpu_vjp; tcol(t) is the tCE or tCI column at position t, tb(t) its tce0 or tci0 entry.  If
 * q > n, every requested output element of the QP is NaN.
 *   sG[i] = sum_j tG[i][j]*x[j]                                           [tG given; else +0.0]
 *   h[i]  = +0.0;  for t ascending: h[i] = h[i] + tcol(t)[i]*lam(t)       [tCE / tCI given, per matrix]
 *           h[i] = h[i] - sG[i]  [tG given];   h[i] = h[i] - tg0[i]  [tg0 given]
 *   s     = sum_i tcol(t)[i]*x[i]  [given; else +0.0];   s = s + tb(t)  [tce0 / tci0 given];   k[t] = -s
 *   L = chol(G);  w = fsub(L, h);  M[:,t] = fsub(L, col(t))
 *   S[s][t] = sum_i M[i][s]*M[i][t] for s >= t,   rs[t] = sum_i M[i][t]*w[i]
 *   r[t] = k[t] - rs[t];  R = chol(S);  dl = bsub(R, fsub(R, r))
 *   y[i] = w[i], then for t ascending y[i] = y[i] + M[i][t]*dl[t];  tx = bsub(L, y)
 *   tu[k] = dl[k] for k < p;  tu[p+j] = dl[t] for inequality j at position t of W;  +0.0 elsewhere
 *   qq = sum_i x[i]*sG[i];  ll = sum_i tg0[i]*x[i]  [tg0 given; else +0.0];  kk = sum_t lam(t)*k[t]
 *   tf = ((0.5*qq) + ll) + kk */
int qpgpu_jvp(const qpgpu_problem_desc* d,
              const double* G, const double* CE, const double* CI,
              const double* x, const double* u, const int32_t* status,
              const double* tG, const double* tg0, const double* tCE, const double* tce0,
              const double* tCI, const double* tci0,
              double* tx, double* tu, double* tf, void* stream);

/* The same for bounds lo <= x <= hi, with u and tu in the layout of qpgpu_solve_batched_box_dual
 * (p + 2n doubles per QP; d->m must be 2 * d->n: anything else is QPGPU_ERR_INVALID_ARGUMENT); thi and
 * tlo are n doubles per QP in the layout of x.  col(t) is generated as in qpgpu_vjp_box; a bound's
 * column has no tangent: its h-step and its s-sum are skipped;  tb(t) = thi[k] for the upper bound
 * of k [thi given],  tb(t) = -tlo[k] (IEEE negation) for the lower bound of k [tlo given].  DEFINED
 * as, and bit-equal to, qpgpu_jvp on BoxProblems.to_dense() with tCI = NULL and tci0 = [thi; -tlo]. */
int qpgpu_jvp_box(const qpgpu_problem_desc* d,
                  const double* G, const double* CE,
                  const double* x, const double* u, const int32_t* status,
                  const double* tG, const double* tg0, const double* tCE, const double* tce0,
                  const double* thi, const double* tlo,
                  double* tx, double* tu, double* tf, void* stream);

/* Name of the kernel a qpgpu_jvp / qpgpu_jvp_box launch of this shape runs: a name containing "jvp",
 * and "lane" (one QP per lane) for n <= 8, "group" (one QP per 16, 32 or 64 lanes) for
 * 8 < n <= 64; "" for n > 64 or n <= 0. */
const char* qpgpu_kernel_name_jvp(int32_t n, int32_t p, int32_t m);

/* ---- K tangent directions on one factorisation ------------------------------------------------------
 * qpgpu_jvp_many is qpgpu_jvp along K = ntan directions of the data of every QP in one launch: the
 * Jacobian dx* / dg0 (n directions), a Gauss-Newton step, a sweep over a handful of parameters.  L, M,
 * S and R do not depend on the direction and are computed once per QP.  Everything said at
 * qpgpu_jvp / qpgpu_jvp_box holds unless stated here: device pointers, enqueue only, no allocation,
 * no workspace (a first call can be captured into a hipGraph); both layouts, natural alignment and
 * sub-ranges; the call writes the requested outputs of its own QPs and nothing else (no TILED64
 * padding slot, no input); d->flags must be 0; status may be NULL; a masked QP gets +0.0 and one
 * with q > n NaN in every requested output of all K directions; tangents of constraints outside W
 * never enter the arithmetic and may hold NaN.
 *
 * Layout of the K directions: a tangent (or output) of an array whose per-QP block has E elements is
 * an array whose per-QP block has K*E elements; direction k's element e is element k*E + e of that
 * block, direction-major, in either layout (TILED64: X + (b/64)*64*K*E + (k*E + e)*64 + b%64).  So a
 * QP-major tG is (batch, K, n, n), tx is K*n doubles per QP, tu K*(p + m) (K*(p + 2n) for box), and tf
 * is K doubles per QP, a per-QP block of E = K in the layout of x (with K = 1: tf[b] in both layouts).
 * Each tangent pointer may be NULL: a zero tangent for all K directions, whose [given] steps are
 * not executed.  Each output may be NULL; with all three NULL the call is QPGPU_SUCCESS and nothing is
 * launched.
 *
 * Definition: for every QP and every k < K, direction k's tx, tu and tf are bit for bit the
 * qpgpu_jvp (qpgpu_jvp_box) definition applied to the k-th slice of each given tangent: every sum is
 * the definition's, serial in its inner index, no FMA.  The results depend neither on K nor on how
 * the directions are chunked; K = 1 has the bits of qpgpu_jvp.
 *
 * Argument rules, decided before any array is read, in this order: qpgpu_jvp's argument rules as
 * they are; ntan < 1 is QPGPU_ERR_INVALID_ARGUMENT; then the shape rule, QPGPU_ERR_UNSUPPORTED_SHAPE for
 * n > 64 and when any of ntan*n*n, ntan*n*p, ntan*n*m, ntan*(p + m) reaches 2^31; batch = 0 is
 * QPGPU_SUCCESS after these. */
int qpgpu_jvp_many(const qpgpu_problem_desc* d, int32_t ntan,
                   const double* G, const double* CE, const double* CI,
                   const double* x, const double* u, const int32_t* status,
                   const double* tG, const double* tg0, const double* tCE, const double* tce0,
                   const double* tCI, const double* tci0,
                   double* tx, double* tu, double* tf, void* stream);
int qpgpu_jvp_box_many(const qpgpu_problem_desc* d, int32_t ntan,
                       const double* G, const double* CE,
                       const double* x, const double* u, const int32_t* status,
                       const double* tG, const double* tg0, const double* tCE, const double* tce0,
                       const double* thi, const double* tlo,
                       double* tx, double* tu, double* tf, void* stream);

/* Name of the kernel a qpgpu_jvp_many / qpgpu_jvp_box_many launch of this shape runs: a name containing
 * "jvp" and "many", and "lane" (one QP per lane) for n <= 8, "group" (one QP per 16, 32 or 64 lanes)
 * for 8 < n <= 64; "" for n > 64 or n <= 0. */
const char* qpgpu_kernel_name_jvp_many(int32_t n, int32_t p, int32_t m);

/* qpgpu_solve_batched with HOST pointers: copies the inputs to the device, solves, copies the outputs back
 * and synchronises.  This is what the ArrayHH drop-in (libquadprog_amd.so) calls for each
 * solve_quadprog(); it always runs the HIP kernel (there is no CPU path in the product).
 * Each host thread has its own device buffers, pinned staging buffer and stream.
 * G receives the Cholesky factor when QPGPU_FLAG_WRITE_FACTOR is set. */
int qpgpu_solve_batched_host(const qpgpu_problem_desc* d,
                             double* G, const double* g0,
                             const double* CE, const double* ce0,
                             const double* CI, const double* ci0,
                             double* x, double* f, int32_t* status, int32_t* iters);

/* Same as qpgpu_solve_batched_host, over several GPUs of one node from one host process: the
 * batch is split into `ndev` contiguous shards (shard k = QPs [k*B/ndev, (k+1)*B/ndev), rounded
 * to whole 64-QP tiles in the TILED64 layout), shard k is solved on device devices[k] by a
 * worker thread of its own (its own device buffers and stream, kept across calls), and each
 * shard's x, f, status, iters (and the factor in G with QPGPU_FLAG_WRITE_FACTOR) land in the
 * caller's buffers at the shard's offset — the gather of SURVEY §8(e) into host memory.  A device
 * may be listed more than once (its shards then run concurrently on separate streams).
 * Returns when every shard is done: the first failing shard's code, or QPGPU_SUCCESS.  Results
 * are identical to one qpgpu_solve_batched_host call on the whole batch.  ndev <= 64.
 * Replaces: the per-QP call at reference src/mgqp.cpp:708, batched over the node's GPUs. */
int qpgpu_solve_batched_multi(const qpgpu_problem_desc* d, int32_t ndev, const int32_t* devices,
                              double* G, const double* g0,
                              const double* CE, const double* ce0,
                              const double* CI, const double* ci0,
                              double* x, double* f, int32_t* status, int32_t* iters);

/* Convert one per-QP array of `elems` doubles per QP between the layouts on the device
 * (to_tiled = 1: QP-major -> TILED64, 0: back).  src and dst must not overlap; the TILED64
 * side holds ceil(batch/64) whole tiles (padding entries are left untouched / not read).
 * Enqueued on `stream`, no synchronisation. */
int qpgpu_relayout(int64_t batch, int32_t elems, const double* src, double* dst, int32_t to_tiled,
                   void* stream);

/* Largest n / m the specialised kernels accept (lane / subgroup / wave families); larger shapes
 * run on the generic kernel (QPGPU_FLAG_FORCE_GENERIC), whose only limits are n*n < 2^31 and
 * n*m < 2^31 and device memory for its workspace. */
int qpgpu_max_n(void);
int qpgpu_max_m(void);

/* Name of the kernel variant qpgpu_solve_batched would launch for this shape ("" if none). */
const char* qpgpu_kernel_name(int32_t n, int32_t p, int32_t m);
/* The same for a launch with these QPGPU_FLAG_* flags (QPGPU_FLAG_FAST selects the lane
 * kernel's fast build where it covers the shape); "" for a flag combination the solve entry
 * points reject (unknown bits, FAST with EXACT or WRITE_FACTOR, two forced families). */
const char* qpgpu_kernel_name_flags(int32_t n, int32_t p, int32_t m, uint32_t flags);

/* Human-readable text for the last QPGPU_ERR_HIP on this thread. */
const char* qpgpu_last_error(void);

/* Number of visible HIP devices (0 if none). */
int qpgpu_device_count(void);

int qpgpu_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* QPGPU_H */
