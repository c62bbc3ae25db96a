// qp_vjp.hip — qpgpu_vjp / qpgpu_vjp_box: the gradients of a batch of QP solutions with respect to
// the problem data, given v = dl/dx (include/qpgpu.h).
//
// Per QP the backward step is dense linear algebra on the final working set W (the equalities, then
// the inequalities with a non-zero multiplier): L = chol(G), w = L^-1 v, M = L^-1 A, S = M^T M,
// R = chol(S), c = S^-1 M^T w, a = L^-T (w - M c), then the outer products that are the gradients.
// The definition fixes every sum's order (serial in its inner index, products rounded before they
// are added: the library is built with -ffp-contract=off), so the parallelism is across QPs, rows
// and columns, in two mappings:
//
//   lane kernel, n <= 8   one QP per lane, templated on n.  L (packed lower triangle), v, w, x, y
//                         and a live in registers, every loop over them unrolled; M (n x q), S / R
//                         (packed, q <= n) and c live in a lane-private LDS slice (element e of
//                         lane l at e * 64 + l: conflict-free), walked by run-time loops over q.
//                         No lane of the arithmetic talks to another.  TILED64 arrays are read
//                         and written coalesced.  QP-major inputs are read with a per-lane stride
//                         (a lane walks its own contiguous block, so every line fetched is used;
//                         staging G through LDS as well measured slower);
//                         QP-major outputs, the larger side, go through LDS pieces: the lanes put
//                         their blocks into a staging buffer (M's and S's slots, free by then) and
//                         the wave stores the 64 blocks' run with lane-consecutive addresses.
//   group kernel, n <= 64 one QP per group of S = 16, 32 or 64 lanes of a wavefront (the smallest
//                         that holds n), one wavefront per workgroup.  L, M and S are S x (S + 1)
//                         tiles of the group's LDS slice.  Lane i owns row i in the two
//                         factorisations (the pivot travels by a shuffle) and in y; lane t owns
//                         column t of M (its forward substitution, in place) and row t of S; the
//                         substitutions on single vectors are one lane's serial walk, as the
//                         definition's order makes them.  v rides along as column q of M.
//
// A QP masked by its status stores +0.0, one with more working columns than variables NaN, in
// every requested output.  A lane or group past the end of the batch reads nothing and stores
// nothing of its own (in the lane kernel's QP-major form it stays to help store the others'
// blocks).  The box entry generates the columns of CI = [-I, +I] (-1.0 among -0.0, +1.0
// among +0.0, as BoxProblems.to_dense() materialises them) and runs the same arithmetic: it reads
// no CI and writes no dCI.  The substitutions, the group's factorisation and the launch are
// qp_dense.h's, shared with qp_jvp.hip.
#include <type_traits>

#include "qp_dense.h"
#include "qp_vjp.h"

namespace qpk {

enum { kVjpOk = 0, kVjpZero = 1, kVjpNaN = 2, kVjpDead = 3 };  // (dead: a lane past the end of the batch)

// fv into every requested output element of QP b, by the lanes first, first + step, ...
template <int T>
__device__ __forceinline__ void vjp_fill(const VjpArgs& g, int64_t b, double fv, int first, int step) {
  const auto fill = [&](double* out, int E) {
    if (!out) return;
    double* o = out + qbase<T>(b, E);
    for (int e = first; e < E; e += step) o[(int64_t)e * T] = fv;
  };
  fill(g.dG, g.n * g.n);
  fill(g.dg0, g.n);
  fill(g.dCE, g.n * g.p);
  fill(g.dce0, g.p);
  fill(g.dCI, g.n * g.m);
  fill(g.dci0, g.m);
  fill(g.dhi, g.n);
  fill(g.dlo, g.n);
}

// The full form (qpgpu_vjp_full) is every kernel below built a second time with
// FULL = true, on VjpFullArgs: g.gu joins r before the q x q solve, g.gf turns c into ct and a into
// ah in the outputs.  Each is a branch on the pointer, uniform over the launch, and a NULL pointer
// leaves the other build's operations (no + 0.0 is added: it would turn a -0.0 into +0.0).  With
// FULL = false nothing of it is compiled.
template <bool FULL>
using VjpArgsOf = std::conditional_t<FULL, VjpFullArgs, VjpArgs>;

// a[i] as dG reads it: ah[i] = a[i] - hh * x[i], hh = 0.5 * gf
template <bool FULL>
__device__ __forceinline__ double vjp_ah(double a, double x, bool hasf, double hh) {
  if constexpr (FULL)
    if (hasf) return a - hh * x;
  return a;
}
// dg0[i] = -(a[i] - gf * x[i])
template <bool FULL>
__device__ __forceinline__ double vjp_dg0(double a, double x, bool hasf, double gf) {
  if constexpr (FULL)
    if (hasf) return -(a - gf * x);
  return -a;
}

// ---- one QP per lane ----------------------------------------------------------------------------
// The arithmetic of QP b in one lane, L holding the lower triangle of its G: a into w, x into xv, c
// into the lane's Cs slots (FULL with gf: ct = c + gfv * lam, once y is formed from c); the QP's
// mode (anything but kVjpOk: nothing was computed).  Ms, Ss, Cs, Ws: the wave's LDS arrays; Lam
// (FULL only): a slot per position for lam(t).  gl(t) and lam(t) are fetched with column t, so their
// latency is the columns': gl(t) waits in the Cs slot that r[t] takes over.
template <int T, int N, bool BOX, bool FULL>
__device__ __forceinline__ int lane_solve(const VjpArgsOf<FULL>& g, int64_t b, int lane, double* Ms, double* Ss, double* Cs,
                                          int* Ws, double (&L)[N * (N + 1) / 2], double (&w)[N], double (&xv)[N],
                                          double gfv, double* Lam) {
  const int p = g.p, m = g.m;
  if (g.status && g.status[b] != QPGPU_QP_OK) return kVjpZero;
  const double* up = (p + m > 0) ? g.u + qbase<T>(b, p + m) : g.x;  // (never read with p + m == 0)
  const double* uip = up + (int64_t)p * T;
  // the working list: positions [0, p) the equalities, then the inequalities with u != 0
  int64_t q = p;
  for (int i = 0; i < m; i++) {
    if (uip[(int64_t)i * T] != 0.0) {
      if (q < N) WS((int)q) = i;
      q++;
    }
  }
  if (q > N) return kVjpNaN;
  const int nq = (int)q;

  {
    const double* xp = g.x + qbase<T>(b, N);
    const double* vp = g.gx + qbase<T>(b, N);
#pragma unroll
    for (int i = 0; i < N; i++) {
      xv[i] = xp[(int64_t)i * T];
      w[i] = vp[(int64_t)i * T];
    }
  }
  // L = chol(G)
#pragma unroll
  for (int j = 0; j < N; j++) {
    double s = L[tri(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) s = s - L[tri(j, k)] * L[tri(j, k)];
    const double d = sqrt(s);
    L[tri(j, j)] = d;
#pragma unroll
    for (int i = j + 1; i < N; i++) {
      double r = L[tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) r = r - L[tri(i, k)] * L[tri(j, k)];
      L[tri(i, j)] = r / d;
    }
  }
  lane_fsub<N>(L, w);
  // M[:, t] = fsub(L, col(t))
  const int64_t qCE = qbase<T>(b, N * p), qCI = BOX ? 0 : qbase<T>(b, N * m);
  for (int t = 0; t < nq; t++) {
    double col[N];
    if constexpr (FULL) {
      const int64_t e = (int64_t)(t < p ? t : p + WS(t)) * T;  // position t's entry of u and of gu
      if (g.gu) CS(t) = g.gu[qbase<T>(b, p + m) + e];
      if (g.gf) Lam[t * 64 + lane] = up[e];
    }
    if (t < p) {
#pragma unroll
      for (int i = 0; i < N; i++) col[i] = g.CE[qCE + ((int64_t)i * p + t) * T];
    } else {
      const int j = WS(t);
#pragma unroll
      for (int i = 0; i < N; i++) {
        if constexpr (BOX)
          col[i] = box_entry(i, j, N);
        else
          col[i] = g.CI[qCI + ((int64_t)i * m + j) * T];
      }
    }
    lane_fsub<N>(L, col);
#pragma unroll
    for (int i = 0; i < N; i++) MS(i, t) = col[i];
  }
  // S = M^T M (lower triangle), r = M^T w
  for (int s = 0; s < nq; s++) {
    for (int t = 0; t <= s; t++) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < N; i++) acc = acc + MS(i, s) * MS(i, t);
      SS(s, t) = acc;
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) acc = acc + MS(i, s) * w[i];
    if constexpr (FULL) {
      if (g.gu) acc = acc + CS(s);  // gl(s), once, after the sum
    }
    CS(s) = acc;
  }
  // R = chol(S), in place
  for (int j = 0; j < nq; j++) {
    double s = SS(j, j);
    for (int k = 0; k < j; k++) s = s - SS(j, k) * SS(j, k);
    const double d = sqrt(s);
    SS(j, j) = d;
    for (int i = j + 1; i < nq; i++) {
      double r = SS(i, j);
      for (int k = 0; k < j; k++) r = r - SS(i, k) * SS(j, k);
      SS(i, j) = r / d;
    }
  }
  lane_lds_solve(Ss, Cs, nq, lane);  // c = bsub(R, fsub(R, r)), in place
  // y = w - M c, a = bsub(L, y)
  for (int t = 0; t < nq; t++) {
    const double ct = CS(t);
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = w[i] - MS(i, t) * ct;
  }
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    double s = w[i];
#pragma unroll
    for (int k = i + 1; k < N; k++) s = s - L[tri(k, i)] * w[k];
    w[i] = s / L[tri(i, i)];
  }
  if constexpr (FULL) {
    if (g.gf) {
      for (int t = 0; t < nq; t++) CS(t) = CS(t) + gfv * Lam[t * 64 + lane];
    }
  }
  return kVjpOk;  // (w is a)
}

template <int T, int N, bool BOX, bool FULL>
__global__ void __launch_bounds__(64) vjp_lane_kernel(VjpArgsOf<FULL> g) {
  constexpr int NT = N * (N + 1) / 2;
  __shared__ double Ls[(N * N + NT) * 64];  // M, then S; once a and c are known, the staging buffer of the QP-major stores
  __shared__ double Cs[N * 64];
  __shared__ int Ws[N * 64];
  double* const Ms = Ls;
  double* const Ss = Ls + N * N * 64;
  const int lane = threadIdx.x;
  const int64_t b0 = g.qp0 + (int64_t)blockIdx.x * 64, b = b0 + lane;
  const bool live = b < g.batch;
  if constexpr (T == 64)
    if (!live) return;
  const int p = g.p, m = g.m;
  double L[NT], w[N], xv[N];
#pragma unroll
  for (int i = 0; i < N; i++) w[i] = xv[i] = 0.0;
  if (live) {
    const double* Gp = g.G + qbase<T>(b, N * N);
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
      for (int k = 0; k <= i; k++) L[tri(i, k)] = Gp[(int64_t)(i * N + k) * T];
  }
  bool hasf = false;
  double gfv = 0.0, hh = 0.0;
  double* Lam = nullptr;
  if constexpr (FULL) {
    __shared__ double Lams[N * 64];
    Lam = Lams;
    hasf = g.gf != nullptr;
    if (hasf && live) {
      gfv = g.gf[b];
      hh = 0.5 * gfv;
    }
  }
  const int mode = live ? lane_solve<T, N, BOX, FULL>(g, b, lane, Ms, Ss, Cs, Ws, L, w, xv, gfv, Lam) : kVjpDead;
  const bool ok = mode == kVjpOk;
  const double fv = mode == kVjpNaN ? __builtin_nan("") : 0.0;
  // (neither is read unless ok)
  const double* up = (p + m > 0 && live) ? g.u + qbase<T>(b, p + m) : g.x;
  const double* uip = up + (int64_t)p * T;

  if constexpr (T == 64) {
    // TILED64: lane-consecutive QPs are address-consecutive, every store below is coalesced
    if (!ok) {
      vjp_fill<T>(g, b, fv, 0, 1);
      return;
    }
    if (g.dg0) {
      double* o = g.dg0 + qbase<T>(b, N);
#pragma unroll
      for (int i = 0; i < N; i++) o[(int64_t)i * T] = vjp_dg0<FULL>(w[i], xv[i], hasf, gfv);
    }
    if (g.dG) {
      double* o = g.dG + qbase<T>(b, N * N);
#pragma unroll
      for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++)
          o[(int64_t)(i * N + j) * T] = -0.5 * (vjp_ah<FULL>(w[i], xv[i], hasf, hh) * xv[j] +
                                                xv[i] * vjp_ah<FULL>(w[j], xv[j], hasf, hh));
    }
    if (g.dCE || g.dce0) {
      double* oc = g.dCE ? g.dCE + qbase<T>(b, N * p) : nullptr;
      double* o0 = g.dce0 ? g.dce0 + qbase<T>(b, p) : nullptr;
      for (int k = 0; k < p; k++) {
        const double uk = up[(int64_t)k * T], ck = CS(k);
        if (oc) {
#pragma unroll
          for (int i = 0; i < N; i++) oc[((int64_t)i * p + k) * T] = w[i] * uk - xv[i] * ck;
        }
        if (o0) o0[(int64_t)k * T] = -ck;
      }
    }
    if constexpr (BOX) {
      if (g.dhi || g.dlo) {
        double* oh = g.dhi ? g.dhi + qbase<T>(b, N) : nullptr;
        double* ol = g.dlo ? g.dlo + qbase<T>(b, N) : nullptr;
        int t = p;
        for (int j = 0; j < 2 * N; j++) {
          const bool on = uip[(int64_t)j * T] != 0.0;
          const double ct = on ? CS(t) : 0.0;
          if (j < N) {
            if (oh) oh[(int64_t)j * T] = on ? -ct : 0.0;
          } else {
            if (ol) ol[(int64_t)(j - N) * T] = ct;
          }
          t += on;
        }
      }
    } else {
      if (g.dCI || g.dci0) {
        double* oc = g.dCI ? g.dCI + qbase<T>(b, N * m) : nullptr;
        double* o0 = g.dci0 ? g.dci0 + qbase<T>(b, m) : nullptr;
        int t = p;
        for (int j = 0; j < m; j++) {
          const double uj = uip[(int64_t)j * T];
          const bool on = uj != 0.0;
          const double ct = on ? CS(t) : 0.0;
          if (oc) {
#pragma unroll
            for (int i = 0; i < N; i++) oc[((int64_t)i * m + j) * T] = on ? w[i] * uj - xv[i] * ct : 0.0;
          }
          if (o0) o0[(int64_t)j * T] = on ? -ct : 0.0;
          t += on;
        }
      }
    }
  } else {
    // QP-major: the wave's 64 blocks of an output are one contiguous run.  Each lane puts a piece
    // of its block into the staging buffer (element ee of lane l at ee * 65 + l: conflict-free
    // both ways), then the wave stores the pieces with lane-consecutive addresses.  Every lane of
    // the wave takes part, the ones past the end of the batch too (they store for the others).
    constexpr int CAP = (N * N + NT) * 64 / 65;  // elements of a piece
    static_assert(N * N <= CAP, "dG is one piece");
    double* const buf = Ls;
    const int nlive = g.batch - b0 < 64 ? (int)(g.batch - b0) : 64;
    // elements [e0, e0 + ec) of every live QP's block of E elements
    const auto flush = [&](double* out, int E, int e0, int ec) {
      sg_sync();
      double* o = out + b0 * (int64_t)E + e0;
      for (int idx = lane; idx < nlive * ec; idx += 64) {
        const int qp = idx / ec, ee = idx - qp * ec;
        o[(int64_t)qp * E + ee] = buf[ee * 65 + qp];
      }
      sg_sync();
    };
    // an R x C row-major output, element (i, j) = val(i, j, a[i], x[i]); val is called with j
    // ascending within a row, and a row is finished before the next begins
    const auto emit = [&](double* out, int R, int C, auto val) {
      if (!out || C == 0) return;
      const int jc_max = C < CAP ? C : CAP;    // whole rows while they fit, else pieces of one row
      const int ic_max = C < CAP ? CAP / C : 1;
      for (int i0 = 0; i0 < R; i0 += ic_max)
        for (int j0 = 0; j0 < C; j0 += jc_max) {
          const int ic = R - i0 < ic_max ? R - i0 : ic_max, jc = C - j0 < jc_max ? C - j0 : jc_max;
          for (int ii = 0; ii < ic; ii++) {
            const double ai = lsel(w, i0 + ii), xi = lsel(xv, i0 + ii);
            for (int jj = 0; jj < jc; jj++) buf[(ii * jc + jj) * 65 + lane] = val(i0 + ii, j0 + jj, ai, xi);
          }
          flush(out, R * C, i0 * C + j0, ic * jc);
        }
    };
    sg_sync();  // every lane is done with M and S
    if (g.dg0) {
#pragma unroll
      for (int i = 0; i < N; i++) buf[i * 65 + lane] = ok ? vjp_dg0<FULL>(w[i], xv[i], hasf, gfv) : fv;
      flush(g.dg0, N, 0, N);
    }
    if (g.dG) {
#pragma unroll
      for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++)
          buf[(i * N + j) * 65 + lane] = ok ? -0.5 * (vjp_ah<FULL>(w[i], xv[i], hasf, hh) * xv[j] +
                                                      xv[i] * vjp_ah<FULL>(w[j], xv[j], hasf, hh))
                                            : fv;
      flush(g.dG, N * N, 0, N * N);
    }
    emit(g.dCE, N, p, [&](int, int k, double ai, double xi) {
      if (!ok) return fv;
      return ai * up[k] - xi * CS(k);
    });
    emit(g.dce0, 1, p, [&](int, int k, double, double) {
      if (!ok) return fv;
      return -CS(k);
    });
    int t = p;  // the position in W of the next inequality with u != 0
    if constexpr (BOX) {
      int nup = 0;  // upper bounds in W
      if (ok)
        for (int j = 0; j < N; j++) nup += uip[j] != 0.0;
      emit(g.dhi, 1, N, [&](int, int j, double, double) {
        if (!ok) return fv;
        if (j == 0) t = p;
        const bool on = uip[j] != 0.0;
        const double ct = on ? CS(t) : 0.0;
        t += on;
        return on ? -ct : 0.0;
      });
      emit(g.dlo, 1, N, [&](int, int j, double, double) {
        if (!ok) return fv;
        if (j == 0) t = p + nup;
        const bool on = uip[N + j] != 0.0;
        const double ct = on ? CS(t) : 0.0;
        t += on;
        return ct;
      });
    } else {
      emit(g.dCI, N, m, [&](int, int j, double ai, double xi) {
        if (!ok) return fv;
        if (j == 0) t = p;
        const double uj = uip[j];
        const bool on = uj != 0.0;
        const double ct = on ? CS(t) : 0.0;
        t += on;
        return on ? ai * uj - xi * ct : 0.0;
      });
      emit(g.dci0, 1, m, [&](int, int j, double, double) {
        if (!ok) return fv;
        if (j == 0) t = p;
        const bool on = uip[j] != 0.0;
        const double ct = on ? CS(t) : 0.0;
        t += on;
        return on ? -ct : 0.0;
      });
    }
  }
}

// ---- one QP per group of S lanes -----------------------------------------------------------------
template <int T, int S, bool BOX, bool FULL>
__global__ void __launch_bounds__(64) vjp_group_kernel(VjpArgsOf<FULL> g) {
  extern __shared__ double vjp_lds[];
  constexpr int LD = S + 1;
  const int lane = threadIdx.x, sub = lane / S, sl = lane % S, base = sub * S;
  const int64_t b = g.qp0 + (int64_t)blockIdx.x * (64 / S) + sub;
  if (b >= g.batch) return;  // whole groups; the others never wait for them
  double* Lm = vjp_lds + sub * group_doubles<S>();
  double* Mm = Lm + S * LD;
  double* Sm = Mm + S * LD;
  double* xs = Sm + S * LD;
  double* av = xs + S;
  double* cv = av + S;
  double* zv = cv + S;
  int* wi = reinterpret_cast<int*>(zv + S);
  const int n = g.n, p = g.p, m = g.m;
  const bool masked = g.status && g.status[b] != QPGPU_QP_OK;
  const double* up = (p + m > 0) ? g.u + qbase<T>(b, p + m) : g.x;  // (never read with p + m == 0)
  const double* uip = up + (int64_t)p * T;

  // the working list: positions [0, p) the equalities, then the inequalities with u != 0
  const uint64_t gmask = S == 64 ? ~0ull : ((1ull << (S & 63)) - 1);
  int64_t q = p;
  for (int i0 = 0; i0 < m; i0 += S) {
    const int i = i0 + sl;
    const bool on = i < m && uip[(int64_t)i * T] != 0.0;
    const uint64_t mk = (__ballot(on) >> base) & gmask;
    const int64_t pos = q + __popcll(mk & ((1ull << sl) - 1));
    if (on && pos < S) wi[pos] = i;
    q += __popcll(mk);
  }
  const int mode = masked ? kVjpZero : (q > n ? kVjpNaN : kVjpOk);
  const int nq = q > n ? 0 : (int)q;  // (q > n: the arithmetic below runs without columns; nothing of it is stored)

  const int64_t qG = qbase<T>(b, n * n);
  for (int e = sl; e < n * n; e += S) Lm[(e / n) * LD + e % n] = g.G[qG + (int64_t)e * T];
  if (sl < n) xs[sl] = g.x[qbase<T>(b, n) + (int64_t)sl * T];
  sg_sync();
  group_chol<S>(Lm, n, n, sl, base);

  // lane t: column t of M = fsub(L, col(t)) in place; column nq: w = fsub(L, gx)
  const int64_t qCE = qbase<T>(b, n * p), qCI = BOX ? 0 : qbase<T>(b, n * m);
  const double* vp = g.gx + qbase<T>(b, n);
  const auto column = [&](int col) {
    const int j = (col >= p && col < nq) ? wi[col] : 0;
    for (int i = 0; i < n; i++) {
      double s;
      if (col >= nq)
        s = vp[(int64_t)i * T];
      else if (col < p)
        s = g.CE[qCE + ((int64_t)i * p + col) * T];
      else if constexpr (BOX)
        s = box_entry(i, j, n);
      else
        s = g.CI[qCI + ((int64_t)i * m + j) * T];
      for (int k = 0; k < i; k++) s = s - Lm[i * LD + k] * Mm[k * LD + col];
      Mm[i * LD + col] = s / Lm[i * LD + i];
    }
  };
  if (sl <= nq) column(sl);
  sg_sync();
  if (nq == S && sl == 0) column(S);  // (the tile's spare column)
  sg_sync();

  // lane s: row s of S = M^T M and r_s = (M^T w)_s
  double rr = 0.0;
  if (sl < nq) {
    for (int t = 0; t <= sl; t++) {
      double acc = 0.0;
      for (int i = 0; i < n; i++) acc = acc + Mm[i * LD + sl] * Mm[i * LD + t];
      Sm[sl * LD + t] = acc;
    }
    for (int i = 0; i < n; i++) rr = rr + Mm[i * LD + sl] * Mm[i * LD + nq];
    if constexpr (FULL) {
      if (g.gu) rr = rr + g.gu[qbase<T>(b, p + m) + (int64_t)(sl < p ? sl : p + wi[sl]) * T];  // gl(s)
    }
  }
  sg_sync();
  group_chol<S>(Sm, nq, n, sl, base);
  const double f = group_fsub<S>(Sm, nq, n, sl, rr, zv);
  const double c = group_bsub<S>(Sm, nq, n, sl, f, zv);
  if (sl < nq) cv[sl] = c;
  sg_sync();
  // lane i: y_i = w_i - sum_t M[i][t] c[t], then a = bsub(L, y)
  double y = 0.0;
  if (sl < n) {
    y = Mm[sl * LD + nq];
    for (int t = 0; t < nq; t++) y = y - Mm[sl * LD + t] * cv[t];
  }
  const double ai = group_bsub<S>(Lm, n, n, sl, y, zv);
  if (sl < n) av[sl] = ai;
  bool hasf = false;
  double gfv = 0.0, hh = 0.0;
  if constexpr (FULL) {
    hasf = g.gf != nullptr;
    if (hasf) {
      gfv = g.gf[b];
      hh = 0.5 * gfv;
      // ct = c + gf * lam for the outputs (y, formed from c, is behind the barriers of bsub)
      if (sl < nq) cv[sl] = c + gfv * (sl < p ? up[(int64_t)sl * T] : uip[(int64_t)wi[sl] * T]);
    }
  }
  sg_sync();

  if (mode != kVjpOk) {
    vjp_fill<T>(g, b, mode == kVjpZero ? 0.0 : __builtin_nan(""), sl, S);
    return;
  }
  if (g.dg0 && sl < n) g.dg0[qbase<T>(b, n) + (int64_t)sl * T] = vjp_dg0<FULL>(ai, xs[sl], hasf, gfv);
  if (g.dG) {
    double* o = g.dG + qG;
    for (int e = sl; e < n * n; e += S) {
      const int i = e / n, j = e % n;
      o[(int64_t)e * T] = -0.5 * (vjp_ah<FULL>(av[i], xs[i], hasf, hh) * xs[j] +
                                  xs[i] * vjp_ah<FULL>(av[j], xs[j], hasf, hh));
    }
  }
  if (g.dCE) {
    double* o = g.dCE + qCE;
    for (int e = sl; e < n * p; e += S) {
      const int i = e / p, k = e % p;
      o[(int64_t)e * T] = av[i] * up[(int64_t)k * T] - xs[i] * cv[k];
    }
  }
  if (g.dce0 && sl < p) g.dce0[qbase<T>(b, p) + (int64_t)sl * T] = -cv[sl];
  if constexpr (BOX) {
    double* oh = g.dhi ? g.dhi + qbase<T>(b, n) : nullptr;
    double* ol = g.dlo ? g.dlo + qbase<T>(b, n) : nullptr;
    if (sl < n) {  // the bounds outside W
      if (oh && uip[(int64_t)sl * T] == 0.0) oh[(int64_t)sl * T] = 0.0;
      if (ol && uip[(int64_t)(n + sl) * T] == 0.0) ol[(int64_t)sl * T] = 0.0;
    }
    if (sl >= p && sl < nq) {
      const int j = wi[sl];
      if (j < n) {
        if (oh) oh[(int64_t)j * T] = -cv[sl];
      } else {
        if (ol) ol[(int64_t)(j - n) * T] = cv[sl];
      }
    }
  } else {
    if (g.dCI) {
      double* o = g.dCI + qCI;
      for (int e = sl; e < n * m; e += S)  // the columns outside W
        if (uip[(int64_t)(e % m) * T] == 0.0) o[(int64_t)e * T] = 0.0;
      for (int t = p; t < nq; t++) {
        const int j = wi[t];
        if (sl < n) o[((int64_t)sl * m + j) * T] = ai * uip[(int64_t)j * T] - xs[sl] * cv[t];
      }
    }
    if (g.dci0) {
      double* o = g.dci0 + qbase<T>(b, m);
      for (int j = sl; j < m; j += S)
        if (uip[(int64_t)j * T] == 0.0) o[(int64_t)j * T] = 0.0;
      if (sl >= p && sl < nq) o[(int64_t)wi[sl] * T] = -cv[sl];
    }
  }
}

template <bool FULL>
using VjpKernel = void (*)(VjpArgsOf<FULL>);

template <int T, bool BOX, bool FULL>
static VjpKernel<FULL> lane_kernel_of(int n) {
  switch (n) {
    case 1: return vjp_lane_kernel<T, 1, BOX, FULL>;
    case 2: return vjp_lane_kernel<T, 2, BOX, FULL>;
    case 3: return vjp_lane_kernel<T, 3, BOX, FULL>;
    case 4: return vjp_lane_kernel<T, 4, BOX, FULL>;
    case 5: return vjp_lane_kernel<T, 5, BOX, FULL>;
    case 6: return vjp_lane_kernel<T, 6, BOX, FULL>;
    case 7: return vjp_lane_kernel<T, 7, BOX, FULL>;
    default: return vjp_lane_kernel<T, 8, BOX, FULL>;
  }
}

template <int T, bool BOX, bool FULL>
static VjpKernel<FULL> group_kernel_of(int n) {
  return n <= 16   ? vjp_group_kernel<T, 16, BOX, FULL>
         : n <= 32 ? vjp_group_kernel<T, 32, BOX, FULL>
                   : vjp_group_kernel<T, 64, BOX, FULL>;
}

template <bool FULL>
static hipError_t launch_vjp(const VjpArgsOf<FULL>* a, int tiled, hipStream_t stream) {
  const int n = a->n;
  if (n < 1 || n > 64) return hipErrorInvalidValue;
  const bool lane = n <= 8, box = a->box != 0;
  VjpKernel<FULL> k;
  if (lane)
    k = tiled ? (box ? lane_kernel_of<64, true, FULL>(n) : lane_kernel_of<64, false, FULL>(n))
              : (box ? lane_kernel_of<1, true, FULL>(n) : lane_kernel_of<1, false, FULL>(n));
  else
    k = tiled ? (box ? group_kernel_of<64, true, FULL>(n) : group_kernel_of<64, false, FULL>(n))
              : (box ? group_kernel_of<1, true, FULL>(n) : group_kernel_of<1, false, FULL>(n));
  return launch_dense(k, a, stream);
}

}  // namespace qpk

extern "C" const char* qpk_vjp_name(int n) {
  static const char* const names[] = {"vjp_lane_n1", "vjp_lane_n2", "vjp_lane_n3",   "vjp_lane_n4",   "vjp_lane_n5",  "vjp_lane_n6",
                                      "vjp_lane_n7", "vjp_lane_n8", "vjp_group_s16", "vjp_group_s32", "vjp_group_s64"};
  return qpk::dense_kernel_name(names, n);
}

extern "C" const char* qpk_vjp_full_name(int n) {
  static const char* const names[] = {"vjp_full_lane_n1",   "vjp_full_lane_n2",   "vjp_full_lane_n3",  "vjp_full_lane_n4",
                                      "vjp_full_lane_n5",   "vjp_full_lane_n6",   "vjp_full_lane_n7",  "vjp_full_lane_n8",
                                      "vjp_full_group_s16", "vjp_full_group_s32", "vjp_full_group_s64"};
  return qpk::dense_kernel_name(names, n);
}

extern "C" hipError_t qpk_launch_vjp(const qpk::VjpArgs* a, int tiled, hipStream_t stream) {
  return qpk::launch_vjp<false>(a, tiled, stream);
}

extern "C" hipError_t qpk_launch_vjp_full(const qpk::VjpFullArgs* a, int tiled, hipStream_t stream) {
  return qpk::launch_vjp<true>(a, tiled, stream);
}
