// qp_jvp.hip — qpgpu_jvp / qpgpu_jvp_box: the forward-mode sensitivities of a batch of QP solutions,
// (tx, tu, tf) for a tangent (tG, tg0, tCE, tce0, tCI, tci0) of the data (include/qpgpu.h).
//
// Per QP this is the backward step's linear algebra (qp_vjp.hip) with other right-hand sides, on the
// same working set W: L = chol(G), M = L^-1 A, S = M^T M, R = chol(S), then h = tA lam - tG x - tg0,
// k = -(tA^T x + tb), w = L^-1 h, dl = S^-1 (k - M^T w), tx = L^-T (w + M dl), and the envelope sum tf.
// The definition fixes every sum's order (serial in its inner index, products rounded before they
// are added: the library is built with -ffp-contract=off), so the parallelism is across QPs, rows
// and columns, in qp_vjp.hip's two mappings.  The I/O is the mirror image of the backward step's:
// large reads (G, tG, CE, tCE, the working columns of CI and tCI), small writes (n + p + m + 1).
//
//   lane kernel, n <= 8   one QP per lane, templated on n.  x, sG, L (packed lower triangle) and
//                         h -> w -> y -> tx live in registers, every loop over them unrolled; M, S / R
//                         (packed), k -> r -> dl and W live in a lane-private LDS slice (element e of
//                         lane l at e * 64 + l: conflict-free).  tG is streamed row by row into sG
//                         before G is loaded, so its n^2 values are never live together with L.
//                         Column t's loop turn loads col(t), tcol(t), lam(t) and tb(t) together:
//                         one memory latency per working column.  No lane talks to another, so a
//                         lane past the end of the batch, a masked one and one with q > n leave at
//                         once.  Every output is stored by its own lane: n + p + m + 1 doubles.
//   group kernel, n <= 64 one QP per group of S = 16, 32 or 64 lanes of a wavefront, one wavefront
//                         per workgroup.  L, M and S are S x (S + 1) tiles of the group's LDS slice.
//                         G and tG arrive with lane-consecutive addresses (tG in S's tile, free
//                         until S exists); lane i then owns row i of tG x.  Lane t owns column t:
//                         it loads tcol(t) into S's tile (CE's columns coalesce across the lanes)
//                         and forms k[t] on the way; lane i forms h[i] from row i of that tile, and
//                         h rides as the spare column of M through the forward substitutions.  The
//                         factorisations and the substitutions are qp_vjp.hip's.
//
// A QP masked by its status stores +0.0, one with more working columns than variables NaN, in every
// requested output.  The box entry generates the columns of CI = [-I, +I] as qp_vjp.hip does; a
// bound's column has no tangent, and tb is thi[k] or -tlo[k].  The substitutions, the group's
// factorisation and the launch are qp_dense.h's, shared with qp_vjp.hip.
#include "qp_dense.h"
#include "qp_jvp.h"

namespace qpk {
namespace jvp {

// fv into every requested output element of QP b, by the lanes first, first + step, ...
template <int T>
__device__ __forceinline__ void fill(const JvpArgs& g, int64_t b, double fv, int first, int step) {
  if (g.tx) {
    double* o = g.tx + qbase<T>(b, g.n);
    for (int e = first; e < g.n; e += step) o[(int64_t)e * T] = fv;
  }
  if (g.tu) {
    const int E = g.p + g.m;
    double* o = g.tu + qbase<T>(b, E);
    for (int e = first; e < E; e += step) o[(int64_t)e * T] = fv;
  }
  if (g.tf && first == 0) g.tf[b] = fv;
}

// ---- one QP per lane ----------------------------------------------------------------------------
template <int T, int N, bool BOX>
__global__ void __launch_bounds__(64) jvp_lane_kernel(JvpArgs g) {
  constexpr int NT = N * (N + 1) / 2;
  __shared__ double Ms[N * N * 64];
  __shared__ double Ss[NT * 64];
  __shared__ double Cs[N * 64];  // k, then r, then dl
  __shared__ int Ws[N * 64];
  const int lane = threadIdx.x;
  const int64_t b = g.qp0 + (int64_t)blockIdx.x * 64 + lane;
  if (b >= g.batch) return;
  const int p = g.p, m = g.m;
  if (g.status && g.status[b] != QPGPU_QP_OK) {
    fill<T>(g, b, 0.0, 0, 1);
    return;
  }
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
  if (q > N) {
    fill<T>(g, b, __builtin_nan(""), 0, 1);
    return;
  }
  const int nq = (int)q;

  double xv[N], sG[N], tg[N], h[N];
  {
    const double* xp = g.x + qbase<T>(b, N);
#pragma unroll
    for (int i = 0; i < N; i++) {
      xv[i] = xp[(int64_t)i * T];
      sG[i] = 0.0;
      tg[i] = 0.0;
      h[i] = 0.0;
    }
  }
  if (g.tg0) {
    const double* tp = g.tg0 + qbase<T>(b, N);
#pragma unroll
    for (int i = 0; i < N; i++) tg[i] = tp[(int64_t)i * T];
  }
  // sG = tG x, tG streamed row by row
  if (g.tG) {
    const double* tp = g.tG + qbase<T>(b, N * N);
#pragma unroll
    for (int i = 0; i < N; i++) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < N; j++) s = s + tp[(int64_t)(i * N + j) * T] * xv[j];
      sG[i] = s;
    }
  }
  // L = chol(G)
  double L[NT];
  {
    const double* Gp = g.G + qbase<T>(b, N * N);
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
      for (int k = 0; k <= i; k++) L[tri(i, k)] = Gp[(int64_t)(i * N + k) * T];
  }
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
  // position t: h += tcol(t) lam(t), k[t] = -(tcol(t)^T x + tb(t)), M[:, t] = fsub(L, col(t))
  const int64_t qCE = qbase<T>(b, N * p), qCI = BOX ? 0 : qbase<T>(b, N * m);
  double kk = 0.0;
  for (int t = 0; t < nq; t++) {
    double col[N], tc[N];
    const int j = t < p ? 0 : WS(t);
    const double lam = up[(int64_t)(t < p ? t : p + j) * T];
    bool has = false, hasb = false;
    double tb = 0.0;
    if (t < p) {
#pragma unroll
      for (int i = 0; i < N; i++) col[i] = g.CE[qCE + ((int64_t)i * p + t) * T];
      if (g.tCE) {
        has = true;
#pragma unroll
        for (int i = 0; i < N; i++) tc[i] = g.tCE[qCE + ((int64_t)i * p + t) * T];
      }
      if (g.tce0) {
        hasb = true;
        tb = g.tce0[qbase<T>(b, p) + (int64_t)t * T];
      }
    } else if constexpr (BOX) {
#pragma unroll
      for (int i = 0; i < N; i++) col[i] = box_entry(i, j, N);
      if (j < N) {
        if (g.thi) {
          hasb = true;
          tb = g.thi[qbase<T>(b, N) + (int64_t)j * T];
        }
      } else {
        if (g.tlo) {
          hasb = true;
          tb = -g.tlo[qbase<T>(b, N) + (int64_t)(j - N) * T];
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < N; i++) col[i] = g.CI[qCI + ((int64_t)i * m + j) * T];
      if (g.tCI) {
        has = true;
#pragma unroll
        for (int i = 0; i < N; i++) tc[i] = g.tCI[qCI + ((int64_t)i * m + j) * T];
      }
      if (g.tci0) {
        hasb = true;
        tb = g.tci0[qbase<T>(b, m) + (int64_t)j * T];
      }
    }
    double s = 0.0;
    if (has) {
#pragma unroll
      for (int i = 0; i < N; i++) {
        h[i] = h[i] + tc[i] * lam;
        s = s + tc[i] * xv[i];
      }
    }
    if (hasb) s = s + tb;
    const double kt = -s;
    CS(t) = kt;
    kk = kk + lam * kt;
    lane_fsub<N>(L, col);
#pragma unroll
    for (int i = 0; i < N; i++) MS(i, t) = col[i];
  }
  if (g.tG) {
#pragma unroll
    for (int i = 0; i < N; i++) h[i] = h[i] - sG[i];
  }
  if (g.tg0) {
#pragma unroll
    for (int i = 0; i < N; i++) h[i] = h[i] - tg[i];
  }
  lane_fsub<N>(L, h);  // (h is w)
  // S = M^T M (lower triangle), r = k - M^T w
  for (int s = 0; s < nq; s++) {
    for (int t = 0; t <= s; t++) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < N; i++) acc = acc + MS(i, s) * MS(i, t);
      SS(s, t) = acc;
    }
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) acc = acc + MS(i, s) * h[i];
    CS(s) = CS(s) - acc;
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
  lane_lds_solve(Ss, Cs, nq, lane);  // dl = bsub(R, fsub(R, r)), in place
  // y = w + M dl, tx = bsub(L, y)
  for (int t = 0; t < nq; t++) {
    const double dt = CS(t);
#pragma unroll
    for (int i = 0; i < N; i++) h[i] = h[i] + MS(i, t) * dt;
  }
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    double s = h[i];
#pragma unroll
    for (int k = i + 1; k < N; k++) s = s - L[tri(k, i)] * h[k];
    h[i] = s / L[tri(i, i)];
  }

  if (g.tx) {
    double* o = g.tx + qbase<T>(b, N);
#pragma unroll
    for (int i = 0; i < N; i++) o[(int64_t)i * T] = h[i];
  }
  if (g.tu) {
    double* o = g.tu + qbase<T>(b, p + m);
    for (int k = 0; k < p; k++) o[(int64_t)k * T] = CS(k);
    int t = p;
    for (int j = 0; j < m; j++) {
      const bool on = uip[(int64_t)j * T] != 0.0;
      o[(int64_t)(p + j) * T] = on ? CS(t) : 0.0;
      t += on;
    }
  }
  if (g.tf) {
    double qq = 0.0, ll = 0.0;
#pragma unroll
    for (int i = 0; i < N; i++) qq = qq + xv[i] * sG[i];
    if (g.tg0) {
#pragma unroll
      for (int i = 0; i < N; i++) ll = ll + tg[i] * xv[i];
    }
    g.tf[b] = ((0.5 * qq) + ll) + kk;
  }
}

// ---- one QP per group of S lanes -----------------------------------------------------------------
template <int T, int S, bool BOX>
__global__ void __launch_bounds__(64) jvp_group_kernel(JvpArgs g) {
  extern __shared__ double jvp_lds[];
  constexpr int LD = S + 1;
  const int lane = threadIdx.x, sub = lane / S, sl = lane % S, base = sub * S;
  const int64_t b = g.qp0 + (int64_t)blockIdx.x * (64 / S) + sub;
  if (b >= g.batch) return;  // whole groups; the others never wait for them
  double* Lm = jvp_lds + sub * group_doubles<S>();
  double* Mm = Lm + S * LD;
  double* Sm = Mm + S * LD;  // tG, then the tangent columns, then S
  double* xs = Sm + S * LD;
  double* lamv = xs + S;
  double* kv = lamv + S;  // k, until kk is formed
  double* dv = kv;        // then dl
  double* zv = kv + S;
  double* sgv = Sm + S;  // element i at sgv[i * LD]: the tile's spare column
  double* g0v = Lm + S;  // the same of L's tile
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
  if (masked || q > n) {  // a whole group: the wave's other groups never wait for it
    fill<T>(g, b, masked ? 0.0 : __builtin_nan(""), sl, S);
    return;
  }
  const int nq = (int)q;
  sg_sync();

  // G into L's tile and tG into S's, lane-consecutive addresses; x, tg0 and lam(t) into their vectors
  const int64_t qG = qbase<T>(b, n * n);
  for (int e = sl; e < n * n; e += S) Lm[(e / n) * LD + e % n] = g.G[qG + (int64_t)e * T];
  if (g.tG)
    for (int e = sl; e < n * n; e += S) Sm[(e / n) * LD + e % n] = g.tG[qG + (int64_t)e * T];
  if (sl < n) {
    xs[sl] = g.x[qbase<T>(b, n) + (int64_t)sl * T];
    g0v[sl * LD] = g.tg0 ? g.tg0[qbase<T>(b, n) + (int64_t)sl * T] : 0.0;
  }
  if (sl < nq) lamv[sl] = up[(int64_t)(sl < p ? sl : p + wi[sl]) * T];
  sg_sync();
  // lane i: sG[i] = sum_j tG[i][j] x[j]
  double sGi = 0.0;
  if (g.tG && sl < n)
    for (int j = 0; j < n; j++) sGi = sGi + Sm[sl * LD + j] * xs[j];
  if (sl < n) sgv[sl * LD] = sGi;
  sg_sync();
  group_chol<S>(Lm, n, n, sl, base);

  // lane t: tcol(t) into column t of S's tile, k[t] = -(tcol(t)^T x + tb(t))
  const int64_t qCE = qbase<T>(b, n * p), qCI = BOX ? 0 : qbase<T>(b, n * m);
  const bool hasCE = g.tCE != nullptr, hasCI = !BOX && g.tCI != nullptr;
  double kt = 0.0;
  if (sl < nq) {
    const int j = sl < p ? 0 : wi[sl];
    double s = 0.0;
    if (sl < p) {
      if (hasCE)
        for (int i = 0; i < n; i++) {
          const double v = g.tCE[qCE + ((int64_t)i * p + sl) * T];
          Sm[i * LD + sl] = v;
          s = s + v * xs[i];
        }
      if (g.tce0) s = s + g.tce0[qbase<T>(b, p) + (int64_t)sl * T];
    } else if constexpr (BOX) {
      if (j < n) {
        if (g.thi) s = s + g.thi[qbase<T>(b, n) + (int64_t)j * T];
      } else {
        if (g.tlo) s = s + -g.tlo[qbase<T>(b, n) + (int64_t)(j - n) * T];
      }
    } else {
      if (hasCI)
        for (int i = 0; i < n; i++) {
          const double v = g.tCI[qCI + ((int64_t)i * m + j) * T];
          Sm[i * LD + sl] = v;
          s = s + v * xs[i];
        }
      if (g.tci0) s = s + g.tci0[qbase<T>(b, m) + (int64_t)j * T];
    }
    kt = -s;
    kv[sl] = kt;
  }
  sg_sync();
  // lane i: h[i], into the column of M after the working ones
  if (sl < n) {
    double h = 0.0;
    if (hasCE)
      for (int t = 0; t < p; t++) h = h + Sm[sl * LD + t] * lamv[t];
    if (hasCI)
      for (int t = p; t < nq; t++) h = h + Sm[sl * LD + t] * lamv[t];
    if (g.tG) h = h - sGi;
    if (g.tg0) h = h - g0v[sl * LD];
    Mm[sl * LD + nq] = h;
  }
  // lane 0: kk = sum_t lam(t) k[t], before dl takes over k's vector
  double kk = 0.0;
  if (g.tf && sl == 0)
    for (int t = 0; t < nq; t++) kk = kk + lamv[t] * kv[t];
  sg_sync();

  // lane t: column t of M = fsub(L, col(t)) in place; column nq: w = fsub(L, h)
  const auto column = [&](int col) {
    const int j = (col >= p && col < nq) ? wi[col] : 0;
    for (int i = 0; i < n; i++) {
      double s;
      if (col >= nq)
        s = Mm[i * LD + col];
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

  // lane s: row s of S = M^T M and r_s = k_s - (M^T w)_s
  double rr = 0.0;
  if (sl < nq) {
    for (int t = 0; t <= sl; t++) {
      double acc = 0.0;
      for (int i = 0; i < n; i++) acc = acc + Mm[i * LD + sl] * Mm[i * LD + t];
      Sm[sl * LD + t] = acc;
    }
    double rs = 0.0;
    for (int i = 0; i < n; i++) rs = rs + Mm[i * LD + sl] * Mm[i * LD + nq];
    rr = kt - rs;
  }
  sg_sync();
  group_chol<S>(Sm, nq, n, sl, base);
  const double f = group_fsub<S>(Sm, nq, n, sl, rr, zv);
  const double dl = group_bsub<S>(Sm, nq, n, sl, f, zv);
  if (sl < nq) dv[sl] = dl;
  sg_sync();
  // lane i: y_i = w_i + sum_t M[i][t] dl[t], then tx = bsub(L, y)
  double y = 0.0;
  if (sl < n) {
    y = Mm[sl * LD + nq];
    for (int t = 0; t < nq; t++) y = y + Mm[sl * LD + t] * dv[t];
  }
  const double txi = group_bsub<S>(Lm, n, n, sl, y, zv);

  if (g.tx && sl < n) g.tx[qbase<T>(b, n) + (int64_t)sl * T] = txi;
  if (g.tu) {
    double* o = g.tu + qbase<T>(b, p + m);
    if (sl < p) o[(int64_t)sl * T] = dl;
    for (int j = sl; j < m; j += S)  // the inequalities outside W
      if (uip[(int64_t)j * T] == 0.0) o[(int64_t)(p + j) * T] = 0.0;
    if (sl >= p && sl < nq) o[(int64_t)(p + wi[sl]) * T] = dl;
  }
  if (g.tf && sl == 0) {
    double qq = 0.0, ll = 0.0;
    for (int i = 0; i < n; i++) qq = qq + xs[i] * sgv[i * LD];
    if (g.tg0)
      for (int i = 0; i < n; i++) ll = ll + g0v[i * LD] * xs[i];
    g.tf[b] = ((0.5 * qq) + ll) + kk;
  }
}

using JvpKernel = void (*)(JvpArgs);

template <int T, bool BOX>
static JvpKernel lane_kernel_of(int n) {
  switch (n) {
    case 1: return jvp_lane_kernel<T, 1, BOX>;
    case 2: return jvp_lane_kernel<T, 2, BOX>;
    case 3: return jvp_lane_kernel<T, 3, BOX>;
    case 4: return jvp_lane_kernel<T, 4, BOX>;
    case 5: return jvp_lane_kernel<T, 5, BOX>;
    case 6: return jvp_lane_kernel<T, 6, BOX>;
    case 7: return jvp_lane_kernel<T, 7, BOX>;
    default: return jvp_lane_kernel<T, 8, BOX>;
  }
}

template <int T, bool BOX>
static JvpKernel group_kernel_of(int n) {
  return n <= 16   ? jvp_group_kernel<T, 16, BOX>
         : n <= 32 ? jvp_group_kernel<T, 32, BOX>
                   : jvp_group_kernel<T, 64, BOX>;
}

static hipError_t launch(const JvpArgs* a, int tiled, hipStream_t stream) {
  const int n = a->n;
  if (n < 1 || n > 64) return hipErrorInvalidValue;
  const bool lane = n <= 8, box = a->box != 0;
  JvpKernel k;
  if (lane)
    k = tiled ? (box ? lane_kernel_of<64, true>(n) : lane_kernel_of<64, false>(n))
              : (box ? lane_kernel_of<1, true>(n) : lane_kernel_of<1, false>(n));
  else
    k = tiled ? (box ? group_kernel_of<64, true>(n) : group_kernel_of<64, false>(n))
              : (box ? group_kernel_of<1, true>(n) : group_kernel_of<1, false>(n));
  return launch_dense(k, a, stream);
}

}  // namespace jvp
}  // namespace qpk

extern "C" const char* qpk_jvp_name(int n) {
  static const char* const names[] = {"jvp_lane_n1", "jvp_lane_n2", "jvp_lane_n3",   "jvp_lane_n4",   "jvp_lane_n5",  "jvp_lane_n6",
                                      "jvp_lane_n7", "jvp_lane_n8", "jvp_group_s16", "jvp_group_s32", "jvp_group_s64"};
  return qpk::dense_kernel_name(names, n);
}

extern "C" hipError_t qpk_launch_jvp(const qpk::JvpArgs* a, int tiled, hipStream_t stream) {
  return qpk::jvp::launch(a, tiled, stream);
}
