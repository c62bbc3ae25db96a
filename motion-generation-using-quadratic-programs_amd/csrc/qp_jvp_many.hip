// qp_jvp_many.hip — qpgpu_jvp_many / qpgpu_jvp_box_many: the forward-mode sensitivities of a batch of QP
// solutions along K = ntan directions per QP in one launch (include/qpgpu.h).
//
// Direction k of a QP is qpgpu_jvp's definition on the k-th slice of every tangent, bit for bit.
// What does not depend on the tangent is computed once per QP: the working set W, L = chol(G),
// M = L^-1 A, S = M^T M, R = chol(S).  Per direction remain h = tA lam - tG x - tg0, k = -(tA^T x + tb),
// w = L^-1 h, dl = S^-1 (k - M^T w), tx = L^-T (w + M dl) and the envelope sum tf: every sum in
// qp_jvp.hip's order (serial in its inner index, no contraction), so neither K nor the chunking of
// the directions reaches a bit.  A tangent or an output of E elements per QP has K * E here,
// direction-major: direction k's element e is element k * E + e of the QP's block, in both layouts.
//
//   lane kernel, n <= 8   one QP per lane, templated on n.  Once: W, lam, M, S / R in the lane's LDS
//                         slice, x and L in registers.  Then a loop over the directions: tG_k streamed
//                         row by row, only tcol_k(t) and tb_k(t) loaded per working column, h -> w -> y ->
//                         tx in registers, k -> r -> dl in the slice.
//   group kernel, n <= 64 one QP per group of S = 16, 32 or 64 lanes.  L, M and R are tiles as in
//                         qp_jvp.hip and stay for all directions, so the tangents have a staging
//                         tile of their own, and the directions advance in chunks of Kc: the group
//                         prepares h_c and k_c of each direction of the chunk lane-parallel (lane i
//                         owns row i, lane t column t) into an n x Kc and an nq x Kc block, then lane
//                         c owns direction c and runs its four triangular solves alone, Kc
//                         directions side by side; the sums between the solves (r, y) are shared
//                         by all lanes.  The kernel is bound by the latency of its loads, so
//                         every loop over global memory issues up to 16 loads before it waits,
//                         and the serial sums over LDS 8 (seq_fma_up / seq_fms_up, qp_common.h).
//
// A QP masked by its status stores +0.0, one with more working columns than variables NaN, in every
// requested output of all K directions.
#include "qp_dense.h"
#include "qp_jvp_many.h"

namespace qpk {
namespace jvp_many {

// offset of element 0 of QP b's block of E elements (E up to 2^31 - 1: K blocks of a tangent)
template <int T>
__device__ __forceinline__ int64_t qoff(int64_t b, int64_t E) {
  if constexpr (T == 1)
    return b * E;
  else
    return (b >> 6) * (64 * E) + (b & 63);
}

// fv into every requested output element of all K directions of QP b, by the lanes first, first + step, ...
template <int T>
__device__ __forceinline__ void fill(const JvpArgs& g, int K, int64_t b, double fv, int first, int step) {
  if (g.tx) {
    const int64_t E = (int64_t)K * g.n;
    double* o = g.tx + qoff<T>(b, E);
    for (int64_t e = first; e < E; e += step) o[e * T] = fv;
  }
  if (g.tu) {
    const int64_t E = (int64_t)K * (g.p + g.m);
    double* o = g.tu + qoff<T>(b, E);
    for (int64_t e = first; e < E; e += step) o[e * T] = fv;
  }
  if (g.tf) {
    double* o = g.tf + qoff<T>(b, K);
    for (int64_t e = first; e < K; e += step) o[e * T] = fv;
  }
}

// ---- one QP per lane ----------------------------------------------------------------------------
#define LS(t) Ls[(t) * 64 + lane]

template <int T, int N, bool BOX>
__global__ void __launch_bounds__(64) jvp_many_lane_kernel(JvpManyArgs ga) {
  constexpr int NT = N * (N + 1) / 2;
  __shared__ double Ms[N * N * 64];
  __shared__ double Ss[NT * 64];
  __shared__ double Cs[N * 64];  // per direction: k, then r, then dl
  __shared__ double Ls[N * 64];  // lam(t)
  __shared__ int Ws[N * 64];
  const JvpArgs& g = ga.a;
  const int K = ga.ntan;
  const int lane = threadIdx.x;
  const int64_t b = g.qp0 + (int64_t)blockIdx.x * 64 + lane;
  if (b >= g.batch) return;
  const int p = g.p, m = g.m;
  if (g.status && g.status[b] != QPGPU_QP_OK) {
    fill<T>(g, K, b, 0.0, 0, 1);
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
    fill<T>(g, K, b, __builtin_nan(""), 0, 1);
    return;
  }
  const int nq = (int)q;
  const int64_t EU = (int64_t)p + m;
  // tu of the inequalities outside W: +0.0 in every direction
  if (g.tu) {
    double* o = g.tu + qoff<T>(b, K * EU);
    for (int j = 0; j < m; j++)
      if (uip[(int64_t)j * T] == 0.0)
        for (int k = 0; k < K; k++) o[(k * EU + p + j) * T] = 0.0;
  }

  double xv[N];
  {
    const double* xp = g.x + qbase<T>(b, N);
#pragma unroll
    for (int i = 0; i < N; i++) xv[i] = xp[(int64_t)i * T];
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
  // position t: lam(t), M[:, t] = fsub(L, col(t))
  const int64_t qCE = qbase<T>(b, N * p), qCI = BOX ? 0 : qbase<T>(b, N * m);
  for (int t = 0; t < nq; t++) {
    double col[N];
    const int j = t < p ? 0 : WS(t);
    LS(t) = up[(int64_t)(t < p ? t : p + j) * T];
    if (t < p) {
#pragma unroll
      for (int i = 0; i < N; i++) col[i] = g.CE[qCE + ((int64_t)i * p + t) * T];
    } else if constexpr (BOX) {
#pragma unroll
      for (int i = 0; i < N; i++) col[i] = box_entry(i, j, N);
    } else {
#pragma unroll
      for (int i = 0; i < N; i++) col[i] = g.CI[qCI + ((int64_t)i * m + j) * T];
    }
    lane_fsub<N>(L, col);
#pragma unroll
    for (int i = 0; i < N; i++) MS(i, t) = col[i];
  }
  // S = M^T M (lower triangle)
  for (int s = 0; s < nq; s++)
    for (int t = 0; t <= s; t++) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < N; i++) acc = acc + MS(i, s) * MS(i, t);
      SS(s, t) = acc;
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

  // the K directions' blocks of this QP
  const double* tGp = g.tG ? g.tG + qoff<T>(b, (int64_t)K * N * N) : nullptr;
  const double* tg0p = g.tg0 ? g.tg0 + qoff<T>(b, (int64_t)K * N) : nullptr;
  const double* tCEp = g.tCE ? g.tCE + qoff<T>(b, (int64_t)K * N * p) : nullptr;
  const double* tce0p = g.tce0 ? g.tce0 + qoff<T>(b, (int64_t)K * p) : nullptr;
  const double* tCIp = (!BOX && g.tCI) ? g.tCI + qoff<T>(b, (int64_t)K * N * m) : nullptr;
  const double* tci0p = (!BOX && g.tci0) ? g.tci0 + qoff<T>(b, (int64_t)K * m) : nullptr;
  const double* thip = (BOX && g.thi) ? g.thi + qoff<T>(b, (int64_t)K * N) : nullptr;
  const double* tlop = (BOX && g.tlo) ? g.tlo + qoff<T>(b, (int64_t)K * N) : nullptr;
  double* txp = g.tx ? g.tx + qoff<T>(b, (int64_t)K * N) : nullptr;
  double* tup = g.tu ? g.tu + qoff<T>(b, K * EU) : nullptr;
  double* tfp = g.tf ? g.tf + qoff<T>(b, K) : nullptr;

  for (int kd = 0; kd < K; kd++) {
    double sG[N], tg[N], h[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
      sG[i] = 0.0;
      tg[i] = 0.0;
      h[i] = 0.0;
    }
    if (tg0p) {
      const double* tp = tg0p + (int64_t)kd * N * T;
#pragma unroll
      for (int i = 0; i < N; i++) tg[i] = tp[(int64_t)i * T];
    }
    // sG = tG x, tG streamed row by row
    if (tGp) {
      const double* tp = tGp + (int64_t)kd * (N * N) * T;
#pragma unroll
      for (int i = 0; i < N; i++) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < N; j++) s = s + tp[(int64_t)(i * N + j) * T] * xv[j];
        sG[i] = s;
      }
    }
    // position t: h += tcol(t) lam(t), k[t] = -(tcol(t)^T x + tb(t))
    double kk = 0.0;
    for (int t = 0; t < nq; t++) {
      double tc[N];
      const int j = t < p ? 0 : WS(t);
      const double lam = LS(t);
      bool has = false, hasb = false;
      double tb = 0.0;
      if (t < p) {
        if (tCEp) {
          has = true;
          const double* tp = tCEp + (int64_t)kd * (N * p) * T;
#pragma unroll
          for (int i = 0; i < N; i++) tc[i] = tp[((int64_t)i * p + t) * T];
        }
        if (tce0p) {
          hasb = true;
          tb = tce0p[((int64_t)kd * p + t) * T];
        }
      } else if constexpr (BOX) {
        if (j < N) {
          if (thip) {
            hasb = true;
            tb = thip[((int64_t)kd * N + j) * T];
          }
        } else {
          if (tlop) {
            hasb = true;
            tb = -tlop[((int64_t)kd * N + (j - N)) * T];
          }
        }
      } else {
        if (tCIp) {
          has = true;
          const double* tp = tCIp + (int64_t)kd * N * m * T;
#pragma unroll
          for (int i = 0; i < N; i++) tc[i] = tp[((int64_t)i * m + j) * T];
        }
        if (tci0p) {
          hasb = true;
          tb = tci0p[((int64_t)kd * m + j) * T];
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
    }
    if (tGp) {
#pragma unroll
      for (int i = 0; i < N; i++) h[i] = h[i] - sG[i];
    }
    if (tg0p) {
#pragma unroll
      for (int i = 0; i < N; i++) h[i] = h[i] - tg[i];
    }
    lane_fsub<N>(L, h);  // (h is w)
    // r = k - M^T w
    for (int s = 0; s < nq; s++) {
      double acc = 0.0;
#pragma unroll
      for (int i = 0; i < N; i++) acc = acc + MS(i, s) * h[i];
      CS(s) = CS(s) - acc;
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

    if (txp) {
      double* o = txp + (int64_t)kd * N * T;
#pragma unroll
      for (int i = 0; i < N; i++) o[(int64_t)i * T] = h[i];
    }
    if (tup) {
      double* o = tup + kd * EU * T;
      for (int t = 0; t < nq; t++) o[(int64_t)(t < p ? t : p + WS(t)) * T] = CS(t);
    }
    if (tfp) {
      double qq = 0.0, ll = 0.0;
#pragma unroll
      for (int i = 0; i < N; i++) qq = qq + xv[i] * sG[i];
      if (tg0p) {
#pragma unroll
        for (int i = 0; i < N; i++) ll = ll + tg[i] * xv[i];
      }
      tfp[(int64_t)kd * T] = ((0.5 * qq) + ll) + kk;
    }
  }
}

// ---- one QP per group of S lanes -----------------------------------------------------------------
// Directions per chunk: the width of the h and k blocks.  The four tiles and the blocks decide how
// many workgroups a CU holds: S = 16 three, S = 32 two, S = 64 one.
template <int S>
constexpr int chunk() {
  return S == 32 ? 8 : 16;
}

// doubles of LDS per group: four S x (S + 1) tiles (L, M, S / R, the staging tile), the h and k
// blocks (S x (Kc + 1) each), four vectors, the working list (S ints)
template <int S>
constexpr int group_doubles_many() {
  return 4 * S * (S + 1) + 2 * S * (chunk<S>() + 1) + 4 * S + S / 2;
}

// Loads per lane issued together before their first use: the kernel is bound by the latency of its
// global loads (two or three wavefronts per CU), so a loop that waits for each load costs its trip
// count in memory latencies, one that issues kLoads of them at once costs one per kLoads.
constexpr int kLoads = 16;

// n x n doubles at src (element e at e * T) into a tile, lane-consecutive addresses
template <int T, int S>
__device__ __forceinline__ void stage_tile(double* tile, const double* src, int n, int sl) {
  constexpr int LD = S + 1;
  const int nn = n * n;
  for (int e0 = sl; e0 < nn; e0 += S * kLoads) {
    double v[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; u++) {
      const int e = e0 + u * S;
      v[u] = e < nn ? src[(int64_t)e * T] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kLoads; u++) {
      const int e = e0 + u * S;
      if (e < nn) tile[(e / n) * LD + e % n] = v[u];
    }
  }
}

// s + sum_i src[i * stride] * xs[i], i ascending, each value also stored at dst[i * LD]
template <int LD>
__device__ __forceinline__ double column_in(double s, const double* src, int64_t stride, int n, double* dst,
                                            const double* xs) {
  for (int i0 = 0; i0 < n; i0 += kLoads) {
    double v[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; u++) v[u] = i0 + u < n ? src[(i0 + u) * stride] : 0.0;
#pragma unroll
    for (int u = 0; u < kLoads; u++)
      if (i0 + u < n) {
        dst[(i0 + u) * LD] = v[u];
        s = s + v[u] * xs[i0 + u];
      }
  }
  return s;
}

template <int T, int S, bool BOX>
__global__ void __launch_bounds__(64) jvp_many_group_kernel(JvpManyArgs ga) {
  extern __shared__ double jvp_many_lds[];
  constexpr int LD = S + 1, KC = chunk<S>(), KL = KC + 1;
  const JvpArgs& g = ga.a;
  const int K = ga.ntan;
  const int lane = threadIdx.x, sub = lane / S, sl = lane % S, base = sub * S;
  const int64_t b = g.qp0 + (int64_t)blockIdx.x * (64 / S) + sub;
  if (b >= g.batch) return;  // whole groups; the others never wait for them
  double* Lm = jvp_many_lds + sub * group_doubles_many<S>();
  double* Mm = Lm + S * LD;
  double* Sm = Mm + S * LD;  // S, then R
  double* Tm = Sm + S * LD;  // a direction's tG, then its tangent columns
  double* HB = Tm + S * LD;  // column c: h -> w -> y -> tx of the chunk's direction c
  double* KB = HB + S * KL;  // column c: k -> r -> dl
  double* xs = KB + S * KL;
  double* lamv = xs + S;
  double* sgv = lamv + S;  // a direction's tG x
  double* g0v = sgv + S;   // a direction's tg0
  int* wi = reinterpret_cast<int*>(g0v + S);
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
    fill<T>(g, K, b, masked ? 0.0 : __builtin_nan(""), sl, S);
    return;
  }
  const int nq = (int)q;
  const int64_t EU = (int64_t)p + m;
  // tu of the inequalities outside W: +0.0 in every direction
  if (g.tu) {
    double* o = g.tu + qoff<T>(b, K * EU);
    for (int j = sl; j < m; j += S)
      if (uip[(int64_t)j * T] == 0.0)
        for (int k = 0; k < K; k++) o[(k * EU + p + j) * T] = 0.0;
  }
  sg_sync();

  // G into L's tile, lane-consecutive addresses; x and lam(t) into their vectors
  const int64_t qG = qbase<T>(b, n * n);
  stage_tile<T, S>(Lm, g.G + qG, n, sl);
  if (sl < n) xs[sl] = g.x[qbase<T>(b, n) + (int64_t)sl * T];
  if (sl < nq) lamv[sl] = up[(int64_t)(sl < p ? sl : p + wi[sl]) * T];
  sg_sync();
  group_chol<S>(Lm, n, n, sl, base);

  // lane t: column t of M = fsub(L, col(t)) in place
  const int64_t qCE = qbase<T>(b, n * p), qCI = BOX ? 0 : qbase<T>(b, n * m);
  if (sl < nq) {
    const int j = sl >= p ? wi[sl] : 0;
    const bool eq = sl < p;
    const double* cp = eq ? g.CE + qCE + (int64_t)sl * T : (BOX ? g.x : g.CI + qCI + (int64_t)j * T);
    const int64_t stride = (int64_t)(eq ? p : m) * T;
    for (int i0 = 0; i0 < n; i0 += kLoads) {
      double v[kLoads];
#pragma unroll
      for (int u = 0; u < kLoads; u++) {
        const int i = i0 + u;
        if (BOX && !eq)
          v[u] = box_entry(i, j, n);
        else
          v[u] = i < n ? cp[i * stride] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kLoads; u++) {
        const int i = i0 + u;
        if (i < n) {
          const double s = seq_fms_up<8>(v[u], 0, i, [&](int k) { return Lm[i * LD + k]; },
                                         [&](int k) { return Mm[k * LD + sl]; });
          Mm[i * LD + sl] = s / Lm[i * LD + i];
        }
      }
    }
  }
  sg_sync();
  // lane s: row s of S = M^T M
  if (sl < nq) {
    for (int t = 0; t <= sl; t++) {
      Sm[sl * LD + t] = seq_fma_up<8>(0.0, 0, n, [&](int i) { return Mm[i * LD + sl]; },
                                      [&](int i) { return Mm[i * LD + t]; });
    }
  }
  sg_sync();
  group_chol<S>(Sm, nq, n, sl, base);

  // the K directions' blocks of this QP
  const int nn = n * n;
  const bool hasCE = g.tCE != nullptr, hasCI = !BOX && g.tCI != nullptr;
  const double* tGp = g.tG ? g.tG + qoff<T>(b, (int64_t)K * nn) : nullptr;
  const double* tg0p = g.tg0 ? g.tg0 + qoff<T>(b, (int64_t)K * n) : nullptr;
  const double* tCEp = hasCE ? g.tCE + qoff<T>(b, (int64_t)K * n * p) : nullptr;
  const double* tce0p = g.tce0 ? g.tce0 + qoff<T>(b, (int64_t)K * p) : nullptr;
  const double* tCIp = hasCI ? g.tCI + qoff<T>(b, (int64_t)K * n * m) : nullptr;
  const double* tci0p = (!BOX && g.tci0) ? g.tci0 + qoff<T>(b, (int64_t)K * m) : nullptr;
  const double* thip = (BOX && g.thi) ? g.thi + qoff<T>(b, (int64_t)K * n) : nullptr;
  const double* tlop = (BOX && g.tlo) ? g.tlo + qoff<T>(b, (int64_t)K * n) : nullptr;
  double* txp = g.tx ? g.tx + qoff<T>(b, (int64_t)K * n) : nullptr;
  double* tup = g.tu ? g.tu + qoff<T>(b, K * EU) : nullptr;
  double* tfp = g.tf ? g.tf + qoff<T>(b, K) : nullptr;

  for (int k0 = 0; k0 < K; k0 += KC) {
    const int kc = K - k0 < KC ? K - k0 : KC;
    // the group prepares h and k of each direction of the chunk
    for (int c = 0; c < kc; c++) {
      const int64_t kd = k0 + c;
      // tG_k into the staging tile, lane-consecutive addresses; tg0_k into its vector
      if (tGp) stage_tile<T, S>(Tm, tGp + kd * nn * T, n, sl);
      if (sl < n) g0v[sl] = tg0p ? tg0p[(kd * n + sl) * T] : 0.0;
      sg_sync();
      // lane i: sG[i] = sum_j tG[i][j] x[j]
      double sGi = 0.0;
      if (tGp && sl < n)
        sGi = seq_fma_up<8>(0.0, 0, n, [&](int j) { return Tm[sl * LD + j]; }, [&](int j) { return xs[j]; });
      if (sl < n) sgv[sl] = sGi;
      sg_sync();
      // lane t: tcol(t) into column t of the staging tile, k[t] = -(tcol(t)^T x + tb(t))
      if (sl < nq) {
        const int j = sl < p ? 0 : wi[sl];
        double s = 0.0;
        if (sl < p) {
          if (hasCE) s = column_in<LD>(s, tCEp + (kd * n * p + sl) * T, (int64_t)p * T, n, Tm + sl, xs);
          if (tce0p) s = s + tce0p[(kd * p + sl) * T];
        } else if constexpr (BOX) {
          if (j < n) {
            if (thip) s = s + thip[(kd * n + j) * T];
          } else {
            if (tlop) s = s + -tlop[(kd * n + (j - n)) * T];
          }
        } else {
          if (hasCI) s = column_in<LD>(s, tCIp + (kd * n * m + j) * T, (int64_t)m * T, n, Tm + sl, xs);
          if (tci0p) s = s + tci0p[(kd * m + j) * T];
        }
        KB[sl * KL + c] = -s;
      }
      sg_sync();
      // lane i: h[i]
      if (sl < n) {
        double h = 0.0;
        const auto tc = [&](int t) { return Tm[sl * LD + t]; };
        const auto lm = [&](int t) { return lamv[t]; };
        if (hasCE) h = seq_fma_up<8>(h, 0, p, tc, lm);
        if (hasCI) h = seq_fma_up<8>(h, p, nq, tc, lm);
        if (tGp) h = h - sGi;
        if (tg0p) h = h - g0v[sl];
        HB[sl * KL + c] = h;
      }
      // the last lane: tf, before dl takes over k's column
      if (tfp && sl == S - 1) {
        double kk = 0.0, qq = 0.0, ll = 0.0;
        for (int t = 0; t < nq; t++) kk = kk + lamv[t] * KB[t * KL + c];
        for (int i = 0; i < n; i++) qq = qq + xs[i] * sgv[i];
        if (tg0p)
          for (int i = 0; i < n; i++) ll = ll + g0v[i] * xs[i];
        tfp[kd * T] = ((0.5 * qq) + ll) + kk;
      }
      sg_sync();
    }
    // The chunk's solves.  A substitution is serial in its rows: lane c runs direction c's alone, in
    // column c of a block, kc directions side by side.  r and y are independent sums: the group's
    // lanes share the (row, direction) pairs, direction fastest.
    const auto Lrow = [&](int i) { return [=](int k) { return Lm[i * LD + k]; }; };
    const auto Lcol = [&](int i) { return [=](int k) { return Lm[k * LD + i]; }; };
    const auto Rrow = [&](int i) { return [=](int k) { return Sm[i * LD + k]; }; };
    const auto Rcol = [&](int i) { return [=](int k) { return Sm[k * LD + i]; }; };
    const auto hcol = [&](int c) { return [=](int k) { return HB[k * KL + c]; }; };
    const auto dcol = [&](int c) { return [=](int k) { return KB[k * KL + c]; }; };
    if (sl < kc)
      for (int i = 0; i < n; i++)  // w = fsub(L, h)
        HB[i * KL + sl] = seq_fms_up<8>(HB[i * KL + sl], 0, i, Lrow(i), hcol(sl)) / Lm[i * LD + i];
    sg_sync();
    for (int e = sl; e < nq * kc; e += S) {  // r = k - M^T w
      const int t = e / kc, c = e % kc;
      const double acc = seq_fma_up<8>(0.0, 0, n, [&](int i) { return Mm[i * LD + t]; }, hcol(c));
      KB[t * KL + c] = KB[t * KL + c] - acc;
    }
    sg_sync();
    if (sl < kc) {  // dl = bsub(R, fsub(R, r))
      for (int i = 0; i < nq; i++)
        KB[i * KL + sl] = seq_fms_up<8>(KB[i * KL + sl], 0, i, Rrow(i), dcol(sl)) / Sm[i * LD + i];
      for (int i = nq - 1; i >= 0; i--)
        KB[i * KL + sl] = seq_fms_up<8>(KB[i * KL + sl], i + 1, nq, Rcol(i), dcol(sl)) / Sm[i * LD + i];
    }
    sg_sync();
    for (int e = sl; e < n * kc; e += S) {  // y = w + M dl
      const int i = e / kc, c = e % kc;
      HB[i * KL + c] = seq_fma_up<8>(HB[i * KL + c], 0, nq, [&](int t) { return Mm[i * LD + t]; }, dcol(c));
    }
    sg_sync();
    if (sl < kc)
      for (int i = n - 1; i >= 0; i--)  // tx = bsub(L, y)
        HB[i * KL + sl] = seq_fms_up<8>(HB[i * KL + sl], i + 1, n, Lcol(i), hcol(sl)) / Lm[i * LD + i];
    sg_sync();
    // the chunk's tx, lane-consecutive addresses, and the working positions of tu
    if (txp) {
      double* o = txp + (int64_t)k0 * n * T;
      for (int e = sl; e < kc * n; e += S) o[(int64_t)e * T] = HB[(e % n) * KL + e / n];
    }
    if (tup && sl < nq) {
      double* o = tup + ((int64_t)k0 * EU + (sl < p ? sl : p + wi[sl])) * T;
      for (int c = 0; c < kc; c++) o[c * EU * T] = KB[sl * KL + c];
    }
    sg_sync();
  }
}

using Kernel = void (*)(JvpManyArgs);

template <int T, bool BOX>
static Kernel lane_kernel_of(int n) {
  switch (n) {
    case 1: return jvp_many_lane_kernel<T, 1, BOX>;
    case 2: return jvp_many_lane_kernel<T, 2, BOX>;
    case 3: return jvp_many_lane_kernel<T, 3, BOX>;
    case 4: return jvp_many_lane_kernel<T, 4, BOX>;
    case 5: return jvp_many_lane_kernel<T, 5, BOX>;
    case 6: return jvp_many_lane_kernel<T, 6, BOX>;
    case 7: return jvp_many_lane_kernel<T, 7, BOX>;
    default: return jvp_many_lane_kernel<T, 8, BOX>;
  }
}

template <int T, bool BOX>
static Kernel group_kernel_of(int n) {
  return n <= 16   ? jvp_many_group_kernel<T, 16, BOX>
         : n <= 32 ? jvp_many_group_kernel<T, 32, BOX>
                   : jvp_many_group_kernel<T, 64, BOX>;
}

// launch_dense (qp_dense.h) with this file's LDS footprint per group
static hipError_t launch(const JvpManyArgs* a, int tiled, hipStream_t stream) {
  const int n = a->a.n;
  if (n < 1 || n > 64 || a->ntan < 1) return hipErrorInvalidValue;
  const bool lane = n <= 8, box = a->a.box != 0;
  Kernel k;
  if (lane)
    k = tiled ? (box ? lane_kernel_of<64, true>(n) : lane_kernel_of<64, false>(n))
              : (box ? lane_kernel_of<1, true>(n) : lane_kernel_of<1, false>(n));
  else
    k = tiled ? (box ? group_kernel_of<64, true>(n) : group_kernel_of<64, false>(n))
              : (box ? group_kernel_of<1, true>(n) : group_kernel_of<1, false>(n));
  const int S = group_lanes(n);
  const int64_t per_wg = lane ? 64 : 64 / S;  // QPs per workgroup
  size_t lds = 0;
  if (!lane) {
    const int per = S == 16 ? group_doubles_many<16>() : S == 32 ? group_doubles_many<32>() : group_doubles_many<64>();
    lds = (size_t)per * (64 / S) * sizeof(double);
    if (lds > 65536) {  // S = 32 and 64: beyond the default limit, inside the CU's 160 KiB
      const hipError_t e = grant_lds(reinterpret_cast<const void*>(k), lds);
      if (e != hipSuccess) return e;
    }
  }
  JvpManyArgs c = *a;
  const int64_t per = (int64_t)1 << 30;  // workgroups per launch: the grid stays inside 32 bits
  for (int64_t w0 = 0; w0 * per_wg < a->a.batch; w0 += per) {
    c.a.qp0 = w0 * per_wg;
    const int64_t left = (a->a.batch - c.a.qp0 + per_wg - 1) / per_wg;
    hipLaunchKernelGGL(k, dim3((unsigned)(left < per ? left : per)), dim3(64), lds, stream, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace jvp_many
}  // namespace qpk

extern "C" const char* qpk_jvp_many_name(int n) {
  static const char* const names[] = {"jvp_many_lane_n1", "jvp_many_lane_n2",   "jvp_many_lane_n3",   "jvp_many_lane_n4",
                                      "jvp_many_lane_n5", "jvp_many_lane_n6",   "jvp_many_lane_n7",   "jvp_many_lane_n8",
                                      "jvp_many_group_s16", "jvp_many_group_s32", "jvp_many_group_s64"};
  return qpk::dense_kernel_name(names, n);
}

extern "C" hipError_t qpk_launch_jvp_many(const qpk::JvpManyArgs* a, int tiled, hipStream_t stream) {
  return qpk::jvp_many::launch(a, tiled, stream);
}
