// qp_vjp_ws.hip — qpgpu_vjp_ws / qpgpu_vjp_box_ws for 64 < n <= 256: the backward step of
// include/qpgpu.h (qpgpu_vjp) where L, M and S of one QP no longer fit on chip.
//
// One workgroup of 256 lanes per QP in flight.  The caller's workspace is cut into slots of
// vjp_ws_doubles(n) doubles; workgroup s owns slot s and walks the QPs s, s + slots, ...  A slot
// holds, all private to this file,
//   Lc  n x n      L = chol(G), column-major (L[i][k] at k * n + i): lanes that own rows read a
//                  column with consecutive addresses
//   Mw  n x (n+1)  row-major with leading dimension n + 1: the working columns, then gx, turned in
//                  place into M = L^-1 A and w = L^-1 gx (column q)
//   Sc  n x n      S = M^T M, then R = chol(S), column-major like Lc (q x q of it is used)
// and the short vectors (x, a, c, r, the working list) live in LDS.
//
// The definition fixes, per element, the operations and their order; the mapping keeps every sum
// serial in its own index and spreads the independent ones:
//   chol       lane i owns row i.  Left-looking in panels of kJB columns: the sums over the columns
//              before the panel run with the panel's pivot rows staged in LDS (one read of
//              L[i][k] serves kJB columns), then the panel's columns follow one by one, the pivot
//              row's panel entries and the pivot travelling through LDS: one barrier per column.
//   M          forward substitution in panels of kKB rows: the panel's kKB x kKB triangle is one
//              lane's serial walk per column; the rows below subtract the panel's kKB products in
//              ascending k, spread over (row, column).  Partial sums rest in Mw between panels:
//              a rounded double stored and loaded again is the same double.
//   S, r       4 x 4 register tiles of the lower triangle (r is row q), M streamed through LDS
//              kIB rows at a time, every entry its own sum over i ascending from +0.0.
//   fsub(R, r) lane i owns element i: once y[k] is final every i > k subtracts R[i][k] * y[k].
//   bsub       serial by definition (row i subtracts z[i+1] first).  Per row the lanes k > i form
//              the products L[k][i] * z[k] into LDS, then every lane runs the same chain of
//              subtractions, so z[i] needs no broadcast: one barrier per row.
// Every barrier sits in control flow uniform over the workgroup: the QP loop, the masked-QP skip
// and the q > n case depend on the QP alone.
//
// The full form (qpgpu_vjp_full) is this file built a second time, by
// qp_vjp_ws_full.hip with QPGPU_VJP_FULL = 1, on VjpFullArgs: g.gu joins r after ws_gram's sum, g.gf
// turns c into ct and a into ah in the outputs.  Each is a branch on the pointer, uniform over the
// launch, and a NULL pointer leaves this build's operations (no + 0.0 is added: it would turn a -0.0
// into +0.0).  Without the macro the translation unit is the text it was.
#include "qp_dense.h"  // box_entry
#include "qp_vjp.h"

#ifndef QPGPU_VJP_FULL
#define QPGPU_VJP_FULL 0
#endif

namespace qpk {

namespace {

#if QPGPU_VJP_FULL
using WsArgs = VjpFullArgs;
#define vjp_ws_kernel vjp_ws_full_kernel
#else
using WsArgs = VjpArgs;
#endif

constexpr int kWsLanes = 256;
constexpr int kJB = 8;     // columns of a factorisation panel
constexpr int kKB = 8;     // rows of a substitution panel
constexpr int kIB = 8;     // rows of M staged per step of S = M^T M
constexpr int kCP = 260;   // leading dimension of LDS rows that hold up to n + 1 = 257 columns
constexpr int kScratch = kWsLanes * kKB + kKB * kCP;  // doubles: the largest phase (Lt + yp)
static_assert(kScratch >= kWsLanes * kJB + kJB * (kJB + 1), "chol: pivot rows + pivot row panel");
static_assert(kScratch >= kIB * kCP, "S: rows of M");

struct VjpWsArgs {
  WsArgs g;
  double* ws;
  int64_t per;  // doubles per slot
};

// A = chol(A): init(i, j) is A[i][j] (i >= j), the factor goes to Lc (column-major, leading
// dimension ld), which may be where init reads from.  scratch: kWsLanes * kJB + kJB * (kJB + 1).
template <class Init>
__device__ __forceinline__ void ws_chol(Init init, double* Lc, int ld, int N, double* scratch, int tid) {
  double* const Lp = scratch;                     // Lp[k * kJB + c] = L[jb + c][k], k < jb
  double* const prow = scratch + kWsLanes * kJB;  // prow[c][c'] = L[jb + c][jb + c'], prow[c][kJB] the pivot
  const int i = tid;
  for (int jb = 0; jb < N; jb += kJB) {
    const int jn = N - jb < kJB ? N - jb : kJB;
    __syncthreads();  // the panel before is stored; nobody reads Lp or prow any more
    for (int e = tid; e < jb * kJB; e += kWsLanes) {
      const int k = e / kJB, c = e % kJB;
      Lp[e] = c < jn ? Lc[(int64_t)k * ld + jb + c] : 0.0;
    }
    __syncthreads();
    const bool act = i >= jb && i < N;
    double acc[kJB], val[kJB];
#pragma unroll
    for (int c = 0; c < kJB; c++) acc[c] = val[c] = 0.0;
    if (act) {
#pragma unroll
      for (int c = 0; c < kJB; c++)
        if (c < jn && jb + c <= i) acc[c] = init(i, jb + c);
      for (int k = 0; k < jb; k++) {
        const double lik = Lc[(int64_t)k * ld + i];
#pragma unroll
        for (int c = 0; c < kJB; c++) acc[c] = acc[c] - lik * Lp[k * kJB + c];
      }
    }
#pragma unroll
    for (int c = 0; c < kJB; c++) {
      if (c < jn) {  // (uniform)
        const int j = jb + c;
        double s = acc[c];
        if (i == j) {
#pragma unroll
          for (int cc = 0; cc < c; cc++) s = s - val[cc] * val[cc];
          const double d = sqrt(s);
          val[c] = d;
#pragma unroll
          for (int cc = 0; cc < c; cc++) prow[c * (kJB + 1) + cc] = val[cc];
          prow[c * (kJB + 1) + kJB] = d;
        }
        __syncthreads();
        if (act && i > j) {
#pragma unroll
          for (int cc = 0; cc < c; cc++) s = s - val[cc] * prow[c * (kJB + 1) + cc];
          val[c] = s / prow[c * (kJB + 1) + kJB];
        }
      }
    }
    if (act) {
#pragma unroll
      for (int c = 0; c < kJB; c++)
        if (c < jn && i >= jb + c) Lc[(int64_t)(jb + c) * ld + i] = val[c];
    }
  }
  __syncthreads();
}

// Mw[:, t] = fsub(L, Mw[:, t]) for the C columns t, in place.  scratch: kWsLanes * kKB + kKB * kCP.
__device__ __forceinline__ void ws_fsub_columns(const double* Lc, int n, double* Mw, int ldm, int C, double* scratch,
                                                int tid) {
  double* const Lt = scratch;                  // Lt[(i - kb) * kKB + kk] = L[i][kb + kk]
  double* const yp = scratch + kWsLanes * kKB;  // yp[kk * kCP + t] = y[kb + kk] of column t
  // the rows below a panel: cg lanes side by side on the columns, 256 / cg rows at a time
  int cg = 32;
  while (cg < C && cg < kWsLanes) cg *= 2;
  const int tc = tid % cg, tr = tid / cg, R = kWsLanes / cg;
  for (int kb = 0; kb < n; kb += kKB) {
    const int kn = n - kb < kKB ? n - kb : kKB;
    __syncthreads();  // the rows below the panel before are stored; nobody reads Lt or yp any more
    for (int kk = 0; kk < kKB; kk++)
      for (int r = tid; r < n - kb; r += kWsLanes)
        Lt[r * kKB + kk] = (kk < kn && r >= kk) ? Lc[(int64_t)(kb + kk) * n + kb + r] : 0.0;
    __syncthreads();
    for (int t = tid; t < C; t += kWsLanes) {
      double y[kKB];
#pragma unroll
      for (int kk = 0; kk < kKB; kk++) {
        y[kk] = 0.0;
        if (kk < kn) {
          double s = Mw[(int64_t)(kb + kk) * ldm + t];
#pragma unroll
          for (int k2 = 0; k2 < kk; k2++) s = s - Lt[kk * kKB + k2] * y[k2];
          y[kk] = s / Lt[kk * kKB + kk];
          Mw[(int64_t)(kb + kk) * ldm + t] = y[kk];
          yp[kk * kCP + t] = y[kk];
        }
      }
    }
    __syncthreads();
    if (kn == kKB) {
      for (int t = tc; t < C; t += cg)
        for (int i = kb + kKB + tr; i < n; i += R) {
          double s = Mw[(int64_t)i * ldm + t];
#pragma unroll
          for (int kk = 0; kk < kKB; kk++) s = s - Lt[(i - kb) * kKB + kk] * yp[kk * kCP + t];
          Mw[(int64_t)i * ldm + t] = s;
        }
    }
  }
  __syncthreads();
}

// S[s][t] = sum_i M[i][s] * M[i][t] for q > s >= t into Sc (column-major, leading dimension ld), and
// rv[t] = sum_i M[i][t] * M[i][q]; every sum from +0.0 over i ascending.  scratch: kIB * kCP.
__device__ __forceinline__ void ws_gram(const double* Mw, int ldm, int n, int q, double* Sc, int ld, double* rv,
                                        double* scratch, int tid) {
  double* const Mt = scratch;  // Mt[ii * kCP + t] = M[i0 + ii][t], zero beyond column q
  const int C = q + 1, nb = (C + 3) / 4, nbl = nb * (nb + 1) / 2, CW = nb * 4;
  for (int blk0 = 0; blk0 < nbl; blk0 += kWsLanes) {
    const int blk = blk0 + tid;
    const bool valid = blk < nbl;
    // blk = bs (bs + 1) / 2 + bt, bt <= bs
    int bs = (int)((sqrt(8.0 * (double)blk + 1.0) - 1.0) * 0.5);
    while (bs * (bs + 1) / 2 > blk) bs--;
    while ((bs + 1) * (bs + 2) / 2 <= blk) bs++;
    const int bt = blk - bs * (bs + 1) / 2;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int c = 0; c < 4; c++) acc[a][c] = 0.0;
    for (int i0 = 0; i0 < n; i0 += kIB) {
      const int in = n - i0 < kIB ? n - i0 : kIB;
      __syncthreads();
      for (int ii = 0; ii < in; ii++)
        for (int t = tid; t < CW; t += kWsLanes) Mt[ii * kCP + t] = t < C ? Mw[(int64_t)(i0 + ii) * ldm + t] : 0.0;
      __syncthreads();
      if (valid) {
        for (int ii = 0; ii < in; ii++) {
          double ms[4], mt[4];
#pragma unroll
          for (int a = 0; a < 4; a++) {
            ms[a] = Mt[ii * kCP + 4 * bs + a];
            mt[a] = Mt[ii * kCP + 4 * bt + a];
          }
#pragma unroll
          for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[a][c] = acc[a][c] + ms[a] * mt[c];
        }
      }
    }
    if (valid) {
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int s = 4 * bs + a, t = 4 * bt + c;
          if (t < q && s >= t) {
            if (s < q)
              Sc[(int64_t)t * ld + s] = acc[a][c];
            else if (s == q)
              rv[t] = acc[a][c];
          }
        }
    }
  }
  __syncthreads();
}

// lane i's element of fsub(A, rhs) (rhs: lane i's element), A column-major with leading dimension
// ld.  zb: two doubles of LDS.
__device__ __forceinline__ double ws_fsub_vector(const double* Ac, int ld, int N, double rhs, double* zb, int tid) {
  const int i = tid;
  const double dii = i < N ? Ac[(int64_t)i * ld + i] : 1.0;
  double s = rhs, out = 0.0;
  double next = (i > 0 && i < N) ? Ac[i] : 0.0;  // L[i][0]; column k + 1 is fetched while step k runs
  for (int k = 0; k < N; k++) {
    if (i == k) {
      out = s / dii;
      zb[k & 1] = out;
    }
    __syncthreads();  // (zb[k & 1] is written again at k + 2, behind the barrier of k + 1)
    const double lik = next;
    if (i > k + 1 && i < N) next = Ac[(int64_t)(k + 1) * ld + i];
    if (i > k && i < N) s = s - lik * zb[k & 1];
  }
  __syncthreads();
  return out;
}

// z = bsub(A, rhs) (A^T z = rhs; rhs: lane i's element) into zout[0, N); lane i's element is
// returned.  dg: N doubles of LDS for the diagonal; pb: two buffers of kWsLanes doubles.
__device__ __forceinline__ double ws_bsub_vector(const double* Ac, int ld, int N, double rhs, double* zout, double* dg,
                                                 double* pb, int tid) {
  if (tid < N) dg[tid] = Ac[(int64_t)tid * ld + tid];
  __syncthreads();
  double z = 0.0;  // lane tid's element, once its row is done
  double lki = 0.0;  // L[tid][i], fetched while row i + 1 runs
  for (int i = N - 1; i >= 0; i--) {
    double* const P = pb + (i & 1) * kWsLanes;
    if (tid > i && tid < N) P[tid] = lki * z;
    if (tid == i) P[i] = rhs;
    __syncthreads();  // (P is written again at row i - 2, behind the barrier of row i - 1)
    if (i > 0 && tid >= i && tid < N) lki = Ac[(int64_t)(i - 1) * ld + tid];
    double s = P[i];
    for (int k = i + 1; k < N; k++) s = s - P[k];
    const double zi = s / dg[i];
    if (tid == i) {
      z = zi;
      zout[i] = zi;
    }
  }
  __syncthreads();
  return z;
}

// fv into every requested output element of QP b
template <int T>
__device__ __forceinline__ void ws_fill(const VjpArgs& g, int64_t b, double fv, int tid) {
  const auto fill = [&](double* out, int64_t E) {
    if (!out) return;
    double* o = out + qbase<T>(b, (int)E);
    for (int64_t e = tid; e < E; e += kWsLanes) o[e * T] = fv;
  };
  fill(g.dG, (int64_t)g.n * g.n);
  fill(g.dg0, g.n);
  fill(g.dCE, (int64_t)g.n * g.p);
  fill(g.dce0, g.p);
  fill(g.dCI, (int64_t)g.n * g.m);
  fill(g.dci0, g.m);
  fill(g.dhi, g.n);
  fill(g.dlo, g.n);
}

template <int T, bool BOX>
__global__ void __launch_bounds__(kWsLanes) vjp_ws_kernel(VjpWsArgs w) {
  __shared__ double scratch[kScratch];
  __shared__ double xs[kWsLanes], av[kWsLanes], cv[kWsLanes], rv[kWsLanes], dg[kWsLanes], pb[2 * kWsLanes], zb[2];
  __shared__ int wi[kWsLanes];
  __shared__ int cnt[2][kWsLanes / 64];
  const WsArgs& g = w.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = g.n, p = g.p, m = g.m, ldm = n + 1;
  double* const Lc = w.ws + (int64_t)blockIdx.x * w.per;
  double* const Mw = Lc + (int64_t)n * n;
  double* const Sc = Mw + (int64_t)n * ldm;

  for (int64_t b = blockIdx.x; b < g.batch; b += gridDim.x) {
    __syncthreads();  // the QP before is stored: LDS is free
    if (g.status && g.status[b] != QPGPU_QP_OK) {
      ws_fill<T>(g, b, 0.0, tid);
      continue;
    }
    const double* up = (p + m > 0) ? g.u + qbase<T>(b, p + m) : g.x;  // (never read with p + m == 0)
    const double* uip = up + (int64_t)p * T;

    // the working list: positions [0, p) the equalities, then the inequalities with u != 0
    int q = p, par = 0;
    for (int i0 = 0; i0 < m; i0 += kWsLanes, par ^= 1) {
      const int i = i0 + tid;
      const bool on = i < m && uip[(int64_t)i * T] != 0.0;
      const uint64_t mk = __ballot(on);
      if (lane == 0) cnt[par][wave] = __popcll(mk);
      __syncthreads();  // (cnt[par] is written again two chunks on, behind the next barrier)
      int before = 0, all = 0;
      for (int v = 0; v < kWsLanes / 64; v++) {
        const int cv_ = cnt[par][v];
        before += v < wave ? cv_ : 0;
        all += cv_;
      }
      const int pos = q + before + __popcll(mk & ((1ull << lane) - 1));
      if (on && pos < n) wi[pos] = i;
      q += all;
      if (q > n) q = n + 1;  // (more than n already: the count itself no longer matters)
    }
    if (q > n) {
      ws_fill<T>(g, b, __builtin_nan(""), tid);
      continue;
    }
    __syncthreads();  // wi is complete
    const int C = q + 1;

    // the working columns and gx into Mw; x into LDS
    const int64_t qG = qbase<T>(b, n * n), qCE = qbase<T>(b, n * p), qCI = BOX ? 0 : qbase<T>(b, n * m);
    const double* vp = g.gx + qbase<T>(b, n);
    if (tid < n) xs[tid] = g.x[qbase<T>(b, n) + (int64_t)tid * T];
    for (int e = tid; e < n * C; e += kWsLanes) {
      const int i = e / C, t = e - i * C;
      double s;
      if (t == q)
        s = vp[(int64_t)i * T];
      else if (t < p)
        s = g.CE[qCE + ((int64_t)i * p + t) * T];
      else if constexpr (BOX)
        s = box_entry(i, wi[t], n);
      else
        s = g.CI[qCI + ((int64_t)i * m + wi[t]) * T];
      Mw[(int64_t)i * ldm + t] = s;
    }

    const double* Gp = g.G + qG;
    ws_chol([&](int i, int j) { return Gp[((int64_t)i * n + j) * T]; }, Lc, n, n, scratch, tid);
    ws_fsub_columns(Lc, n, Mw, ldm, C, scratch, tid);
    ws_gram(Mw, ldm, n, q, Sc, n, rv, scratch, tid);
    ws_chol([&](int i, int j) { return Sc[(int64_t)j * n + i]; }, Sc, n, q, scratch, tid);
#if QPGPU_VJP_FULL
    double rr = tid < q ? rv[tid] : 0.0;  // gl(t) is added once, after ws_gram's sum
    if (g.gu && tid < q) rr = rr + g.gu[qbase<T>(b, p + m) + (int64_t)(tid < p ? tid : p + wi[tid]) * T];
    const double f = ws_fsub_vector(Sc, n, q, rr, zb, tid);
#else
    const double f = ws_fsub_vector(Sc, n, q, tid < q ? rv[tid] : 0.0, zb, tid);
#endif
    ws_bsub_vector(Sc, n, q, f, cv, dg, pb, tid);
    // lane i: y_i = w_i - sum_t M[i][t] c[t], then a = bsub(L, y)
    double y = 0.0;
    if (tid < n) {
      const double* Mi = Mw + (int64_t)tid * ldm;
      y = Mi[q];
      for (int t = 0; t < q; t++) y = y - Mi[t] * cv[t];
    }
    ws_bsub_vector(Lc, n, n, y, av, dg, pb, tid);

#if QPGPU_VJP_FULL
    const bool hasf = g.gf != nullptr;  // (uniform)
    double gfv = 0.0, hh = 0.0;
    if (hasf) {
      gfv = g.gf[b];
      hh = 0.5 * gfv;
      // ct = c + gf * lam for the outputs (y is formed, and a barrier lies behind it)
      if (tid < q) cv[tid] = cv[tid] + gfv * (tid < p ? up[(int64_t)tid * T] : uip[(int64_t)wi[tid] * T]);
      __syncthreads();
    }
#endif
    if (g.dg0) {
      double* o = g.dg0 + qbase<T>(b, n);
#if QPGPU_VJP_FULL
      if (tid < n) o[(int64_t)tid * T] = hasf ? -(av[tid] - gfv * xs[tid]) : -av[tid];
#else
      if (tid < n) o[(int64_t)tid * T] = -av[tid];
#endif
    }
    if (g.dG) {
      double* o = g.dG + qG;
      for (int e = tid; e < n * n; e += kWsLanes) {
        const int i = e / n, j = e - i * n;
#if QPGPU_VJP_FULL
        const double ahi = hasf ? av[i] - hh * xs[i] : av[i], ahj = hasf ? av[j] - hh * xs[j] : av[j];
        o[(int64_t)e * T] = -0.5 * (ahi * xs[j] + xs[i] * ahj);
#else
        o[(int64_t)e * T] = -0.5 * (av[i] * xs[j] + xs[i] * av[j]);
#endif
      }
    }
    if (g.dCE) {
      double* o = g.dCE + qCE;
      for (int e = tid; e < n * p; e += kWsLanes) {
        const int i = e / p, k = e - i * p;
        o[(int64_t)e * T] = av[i] * up[(int64_t)k * T] - xs[i] * cv[k];
      }
    }
    if (g.dce0) {
      double* o = g.dce0 + qbase<T>(b, p);
      if (tid < p) o[(int64_t)tid * T] = -cv[tid];
    }
    // the position in W of inequality j, which is in W (wi[p, q) ascends)
    const auto position = [&](int j) {
      int lo = p, hi = q;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (wi[mid] < j)
          lo = mid + 1;
        else
          hi = mid;
      }
      return lo;
    };
    if constexpr (BOX) {
      if (tid < n) {
        if (g.dhi) {
          const bool on = uip[(int64_t)tid * T] != 0.0;
          g.dhi[qbase<T>(b, n) + (int64_t)tid * T] = on ? -cv[position(tid)] : 0.0;
        }
        if (g.dlo) {
          const bool on = uip[(int64_t)(n + tid) * T] != 0.0;
          g.dlo[qbase<T>(b, n) + (int64_t)tid * T] = on ? cv[position(n + tid)] : 0.0;
        }
      }
    } else {
      if (g.dCI) {
        double* o = g.dCI + qCI;
        for (int64_t e = tid; e < (int64_t)n * m; e += kWsLanes) {
          const int i = (int)(e / m), j = (int)(e - (int64_t)i * m);
          const double uj = uip[(int64_t)j * T];
          o[e * T] = uj != 0.0 ? av[i] * uj - xs[i] * cv[position(j)] : 0.0;
        }
      }
      if (g.dci0) {
        double* o = g.dci0 + qbase<T>(b, m);
        for (int j = tid; j < m; j += kWsLanes) o[(int64_t)j * T] = uip[(int64_t)j * T] != 0.0 ? -cv[position(j)] : 0.0;
      }
    }
  }
}

}  // namespace

}  // namespace qpk

#if QPGPU_VJP_FULL
#undef vjp_ws_kernel

extern "C" const char* qpk_vjp_ws_full_name(int n) { return (n > 64 && n <= 256) ? "vjp_full_ws_g256" : nullptr; }

extern "C" hipError_t qpk_launch_vjp_ws_full(const qpk::VjpFullArgs* a, int tiled, void* ws, int64_t slots,
                                             hipStream_t stream) {
  using namespace qpk;
  if (!qpk_vjp_ws_name(a->n) || !ws || slots < 1) return hipErrorInvalidValue;
  if (slots > a->batch) slots = a->batch;
  if (slots > ((int64_t)1 << 30)) slots = (int64_t)1 << 30;  // the grid stays inside 32 bits
  VjpWsArgs w = {*a, static_cast<double*>(ws), qpk_vjp_ws_doubles(a->n)};
  w.g.qp0 = 0;
  const bool box = a->box != 0;
  void (*k)(VjpWsArgs) = tiled ? (box ? vjp_ws_full_kernel<64, true> : vjp_ws_full_kernel<64, false>)
                               : (box ? vjp_ws_full_kernel<1, true> : vjp_ws_full_kernel<1, false>);
  hipLaunchKernelGGL(k, dim3((unsigned)slots), dim3(kWsLanes), 0, stream, w);
  return hipGetLastError();
}
#else
extern "C" const char* qpk_vjp_ws_name(int n) { return (n > 64 && n <= 256) ? "vjp_ws_g256" : nullptr; }

extern "C" int64_t qpk_vjp_ws_doubles(int n) { return (n > 64 && n <= 256) ? 3 * (int64_t)n * n + n : 0; }

extern "C" hipError_t qpk_launch_vjp_ws(const qpk::VjpArgs* a, int tiled, void* ws, int64_t slots, hipStream_t stream) {
  using namespace qpk;
  if (!qpk_vjp_ws_name(a->n) || !ws || slots < 1) return hipErrorInvalidValue;
  if (slots > a->batch) slots = a->batch;
  if (slots > ((int64_t)1 << 30)) slots = (int64_t)1 << 30;  // the grid stays inside 32 bits
  VjpWsArgs w = {*a, static_cast<double*>(ws), qpk_vjp_ws_doubles(a->n)};
  w.g.qp0 = 0;
  const bool box = a->box != 0;
  void (*k)(VjpWsArgs) = tiled ? (box ? vjp_ws_kernel<64, true> : vjp_ws_kernel<64, false>)
                               : (box ? vjp_ws_kernel<1, true> : vjp_ws_kernel<1, false>);
  hipLaunchKernelGGL(k, dim3((unsigned)slots), dim3(kWsLanes), 0, stream, w);
  return hipGetLastError();
}
#endif
